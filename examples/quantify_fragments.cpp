// examples/quantify_fragments.cpp -- a C++14 driver over include/sbgpu_host.hpp, the way
// Strawberry's own Sample::procSample would use libsbgpu.so: read an annotation
// and read pairs, quantify every locus in one batch on the GPU, write the reference's two output
// files (GTF and the -f context table).  Used by tests/test_cpp_driver.py, which checks the files
// byte for byte against what the reference binary wrote for the same input.
//
//   g++ -std=c++14 -O2 -Iinclude examples/quantify_fragments.cpp -Lstrawberry_amd/lib -lsbgpu
//       -Wl,-rpath,$PWD/strawberry_amd/lib -o quantify_fragments
//   ./quantify_fragments input.txt out.gtf ctx.tsv [genome.fa] [--rank R --world W --comm-id FILE [--comm-nonce N]]
//         (genome.fa: the reference's `-b` option -- six sequence columns per bin in the -f table,
//          src/alignments.cpp:1622-1636)
//   Several GPUs: one process per GPU, rank R of W on GPU R; locus l belongs to rank l mod W.  Every rank reads
//   the whole input, keeps its loci and their pairs, and writes out.gtf / ctx.tsv with the suffix ".rank<R>";
//   the two sums over all loci -- mapped reads before the EM, FPKM after it (src/alignments.cpp:1372, :1821-1824)
//   -- are all-reduced over RCCL (sbgpu::Comm; rank 0 leaves the RCCL id in FILE for the others).
//
// Input (plain text, whitespace separated):
//   sample <name>  chrom <name>  strand <+|->  insert <mean> <sd>  read_len <n>  min_isoform_frac <x>  long_read <0|1>
//         (insert 0 0: no -i, empirical distribution; long_read: the reference's long-read workflow,
//          Strawberry.cpp:292-303, decided by the caller from the read lengths)
//   loci <L>
//     locus <gene_id> <n_isoforms> <+|-> <chrom>                (the gene's strand and chromosome)
//       iso <transcript_id> <n_exons> <left> <right> ...          (the reference's isoform order)
//   pairs <P>
//     pair <locus> <mass> <n_left_blocks> <l> <r> ... <n_right_blocks> <l> <r> ...
//         (every sequenced read pair, in any order: aligned blocks of each mate; mass = the pair's raw
//          mass, 1 / NH -- duplicates are collapsed by the library like the reference does)
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "sbgpu_host.hpp"

namespace {

struct Pair {
   int locus;
   double mass;
   std::vector<std::pair<uint32_t, uint32_t>> left, right;
};

// readhit_2_genomicFeats for an M/N CIGAR (src/contig.cpp:12-53): blocks with the introns between them
void mate_features(const std::vector<std::pair<uint32_t, uint32_t>> &blocks, std::vector<uint8_t> &c, std::vector<uint32_t> &l,
                   std::vector<uint32_t> &r)
{
   for (size_t k = 0; k < blocks.size(); ++k) {
      if (k) {
         c.push_back(1);
         l.push_back(blocks[k - 1].second + 1);
         r.push_back(blocks[k].first - 1);
      }
      c.push_back(0);
      l.push_back(blocks[k].first);
      r.push_back(blocks[k].second);
   }
}

} // namespace

int main(int argc, char **argv)
{
   int rank = 0, world = 1;
   std::string comm_id_file;
   unsigned long long comm_nonce = 0; // the same value on every rank of ONE launch: an older launch's id file is not ours
   {
      // trailing options; what is left are the positional arguments
      int n = argc;
      for (int i = 1; i + 1 < n;) {
         const std::string a = argv[i];
         if (a == "--rank" || a == "--world" || a == "--comm-id" || a == "--comm-nonce") {
            if (a == "--rank") rank = std::atoi(argv[i + 1]);
            else if (a == "--world") world = std::atoi(argv[i + 1]);
            else if (a == "--comm-nonce") comm_nonce = std::strtoull(argv[i + 1], nullptr, 10);
            else comm_id_file = argv[i + 1];
            for (int k = i; k + 2 < n; ++k) argv[k] = argv[k + 2];
            n -= 2;
         } else {
            ++i;
         }
      }
      argc = n;
   }
   if ((argc != 4 && argc != 5) || world < 1 || rank < 0 || rank >= world) {
      std::fprintf(stderr, "usage: %s input.txt out.gtf ctx.tsv [genome.fa] [--rank R --world W --comm-id FILE [--comm-nonce N]]\n", argv[0]);
      return 2;
   }
   const std::string part = world > 1 ? ".rank" + std::to_string(rank) : std::string();
   std::ifstream in(argv[1]);
   std::string tok, sample, chrom, strand;
   double ins_mean = 0, ins_sd = 0, min_frac = 0;
   int read_len = 0;
   int long_read = 0;
   in >> tok >> sample >> tok >> chrom >> tok >> strand >> tok >> ins_mean >> ins_sd >> tok >> read_len >> tok >> min_frac >> tok >>
      long_read;
   int64_t L = 0, P = 0;
   in >> tok >> L;
   sbgpu::LocusBatch batch;
   batch.keep_handle = true; // (the -f table below reads the handle: sbgpu::ContextTable::host)
   std::vector<std::string> gene_id, gene_strand, gene_chrom;
   std::vector<std::vector<std::string>> tx_id;
   std::vector<std::vector<std::vector<std::pair<uint32_t, uint32_t>>>> tx_exons;
   for (int64_t l = 0; l < L; ++l) {
      std::string g, gs, gc;
      int niso;
      in >> tok >> g >> niso >> gs >> gc;
      gene_id.push_back(g);
      gene_strand.push_back(gs);
      gene_chrom.push_back(gc);
      tx_id.emplace_back();
      tx_exons.emplace_back();
      for (int j = 0; j < niso; ++j) {
         std::string t;
         int ne;
         in >> tok >> t >> ne;
         std::vector<std::pair<uint32_t, uint32_t>> ex((size_t)ne);
         for (auto &e : ex) in >> e.first >> e.second;
         tx_id.back().push_back(t);
         tx_exons.back().push_back(ex);
      }
      batch.add_locus(tx_exons.back());
   }
   in >> tok >> P;
   std::vector<Pair> pairs((size_t)P);
   for (auto &p : pairs) {
      int nl, nr;
      in >> tok >> p.locus >> p.mass >> nl;
      p.left.resize((size_t)nl);
      for (auto &b : p.left) in >> b.first >> b.second;
      in >> nr;
      p.right.resize((size_t)nr);
      for (auto &b : p.right) in >> b.first >> b.second;
   }
   if (!in) {
      std::fprintf(stderr, "malformed input\n");
      return 2;
   }
   // every sequenced copy goes in as it is; the library does HitCluster::collapseAndFilterHits
   // (sort by the pair's ends, span filter, collapse of equal pairs) and Contig(PairedHit)
   std::vector<int32_t> p_locus;
   std::vector<double> p_mass;
   std::vector<int64_t> lo{0}, ro{0};
   std::vector<uint8_t> lc, rc;
   std::vector<uint32_t> ll, lr, rl, rr;
   for (const Pair &p : pairs) {
      if (p.locus % world != rank) continue; // another rank's locus
      p_locus.push_back(p.locus);
      p_mass.push_back(p.mass);
      mate_features(p.left, lc, ll, lr);
      mate_features(p.right, rc, rl, rr);
      lo.push_back((int64_t)lc.size());
      ro.push_back((int64_t)rc.size());
   }
   const sbgpu_pairs_t raw = {(int64_t)p_locus.size(), p_locus.data(), p_mass.data(), lo.data(), lc.data(), ll.data(), lr.data(),
                              ro.data(), rc.data(), rl.data(), rr.data()};
   int total_mapped = 0;
   try {
      total_mapped = batch.set_hits_from_pairs(raw);
   } catch (const std::exception &e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }

   try {
      sbgpu::Context ctx(rank % std::max(1, sbgpu_device_count()));
      sbgpu::Comm comm(ctx, rank, world, comm_id_file, comm_nonce);
      // Sample::_total_mapped_reads counts the whole sample (src/alignments.cpp:1372): sum over the ranks
      total_mapped = (int)comm.allreduce_sum((int64_t)total_mapped);
      sbgpu::InsertSize ins(ins_mean, ins_sd); // `insert 0 0`: no -i, build the empirical distribution
      sbgpu_abundance_params_t par = {};
      par.total_mapped_reads = total_mapped;
      par.filter_by_expression = 1;
      par.min_isoform_frac = min_frac;
      batch.quantify(ctx, (ins_mean != 0 && ins_sd != 0) ? &ins : nullptr, read_len, par, long_read != 0); // Strawberry.cpp:339-356
      // loci of other ranks hold no hits here: they are not this rank's to report
      for (int64_t l = 0; l < L; ++l)
         if (l % world != rank)
            for (int64_t j = batch.iso_off[(size_t)l]; j < batch.iso_off[(size_t)l + 1]; ++j) batch.isoforms[(size_t)j].kept = false;
      // the FPKM total runs over every isoform of the sample (src/alignments.cpp:1821-1824): sum over the ranks
      sbgpu::finalize_tpm(batch.isoforms, comm.allreduce_sum(sbgpu::sum_fpkm(batch.isoforms)));
   } catch (const std::exception &e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }

   // ---- GTF: Contig::print2gtf for every kept isoform, locus by locus (src/alignments.cpp:1831-1834)
   std::ofstream gtf(std::string(argv[2]) + part);
   std::vector<char> buf(1 << 20);
   for (int64_t l = 0; l < L; ++l) {
      for (size_t j = 0; j < tx_id[(size_t)l].size(); ++j) {
         const sbgpu::Isoform &t = batch.isoforms[(size_t)batch.iso_off[(size_t)l] + j];
         if (!t.kept) continue;
         std::vector<int32_t> el, er;
         for (const auto &e : tx_exons[(size_t)l][j]) {
            el.push_back((int32_t)e.first);
            er.push_back((int32_t)e.second);
         }
         const int n = sbgpu_format_gtf_transcript(buf.data(), (int)buf.size(), gene_chrom[(size_t)l].c_str(), gene_strand[(size_t)l][0], gene_id[(size_t)l].c_str(),
                                                   tx_id[(size_t)l][j].c_str(), gene_id[(size_t)l].c_str(), gene_id[(size_t)l].c_str(),
                                                   (int)el.size(), el.data(), er.data(), t.FPKM, t.frac, t.TPM,
                                                   t.FPKM_s == "NA" ? 2 : 1);
         sbgpu::check(n, "sbgpu_format_gtf_transcript");
         gtf.write(buf.data(), n);
      }
   }
   // ---- the -f table: Sample::printContext (src/alignments.cpp:1549-1639)
   std::ofstream ctxf(std::string(argv[3]) + part);
   ctxf << "sample\tsample_frag_count\tgene_id\tgene_frag_count\ttranscripts\tFPKMs\tconditional_probabilities\t"
           "class_probabilities\tpath_symbol\tpath_count\tpath_gc_content\tpath_hexmer_entropy\tgc_stretch_0.8_20\t"
           "gc_stretch_0.9_20\tgc_stretch_0.8_40\tgc_stretch_0.9_40\n";
   // printContext runs after the expression filter, over the surviving isoforms only: which bins get a row, in which
   // order, with how many hits and which probabilities is the library's sbgpu_context_table_host (sbgpu::ContextTable)
   const int64_t n_bins = batch.row_off.back();
   sbgpu::ContextTable table;
   try {
      std::vector<int32_t> keep(batch.isoforms.size() + 1, 0);
      for (size_t j = 0; j < batch.isoforms.size(); ++j) keep[j] = batch.isoforms[j].kept ? 1 : 0;
      table = sbgpu::ContextTable::host(batch.bins_handle.get(), batch.compat.data(), batch.compat_words, nullptr, keep.data(), batch.status.data());
   } catch (const std::exception &e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
   // -b genome.fa: GC ratio, hexamer entropy and high-GC-stretch flags of every bin's sequence, one kernel launch
   sbgpu::BinSequenceStats seq_stats;
   if (argc == 5) {
      for (const std::string &gc : gene_chrom)
         if (gc != chrom) {
            std::fprintf(stderr, "genome.fa: this driver takes one chromosome per run (header `chrom %s`, a locus on %s)\n", chrom.c_str(), gc.c_str());
            return 2;
         }
      std::ifstream fa(argv[4], std::ios::binary);
      if (!fa) {
         std::fprintf(stderr, "cannot open %s\n", argv[4]);
         return 2;
      }
      // the library's reader (sbgpu::FastaGenome): the run's chromosome by name, out of a FASTA of any number of contigs
      const std::string fa_bytes((std::istreambuf_iterator<char>(fa)), std::istreambuf_iterator<char>());
      std::string genome;
      try {
         const sbgpu::FastaGenome fasta = sbgpu::FastaGenome::host((const uint8_t *)fa_bytes.data(), (int64_t)fa_bytes.size());
         const int64_t contig = fasta.find(chrom);
         if (contig < 0) {
            std::fprintf(stderr, "%s: no contig named %s among its %lld\n", argv[4], chrom.c_str(), (long long)fasta.n_contigs());
            return 2;
         }
         genome = fasta.sequence(contig);
      } catch (const std::exception &e) {
         std::fprintf(stderr, "error: %s\n", e.what());
         return 1;
      }
      try {
         sbgpu::Context ctx(rank % std::max(1, sbgpu_device_count()));
         seq_stats = sbgpu::bin_sequence_stats(ctx, batch, genome);
      } catch (const std::exception &e) {
         std::fprintf(stderr, "error: %s\n", e.what());
         return 1;
      }
   }
   for (int64_t l = 0; l < L; ++l) {
      const int64_t j0 = batch.iso_off[(size_t)l], niso = batch.iso_off[(size_t)l + 1] - j0;
      const int64_t s0 = batch.seg_off[(size_t)l], nseg = batch.seg_off[(size_t)l + 1] - s0;
      std::vector<int> kept;
      std::vector<const char *> names;
      std::vector<double> fpkm, frac;
      for (int64_t j = 0; j < niso; ++j) {
         if (!batch.isoforms[(size_t)(j0 + j)].kept) continue;
         kept.push_back((int)j);
         names.push_back(tx_id[(size_t)l][(size_t)j].c_str());
         fpkm.push_back(batch.isoforms[(size_t)(j0 + j)].FPKM);
         frac.push_back(batch.isoforms[(size_t)(j0 + j)].frac);
      }
      // the locus' rows, already in std::map order of the bins' coordinate sets (:1552-1563)
      for (int64_t r = table.locus_row_off[(size_t)l]; r < table.locus_row_off[(size_t)l + 1]; ++r) {
         const int64_t b = table.row_bin[(size_t)r];
         std::vector<uint32_t> sl, sr;
         for (int64_t s = 0; s < nseg; ++s)
            if ((batch.bin_key[(size_t)(b * batch.key_words + (s >> 5))] >> (s & 31)) & 1u) {
               sl.push_back(batch.seg_left[(size_t)(s0 + s)]);
               sr.push_back(batch.seg_right[(size_t)(s0 + s)]);
            }
         const std::string row = table.format_row(l, r, batch.iso_off.data(), batch.f_off.data(), sample.c_str(), total_mapped, gene_id[(size_t)l].c_str(),
                                                  kept, names, fpkm.data(), frac.data(), (int)sl.size(), sl.data(), sr.data(),
                                                  seq_stats.gc.empty() ? nullptr : &seq_stats);
         ctxf.write(row.data(), (std::streamsize)row.size());
      }
   }
   std::fprintf(stderr, "%lld loci, %lld hits, %lld bins, %d mapped reads\n", (long long)L, (long long)batch.n_hits(), (long long)n_bins,
                total_mapped);
   return 0;
}
