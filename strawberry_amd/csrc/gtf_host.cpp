// strawberry_amd/csrc/gtf_host.cpp -- sbgpu_gtf_read_host and what the handle answers (include/sbgpu.h, sbgpu_gtf_*): a GTF
// annotation's bytes -> the annotation's CSR arrays, the clusters and the names.  The line's rule is gtf_rules.h's (the parse
// kernel calls the same function); a transcript is found in a hash map whose keys are compared byte by byte; the step from the
// transcripts to the arrays (gtf_finish) is the device form's too.  No kernels here, and nothing of HIP: a plain C++ compiler
// takes this file with gtf_rules.h, gtf_schedule.h and gtf_host.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sbgpu.h"
#include "gtf_host.h"
#include "gtf_rules.h"
#include "gtf_schedule.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (api_internal.h; a stand-alone program over this file defines its own)

int gtf_check_opts(const std::string &who, const sbgpu_gtf_opts_t *o)
{
   if (!o) return SBGPU_OK;
   if (o->n_ref < 0 || (o->n_ref > 0 && !o->ref_name)) return api_fail(SBGPU_EINVAL, who + ": n_ref < 0, or names without a table");
   for (int64_t k = 0; k < o->n_ref; ++k)
      if (!o->ref_name[k]) return api_fail(SBGPU_EINVAL, who + ": a null name in ref_name");
   if (o->hash_bits < 0 || o->hash_bits > 64) return api_fail(SBGPU_EINVAL, who + ": hash_bits outside 0 .. 64");
   return SBGPU_OK;
}

static std::string lower_of(const uint8_t *p, int64_t n)
{
   std::string s((size_t)n, '\0');
   for (int64_t i = 0; i < n; ++i) s[(size_t)i] = (char)gtf_lower(p[i]);
   return s;
}

int gtf_finish(const std::string &who, std::vector<GtfRawTx> &raw, std::vector<uint8_t> &&line_status, const sbgpu_gtf_opts_t *opts, sbgpu_gtf *g)
{
   const int64_t n_ref = opts ? opts->n_ref : 0;
   // ---- chromosomes: a table's index (names compared lower-cased, gff.cpp:118, read.cpp:964,980), else by first appearance in
   // the file (alignments.cpp:846-849)
   std::sort(raw.begin(), raw.end(), [](const GtfRawTx &a, const GtfRawTx &b) { return a.first_line < b.first_line; });
   std::unordered_map<std::string, int32_t> chrom_id;
   g->chrom_off.assign(1, 0);
   for (int64_t k = 0; k < n_ref; ++k) {
      const char *name = opts->ref_name[k];
      const size_t len = std::strlen(name);
      chrom_id.emplace(lower_of((const uint8_t *)name, (int64_t)len), (int32_t)k); // (a name the table has twice: its first place)
      g->chrom.append(name, len);
      g->chrom_off.push_back((int64_t)g->chrom.size());
   }
   struct Kept {
      const GtfRawTx *t;
      int32_t chrom;
   };
   std::vector<Kept> kept;
   kept.reserve(raw.size());
   int64_t dropped = 0, merges = 0;
   for (const GtfRawTx &t : raw) {
      merges += t.merges;
      const std::string key = lower_of(t.chrom, t.l_chrom);
      auto it = chrom_id.find(key);
      if (it == chrom_id.end()) {
         if (n_ref > 0) {
            ++dropped;
            continue;
         }
         it = chrom_id.emplace(key, (int32_t)chrom_id.size()).first;
         g->chrom.append((const char *)t.chrom, (size_t)t.l_chrom);
         g->chrom_off.push_back((int64_t)g->chrom.size());
      }
      kept.push_back({&t, it->second});
   }
   // ---- the order: chromosome, then the exon coordinates l1 r1 l2 r2 .. (a proper prefix first: Contig::operator< over
   // GenomicFeature::operator<, contig.cpp:186-193,342-347), then the first line (the reference's std::sort leaves these open)
   std::sort(kept.begin(), kept.end(), [](const Kept &a, const Kept &b) {
      if (a.chrom != b.chrom) return a.chrom < b.chrom;
      const int64_t n = std::min(a.t->n_exons, b.t->n_exons);
      for (int64_t i = 0; i < n; ++i) {
         if (a.t->xl[i] != b.t->xl[i]) return a.t->xl[i] < b.t->xl[i];
         if (a.t->xr[i] != b.t->xr[i]) return a.t->xr[i] < b.t->xr[i];
      }
      if (a.t->n_exons != b.t->n_exons) return a.t->n_exons < b.t->n_exons;
      return a.t->first_line < b.t->first_line;
   });
   // ---- loci: the kept transcripts of one (chromosome, gene_id as written), by their first isoform's place
   std::unordered_map<std::string, int64_t> locus_of;
   std::vector<std::vector<int64_t>> loci;
   for (int64_t k = 0; k < (int64_t)kept.size(); ++k) {
      std::string key((const char *)&kept[(size_t)k].chrom, 4);
      key.append((const char *)kept[(size_t)k].t->gene, (size_t)kept[(size_t)k].t->l_gene);
      const auto it = locus_of.emplace(key, (int64_t)loci.size());
      if (it.second) loci.emplace_back();
      loci[(size_t)it.first->second].push_back(k);
   }
   const int64_t nl = (int64_t)loci.size();
   g->iso_off.assign(1, 0), g->exon_off.assign(1, 0);
   g->gene_id_off.assign(1, 0), g->gene_name_off.assign(1, 0), g->tx_id_off.assign(1, 0);
   for (const std::vector<int64_t> &members : loci) {
      const Kept &head = kept[(size_t)members[0]];
      uint32_t left = 0xffffffffu, right = 0;
      for (const int64_t k : members) {
         const GtfRawTx &t = *kept[(size_t)k].t;
         int64_t len = 0;
         for (int64_t e = 0; e < t.n_exons; ++e) {
            g->exon_left.push_back(t.xl[e]), g->exon_right.push_back(t.xr[e]);
            len += (int64_t)t.xr[e] - (int64_t)t.xl[e] + 1;
         }
         left = std::min(left, t.xl[0]), right = std::max(right, t.xr[t.n_exons - 1]);
         g->exon_off.push_back((int64_t)g->exon_left.size());
         g->iso_len.push_back((int32_t)std::min<int64_t>(len, 0x7fffffff)), g->iso_strand.push_back(t.strand);
         g->tx_id.append((const char *)t.tx, (size_t)t.l_tx), g->tx_id_off.push_back((int64_t)g->tx_id.size());
      }
      g->iso_off.push_back((int64_t)g->iso_len.size());
      g->c_ref.push_back(head.chrom), g->c_left.push_back(left), g->c_right.push_back(right), g->c_strand.push_back(head.t->strand);
      g->gene_id.append((const char *)head.t->gene, (size_t)head.t->l_gene), g->gene_id_off.push_back((int64_t)g->gene_id.size());
      g->gene_name.append((const char *)head.t->gname, (size_t)head.t->l_gname), g->gene_name_off.push_back((int64_t)g->gene_name.size());
   }
   // ---- the disjoint segments: sbgpu_segments_host as it stands
   g->seg_off.assign((size_t)nl + 1, 0);
   const int64_t n_seg = sbgpu_segments_host(nl, g->iso_off.data(), g->exon_off.data(), g->exon_left.data(), g->exon_right.data(), g->seg_off.data(), nullptr, nullptr, 0);
   if (n_seg < 0) return (int)n_seg;
   g->seg_left.assign((size_t)n_seg + 1, 0), g->seg_right.assign((size_t)n_seg + 1, 0);
   const int64_t n_seg2 = sbgpu_segments_host(nl, g->iso_off.data(), g->exon_off.data(), g->exon_left.data(), g->exon_right.data(), g->seg_off.data(),
                                              g->seg_left.data(), g->seg_right.data(), n_seg);
   if (n_seg2 != n_seg) return n_seg2 < 0 ? (int)n_seg2 : api_fail(SBGPU_EINVAL, who + ": the segments changed between two passes");
   // (every array keeps one element beyond its last: an empty annotation's pointers are still arrays)
   g->exon_left.push_back(0), g->exon_right.push_back(0), g->c_ref.push_back(0), g->c_left.push_back(0), g->c_right.push_back(0);
   g->c_strand.push_back(0), g->iso_len.push_back(0), g->iso_strand.push_back(0);
   g->line_status = std::move(line_status);
   for (int k = 0; k < 16; ++k) g->info[k] = 0;
   g->info[0] = (int64_t)g->line_status.size();
   for (const uint8_t s : g->line_status) ++g->info[1 + (s <= kGtfNoGene ? s : kGtfNoGene)];
   g->line_status.push_back(0);
   g->info[8] = (int64_t)kept.size(), g->info[9] = nl, g->info[10] = g->exon_off.back(), g->info[11] = n_seg;
   g->info[12] = (int64_t)g->chrom_off.size() - 1, g->info[13] = merges, g->info[14] = dropped;
   g->annot.n_loci = nl, g->annot.iso_off = g->iso_off.data(), g->annot.exon_off = g->exon_off.data();
   g->annot.exon_left = g->exon_left.data(), g->annot.exon_right = g->exon_right.data();
   g->annot.seg_off = g->seg_off.data(), g->annot.seg_left = g->seg_left.data(), g->annot.seg_right = g->seg_right.data();
   g->clusters.n_clusters = nl, g->clusters.ref = g->c_ref.data(), g->clusters.left = g->c_left.data(), g->clusters.right = g->c_right.data();
   g->clusters.strand = g->c_strand.data();
   g->names.gene_id_off = g->gene_id_off.data(), g->names.gene_id = g->gene_id.c_str();
   g->names.gene_name_off = g->gene_name_off.data(), g->names.gene_name = g->gene_name.c_str();
   g->names.transcript_id_off = g->tx_id_off.data(), g->names.transcript_id = g->tx_id.c_str();
   g->names.chrom_off = g->chrom_off.data(), g->names.chrom = g->chrom.c_str();
   return SBGPU_OK;
}

} // namespace sb

using sb::api_fail;

namespace {
struct HostTx {
   int64_t first_line;
   const uint8_t *line; // the first line's bytes
   sb::GtfLine first;
   std::vector<uint32_t> xl, xr;
   int64_t merges = 0;
};
} // namespace

extern "C" {

int sbgpu_gtf_read_host(const uint8_t *bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, sbgpu_gtf_t **out)
{
   const std::string who = "sbgpu_gtf_read_host";
   if (!out || n_bytes < 0 || (n_bytes && !bytes)) return api_fail(SBGPU_EINVAL, who + ": bad argument");
   *out = nullptr;
   if (const int rc = sb::gtf_check_opts(who, opts)) return rc;
   try {
      std::vector<uint8_t> status;
      std::vector<HostTx> txs;
      std::unordered_map<std::string, size_t> tx_of; // (chromosome lower-cased, '\t', strand, transcript_id) -> txs
      sb::GtfBytes rd;
      std::string key;
      for (int64_t p = 0; p < n_bytes;) {
         const void *nl = std::memchr(bytes + p, '\n', (size_t)(n_bytes - p));
         const int64_t end = nl ? (const uint8_t *)nl - bytes : n_bytes;
         const uint8_t *line = bytes + p;
         const int64_t len = sb::gtf_line_len(line, end - p), r = (int64_t)status.size();
         sb::GtfLine x;
         sb::gtf_parse_line(rd, line, len, x);
         if (x.status == sb::kGtfNameLong)
            return api_fail(SBGPU_EUNSUPPORTED, who + ": a name of more than 255 bytes (line " + std::to_string(r + 1) + ")");
         status.push_back(x.status);
         if (x.status == sb::kGtfOk) {
            key.clear();
            for (int64_t i = 0; i < x.l_chrom; ++i) key.push_back((char)sb::gtf_lower(line[i]));
            key.push_back('\t'), key.push_back((char)x.strand);
            key.append((const char *)line + x.o_tx, (size_t)x.l_tx);
            const auto it = tx_of.emplace(key, txs.size());
            if (it.second) {
               txs.emplace_back();
               txs.back().first_line = r, txs.back().line = line, txs.back().first = x;
            }
            HostTx &t = txs[it.first->second];
            t.xl.push_back(x.left), t.xr.push_back(x.right);
         }
         p = end + 1;
      }
      // a transcript's exons: sorted by (left, right), then equal, overlapping and touching ones merged into their union
      std::vector<sb::GtfRawTx> raw;
      raw.reserve(txs.size());
      std::vector<std::pair<uint32_t, uint32_t>> ex;
      for (HostTx &t : txs) {
         ex.clear();
         for (size_t i = 0; i < t.xl.size(); ++i) ex.emplace_back(t.xl[i], t.xr[i]);
         std::sort(ex.begin(), ex.end());
         size_t n = 0;
         for (size_t i = 0; i < ex.size(); ++i) {
            if (n && sb::gtf_exons_join(t.xr[n - 1], ex[i].first)) {
               t.xr[n - 1] = std::max(t.xr[n - 1], ex[i].second);
               ++t.merges;
            } else {
               t.xl[n] = ex[i].first, t.xr[n] = ex[i].second, ++n;
            }
         }
         sb::GtfRawTx q;
         q.first_line = t.first_line;
         q.chrom = t.line, q.gene = t.line + t.first.o_gene, q.tx = t.line + t.first.o_tx, q.gname = t.line + t.first.o_gname;
         q.l_chrom = (int32_t)t.first.l_chrom, q.l_gene = (int32_t)t.first.l_gene, q.l_tx = (int32_t)t.first.l_tx, q.l_gname = (int32_t)t.first.l_gname;
         q.strand = t.first.strand;
         q.xl = t.xl.data(), q.xr = t.xr.data(), q.n_exons = (int64_t)n, q.merges = t.merges;
         raw.push_back(q);
      }
      std::unique_ptr<sbgpu_gtf> g(new sbgpu_gtf());
      if (const int rc = sb::gtf_finish(who, raw, std::move(status), opts, g.get())) return rc;
      *out = g.release();
   } catch (const std::bad_alloc &) {
      return api_fail(SBGPU_ENOMEM, who + ": out of memory");
   } catch (const std::exception &e) { // (std::length_error of a container: nothing C++ crosses the C ABI)
      return api_fail(SBGPU_ENOMEM, who + ": " + e.what());
   }
   return SBGPU_OK;
}

void sbgpu_gtf_destroy(sbgpu_gtf_t *g) { delete g; }

int sbgpu_gtf_annotation(const sbgpu_gtf_t *g, sbgpu_annotation_t *annot, sbgpu_clusters_t *clusters, const int32_t **iso_len, const uint8_t **iso_strand)
{
   if (!g) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_annotation: null handle");
   if (annot) *annot = g->annot;
   if (clusters) *clusters = g->clusters;
   if (iso_len) *iso_len = g->iso_len.data();
   if (iso_strand) *iso_strand = g->iso_strand.data();
   return SBGPU_OK;
}

int sbgpu_gtf_names(const sbgpu_gtf_t *g, sbgpu_gtf_names_t *names)
{
   if (!g || !names) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_names: null argument");
   *names = g->names;
   return SBGPU_OK;
}

int sbgpu_gtf_info(const sbgpu_gtf_t *g, int64_t info[16])
{
   if (!g || !info) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_info: null argument");
   for (int k = 0; k < 16; ++k) info[k] = g->info[k];
   return SBGPU_OK;
}

int sbgpu_gtf_line_status(const sbgpu_gtf_t *g, uint8_t *status)
{
   if (!g || (g->info[0] && !status)) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_line_status: null argument");
   if (g->info[0]) std::memcpy(status, g->line_status.data(), (size_t)g->info[0]);
   return SBGPU_OK;
}

int sbgpu_gtf_limits(int64_t limits[8])
{
   if (!limits) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_limits: null argument");
   limits[0] = sb::kGtfTileLines, limits[1] = sb::kGtfStageLimit, limits[2] = sb::kGtfMaxLine, limits[3] = sb::kGtfScanTile;
   limits[4] = sb::kGtfIndexTile, limits[5] = sb::kGtfGridCap, limits[6] = sb::kGtfMaxName, limits[7] = sb::kGtfMaxLines;
   return SBGPU_OK;
}

} // extern "C"
