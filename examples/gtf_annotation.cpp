// examples/gtf_annotation.cpp -- a GTF annotation's loci from C++14 over the library's reader (sbgpu::GtfAnnotation,
// include/sbgpu_host.hpp): the `loci` section of examples/quantify_fragments.cpp's input, in the reference's locus and
// isoform order.
//
//   g++ -std=c++14 -Iinclude examples/gtf_annotation.cpp -Lstrawberry_amd/lib -lsbgpu -Wl,-rpath,$PWD/strawberry_amd/lib
//   ./a.out genes.gtf [--device] [chromosome names of the BAM header ...] > loci.txt
//
//   loci <L>
//     locus <gene_id> <n_isoforms> <+|-|.> <chrom>
//       iso <transcript_id> <n_exons> <left> <right> ...
//
// Without --device the host form reads the file (no GPU); with it the bytes are parsed on the device.  Counts go to stderr.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sbgpu_host.hpp"

int main(int argc, char **argv)
{
   if (argc < 2) {
      std::fprintf(stderr, "usage: %s genes.gtf [--device] [reference names ...]\n", argv[0]);
      return 2;
   }
   bool on_device = false;
   std::vector<std::string> refs;
   for (int i = 2; i < argc; ++i) {
      if (!std::strcmp(argv[i], "--device")) on_device = true;
      else refs.push_back(argv[i]);
   }
   std::FILE *f = std::fopen(argv[1], "rb");
   if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[1]);
      return 1;
   }
   std::vector<uint8_t> file, chunk(1 << 20);
   for (size_t n; (n = std::fread(chunk.data(), 1, chunk.size(), f)) > 0;) file.insert(file.end(), chunk.begin(), chunk.begin() + n);
   std::fclose(f);
   try {
      sbgpu::GtfAnnotation g = on_device ? sbgpu::GtfAnnotation::device(sbgpu::Context(0), file.data(), (int64_t)file.size(), refs)
                                         : sbgpu::GtfAnnotation::host(file.data(), (int64_t)file.size(), refs);
      const sbgpu_annotation_t &a = g.annot();
      const sbgpu_clusters_t &c = g.clusters();
      std::printf("loci %lld\n", (long long)a.n_loci);
      for (int64_t l = 0; l < a.n_loci; ++l) {
         std::printf("locus %s %lld %c %s\n", g.gene_id(l).c_str(), (long long)(a.iso_off[l + 1] - a.iso_off[l]), ".+-"[c.strand[l] % 3], g.chrom(c.ref[l]).c_str());
         for (int64_t i = a.iso_off[l]; i < a.iso_off[l + 1]; ++i) {
            std::printf("iso %s %lld", g.transcript_id(i).c_str(), (long long)(a.exon_off[i + 1] - a.exon_off[i]));
            for (int64_t e = a.exon_off[i]; e < a.exon_off[i + 1]; ++e) std::printf(" %u %u", a.exon_left[e], a.exon_right[e]);
            std::printf("\n");
         }
      }
      std::fprintf(stderr, "%lld lines, %lld exon lines, %lld transcripts, %lld loci, %lld exons (%lld merged away), %lld segments, %lld transcripts on unknown chromosomes\n",
                   (long long)g.info(0), (long long)g.info(1), (long long)g.info(8), (long long)g.info(9), (long long)g.info(10), (long long)g.info(13),
                   (long long)g.info(11), (long long)g.info(14));
   } catch (const std::exception &e) {
      std::fprintf(stderr, "%s: %s\n", argv[1], e.what());
      return 1;
   }
   return 0;
}
