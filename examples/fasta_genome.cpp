// examples/fasta_genome.cpp -- a genome FASTA's .fai index from C++14 over the library's reader (sbgpu::FastaGenome,
// include/sbgpu_host.hpp): what `samtools faidx genome.fa` writes beside the file, to stdout.
//
//   g++ -std=c++14 -Iinclude examples/fasta_genome.cpp -Lstrawberry_amd/lib -lsbgpu -Wl,-rpath,$PWD/strawberry_amd/lib
//   ./a.out genome.fa [--device] > genome.fa.fai
//
// Without --device the host form reads the file (no GPU); with it the bytes are packed on the device.  Counts go to stderr.  A
// contig whose lines are of unequal length, or one without a name, has no index line: the program says which and fails.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sbgpu_host.hpp"

int main(int argc, char **argv)
{
   if (argc < 2) {
      std::fprintf(stderr, "usage: %s genome.fa [--device]\n", argv[0]);
      return 2;
   }
   const bool on_device = argc > 2 && !std::strcmp(argv[2], "--device");
   std::FILE *f = std::fopen(argv[1], "rb");
   if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[1]);
      return 1;
   }
   std::vector<uint8_t> file, chunk(1 << 20);
   for (size_t n; (n = std::fread(chunk.data(), 1, chunk.size(), f)) > 0;) file.insert(file.end(), chunk.begin(), chunk.begin() + n);
   std::fclose(f);
   try {
      sbgpu::FastaGenome g = on_device ? sbgpu::FastaGenome::device(sbgpu::Context(0), file.data(), (int64_t)file.size())
                                       : sbgpu::FastaGenome::host(file.data(), (int64_t)file.size());
      std::fprintf(stderr, "%lld bytes, %lld lines, %lld contigs, %lld bases; %lld empty, %lld ragged, %lld duplicate names, %lld without a name\n", (long long)g.info(0),
                   (long long)g.info(1), (long long)g.info(2), (long long)g.info(3), (long long)g.info(4), (long long)g.info(5), (long long)g.info(6),
                   (long long)g.info(7));
      const std::string fai = g.fai_text();
      std::fwrite(fai.data(), 1, fai.size(), stdout);
   } catch (const std::exception &e) {
      std::fprintf(stderr, "%s: %s\n", argv[1], e.what());
      return 1;
   }
   return 0;
}
