"""The FASTA reader's host form (csrc/fasta_host.cpp over fasta_rules.h) and the device form's host decisions
(csrc/fasta_schedule.h) from a stand-alone C++ program built with g++ under AddressSanitizer and UBSan: adversarial buffers
that end exactly where their allocation ends -- truncated headers, a '>' as the only byte, '\r' as the last byte, a megabyte of
'>' --, and every decision of fasta_schedule.h stated a second time at 0, 1, tile +- 1, 2^31 +- 1, 2^32 +- 1 and 2^35 bytes.
No GPU, no library; nothing with a sanitizer is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "fasta_host.h"
#include "fasta_rules.h"
#include "fasta_schedule.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static std::string last_error;
namespace sb {
int api_fail(int code, const std::string &msg) { last_error = msg; return code; }
}

// the bytes in an allocation of exactly their size: one byte read beyond them is the sanitizer's
struct Exact {
   std::unique_ptr<uint8_t[]> p;
   int64_t n;
   explicit Exact(const std::string &s) : p(new uint8_t[s.size() ? s.size() : 1]), n((int64_t)s.size()) { std::memcpy(p.get(), s.data(), s.size()); }
};
struct Read {
   int rc = 0;
   int64_t info[16] = {};
   std::vector<std::string> names, seqs;
   std::vector<int64_t> offset, lb, lw;
   std::vector<int> flags;
   std::string fai;
   int fai_rc = 0;
};
static Read read(const std::string &s)
{
   Exact b(s);
   Read r;
   sbgpu_fasta_t *g = nullptr;
   r.rc = sbgpu_fasta_read_host(s.empty() ? nullptr : b.p.get(), b.n, &g);
   if (r.rc != SBGPU_OK) return r;
   sbgpu_fasta_info(g, r.info);
   const int64_t *seq_off, *offset, *lb, *lw, *name_off;
   const uint8_t *flags;
   const char *names;
   sbgpu_fasta_index(g, &seq_off, &offset, &lb, &lw, &flags);
   sbgpu_fasta_names(g, &name_off, &names);
   for (int64_t c = 0; c < r.info[2]; ++c) {
      r.names.emplace_back(names + name_off[c], names + name_off[c + 1]);
      std::string q((size_t)(seq_off[c + 1] - seq_off[c]), '?');
      if (!q.empty() && sbgpu_fasta_fetch(g, c, 1, (int64_t)q.size(), (uint8_t *)&q[0]) != SBGPU_OK) q = "<fetch failed>";
      r.seqs.push_back(q);
      r.offset.push_back(offset[c]), r.lb.push_back(lb[c]), r.lw.push_back(lw[c]), r.flags.push_back(flags[c]);
   }
   int64_t need = 0;
   r.fai_rc = sbgpu_fasta_fai(g, nullptr, 0, &need);
   if (r.fai_rc == SBGPU_OK) {
      r.fai.assign((size_t)need, '\0');
      if (need) sbgpu_fasta_fai(g, &r.fai[0], need, &need);
   }
   sbgpu_fasta_destroy(g);
   return r;
}
static bool laid_out(const std::vector<size_t> &off, const std::vector<size_t> &bytes, size_t total)
{
   for (size_t i = 0; i < off.size(); ++i) {
      if (off[i] % 256) return false;
      if (off[i] + bytes[i] > (i + 1 < off.size() ? off[i + 1] : total)) return false;
   }
   return total % 256 == 0;
}

int main()
{
   using namespace sb;
   // ---- adversarial buffers
   {
      Read r = read("");
      CHECK(r.rc == 0 && r.info[2] == 0 && r.info[1] == 0 && r.fai.empty());
      r = read(">");
      CHECK(r.rc == 0 && r.info[2] == 1 && r.names[0].empty() && r.flags[0] == (SBGPU_FASTA_EMPTY | SBGPU_FASTA_NONAME) && r.offset[0] == 1 && r.fai.empty());
      r = read(">a");
      CHECK(r.rc == 0 && r.names[0] == "a" && r.offset[0] == 2 && r.flags[0] == SBGPU_FASTA_EMPTY);
      r = read(">a\r");
      CHECK(r.rc == 0 && r.names[0] == "a" && r.offset[0] == 3 && r.flags[0] == SBGPU_FASTA_EMPTY && r.info[1] == 1);
      r = read(">a b\r\n");
      CHECK(r.rc == 0 && r.names[0] == "a" && r.offset[0] == 6 && r.flags[0] == SBGPU_FASTA_EMPTY);
      r = read(">a\nACGT\r");
      CHECK(r.rc == 0 && r.seqs[0] == "ACGT\r" && r.lb[0] == 5 && r.lw[0] == 5 && r.flags[0] == 0 && r.fai == "a\t5\t3\t5\t5\n");
      r = read(">a\nACGT\r\n");
      CHECK(r.rc == 0 && r.seqs[0] == "ACGT" && r.lb[0] == 4 && r.lw[0] == 6 && r.fai == "a\t4\t3\t4\t6\n");
      r = read(">a\nAC\n>");
      CHECK(r.rc == 0 && r.info[2] == 2 && r.flags[1] == (SBGPU_FASTA_EMPTY | SBGPU_FASTA_NONAME) && r.fai == "a\t2\t3\t2\t3\n");
      r = read("\r");
      CHECK(r.rc == SBGPU_EINVAL && last_error.find("offset 0") != std::string::npos);
      r = read("\n\n\r\n");
      CHECK(r.rc == 0 && r.info[2] == 0 && r.info[1] == 3);
      r = read(std::string("\n\0>a\n", 5));
      CHECK(r.rc == SBGPU_EINVAL && last_error.find("offset 1") != std::string::npos);
      r = read(std::string(">a\0b\n\0\n", 7));
      CHECK(r.rc == 0 && r.names[0] == std::string("a\0b", 3) && r.seqs[0] == std::string("\0", 1));
      r = read(">a\nACGT\nACGTA\n");
      CHECK(r.rc == 0 && r.flags[0] == SBGPU_FASTA_RAGGED && r.fai_rc == SBGPU_EUNSUPPORTED && last_error.find("'a'") != std::string::npos);
      // a megabyte of '>': one header whose name is the rest
      std::string many((size_t)1 << 20, '>');
      r = read(many);
      CHECK(r.rc == 0 && r.info[2] == 1 && r.names[0].size() == many.size() - 1 && r.flags[0] == SBGPU_FASTA_EMPTY);
      // ... and a megabyte of ">\n": half a million nameless, empty contigs
      many.clear();
      for (int i = 0; i < (1 << 19); ++i) many += ">\n";
      r = read(many);
      CHECK(r.rc == 0 && r.info[2] == (1 << 19) && r.info[4] == (1 << 19) && r.info[6] == (1 << 19) - 1 && r.info[7] == (1 << 19) && r.fai.empty());
      // the lookup and a window from a handle
      Exact b(">Chr1 x\nACGT\nAC\n>chr1\nGG\n");
      sbgpu_fasta_t *g = nullptr;
      CHECK(sbgpu_fasta_read_host(b.p.get(), b.n, &g) == SBGPU_OK);
      int64_t c = -2;
      CHECK(sbgpu_fasta_find(g, "CHR1", 4, &c) == SBGPU_OK && c == 0 && sbgpu_fasta_find(g, "chr", 3, &c) == SBGPU_OK && c == -1);
      uint8_t w[2];
      CHECK(sbgpu_fasta_fetch(g, 0, 5, 2, w) == SBGPU_OK && w[0] == 'A' && w[1] == 'C' && sbgpu_fasta_fetch(g, 0, 6, 2, w) == SBGPU_EINVAL);
      CHECK(sbgpu_fasta_fetch(g, 2, 1, 1, w) == SBGPU_EINVAL && sbgpu_fasta_fetch(g, 1, 0, 1, w) == SBGPU_EINVAL);
      sbgpu_fasta_destroy(g);
   }
   // ---- the rule's shared pieces
   CHECK(fasta_isspace(' ') && fasta_isspace('\t') && fasta_isspace('\n') && fasta_isspace('\v') && fasta_isspace('\f') && fasta_isspace('\r'));
   CHECK(!fasta_isspace(0) && !fasta_isspace('a') && !fasta_isspace(0x85) && !fasta_isspace(0xa0) && !fasta_isspace(8) && !fasta_isspace(14));
   CHECK(fasta_lower('A') == 'a' && fasta_lower('Z') == 'z' && fasta_lower('@') == '@' && fasta_lower('[') == '[' && fasta_lower(0xc4) == 0xc4);
   CHECK(fasta_is_term('\n', -1) && fasta_is_term('\r', '\n') && !fasta_is_term('\r', -1) && !fasta_is_term('\r', '\r') && !fasta_is_term('A', '\n'));
   {
      int64_t b = -1, w = -1;
      fasta_first_line(10, 100, 70, false, &b, &w);
      CHECK(b == 60 && w == 61);
      fasta_first_line(10, 100, 71, true, &b, &w);
      CHECK(b == 60 && w == 62);
      fasta_first_line(10, 100, 100, false, &b, &w);
      CHECK(b == 90 && w == 90);
      fasta_first_line(10, 10, 0x7f7f7f7f7f7f7f7fll, false, &b, &w);
      CHECK(b == 0 && w == 0);
      fasta_first_line(10, 100, 10, false, &b, &w);
      CHECK(b == 0 && w == 1);
   }
   CHECK(!fasta_base_out_of_phase(59, 60) && fasta_base_out_of_phase(60, 60) && fasta_base_out_of_phase(0, 0));
   CHECK(!fasta_line_end_odd(60, 60, 61, false) && fasta_line_end_odd(60, 60, 61, true) && fasta_line_end_odd(59, 60, 61, false));
   CHECK(!fasta_line_end_odd(61, 60, 62, true) && fasta_line_end_odd(60, 60, 62, false) && fasta_line_end_odd(0, 60, 62, true));
   // ---- fasta_schedule.h, stated a second time
   int64_t lim[8];
   CHECK(sbgpu_fasta_limits(lim) == SBGPU_OK && lim[0] == 16384 && lim[1] == 1024 && lim[2] == 2048 && lim[3] == 65535 && lim[4] == (1 << 24));
   CHECK(kFastaTile == lim[0] && kFastaScanTile == lim[1] && kFastaGridCap == lim[2] && kFastaMaxHeader == lim[3] && kFastaMaxContigs == lim[4]);
   const int64_t T = 16384, two31 = (int64_t)1 << 31, two32 = (int64_t)1 << 32, two35 = (int64_t)1 << 35;
   for (int64_t n : {(int64_t)0, (int64_t)1, T - 1, T, T + 1, two31 - 1, two31, two31 + 1, two32 - 1, two32, two32 + 1, two35}) {
      const int64_t t = n / T + (n % T ? 1 : 0);
      CHECK(fasta_tiles(n) == t);
      CHECK(fasta_grid(t) == (unsigned)(t < 1 ? 1 : t > 2048 ? 2048 : t));
      CHECK(fasta_scan_rounds(t) == t / 1024 + (t % 1024 ? 1 : 0));
      const FastaTileLayout L = fasta_tile_layout(n);
      const size_t u = (size_t)t;
      CHECK(L.tiles == t && L.words_bytes == 64 && laid_out({L.hdr_cnt, L.hdr_at, L.base_cnt, L.base_at, L.words}, {u * 4, (u + 1) * 8, u * 4, (u + 1) * 8, 64}, L.bytes));
      CHECK(L.bytes <= 24 * u + 256 * 6);   // O(tiles)
   }
   CHECK(fasta_tiles(-5) == 0 && fasta_scan_rounds(0) == 0 && fasta_scan_rounds(1024) == 1 && fasta_scan_rounds(1025) == 2);
   CHECK(fasta_grid_contigs(0) == 1 && fasta_grid_contigs(4) == 1 && fasta_grid_contigs(5) == 2 && fasta_grid_contigs(1 << 24) == 2048);
   CHECK(fasta_grid256(1) == 1 && fasta_grid256(256) == 1 && fasta_grid256(257) == 2 && fasta_grid256((int64_t)1 << 40) == 2048);
   CHECK(fasta_header_fits(65535) && !fasta_header_fits(65536) && fasta_contigs_fit(1 << 24) && !fasta_contigs_fit((1 << 24) + 1));
   CHECK(fasta_line_count(0, 0, 0) == 0 && fasta_line_count(1, 1, '\n') == 1 && fasta_line_count(1, 0, 'x') == 1 && fasta_line_count(5, 2, 'x') == 3);
   CHECK(fasta_line_count(two35, two32, '\n') == two32 && fasta_line_count(two35, two32, 'A') == two32 + 1);
   for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)1 << 24}) {
      const FastaContigLayout L = fasta_contig_layout(n);
      const size_t m = (size_t)n;
      CHECK(laid_out({L.hdr_off, L.offset, L.name_len, L.name_at, L.hdr_len, L.first_nl, L.first_odd, L.line_bases, L.line_width, L.seq_off, L.ragged},
                     {(m + 1) * 8, m * 8, m * 4, (m + 1) * 8, m * 8, m * 8, m * 8, m * 8, m * 8, (m + 1) * 8, m * 4}, L.bytes));
      CHECK(L.mins == L.first_nl && L.mins + L.mins_bytes == L.line_bases && L.first_odd > L.first_nl && L.first_odd + m * 8 <= L.mins + L.mins_bytes);
   }
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_reader_cpp")
    src, exe = d / "fasta_reader.cpp", d / "fasta_reader"
    src.write_text(PROGRAM)
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, str(src), os.path.join(csrc, "fasta_host.cpp"), "-o", str(exe)])
    return exe


def test_adversarial_buffers_and_the_schedule_restated(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-3000:])
