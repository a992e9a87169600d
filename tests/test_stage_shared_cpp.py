"""What the retained-result stages share on the host (csrc/stage_host.h), from a stand-alone C++ program that
includes that header alone and is built with AddressSanitizer and UBSan: the work-item builder, the arenas' layouts and the host
forms' column pass, each against a plain restatement written here.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "stage_host.h"
#include <cstdio>
#include <cstring>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// the items, restated: a locus of n hits is ceil(n / 16384) ranges, split when there is more than one
static std::vector<sb::HitItem> items_by_hand(const std::vector<int64_t> &hit_off, const std::vector<int64_t> &row_off, bool skip_binless)
{
   std::vector<sb::HitItem> out;
   for (size_t l = 0; l + 1 < hit_off.size(); ++l) {
      const int64_t n = hit_off[l + 1] - hit_off[l], pieces = (n + 16383) / 16384;
      if (skip_binless && row_off[l + 1] == row_off[l]) continue;
      for (int64_t i = 0; i < pieces; ++i) {
         sb::HitItem it;
         it.h0 = hit_off[l] + i * 16384, it.h1 = i + 1 < pieces ? it.h0 + 16384 : hit_off[l + 1];
         it.locus = (int32_t)l, it.split = pieces > 1;
         out.push_back(it);
      }
   }
   return out;
}
static bool same_items(const std::vector<sb::HitItem> &a, const std::vector<sb::HitItem> &b)
{
   if (a.size() != b.size()) return false;
   for (size_t i = 0; i < a.size(); ++i)
      if (a[i].h0 != b[i].h0 || a[i].h1 != b[i].h1 || a[i].locus != b[i].locus || a[i].split != b[i].split) return false;
   return true;
}
// entries (offset, bytes) in the order they were taken: aligned, behind each other, inside the arena
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
   static_assert(sizeof(sb::HitItem) == 24, "the kernels read 24-byte items");
   CHECK(sb::kStageMaxBins == 5632 && sb::kStageMaxWords == 128 && sb::kStageItemHits == 16384);
   // ---- the item builder: 0, 1, 16384, 16385, 32768, 32769 hits, then a locus with hits and no bins
   {
      const int64_t counts[7] = {0, 1, 16384, 16385, 32768, 32769, 5}, bins[7] = {2, 1, 1, 3, 1, 1, 0};
      std::vector<int64_t> hit_off(8, 0), row_off(8, 0);
      for (int l = 0; l < 7; ++l) hit_off[l + 1] = hit_off[l] + counts[l], row_off[l + 1] = row_off[l] + bins[l];
      const std::vector<sb::HitItem> all = sb::build_hit_items(hit_off.data(), 7, nullptr), binned = sb::build_hit_items(hit_off.data(), 7, row_off.data());
      CHECK(same_items(all, items_by_hand(hit_off, row_off, false)));
      CHECK(same_items(binned, items_by_hand(hit_off, row_off, true)));
      CHECK(all.size() == 0 + 1 + 1 + 2 + 2 + 3 + 1 && binned.size() == all.size() - 1);
      CHECK(all[1].split == 0 && all[1].h1 - all[1].h0 == 16384);                       // exactly one item's worth: unsplit
      CHECK(all[2].split == 1 && all[3].split == 1 && all[3].h1 - all[3].h0 == 1);      // one more: split, the second item holds it
      CHECK(all.back().locus == 6 && binned.back().locus == 5);
      CHECK(sb::build_hit_items(hit_off.data(), 0, nullptr).empty());
   }
   // ---- the layouts.  The expected numbers are written out by hand from the ladders the launchers carried:
   //      every entry rounded up to 256 bytes, at least one element each, the optional entries zero bytes when absent.
   {
      const sb::CovLayout a = sb::cov_layout(40, 300, 70, 100, 11, true);
      CHECK(a.roff == 0 && a.ioff == 512 && a.foff == 1024 && a.items == 1536 && a.eoff == 2048 && a.eleft == 2816 && a.eright == 3328);
      CHECK(a.upload_bytes == 3840 && a.live == 3840 && a.gain == 4352 && a.bases == 5120 && a.junc == 6144 && a.unex == 7168);
      CHECK(a.sums_bytes == 2560 && a.iso == 7680 && a.bytes == 8448);
      CHECK(laid_out({a.roff, a.ioff, a.foff, a.items, a.eoff, a.eleft, a.eright, a.live, a.gain, a.bases, a.junc, a.unex, a.iso},
                     {41 * 8, 41 * 8, 41 * 8, 11 * 24, 71 * 8, 100 * 4, 100 * 4, 300, 71 * 8, 100 * 8, 100 * 8, 41 * 8, 71 * 8}, a.bytes));
      const sb::CovLayout b = sb::cov_layout(40, 300, 70, 100, 11, false);
      CHECK(b.items == 1536 && b.eoff == 2048 && b.eleft == 2048 && b.eright == 2048 && b.upload_bytes == 2048 && b.live == 2048);
      CHECK(b.gain == 2560 && b.bases == 3328 && b.junc == 4352 && b.unex == 5376 && b.sums_bytes == 2560 && b.iso == 5888 && b.bytes == 6656);
      const sb::FitLayout f = sb::fit_layout(40, 300, 70, 30, 100, true, true);
      CHECK(f.small == 0 && f.large == 256 && f.upload_bytes == 768 && f.keep == 768 && f.status == 1280 && f.live == 1536 && f.gain == 2048);
      CHECK(f.exp == 2816 && f.res == 5376 && f.score == 7936 && f.ll == 8704 && f.dev == 9216 && f.pear == 9728);
      CHECK(f.nlive == 10240 && f.ndrop == 10752 && f.nimp == 11264 && f.dof == 11776 && f.worst == 12032 && f.bytes == 12288);
      CHECK(laid_out({f.small, f.large, f.keep, f.status, f.live, f.gain, f.exp, f.res, f.score, f.ll, f.dev, f.pear, f.nlive, f.ndrop, f.nimp, f.dof, f.worst},
                     {31 * 4, 101 * 4, 70 * 4, 41 * 4, 300, 70 * 8, 300 * 8, 300 * 8, 70 * 8, 41 * 8, 41 * 8, 41 * 8, 41 * 8, 41 * 8, 41 * 8, 41 * 4, 41 * 4}, f.bytes));
      const sb::FitLayout g = sb::fit_layout(40, 300, 70, 30, 100, false, false);
      CHECK(g.upload_bytes == 768 && g.keep == 768 && g.status == 768 && g.live == 768 && g.gain == 1280 && g.exp == 2048 && g.res == 4608);
      CHECK(g.score == 7168 && g.ll == 7936 && g.dev == 8448 && g.pear == 8960 && g.nlive == 9472 && g.ndrop == 9984 && g.nimp == 10496);
      CHECK(g.dof == 11008 && g.worst == 11264 && g.bytes == 11520);
      // the table's and the assignment's: nothing optional; an empty sample still gives every array one element
      const sb::CtxLayout c = sb::ctx_layout(40, 300, 2000, 11);
      CHECK(c.hoff == 0 && c.roff == 512 && c.items == 2048 && c.upload_bytes == 2560 && c.tot == c.lroff + 512 && c.rbin == c.tot + 256);
      CHECK(laid_out({c.hoff, c.roff, c.ioff, c.foff, c.items, c.nin, c.last, c.nrows, c.lhits, c.lroff, c.tot, c.rbin, c.rhits, c.rlast, c.prob},
                     {41 * 8, 41 * 8, 41 * 8, 41 * 8, 11 * 24, 300 * 4, 300 * 4, 41 * 4, 41 * 4, 41 * 8, 8, 300 * 8, 300 * 4, 300 * 8, 2000 * 8}, c.bytes));
      const sb::AsgLayout s = sb::asg_layout(40, 300, 70, 20000, 11);
      CHECK(s.items == 2048 && s.upload_bytes == 2560 && s.live == 2560 && s.uniq == s.gain + 768 && s.sums_bytes == 3 * 768 + 512);
      CHECK(laid_out({s.hoff, s.roff, s.ioff, s.foff, s.items, s.live, s.gain, s.uniq, s.map, s.post, s.unas, s.iso, s.cand, s.prob},
                     {41 * 8, 41 * 8, 41 * 8, 41 * 8, 11 * 24, 300, 70 * 8, 70 * 8, 70 * 8, 70 * 8, 41 * 8, 20000 * 4, 20000 * 4, 20000 * 8}, s.bytes));
      const sb::AsgLayout e = sb::asg_layout(0, 0, 0, 0, 0);
      CHECK(e.bytes == 14 * 256 && e.sums_bytes == 4 * 256);
      CHECK(sb::ctx_layout(0, 0, 0, 0).bytes == 15 * 256);
   }
   // ---- the column pass on three loci: one with an all-dead bin, one whose EM never started, one with a filtered isoform
   {
      const int64_t row_off[4] = {0, 3, 5, 9}, iso_off[4] = {0, 2, 5, 8}, f_off[4] = {0, 6, 12, 24};
      const double F[24] = {0.1, 0.7, /* dead: */ 0.0, SBGPU_EM_ROW_EPS, 0.2, 0.3,
                            0.5, 0.25, 0.125, 1.0, 2.0, 3.0,
                            0.1, 1e-3, 0.3, 0.2, 0.0, 1e16, 0.3, 7.0, -1e16, 1e-7, 0.0, 0.0};
      const double theta[8] = {3.0, 4.0, 1.0, 2.0, 3.0, 10.0, 20.0, 30.0};
      const int32_t keep[8] = {1, 1, 1, 1, 1, 1, 0, 1}, status[3] = {SBGPU_EM_OK, SBGPU_EM_INIT_EMPTY, SBGPU_EM_OK};
      sb::ColumnPass col;
      CHECK(sb::column_pass(3, row_off, iso_off, f_off, F, theta, keep, status, 1, &col));
      uint8_t live[9];
      double gain[8];
      uint32_t kept[3];
      for (int l = 0; l < 3; ++l) {
         const int niso = (int)(iso_off[l + 1] - iso_off[l]);
         kept[l] = 0;
         for (int j = 0; j < niso; ++j)
            if (status[l] != SBGPU_EM_INIT_EMPTY && keep[iso_off[l] + j]) kept[l] |= 1u << j;
         for (int64_t b = row_off[l]; b < row_off[l + 1]; ++b) {
            live[b] = 0;
            for (int j = 0; j < niso; ++j) live[b] |= F[f_off[l] + (b - row_off[l]) * niso + j] > SBGPU_EM_ROW_EPS;
         }
         for (int j = 0; j < niso; ++j) {
            double c = 0.0;
            for (int64_t b = row_off[l]; b < row_off[l + 1]; ++b)
               if (live[b]) c += F[f_off[l] + (b - row_off[l]) * niso + j];
            gain[iso_off[l] + j] = ((kept[l] >> j) & 1u) && c != 0.0 ? theta[iso_off[l] + j] / c : 0.0;
         }
      }
      CHECK(!live[1] && live[0] && live[2] && live[8] == 0 && kept[1] == 0 && kept[2] == 5u);
      CHECK(col.word_off[0] == 0 && col.word_off[1] == 1 && col.word_off[2] == 2 && col.word_off[3] == 3);
      CHECK(std::memcmp(col.kept.data(), kept, sizeof kept) == 0);
      CHECK(std::memcmp(col.live.data(), live, sizeof live) == 0);
      CHECK(std::memcmp(col.gain.data(), gain, sizeof gain) == 0);
      CHECK(gain[2] == 0.0 && gain[6] == 0.0 && gain[5] != 0.0);
      // the third locus' last column: (0.3 + 1e16) + -1e16 is 0.0 in ascending bins; another order gives 0.3 (its last bin is dead)
      CHECK(col.gain[7] == 0.0);
      // one locus at a time, with the column sums kept (the model fit's use)
      std::vector<int32_t> ones;
      uint32_t K[1];
      uint8_t lv[4];
      double g[3], c[3];
      CHECK(sb::kept_words(nullptr, 3, nullptr, ones, K) == 1 && K[0] == 7u);
      sb::column_pass_locus(F + 12, 4, 3, theta + 5, K, lv, g, c);
      CHECK(c[0] == (0.1 + 0.2) + 0.3 && c[1] == (1e-3 + 0.0) + 7.0 && g[1] == 20.0 / c[1] && std::memcmp(lv, live + 5, 4) == 0);
      CHECK(!sb::column_pass(3, row_off, iso_off, f_off, F, theta, keep, status, 0, &col)); // compat words that cover no locus
   }
   // ---- which locus a hit is in: by its bin, or -- without one -- by the hits' grouping
   {
      const int64_t row_off[4] = {0, 3, 3, 9}, hit_off[4] = {0, 10, 15, 40};
      CHECK(sb::locus_of_hit(0, 2, 0, 3, row_off, hit_off) == 0 && sb::locus_of_hit(20, 3, 0, 3, row_off, hit_off) == 2);
      CHECK(sb::locus_of_hit(12, -1, 0, 3, row_off, hit_off) == 1 && sb::locus_of_hit(39, -1, 1, 3, row_off, hit_off) == 2);
      CHECK(sb::locus_of_hit(12, -1, 0, 3, row_off, nullptr) == -1 && sb::locus_of_hit(12, 8, 2, 3, row_off, nullptr) == 2);
   }
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_shared_cpp")
    src, exe = d / "stage_shared.cpp", d / "stage_shared"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_items_layouts_and_column_pass_match_their_restatements(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
