"""The index math of the block form's row-lane reduce-scatter (csrc/em_row_scatter.h) from a stand-alone C++ program that includes
that header alone and is built with AddressSanitizer and UBSan.  The program runs the exchange on the CPU the way em_device.h
runs it on the device -- 4 waves x 64 lanes x S slots of distinct values, the steps, the all-reduce over the other row-lane bits,
the stores, the reads after the barrier -- for every (S, CL) of the block form and every isoform count the layout can hold, and
checks at each step that the paired slots hold the same column, that each (column lane, column, wave) is stored by exactly one
lane with that wave's sum over its row lanes, that every slot of every lane reads back the total of the column it holds, and that
a column beyond the locus is never stored as anything but zero.  Values are small integers: every sum is exact, so the
comparisons are.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "em_row_scatter.h"
#include <cstdio>
#include <vector>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s (S %d CL %d niso %d)\n", __LINE__, #x, S, CL, niso); return 1; } } while (0)

constexpr int NW = 4, WAVE = 64;
// the matrix lane map's column lane, restated (em_device.h: column_lane): the top log2(CL) of lane bits 3, 2, 1
static int column_lane(int lane, int lb_cl) { return (lane >> (4 - lb_cl)) & ((1 << lb_cl) - 1); }
static double value(int wave, int lane, int column) { return 1.0 + column + 64.0 * (lane + 64.0 * wave); }

static int run(int S, int lb_cl, int niso)
{
   using namespace sb;
   const int CL = 1 << lb_cl, L = rs_steps(S, lb_cl), P = 1 << L;
   CHECK(L >= 1 && L <= 3 && S % P == 0);
   // the bits: scatter bits are distinct row-lane bits below 4, the rest is the rest, and no column-lane bit is touched
   const int row_low = rs_row_bits_low(lb_cl), smask = rs_scatter_mask(S, lb_cl), rest = rs_rest_mask(S, lb_cl);
   int seen = 0;
   for (int t = 0; t < L; ++t) {
      const int b = rs_scatter_bit(lb_cl, t);
      CHECK(b >= 0 && b < 4 && ((row_low >> b) & 1) && !((seen >> b) & 1));
      seen |= 1 << b;
   }
   CHECK(seen == smask && (smask & rest) == 0 && (smask | rest) == row_low);
   CHECK((row_low & ((CL - 1) << (4 - lb_cl))) == 0);

   // x[wave][lane][slot]: the lane's partial of the column its slot holds; a column beyond the locus contributes zero
   std::vector<double> x((size_t)NW * WAVE * S), y;
   auto at = [&](std::vector<double> &v, int w, int lane, int s) -> double & { return v.at(((size_t)w * WAVE + lane) * S + s); };
   std::vector<double> wave_sum((size_t)NW * CL * S, 0.0), total((size_t)CL * S, 0.0); // [wave][gc][column], [gc][column]
   for (int w = 0; w < NW; ++w)
      for (int lane = 0; lane < WAVE; ++lane) {
         const int gc = column_lane(lane, lb_cl), perm = rs_perm(S, lb_cl, lane);
         CHECK(perm >= 0 && perm < P);
         std::vector<int> held(S, 0);
         for (int s = 0; s < S; ++s) {
            const int c = rs_slot_column(s, perm);
            CHECK(c >= 0 && c < S && !held[c]); // a lane's slots hold each of its S columns once
            held[c] = 1;
            const double v = gc * S + c < niso ? value(w, lane, c) : 0.0;
            at(x, w, lane, s) = v;
            wave_sum.at(((size_t)w * CL + gc) * S + c) += v;
            total.at((size_t)gc * S + c) += v;
         }
      }
   // the scatter steps
   for (int t = 0; t < L; ++t) {
      const int bit = rs_scatter_bit(lb_cl, t), D = rs_step_distance(S, lb_cl, t);
      CHECK(D == (P >> (t + 1)));
      y = x;
      for (int w = 0; w < NW; ++w)
         for (int lane = 0; lane < WAVE; ++lane) {
            const int partner = lane ^ (1 << bit);
            CHECK(column_lane(partner, lb_cl) == column_lane(lane, lb_cl));
            for (int s = 0; s < S; ++s) {
               if (!rs_step_keeps(S, lb_cl, t, s)) continue;
               CHECK(s + D < S && !rs_step_keeps(S, lb_cl, t, s + D));
               // the paired slots hold the same column
               CHECK(rs_slot_column(s, rs_perm(S, lb_cl, lane)) == rs_slot_column(s + D, rs_perm(S, lb_cl, partner)));
               at(y, w, lane, s) = at(x, w, lane, s) + at(x, w, partner, s + D);
            }
         }
      x = y;
   }
   // the remaining slots: all-reduce over the row-lane bits that were not scattered, bits 4 and 5 among them
   const int rest_all = rest | 0x30;
   y = x;
   int n_remain = 0;
   for (int s = 0; s < S; ++s) n_remain += rs_slot_remains(S, lb_cl, s) ? 1 : 0;
   CHECK(n_remain == S / P);
   for (int w = 0; w < NW; ++w)
      for (int lane = 0; lane < WAVE; ++lane)
         for (int s = 0; s < S; ++s) {
            if (!rs_slot_remains(S, lb_cl, s)) continue;
            for (int t = 0; t < L; ++t) CHECK(rs_step_keeps(S, lb_cl, t, s)); // it took part in every step
            double sum = 0.0;
            for (int m = 0; m < WAVE; ++m) {
               if ((m & ~rest_all) != 0) continue;
               CHECK(rs_perm(S, lb_cl, lane ^ m) == rs_perm(S, lb_cl, lane) && column_lane(lane ^ m, lb_cl) == column_lane(lane, lb_cl));
               sum += at(x, w, lane ^ m, s);
            }
            at(y, w, lane, s) = sum;
         }
   x = y;
   // the stores: one phase of [wave][column][column lane]
   const int lds_size = S * CL * NW;
   std::vector<double> lds((size_t)lds_size, -1.0);
   std::vector<int> stores((size_t)lds_size, 0);
   for (int w = 0; w < NW; ++w)
      for (int lane = 0; lane < WAVE; ++lane) {
         if (!rs_lane_stores(S, lb_cl, lane)) continue;
         const int gc = column_lane(lane, lb_cl), perm = rs_perm(S, lb_cl, lane), key = rs_lane_key(perm, gc, CL);
         for (int s = 0; s < S; ++s) {
            if (!rs_slot_remains(S, lb_cl, s)) continue;
            const int idx = rs_read_index(s, key, CL) + w * rs_wave_stride(S, CL);
            CHECK(idx >= 0 && idx < lds_size);
            CHECK(idx == rs_lds_index(rs_slot_column(s, perm), gc, w, S, CL));
            lds.at((size_t)idx) = at(x, w, lane, s);
            stores.at((size_t)idx) += 1;
         }
      }
   for (int c = 0; c < S; ++c)
      for (int gc = 0; gc < CL; ++gc)
         for (int w = 0; w < NW; ++w) {
            const int idx = rs_lds_index(c, gc, w, S, CL);
            CHECK(stores.at((size_t)idx) == 1);                                          // by exactly one lane
            CHECK(lds.at((size_t)idx) == wave_sum.at(((size_t)w * CL + gc) * S + c));     // the wave's sum over its row lanes
            if (gc * S + c >= niso) CHECK(lds.at((size_t)idx) == 0.0);                   // beyond the locus: zero
         }
   // the reads: every slot of every lane ends with the total of the column it holds
   for (int w = 0; w < NW; ++w)
      for (int lane = 0; lane < WAVE; ++lane) {
         const int gc = column_lane(lane, lb_cl), perm = rs_perm(S, lb_cl, lane), key = rs_lane_key(perm, gc, CL);
         for (int s = 0; s < S; ++s) {
            const int idx = rs_read_index(s, key, CL), stride = rs_wave_stride(S, CL);
            CHECK(idx >= 0 && idx + (NW - 1) * stride < lds_size);
            double sum = lds.at((size_t)idx);
            for (int v = 1; v < NW; ++v) sum += lds.at((size_t)idx + (size_t)v * stride);
            CHECK(sum == total.at((size_t)gc * S + rs_slot_column(s, perm)));
         }
      }
   return 0;
}

int main()
{
   using namespace sb;
   // the step counts and bit orders of the eight block instantiations, by hand
   static_assert(rs_steps(8, 0) == 3 && rs_steps(8, 1) == 3 && rs_steps(8, 2) == 2 && rs_steps(8, 3) == 1, "S = 8");
   static_assert(rs_steps(6, 0) == 1 && rs_steps(6, 1) == 1 && rs_steps(6, 2) == 1 && rs_steps(6, 3) == 1, "S = 6");
   static_assert(rs_scatter_bit(0, 0) == 0 && rs_scatter_bit(0, 1) == 1 && rs_scatter_bit(0, 2) == 3, "CL = 1: 0 1 3");
   static_assert(rs_scatter_bit(1, 0) == 0 && rs_scatter_bit(1, 1) == 1 && rs_scatter_bit(1, 2) == 2, "CL = 2: 0 1 2");
   static_assert(rs_rest_mask(8, 0) == 4 && rs_rest_mask(8, 1) == 0 && rs_rest_mask(8, 2) == 0 && rs_rest_mask(8, 3) == 0, "S = 8");
   static_assert(rs_rest_mask(6, 0) == 14 && rs_rest_mask(6, 1) == 6 && rs_rest_mask(6, 2) == 2 && rs_rest_mask(6, 3) == 0, "S = 6");
   int n_cases = 0;
   for (int S : {6, 8})
      for (int lb_cl = 0; lb_cl <= 3; ++lb_cl)
         for (int niso = 1; niso <= S << lb_cl; ++niso) {
            if (run(S, lb_cl, niso)) return 1;
            ++n_cases;
         }
   if (n_cases != 15 * 6 + 15 * 8) { std::printf("%d cases\n", n_cases); return 1; }
   // the critical layout: 8 slots on 2 column lanes -- sixteen lanes of a wave store, one value each
   int storing = 0;
   for (int lane = 0; lane < 64; ++lane) storing += rs_lane_stores(8, 1, lane) ? 1 : 0;
   if (storing != 16) { std::printf("%d storing lanes\n", storing); return 1; }
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("em_row_scatter_cpp")
    src, exe = d / "em_row_scatter.cpp", d / "em_row_scatter"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_every_block_layout_scatters_stores_and_reads_back_its_columns(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
