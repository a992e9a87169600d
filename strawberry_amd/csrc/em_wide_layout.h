// strawberry_amd/csrc/em_wide_layout.h -- the shapes of the wide-locus kernel (em_wide.h) that the host plans with, free of HIP:
// the layouts on offer, what each costs in rows and LDS, which one serves a locus, and the descriptor of a locus inside a
// cooperative launch.  em_wide.h includes this for the kernel; plan.cpp (pack_wide_rounds) for the rounds.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sb {

constexpr int kWideWaves = 8;                  // 2 per SIMD: up to 256 VGPRs each (the sums over the waves are written as trees of 8)
constexpr int kWideThreads = 64 * kWideWaves;
constexpr unsigned kWideSpinLimit = 1u << 20;  // sweeps of an exchange's partials before giving up (~ seconds)
constexpr int kWideSweep = 8;                  // granules a thread has in flight per sweep
constexpr size_t kWideLdsCap = 159 * 1024;     // of the 160 KB a workgroup may ask for on gfx950

// (log2 column lanes, columns per lane, rows per lane in registers, rows per lane in LDS, register rows that share one
// v_rcp_f64, LDS rows per block): 64-72 doubles of F per lane in registers -- what fits beside the ~100 registers the
// iteration itself needs (phi and the partial sums of the lane's columns, a block's denominators and reciprocals, an
// LDS block's weights in flight, the owner thread's theta / phi / scale) -- and what the LDS holds beside
struct WideLayout {
   int lb_cl, cpl, r, rl, rblk, lblk;
};
constexpr int kWideLayouts = 13;
constexpr WideLayout wide_layout(int id)
{
   constexpr WideLayout t[kWideLayouts] = {
      {4, 4, 16, 9, 4, 2}, {4, 5, 14, 7, 4, 2}, {4, 6, 12, 6, 4, 2}, {4, 7, 10, 5, 2, 1}, {4, 8, 9, 4, 2, 1},
      {5, 5, 14, 6, 4, 2}, {5, 6, 12, 5, 4, 2}, {5, 7, 10, 4, 2, 1}, {5, 8, 9, 4, 2, 1},
      {6, 5, 14, 6, 4, 2}, {6, 6, 12, 4, 4, 2}, {6, 7, 10, 4, 2, 1}, {6, 8, 9, 3, 2, 1}};
   return t[id];
}
constexpr int wide_cols(int id) { return (1 << wide_layout(id).lb_cl) * wide_layout(id).cpl; } // 64 ... 512
constexpr int wide_rows_per_block(int id) { return kWideWaves * (64 >> wide_layout(id).lb_cl) * (wide_layout(id).r + wide_layout(id).rl); }
constexpr int kWideMaxCols = 512;
// dynamic LDS of a workgroup: phi[npad] | accw[waves][npad] | part[waves] | misc[8] doubles | zf[16 ints] |
// row[rows per block] {count, flag} | stage[2 npad] granules (the two-level exchange) | F[rl][cpl][threads] doubles
constexpr size_t wide_lds_bytes(int id)
{
   return (size_t)(wide_cols(id) * (1 + kWideWaves) + kWideWaves + 8) * sizeof(double) + 16 * sizeof(int) +
          (size_t)wide_rows_per_block(id) * 8 + (size_t)2 * wide_cols(id) * 16 +
          (size_t)wide_layout(id).rl * wide_layout(id).cpl * kWideThreads * sizeof(double);
}
constexpr bool wide_layouts_fit()
{
   for (int id = 0; id < kWideLayouts; ++id)
      if (wide_lds_bytes(id) > kWideLdsCap || wide_cols(id) > kWideMaxCols) return false;
   return true;
}
static_assert(wide_layouts_fit(), "a wide layout asks for more LDS than a workgroup may have");
// the layout that serves a locus with the fewest workgroups (then the narrowest: less to exchange); -1: too wide
inline int wide_layout_for(int64_t niso, int64_t nrow)
{
   int best = -1;
   int64_t best_g = 0;
   for (int id = 0; id < kWideLayouts; ++id) {
      if (niso > wide_cols(id)) continue;
      const int64_t rpb = wide_rows_per_block(id);
      const int64_t g = nrow <= rpb ? 1 : (nrow + rpb - 1) / rpb;
      if (best < 0 || g < best_g || (g == best_g && wide_cols(id) < wide_cols(best))) best = id, best_g = g;
   }
   return best;
}
// columns per slice of the two-level exchange: the smallest power of two m with m * G >= npad (m * G < 2 npad unless
// m = 1: G may exceed 2 npad, and the exchange then stages the partials in several passes)
inline int wide_lb_slice(int npad, int G)
{
   int lb = 0;
   while (((int64_t)G << lb) < npad) ++lb;
   return lb;
}

struct WideDesc {
   int32_t locus;
   int32_t first_block; // in this launch
   int32_t n_blocks;    // G
   int32_t rows_per_block;
   int64_t buf_off;     // doubles: start of this locus' 2 x G x npad exchange granules (16 bytes each)
   int32_t layout;      // wide_layout id
   int32_t npad;        // wide_cols(layout)
   int32_t lb_slice;    // two-level exchange (G > kWideSweep): a workgroup sums the 2^lb_slice columns from its index << lb_slice
   int32_t pad_;
};

} // namespace sb
