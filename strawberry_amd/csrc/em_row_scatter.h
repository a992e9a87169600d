// strawberry_amd/csrc/em_row_scatter.h -- the index math of the block form's row-lane reduce-scatter (em_device.h:
// row_lanes_scatter), free of HIP: a plain C++ compiler takes this header alone.  em_device.h asks these functions which
// lane bits the exchange runs over, which column a slot of a lane holds, which lanes store a column's wave total and where a
// slot reads its total back; it decides none of that itself.  tests/test_em_row_scatter_cpp.py runs the exchange on the CPU
// over all 256 lanes from these functions alone.
//
// The setting: a block-form lane owns S column slots (S = 6 or 8) of its column lane gc, and the M-step needs, for every
// column, the sum of a per-lane partial over all row lanes of the workgroup.  Inside a wave the row lanes are the lane bits
// 4 and 5 plus the bits below 4 that the CL column lanes leave (em_device.h, "the matrix lane map"):
//      CL   column-lane bits    row-lane bits below 4
//       1   -                   0 1 2 3
//       2   3                   0 1 2
//       4   3 2                 0 1
//       8   3 2 1               0
// L of the row-lane bits below 4 are SCATTER bits: step t = 0 .. L - 1 exchanges across scatter bit t and halves the live
// slots, so that after L steps a lane holds S / 2^L partial sums instead of S.  Slot s of a lane holds column s ^ perm,
// perm made of the lane's scatter bits with the FIRST step's bit on top: step t pairs slot s (kept: (s mod P) < D,
// P = 2^L, D = P >> (t + 1)) with the partner's slot s + D, which holds the same column in the partner's order.  No select
// anywhere: a lane always keeps the same slots.  The row-lane bits below 4 that are not scattered are all-reduced on the
// values that remain, bits 4 and 5 by one matrix instruction per remaining value; then the lanes whose non-scatter row bits
// are all zero store the wave's totals -- one lane per (column, column lane, wave) -- and after the barrier every lane reads,
// for each of its slots, the wave partials of the column that slot holds.
#pragma once

namespace sb {

constexpr int rs_pow2_factor(int x) { return (x & 1) ? 0 : 1 + rs_pow2_factor(x >> 1); } // x > 0

// scatter bits a layout offers (row-lane bits below 4, minus bit 2 for one column lane: see rs_scatter_bit)
constexpr int rs_scatter_bits_available(int lb_cl) { return lb_cl <= 1 ? 3 : (lb_cl == 2 ? 2 : 1); }
// steps of the exchange: the slots must halve evenly at every step
constexpr int rs_steps(int S, int lb_cl)
{
   return rs_pow2_factor(S) < rs_scatter_bits_available(lb_cl) ? rs_pow2_factor(S) : rs_scatter_bits_available(lb_cl);
}
// the lane bit step t exchanges across, cheapest first (the first step moves the most slots): bits 0 and 1 are quad
// permutes; then bit 3 for one column lane (a rotation of the 16-lane row by 8) and bit 2 for two (two masked row shifts)
constexpr int rs_scatter_bit(int lb_cl, int t) { return t < 2 ? t : (lb_cl == 0 ? 3 : 2); }
// mask of the row-lane bits below 4
constexpr int rs_row_bits_low(int lb_cl) { return 0xF >> lb_cl; }
constexpr int rs_scatter_mask(int S, int lb_cl)
{
   int m = 0;
   for (int t = 0; t < rs_steps(S, lb_cl); ++t) m |= 1 << rs_scatter_bit(lb_cl, t);
   return m;
}
// row-lane bits below 4 that are not scattered: all-reduced on the remaining values
constexpr int rs_rest_mask(int S, int lb_cl) { return rs_row_bits_low(lb_cl) & ~rs_scatter_mask(S, lb_cl); }

// the lane's slot order: slot s holds column s ^ rs_perm (of the lane's column lane: column gc * S + (s ^ perm) of the locus)
constexpr int rs_perm(int S, int lb_cl, int lane)
{
   const int L = rs_steps(S, lb_cl);
   int p = 0;
   for (int t = 0; t < L; ++t) p |= ((lane >> rs_scatter_bit(lb_cl, t)) & 1) << (L - 1 - t);
   return p;
}
constexpr int rs_slot_column(int s, int perm) { return s ^ perm; }

// step t: a kept slot s adds the partner's slot s + rs_step_distance
constexpr int rs_step_distance(int S, int lb_cl, int t) { return (1 << rs_steps(S, lb_cl)) >> (t + 1); }
constexpr bool rs_step_keeps(int S, int lb_cl, int t, int s)
{
   return (s & ((1 << rs_steps(S, lb_cl)) - 1)) < rs_step_distance(S, lb_cl, t);
}
// the slots that hold a value when the steps are over: 0, P, 2P, ...
constexpr bool rs_slot_remains(int S, int lb_cl, int s) { return (s & ((1 << rs_steps(S, lb_cl)) - 1)) == 0; }

// the lanes that store their remaining slots' wave totals: every non-scatter row bit zero (bits 4 and 5 among them)
constexpr bool rs_lane_stores(int S, int lb_cl, int lane) { return (lane & (0x30 | rs_rest_mask(S, lb_cl))) == 0; }

// LDS layout of one phase, in elements: [wave][column of the column lane][column lane].  The lanes of a wave read, for one
// slot and one wave's partial, the columns s ^ perm of their own column lanes: up to sixteen DIFFERENT elements, and in this
// layout they are consecutive -- one row of LDS banks, no conflict.  (With the wave index innermost, the all-reduce's
// layout, the same sixteen sit 32 bytes apart and collide four deep: measured, the base kernel took 1 007 us instead of
// 652, profiles/EXPERIMENTS_r12.md.)
constexpr int rs_lds_index(int column, int gc, int wave, int S, int CL) { return (wave * S + column) * CL + gc; }
constexpr int rs_wave_stride(int S, int CL) { return S * CL; }
// A lane's key: the index of wave 0's partial of the column its slot 0 holds.  CL is a power of two and gc < CL, so the
// xor with a slot's own multiple of CL below touches the column field alone.
constexpr int rs_lane_key(int perm, int gc, int CL) { return rs_lds_index(perm, gc, 0, 0, CL); }
// where slot s reads wave 0's partial of its column (the other waves': + wave * rs_wave_stride): rs_lds_index(s ^ perm,
// gc, 0) without a multiply
constexpr int rs_read_index(int s, int key, int CL) { return (s * CL) ^ key; }

} // namespace sb
