"""What the front end (records -> unique hits) decides on the host (csrc/front_schedule.h) from a stand-alone C++ program that
includes that header alone and is built with AddressSanitizer and UBSan: the eight layouts against the `off += up256(...)` chains
they replace (written out here from the launchers as they were before the layouts were functions), the zeroed ranges against the
arrays those launchers zeroed, the mate sort's key against a table worked out by hand from the loop it was, the collapse's
one sort or two, the decode kernels' launches, the stream's window arithmetic and the growth rule.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "front_schedule.h"
#include <cstdio>
#include <vector>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
using namespace sb;

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
// the launchers' `take`: an empty array takes 8 bytes, so 256
struct Chain {
   size_t off = 0;
   size_t take(size_t bytes)
   {
      const size_t o = off;
      off += up(bytes ? bytes : 8);
      return o;
   }
};

// ---- mate pairing: scratch, the sorted form's block, the pairs' arena
static int check_mate(int64_t nr, int64_t n_loci, size_t tmp_bytes, size_t sort_tmp_bytes)
{
   const size_t n = (size_t)nr, n1 = n + 1, nl1 = (size_t)n_loci + 1;
   const size_t nt = (n1 + 63) / 64, nt1 = nt + 1;
   Chain c;
   const size_t o_roff = c.take(nl1 * 8), o_rarr = c.take(n * 24), o_lefts = c.take(n * 4), o_claim = c.take(n * 4), o_slot = c.take(n * 8), o_runlen = c.take(n * 4);
   const size_t o_done = c.take(n * 8), o_td = c.take(nt1 * 4), o_tda = c.take(nt1 * 8), o_prec = c.take(n * 4), o_pval = c.take(n * 4);
   const size_t o_lf = c.take(n1 * 4), o_rf = c.take(n1 * 4), o_tl = c.take(nt1 * 4), o_tr = c.take(nt1 * 4), o_ls = c.take(nt1 * 8), o_rs = c.take(nt1 * 8), o_poff = c.take(nl1 * 8),
                o_counts = c.take(64 * 64 + 256), o_tmp = c.take(tmp_bytes);
   const MateScratchLayout L = mate_scratch_layout(nr, n_loci, tmp_bytes);
   CHECK(L.roff == o_roff && L.rarr == o_rarr && L.lefts == o_lefts && L.claim == o_claim && L.slot == o_slot && L.runlen == o_runlen);
   CHECK(L.done == o_done && L.td == o_td && L.tda == o_tda && L.prec == o_prec && L.pval == o_pval);
   CHECK(L.lf == o_lf && L.rf == o_rf && L.tl == o_tl && L.tr == o_tr && L.ls == o_ls && L.rs == o_rs && L.poff == o_poff && L.counts == o_counts && L.tmp == o_tmp);
   CHECK(L.bytes == c.off && L.bytes % 256 == 0);
   // what was zeroed: the counters' block whole; the entry beyond the last DONE tile of tile_done ((n + 63) / 64: the tiles of
   // the n records), the entry beyond the last tile of tile_l and tile_r ((n + 1 + 63) / 64); `slot` whole for the positional form
   CHECK(L.counts_bytes == 64 * 64 + 256 && L.counts + L.counts_bytes <= L.tmp && L.trouble == o_counts + 64 * 64 && L.trouble + 4 <= L.counts + L.counts_bytes);
   CHECK(L.done_tiles == (n + 63) / 64 && L.pair_tiles == nt && L.done_tiles <= L.pair_tiles);
   CHECK(L.td_tail == o_td + ((n + 63) / 64) * 4 && L.td_tail + 4 <= L.tda); // inside tile_done's nt1 entries
   CHECK(L.tl_tail == o_tl + nt * 4 && L.tl_tail + 4 <= L.tr && L.tr_tail == o_tr + nt * 4 && L.tr_tail + 4 <= L.ls);
   CHECK(L.slot_bytes == n * 8 && L.slot + L.slot_bytes <= L.runlen);
   // what was read back: the two scans' totals
   CHECK(L.ls_total == o_ls + nt * 8 && L.ls_total + 8 <= L.rs && L.rs_total == o_rs + nt * 8 && L.rs_total + 8 <= L.poff);

   Chain c2;
   const size_t o_key = c2.take(n * 4), o_skey = c2.take(n * 4), o_order = c2.take(n * 4), o_rec = c2.take(n * 24), o_state = c2.take(n), o_stmp = c2.take(sort_tmp_bytes);
   const MateSortedLayout S = mate_sorted_layout(nr, sort_tmp_bytes);
   CHECK(S.key == o_key && S.skey == o_skey && S.order == o_order && S.rec == o_rec && S.state == o_state && S.stmp == o_stmp && S.bytes == c2.off);
   return 0;
}
static int check_mate_pairs(int64_t n_pairs, int64_t n_lfeat, int64_t n_rfeat)
{
   const size_t np1 = (size_t)n_pairs + 1, nlf = (size_t)n_lfeat + 1, nrf = (size_t)n_rfeat + 1;
   size_t t = 0;
   const size_t u_mass = t; t += up(np1 * 8);
   const size_t u_loff = t; t += up(np1 * 8);
   const size_t u_roff = t; t += up(np1 * 8);
   const size_t u_ll = t; t += up(nlf * 4);
   const size_t u_lr = t; t += up(nlf * 4);
   const size_t u_rl = t; t += up(nrf * 4);
   const size_t u_rr = t; t += up(nrf * 4);
   const size_t u_lc = t; t += up(nlf);
   const size_t u_rc = t; t += up(nrf);
   const MatePairsLayout P = mate_pairs_layout(n_pairs, n_lfeat, n_rfeat);
   CHECK(P.mass == u_mass && P.loff == u_loff && P.roff == u_roff && P.ll == u_ll && P.lr == u_lr && P.rl == u_rl && P.rr == u_rr && P.lc == u_lc && P.rc == u_rc && P.bytes == t);
   return 0;
}

// ---- collapse: scratch, the unique hits' arena
static int check_collapse(int64_t np, int64_t n_loci, size_t tmp_bytes)
{
   const size_t n = (size_t)np, n1 = n + 1, nl1 = (size_t)n_loci + 1;
   Chain c;
   const size_t o_poff = c.take(nl1 * 8), o_kr = c.take(n * 4), o_kr2 = c.take(n * 4), o_khi = c.take(n * 8), o_sl = c.take(n * 4), o_sr = c.take(n * 4);
   const size_t o_sum = c.take(nl1 * 8), o_sq = c.take(nl1 * 8), o_nm = c.take(nl1 * 4), o_clf = c.take(nl1 * 4), o_cm = c.take(nl1 * 8), o_mean = c.take(nl1 * 8), o_sd = c.take(nl1 * 8);
   const size_t o_perm1 = c.take(n * 4), o_key2 = c.take(n * 8), o_key2s = c.take(n * 8), o_order = c.take(n * 4);
   const size_t o_skip = c.take(n), o_head = c.take(n), o_kept = c.take(n * 4), o_last = c.take(n * 4), o_nfeat = c.take(n1 * 4), o_ishit = c.take(n1 * 4);
   const size_t o_gid = c.take(n * 4), o_hrank = c.take(n1 * 8), o_fbase = c.take(n1 * 8), o_gmass = c.take(n1 * 8), o_hoff = c.take(nl1 * 8);
   const size_t o_minl = c.take(nl1 * 4), o_maxl = c.take(nl1 * 4), o_cspan = c.take(nl1 * 8), o_cbase = c.take(nl1 * 8), o_clof = c.take(n * 4), o_ostat = c.take(64);
   const size_t o_counts = c.take(64), o_flag = c.take(64), o_tmp = c.take(tmp_bytes);
   const CollapseScratchLayout L = collapse_scratch_layout(np, n_loci, tmp_bytes);
   CHECK(L.poff == o_poff && L.kr == o_kr && L.kr2 == o_kr2 && L.khi == o_khi && L.sl == o_sl && L.sr == o_sr);
   CHECK(L.sum == o_sum && L.sq == o_sq && L.nm == o_nm && L.clf == o_clf && L.cm == o_cm && L.mean == o_mean && L.sd == o_sd);
   CHECK(L.perm1 == o_perm1 && L.key2 == o_key2 && L.key2s == o_key2s && L.order == o_order);
   CHECK(L.skip == o_skip && L.head == o_head && L.kept == o_kept && L.last == o_last && L.nfeat == o_nfeat && L.ishit == o_ishit);
   CHECK(L.gid == o_gid && L.hrank == o_hrank && L.fbase == o_fbase && L.gmass == o_gmass && L.hoff == o_hoff);
   CHECK(L.minl == o_minl && L.maxl == o_maxl && L.cspan == o_cspan && L.cbase == o_cbase && L.clof == o_clof && L.ostat == o_ostat);
   CHECK(L.counts == o_counts && L.flag == o_flag && L.tmp == o_tmp && L.bytes == c.off);
   // what was zeroed: [o_sum, o_mean) -- exactly S1, S2, the mates' counts, the clusters' flags and masses --, [o_counts, o_tmp)
   // -- exactly the counters and the flags --, gmass whole, minl (0xFF) and maxl, ostat, the two scan inputs' last entry
   CHECK(L.sums_bytes == o_mean - o_sum && L.sums_bytes == 3 * up(nl1 * 8) + 2 * up(nl1 * 4) && L.sum + L.sums_bytes == L.mean);
   CHECK(L.counters_bytes == o_tmp - o_counts && L.counters_bytes == 512 && L.counts + L.counters_bytes == L.tmp && L.flag == L.counts + 256);
   CHECK(L.gmass_bytes == n1 * 8 && L.gmass + L.gmass_bytes <= L.hoff);
   CHECK(L.cluster_words_bytes == nl1 * 4 && L.minl + L.cluster_words_bytes <= L.maxl && L.maxl + L.cluster_words_bytes <= L.cspan && L.clf_words == nl1);
   CHECK(L.ostat_bytes == 64 && L.ostat + 64 <= L.counts);
   CHECK(L.nfeat_tail == o_nfeat + n * 4 && L.nfeat_tail + 4 <= L.ishit && L.ishit_tail == o_ishit + n * 4 && L.ishit_tail + 4 <= L.gid);
   // what was read back
   CHECK(L.x_total == o_cbase + (size_t)n_loci * 8 && L.x_total + 8 <= L.clof && L.n_feat == o_fbase + n * 8 && L.n_feat + 8 <= L.gmass);
   return 0;
}
static int check_collapse_hits(int64_t n_hits, int64_t n_feat)
{
   const size_t nh1 = (size_t)n_hits + 1, nfe1 = (size_t)n_feat + 1;
   size_t t = 0;
   const size_t u_off = t; t += up(nh1 * 8);
   const size_t u_loc = t; t += up(nh1 * 4);
   const size_t u_mass = t; t += up(nh1 * 4);
   const size_t u_left = t; t += up(nfe1 * 4);
   const size_t u_right = t; t += up(nfe1 * 4);
   const size_t u_code = t; t += up(nfe1);
   const CollapseHitsLayout H = collapse_hits_layout(n_hits, n_feat);
   CHECK(H.off == u_off && H.loc == u_loc && H.mass == u_mass && H.left == u_left && H.right == u_right && H.code == u_code && H.bytes == t);
   return 0;
}

// ---- decode: the handle's arrays, the one-pass scratch, the two-pass scratch
static int check_decode(int64_t n_records, int64_t n_reads, int64_t n_blocks, size_t tmp_bytes)
{
   {
      const size_t n = (size_t)n_records, m = (size_t)n_reads, nb = (size_t)n_blocks;
      Chain c;
      const size_t status = c.take(n), record = c.take(m * 8), read_id = c.take(m * 8), ref = c.take(m * 4), nh = c.take(m * 4), nm = c.take(m * 4), read_len = c.take(m * 4);
      const size_t left = c.take(m * 4), right = c.take(m * 4), partner_pos = c.take(m * 4), sam_flag = c.take(m * 4), flags = c.take(m), block_off = c.take((m + 1) * 8);
      const size_t block_left = c.take(nb * 4), block_right = c.take(nb * 4);
      const BamReadsLayout R = bam_reads_layout(n_records, n_reads, n_blocks);
      CHECK(R.status == status && R.record == record && R.read_id == read_id && R.ref == ref && R.nh == nh && R.nm == nm && R.read_len == read_len);
      CHECK(R.left == left && R.right == right && R.partner_pos == partner_pos && R.sam_flag == sam_flag && R.flags == flags && R.block_off == block_off);
      CHECK(R.block_left == block_left && R.block_right == block_right && R.bytes == c.off);
   }
   {
      const size_t tiles = ((size_t)n_records + 1024 - 1) / 1024;
      const size_t o_state = 0, o_cnt1 = up(tiles * 8), o_ticket = o_cnt1 + up(16 * 8), w_bytes = o_ticket + 256;
      const BamOnepassScratch W = bam_onepass_scratch((int64_t)tiles);
      CHECK(W.state == o_state && W.counts == o_cnt1 && W.ticket == o_ticket && W.bytes == w_bytes); // zeroed whole
   }
   {
      const size_t nn = (size_t)n_records, n1 = nn + 1, nt = (nn + 63) / 64, nt1 = nt + 1;
      Chain c;
      const size_t o_status = c.take(nn), o_acc = c.take(n1), o_nb = c.take(n1 * 4), o_rid = c.take(nn * 8), o_ref = c.take(nn * 4), o_nh = c.take(nn * 4),
                   o_nm = c.take(nn * 4), o_rl = c.take(nn * 4), o_left = c.take(nn * 4), o_right = c.take(nn * 4), o_pp = c.take(nn * 4), o_sf = c.take(nn * 4),
                   o_fl = c.take(nn), o_ib = c.take(nn * 4 * 2 * 3), o_tr = c.take(nt1 * 4), o_tb = c.take(nt1 * 4), o_rat = c.take(nt1 * 8), o_bat = c.take(nt1 * 8),
                   o_cnt = c.take(16 * 8), o_tmp = c.take(tmp_bytes);
      const BamScanScratch L = bam_scan_scratch(n_records, tmp_bytes);
      CHECK(L.status == o_status && L.acc == o_acc && L.nb == o_nb && L.rid == o_rid && L.ref == o_ref && L.nh == o_nh && L.nm == o_nm && L.rl == o_rl);
      CHECK(L.left == o_left && L.right == o_right && L.pp == o_pp && L.sf == o_sf && L.fl == o_fl && L.ib == o_ib && L.tr == o_tr && L.tb == o_tb);
      CHECK(L.rat == o_rat && L.bat == o_bat && L.cnt == o_cnt && L.tmp == o_tmp && L.bytes == c.off && L.tiles == nt);
      CHECK(L.cnt_bytes == 16 * 8 && L.cnt + L.cnt_bytes <= L.tmp);
      CHECK(L.tr_tail == o_tr + nt * 4 && L.tr_tail + 4 <= L.tb && L.tb_tail == o_tb + nt * 4 && L.tb_tail + 4 <= L.rat);
      CHECK(L.rat_total == o_rat + nt * 8 && L.rat_total + 8 <= L.bat && L.bat_total == o_bat + nt * 8 && L.bat_total + 8 <= L.cnt);
   }
   return 0;
}

// ---- the mate sort's key, restated as the loop it was
static MateSortKey key_by_loop(int64_t n_loci, const int64_t *locus_read_off)
{
   unsigned locus_bits = 1;
   while (((int64_t)1 << locus_bits) < n_loci) ++locus_bits;
   unsigned hash_bits = 32, group_shift = locus_bits, sort_bits = 32;
   for (unsigned g = 0; g <= locus_bits; ++g) {
      int64_t biggest = 1;
      for (int64_t l = 0; l < n_loci; l += (int64_t)1 << g) biggest = std::max(biggest, locus_read_off[std::min<int64_t>(n_loci, l + ((int64_t)1 << g))] - locus_read_off[l]);
      unsigned hb = 2;
      while (((int64_t)1 << (hb - 2)) < biggest) ++hb;
      if (locus_bits - g + hb <= 32 || g == locus_bits) {
         hash_bits = std::min(32u, hb), group_shift = g;
         sort_bits = std::min(32u, locus_bits - g + hash_bits);
         break;
      }
   }
   return {locus_bits, group_shift, hash_bits, sort_bits};
}
static bool key_is(const std::vector<int64_t> &counts, unsigned locus_bits, unsigned group_shift, unsigned hash_bits, unsigned sort_bits)
{
   std::vector<int64_t> off(counts.size() + 1, 0);
   for (size_t l = 0; l < counts.size(); ++l) off[l + 1] = off[l] + counts[l];
   const MateSortKey k = mate_sort_key((int64_t)counts.size(), off.data()), w = key_by_loop((int64_t)counts.size(), off.data());
   if (k.locus_bits != w.locus_bits || k.group_shift != w.group_shift || k.hash_bits != w.hash_bits || k.sort_bits != w.sort_bits) return false;
   if (k.locus_bits != locus_bits || k.group_shift != group_shift || k.hash_bits != hash_bits || k.sort_bits != sort_bits)
      std::printf("key: %u %u %u %u\n", k.locus_bits, k.group_shift, k.hash_bits, k.sort_bits);
   return k.locus_bits == locus_bits && k.group_shift == group_shift && k.hash_bits == hash_bits && k.sort_bits == sort_bits;
}

int main()
{
   CHECK(kFlatRecBytes == 24 && kFrontOneWaves == 4 && kFrontOneTile == 1024 && kFrontInlineBlocks == 3);
   CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
   {  // the arena's two takes: an empty array takes nothing, or a place of its own
      Arena a;
      CHECK(a.take(0) == 0 && a.size == 0 && a.take_nonempty(0) == 0 && a.size == 256 && a.take(300) == 256 && a.size == 768 && a.take_nonempty(1) == 768 && a.size == 1024);
   }

   // ---- the layouts: n = 1, 63, 64, 65, 2^31 - 3; one cluster and 2^23; nothing found
   const int64_t big = ((int64_t)1 << 31) - 3;
   for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4097, big})
      for (int64_t n_loci : {(int64_t)1, (int64_t)1 << 23})
         for (size_t tmp : {(size_t)0, (size_t)1, (size_t)123457}) {
            if (check_mate(n, n_loci, tmp, tmp * 3)) return 1;
            if (check_collapse(n, n_loci, tmp)) return 1;
            if (check_decode(n, n, 2 * n + 1024, tmp)) return 1; // the one-pass attempt's handle: every record, two blocks each
            if (check_decode(n, n / 2, n / 3, tmp)) return 1;
            if (check_decode(n, 0, 0, tmp)) return 1;             // no record accepted
         }
   for (int64_t np : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, big})
      for (int64_t nf : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, 3 * big}) {
         if (check_mate_pairs(np, nf, 0) || check_mate_pairs(np, 0, nf) || check_mate_pairs(np, nf, nf / 2)) return 1;
         if (check_collapse_hits(np, nf)) return 1;
      }

   // ---- mate_sort_key, by hand from the loop: locus_bits is the smallest b >= 1 with 2^b >= n_loci; hb is 2 + the smallest e with
   // 2^e >= the biggest group's records; the first g with locus_bits - g + hb <= 32 is taken (g == locus_bits at the latest)
   // one cluster of 5 records: locus_bits 1, g = 0: hb = 2 + 3 = 5, 1 + 5 <= 32 -> sort over 1 + 5 bits
   CHECK(key_is({5}, 1, 0, 5, 6));
   // one cluster of one record: hb = 2
   CHECK(key_is({1}, 1, 0, 2, 3));
   // 2^23 clusters of 2 records: locus_bits 23, hb = 3: 26 bits at g = 0
   CHECK(key_is(std::vector<int64_t>((size_t)1 << 23, 2), 23, 0, 3, 26));
   {  // 2^20 clusters of one record, one of them with 4096: g = 0: hb = 14, 20 + 14 = 34; g = 1: the group holds 4097: hb = 15,
      // 19 + 15 = 34; g = 2: 4099: 18 + 15 = 33; g = 3: 4103: 17 + 15 = 32 fits
      std::vector<int64_t> counts((size_t)1 << 20, 1);
      counts[777] = 4096;
      CHECK(key_is(counts, 20, 3, 15, 32));
   }
   // one cluster of 2^31 - 3 records: hb = 2 + 31 = 33; g = 0: 1 + 33 > 32; g = 1 is the last: the hash is capped at 32 bits
   CHECK(key_is({big}, 1, 1, 32, 32));
   // 5 clusters (no power of two): locus_bits 3; the group beyond the last cluster ends at n_loci
   CHECK(key_is({3, 0, 9, 1, 2}, 3, 0, 6, 9));
   // 3 clusters, the last group of g = 1 is cut at n_loci: g = 0 already fits, and 2^28 records want 30 bits: 2 + 30 = 32
   CHECK(key_is({(int64_t)1 << 28, (int64_t)1 << 28, 7}, 2, 0, 30, 32));
   // ... one record more and g = 0 (2 + 31) does not fit; g = 1: groups {0, 1} and {2}: 2^29 + 1 records: hb = 32, 1 + 32 > 32; g = 2 is the last
   CHECK(key_is({((int64_t)1 << 28) + 1, (int64_t)1 << 28, 7}, 2, 2, 32, 32));

   // ---- collapse_sort_choice
   {
      const unsigned long long top = ~0ull;
      CollapseSortChoice c = collapse_sort_choice(top >> 44, top >> 20, 0, false); // 20 + 44 = 64
      CHECK(c.one_sort && c.span_bits == 20 && c.x_bits == 44 && c.end_bit == 64);
      c = collapse_sort_choice(top >> 43, top >> 20, 0, false);                     // 21 + 44 = 65
      CHECK(!c.one_sort && c.span_bits == 21 && c.x_bits == 44);
      c = collapse_sort_choice(1000, 5000, 3, false);                              // pairs out of order
      CHECK(!c.one_sort && c.span_bits == 10 && c.x_bits == 13);
      c = collapse_sort_choice(1000, 5000, 0, true);                               // the tests' hook
      CHECK(!c.one_sort);
      c = collapse_sort_choice(1000, 5000, 0, false);
      CHECK(c.one_sort && c.end_bit == 23);
      c = collapse_sort_choice(0, 0, 0, false);                                    // all zeros: a sort over one bit
      CHECK(c.one_sort && c.span_bits == 0 && c.x_bits == 0 && c.end_bit == 1);
      c = collapse_sort_choice(top, top, 0, false);
      CHECK(!c.one_sort && c.span_bits == 64 && c.x_bits == 64);
      CHECK(front_locus_bits(0) == 1 && front_locus_bits(1) == 1 && front_locus_bits(2) == 1 && front_locus_bits(3) == 2 && front_locus_bits(5) == 3);
      CHECK(front_locus_bits((int64_t)1 << 23) == 23 && front_locus_bits(((int64_t)1 << 23) + 1) == 24);
   }

   // ---- the decode's launches (256 CUs, 64 KB of LDS per workgroup, unless said otherwise)
   {
      // tiny records (36 bytes): the floors.  One pass: 64 * 37 * 26 / 25 + 512 = 2974 -> 3072 < 4096; 160 KB / (4 * 4096 + 512) = 9 -> 8 resident
      BamOnepassLaunch p = bam_onepass_launch(1000000, 36000000, 65536, 256);
      CHECK(p.block_cap == 2001024 && p.tiles == 977 && p.stage_bytes == 4096 && p.resident == 8 && p.grid == 977);
      // the scan: 70 * 37 = 2590 < 8 KB; 160 KB / (8192 + 256) = 19 -> 16 resident; 15625 waves < 256 * 16 * 4
      BamScanLaunch q = bam_scan_launch(1000000, 36000000, 65536, 256);
      CHECK(q.stage_bytes == 8192 && q.resident == 16 && q.scan_blocks == 15625 && q.fill_blocks == 3907);
      // 1 KB records: the caps.  One pass: 64 * 1025 * 1.04 + 512 > 32 KB -> 32 KB, but a workgroup gets (65536 - 512) / 4 = 16256 -> 16128
      p = bam_onepass_launch(1000000, 1024000000, 65536, 256);
      CHECK(p.stage_bytes == 16128 && p.resident == 2 && p.grid == 512);
      // ... with 160 KB to ask for, the cap itself: 32 KB a wave, one workgroup per CU
      p = bam_onepass_launch(1000000, 1024000000, 160 * 1024, 256);
      CHECK(p.stage_bytes == 32768 && p.resident == 1 && p.grid == 256);
      // the scan: 70 * 1025 > 64 KB -> 64 KB, less the static words: 65536 - 256; 160 KB / 65536 = 2 resident
      q = bam_scan_launch(1000000, 1024000000, 65536, 256);
      CHECK(q.stage_bytes == 65280 && q.resident == 2 && q.scan_blocks == 2048 && q.fill_blocks == 3907);
      q = bam_scan_launch(1000000, 1024000000, 160 * 1024, 256);
      CHECK(q.stage_bytes == 65536 && q.resident == 2);
      // in between: 200-byte records: 64 * 201 * 26 / 25 + 512 = 13890 -> 14080; 160 KB / (4 * 14080 + 512) = 2
      p = bam_onepass_launch(1 << 20, 200ll << 20, 65536, 256);
      CHECK(p.stage_bytes == 14080 && p.resident == 2 && p.tiles == 1024 && p.grid == 512);
      // ... the scan: 70 * 201 = 14070 -> 8 KB + 3 * 2 KB = 14336; 160 KB / 14592 = 11; 16384 waves > 256 * 11 * 4
      q = bam_scan_launch(1 << 20, 200ll << 20, 65536, 256);
      CHECK(q.stage_bytes == 14336 && q.resident == 11 && q.scan_blocks == 11264 && q.fill_blocks == 4096);
      // a device that grants no LDS to speak of: no staging buffer, the most workgroups
      p = bam_onepass_launch(1000, 100000, 512, 256);
      CHECK(p.stage_bytes == 0 && p.resident == 8);
      p = bam_onepass_launch(1000, 100000, 1000, 256); // (1000 - 512) / 4 = 122 -> 0 in steps of 256
      CHECK(p.stage_bytes == 0);
      p = bam_onepass_launch(1000, 100000, 100, 256);  // (less than the static words)
      CHECK(p.stage_bytes == 0);
      q = bam_scan_launch(1000, 100000, 256, 256);
      CHECK(q.stage_bytes == 0 && q.resident == 16);
      q = bam_scan_launch(1000, 100000, 100, 256);
      CHECK(q.stage_bytes == 0 && q.resident == 16);
      // fewer records than a tile: one workgroup
      p = bam_onepass_launch(1, 36, 65536, 256);
      CHECK(p.tiles == 1 && p.grid == 1 && p.block_cap == 1026 && p.stage_bytes == 4096);
      p = bam_onepass_launch(1023, 36 * 1023, 65536, 256);
      CHECK(p.tiles == 1 && p.grid == 1);
      p = bam_onepass_launch(1025, 36 * 1025, 65536, 256);
      CHECK(p.tiles == 2 && p.grid == 2);
      q = bam_scan_launch(1, 36, 65536, 256);
      CHECK(q.scan_blocks == 1 && q.fill_blocks == 1);
      q = bam_scan_launch(63, 36 * 63, 65536, 256);
      CHECK(q.scan_blocks == 1 && q.fill_blocks == 1);
      q = bam_scan_launch(257, 36 * 257, 65536, 256);
      CHECK(q.scan_blocks == 5 && q.fill_blocks == 2);
      // the grids' caps: CUs x resident (x 4 for the scan's one-wave workgroups), CUs x 32 for the fill
      p = bam_onepass_launch(big, 36 * big, 65536, 4);
      CHECK(p.grid == 32 && p.tiles == (big + 1023) / 1024 && p.block_cap == 2 * big + 1024);
      q = bam_scan_launch(big, 36 * big, 65536, 4);
      CHECK(q.scan_blocks == 4 * 16 * 4 && q.fill_blocks == 128);
   }

   // ---- the stream's window arithmetic.  roff[k + 1]: the first read behind cluster k's end
   {
      const int64_t roff[] = {0, 4, 4, 9, 12};
      StreamDone d = stream_clusters_done(roff, 4, 12, false); // the last cluster's end has no read behind it yet
      CHECK(d.n_done == 3 && d.reads_done == 9);
      d = stream_clusters_done(roff, 4, 13, false);            // all complete: a read behind every end
      CHECK(d.n_done == 4 && d.reads_done == 12);
      d = stream_clusters_done(roff, 4, 4, false);             // none complete
      CHECK(d.n_done == 0 && d.reads_done == 0);
      d = stream_clusters_done(roff, 4, 12, true);             // nothing more will come: all, reads_done == n_reads
      CHECK(d.n_done == 4 && d.reads_done == 12);
      d = stream_clusters_done(roff, 4, 20, true);             // (the reads behind the last cluster are nobody's)
      CHECK(d.n_done == 4 && d.reads_done == 12);
      const int64_t none[] = {0, 0, 0};
      d = stream_clusters_done(none, 2, 0, true);              // last, with no reads
      CHECK(d.n_done == 2 && d.reads_done == 0);
      d = stream_clusters_done(none, 2, 0, false);
      CHECK(d.n_done == 0 && d.reads_done == 0);
      d = stream_clusters_done(none, 0, 7, false);             // no cluster left: every read is consumed
      CHECK(d.n_done == 0 && d.reads_done == 7);
      d = stream_clusters_done(none, 0, 7, true);
      CHECK(d.n_done == 0 && d.reads_done == 7);
      StreamCarry c = stream_carry(1000, 1000, 65536);         // nothing is carried
      CHECK(c.bytes == 0 && c.fits);
      c = stream_carry(100000, 100000 - 65536, 65536);         // exactly a chunk's capacity
      CHECK(c.bytes == 65536 && c.fits);
      c = stream_carry(100000, 100000 - 65537, 65536);         // one byte more
      CHECK(c.bytes == 65537 && !c.fits);
      c = stream_carry(65536, 0, 65536);                       // no record whole yet: the window's bytes wait
      CHECK(c.bytes == 65536 && c.fits);
      c = stream_carry(65537, 0, 65536);
      CHECK(!c.fits);
   }

   // ---- grow_capacity: max(want, cap + cap / 2); nothing to do where want <= cap
   CHECK(grow_capacity(0, 0) == 0 && grow_capacity(100, 100) == 100 && grow_capacity(7, 100) == 100);
   CHECK(grow_capacity(101, 100) == 150 && grow_capacity(150, 100) == 150 && grow_capacity(151, 100) == 151 && grow_capacity(8, 0) == 8 && grow_capacity(2, 1) == 2);
   CHECK(grow_capacity(((size_t)1 << 40) + 1, (size_t)1 << 40) == ((size_t)3 << 39));
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("front_schedule_cpp")
    src, exe = d / "front_schedule.cpp", d / "front_schedule"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_layouts_sort_keys_launches_and_window_arithmetic_match_their_restatements(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
