// strawberry_amd/csrc/front_schedule.h -- what the front end (records -> unique hits: bamdecode_api.hip, matepair_api.hip,
// collapse_api.hip, front_stream_api.hip) decides on the host, as data and free of HIP: a plain C++ compiler takes this header
// alone.  The arenas' layouts -- every zeroed range and every read-back word a named member --, the mate sort's key, the
// collapse's one sort or two, the decode kernels' staging buffers and grids, the stream's window arithmetic.  The launchers
// issue what these functions return and decide nothing of this themselves; tests/test_front_schedule_cpp.py states the rules a
// second time.
#pragma once

#include "stage_host.h"

namespace sb {

// what the kernel headers fix (each launcher asserts its own against the header's)
constexpr size_t kFlatRecBytes = 24;                         // sizeof(FlatRec), matepair_flat.h
constexpr int kFrontOneWaves = 4, kFrontOneTile = 64 * 4 * 4; // kOneWaves, kOneTile, bamdecode_device.h
constexpr int kFrontInlineBlocks = 3;                        // kBamInlineBlocks
constexpr int64_t kFrontCuLds = 160 * 1024;                  // a CU's LDS

// the smallest b >= 1 with 2^b >= n_loci: the bits of a cluster's number in a sort key
inline unsigned front_locus_bits(int64_t n_loci)
{
   unsigned b = 1;
   while (((int64_t)1 << b) < n_loci) ++b;
   return b;
}
// tiles of 64 entries: a wave's pass
inline size_t front_tiles64(size_t n) { return (n + 63) / 64; }
// the bits v needs (0 for 0)
inline unsigned front_bits_of(unsigned long long v)
{
   unsigned b = 0;
   while (b < 64 && (v >> b)) ++b;
   return b;
}

// ---- mate pairing (matepair_flat.h)

// The sorted form's key (flat_mate_keys_kernel): 32 bits = the number of a group of 2^group_shift neighbouring clusters, then a
// hash of (cluster, read id) of two bits more than the logarithm of the biggest group's record count; the smallest shift that fits.
struct MateSortKey {
   unsigned locus_bits, group_shift, hash_bits, sort_bits;
};
inline MateSortKey mate_sort_key(int64_t n_loci, const int64_t *locus_read_off)
{
   MateSortKey k = {front_locus_bits(n_loci), 0, 32, 32};
   k.group_shift = k.locus_bits;
   for (unsigned g = 0; g <= k.locus_bits; ++g) {
      int64_t biggest = 1;
      for (int64_t l = 0; l < n_loci; l += (int64_t)1 << g) biggest = std::max(biggest, locus_read_off[std::min<int64_t>(n_loci, l + ((int64_t)1 << g))] - locus_read_off[l]);
      unsigned hb = 2;
      while (((int64_t)1 << (hb - 2)) < biggest) ++hb;
      if (k.locus_bits - g + hb <= 32 || g == k.locus_bits) {
         k.hash_bits = std::min(32u, hb), k.group_shift = g;
         k.sort_bits = std::min(32u, k.locus_bits - g + k.hash_bits);
         break;
      }
   }
   return k;
}

// The scratch of one call.  Every member but the counts and *_bytes is an offset.
struct MateScratchLayout {
   size_t done_tiles, pair_tiles; // tiles of 64: over the n records (flat_mate_done_tiles_kernel), over the n + 1 entries of the
                                  // feature counts (flat_mate_count_kernel's waves).  The tile arrays have pair_tiles + 1 entries
   size_t roff, rarr, lefts, claim, slot, runlen, done, td, tda, prec, pval, lf, rf, tl, tr, ls, rs, poff, counts, tmp, bytes;
   size_t slot_bytes;               // zeroed in front of the positional form: [slot, slot + slot_bytes)
   size_t counts_bytes, trouble;    // zeroed per form: [counts, counts + counts_bytes) -- 64 slots of 64 bytes, then `trouble`
   size_t td_tail, tl_tail, tr_tail; // zeroed, 4 bytes each: the scans' entry beyond the last tile (td: beyond the last DONE tile)
   size_t ls_total, rs_total;       // read back, 8 bytes each: the scans' totals
};
inline MateScratchLayout mate_scratch_layout(int64_t n_reads, int64_t n_loci, size_t tmp_bytes)
{
   const size_t n = (size_t)n_reads, n1 = n + 1, nl1 = (size_t)n_loci + 1;
   Arena a;
   MateScratchLayout L;
   L.done_tiles = front_tiles64(n), L.pair_tiles = front_tiles64(n1);
   const size_t nt1 = L.pair_tiles + 1;
   L.roff = a.take_nonempty(nl1 * 8), L.rarr = a.take_nonempty(n * kFlatRecBytes), L.lefts = a.take_nonempty(n * 4), L.claim = a.take_nonempty(n * 4);
   L.slot = a.take_nonempty(n * 8), L.runlen = a.take_nonempty(n * 4);
   L.done = a.take_nonempty(n * 8), L.td = a.take_nonempty(nt1 * 4), L.tda = a.take_nonempty(nt1 * 8), L.prec = a.take_nonempty(n * 4), L.pval = a.take_nonempty(n * 4);
   L.lf = a.take_nonempty(n1 * 4), L.rf = a.take_nonempty(n1 * 4), L.tl = a.take_nonempty(nt1 * 4), L.tr = a.take_nonempty(nt1 * 4);
   L.ls = a.take_nonempty(nt1 * 8), L.rs = a.take_nonempty(nt1 * 8), L.poff = a.take_nonempty(nl1 * 8);
   L.counts_bytes = 64 * 64 + 256;
   L.counts = a.take_nonempty(L.counts_bytes), L.tmp = a.take_nonempty(tmp_bytes);
   L.bytes = a.size;
   L.slot_bytes = n * 8;
   L.trouble = L.counts + 64 * 64;
   L.td_tail = L.td + L.done_tiles * 4, L.tl_tail = L.tl + L.pair_tiles * 4, L.tr_tail = L.tr + L.pair_tiles * 4;
   L.ls_total = L.ls + L.pair_tiles * 8, L.rs_total = L.rs + L.pair_tiles * 8;
   return L;
}

// the sorted form's second block
struct MateSortedLayout {
   size_t key, skey, order, rec, state, stmp, bytes;
};
inline MateSortedLayout mate_sorted_layout(int64_t n_reads, size_t sort_tmp_bytes)
{
   const size_t n = (size_t)n_reads;
   Arena a;
   MateSortedLayout L;
   L.key = a.take_nonempty(n * 4), L.skey = a.take_nonempty(n * 4), L.order = a.take_nonempty(n * 4), L.rec = a.take_nonempty(n * kFlatRecBytes);
   L.state = a.take_nonempty(n), L.stmp = a.take_nonempty(sort_tmp_bytes);
   L.bytes = a.size;
   return L;
}

// the pairs' own arena (the handle keeps it)
struct MatePairsLayout {
   size_t mass, loff, roff, ll, lr, rl, rr, lc, rc, bytes;
};
inline MatePairsLayout mate_pairs_layout(int64_t n_pairs, int64_t n_lfeat, int64_t n_rfeat)
{
   const size_t np1 = (size_t)n_pairs + 1, nlf = (size_t)n_lfeat + 1, nrf = (size_t)n_rfeat + 1;
   Arena a;
   MatePairsLayout L;
   L.mass = a.take(np1 * 8), L.loff = a.take(np1 * 8), L.roff = a.take(np1 * 8);
   L.ll = a.take(nlf * 4), L.lr = a.take(nlf * 4), L.rl = a.take(nrf * 4), L.rr = a.take(nrf * 4);
   L.lc = a.take(nlf), L.rc = a.take(nrf);
   L.bytes = a.size;
   return L;
}

// ---- collapse (collapse_flat.h)

// The order of std::sort on (left end, right end), ties in input order.  ONE stable sort where the key fits 64 bits: a cluster's
// left ends relative to its leftmost, the clusters' ranges laid end to end (x_total: their sum), the pair's length below
// (max_span: the longest).  Otherwise -- or where the keys kernel saw pairs out of order (disorder), or the tests force it -- two
// sorts, least significant key first: by the right end (32 bits), then by (cluster << 32 | left end) (32 + locus_bits bits).
struct CollapseSortChoice {
   bool one_sort;
   unsigned span_bits, x_bits;
   unsigned end_bit; // the one sort's key width
};
inline CollapseSortChoice collapse_sort_choice(unsigned long long max_span, unsigned long long x_total, unsigned long long disorder, bool force_two_sorts)
{
   CollapseSortChoice c;
   c.span_bits = front_bits_of(max_span), c.x_bits = front_bits_of(x_total);
   c.one_sort = !force_two_sorts && !disorder && c.span_bits + c.x_bits <= 64;
   c.end_bit = std::max(1u, c.span_bits + c.x_bits);
   return c;
}

struct CollapseScratchLayout {
   size_t poff, kr, kr2, khi, sl, sr;
   size_t sum, sq, nm, clf, cm, sums_bytes; // the clusters' S1, S2, counts, flags, masses, zeroed together: [sum, sum + sums_bytes)
   size_t mean, sd;
   size_t perm1, key2, key2s, order, skip, head, kept, last, nfeat, ishit, gid, hrank, fbase, gmass, hoff;
   size_t minl, maxl, cspan, cbase, clof, ostat;
   size_t counts, flag, counters_bytes;     // the counters and the flags, zeroed together: [counts, counts + counters_bytes)
   size_t tmp, bytes;
   size_t gmass_bytes, cluster_words_bytes; // zeroed: gmass whole; minl (to 0xFF) and maxl, cluster_words_bytes each
   size_t ostat_bytes;                      // zeroed: ostat; its first 16 bytes are read back (the longest pair, the disorder count)
   size_t nfeat_tail, ishit_tail;           // zeroed, 4 bytes each: the entry beyond the last pair of the two scan inputs
   size_t x_total, n_feat;                  // read back, 8 bytes each: the scans' totals (cbase's, fbase's)
   size_t clf_words;                        // the cluster flags' 32-bit words (SBGPU_COLLAPSE_FORCE_SEQ sets them all)
};
inline CollapseScratchLayout collapse_scratch_layout(int64_t n_pairs, int64_t n_loci, size_t tmp_bytes)
{
   const size_t n = (size_t)n_pairs, n1 = n + 1, nl1 = (size_t)n_loci + 1;
   Arena a;
   CollapseScratchLayout L;
   L.poff = a.take_nonempty(nl1 * 8), L.kr = a.take_nonempty(n * 4), L.kr2 = a.take_nonempty(n * 4), L.khi = a.take_nonempty(n * 8);
   L.sl = a.take_nonempty(n * 4), L.sr = a.take_nonempty(n * 4);
   L.sum = a.take_nonempty(nl1 * 8), L.sq = a.take_nonempty(nl1 * 8), L.nm = a.take_nonempty(nl1 * 4), L.clf = a.take_nonempty(nl1 * 4), L.cm = a.take_nonempty(nl1 * 8);
   L.sums_bytes = a.size - L.sum;
   L.mean = a.take_nonempty(nl1 * 8), L.sd = a.take_nonempty(nl1 * 8);
   L.perm1 = a.take_nonempty(n * 4), L.key2 = a.take_nonempty(n * 8), L.key2s = a.take_nonempty(n * 8), L.order = a.take_nonempty(n * 4);
   L.skip = a.take_nonempty(n), L.head = a.take_nonempty(n), L.kept = a.take_nonempty(n * 4), L.last = a.take_nonempty(n * 4);
   L.nfeat = a.take_nonempty(n1 * 4), L.ishit = a.take_nonempty(n1 * 4);
   L.gid = a.take_nonempty(n * 4), L.hrank = a.take_nonempty(n1 * 8), L.fbase = a.take_nonempty(n1 * 8), L.gmass = a.take_nonempty(n1 * 8), L.hoff = a.take_nonempty(nl1 * 8);
   L.minl = a.take_nonempty(nl1 * 4), L.maxl = a.take_nonempty(nl1 * 4), L.cspan = a.take_nonempty(nl1 * 8), L.cbase = a.take_nonempty(nl1 * 8);
   L.clof = a.take_nonempty(n * 4), L.ostat = a.take_nonempty(64);
   L.counts = a.take_nonempty(64), L.flag = a.take_nonempty(64);
   L.counters_bytes = a.size - L.counts;
   L.tmp = a.take_nonempty(tmp_bytes);
   L.bytes = a.size;
   L.gmass_bytes = n1 * 8, L.cluster_words_bytes = nl1 * 4, L.ostat_bytes = 64, L.clf_words = nl1;
   L.nfeat_tail = L.nfeat + n * 4, L.ishit_tail = L.ishit + n * 4;
   L.x_total = L.cbase + (size_t)n_loci * 8, L.n_feat = L.fbase + n * 8;
   return L;
}

// the unique hits' own arena (sbgpu_hits_t layout + masses; the handle keeps it)
struct CollapseHitsLayout {
   size_t off, loc, mass, left, right, code, bytes;
};
inline CollapseHitsLayout collapse_hits_layout(int64_t n_hits, int64_t n_feat)
{
   const size_t nh1 = (size_t)n_hits + 1, nfe1 = (size_t)n_feat + 1;
   Arena a;
   CollapseHitsLayout L;
   L.off = a.take(nh1 * 8), L.loc = a.take(nh1 * 4), L.mass = a.take(nh1 * 4);
   L.left = a.take(nfe1 * 4), L.right = a.take(nfe1 * 4), L.code = a.take(nfe1);
   L.bytes = a.size;
   return L;
}

// ---- BAM decode (bamdecode_device.h)

// the handle's arrays inside one block of memory (host form: a vector; device form: an arena)
struct BamReadsLayout {
   size_t status, record, read_id, ref, nh, nm, read_len, left, right, partner_pos, sam_flag, flags, block_off, block_left, block_right, bytes;
};
inline BamReadsLayout bam_reads_layout(int64_t n_records, int64_t n_reads, int64_t n_blocks)
{
   const size_t n = (size_t)n_records, m = (size_t)n_reads, nb = (size_t)n_blocks;
   Arena a;
   BamReadsLayout L;
   L.status = a.take_nonempty(n);
   L.record = a.take_nonempty(m * 8), L.read_id = a.take_nonempty(m * 8);
   L.ref = a.take_nonempty(m * 4), L.nh = a.take_nonempty(m * 4), L.nm = a.take_nonempty(m * 4), L.read_len = a.take_nonempty(m * 4);
   L.left = a.take_nonempty(m * 4), L.right = a.take_nonempty(m * 4), L.partner_pos = a.take_nonempty(m * 4), L.sam_flag = a.take_nonempty(m * 4);
   L.flags = a.take_nonempty(m);
   L.block_off = a.take_nonempty((m + 1) * 8);
   L.block_left = a.take_nonempty(nb * 4), L.block_right = a.take_nonempty(nb * 4);
   L.bytes = a.size;
   return L;
}

// One pass (bam_onepass_kernel): the handle's arrays get room for EVERY record and block_cap blocks.  A wave's part of the
// staging buffer: 64 average records + 4 % + 512 bytes, in steps of 256, 4096 .. 32 KB, and no more than the device lets a
// workgroup ask for (a pass whose records do not fit walks them in global memory: slower, same results) -- three workgroups of
// four waves then fit a CU's 160 KB up to ~195 bytes per record.
struct BamOnepassLaunch {
   int64_t block_cap, tiles;
   int stage_bytes, resident; // per wave; workgroups a CU holds
   int64_t grid;
};
inline BamOnepassLaunch bam_onepass_launch(int64_t n, int64_t n_bytes, int lds_max, int n_cu)
{
   BamOnepassLaunch p;
   p.block_cap = 2 * n + 1024;
   p.tiles = (n + kFrontOneTile - 1) / kFrontOneTile;
   int stage = (int)std::min<int64_t>(std::max<int64_t>(4096, ((64 * (n_bytes / n + 1)) * 26 / 25 + 512 + 255) & ~(int64_t)255), 32 * 1024);
   p.stage_bytes = std::max(0, std::min(stage, (lds_max - 512) / kFrontOneWaves)) & ~255;
   p.resident = std::max(1, std::min(8, (int)(kFrontCuLds / ((int64_t)p.stage_bytes * kFrontOneWaves + 512))));
   p.grid = std::min<int64_t>(p.tiles, (int64_t)n_cu * p.resident);
   return p;
}
// its scratch: zeroed whole
struct BamOnepassScratch {
   size_t state, counts, ticket, bytes;
};
inline BamOnepassScratch bam_onepass_scratch(int64_t tiles)
{
   BamOnepassScratch L;
   L.state = 0, L.counts = up256((size_t)tiles * 8), L.ticket = L.counts + up256(16 * 8), L.bytes = L.ticket + 256;
   return L;
}

// Two passes: decide and count (bam_scan_kernel: a workgroup is one wave, 64 records), scans over the waves' totals, compact
// (bam_fill_kernel).  The scan's staging buffer: 1.1 x 64 average records, 8 .. 64 KB in steps of 2 KB, and what a workgroup
// may ask for less the kernel's static words.
struct BamScanLaunch {
   int stage_bytes, resident;
   int64_t scan_blocks, fill_blocks;
};
inline BamScanLaunch bam_scan_launch(int64_t n, int64_t n_bytes, int lds_max, int n_cu)
{
   BamScanLaunch p;
   int stage = 8 * 1024;
   while (stage < 64 * 1024 && (int64_t)stage < 70 * (n_bytes / n + 1)) stage += 2 * 1024;
   p.stage_bytes = std::max(0, std::min(stage, lds_max - 256));
   p.resident = std::max(1, std::min(16, (int)(kFrontCuLds / (p.stage_bytes + 256))));
   p.scan_blocks = std::min<int64_t>((n + 63) / 64, (int64_t)n_cu * p.resident * 4);
   p.fill_blocks = std::min<int64_t>((n + 255) / 256, (int64_t)n_cu * 32);
   return p;
}
struct BamScanScratch {
   size_t tiles; // of 64 records; the tile arrays have tiles + 1 entries
   size_t status, acc, nb, rid, ref, nh, nm, rl, left, right, pp, sf, fl, ib, tr, tb, rat, bat, cnt, tmp, bytes;
   size_t cnt_bytes;            // zeroed: [cnt, cnt + cnt_bytes)
   size_t tr_tail, tb_tail;     // zeroed, 4 bytes each: the scans' entry beyond the last tile
   size_t rat_total, bat_total; // read back, 8 bytes each: the accepted reads, their blocks
};
inline BamScanScratch bam_scan_scratch(int64_t n_records, size_t tmp_bytes)
{
   const size_t nn = (size_t)n_records, n1 = nn + 1;
   Arena a;
   BamScanScratch L;
   L.tiles = front_tiles64(nn);
   const size_t nt1 = L.tiles + 1;
   L.status = a.take_nonempty(nn), L.acc = a.take_nonempty(n1), L.nb = a.take_nonempty(n1 * 4), L.rid = a.take_nonempty(nn * 8);
   L.ref = a.take_nonempty(nn * 4), L.nh = a.take_nonempty(nn * 4), L.nm = a.take_nonempty(nn * 4), L.rl = a.take_nonempty(nn * 4);
   L.left = a.take_nonempty(nn * 4), L.right = a.take_nonempty(nn * 4), L.pp = a.take_nonempty(nn * 4), L.sf = a.take_nonempty(nn * 4);
   L.fl = a.take_nonempty(nn), L.ib = a.take_nonempty(nn * 4 * 2 * kFrontInlineBlocks);
   L.tr = a.take_nonempty(nt1 * 4), L.tb = a.take_nonempty(nt1 * 4), L.rat = a.take_nonempty(nt1 * 8), L.bat = a.take_nonempty(nt1 * 8);
   L.cnt_bytes = 16 * 8;
   L.cnt = a.take_nonempty(L.cnt_bytes), L.tmp = a.take_nonempty(tmp_bytes);
   L.bytes = a.size;
   L.tr_tail = L.tr + L.tiles * 4, L.tb_tail = L.tb + L.tiles * 4;
   L.rat_total = L.rat + L.tiles * 8, L.bat_total = L.bat + L.tiles * 8;
   return L;
}

// ---- the chunked stream (front_stream_api.hip)

// Which of the nc remaining clusters are complete: a read behind the cluster's end has been seen (roff[k + 1] < n_reads), or
// nothing more will come (last); reads_done: the reads they consume (all, where there is no cluster left)
struct StreamDone {
   int64_t n_done, reads_done;
};
inline StreamDone stream_clusters_done(const int64_t *roff, int64_t nc, int64_t n_reads, bool last)
{
   StreamDone d = {0, 0};
   if (last) d.n_done = nc;
   else
      while (d.n_done < nc && roff[d.n_done + 1] < n_reads) ++d.n_done;
   d.reads_done = nc > 0 ? roff[d.n_done] : n_reads;
   return d;
}
// What the next window carries: the bytes of the window [0, w_end) from c0 on; it must fit a chunk's capacity
struct StreamCarry {
   int64_t bytes;
   bool fits;
};
inline StreamCarry stream_carry(int64_t w_end, int64_t c0, int64_t chunk_cap)
{
   const int64_t cb = w_end - c0;
   return {cb, cb <= chunk_cap};
}
// a growing device array's next capacity (geometric)
inline size_t grow_capacity(size_t want, size_t cap) { return want <= cap ? cap : std::max(want, cap + cap / 2); }

} // namespace sb
