// strawberry_amd/csrc/stage_host.h -- what the retained-result stages (the `-f` table, the fragment assignment, the isoform
// coverage, the model fit, the isoform information, the body profile) share on the host, free of HIP: a plain C++ compiler takes this header alone.
//   - the limits of one locus and the work item of the hit kernels (one definition; the stages' headers alias them),
//   - the builder of the work items,
//   - the arena's layout: Arena::take, and each stage's offsets as one struct made by one function,
//   - the two loops the host forms share: the column pass (kept words, live flags, gains) and "which locus is this hit in".
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "assign_rules.h"

namespace sb {

constexpr int kStageMaxBins = 5632;   // bins of one locus whose per-bin arrays fit LDS (the device grouping stops at 5600: kBinsMaxBig)
constexpr int kStageMaxWords = 128;   // compat / kept words of one locus in LDS (4096 isoforms)
constexpr int kStageItemHits = 16384; // hits of one work item: a deeper locus is split

struct HitItem {
   int64_t h0, h1;  // hits [h0, h1) of the locus
   int32_t locus;
   int32_t split;   // 1: the locus has other items (global atomics), 0: this item owns its results (plain stores)
};

// A locus' hits in ranges of kStageItemHits, loci in ascending order.  row_off given: a locus without bins gets no item (the
// table counts hits per bin); null: it does (its hits are counted as unassigned / unexplained).
inline std::vector<HitItem> build_hit_items(const int64_t *locus_hit_off, int64_t n_loci, const int64_t *row_off)
{
   std::vector<HitItem> items;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t q0 = locus_hit_off[l], q1 = locus_hit_off[l + 1];
      if (row_off && row_off[l + 1] == row_off[l]) continue;
      const int32_t split = q1 - q0 > kStageItemHits;
      for (int64_t h = q0; h < q1; h += kStageItemHits) items.push_back({h, std::min<int64_t>(h + kStageItemHits, q1), (int32_t)l, split});
   }
   return items;
}

// One device block cut into arrays that begin at multiples of 256 bytes, in the order they are taken (csrc's one rounding and
// one arena helper: the chain's, the bootstrap's and the front end's layouts use them too)
inline size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct Arena {
   size_t size = 0;
   size_t take(size_t bytes)
   {
      const size_t at = size;
      size += up256(bytes);
      return at;
   }
   // an array that keeps a place of its own even when it is empty (the front end's arenas, the chain's uploads)
   size_t take_nonempty(size_t bytes) { return take(bytes ? bytes : 8); }
};
inline size_t at_least_1(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

// The stages' arenas.  Every member but the *_bytes is an offset; `upload_bytes` ends the part that one host block fills.
struct CtxLayout {
   size_t hoff, roff, ioff, foff, items, upload_bytes; // the four offset arrays, the items
   size_t nin, last;                                   // per-bin scratch
   size_t nrows, lhits, lroff, tot;                    // per-locus results, the row count
   size_t rbin, rhits, rlast, prob, bytes;             // rows
};
inline CtxLayout ctx_layout(int64_t n_loci, int64_t n_bins, int64_t n_elem, int64_t n_items)
{
   const size_t nl1 = (size_t)n_loci + 1, nb1 = at_least_1(n_bins);
   Arena a;
   CtxLayout L;
   L.hoff = a.take(nl1 * 8), L.roff = a.take(nl1 * 8), L.ioff = a.take(nl1 * 8), L.foff = a.take(nl1 * 8);
   L.items = a.take(at_least_1(n_items) * sizeof(HitItem));
   L.upload_bytes = a.size;
   L.nin = a.take(nb1 * 4), L.last = a.take(nb1 * 4);
   L.nrows = a.take(nl1 * 4), L.lhits = a.take(nl1 * 4), L.lroff = a.take(nl1 * 8), L.tot = a.take(256);
   L.rbin = a.take(nb1 * 8), L.rhits = a.take(nb1 * 4), L.rlast = a.take(nb1 * 8), L.prob = a.take(at_least_1(n_elem) * 8);
   L.bytes = a.size;
   return L;
}

struct AsgLayout {
   size_t hoff, roff, ioff, foff, items, upload_bytes; // the four offset arrays, the items
   size_t live, gain;
   size_t uniq, map, post, unas, sums_bytes;           // the sums, zeroed per call: [uniq, uniq + sums_bytes)
   size_t iso, cand, prob, bytes;                      // the per-hit results
};
inline AsgLayout asg_layout(int64_t n_loci, int64_t n_bins, int64_t n_iso, int64_t n_hits, int64_t n_items)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = at_least_1(n_iso), nh1 = at_least_1(n_hits);
   Arena a;
   AsgLayout L;
   L.hoff = a.take(nl1 * 8), L.roff = a.take(nl1 * 8), L.ioff = a.take(nl1 * 8), L.foff = a.take(nl1 * 8);
   L.items = a.take(at_least_1(n_items) * sizeof(HitItem));
   L.upload_bytes = a.size;
   L.live = a.take(at_least_1(n_bins)), L.gain = a.take(ni1 * 8);
   L.uniq = a.take(ni1 * 8), L.map = a.take(ni1 * 8), L.post = a.take(ni1 * 8), L.unas = a.take(nl1 * 8);
   L.sums_bytes = a.size - L.uniq;
   L.iso = a.take(nh1 * 4), L.cand = a.take(nh1 * 4), L.prob = a.take(nh1 * 8);
   L.bytes = a.size;
   return L;
}

struct CovLayout {
   size_t roff, ioff, foff, items, eoff, eleft, eright, upload_bytes; // the three offset arrays, the items, the exon arrays
   size_t live, gain;
   size_t bases, junc, unex, sums_bytes;                              // the sums, zeroed per call: [bases, bases + sums_bytes)
   size_t iso, bytes;
};
// upload_exons: the exon arrays travel with the offsets (false: the context holds the annotation pinned; they take no room)
inline CovLayout cov_layout(int64_t n_loci, int64_t n_bins, int64_t n_iso, int64_t n_exon, int64_t n_items, bool upload_exons)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = (size_t)n_iso + 1, ne1 = at_least_1(n_exon);
   Arena a;
   CovLayout L;
   L.roff = a.take(nl1 * 8), L.ioff = a.take(nl1 * 8), L.foff = a.take(nl1 * 8);
   L.items = a.take(at_least_1(n_items) * sizeof(HitItem));
   L.eoff = a.take(upload_exons ? ni1 * 8 : 0), L.eleft = a.take(upload_exons ? ne1 * 4 : 0), L.eright = a.take(upload_exons ? ne1 * 4 : 0);
   L.upload_bytes = a.size;
   L.live = a.take(at_least_1(n_bins)), L.gain = a.take(ni1 * 8);
   L.bases = a.take(ne1 * 8), L.junc = a.take(ne1 * 8), L.unex = a.take(nl1 * 8);
   L.sums_bytes = a.size - L.bases;
   L.iso = a.take(ni1 * 8);
   L.bytes = a.size;
   return L;
}

// The body profile.  epre: every exon's prefix length inside its isoform; ilen: every isoform's length; strand:
// one byte per isoform -- all three made on the host, once per call.
struct BodyLayout {
   size_t roff, ioff, foff, items, eoff, eleft, eright, epre, ilen, strand, upload_bytes;
   size_t live, gain;
   size_t bases, cprof, cn, sums_bytes; // the sums, zeroed per call: [bases, bases + sums_bytes)
   size_t total, center, cv, bytes;
};
inline BodyLayout body_layout(int64_t n_loci, int64_t n_bins, int64_t n_iso, int64_t n_exon, int64_t n_items, int n_pos, bool upload_exons)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = (size_t)n_iso + 1, ne1 = at_least_1(n_exon);
   Arena a;
   BodyLayout L;
   L.roff = a.take(nl1 * 8), L.ioff = a.take(nl1 * 8), L.foff = a.take(nl1 * 8);
   L.items = a.take(at_least_1(n_items) * sizeof(HitItem));
   L.eoff = a.take(upload_exons ? ni1 * 8 : 0), L.eleft = a.take(upload_exons ? ne1 * 4 : 0), L.eright = a.take(upload_exons ? ne1 * 4 : 0);
   L.epre = a.take(ne1 * 8), L.ilen = a.take(ni1 * 8), L.strand = a.take(ni1);
   L.upload_bytes = a.size;
   L.live = a.take(at_least_1(n_bins)), L.gain = a.take(ni1 * 8);
   L.bases = a.take(ni1 * (size_t)n_pos * 8), L.cprof = a.take(4 * (size_t)n_pos * 8), L.cn = a.take(4 * 8);
   L.sums_bytes = a.size - L.bases;
   L.total = a.take(ni1 * 8), L.center = a.take(ni1 * 8), L.cv = a.take(ni1 * 8);
   L.bytes = a.size;
   return L;
}

struct FitLayout {
   size_t small, large, upload_bytes; // the two lists of loci
   size_t keep, status;               // where the caller gave none
   size_t live, gain;
   size_t exp, res, score, ll, dev, pear, nlive, ndrop, nimp, dof, worst, bytes;
};
inline FitLayout fit_layout(int64_t n_loci, int64_t n_bins, int64_t n_iso, size_t n_small, size_t n_large, bool own_keep, bool own_status)
{
   const size_t nl1 = (size_t)n_loci + 1, nb1 = at_least_1(n_bins), ni1 = at_least_1(n_iso);
   Arena a;
   FitLayout L;
   L.small = a.take((n_small + 1) * 4), L.large = a.take((n_large + 1) * 4);
   L.upload_bytes = a.size;
   L.keep = a.take(own_keep ? ni1 * 4 : 0), L.status = a.take(own_status ? nl1 * 4 : 0);
   L.live = a.take(nb1), L.gain = a.take(ni1 * 8);
   L.exp = a.take(nb1 * 8), L.res = a.take(nb1 * 8), L.score = a.take(ni1 * 8);
   L.ll = a.take(nl1 * 8), L.dev = a.take(nl1 * 8), L.pear = a.take(nl1 * 8);
   L.nlive = a.take(nl1 * 8), L.ndrop = a.take(nl1 * 8), L.nimp = a.take(nl1 * 8);
   L.dof = a.take(nl1 * 4), L.worst = a.take(nl1 * 4);
   L.bytes = a.size;
   return L;
}

// The variational Bayes solve.  norm: the normalised weights of the loci too large for LDS, at the batch's own
// f_off (n_elem doubles where there is such a locus, none otherwise).
struct VbLayout {
   size_t small, large, upload_bytes; // the two lists of loci
   size_t norm;
   size_t count, share, sd, status, iters, elbo, nact, nfrag, bytes;
};
inline VbLayout vb_layout(int64_t n_loci, int64_t n_iso, int64_t n_norm, size_t n_small, size_t n_large)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = at_least_1(n_iso);
   Arena a;
   VbLayout L;
   L.small = a.take((n_small + 1) * 4), L.large = a.take((n_large + 1) * 4);
   L.upload_bytes = a.size;
   L.norm = a.take((size_t)n_norm * 8);
   L.count = a.take(ni1 * 8), L.share = a.take(ni1 * 8), L.sd = a.take(ni1 * 8);
   L.status = a.take(nl1 * 4), L.iters = a.take(nl1 * 4), L.elbo = a.take(nl1 * 8), L.nact = a.take(nl1 * 4), L.nfrag = a.take(nl1 * 8);
   L.bytes = a.size;
   return L;
}

struct InfoLayout {
   size_t small, large, covoff, upload_bytes; // the two lists of loci, the packed covariance's offsets
   size_t keep, status;                       // where the caller gave none
   size_t live, gain, w;
   size_t se, pcorr, ident, alias, partner, minpiv, rank, nfree, istatus;
   size_t cov, cov_bytes, bytes;              // zeroed per call: [cov, cov + cov_bytes)
};
inline InfoLayout info_layout(int64_t n_loci, int64_t n_bins, int64_t n_iso, int64_t n_cov, size_t n_small, size_t n_large, bool own_keep, bool own_status)
{
   const size_t nl1 = (size_t)n_loci + 1, nb1 = at_least_1(n_bins), ni1 = at_least_1(n_iso);
   Arena a;
   InfoLayout L;
   L.small = a.take((n_small + 1) * 4), L.large = a.take((n_large + 1) * 4), L.covoff = a.take(nl1 * 8);
   L.upload_bytes = a.size;
   L.keep = a.take(own_keep ? ni1 * 4 : 0), L.status = a.take(own_status ? nl1 * 4 : 0);
   L.live = a.take(nb1), L.gain = a.take(ni1 * 8), L.w = a.take(nb1 * 8);
   L.se = a.take(ni1 * 8), L.pcorr = a.take(ni1 * 8);
   L.ident = a.take(ni1 * 4), L.alias = a.take(ni1 * 4), L.partner = a.take(ni1 * 4);
   L.minpiv = a.take(nl1 * 8), L.rank = a.take(nl1 * 4), L.nfree = a.take(nl1 * 4), L.istatus = a.take(nl1 * 4);
   L.cov = a.take(at_least_1(n_cov) * 8);
   L.cov_bytes = a.size - L.cov;
   L.bytes = a.size;
   return L;
}

// The isoform support: the results of the whole batch and what the host makes of its shapes, then -- behind
// `chunk` -- the working set of one chunk of sub-problems, which every chunk of a call reuses.
struct LooLayout {
   size_t lstat, woff, rank, first, koff, kcol, upload_bytes; // made on the host: statuses, packed offsets, kept ranks and lists
   size_t lr, hgain, refit, nuniq, heir, stw, itw, supp;      // per isoform
   size_t llb, stb, itb;                                      // per locus
   size_t wo, chunk, bytes;
};
inline LooLayout loo_layout(int64_t n_loci, int64_t n_iso, int64_t n_kept, int64_t n_without, size_t chunk_bytes)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = (size_t)n_iso + 1;
   Arena a;
   LooLayout L;
   L.lstat = a.take(nl1 * 4), L.woff = a.take(ni1 * 8), L.rank = a.take(ni1 * 4), L.first = a.take(nl1 * 8), L.koff = a.take(nl1 * 8);
   L.kcol = a.take(at_least_1(n_kept) * 4);
   L.upload_bytes = a.size;
   L.lr = a.take(ni1 * 8), L.hgain = a.take(ni1 * 8), L.refit = a.take(ni1 * 8), L.nuniq = a.take(ni1 * 8);
   L.heir = a.take(ni1 * 4), L.stw = a.take(ni1 * 4), L.itw = a.take(ni1 * 4), L.supp = a.take(ni1 * 4);
   L.llb = a.take(nl1 * 8), L.stb = a.take(nl1 * 4), L.itb = a.take(nl1 * 4);
   L.wo = a.take(at_least_1(n_without) * 8);
   L.chunk = a.take(chunk_bytes);
   L.bytes = a.size;
   return L;
}
struct LooTile {
   int32_t locus, row0, rows, pad; // rows [row0, row0 + rows) of the locus
};
struct LooChunkLayout {
   size_t tiles, upload_bytes;
   size_t count, F, theta, status, iters, fit, bytes;
};
inline LooChunkLayout loo_chunk_layout(int64_t n_tiles, int64_t n_sub, int64_t sub_rows, int64_t sub_iso, int64_t sub_elem, size_t fit_bytes)
{
   Arena a;
   LooChunkLayout L;
   L.tiles = a.take(at_least_1(n_tiles) * sizeof(LooTile));
   L.upload_bytes = a.size;
   L.count = a.take(at_least_1(sub_rows) * 4), L.F = a.take(at_least_1(sub_elem) * 8), L.theta = a.take(at_least_1(sub_iso) * 8);
   L.status = a.take(at_least_1(n_sub) * 4), L.iters = a.take(at_least_1(n_sub) * 4);
   L.fit = a.take(fit_bytes);
   L.bytes = a.size;
   return L;
}

// The differential usage: as the isoform support's -- the whole call's results and what the host makes of its
// shapes, then, behind `chunk`, one chunk's working set.
struct DiffLayout {
   size_t lstat, rank, first, koff, kcol, upload_bytes;               // made on the host: statuses, kept ranks and lists
   size_t th_a, th_b, th_p, us_a, us_b, us_p, delta;                    // per isoform
   size_t lr, ll_a, ll_b, llx_a, llx_b, n_a, n_b, shift;                // per locus
   size_t dof, status, top, st_a, st_b, st_p, it_a, it_b, it_p;
   size_t sum_a, sum_b, sum_p;                                          // per locus: the statistics' first launch's notes for its second
   size_t chunk, bytes;
};
inline DiffLayout diff_layout(int64_t n_loci, int64_t n_iso, int64_t n_kept, size_t chunk_bytes)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = (size_t)n_iso + 1;
   Arena a;
   DiffLayout L;
   L.lstat = a.take(nl1 * 4), L.rank = a.take(ni1 * 4), L.first = a.take(nl1 * 8), L.koff = a.take(nl1 * 8), L.kcol = a.take(at_least_1(n_kept) * 4);
   L.upload_bytes = a.size;
   L.th_a = a.take(ni1 * 8), L.th_b = a.take(ni1 * 8), L.th_p = a.take(ni1 * 8), L.us_a = a.take(ni1 * 8), L.us_b = a.take(ni1 * 8);
   L.us_p = a.take(ni1 * 8), L.delta = a.take(ni1 * 8);
   L.lr = a.take(nl1 * 8), L.ll_a = a.take(nl1 * 8), L.ll_b = a.take(nl1 * 8), L.llx_a = a.take(nl1 * 8), L.llx_b = a.take(nl1 * 8);
   L.n_a = a.take(nl1 * 8), L.n_b = a.take(nl1 * 8), L.shift = a.take(nl1 * 8);
   L.dof = a.take(nl1 * 4), L.status = a.take(nl1 * 4), L.top = a.take(nl1 * 4), L.st_a = a.take(nl1 * 4), L.st_b = a.take(nl1 * 4);
   L.st_p = a.take(nl1 * 4), L.it_a = a.take(nl1 * 4), L.it_b = a.take(nl1 * 4), L.it_p = a.take(nl1 * 4);
   L.sum_a = a.take(nl1 * 8), L.sum_b = a.take(nl1 * 8), L.sum_p = a.take(nl1 * 8);
   L.chunk = a.take(chunk_bytes);
   L.bytes = a.size;
   return L;
}
struct DiffTile {
   int32_t locus, sample, row0, rows; // rows [row0, row0 + rows) of the locus in sample 0 (A) or 1 (B)
};
struct DiffScaleItem {
   int32_t first, n, lanes, rows; // loci list[first .. first + n) share a workgroup, `lanes` lanes each (0: one locus, all threads); rows: the most bins of one sample among them
};
struct DiffChunkLayout {
   size_t tiles, items, list, upload_bytes;
   size_t alpha, count, F, theta, status, iters, x_theta, x_status, fit, x_fit, bytes;
};
inline DiffChunkLayout diff_chunk_layout(int64_t n_tiles, int64_t n_items, int64_t n_list, int64_t n_kept, int64_t n_sub, int64_t sub_rows,
                                         int64_t sub_iso, int64_t sub_elem, size_t fit_bytes)
{
   Arena a;
   DiffChunkLayout L;
   L.tiles = a.take(at_least_1(n_tiles) * sizeof(DiffTile)), L.items = a.take(at_least_1(n_items) * sizeof(DiffScaleItem));
   L.list = a.take(at_least_1(n_list) * 4);
   L.upload_bytes = a.size;
   L.alpha = a.take(at_least_1(2 * n_kept) * 8);
   L.count = a.take(at_least_1(sub_rows) * 4), L.F = a.take(at_least_1(sub_elem) * 8), L.theta = a.take(at_least_1(sub_iso) * 8);
   L.status = a.take(at_least_1(n_sub) * 4), L.iters = a.take(at_least_1(n_sub) * 4);
   L.x_theta = a.take(at_least_1(sub_iso) * 8), L.x_status = a.take(at_least_1(n_sub) * 4);
   L.fit = a.take(fit_bytes), L.x_fit = a.take(fit_bytes);
   L.bytes = a.size;
   return L;
}

// The differential usage between two groups of replicates: as DiffLayout -- the whole call's results and what
// the host makes of its shapes, then, behind `chunk`, one chunk's working set.  A per-sample array is sample-major with a
// stride of exactly n_iso or n_loci (the caller's layout); S: the samples, slots = S + 3 (the samples, the two groups, ALL).
struct GdiffSample {
   const int64_t *row_off, *f_off; // one sample's arrays in HBM: the kernels index a device table of these by sample
   const int32_t *count;
   const double *F;
};
struct GdiffLayout {
   size_t lstat, p_a, p_b, rank, koff, kcol, slot, table, upload_bytes; // made on the host
   size_t th_s, th_g, th_all, us_s, us_g, us_all, delta;                // per isoform
   size_t lr_b, lr_w, ll_own, ll_grp, ll_all, n_frag, shift;            // per locus
   size_t dof_b, dof_w, status, top, st_s, it_s, st_g, it_g, st_all, it_all;
   size_t sum;                                                          // [slots x n_loci]: the statistics' first launch's notes for its second
   size_t chunk, bytes;
};
inline GdiffLayout gdiff_layout(int S, int64_t n_loci, int64_t n_iso, int64_t n_kept, size_t chunk_bytes)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = (size_t)n_iso + 1, s = (size_t)S, sl = s * (size_t)n_loci + 1, si = s * (size_t)n_iso + 1;
   Arena a;
   GdiffLayout L;
   L.lstat = a.take(nl1 * 4), L.p_a = a.take(nl1 * 4), L.p_b = a.take(nl1 * 4), L.rank = a.take(ni1 * 4), L.koff = a.take(nl1 * 8);
   L.kcol = a.take(at_least_1(n_kept) * 4), L.slot = a.take(((s + 3) * (size_t)n_loci + 1) * 8), L.table = a.take(s * sizeof(GdiffSample));
   L.upload_bytes = a.size;
   L.th_s = a.take(si * 8), L.th_g = a.take((2 * (size_t)n_iso + 1) * 8), L.th_all = a.take(ni1 * 8);
   L.us_s = a.take(si * 8), L.us_g = a.take((2 * (size_t)n_iso + 1) * 8), L.us_all = a.take(ni1 * 8), L.delta = a.take(ni1 * 8);
   L.lr_b = a.take(nl1 * 8), L.lr_w = a.take(nl1 * 8), L.ll_own = a.take(sl * 8), L.ll_grp = a.take(sl * 8), L.ll_all = a.take(sl * 8);
   L.n_frag = a.take(sl * 8), L.shift = a.take(nl1 * 8);
   L.dof_b = a.take(nl1 * 4), L.dof_w = a.take(nl1 * 4), L.status = a.take(nl1 * 4), L.top = a.take(nl1 * 4);
   L.st_s = a.take(sl * 4), L.it_s = a.take(sl * 4), L.st_g = a.take((2 * (size_t)n_loci + 1) * 4), L.it_g = a.take((2 * (size_t)n_loci + 1) * 4);
   L.st_all = a.take(nl1 * 4), L.it_all = a.take(nl1 * 4);
   L.sum = a.take(((s + 3) * (size_t)n_loci + 1) * 8);
   L.chunk = a.take(chunk_bytes);
   L.bytes = a.size;
   return L;
}
struct GdiffTile {
   int32_t locus, sample, row0, rows; // rows [row0, row0 + rows) of the locus in one sample
   int32_t own_q, grp_q, all_q;       // the chunk's sub-problems the rows go to; grp_q -1: the sample's group has none
   int32_t grp_row0, all_row0;        // the sample's first row inside the stacked sub-problems: the earlier present samples' bins
   int32_t pad[3];
};
struct GdiffScaleItem {
   int32_t first, n, lanes, rows; // as DiffScaleItem; rows: the most bins of one sample among the item's loci
   int32_t mask, pad[3];          // bit s: sample s is present at one of the item's loci
};
struct GdiffChunkLayout {
   size_t tiles, items, list, src_g, src_a, upload_bytes;
   size_t c, alpha_g, alpha_a, count, F, theta, status, iters, g_theta, g_status, a_theta, a_status, fit, g_fit, a_fit, bytes;
};
inline GdiffChunkLayout gdiff_chunk_layout(int S, int64_t n_tiles, int64_t n_items, int64_t n_list, int64_t n_kept, int64_t n_sub, int64_t sub_rows,
                                           int64_t sub_iso, int64_t sub_elem, size_t fit_bytes)
{
   Arena a;
   GdiffChunkLayout L;
   L.tiles = a.take(at_least_1(n_tiles) * sizeof(GdiffTile)), L.items = a.take(at_least_1(n_items) * sizeof(GdiffScaleItem));
   L.list = a.take(at_least_1(n_list) * 4), L.src_g = a.take(at_least_1(n_sub) * 4), L.src_a = a.take(at_least_1(n_sub) * 4);
   L.upload_bytes = a.size;
   L.c = a.take(at_least_1(S * n_kept) * 8), L.alpha_g = a.take(at_least_1(S * n_kept) * 8), L.alpha_a = a.take(at_least_1(S * n_kept) * 8);
   L.count = a.take(at_least_1(sub_rows) * 4), L.F = a.take(at_least_1(sub_elem) * 8), L.theta = a.take(at_least_1(sub_iso) * 8);
   L.status = a.take(at_least_1(n_sub) * 4), L.iters = a.take(at_least_1(n_sub) * 4);
   L.g_theta = a.take(at_least_1(sub_iso) * 8), L.g_status = a.take(at_least_1(n_sub) * 4);
   L.a_theta = a.take(at_least_1(sub_iso) * 8), L.a_status = a.take(at_least_1(n_sub) * 4);
   L.fit = a.take(fit_bytes), L.g_fit = a.take(fit_bytes), L.a_fit = a.take(fit_bytes);
   L.bytes = a.size;
   return L;
}

// The bin-table merge.  Its match works in a block of its own (the union's size is only known behind it, and a
// context's scratch slot loses its contents when it grows); the merged arrays, which outlive the call, are the slot's.
struct MergeItem {
   int32_t first, n, lanes, pad; // small form: loci list[first .. first + n) share a workgroup, `lanes` lanes each
};
struct MergeTile {
   int32_t locus, row0, rows, pad; // union rows [row0, row0 + rows) of the locus
};
struct MergeMatchLayout {
   size_t roff_a, roff_b, ioff, foff_a, foff_b, small, items, deep, upload_bytes; // the offsets, the two lists of loci, the small form's items
   size_t b_of_a, b_only, n_only, bytes;
};
inline MergeMatchLayout merge_match_layout(int64_t n_loci, int64_t n_bins_a, int64_t n_bins_b, size_t n_small, size_t n_items, size_t n_deep)
{
   const size_t nl1 = (size_t)n_loci + 1;
   Arena a;
   MergeMatchLayout L;
   L.roff_a = a.take(nl1 * 8), L.roff_b = a.take(nl1 * 8), L.ioff = a.take(nl1 * 8), L.foff_a = a.take(nl1 * 8), L.foff_b = a.take(nl1 * 8);
   L.small = a.take((n_small + 1) * 4), L.items = a.take((n_items + 1) * sizeof(MergeItem)), L.deep = a.take((n_deep + 1) * 4);
   L.upload_bytes = a.size;
   L.b_of_a = a.take(at_least_1(n_bins_a) * 4), L.b_only = a.take(at_least_1(n_bins_b) * 4), L.n_only = a.take(nl1 * 4);
   L.bytes = a.size;
   return L;
}
struct MergeLayout {
   size_t roff_u, foff_u, tiles, upload_bytes;
   size_t row_a, row_b, count_a, count_b, F_a, F_b, bytes;
};
inline MergeLayout merge_layout(int64_t n_loci, int64_t n_bins_u, int64_t n_elem_u, size_t n_tiles)
{
   const size_t nl1 = (size_t)n_loci + 1, nb1 = at_least_1(n_bins_u), ne1 = at_least_1(n_elem_u);
   Arena a;
   MergeLayout L;
   L.roff_u = a.take(nl1 * 8), L.foff_u = a.take(nl1 * 8), L.tiles = a.take((n_tiles + 1) * sizeof(MergeTile));
   L.upload_bytes = a.size;
   L.row_a = a.take(nb1 * 4), L.row_b = a.take(nb1 * 4), L.count_a = a.take(nb1 * 4), L.count_b = a.take(nb1 * 4);
   L.F_a = a.take(ne1 * 8), L.F_b = a.take(ne1 * 8);
   L.bytes = a.size;
   return L;
}

// ---- the host forms' shared loops.  Every sum runs in the order the kernels' do: a column's over the live bins, ascending.

// The kept words of one locus into K [(niso + 31) / 32] -> their number.  keep_of_locus null: no filter was given and every
// isoform is kept (`ones` is the caller's scratch for that); status null: every locus started.
inline int kept_words(const int32_t *keep_of_locus, int niso, const int32_t *status_of_locus, std::vector<int32_t> &ones, uint32_t *K)
{
   if (!keep_of_locus && (int)ones.size() < niso) ones.assign((size_t)niso, 1);
   const int words = (niso + 31) / 32;
   for (int w = 0; w < words; ++w) K[w] = ctx_kept_word(keep_of_locus ? keep_of_locus : ones.data(), niso, status_of_locus ? *status_of_locus : SBGPU_EM_OK, w);
   return words;
}

// One locus' column pass: live [nb], then per column the sum c_j over the live bins (kept where `c` is given) and the gain g_j.
// Fl: the locus' weights, row-major; K: its kept words.
inline void column_pass_locus(const double *Fl, int64_t nb, int niso, const double *theta_of_locus, const uint32_t *K, uint8_t *live, double *g, double *c)
{
   for (int64_t b = 0; b < nb; ++b) live[b] = asg_row_live(Fl + b * niso, niso);
   for (int j = 0; j < niso; ++j) {
      double cj = 0.0;
      for (int64_t b = 0; b < nb; ++b)
         if (live[b]) cj += Fl[b * niso + j];
      if (c) c[j] = cj;
      g[j] = asg_gain(theta_of_locus[j], cj, (K[j >> 5] >> (j & 31)) & 1u);
   }
}

// The column pass of a whole sample: what asg_column_kernel leaves, plus the kept words (locus l's begin at word_off[l])
struct ColumnPass {
   std::vector<int64_t> word_off; // [n_loci + 1]
   std::vector<uint32_t> kept;
   std::vector<uint8_t> live;     // [n_bins]
   std::vector<double> gain;      // [n_iso]
};
// -> false when a locus has more kept words than max_words (the hits' compat words do not cover it)
inline bool column_pass(int64_t n_loci, const int64_t *row_off, const int64_t *iso_off, const int64_t *f_off, const double *F, const double *theta,
                        const int32_t *keep, const int32_t *status, int max_words, ColumnPass *out)
{
   out->word_off.assign((size_t)n_loci + 1, 0);
   for (int64_t l = 0; l < n_loci; ++l) out->word_off[(size_t)l + 1] = out->word_off[(size_t)l] + (iso_off[l + 1] - iso_off[l] + 31) / 32;
   out->kept.assign((size_t)out->word_off[(size_t)n_loci] + 1, 0u);
   out->live.assign((size_t)row_off[n_loci] + 1, 0);
   out->gain.assign((size_t)iso_off[n_loci] + 1, 0.0);
   std::vector<int32_t> ones;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t i0 = iso_off[l], b0 = row_off[l];
      const int niso = (int)(iso_off[l + 1] - i0);
      if ((niso + 31) / 32 > max_words) return false;
      uint32_t *K = out->kept.data() + out->word_off[(size_t)l];
      kept_words(keep ? keep + i0 : nullptr, niso, status ? status + l : nullptr, ones, K);
      column_pass_locus(F + f_off[l], row_off[l + 1] - b0, niso, theta + i0, K, out->live.data() + b0, out->gain.data() + i0, nullptr);
   }
   return true;
}

// Which locus hit h is in, given its bin b (< 0: none) and the answer for the hit before, l: the bin's locus, or -- a hit
// without a bin says nothing of its locus -- the hits' grouping's.  -1: no bin and no grouping (locus_hit_off null).
inline int64_t locus_of_hit(int64_t h, int64_t b, int64_t l, int64_t n_loci, const int64_t *row_off, const int64_t *locus_hit_off)
{
   const int64_t *off = b >= 0 ? row_off : locus_hit_off;
   const int64_t x = b >= 0 ? b : h;
   if (!off) return -1;
   return x < off[l] || x >= off[l + 1] ? std::upper_bound(off, off + n_loci + 1, x) - off - 1 : l;
}

} // namespace sb
