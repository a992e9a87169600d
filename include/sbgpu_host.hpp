/*
 * include/sbgpu_host.hpp -- the host side above the C ABI, in the reference's own language.
 *
 * ruolin/strawberry is C++14; this header (C++14, header-only, depends only on sbgpu.h) is what
 * its driver would include.  It mirrors the reference's call surface for the path:
 *
 *   sbgpu::EmSolver            include/estimate.hpp:230-257  (init / run / _theta), one locus
 *   sbgpu::EmBatch             the same for many loci in ONE device call: collect -> solve
 *   sbgpu::LocusBatch          LocusContext's constructor + estimate_abundances for many loci
 *                              (include/estimate.hpp:60-103, src/estimate.cpp:279-355):
 *                              fragments -> exon bins -> bin weights -> EM -> FPKM / Frac
 *   sbgpu::finalize_tpm        Sample::procSample's tail, src/alignments.cpp:1821-1829
 *
 * Every number comes from libsbgpu.so (HIP kernels); the only arithmetic here is the reference's
 * own host epilogue (theta -> FPKM / Frac / TPM, a dozen flops per isoform), kept as host code on
 * purpose: INTEGRATION.md section 2.  Errors are exceptions carrying sbgpu_last_error().
 */
#ifndef SBGPU_HOST_HPP_
#define SBGPU_HOST_HPP_

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <stdexcept>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "sbgpu.h"

namespace sbgpu {

struct Error : std::runtime_error {
   int code;
   Error(int c, const std::string &what) : std::runtime_error(what + ": " + sbgpu_last_error()), code(c) {}
};
inline void check(int rc, const char *what)
{
   if (rc < 0) throw Error(rc, what);
}

/* One per process and GPU. */
class Context {
   sbgpu_ctx_t *h_ = nullptr;

public:
   explicit Context(int device = 0) { check(sbgpu_init(device, &h_), "sbgpu_init"); }
   ~Context()
   {
      if (h_) sbgpu_finalize(h_);
   }
   Context(const Context &) = delete;
   Context &operator=(const Context &) = delete;
   sbgpu_ctx_t *get() const { return h_; }
};

/* Many loci, one solve.  add() takes exactly EmSolver::init's arguments. */
class EmBatch {
public:
   std::vector<int64_t> row_off{0}, iso_off{0}, f_off{0};
   std::vector<int32_t> count;
   std::vector<double> F;
   std::vector<double> theta;   /* after solve(): em._theta of every locus, concatenated */
   std::vector<int32_t> status; /* SBGPU_EM_* per locus                                   */
   std::vector<int32_t> iters;

   int64_t size() const { return (int64_t)row_off.size() - 1; }

   int64_t add(int num_iso, const std::vector<int> &n, const std::vector<std::vector<double>> &alpha)
   {
      for (size_t i = 0; i < n.size(); ++i) {
         count.push_back(n[i]);
         for (int j = 0; j < num_iso; ++j) F.push_back(alpha[i][(size_t)j]);
      }
      row_off.push_back((int64_t)count.size());
      iso_off.push_back(iso_off.back() + num_iso);
      f_off.push_back((int64_t)F.size());
      return size() - 1;
   }

   void solve(const Context &ctx)
   {
      const int64_t n = size();
      theta.assign((size_t)iso_off.back() + 1, 0.0);
      status.assign((size_t)n + 1, 0);
      iters.assign((size_t)n + 1, 0);
      sbgpu_batch_t b = {n, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()};
      check(sbgpu_em_batch(ctx.get(), &b, theta.data(), status.data(), iters.data()), "sbgpu_em_batch");
   }
   /* the two bools of the reference, src/estimate.cpp:307-308 */
   bool init_ok(int64_t l) const { return status[(size_t)l] != SBGPU_EM_INIT_EMPTY; }
   bool run_ok(int64_t l) const { return status[(size_t)l] == SBGPU_EM_OK || status[(size_t)l] == SBGPU_EM_MAXITER; }

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
   /* The EM bootstrap of the batch (sbgpu_em_bootstrap_device): replicates rep_first .. rep_first + n_rep - 1 under `seed`.
    * The C ABI's bootstrap works on device arrays, and this header allocates nothing on the device by itself: the member
    * exists for a translation unit that included <hip/hip_runtime_api.h> before this header (and links the HIP runtime).
    * locus_id: the loci's global ids (size() entries), or empty: their index in the batch.                           */
   struct Bootstrap {
      std::vector<double> mean, var;     /* per isoform */
      std::vector<int32_t> status_count; /* [size()][4]: replicates per SBGPU_EM_* status */
   };
   Bootstrap bootstrap(const Context &ctx, int n_rep, uint64_t seed, int rep_first = 0, const std::vector<int64_t> &locus_id = {}) const
   {
      const int64_t n = size();
      const size_t n_iso = (size_t)iso_off.back();
      if (!locus_id.empty() && (int64_t)locus_id.size() != n) throw std::invalid_argument("EmBatch::bootstrap: one id per locus");
      Bootstrap out;
      out.mean.assign(n_iso, 0.0), out.var.assign(n_iso, 0.0), out.status_count.assign((size_t)n * 4, 0);
      if (n == 0) return out;
      struct Dev { /* frees on every way out */
         void *p = nullptr;
         ~Dev() { if (p) (void)hipFree(p); }
         void up(const void *src, size_t bytes, const char *what)
         {
            if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess || (bytes && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess))
               throw std::runtime_error(std::string("EmBatch::bootstrap: ") + what);
         }
      } d_count, d_F;
      d_count.up(count.data(), count.size() * sizeof(int32_t), "count");
      d_F.up(F.data(), F.size() * sizeof(double), "F");
      Dev d_m, d_v, d_s;
      d_m.up(out.mean.data(), n_iso * sizeof(double), "mean");
      d_v.up(out.var.data(), n_iso * sizeof(double), "var");
      d_s.up(out.status_count.data(), out.status_count.size() * sizeof(int32_t), "status counts");
      sbgpu_plan_t *plan = nullptr;
      check(sbgpu_plan_create(ctx.get(), n, row_off.data(), iso_off.data(), f_off.data(), &plan), "sbgpu_plan_create");
      const sbgpu_bootstrap_params_t par = {n_rep, rep_first, seed, locus_id.empty() ? nullptr : locus_id.data()};
      int rc = sbgpu_em_bootstrap_device(ctx.get(), plan, (const int32_t *)d_count.p, (const double *)d_F.p, &par, (double *)d_m.p, (double *)d_v.p,
                                         (int32_t *)d_s.p, nullptr, nullptr, nullptr, nullptr);
      if (rc == SBGPU_OK) rc = sbgpu_synchronize(ctx.get(), nullptr);
      const bool copied = rc != SBGPU_OK || (hipMemcpy(out.mean.data(), d_m.p, n_iso * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                                             hipMemcpy(out.var.data(), d_v.p, n_iso * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                                             hipMemcpy(out.status_count.data(), d_s.p, out.status_count.size() * sizeof(int32_t),
                                                       hipMemcpyDeviceToHost) == hipSuccess);
      sbgpu_plan_destroy(plan);
      check(rc, "sbgpu_em_bootstrap_device");
      if (!copied) throw std::runtime_error("EmBatch::bootstrap: the results could not be copied back");
      return out;
   }
#endif
};

/* include/estimate.hpp:230-257 for a single locus (tests; a caller with one locus at hand).
 * The device call happens in init(): it returns the reference's bool, _theta holds theta_0 until
 * run() -- which returns the reference's second bool -- installs the solution.               */
class EmSolver {
   const Context &ctx_;
   std::vector<double> solved_;
   int32_t status_ = SBGPU_EM_INIT_EMPTY;

public:
   std::vector<double> _theta;
   explicit EmSolver(const Context &ctx) : ctx_(ctx) {}
   bool init(const int num_iso, const std::vector<int> &count, const std::vector<std::vector<double>> &model)
   {
      EmBatch b;
      b.add(num_iso, count, model);
      b.solve(ctx_);
      status_ = b.status[0];
      solved_.assign(b.theta.begin(), b.theta.begin() + num_iso);
      double total = 0.0;
      for (int c : count) total += (double)c;
      _theta.assign((size_t)num_iso, total / num_iso); /* src/estimate.cpp:374-375 */
      return status_ != SBGPU_EM_INIT_EMPTY;
   }
   bool run()
   {
      if (status_ == SBGPU_EM_INIT_EMPTY || status_ == SBGPU_EM_DENOM_ZERO) return false; /* theta_0 stays */
      _theta = solved_;
      return true;
   }
};

struct InsertSize { /* include/read.hpp:176-192 */
   double mean = 200.0, sd = 80.0;
   bool use_emp = false;
   int start_offset = 0, end_offset = 0, total_reads = 0;
   std::vector<double> emp_dist;
   InsertSize() = default;
   InsertSize(double m, double s) : mean(m), sd(s) {}
   /* InsertSize(const vector<int> frag_lens), src/read.cpp:238-262 (+ mean_and_sd_insert_size, :14-20) */
   explicit InsertSize(const std::vector<int> &frag_lens) : use_emp(true)
   {
      total_reads = (int)frag_lens.size();
      if (total_reads < 1) throw std::runtime_error("Not enough reads");
      double sum = 0.0, sq = 0.0;
      int lo = frag_lens[0], hi = frag_lens[0];
      for (int v : frag_lens) {
         sum += v;
         lo = v < lo ? v : lo;
         hi = v > hi ? v : hi;
      }
      for (int v : frag_lens) sq += (double)v * v;
      mean = sum / frag_lens.size();
      sd = std::sqrt(sq / frag_lens.size() - mean * mean);
      start_offset = lo;
      end_offset = hi;
      emp_dist.assign((size_t)(hi - lo + 1), 0.0);
      for (int v : frag_lens) emp_dist[(size_t)(v - lo)] += 1.0;
   }
};

struct Isoform { /* what the epilogue fills: include/isoform.h:40-58 */
   int length = 0;
   double theta = 0.0, FPKM = 0.0, frac = 0.0, TPM = 0.0;
   std::string FPKM_s = "nan", frac_s = "nan", TPM_s = "nan";
   bool kept = true;
};

/* Fragments of many loci -> abundances.  Fill with add_locus / add_hit in the reference's order
 * (isoforms as LocusContext::_transcripts, hits as HitCluster::uniq_hits()), then quantify().   */
class LocusBatch {
public:
   /* annotation */
   std::vector<int64_t> iso_off{0}, exon_off{0}, seg_off;
   std::vector<uint32_t> exon_left, exon_right, seg_left, seg_right;
   /* hits */
   std::vector<int32_t> hit_locus;
   std::vector<int64_t> feat_off{0};
   std::vector<uint8_t> feat_code;
   std::vector<uint32_t> feat_left, feat_right;
   std::vector<float> hit_mass;
   /* results */
   std::vector<int64_t> row_off, f_off, hit_bin;
   /* keep_handle: quantify() leaves its handle in bins_handle (hit -> bin, F: what ContextTable::host reads) and does not destroy it */
   bool keep_handle = false;
   std::shared_ptr<sbgpu_bins_t> bins_handle;
   std::vector<int32_t> count, status, iters;
   std::vector<uint32_t> compat, key, bin_key;
   std::vector<double> F, theta;
   std::vector<Isoform> isoforms; /* all loci, concatenated like iso_off */
   int32_t compat_words = 1, key_words = 1;

   int64_t n_loci() const { return (int64_t)iso_off.size() - 1; }
   int64_t n_hits() const { return (int64_t)hit_locus.size(); }

   /* exons: the S_MATCH features of each transcript's Contig::_genomic_feats, closed coordinates */
   int64_t add_locus(const std::vector<std::vector<std::pair<uint32_t, uint32_t>>> &transcripts)
   {
      for (const auto &t : transcripts) {
         for (const auto &e : t) {
            exon_left.push_back(e.first);
            exon_right.push_back(e.second);
         }
         exon_off.push_back((int64_t)exon_left.size());
      }
      iso_off.push_back((int64_t)exon_off.size() - 1);
      return n_loci() - 1;
   }
   /* one unique hit: its Contig features (code 0 MATCH / 1 INTRON / 2 GAP) and (float) collapse mass */
   void add_hit(int32_t locus, int n_feat, const uint8_t *code, const uint32_t *left, const uint32_t *right, float mass)
   {
      hit_locus.push_back(locus);
      feat_code.insert(feat_code.end(), code, code + n_feat);
      feat_left.insert(feat_left.end(), left, left + n_feat);
      feat_right.insert(feat_right.end(), right, right + n_feat);
      feat_off.push_back((int64_t)feat_code.size());
      hit_mass.push_back(mass);
   }
   /* a read pair given by its mates' features: Contig(PairedHit), src/contig.cpp:216-267.
    * Returns false when the reference rejects the pair (it then only counts towards the mapped total). */
   bool add_pair(int32_t locus, const std::vector<uint8_t> &lc, const std::vector<uint32_t> &ll, const std::vector<uint32_t> &lr,
                 const std::vector<uint8_t> &rc, const std::vector<uint32_t> &rl, const std::vector<uint32_t> &rr, float mass)
   {
      const size_t cap = lc.size() + rc.size() + 1;
      std::vector<uint8_t> c(cap);
      std::vector<uint32_t> l(cap), r(cap);
      const int n = sbgpu_hit_features((int)lc.size(), lc.data(), ll.data(), lr.data(), (int)rc.size(), rc.data(), rl.data(),
                                       rr.data(), c.data(), l.data(), r.data());
      check(n, "sbgpu_hit_features");
      if (n == 0) return false;
      add_hit(locus, n, c.data(), l.data(), r.data(), mass);
      return true;
   }

   /* All aligned read pairs of the batch at once: HitCluster::collapseAndFilterHits + Contig(PairedHit)
    * (sbgpu_collapse_pairs_host).  Replaces the hits added so far; returns the reference's
    * _total_mapped_reads (sum over loci of the int-truncated cluster mass, src/alignments.cpp:1372).   */
   int set_hits_from_pairs(const sbgpu_pairs_t &pairs)
   {
      sbgpu_uniq_t *u = nullptr;
      check(sbgpu_collapse_pairs_host(n_loci(), &pairs, &u), "sbgpu_collapse_pairs_host");
      int64_t info[8];
      sbgpu_uniq_info(u, info);
      hit_locus.assign((size_t)info[0], 0);
      feat_off.assign((size_t)info[0] + 1, 0);
      feat_code.assign((size_t)info[1], 0);
      feat_left.assign((size_t)info[1], 0);
      feat_right.assign((size_t)info[1], 0);
      hit_mass.assign((size_t)info[0], 0.0f);
      const int rc = sbgpu_uniq_export(u, hit_locus.data(), feat_off.data(), feat_code.data(), feat_left.data(), feat_right.data(),
                                       hit_mass.data(), nullptr);
      sbgpu_uniq_destroy(u);
      check(rc, "sbgpu_uniq_export");
      return (int)info[4];
   }

   sbgpu_annotation_t annotation() const
   {
      sbgpu_annotation_t a = {n_loci(), iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(),
                              seg_off.data(), seg_left.data(), seg_right.data()};
      return a;
   }
   sbgpu_hits_t hits() const
   {
      sbgpu_hits_t h = {n_hits(), hit_locus.data(), feat_off.data(), feat_code.data(), feat_left.data(), feat_right.data()};
      return h;
   }

   InsertSize insert; /* the distribution quantify() used (the empirical one when it was asked to build it) */

   /* LocusContext ctor + estimate_abundances for every locus.  total_mapped_reads, min_isoform_frac
    * etc. are the globals the reference reads (sbgpu_abundance_params_t).  ins_in == nullptr: no -i was
    * given, the empirical insert-size distribution is built from the hits first (Sample::fragLenDist,
    * src/alignments.cpp:1363-1407 + Strawberry.cpp:345-355).                                       */
   void quantify(const Context &ctx, const InsertSize *ins_in, int read_len, const sbgpu_abundance_params_t &par,
                 bool long_read = false)
   {
      const int64_t nl = n_loci();
      /* _exon_segs, include/estimate.hpp:80-91 */
      seg_off.assign((size_t)nl + 1, 0);
      int64_t ns = sbgpu_segments_host(nl, iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(), seg_off.data(),
                                       nullptr, nullptr, 0);
      check((int)(ns < 0 ? ns : 0), "sbgpu_segments_host");
      seg_left.assign((size_t)ns + 1, 0);
      seg_right.assign((size_t)ns + 1, 0);
      sbgpu_segments_host(nl, iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(), seg_off.data(),
                          seg_left.data(), seg_right.data(), ns);
      int64_t max_iso = 1, max_seg = 1;
      for (int64_t l = 0; l < nl; ++l) {
         max_iso = std::max(max_iso, iso_off[(size_t)l + 1] - iso_off[(size_t)l]);
         max_seg = std::max(max_seg, seg_off[(size_t)l + 1] - seg_off[(size_t)l]);
      }
      compat_words = (int32_t)((max_iso + 31) / 32);
      key_words = (int32_t)((max_seg + 31) / 32);
      /* assign_exon_bin + set_theory_bin_weight + EmSolver for all loci: one call, everything between the
       * hits and theta stays on the device (sbgpu_quantify_host) */
      const int64_t nh = n_hits();
      const int64_t n_iso = iso_off[(size_t)nl];
      compat.assign((size_t)nh * compat_words + 1, 0);
      theta.assign((size_t)n_iso + 1, 0.0);
      status.assign((size_t)nl + 1, 0);
      iters.assign((size_t)nl + 1, 0);
      sbgpu_annotation_t an = annotation();
      sbgpu_hits_t ht = hits();
      sbgpu_insert_t si, used;
      if (ins_in) {
         insert = *ins_in;
         si.mean = insert.mean;
         si.sd = insert.sd;
         si.use_emp = insert.use_emp;
         si.start_offset = insert.start_offset;
         si.end_offset = insert.end_offset;
         si.total_reads = insert.total_reads;
         si.emp_hist = insert.emp_dist.empty() ? nullptr : insert.emp_dist.data();
         si.read_len = read_len;
         si.long_read = long_read;
      }
      sbgpu_bins_t *bins = nullptr;
      check(sbgpu_quantify_host(ctx.get(), &an, &ht, hit_mass.data(), ins_in ? &si : nullptr, read_len, long_read, theta.data(),
                                status.data(), iters.data(), compat.data(), &used, &bins),
            "sbgpu_quantify_host");
      if (!ins_in) { /* the empirical law the library built (Sample::fragLenDist + InsertSize(frag_lens)) */
         insert = InsertSize();
         insert.mean = used.mean;
         insert.sd = used.sd;
         insert.use_emp = true;
         insert.start_offset = used.start_offset;
         insert.end_offset = used.end_offset;
         insert.total_reads = used.total_reads;
         insert.emp_dist.assign(used.emp_hist, used.emp_hist + (used.end_offset - used.start_offset + 1));
      }
      int64_t info[8];
      sbgpu_bins_info(bins, info);
      const int64_t n_bins = info[2], n_elem = info[3];
      row_off.assign((size_t)nl + 1, 0);
      f_off.assign((size_t)nl + 1, 0);
      count.assign((size_t)n_bins + 1, 0);
      std::vector<int32_t> iso_len((size_t)n_iso + 1, 0);
      bin_key.assign((size_t)n_bins * key_words + 1, 0);
      hit_bin.assign((size_t)nh + 1, -1);
      F.assign((size_t)n_elem + 1, 0.0);
      int rc = sbgpu_bins_export(bins, row_off.data(), nullptr, f_off.data(), count.data(), iso_len.data(), bin_key.data(), nullptr,
                                 hit_bin.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
      if (rc == SBGPU_OK) rc = sbgpu_bins_export_weights(bins, F.data());
      bins_handle.reset(bins, sbgpu_bins_destroy);
      if (!keep_handle) bins_handle.reset();
      check(rc, "sbgpu_bins_export");
      /* the reference's own epilogue, src/estimate.cpp:310-355 */
      isoforms.assign((size_t)n_iso, Isoform());
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t j0 = iso_off[(size_t)l], j1 = iso_off[(size_t)l + 1];
         for (int64_t j = j0; j < j1; ++j) isoforms[(size_t)j].length = iso_len[(size_t)j];
         if (status[(size_t)l] == SBGPU_EM_INIT_EMPTY) { /* estimate_abundances() == false: the locus is dropped */
            for (int64_t j = j0; j < j1; ++j) isoforms[(size_t)j].kept = false;
            continue;
         }
         double sum_fpkm = 0.0;
         for (int64_t j = j0; j < j1; ++j) {
            Isoform &t = isoforms[(size_t)j];
            t.theta = theta[(size_t)j];
            double kb;
            if (par.effective_len_norm) {
               kb = t.length - par.insert_mean;
               if (kb < 0) {
                  t.FPKM_s = "NA";
                  continue;
               }
               kb = 1e3 / kb;
            } else {
               kb = 1e3 / t.length;
            }
            const double rpm = 1e6 / par.total_mapped_reads;
            t.FPKM = t.theta * rpm * kb;
            sum_fpkm += t.FPKM;
            t.FPKM_s = std::to_string(t.FPKM);
         }
         for (int64_t j = j0; j < j1; ++j) {
            Isoform &t = isoforms[(size_t)j];
            if (t.FPKM_s == "NA") {
               t.frac_s = "NA";
               continue;
            }
            t.frac = t.FPKM / sum_fpkm;
            t.frac_s = std::to_string(t.frac);
         }
         if (par.filter_by_expression)
            for (int64_t j = j0; j < j1; ++j)
               if (isoforms[(size_t)j].frac < par.min_isoform_frac) isoforms[(size_t)j].kept = false;
      }
   }
};

/* The collective of a multi-GPU run (one process per GPU, loci sharded over the ranks): the two cross-locus
 * sums of the reference, `_total_mapped_reads` (src/alignments.cpp:1372) and the FPKM total (:1821-1824).
 * Rank 0 makes the RCCL id and leaves it in `id_file` (written under a temporary name and renamed, so a reader
 * never sees half of it); the other ranks wait for the file.  world == 1 needs no file and no RCCL.
 * A file left behind by an earlier launch must not be taken for this one's: the file starts with `nonce` -- a value
 * the launcher gives to ALL ranks of one launch (job id, start time; `--comm-nonce` of examples/quantify_fragments) --
 * and readers wait for a file that carries theirs; rank 0 also removes a stale file before it writes and removes its
 * own once every rank has joined (sbgpu_comm_init is collective: it returns when all have read the id).  With the
 * default nonce 0 the path must not exist when the launch begins.                                              */
class Comm {
 public:
   Comm(const Context &ctx, int rank, int world, const std::string &id_file = std::string(), uint64_t nonce = 0) : h_(nullptr)
   {
      uint8_t id[SBGPU_COMM_ID_BYTES] = {0};
      if (world > 1) {
         if (id_file.empty()) throw Error(SBGPU_EINVAL, "sbgpu::Comm: a world of several ranks needs an id file");
         if (rank == 0) {
            std::remove(id_file.c_str()); /* whatever an earlier launch left */
            check(sbgpu_comm_unique_id(id), "sbgpu_comm_unique_id");
            const std::string tmp = id_file + ".tmp";
            FILE *f = std::fopen(tmp.c_str(), "wb");
            if (!f || std::fwrite(&nonce, 1, sizeof(nonce), f) != sizeof(nonce) || std::fwrite(id, 1, sizeof(id), f) != sizeof(id) ||
                std::fclose(f) != 0 || std::rename(tmp.c_str(), id_file.c_str()) != 0)
               throw Error(SBGPU_EINVAL, "sbgpu::Comm: cannot write " + id_file);
         } else {
            for (int tries = 0;; ++tries) {
               FILE *f = std::fopen(id_file.c_str(), "rb");
               if (f) {
                  uint64_t theirs = 0;
                  const size_t n0 = std::fread(&theirs, 1, sizeof(theirs), f);
                  const size_t n = std::fread(id, 1, sizeof(id), f);
                  std::fclose(f);
                  if (n0 == sizeof(theirs) && n == sizeof(id) && theirs == nonce) break; /* (another launch's file: keep waiting) */
               }
               if (tries > 6000) throw Error(SBGPU_ERCCL, "sbgpu::Comm: no id of this launch in " + id_file + " after 60 s");
               struct timespec ts = {0, 10 * 1000 * 1000};
               nanosleep(&ts, nullptr);
            }
         }
      }
      check(sbgpu_comm_init(ctx.get(), rank, world, world > 1 ? id : nullptr, &h_), "sbgpu_comm_init");
      if (world > 1 && rank == 0) std::remove(id_file.c_str()); /* every rank has joined: nothing is left for the next launch to trip over */
   }
   ~Comm() { sbgpu_comm_destroy(h_); }
   Comm(const Comm &) = delete;
   Comm &operator=(const Comm &) = delete;
   double allreduce_sum(double x) const
   {
      check(sbgpu_allreduce_sum_f64_host(h_, &x, 1), "sbgpu_allreduce_sum_f64_host");
      return x;
   }
   int64_t allreduce_sum(int64_t x) const
   {
      check(sbgpu_allreduce_sum_i64_host(h_, &x, 1), "sbgpu_allreduce_sum_i64_host");
      return x;
   }
   sbgpu_comm_t *get() const { return h_; }

 private:
   sbgpu_comm_t *h_;
};

/* Sample::procSample's tail (src/alignments.cpp:1821-1829) over every isoform that is written.
 * With loci sharded over ranks, all-reduce `total_fpkm` between the two loops.                 */
inline double sum_fpkm(const std::vector<Isoform> &isoforms)
{
   double total = 0.0;
   for (const Isoform &t : isoforms)
      if (t.kept) total += t.FPKM;
   return total;
}
inline void finalize_tpm(std::vector<Isoform> &isoforms, double total_fpkm)
{
   for (Isoform &t : isoforms) {
      if (!t.kept) continue;
      t.TPM = 1e6 * t.FPKM / total_fpkm;
      t.TPM_s = std::to_string(t.TPM);
   }
}

/* The six sequence columns of the `-f` table under `-b genome.fa` (src/alignments.cpp:1622-1636) for every bin of
 * a quantified batch: ExonBin::bin_dnaseq + Kmer<string>::GCRatio / Entropy / HighGCStrech, one kernel launch.
 * `chrom_seq` holds the chromosome's bases as load_chrom_fasta keeps them (base 1 first).                      */
struct BinSequenceStats {
   std::vector<double> gc, entropy; /* per bin, batch order                                     */
   std::vector<uint8_t> flags;      /* bit 0..3 = stretch (20, 0.8), (20, 0.9), (40, 0.8), (40, 0.9) */
};
inline BinSequenceStats bin_sequence_stats(const Context &ctx, const LocusBatch &batch, const std::string &chrom_seq)
{
   const int64_t n_loci = (int64_t)batch.row_off.size() - 1, n_bins = batch.row_off.back();
   std::vector<int64_t> off(1, 0);
   std::vector<uint32_t> sl, sr;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t s0 = batch.seg_off[(size_t)l], nseg = batch.seg_off[(size_t)l + 1] - s0;
      for (int64_t b = batch.row_off[(size_t)l]; b < batch.row_off[(size_t)l + 1]; ++b) {
         for (int64_t s = 0; s < nseg; ++s)
            if ((batch.bin_key[(size_t)(b * batch.key_words + (s >> 5))] >> (s & 31)) & 1u) {
               sl.push_back(batch.seg_left[(size_t)(s0 + s)]);
               sr.push_back(batch.seg_right[(size_t)(s0 + s)]);
            }
         off.push_back((int64_t)sl.size());
      }
   }
   BinSequenceStats out;
   out.gc.resize((size_t)n_bins);
   out.entropy.resize((size_t)n_bins);
   out.flags.resize((size_t)n_bins);
   check(sbgpu_binseq_host(ctx.get(), (const uint8_t *)chrom_seq.data(), 1, (int64_t)chrom_seq.size(), n_bins, off.data(), sl.data(),
                           sr.data(), out.gc.data(), out.entropy.data(), out.flags.data()),
         "sbgpu_binseq_host");
   return out;
}

/* The `-f` fragment-context table (Sample::printContext, src/alignments.cpp:1549-1639) as arrays, from either form of
 * sbgpu_context_table_* (include/sbgpu.h): which bins of every locus get a row, in which order, with how many hits and
 * which conditional probabilities.  host(): on a handle that holds hit -> bin (sbgpu_bins_create, sbgpu_quantify_host).
 * device(): right after an sbgpu_quantify_resident / sbgpu_front_stream_end call made while sbgpu_context_table_keep was
 * on, on that call's handle.  format_row() prints one row with the library's formatter; the caller supplies what the
 * table does not hold: the kept isoforms' names, FPKM and Frac, and the bins' segments (the handle's bin keys).           */
class ContextTable {
 public:
   std::vector<int64_t> locus_row_off, row_bin;
   std::vector<uint32_t> locus_hits, row_hits;
   std::vector<double> row_prob;
   int64_t n_rows = 0;

   static ContextTable host(const sbgpu_bins_t *bins, const uint32_t *compat, int32_t compat_words, const double *F, const int32_t *keep,
                            const int32_t *status)
   {
      ContextTable t;
      sbgpu_context_table_t s = t.prepare(bins);
      check(sbgpu_context_table_host(bins, compat, compat_words, F, keep, status, &s), "sbgpu_context_table_host");
      t.finish(s);
      return t;
   }
   static void keep(const Context &ctx, bool on) { check(sbgpu_context_table_keep(ctx.get(), on ? 1 : 0), "sbgpu_context_table_keep"); }
   static ContextTable device(const Context &ctx, const sbgpu_bins_t *bins, void *stream = nullptr)
   {
      ContextTable t;
      sbgpu_context_table_t s = t.prepare(bins);
      check(sbgpu_context_table_device(ctx.get(), bins, stream, &s), "sbgpu_context_table_device");
      t.finish(s);
      return t;
   }
   /* the probabilities of row r (global) of locus l: one per isoform of the locus */
   const double *row(int64_t l, int64_t r, const int64_t *iso_off, const int64_t *f_off) const
   {
      return row_prob.data() + f_off[l] + (r - locus_row_off[(size_t)l]) * (iso_off[l + 1] - iso_off[l]);
   }
   /* Row r of locus l as text.  kept[k]: index (inside the locus) of the k-th surviving isoform; names / fpkm / frac: per
    * surviving isoform; seg_left / seg_right: the n_seg segments of bin row_bin[r]; stats != nullptr: the six columns of -b. */
   std::string format_row(int64_t l, int64_t r, const int64_t *iso_off, const int64_t *f_off, const char *sample, int32_t sample_frag_count,
                          const char *gene_id, const std::vector<int> &kept, const std::vector<const char *> &names, const double *fpkm,
                          const double *frac, int n_seg, const uint32_t *seg_left, const uint32_t *seg_right,
                          const BinSequenceStats *stats = nullptr) const
   {
      const double *p = row(l, r, iso_off, f_off);
      std::vector<double> cond(kept.size());
      for (size_t k = 0; k < kept.size(); ++k) cond[k] = p[kept[k]];
      const int64_t b = row_bin[(size_t)r];
      std::string buf(1024, '\0');
      for (int pass = 0; pass < 2; ++pass) {
         const int n = stats ? sbgpu_format_context_row_seq(&buf[0], (int)buf.size(), sample, sample_frag_count, gene_id, locus_hits[(size_t)l],
                                                            (int)kept.size(), names.data(), fpkm, cond.data(), frac, n_seg, seg_left, seg_right,
                                                            row_hits[(size_t)r], stats->gc[(size_t)b], stats->entropy[(size_t)b], stats->flags[(size_t)b])
                             : sbgpu_format_context_row(&buf[0], (int)buf.size(), sample, sample_frag_count, gene_id, locus_hits[(size_t)l],
                                                        (int)kept.size(), names.data(), fpkm, cond.data(), frac, n_seg, seg_left, seg_right,
                                                        row_hits[(size_t)r]);
         check(n < 0 ? n : 0, "sbgpu_format_context_row");
         if (n < (int)buf.size()) {
            buf.resize((size_t)n);
            break;
         }
         buf.assign((size_t)n + 1, '\0');
      }
      return buf;
   }

 private:
   sbgpu_context_table_t prepare(const sbgpu_bins_t *bins)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      locus_row_off.assign((size_t)info[0] + 1, 0);
      locus_hits.assign((size_t)info[0] + 1, 0);
      row_bin.assign((size_t)info[2] + 1, 0);
      row_hits.assign((size_t)info[2] + 1, 0);
      row_prob.assign((size_t)info[3] + 1, 0.0);
      sbgpu_context_table_t s = {};
      s.locus_row_off = locus_row_off.data(), s.locus_hits = locus_hits.data(), s.row_bin = row_bin.data(), s.row_hits = row_hits.data();
      s.row_prob = row_prob.data();
      return s;
   }
   void finish(const sbgpu_context_table_t &s)
   {
      n_rows = s.n_rows;
      row_bin.resize((size_t)n_rows);
      row_hits.resize((size_t)n_rows);
   }
};

/* Fragment assignment (sbgpu_fragment_assign_*, include/sbgpu.h states the rule): every hit's MAP isoform (the index inside its
 * locus, -1: unassigned), its posterior and its number of candidates; per isoform the mass of the hits only it explains, of the
 * hits whose MAP it is, and the posterior mass; per locus the unassigned hits.  host(): on a handle that holds hit -> bin
 * (n_hits: the hits the handle was made from).  device(): under ContextTable::device's conditions (ContextTable::keep before the
 * resident call), n_hits and d_hit_mass (nullptr: unit masses) as that call was given them, d_theta normally its d_theta.       */
class FragmentAssignment {
 public:
   std::vector<int32_t> map_iso, n_cand;             /* [n_hits] */
   std::vector<double> map_prob;                     /* [n_hits] */
   std::vector<double> unique_mass, map_mass, post_mass; /* [n_iso] */
   std::vector<int64_t> unassigned;                  /* [n_loci] */
   sbgpu_fragment_assign_t raw{};  /* device(): the device arrays -- the context's, valid until its next quantify or assignment call */

   static FragmentAssignment host(const sbgpu_bins_t *bins, int64_t n_hits, const uint32_t *compat, int32_t compat_words, const double *F,
                                  const double *theta, const int32_t *keep, const int32_t *status, const float *hit_mass)
   {
      FragmentAssignment t;
      t.prepare(bins, n_hits);
      check(sbgpu_fragment_assign_host(bins, compat, compat_words, F, theta, keep, status, hit_mass, &t.raw), "sbgpu_fragment_assign_host");
      return t;
   }
   static FragmentAssignment device(const Context &ctx, const sbgpu_bins_t *bins, int64_t n_hits, const double *d_theta,
                                    const float *d_hit_mass = nullptr, void *stream = nullptr)
   {
      FragmentAssignment t;
      t.prepare(bins, n_hits);
      check(sbgpu_fragment_assign_device(ctx.get(), bins, d_theta, d_hit_mass, stream, &t.raw), "sbgpu_fragment_assign_device");
      return t;
   }

 private:
   void prepare(const sbgpu_bins_t *bins, int64_t n_hits)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      if (n_hits < 0) throw std::invalid_argument("FragmentAssignment: negative hit count");
      map_iso.assign((size_t)n_hits, -1), n_cand.assign((size_t)n_hits, 0), map_prob.assign((size_t)n_hits, 0.0);
      unique_mass.assign((size_t)info[1], 0.0), map_mass.assign((size_t)info[1], 0.0), post_mass.assign((size_t)info[1], 0.0);
      unassigned.assign((size_t)info[0], 0);
      raw = sbgpu_fragment_assign_t{};
      /* (the vectors' own buffers: moving the object moves them, and raw's host pointers with them) */
      raw.map_iso = map_iso.data(), raw.n_cand = n_cand.data(), raw.map_prob = map_prob.data();
      raw.unique_mass = unique_mass.data(), raw.map_mass = map_mass.data(), raw.post_mass = post_mass.data();
      raw.unassigned = unassigned.data();
      raw.n_hits = n_hits;
   }
};

/* Isoform-resolved coverage (sbgpu_isoform_coverage_*, include/sbgpu.h states the rule): per annotated exon the posterior-weighted
 * sequenced bases and -- for an exon that is not its isoform's last -- the mass of the spliced hits that support the junction
 * behind it; per isoform the bases of its exons; per locus the bases of the hits no kept isoform explains.  host(): on a handle
 * that holds hit -> bin, with the annotation and the hits it was made from.  device(): under FragmentAssignment::device's
 * conditions, annot with HOST pointers, d_hits and d_hit_mass (nullptr: unit masses) the device arrays the resident call was
 * given, d_theta normally its d_theta.  exon_depth() / iso_depth(): bases over length.                                        */
class IsoformCoverage {
 public:
   std::vector<double> exon_bases, junction_mass; /* [exon_off[n_iso]] */
   std::vector<double> iso_bases;                 /* [n_iso] */
   std::vector<double> unexplained_bases;         /* [n_loci] */
   sbgpu_isoform_coverage_t raw{};  /* device(): the device arrays -- the context's, valid until its next quantify or coverage call;
                                       its host pointers are null after the call: the vectors above are the results, in a copy too */

   static IsoformCoverage host(const sbgpu_bins_t *bins, const sbgpu_annotation_t &annot, const sbgpu_hits_t &hits, const uint32_t *compat,
                               int32_t compat_words, const double *F, const double *theta, const int32_t *keep, const int32_t *status,
                               const float *hit_mass)
   {
      IsoformCoverage t;
      t.prepare(bins, annot);
      check(sbgpu_isoform_coverage_host(bins, &annot, &hits, compat, compat_words, F, theta, keep, status, hit_mass, &t.raw), "sbgpu_isoform_coverage_host");
      t.done();
      return t;
   }
   static IsoformCoverage device(const Context &ctx, const sbgpu_bins_t *bins, const sbgpu_annotation_t &annot, const sbgpu_hits_t &d_hits,
                                 const double *d_theta, const float *d_hit_mass = nullptr, void *stream = nullptr)
   {
      IsoformCoverage t;
      t.prepare(bins, annot);
      check(sbgpu_isoform_coverage_device(ctx.get(), bins, &annot, &d_hits, d_theta, d_hit_mass, stream, &t.raw), "sbgpu_isoform_coverage_device");
      t.done();
      return t;
   }
   std::vector<double> exon_depth(const sbgpu_annotation_t &annot) const
   {
      std::vector<double> d(exon_bases.size());
      for (size_t e = 0; e < d.size(); ++e) d[e] = exon_bases[e] / ((double)annot.exon_right[e] - (double)annot.exon_left[e] + 1.0);
      return d;
   }
   std::vector<double> iso_depth(const sbgpu_annotation_t &annot) const
   {
      std::vector<double> d(iso_bases.size(), 0.0);
      for (size_t i = 0; i < d.size(); ++i) {
         int64_t len = 0;
         for (int64_t e = annot.exon_off[i]; e < annot.exon_off[i + 1]; ++e) len += (int64_t)annot.exon_right[e] - (int64_t)annot.exon_left[e] + 1;
         if (len > 0) d[i] = iso_bases[i] / (double)len;
      }
      return d;
   }

 private:
   void prepare(const sbgpu_bins_t *bins, const sbgpu_annotation_t &annot)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      if (!annot.iso_off || !annot.exon_off || annot.n_loci != info[0] || annot.iso_off[annot.n_loci] != info[1])
         throw std::invalid_argument("IsoformCoverage: the annotation is not the handle's");
      const size_t n_exon = (size_t)annot.exon_off[info[1]];
      exon_bases.assign(n_exon, 0.0), junction_mass.assign(n_exon, 0.0);
      iso_bases.assign((size_t)info[1], 0.0), unexplained_bases.assign((size_t)info[0], 0.0);
      raw = sbgpu_isoform_coverage_t{};
      raw.exon_bases = exon_bases.data(), raw.junction_mass = junction_mass.data();
      raw.iso_bases = iso_bases.data(), raw.unexplained_bases = unexplained_bases.data();
   }
   void done() { raw.exon_bases = raw.junction_mass = raw.iso_bases = raw.unexplained_bases = nullptr; }
};

/* Transcript-body coverage profile (sbgpu_body_profile_*, include/sbgpu.h states the rule): per isoform the posterior-weighted
 * sequenced bases in n_pos positional bins from 5' to 3' (iso_strand: 0 / 1 / 2 per isoform, a HOST array; nullptr: all 0), their
 * total, centre and coefficient of variation; per length class the sum of the expressed isoforms' profiles and their number.
 * host() / device(): under IsoformCoverage's conditions, with its arguments.  class_curve(c): class_profile over class_n.    */
class BodyProfile {
 public:
   int32_t n_pos = 0;
   std::vector<double> body_bases;                          /* [n_iso * n_pos] */
   std::vector<double> body_total, body_center, body_cv;    /* [n_iso] */
   std::vector<double> class_profile;                       /* [4 * n_pos] */
   std::vector<int64_t> class_n;                            /* [4] */
   sbgpu_body_profile_t raw{};  /* device(): the device arrays -- the context's, valid until its next quantify or body-profile call;
                                   its host pointers are null after the call: the vectors above are the results, in a copy too */

   static BodyProfile host(const sbgpu_bins_t *bins, const sbgpu_annotation_t &annot, const sbgpu_hits_t &hits, const uint32_t *compat,
                           int32_t compat_words, const double *F, const double *theta, const int32_t *keep, const int32_t *status,
                           const float *hit_mass, const uint8_t *iso_strand = nullptr, int32_t n_pos = 20)
   {
      BodyProfile t;
      t.prepare(bins, n_pos);
      check(sbgpu_body_profile_host(bins, &annot, &hits, compat, compat_words, F, theta, keep, status, hit_mass, iso_strand, n_pos, &t.raw),
            "sbgpu_body_profile_host");
      t.done();
      return t;
   }
   static BodyProfile device(const Context &ctx, const sbgpu_bins_t *bins, const sbgpu_annotation_t &annot, const sbgpu_hits_t &d_hits,
                             const double *d_theta, const float *d_hit_mass = nullptr, const uint8_t *iso_strand = nullptr, int32_t n_pos = 20,
                             void *stream = nullptr)
   {
      BodyProfile t;
      t.prepare(bins, n_pos);
      check(sbgpu_body_profile_device(ctx.get(), bins, &annot, &d_hits, d_theta, d_hit_mass, iso_strand, n_pos, stream, &t.raw),
            "sbgpu_body_profile_device");
      t.done();
      return t;
   }
   std::vector<double> class_curve(int c) const
   {
      std::vector<double> d((size_t)n_pos, 0.0);
      if (class_n[(size_t)c])
         for (int p = 0; p < n_pos; ++p) d[(size_t)p] = class_profile[(size_t)(c * n_pos + p)] / (double)class_n[(size_t)c];
      return d;
   }

 private:
   void prepare(const sbgpu_bins_t *bins, int32_t P)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      n_pos = P;
      const size_t n_iso = (size_t)info[1], p = (size_t)(P < 1 ? 1 : P > SBGPU_BODY_MAX_POS ? SBGPU_BODY_MAX_POS : P);
      body_bases.assign(n_iso * p, 0.0), body_total.assign(n_iso, 0.0), body_center.assign(n_iso, 0.0), body_cv.assign(n_iso, 0.0);
      class_profile.assign(4 * p, 0.0), class_n.assign(4, 0);
      raw = sbgpu_body_profile_t{};
      raw.body_bases = body_bases.data(), raw.body_total = body_total.data(), raw.body_center = body_center.data(), raw.body_cv = body_cv.data();
      raw.class_profile = class_profile.data(), raw.class_n = class_n.data();
   }
   void done()
   {
      raw.body_bases = raw.body_total = raw.body_center = raw.body_cv = raw.class_profile = nullptr;
      raw.class_n = nullptr;
   }
};

/* The model fit (sbgpu_em_fit_* / sbgpu_model_fit_device, include/sbgpu.h states the rule): expected counts and Pearson residuals
 * per bin, the EM's score per isoform, likelihood, deviance, Pearson statistic, fragment counts, degrees of freedom and the worst
 * bin per locus.  host(): any batch with theta (keep / status: nullptr = everything kept / every locus started); no GPU.
 * device(plan, ...): for a batch sbgpu_em_run_device solves, on its device arrays; device(bins, ...): right after a resident call
 * made with AbundanceBootstrap::keep on, on that call's handle.  reduced_chi2(): pearson / dof, NaN where dof is 0.           */
class ModelFit {
 public:
   std::vector<double> expected, resid;                  /* [n_bins] */
   std::vector<double> score;                            /* [n_iso] */
   std::vector<double> loglik, deviance, pearson;        /* [n_loci] */
   std::vector<int64_t> n_live, n_dropped, n_impossible; /* [n_loci] */
   std::vector<int32_t> dof, worst_bin;                  /* [n_loci] */
   sbgpu_em_fit_t raw{};  /* device(): the device arrays -- the context's, valid until its next quantify or fit call; its host
                             pointers are null after the call: the vectors above are the results, in a copy too */

   static ModelFit host(const sbgpu_batch_t &batch, const double *theta, const int32_t *keep = nullptr, const int32_t *status = nullptr)
   {
      if (batch.n_loci < 0 || !batch.row_off || !batch.iso_off) throw std::invalid_argument("ModelFit::host: bad n_loci or null offset array");
      ModelFit t;
      t.prepare(batch.n_loci, batch.row_off[batch.n_loci], batch.iso_off[batch.n_loci]);
      check(sbgpu_em_fit_host(&batch, theta, keep, status, &t.raw), "sbgpu_em_fit_host");
      t.done();
      return t;
   }
   static ModelFit device(const Context &ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const double *d_theta,
                          const int32_t *d_keep = nullptr, const int32_t *d_status = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_plan_info(plan, info), "sbgpu_plan_info");
      ModelFit t;
      t.prepare(info[0], info[1], info[2]);
      check(sbgpu_em_fit_device(ctx.get(), plan, d_count, d_F, d_theta, d_keep, d_status, stream, &t.raw), "sbgpu_em_fit_device");
      t.done();
      return t;
   }
   static ModelFit device(const Context &ctx, const sbgpu_bins_t *bins, const double *d_theta, const int32_t *d_keep = nullptr,
                          const int32_t *d_status = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      ModelFit t;
      t.prepare(info[0], info[2], info[1]);
      check(sbgpu_model_fit_device(ctx.get(), bins, d_theta, d_keep, d_status, stream, &t.raw), "sbgpu_model_fit_device");
      t.done();
      return t;
   }
   std::vector<double> reduced_chi2() const
   {
      std::vector<double> x(pearson.size());
      for (size_t l = 0; l < x.size(); ++l) x[l] = dof[l] > 0 ? pearson[l] / (double)dof[l] : std::nan("");
      return x;
   }

 private:
   void prepare(int64_t n_loci, int64_t n_bins, int64_t n_iso)
   {
      const size_t nl = (size_t)n_loci + 1, nb = (size_t)n_bins + 1, ni = (size_t)n_iso + 1; /* (one spare entry: data() of an empty vector may be null) */
      expected.assign(nb, 0.0), resid.assign(nb, 0.0), score.assign(ni, 0.0);
      loglik.assign(nl, 0.0), deviance.assign(nl, 0.0), pearson.assign(nl, 0.0);
      n_live.assign(nl, 0), n_dropped.assign(nl, 0), n_impossible.assign(nl, 0);
      dof.assign(nl, 0), worst_bin.assign(nl, -1);
      raw = sbgpu_em_fit_t{};
      raw.expected = expected.data(), raw.resid = resid.data(), raw.score = score.data();
      raw.loglik = loglik.data(), raw.deviance = deviance.data(), raw.pearson = pearson.data();
      raw.n_live = n_live.data(), raw.n_dropped = n_dropped.data(), raw.n_impossible = n_impossible.data();
      raw.dof = dof.data(), raw.worst_bin = worst_bin.data();
   }
   void done()
   {
      raw.expected = raw.resid = raw.score = raw.loglik = raw.deviance = raw.pearson = nullptr;
      raw.n_live = raw.n_dropped = raw.n_impossible = nullptr;
      raw.dof = raw.worst_bin = nullptr;
      expected.pop_back(), resid.pop_back(), score.pop_back(), loglik.pop_back(), deviance.pop_back(), pearson.pop_back();
      n_live.pop_back(), n_dropped.pop_back(), n_impossible.pop_back(), dof.pop_back(), worst_bin.pop_back();
   }
};

/* The variational Bayes solve (sbgpu_em_vb_* / sbgpu_model_vb_device, include/sbgpu.h states the rule): under a Dirichlet(alpha)
 * prior on every locus' isoform shares, the posterior's count, share and its standard deviation per isoform, and status,
 * iterations, evidence bound, active isoforms and fragments per locus.  host(): any batch; no GPU.  device(plan, ...): for a batch
 * sbgpu_em_run_device solves, on its device arrays; device(bins, ...): right after a resident call made with
 * AbundanceBootstrap::keep on, on that call's handle.  params: nullptr = alpha 0.01 and the EM's stopping rule.            */
class VariationalFit {
 public:
   std::vector<double> count, share, share_sd; /* [n_iso] */
   std::vector<int32_t> status, iters;         /* [n_loci] */
   std::vector<double> elbo;                   /* [n_loci] */
   std::vector<int32_t> n_active;              /* [n_loci] */
   std::vector<int64_t> n_frag;                /* [n_loci] */
   sbgpu_em_vb_t raw{};   /* device(): the device arrays -- the context's, valid until its next quantify or variational call; its
                             host pointers are null after the call */

   static VariationalFit host(const sbgpu_batch_t &batch, const sbgpu_vb_params_t *params = nullptr)
   {
      if (batch.n_loci < 0 || !batch.iso_off) throw std::invalid_argument("VariationalFit::host: bad n_loci or null offset array");
      VariationalFit t;
      t.prepare(batch.n_loci, batch.iso_off[batch.n_loci]);
      check(sbgpu_em_vb_host(&batch, params, &t.raw), "sbgpu_em_vb_host");
      t.done();
      return t;
   }
   static VariationalFit device(const Context &ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                                const sbgpu_vb_params_t *params = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_plan_info(plan, info), "sbgpu_plan_info");
      VariationalFit t;
      t.prepare(info[0], info[2]);
      check(sbgpu_em_vb_device(ctx.get(), plan, d_count, d_F, params, stream, &t.raw), "sbgpu_em_vb_device");
      t.done();
      return t;
   }
   static VariationalFit device(const Context &ctx, const sbgpu_bins_t *bins, const sbgpu_vb_params_t *params = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      VariationalFit t;
      t.prepare(info[0], info[1]);
      check(sbgpu_model_vb_device(ctx.get(), bins, params, stream, &t.raw), "sbgpu_model_vb_device");
      t.done();
      return t;
   }
   /* the isoforms the posterior leaves at least min_count fragments */
   std::vector<char> supported(double min_count = 1.0) const
   {
      std::vector<char> x(count.size());
      for (size_t i = 0; i < x.size(); ++i) x[i] = count[i] >= min_count;
      return x;
   }

 private:
   void prepare(int64_t n_loci, int64_t n_iso)
   {
      const size_t nl = (size_t)n_loci + 1, ni = (size_t)n_iso + 1; /* (one spare entry: data() of an empty vector may be null) */
      count.assign(ni, 0.0), share.assign(ni, 0.0), share_sd.assign(ni, 0.0);
      status.assign(nl, 0), iters.assign(nl, 0), elbo.assign(nl, 0.0), n_active.assign(nl, 0), n_frag.assign(nl, 0);
      raw = sbgpu_em_vb_t{};
      raw.count = count.data(), raw.share = share.data(), raw.share_sd = share_sd.data();
      raw.status = status.data(), raw.iters = iters.data(), raw.elbo = elbo.data(), raw.n_active = n_active.data(), raw.n_frag = n_frag.data();
   }
   void done()
   {
      raw.count = raw.share = raw.share_sd = raw.elbo = nullptr;
      raw.status = raw.iters = raw.n_active = nullptr;
      raw.n_frag = nullptr;
      count.pop_back(), share.pop_back(), share_sd.pop_back(), status.pop_back(), iters.pop_back(), elbo.pop_back(), n_active.pop_back(), n_frag.pop_back();
   }
};

/* The isoform information (sbgpu_em_info_* / sbgpu_model_info_device, include/sbgpu.h states the rule): which isoforms of every
 * locus the counted bins identify, alias or never see, the standard error of theta given the locus' total, the strongest
 * partner of every isoform, and -- packed by cov_off, the upper triangle over a locus' isoforms -- the covariance itself.
 * host(): any batch with theta; no GPU.  device(plan, iso_off, ...) / device(bins, iso_off, ...): as ModelFit's; iso_off: the
 * batch's host offsets [n_loci + 1], from which cov is sized (nullptr: no cov is brought to the host).                        */
class IsoformInfo {
 public:
   std::vector<double> se, partner_corr;          /* [n_iso] */
   std::vector<int32_t> ident, alias_of, partner; /* [n_iso] */
   std::vector<double> min_pivot;                 /* [n_loci] */
   std::vector<int32_t> rank, n_free, info_status; /* [n_loci] */
   std::vector<double> cov;                       /* [cov_off[n_loci]] */
   std::vector<int64_t> cov_off;                  /* [n_loci + 1] */
   sbgpu_em_info_t raw{}; /* device(): the device arrays -- the context's, valid until its next quantify or info call; its host
                             pointers are null after the call */

   static IsoformInfo host(const sbgpu_batch_t &batch, const double *theta, const int32_t *keep = nullptr, const int32_t *status = nullptr)
   {
      if (batch.n_loci < 0 || !batch.row_off || !batch.iso_off) throw std::invalid_argument("IsoformInfo::host: bad n_loci or null offset array");
      IsoformInfo t;
      t.prepare(batch.n_loci, batch.iso_off[batch.n_loci], batch.iso_off);
      check(sbgpu_em_info_host(&batch, theta, keep, status, &t.raw), "sbgpu_em_info_host");
      t.done();
      return t;
   }
   static IsoformInfo device(const Context &ctx, const sbgpu_plan_t *plan, const int64_t *iso_off, const int32_t *d_count, const double *d_F,
                             const double *d_theta, const int32_t *d_keep = nullptr, const int32_t *d_status = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_plan_info(plan, info), "sbgpu_plan_info");
      IsoformInfo t;
      t.prepare(info[0], info[2], iso_off);
      check(sbgpu_em_info_device(ctx.get(), plan, d_count, d_F, d_theta, d_keep, d_status, stream, &t.raw), "sbgpu_em_info_device");
      t.done();
      return t;
   }
   static IsoformInfo device(const Context &ctx, const sbgpu_bins_t *bins, const int64_t *iso_off, const double *d_theta,
                             const int32_t *d_keep = nullptr, const int32_t *d_status = nullptr, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      IsoformInfo t;
      t.prepare(info[0], info[1], iso_off);
      check(sbgpu_model_info_device(ctx.get(), bins, d_theta, d_keep, d_status, stream, &t.raw), "sbgpu_model_info_device");
      t.done();
      return t;
   }
   /* entry (j, k) of locus l's covariance; 0.0 where the locus has no packed block */
   double covariance(int64_t l, int64_t niso, int64_t j, int64_t k) const
   {
      if (j > k) std::swap(j, k);
      if (cov_off.empty() || cov_off[(size_t)l + 1] - cov_off[(size_t)l] != niso * (niso + 1) / 2) return 0.0;
      return cov[(size_t)(cov_off[(size_t)l] + j * niso - j * (j - 1) / 2 + (k - j))];
   }

 private:
   void prepare(int64_t n_loci, int64_t n_iso, const int64_t *iso_off)
   {
      const size_t nl = (size_t)n_loci + 1, ni = (size_t)n_iso + 1; /* (one spare entry: data() of an empty vector may be null) */
      se.assign(ni, 0.0), partner_corr.assign(ni, 0.0), ident.assign(ni, 0), alias_of.assign(ni, -1), partner.assign(ni, -1);
      min_pivot.assign(nl, 0.0), rank.assign(nl, 0), n_free.assign(nl, 0), info_status.assign(nl, 0);
      raw = sbgpu_em_info_t{};
      cov_off.clear(), cov.clear();
      if (iso_off) {
         cov_off.assign(nl, 0);
         check(sbgpu_em_info_cov_offsets(iso_off, n_loci, cov_off.data()), "sbgpu_em_info_cov_offsets");
         cov.assign((size_t)cov_off[(size_t)n_loci] + 1, 0.0);
         raw.cov = cov.data(), raw.cov_off = cov_off.data();
      }
      raw.se = se.data(), raw.partner_corr = partner_corr.data(), raw.ident = ident.data(), raw.alias_of = alias_of.data(), raw.partner = partner.data();
      raw.min_pivot = min_pivot.data(), raw.rank = rank.data(), raw.n_free = n_free.data(), raw.info_status = info_status.data();
   }
   void done()
   {
      raw.se = raw.partner_corr = raw.min_pivot = raw.cov = nullptr;
      raw.ident = raw.alias_of = raw.partner = raw.rank = raw.n_free = raw.info_status = nullptr;
      raw.cov_off = nullptr;
      se.pop_back(), partner_corr.pop_back(), ident.pop_back(), alias_of.pop_back(), partner.pop_back();
      min_pivot.pop_back(), rank.pop_back(), n_free.pop_back(), info_status.pop_back();
      if (!cov.empty()) cov.pop_back();
   }
};

/* The drop-one isoform support (sbgpu_em_loo_device / sbgpu_model_loo_device, include/sbgpu.h): for every kept
 * isoform of a locus of 2..64 kept isoforms, the likelihood-ratio statistic of the locus solved without it, the fragments only it
 * explains and where its mass goes.  device(): for a batch (plan) or right after a resident call (bins); iso_off and keep
 * ([n_iso] or null: everything kept) on the host size the packed theta_without.                                            */
class IsoformSupport {
 public:
   std::vector<double> lr_stat, heir_gain, theta_refit;                 /* [n_iso] */
   std::vector<int64_t> n_unique;                                       /* [n_iso] */
   std::vector<int32_t> heir, status_without, iters_without, support;   /* [n_iso] */
   std::vector<double> loglik_base;                                     /* [n_loci] */
   std::vector<int32_t> loo_status, status_base, iters_base;            /* [n_loci] */
   std::vector<double> theta_without;                                   /* [without_off[n_iso]] */
   std::vector<int64_t> without_off;                                    /* [n_iso + 1] */
   sbgpu_em_loo_t raw{}; /* the device arrays -- the context's, valid until its next quantify or support call; its host pointers
                            are null after the call */

   static IsoformSupport device(const Context &ctx, const sbgpu_plan_t *plan, const int64_t *iso_off, const int32_t *d_count, const double *d_F,
                                const int32_t *d_keep = nullptr, const int32_t *keep = nullptr, int64_t max_bytes = 0, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_plan_info(plan, info), "sbgpu_plan_info");
      IsoformSupport t;
      t.prepare(info[0], info[2], iso_off, keep);
      const sbgpu_loo_params_t par{max_bytes, 0};
      check(sbgpu_em_loo_device(ctx.get(), plan, d_count, d_F, d_keep, &par, stream, &t.raw), "sbgpu_em_loo_device");
      t.done();
      return t;
   }
   static IsoformSupport device(const Context &ctx, const sbgpu_bins_t *bins, const int64_t *iso_off, const int32_t *d_keep = nullptr,
                                const int32_t *keep = nullptr, int64_t max_bytes = 0, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      IsoformSupport t;
      t.prepare(info[0], info[1], iso_off, keep);
      const sbgpu_loo_params_t par{max_bytes, 0};
      check(sbgpu_model_loo_device(ctx.get(), bins, d_keep, &par, stream, &t.raw), "sbgpu_model_loo_device");
      t.done();
      return t;
   }
   /* 0.5 * erfc(sqrt(max(stat, 0) / 2)): the boundary mixture 1/2 chi2_0 + 1/2 chi2_1; 0 for +inf, 1 for a statistic <= 0 */
   double p_value(int64_t i) const
   {
      const double x = lr_stat[(size_t)i];
      return x == HUGE_VAL ? 0.0 : !(x > 0.0) ? 1.0 : 0.5 * std::erfc(std::sqrt(x / 2.0));
   }

   /* (public for a caller that fills raw through the host form's three calls) */
   void prepare(int64_t n_loci, int64_t n_iso, const int64_t *iso_off, const int32_t *keep)
   {
      const size_t nl = (size_t)n_loci + 1, ni = (size_t)n_iso + 1; /* (one spare entry: data() of an empty vector may be null) */
      lr_stat.assign(ni, 0.0), heir_gain.assign(ni, 0.0), theta_refit.assign(ni, 0.0), n_unique.assign(ni, 0);
      heir.assign(ni, -1), status_without.assign(ni, -1), iters_without.assign(ni, -1), support.assign(ni, 0);
      loglik_base.assign(nl, 0.0), loo_status.assign(nl, 0), status_base.assign(nl, -1), iters_base.assign(nl, -1);
      raw = sbgpu_em_loo_t{};
      without_off.clear(), theta_without.clear();
      if (iso_off) {
         without_off.assign(ni, 0);
         check(sbgpu_em_loo_offsets(iso_off, keep, n_loci, without_off.data()), "sbgpu_em_loo_offsets");
         theta_without.assign((size_t)without_off[(size_t)n_iso] + 1, 0.0);
         raw.theta_without = theta_without.data(), raw.without_off = without_off.data();
      }
      raw.lr_stat = lr_stat.data(), raw.heir_gain = heir_gain.data(), raw.theta_refit = theta_refit.data(), raw.n_unique = n_unique.data();
      raw.heir = heir.data(), raw.status_without = status_without.data(), raw.iters_without = iters_without.data(), raw.support = support.data();
      raw.loglik_base = loglik_base.data(), raw.loo_status = loo_status.data(), raw.status_base = status_base.data(), raw.iters_base = iters_base.data();
   }
   void done()
   {
      raw.lr_stat = raw.heir_gain = raw.theta_refit = raw.loglik_base = raw.theta_without = nullptr;
      raw.n_unique = nullptr, raw.without_off = nullptr;
      raw.heir = raw.status_without = raw.iters_without = raw.support = raw.loo_status = raw.status_base = raw.iters_base = nullptr;
      lr_stat.pop_back(), heir_gain.pop_back(), theta_refit.pop_back(), n_unique.pop_back();
      heir.pop_back(), status_without.pop_back(), iters_without.pop_back(), support.pop_back();
      loglik_base.pop_back(), loo_status.pop_back(), status_base.pop_back(), iters_base.pop_back();
      if (!theta_without.empty()) theta_without.pop_back();
   }
};

/* Differential isoform usage of two samples (sbgpu_em_diff_device / sbgpu_model_diff_device, include/sbgpu.h): per
 * locus the likelihood-ratio statistic of "one shared theta" against "a theta per sample" with its degrees of freedom, per
 * isoform the three thetas, usages and the usage difference.  device(): for two batches (plans) of one annotation, or right
 * after two resident calls on two contexts of one device (bins).  p-values (chi-squared with dof degrees of freedom, NaN where
 * lost_shift != 0) are the caller's.                                                                                       */
class DifferentialUsage {
 public:
   std::vector<double> theta_a, theta_b, theta_pooled, usage_a, usage_b, usage_pooled, delta_usage;   /* [n_iso]  */
   std::vector<double> lr_stat, loglik_a, loglik_b, loglik_a_pooled, loglik_b_pooled;                  /* [n_loci] */
   std::vector<int64_t> n_a, n_b, lost_shift;                                                          /* [n_loci] */
   std::vector<int32_t> dof, diff_status, top_iso, status_a, status_b, status_pooled, iters_a, iters_b, iters_pooled; /* [n_loci] */
   sbgpu_em_diff_t raw{}; /* the device arrays -- the (first) context's, valid until its next quantify or diff call; its host
                             pointers are null after the call */

   static DifferentialUsage device(const Context &ctx, const sbgpu_plan_t *plan_a, const int32_t *d_count_a, const double *d_F_a,
                                   const sbgpu_plan_t *plan_b, const int32_t *d_count_b, const double *d_F_b, const int32_t *d_keep_a = nullptr,
                                   const int32_t *d_keep_b = nullptr, int64_t max_bytes = 0, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_plan_info(plan_a, info), "sbgpu_plan_info");
      DifferentialUsage t;
      t.prepare(info[0], info[2]);
      const sbgpu_diff_params_t par{max_bytes, 0};
      check(sbgpu_em_diff_device(ctx.get(), plan_a, d_count_a, d_F_a, plan_b, d_count_b, d_F_b, d_keep_a, d_keep_b, &par, stream, &t.raw),
            "sbgpu_em_diff_device");
      t.done();
      return t;
   }
   static DifferentialUsage device(const Context &ctx_a, const sbgpu_bins_t *bins_a, const Context &ctx_b, const sbgpu_bins_t *bins_b,
                                   const int32_t *d_keep_a = nullptr, const int32_t *d_keep_b = nullptr, int64_t max_bytes = 0, void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins_a, info), "sbgpu_bins_info");
      DifferentialUsage t;
      t.prepare(info[0], info[1]);
      const sbgpu_diff_params_t par{max_bytes, 0};
      check(sbgpu_model_diff_device(ctx_a.get(), bins_a, ctx_b.get(), bins_b, d_keep_a, d_keep_b, &par, stream, &t.raw), "sbgpu_model_diff_device");
      t.done();
      return t;
   }
   /* The same on ONE bin table for both samples: the union of their bins by key (sbgpu_model_diff_merged_device).
    * merged, merged_row_off, merged_f_off: the merge -- its sizes, device arrays (ctx_a's, valid until its next quantify or merge
    * call; sbgpu_bins_merge_fetch copies them) and the union's offsets.                                                        */
   sbgpu_bins_merged_t merged{};
   std::vector<int64_t> merged_row_off, merged_f_off; /* [n_loci + 1] */
   static DifferentialUsage device_merged(const Context &ctx_a, const sbgpu_bins_t *bins_a, const Context &ctx_b, const sbgpu_bins_t *bins_b,
                                          const int32_t *d_keep_a = nullptr, const int32_t *d_keep_b = nullptr, int64_t max_bytes = 0,
                                          void *stream = nullptr)
   {
      int64_t info[8];
      check(sbgpu_bins_info(bins_a, info), "sbgpu_bins_info");
      DifferentialUsage t;
      t.prepare(info[0], info[1]);
      t.merged_row_off.assign((size_t)info[0] + 1, 0), t.merged_f_off.assign((size_t)info[0] + 1, 0);
      t.merged.row_off = t.merged_row_off.data(), t.merged.f_off = t.merged_f_off.data();
      const sbgpu_diff_params_t par{max_bytes, 0};
      check(sbgpu_model_diff_merged_device(ctx_a.get(), bins_a, ctx_b.get(), bins_b, d_keep_a, d_keep_b, &par, stream, &t.raw, &t.merged),
            "sbgpu_model_diff_merged_device");
      t.merged.row_off = t.merged.f_off = nullptr;
      t.done();
      return t;
   }

   /* (public for a caller that fills raw through the host form's three calls) */
   void prepare(int64_t n_loci, int64_t n_iso)
   {
      const size_t nl = (size_t)n_loci + 1, ni = (size_t)n_iso + 1; /* (one spare entry: data() of an empty vector may be null) */
      for (std::vector<double> *v : {&theta_a, &theta_b, &theta_pooled, &usage_a, &usage_b, &usage_pooled, &delta_usage}) v->assign(ni, 0.0);
      for (std::vector<double> *v : {&lr_stat, &loglik_a, &loglik_b, &loglik_a_pooled, &loglik_b_pooled}) v->assign(nl, 0.0);
      for (std::vector<int64_t> *v : {&n_a, &n_b, &lost_shift}) v->assign(nl, 0);
      for (std::vector<int32_t> *v : {&dof, &diff_status, &top_iso, &status_a, &status_b, &status_pooled, &iters_a, &iters_b, &iters_pooled}) v->assign(nl, 0);
      raw = sbgpu_em_diff_t{};
      raw.theta_a = theta_a.data(), raw.theta_b = theta_b.data(), raw.theta_pooled = theta_pooled.data();
      raw.usage_a = usage_a.data(), raw.usage_b = usage_b.data(), raw.usage_pooled = usage_pooled.data(), raw.delta_usage = delta_usage.data();
      raw.lr_stat = lr_stat.data(), raw.loglik_a = loglik_a.data(), raw.loglik_b = loglik_b.data();
      raw.loglik_a_pooled = loglik_a_pooled.data(), raw.loglik_b_pooled = loglik_b_pooled.data();
      raw.n_a = n_a.data(), raw.n_b = n_b.data(), raw.lost_shift = lost_shift.data();
      raw.dof = dof.data(), raw.diff_status = diff_status.data(), raw.top_iso = top_iso.data();
      raw.status_a = status_a.data(), raw.status_b = status_b.data(), raw.status_pooled = status_pooled.data();
      raw.iters_a = iters_a.data(), raw.iters_b = iters_b.data(), raw.iters_pooled = iters_pooled.data();
   }
   void done()
   {
      raw.theta_a = raw.theta_b = raw.theta_pooled = raw.usage_a = raw.usage_b = raw.usage_pooled = raw.delta_usage = nullptr;
      raw.lr_stat = raw.loglik_a = raw.loglik_b = raw.loglik_a_pooled = raw.loglik_b_pooled = nullptr;
      raw.n_a = raw.n_b = raw.lost_shift = nullptr;
      raw.dof = raw.diff_status = raw.top_iso = raw.status_a = raw.status_b = raw.status_pooled = raw.iters_a = raw.iters_b = raw.iters_pooled = nullptr;
      for (std::vector<double> *v : {&theta_a, &theta_b, &theta_pooled, &usage_a, &usage_b, &usage_pooled, &delta_usage, &lr_stat, &loglik_a, &loglik_b,
                                     &loglik_a_pooled, &loglik_b_pooled})
         v->pop_back();
      for (std::vector<int64_t> *v : {&n_a, &n_b, &lost_shift}) v->pop_back();
      for (std::vector<int32_t> *v : {&dof, &diff_status, &top_iso, &status_a, &status_b, &status_pooled, &iters_a, &iters_b, &iters_pooled}) v->pop_back();
   }
};

/* Differential isoform usage between two GROUPS of replicate samples (sbgpu_em_gdiff_device / sbgpu_model_gdiff_device,
 * include/sbgpu.h): per locus lr_between ("one theta for all" against "a theta per group") and lr_within ("a theta
 * per group" against "a theta per sample") with their degrees of freedom, per isoform the thetas and usages of every sample, of
 * the two groups and of all, and the groups' usage difference.  Samples are numbered group A's first; a per-sample array is
 * sample-major ([S x n_iso] or [S x n_loci]), a per-group one [2 x ...].  device(): for S batches (plans) of one annotation, or
 * right after S resident calls on S contexts of one device (bins).  p-values are the caller's.                              */
class GroupDifferentialUsage {
 public:
   int32_t n_a = 0, n_b = 0;
   std::vector<double> theta_sample, theta_group, theta_all, usage_sample, usage_group, usage_all, delta_usage;
   std::vector<double> lr_between, lr_within, loglik_own, loglik_group, loglik_all;
   std::vector<int64_t> n_frag, lost_shift;
   std::vector<int32_t> dof_between, dof_within, p_a, p_b, gdiff_status, top_iso, status_sample, iters_sample, status_group, iters_group, status_all,
      iters_all;
   sbgpu_em_gdiff_t raw{}; /* the device arrays -- the (first) context's, valid until its next quantify or gdiff call; its host
                              pointers are null after the call */

   /* plans, d_count, d_F: n_a + n_b entries, group A's first; d_keep: as many (any null), or empty: everything kept */
   static GroupDifferentialUsage device(const Context &ctx, int32_t n_a, int32_t n_b, const std::vector<const sbgpu_plan_t *> &plans,
                                        const std::vector<const int32_t *> &d_count, const std::vector<const double *> &d_F,
                                        const std::vector<const int32_t *> &d_keep = {}, int64_t max_bytes = 0, void *stream = nullptr)
   {
      const size_t S = (size_t)(n_a + n_b);
      if (n_a < 1 || n_b < 1 || plans.size() != S || d_count.size() != S || d_F.size() != S || (!d_keep.empty() && d_keep.size() != S))
         throw std::runtime_error("GroupDifferentialUsage::device: one plan, d_count and d_F per sample, at least one sample per group");
      int64_t info[8];
      check(sbgpu_plan_info(plans[0], info), "sbgpu_plan_info");
      GroupDifferentialUsage t;
      t.prepare(n_a, n_b, info[0], info[2]);
      const sbgpu_gdiff_params_t par{max_bytes, 0};
      check(sbgpu_em_gdiff_device(ctx.get(), n_a, n_b, plans.data(), d_count.data(), d_F.data(), d_keep.empty() ? nullptr : d_keep.data(), &par, stream,
                                  &t.raw),
            "sbgpu_em_gdiff_device");
      t.done();
      return t;
   }
   static GroupDifferentialUsage device(int32_t n_a, int32_t n_b, const std::vector<const Context *> &ctxs, const std::vector<const sbgpu_bins_t *> &bins,
                                        const std::vector<const int32_t *> &d_keep = {}, int64_t max_bytes = 0, void *stream = nullptr)
   {
      const size_t S = (size_t)(n_a + n_b);
      if (n_a < 1 || n_b < 1 || ctxs.size() != S || bins.size() != S || (!d_keep.empty() && d_keep.size() != S))
         throw std::runtime_error("GroupDifferentialUsage::device: one context and one handle per sample, at least one sample per group");
      std::vector<sbgpu_ctx_t *> raw_ctx;
      for (const Context *c : ctxs) raw_ctx.push_back(c ? c->get() : nullptr);
      int64_t info[8];
      check(sbgpu_bins_info(bins[0], info), "sbgpu_bins_info");
      GroupDifferentialUsage t;
      t.prepare(n_a, n_b, info[0], info[1]);
      const sbgpu_gdiff_params_t par{max_bytes, 0};
      check(sbgpu_model_gdiff_device(n_a, n_b, raw_ctx.data(), bins.data(), d_keep.empty() ? nullptr : d_keep.data(), &par, stream, &t.raw),
            "sbgpu_model_gdiff_device");
      t.done();
      return t;
   }

   /* (public for a caller that fills raw through the host form's three calls) */
   void prepare(int32_t groups_a, int32_t groups_b, int64_t n_loci, int64_t n_iso)
   {
      n_a = groups_a, n_b = groups_b;
      const size_t S = (size_t)(n_a + n_b), nl = (size_t)n_loci, ni = (size_t)n_iso; /* (one spare entry each: data() of an empty vector may be null) */
      for (std::vector<double> *v : {&theta_sample, &usage_sample}) v->assign(S * ni + 1, 0.0);
      for (std::vector<double> *v : {&theta_group, &usage_group}) v->assign(2 * ni + 1, 0.0);
      for (std::vector<double> *v : {&theta_all, &usage_all, &delta_usage}) v->assign(ni + 1, 0.0);
      for (std::vector<double> *v : {&lr_between, &lr_within}) v->assign(nl + 1, 0.0);
      for (std::vector<double> *v : {&loglik_own, &loglik_group, &loglik_all}) v->assign(S * nl + 1, 0.0);
      n_frag.assign(S * nl + 1, 0), lost_shift.assign(nl + 1, 0);
      for (std::vector<int32_t> *v : {&dof_between, &dof_within, &p_a, &p_b, &gdiff_status, &top_iso, &status_all, &iters_all}) v->assign(nl + 1, 0);
      for (std::vector<int32_t> *v : {&status_sample, &iters_sample}) v->assign(S * nl + 1, 0);
      for (std::vector<int32_t> *v : {&status_group, &iters_group}) v->assign(2 * nl + 1, 0);
      raw = sbgpu_em_gdiff_t{};
      raw.theta_sample = theta_sample.data(), raw.theta_group = theta_group.data(), raw.theta_all = theta_all.data();
      raw.usage_sample = usage_sample.data(), raw.usage_group = usage_group.data(), raw.usage_all = usage_all.data(), raw.delta_usage = delta_usage.data();
      raw.lr_between = lr_between.data(), raw.lr_within = lr_within.data();
      raw.loglik_own = loglik_own.data(), raw.loglik_group = loglik_group.data(), raw.loglik_all = loglik_all.data();
      raw.n_frag = n_frag.data(), raw.lost_shift = lost_shift.data();
      raw.dof_between = dof_between.data(), raw.dof_within = dof_within.data(), raw.p_a = p_a.data(), raw.p_b = p_b.data();
      raw.gdiff_status = gdiff_status.data(), raw.top_iso = top_iso.data();
      raw.status_sample = status_sample.data(), raw.iters_sample = iters_sample.data(), raw.status_group = status_group.data();
      raw.iters_group = iters_group.data(), raw.status_all = status_all.data(), raw.iters_all = iters_all.data();
   }
   void done()
   {
      raw.theta_sample = raw.theta_group = raw.theta_all = raw.usage_sample = raw.usage_group = raw.usage_all = raw.delta_usage = nullptr;
      raw.lr_between = raw.lr_within = raw.loglik_own = raw.loglik_group = raw.loglik_all = nullptr;
      raw.n_frag = raw.lost_shift = nullptr;
      raw.dof_between = raw.dof_within = raw.p_a = raw.p_b = raw.gdiff_status = raw.top_iso = nullptr;
      raw.status_sample = raw.iters_sample = raw.status_group = raw.iters_group = raw.status_all = raw.iters_all = nullptr;
      for (std::vector<double> *v : {&theta_sample, &theta_group, &theta_all, &usage_sample, &usage_group, &usage_all, &delta_usage, &lr_between, &lr_within,
                                     &loglik_own, &loglik_group, &loglik_all})
         v->pop_back();
      for (std::vector<int64_t> *v : {&n_frag, &lost_shift}) v->pop_back();
      for (std::vector<int32_t> *v : {&dof_between, &dof_within, &p_a, &p_b, &gdiff_status, &top_iso, &status_sample, &iters_sample, &status_group,
                                      &iters_group, &status_all, &iters_all})
         v->pop_back();
   }
};

/* The bootstrap of the resident path (sbgpu_bootstrap_keep / sbgpu_abundance_bootstrap_device, include/sbgpu.h): FPKM and TPM
 * mean, variance and percentile interval over resampled bin counts, with the replicates in which the expression filter kept
 * each isoform.  keep(): before the resident call; device(): right after it, on that call's handle.  interval_ranks(): the two
 * integer positions of the central `level` interval, level given as a fraction num / den so that no rounding picks the rank.   */
class AbundanceBootstrap {
 public:
   std::vector<double> theta_mean, theta_var, fpkm_mean, fpkm_var, fpkm_lo, fpkm_hi, tpm_mean, tpm_var, tpm_lo, tpm_hi; /* [n_iso] */
   std::vector<int32_t> keep_count;    /* [n_iso] */
   std::vector<int32_t> status_count;  /* [n_loci][4] */
   std::vector<double> total_fpkm_rep; /* [n_rep] */
   std::vector<double> fpkm_rep;       /* [n_rep][n_iso], with keep_replicates */
   std::vector<int32_t> keep_rep;      /* [n_rep][n_iso], with keep_replicates */
   int32_t rank_lo = 0, rank_hi = 0;
   sbgpu_abundance_bootstrap_t raw{};  /* the device arrays: the context's, valid until its next bootstrap or quantify call */

   static void keep(const Context &ctx, bool on) { check(sbgpu_bootstrap_keep(ctx.get(), on ? 1 : 0), "sbgpu_bootstrap_keep"); }
   static void interval_ranks(int32_t n_rep, int64_t level_num, int64_t level_den, int32_t *lo, int32_t *hi)
   {
      int64_t l = (int64_t)n_rep * (level_den - level_num) / (2 * level_den); /* floor(n_rep (1 - level) / 2) */
      if (l > (n_rep - 1) / 2) l = (n_rep - 1) / 2;
      *lo = (int32_t)l, *hi = n_rep - 1 - (int32_t)l;
   }
   static AbundanceBootstrap device(const Context &ctx, const sbgpu_bins_t *bins, int32_t n_rep, uint64_t seed, int32_t rank_lo, int32_t rank_hi,
                                    int32_t rep_first = 0, const int64_t *locus_id = nullptr, bool keep_theta_rep = false,
                                    sbgpu_comm_t *comm = nullptr, void *stream = nullptr, bool keep_replicates = false)
   {
      AbundanceBootstrap b;
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      const size_t ni = (size_t)info[1] + 1, nl = (size_t)info[0] + 1;
      sbgpu_abundance_bootstrap_t &o = b.raw;
      std::vector<double> *stat[10] = {&b.theta_mean, &b.theta_var, &b.fpkm_mean, &b.fpkm_var, &b.fpkm_lo, &b.fpkm_hi, &b.tpm_mean, &b.tpm_var, &b.tpm_lo, &b.tpm_hi};
      double **slot[10] = {&o.theta_mean, &o.theta_var, &o.fpkm_mean, &o.fpkm_var, &o.fpkm_lo, &o.fpkm_hi, &o.tpm_mean, &o.tpm_var, &o.tpm_lo, &o.tpm_hi};
      for (int i = 0; i < 10; ++i) {
         stat[i]->assign(ni, 0.0);
         *slot[i] = stat[i]->data();
      }
      b.keep_count.assign(ni, 0), b.status_count.assign(nl * 4, 0), b.total_fpkm_rep.assign((size_t)(n_rep > 0 ? n_rep : 1), 0.0);
      o.keep_count = b.keep_count.data(), o.status_count = b.status_count.data(), o.total_fpkm_rep = b.total_fpkm_rep.data();
      if (keep_replicates && n_rep > 0 && info[1] > 0) {
         b.fpkm_rep.assign((size_t)n_rep * (size_t)info[1], 0.0), b.keep_rep.assign((size_t)n_rep * (size_t)info[1], 0);
         o.fpkm_rep = b.fpkm_rep.data(), o.keep_rep = b.keep_rep.data();
      }
      const sbgpu_bootstrap_params_t par = {n_rep, rep_first, seed, locus_id};
      check(sbgpu_abundance_bootstrap_device(ctx.get(), bins, &par, rank_lo, rank_hi, keep_theta_rep ? 1 : 0, comm, stream, &o),
            "sbgpu_abundance_bootstrap_device");
      for (int i = 0; i < 10; ++i) stat[i]->resize(ni - 1);
      b.keep_count.resize(ni - 1), b.status_count.resize((nl - 1) * 4);
      b.rank_lo = rank_lo, b.rank_hi = rank_hi;
      return b;
   }
};

/* Abundances per locus (a locus is the reference's gene): sbgpu_locus_abundance_host on one abundance vector -- the sum of the
 * kept isoforms' FPKM in isoform order, the number of kept isoforms, and 1e6 * sum / total_fpkm (0.0 where nothing is kept).  */
struct LocusAbundance {
   std::vector<double> fpkm, tpm; /* [n_loci] */
   std::vector<int32_t> kept;     /* [n_loci] */
};
inline LocusAbundance locus_abundance(const std::vector<int64_t> &iso_off, const double *fpkm, const int32_t *keep, double total_fpkm)
{
   if (iso_off.empty()) throw std::invalid_argument("locus_abundance: iso_off holds n_loci + 1 offsets");
   const size_t nl = iso_off.size() - 1;
   LocusAbundance r;
   r.fpkm.assign(nl + 1, 0.0), r.tpm.assign(nl + 1, 0.0), r.kept.assign(nl + 1, 0);
   check(sbgpu_locus_abundance_host((int64_t)nl, iso_off.data(), fpkm, keep, total_fpkm, r.fpkm.data(), r.tpm.data(), r.kept.data()),
         "sbgpu_locus_abundance_host");
   r.fpkm.resize(nl), r.tpm.resize(nl), r.kept.resize(nl);
   return r;
}

/* sbgpu_locus_bootstrap_device: AbundanceBootstrap's results (`iso`, bit for bit that call's) and beside them mean, variance and
 * interval of Frac per isoform and of FPKM / TPM per locus, with the replicates in which each locus kept an isoform.           */
class LocusBootstrap {
 public:
   AbundanceBootstrap iso;
   std::vector<double> frac_mean, frac_var, frac_lo, frac_hi;                         /* [n_iso]  */
   std::vector<double> locus_fpkm_mean, locus_fpkm_var, locus_fpkm_lo, locus_fpkm_hi; /* [n_loci] */
   std::vector<double> locus_tpm_mean, locus_tpm_var, locus_tpm_lo, locus_tpm_hi;     /* [n_loci] */
   std::vector<int32_t> locus_kept_count; /* [n_loci] */
   std::vector<double> frac_rep;          /* [n_rep][n_iso], with keep_replicates  */
   std::vector<double> locus_fpkm_rep;    /* [n_rep][n_loci], with keep_replicates */
   std::vector<int32_t> locus_kept_rep;   /* [n_rep][n_loci], with keep_replicates */
   sbgpu_locus_bootstrap_t raw{};         /* the device arrays: the context's, valid until its next bootstrap or quantify call */

   static LocusBootstrap device(const Context &ctx, const sbgpu_bins_t *bins, int32_t n_rep, uint64_t seed, int32_t rank_lo, int32_t rank_hi,
                                int32_t rep_first = 0, const int64_t *locus_id = nullptr, bool keep_theta_rep = false,
                                sbgpu_comm_t *comm = nullptr, void *stream = nullptr, bool keep_replicates = false)
   {
      LocusBootstrap b;
      int64_t info[8];
      check(sbgpu_bins_info(bins, info), "sbgpu_bins_info");
      const size_t ni = (size_t)info[1] + 1, nl = (size_t)info[0] + 1;
      sbgpu_abundance_bootstrap_t &o = b.iso.raw;
      std::vector<double> *stat[10] = {&b.iso.theta_mean, &b.iso.theta_var, &b.iso.fpkm_mean, &b.iso.fpkm_var, &b.iso.fpkm_lo, &b.iso.fpkm_hi,
                                       &b.iso.tpm_mean, &b.iso.tpm_var, &b.iso.tpm_lo, &b.iso.tpm_hi};
      double **slot[10] = {&o.theta_mean, &o.theta_var, &o.fpkm_mean, &o.fpkm_var, &o.fpkm_lo, &o.fpkm_hi, &o.tpm_mean, &o.tpm_var, &o.tpm_lo, &o.tpm_hi};
      for (int i = 0; i < 10; ++i) {
         stat[i]->assign(ni, 0.0);
         *slot[i] = stat[i]->data();
      }
      b.iso.keep_count.assign(ni, 0), b.iso.status_count.assign(nl * 4, 0), b.iso.total_fpkm_rep.assign((size_t)(n_rep > 0 ? n_rep : 1), 0.0);
      o.keep_count = b.iso.keep_count.data(), o.status_count = b.iso.status_count.data(), o.total_fpkm_rep = b.iso.total_fpkm_rep.data();
      sbgpu_locus_bootstrap_t &l = b.raw;
      std::vector<double> *lstat[12] = {&b.frac_mean, &b.frac_var, &b.frac_lo, &b.frac_hi, &b.locus_fpkm_mean, &b.locus_fpkm_var, &b.locus_fpkm_lo,
                                        &b.locus_fpkm_hi, &b.locus_tpm_mean, &b.locus_tpm_var, &b.locus_tpm_lo, &b.locus_tpm_hi};
      double **lslot[12] = {&l.frac_mean, &l.frac_var, &l.frac_lo, &l.frac_hi, &l.locus_fpkm_mean, &l.locus_fpkm_var, &l.locus_fpkm_lo,
                            &l.locus_fpkm_hi, &l.locus_tpm_mean, &l.locus_tpm_var, &l.locus_tpm_lo, &l.locus_tpm_hi};
      for (int i = 0; i < 12; ++i) {
         lstat[i]->assign(i < 4 ? ni : nl, 0.0);
         *lslot[i] = lstat[i]->data();
      }
      b.locus_kept_count.assign(nl, 0);
      l.locus_kept_count = b.locus_kept_count.data();
      if (keep_replicates && n_rep > 0) {
         if (info[1] > 0) {
            b.iso.fpkm_rep.assign((size_t)n_rep * (size_t)info[1], 0.0), b.iso.keep_rep.assign((size_t)n_rep * (size_t)info[1], 0);
            b.frac_rep.assign((size_t)n_rep * (size_t)info[1], 0.0);
            o.fpkm_rep = b.iso.fpkm_rep.data(), o.keep_rep = b.iso.keep_rep.data(), l.frac_rep = b.frac_rep.data();
         }
         if (info[0] > 0) {
            b.locus_fpkm_rep.assign((size_t)n_rep * (size_t)info[0], 0.0), b.locus_kept_rep.assign((size_t)n_rep * (size_t)info[0], 0);
            l.locus_fpkm_rep = b.locus_fpkm_rep.data(), l.locus_kept_rep = b.locus_kept_rep.data();
         }
      }
      const sbgpu_bootstrap_params_t par = {n_rep, rep_first, seed, locus_id};
      check(sbgpu_locus_bootstrap_device(ctx.get(), bins, &par, rank_lo, rank_hi, keep_theta_rep ? 1 : 0, comm, stream, &o, &l),
            "sbgpu_locus_bootstrap_device");
      for (int i = 0; i < 10; ++i) stat[i]->resize(ni - 1);
      for (int i = 0; i < 12; ++i) lstat[i]->resize((i < 4 ? ni : nl) - 1);
      b.iso.keep_count.resize(ni - 1), b.iso.status_count.resize((nl - 1) * 4), b.locus_kept_count.resize(nl - 1);
      b.iso.rank_lo = rank_lo, b.iso.rank_hi = rank_hi;
      return b;
   }
};

/* Splicing events (sbgpu_splice_*, include/sbgpu.h states the rule): the event table of an annotation -- every distinct exon and
 * intron of every locus, the isoforms that include it and the number that span it.  Owns its vectors; raw names them (a host
 * table: what sbgpu_splice_psi_host / sbgpu_splice_support_host take).  Built once per annotation, on the host, no GPU needed. */
class SpliceEvents {
 public:
   std::vector<int64_t> event_off, incl_off, incl_exon, iso_off;
   std::vector<int32_t> event_locus, n_span, incl_iso;
   std::vector<uint8_t> event_kind, event_flags;
   std::vector<uint32_t> event_left, event_right, iso_left, iso_right;
   sbgpu_splice_events_t raw{};

   explicit SpliceEvents(const sbgpu_annotation_t &annot)
   {
      int64_t shape[2] = {0, 0};
      check(sbgpu_splice_events_shapes_host(&annot, shape), "sbgpu_splice_events_shapes_host");
      const size_t nl = (size_t)annot.n_loci, ni = (size_t)annot.iso_off[annot.n_loci], nu = (size_t)shape[0], nc = (size_t)shape[1];
      event_off.assign(nl + 1, 0), iso_off.assign(nl + 1, 0), incl_off.assign(nu + 1, 0);
      event_locus.assign(nu, 0), n_span.assign(nu, 0), event_kind.assign(nu, 0), event_flags.assign(nu, 0), event_left.assign(nu, 0), event_right.assign(nu, 0);
      incl_iso.assign(nc, 0), incl_exon.assign(nc, 0), iso_left.assign(ni, 0), iso_right.assign(ni, 0);
      raw.n_events = shape[0], raw.n_incl = shape[1];
      name();
      check(sbgpu_splice_events_build_host(&annot, &raw), "sbgpu_splice_events_build_host");
   }
   SpliceEvents(const SpliceEvents &o) { *this = o; }
   SpliceEvents &operator=(const SpliceEvents &o)
   {
      event_off = o.event_off, incl_off = o.incl_off, incl_exon = o.incl_exon, iso_off = o.iso_off;
      event_locus = o.event_locus, n_span = o.n_span, incl_iso = o.incl_iso, event_kind = o.event_kind, event_flags = o.event_flags;
      event_left = o.event_left, event_right = o.event_right, iso_left = o.iso_left, iso_right = o.iso_right;
      raw = o.raw;
      name();
      return *this;
   }
   int64_t n_events() const { return raw.n_events; }
   int64_t n_incl(int64_t u) const { return incl_off[(size_t)u + 1] - incl_off[(size_t)u]; }
   bool alternative(int64_t u) const { return n_incl(u) != n_span[(size_t)u]; }

 private:
   void name()
   {
      raw.event_off = event_off.data(), raw.event_locus = event_locus.data(), raw.event_kind = event_kind.data();
      raw.event_left = event_left.data(), raw.event_right = event_right.data(), raw.event_flags = event_flags.data(), raw.n_span = n_span.data();
      raw.incl_off = incl_off.data(), raw.incl_iso = incl_iso.data(), raw.incl_exon = incl_exon.data();
      raw.iso_off = iso_off.data(), raw.iso_left = iso_left.data(), raw.iso_right = iso_right.data();
   }
};

/* PSI of every event for n_rows abundance rows (x / keep: [n_rows][n_iso], keep may be nullptr).  host(): psi [n_rows * n_events]
 * and defined_count [n_events], no GPU.  device(): d_events is a table of DEVICE pointers the caller uploaded (the struct of a
 * SpliceEvents with every pointer replaced), every other array a device array; one launch, asynchronous on `stream`.
 * support_host() / support_device(): the events' support from the coverage's exon_bases / junction_mass (either may be nullptr). */
class SplicePsi {
 public:
   int64_t n_rows = 0;
   std::vector<double> psi;
   std::vector<int32_t> defined_count;

   static SplicePsi host(const SpliceEvents &events, int64_t n_rows, const double *x, const int32_t *keep = nullptr)
   {
      SplicePsi r;
      r.n_rows = n_rows;
      r.psi.assign((size_t)(n_rows > 0 ? n_rows : 0) * (size_t)events.n_events(), 0.0), r.defined_count.assign((size_t)events.n_events(), 0);
      check(sbgpu_splice_psi_host(&events.raw, n_rows, x, keep, r.psi.data(), r.defined_count.data()), "sbgpu_splice_psi_host");
      return r;
   }
   static void device(const Context &ctx, const sbgpu_splice_events_t &d_events, int64_t n_rows, const double *d_x, const int32_t *d_keep, double *d_psi,
                      int32_t *d_defined_count = nullptr, void *stream = nullptr)
   {
      check(sbgpu_splice_psi_device(ctx.get(), &d_events, n_rows, d_x, d_keep, d_psi, d_defined_count, stream), "sbgpu_splice_psi_device");
   }
   static std::vector<double> support_host(const SpliceEvents &events, const double *exon_bases, const double *junction_mass)
   {
      std::vector<double> s((size_t)events.n_events(), 0.0);
      check(sbgpu_splice_support_host(&events.raw, exon_bases, junction_mass, s.data()), "sbgpu_splice_support_host");
      return s;
   }
   static void support_device(const Context &ctx, const sbgpu_splice_events_t &d_events, const double *d_exon_bases, const double *d_junction_mass,
                              double *d_support, void *stream = nullptr)
   {
      check(sbgpu_splice_support_device(ctx.get(), &d_events, d_exon_bases, d_junction_mass, d_support, stream), "sbgpu_splice_support_device");
   }
};

/* A GTF annotation read by the library (sbgpu_gtf_*, include/sbgpu.h states the rule).  host(): no GPU.  device(): the file's
 * bytes are uploaded through the context's pool and parsed and grouped into transcripts on the device; the same arrays, names
 * and counts come back.  The handle's arrays are the object's: annot() / clusters() point into it and live as long as it does.
 * ref_names: a BAM header's reference names (empty: chromosome ids by first appearance in the file).                          */
class GtfAnnotation {
 public:
   static GtfAnnotation host(const uint8_t *bytes, int64_t n_bytes, const std::vector<std::string> &ref_names = {})
   {
      GtfAnnotation g;
      const Opts o(ref_names);
      check(sbgpu_gtf_read_host(bytes, n_bytes, &o.raw, &g.h_), "sbgpu_gtf_read_host");
      g.load();
      return g;
   }
   static GtfAnnotation device(const Context &ctx, const uint8_t *bytes, int64_t n_bytes, const std::vector<std::string> &ref_names = {}, void *stream = nullptr)
   {
      GtfAnnotation g;
      const Opts o(ref_names);
      check(sbgpu_gtf_read_upload(ctx.get(), bytes, n_bytes, &o.raw, stream, &g.h_), "sbgpu_gtf_read_upload");
      g.load();
      return g;
   }
   GtfAnnotation(GtfAnnotation &&o) noexcept { *this = std::move(o); }
   GtfAnnotation &operator=(GtfAnnotation &&o) noexcept
   {
      if (this != &o) {
         sbgpu_gtf_destroy(h_);
         h_ = o.h_, o.h_ = nullptr;
         annot_ = o.annot_, clusters_ = o.clusters_, names_ = o.names_, iso_len_ = o.iso_len_, iso_strand_ = o.iso_strand_;
         for (int k = 0; k < 16; ++k) info_[k] = o.info_[k];
      }
      return *this;
   }
   GtfAnnotation(const GtfAnnotation &) = delete;
   GtfAnnotation &operator=(const GtfAnnotation &) = delete;
   ~GtfAnnotation() { sbgpu_gtf_destroy(h_); }

   const sbgpu_annotation_t &annot() const { return annot_; }
   const sbgpu_clusters_t &clusters() const { return clusters_; }
   const int32_t *iso_len() const { return iso_len_; }
   const uint8_t *iso_strand() const { return iso_strand_; }
   int64_t n_loci() const { return annot_.n_loci; }
   int64_t n_iso() const { return annot_.iso_off[annot_.n_loci]; }
   int64_t info(int k) const { return info_[k]; } // sbgpu_gtf_info's words
   std::string gene_id(int64_t locus) const { return std::string(names_.gene_id + names_.gene_id_off[locus], names_.gene_id + names_.gene_id_off[locus + 1]); }
   std::string gene_name(int64_t locus) const { return std::string(names_.gene_name + names_.gene_name_off[locus], names_.gene_name + names_.gene_name_off[locus + 1]); }
   std::string transcript_id(int64_t iso) const
   {
      return std::string(names_.transcript_id + names_.transcript_id_off[iso], names_.transcript_id + names_.transcript_id_off[iso + 1]);
   }
   std::string chrom(int64_t id) const { return std::string(names_.chrom + names_.chrom_off[id], names_.chrom + names_.chrom_off[id + 1]); }
   std::vector<uint8_t> line_status() const
   {
      std::vector<uint8_t> s((size_t)info_[0] + 1);
      check(sbgpu_gtf_line_status(h_, s.data()), "sbgpu_gtf_line_status");
      s.pop_back();
      return s;
   }

 private:
   struct Opts {
      std::vector<const char *> names;
      sbgpu_gtf_opts_t raw;
      explicit Opts(const std::vector<std::string> &ref_names)
      {
         for (const std::string &n : ref_names) names.push_back(n.c_str());
         raw.n_ref = (int64_t)names.size(), raw.ref_name = names.empty() ? nullptr : names.data(), raw.hash_bits = 0;
      }
   };
   GtfAnnotation() {}
   void load()
   {
      check(sbgpu_gtf_annotation(h_, &annot_, &clusters_, &iso_len_, &iso_strand_), "sbgpu_gtf_annotation");
      check(sbgpu_gtf_names(h_, &names_), "sbgpu_gtf_names");
      check(sbgpu_gtf_info(h_, info_), "sbgpu_gtf_info");
   }
   sbgpu_gtf_t *h_ = nullptr;
   sbgpu_annotation_t annot_{};
   sbgpu_clusters_t clusters_{};
   sbgpu_gtf_names_t names_{};
   const int32_t *iso_len_ = nullptr;
   const uint8_t *iso_strand_ = nullptr;
   int64_t info_[16] = {};
};

/* A genome FASTA read by the library (sbgpu_fasta_*, include/sbgpu.h states the rule).  host(): no GPU, the packed sequence is
 * in host memory.  device(): the file's bytes are uploaded through the context's pool and packed on the device, where the
 * sequence stays -- the genome of binseq_device().  The index arrays point into the handle and live as long as the object.    */
class FastaGenome {
 public:
   static FastaGenome host(const uint8_t *bytes, int64_t n_bytes)
   {
      FastaGenome g;
      check(sbgpu_fasta_read_host(bytes, n_bytes, &g.h_), "sbgpu_fasta_read_host");
      g.load();
      return g;
   }
   static FastaGenome device(const Context &ctx, const uint8_t *bytes, int64_t n_bytes, void *stream = nullptr)
   {
      FastaGenome g;
      check(sbgpu_fasta_read_upload(ctx.get(), bytes, n_bytes, stream, &g.h_), "sbgpu_fasta_read_upload");
      g.load();
      return g;
   }
   FastaGenome(FastaGenome &&o) noexcept { *this = std::move(o); }
   FastaGenome &operator=(FastaGenome &&o) noexcept
   {
      if (this != &o) {
         sbgpu_fasta_destroy(h_);
         h_ = o.h_, o.h_ = nullptr;
         seq_off_ = o.seq_off_, offset_ = o.offset_, line_bases_ = o.line_bases_, line_width_ = o.line_width_, name_off_ = o.name_off_;
         flags_ = o.flags_, names_ = o.names_;
         for (int k = 0; k < 16; ++k) info_[k] = o.info_[k];
      }
      return *this;
   }
   FastaGenome(const FastaGenome &) = delete;
   FastaGenome &operator=(const FastaGenome &) = delete;
   ~FastaGenome() { sbgpu_fasta_destroy(h_); }

   const sbgpu_fasta_t *get() const { return h_; }
   int64_t n_contigs() const { return info_[2]; }
   int64_t info(int k) const { return info_[k]; } // sbgpu_fasta_info's words
   bool on_device() const { return info_[10] != 0; }
   std::string name(int64_t c) const { return std::string(names_ + name_off_[c], names_ + name_off_[c + 1]); }
   int64_t length(int64_t c) const { return seq_off_[c + 1] - seq_off_[c]; }
   int64_t offset(int64_t c) const { return offset_[c]; }
   int64_t line_bases(int64_t c) const { return line_bases_[c]; }
   int64_t line_width(int64_t c) const { return line_width_[c]; }
   uint8_t flags(int64_t c) const { return flags_[c]; }
   const int64_t *seq_off() const { return seq_off_; }
   /* the first contig of that name, compared ASCII-lower-cased; -1: none */
   int64_t find(const std::string &name) const
   {
      int64_t c = -1;
      check(sbgpu_fasta_find(h_, name.data(), (int64_t)name.size(), &c), "sbgpu_fasta_find");
      return c;
   }
   /* `len` bases of contig c from base `start` (1-based) */
   std::string fetch(int64_t c, int64_t start, int64_t len) const
   {
      std::string s((size_t)(len > 0 ? len : 0), '\0');
      check(sbgpu_fasta_fetch(h_, c, start, len, s.empty() ? nullptr : (uint8_t *)&s[0]), "sbgpu_fasta_fetch");
      return s;
   }
   std::string sequence(int64_t c) const { return fetch(c, 1, length(c)); }
   std::string fai_text() const
   {
      int64_t need = 0;
      check(sbgpu_fasta_fai(h_, nullptr, 0, &need), "sbgpu_fasta_fai");
      std::string s((size_t)need, '\0');
      if (need) check(sbgpu_fasta_fai(h_, &s[0], need, &need), "sbgpu_fasta_fai");
      return s;
   }
   /* `-b` over chromosomes with host arrays (sbgpu_binseq_fasta_host): bins [run_off[r], run_off[r + 1]) lie on contig run_contig[r] */
   void binseq(const Context &ctx, const std::vector<int64_t> &run_off, const std::vector<int32_t> &run_contig, const std::vector<int64_t> &seg_off,
               const std::vector<uint32_t> &seg_left, const std::vector<uint32_t> &seg_right, std::vector<double> &gc, std::vector<double> &entropy,
               std::vector<uint8_t> &flags) const
   {
      const int64_t n_bins = (int64_t)seg_off.size() - 1;
      gc.assign((size_t)n_bins, 0.0), entropy.assign((size_t)n_bins, 0.0), flags.assign((size_t)n_bins, 0);
      check(sbgpu_binseq_fasta_host(ctx.get(), h_, (int64_t)run_contig.size(), run_off.data(), run_contig.data(), n_bins, seg_off.data(), seg_left.data(),
                                    seg_right.data(), gc.data(), entropy.data(), flags.data()),
            "sbgpu_binseq_fasta_host");
   }
   /* the same on device arrays, with the sequence resident (sbgpu_binseq_fasta_device) */
   void binseq_device(const Context &ctx, const std::vector<int64_t> &run_off, const std::vector<int32_t> &run_contig, int64_t n_bins, const int64_t *d_seg_off,
                      const uint32_t *d_seg_left, const uint32_t *d_seg_right, double *d_gc, double *d_entropy, uint8_t *d_flags, int32_t *d_error,
                      void *stream = nullptr) const
   {
      check(sbgpu_binseq_fasta_device(ctx.get(), h_, (int64_t)run_contig.size(), run_off.data(), run_contig.data(), n_bins, d_seg_off, d_seg_left, d_seg_right,
                                      d_gc, d_entropy, d_flags, d_error, stream),
            "sbgpu_binseq_fasta_device");
   }

 private:
   FastaGenome() {}
   void load()
   {
      check(sbgpu_fasta_index(h_, &seq_off_, &offset_, &line_bases_, &line_width_, &flags_), "sbgpu_fasta_index");
      check(sbgpu_fasta_names(h_, &name_off_, &names_), "sbgpu_fasta_names");
      check(sbgpu_fasta_info(h_, info_), "sbgpu_fasta_info");
   }
   sbgpu_fasta_t *h_ = nullptr;
   const int64_t *seq_off_ = nullptr, *offset_ = nullptr, *line_bases_ = nullptr, *line_width_ = nullptr, *name_off_ = nullptr;
   const uint8_t *flags_ = nullptr;
   const char *names_ = nullptr;
   int64_t info_[16] = {};
};

} // namespace sbgpu
#endif /* SBGPU_HOST_HPP_ */
