/*
 * include/sbgpu.h -- C ABI of libsbgpu.so, the MI355X (gfx950) implementation of
 * Strawberry's per-locus EM hot path.
 *
 * The reference (ruolin/strawberry v1.1.2, /root/reference) has no plugin / FFI
 * boundary; the narrowest seam is the EmSolver class and its single call site:
 *
 *     EmSolver em;                                   include/estimate.hpp:230-257
 *     success = em.init(niso, n, alpha);             src/estimate.cpp:305-307
 *     if (success) em.run();                         src/estimate.cpp:308
 *     ... em._theta[i] ...                           src/estimate.cpp:310-329
 *
 * One call per locus would serialise the GPU, so the boundary is BATCHED: the
 * host collects the (n, alpha) of many loci into a CSR-of-loci arena, one call
 * solves them all, and the per-locus result is (theta, status, iters).  The
 * per-locus EmSolver-shaped adapter lives above this ABI (include/sbgpu_host.hpp in
 * C++14, strawberry_amd/em.py for the Python harness).
 *
 * Around that seam the same batching covers what feeds it: read pairs ->
 * unique hits (sbgpu_collapse_pairs_host), hit x isoform compatibility and exon bins
 * (sbgpu_exonbin_*, sbgpu_bins_create*), bin weights (sbgpu_binweight_*), and what follows it:
 * FPKM / Frac / TPM (sbgpu_abundance_device, sbgpu_tpm_device) and the reference's two output
 * formats (sbgpu_format_*).  sbgpu_quantify_host chains them in one call.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success and a negative SBGPU_E* code on failure (sbgpu_last_error() has the
 * text).  Per-locus outcomes are NOT errors, they are `status` values that
 * mirror the reference's bool returns.  "d_" pointers are device (HBM)
 * addresses, everything else is host memory.  `stream` is a hipStream_t passed
 * as void* (NULL = HIP's null stream, as everywhere in HIP).  A context is used from one host
 * thread at a time (one process per GPU).
 */
#ifndef SBGPU_H_
#define SBGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBGPU_VERSION_MAJOR 0
#define SBGPU_VERSION_MINOR 1

/* ---- function return codes ------------------------------------------------ */
#define SBGPU_OK 0
#define SBGPU_EINVAL (-1)   /* bad argument / malformed batch                    */
#define SBGPU_EHIP (-2)     /* a HIP runtime call failed                          */
#define SBGPU_ENODEV (-3)   /* no gfx950 device / device index out of range       */
#define SBGPU_ENOMEM (-4)   /* host or device allocation failed                   */
#define SBGPU_ESHAPE (-5)   /* a locus exceeds the supported shape (niso > 512)   */
#define SBGPU_EUNSUPPORTED (-6) /* the device form does not cover this input: use the host form (see the call) */
#define SBGPU_ERCCL (-7)    /* RCCL could not be loaded or one of its calls failed    */

/* ---- per-locus status: the reference's two bools, src/estimate.cpp:305-308 - */
#define SBGPU_EM_OK 0          /* init()==true,  run()==true, converged (estimate.cpp:480 break) */
#define SBGPU_EM_INIT_EMPTY 1  /* init()==false: no row has a weight > 1e-5 (estimate.cpp:391);
                                  theta = theta0; the caller drops the locus (alignments.cpp:1524) */
#define SBGPU_EM_DENOM_ZERO 2  /* run()==false: a row denominator was 0 (estimate.cpp:451-453);
                                  theta = theta0; the caller proceeds (bool ignored, estimate.cpp:308) */
#define SBGPU_EM_MAXITER 3     /* run()==true after all 1000 iterations (estimate.hpp:237)         */
#define SBGPU_EM_UNSOLVED (-1) /* no kernel wrote a result for the locus: what sbgpu_em_run_device sets every status
                                  to before it launches; only seen together with an SBGPU_EHIP from
                                  sbgpu_synchronize / sbgpu_em_batch / sbgpu_quantify_host (a wide-locus
                                  barrier timed out)                                                */

/* EmSolver constants, include/estimate.hpp:237,241 and src/estimate.cpp:380 */
#define SBGPU_EM_MAX_ITER 1000
#define SBGPU_EM_THETA_CHANGE_LIMIT 1e-2
#define SBGPU_EM_ROW_EPS 1e-5

typedef struct sbgpu_ctx sbgpu_ctx_t;   /* one per GPU / process */
typedef struct sbgpu_plan sbgpu_plan_t; /* shapes of one batch + its size-class schedule */

/*
 * A batch of loci in CSR-of-loci form = the arguments of EmSolver::init
 * (src/estimate.cpp:366-368: num_iso, count, model) for n_loci loci:
 *   locus l has nrow_l = row_off[l+1]-row_off[l] exon bins (rows) and
 *   niso_l = iso_off[l+1]-iso_off[l] isoforms (columns);
 *   count[row_off[l] + i]               = n_i        (vector<int> count)
 *   F[f_off[l] + i*niso_l + j]          = alpha[i][j] (vector<vector<double>> model)
 *   f_off[l+1]-f_off[l] must equal nrow_l*niso_l.
 */
typedef struct {
   int64_t n_loci;
   const int64_t *row_off; /* [n_loci+1] */
   const int64_t *iso_off; /* [n_loci+1] */
   const int64_t *f_off;   /* [n_loci+1] */
   const int32_t *count;   /* [row_off[n_loci]] */
   const double *F;        /* [f_off[n_loci]]   */
} sbgpu_batch_t;

/* Globals the reference's epilogue reads (include/common.h:25-85), passed
 * explicitly: no globals cross the ABI.                                         */
typedef struct {
   int32_t total_mapped_reads;   /* Sample::total_mapped_reads(), alignments.cpp:1372      */
   int32_t effective_len_norm;   /* common.cpp default false; estimate.cpp:317             */
   int32_t filter_by_expression; /* common.cpp default true;  estimate.cpp:346             */
   int32_t reserved;
   double insert_mean;           /* InsertSize::_mean, only read when effective_len_norm   */
   double min_isoform_frac;      /* kMinIsoformFrac: 0.01, or 0 under -r (Strawberry.cpp:158-162) */
} sbgpu_abundance_params_t;

/* ---- library / context ------------------------------------------------------ */
const char *sbgpu_version(void);
const char *sbgpu_last_error(void);
/* 16 hex digits: a hash of every source file the library was built from (csrc/Makefile).  Profiles name the build
 * they were taken with; a reader (bench.py) does not quote them for another build.                              */
const char *sbgpu_build_id(void);
int sbgpu_device_count(void);

/* Bind to HIP device `device`; creates the context's streams and workspace.
 * Concurrency.  A context (and every plan / bins handle made with it) serves ONE call at a time, from one host thread:
 * the multi-stage entry points (sbgpu_quantify_*, sbgpu_bins_create_device, sbgpu_binweight_device,
 * sbgpu_collapse_pairs_device, sbgpu_em_batch) share per-context device state -- grow-only scratch arenas, the
 * insert-size table's support, a plan's exchange buffers and epoch -- so two of them in flight on one context, even on
 * different streams, race.  Use one context per concurrent caller (contexts are cheap; one process per GPU uses one).
 * Device inputs handed to sbgpu_quantify_device / sbgpu_collapse_pairs_device must be complete when the call is made
 * (synchronise the stream that produced them): those entry points run on the context's own stream.                */
int sbgpu_init(int device, sbgpu_ctx_t **ctx_out);
int sbgpu_finalize(sbgpu_ctx_t *ctx);
/* Device memory the library keeps between calls: the arenas of handles and plans go back to a process-wide pool when they are
 * released (a sample-sized call's arenas are tens of GB; allocating and freeing them per call costs seconds), at most
 * half of the device's memory (environment: SBGPU_POOL_GB).  A caller that wants that memory for something else
 * hands it back to the driver with this; returns the bytes released.                                                  */
int64_t sbgpu_release_idle_memory(void);
/* Device facts for roofline accounting: out[0]=#CUs, out[1]=wave size,
 * out[2]=LDS bytes per CU, out[3]=max clock kHz, out[4]=total HBM bytes (MiB).   */
int sbgpu_device_info(sbgpu_ctx_t *ctx, int64_t out[8]);
int sbgpu_synchronize(sbgpu_ctx_t *ctx, void *stream);

/* ---- plan: shapes -> size classes --------------------------------------------
 * Reads only the three HOST offset arrays.  Sorts loci into (columns, rows per
 * lane, lanes per locus) size classes, orders each class by decreasing work and
 * uploads offsets + class lists.  A plan is reusable for any (count, F) of the
 * same shapes (e.g. every bench step).                                          */
int sbgpu_plan_create(sbgpu_ctx_t *ctx, int64_t n_loci, const int64_t *row_off,
                      const int64_t *iso_off, const int64_t *f_off,
                      sbgpu_plan_t **plan_out);
int sbgpu_plan_destroy(sbgpu_plan_t *plan);
/* out[0]=n_loci, out[1]=total rows, out[2]=total isoforms, out[3]=total F elements,
 * out[4]=#size classes in use, out[5]=#loci on the streaming (large-shape) path,
 * out[6]=algorithmic bytes of the batch (SURVEY 8(d) B_locus summed, fp64),
 * out[7]=#loci of out[5] served by the wide multi-workgroup kernel; the other
 * out[5] - out[7] run on the one-workgroup streaming kernel.                     */
int sbgpu_plan_info(const sbgpu_plan_t *plan, int64_t out[8]);
/* Per-class description for profiling: fills up to `cap` rows of 6 int64:
 * {kind (0 tile,1 stream), C, R, G, n_loci, n_waves}.  Returns #classes.          */
int sbgpu_plan_classes(const sbgpu_plan_t *plan, int64_t *out, int cap);

/* Which kernel serves each locus: out[l] = 0/1/2 wave kinds (half/base/double tile),
 * 3 block, 4 tall block, 5 streaming kind (profiling / roofline accounting only).  */
int sbgpu_plan_locus_kinds(const sbgpu_plan_t *plan, int8_t *out);

/* ---- the hot path: EmSolver::init + run for every locus of the plan ----------
 * Replaces src/estimate.cpp:305-308 (EmSolver::init :366-409, ::run :411-488).
 * Inputs resident in HBM; outputs written to HBM:
 *   d_theta[iso_off[n_loci]]  = em._theta of every locus (concatenated)
 *   d_status[n_loci]          = SBGPU_EM_*
 *   d_iters[n_loci]           = E-steps started (0 for INIT_EMPTY).  The reference's iteration count for status
 *                               OK and MAXITER.  UNSPECIFIED (+-1) for SBGPU_EM_DENOM_ZERO: the count of a failed
 *                               solve is not part of the reference's output, and WHEN a decaying denominator is
 *                               flushed to zero depends on one rounding -- the E-step's dot product is a chain of
 *                               fused multiply-adds (csrc/em_device.h: `sum = fma(F, theta, sum)`), in which a product
 *                               that is subnormal by itself survives, where the reference's separate multiply
 *                               (-Ofast: FTZ) flushes it: one locus in 6e5 of the stress runs sees its zero one
 *                               iteration later (theta and status identical; profiles/r05_stress.txt)
 * Asynchronous on `stream`.                                                     */
int sbgpu_em_run_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan,
                        const int32_t *d_count, const double *d_F,
                        double *d_theta, int32_t *d_status, int32_t *d_iters,
                        void *stream);

/* The same for a caller that runs batch after batch: the kernels start behind `fork_stream`'s work (the inputs) and their
 * completion is joined into `join_stream` -- the stream the caller's epilogue for THIS batch runs on -- instead of into the
 * stream they started from.  `fork_stream` is then free at once: the next call's kernels queue behind this call's on the
 * library's own streams, kind by kind, without a cross-stream hand-off between two batches (the hand-offs are ~70 us of a
 * 0.84 ms C3 step).  Two consecutive calls' kernels may run side by side (the kinds that end last alternate between two of
 * the library's streams), call i + 2's run behind call i's: the caller keeps consecutive batches' outputs apart -- theta /
 * status / iterations of call i + 1 in other buffers than call i's -- and lets `fork_stream` wait for the epilogue that
 * last read a buffer set before it hands the set to a new call.                                                          */
int sbgpu_em_run_device_split(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                              double *d_theta, int32_t *d_status, int32_t *d_iters, void *fork_stream,
                              void *join_stream);

/* The fp32 variant (BASELINE config 5, "fp32 vs fp64 tolerance sweep"): the same kernels with F, theta and all
 * arithmetic in fp32 (d_F, d_theta are float arrays; fp32 denormals flush too).  It exists to measure what
 * fp32 costs in accuracy and buys in speed; it is NOT a parity path: results differ from the reference's fp64
 * EmSolver (tools/c5_sweep.py).  Loci of up to 64 isoforms only (else SBGPU_EUNSUPPORTED).        */
int sbgpu_em_run_device_f32(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan,
                            const int32_t *d_count, const float *d_F,
                            float *d_theta, int32_t *d_status, int32_t *d_iters,
                            void *stream);

/* BASELINE config 5, "bias kernel fused into the E-step": the weight of (bin i, isoform j) is
 * F_ij * 2^(row_bias[i] * iso_bias[j]); the factor is applied to the operand while the register tile is loaded (once
 * per solve), the iterations then run on the biased tile.  d_row_bias[total rows], d_iso_bias[total isoforms], both in
 * [-1, 1] (b_ij in [0.5, 2]); how they are derived is the caller's model -- the reference has no bias arithmetic
 * (src/bias.cpp is comments), so this is NOT a parity path; bench.py --workload c5 derives row_bias from the bins'
 * GC ratio as sbgpu_binseq_device measures it.  Same result as sbgpu_em_run_device on the pre-multiplied weights up
 * to exp2's rounding.  Served by the tile kernels and the multi-workgroup kernel of the wide loci (up to 512 isoforms);
 * a plan with phases, or with a locus on the streaming fallback (a locus that would need more workgroups than the device
 * has CUs, or one of more than 64 isoforms without rows): SBGPU_EUNSUPPORTED.
 * The fp32 form covers loci of up to 64 isoforms only (it is a tolerance experiment, not a product path).              */
int sbgpu_em_run_device_bias(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                             const double *d_row_bias, const double *d_iso_bias, double *d_theta, int32_t *d_status,
                             int32_t *d_iters, void *stream);
int sbgpu_em_run_device_bias_f32(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const float *d_F,
                                 const float *d_row_bias, const float *d_iso_bias, float *d_theta, int32_t *d_status,
                                 int32_t *d_iters, void *stream);

/* Timing events around the EM kernels are off by default (they cost a few microseconds
 * per call); sbgpu_set_timing(ctx, 1) turns them on for the calls that follow.       */
int sbgpu_set_timing(sbgpu_ctx_t *ctx, int on);
/* With timing on, sbgpu_quantify_host / _device bracket each of their kernel stages (exon bins, grouping, packing,
 * pairs, bin weights, EM) with HIP events on the stream the kernels run on.  Reads the stages of the last such call
 * (waits for them): fills ms[i] / names[i] (static strings) for up to `cap` stages, returns their number or a
 * negative SBGPU_E* code.  The times are the kernels' own: host work between the stages is not in them.       */
int sbgpu_last_stage_ms(sbgpu_ctx_t *ctx, int cap, float *ms, const char **names);

/* Device time of the last sbgpu_em_run_device per kernel kind (HIP events recorded
 * on the stream each kind was launched on, all phases of the kind included):
 * ms[6] = {wave half tile, wave base tile, wave double tile, block, tall block,
 * stream}, 0 for kinds not launched or when timing is off.  Synchronises with those
 * events.                                                                          */
int sbgpu_em_last_kernel_ms(sbgpu_ctx_t *ctx, float ms[6]);

/* The wave kind runs in phases: phase 0 takes every locus up to a first iteration
 * limit, each later phase continues the loci still running in layouts with more lanes
 * per locus.  Fills ms[0 .. n) with the device time of each phase of the
 * last sbgpu_em_run_device (timing on) and returns n (0: one phase or timing off).   */
int sbgpu_em_last_phase_ms(sbgpu_ctx_t *ctx, float *ms, int cap);

/* Host-buffer convenience form (what a cgo/JNI/ctypes or the C++ driver binds
 * first): plans, uploads, solves, downloads, synchronises.                      */
int sbgpu_em_batch(sbgpu_ctx_t *ctx, const sbgpu_batch_t *host_batch,
                   double *theta_out, int32_t *status_out, int32_t *iters_out);

/* ---- abundance epilogue: theta -> FPKM / Frac / keep -------------------------
 * Replaces LocusContext::estimate_abundances, src/estimate.cpp:314-355.
 *   d_length[n_iso]  exonic length L_j of every isoform (estimate.hpp:98)
 *   d_fpkm, d_frac   [n_iso] doubles
 *   d_keep[n_iso]    0 erased (Frac < min_isoform_frac, or locus INIT_EMPTY),
 *                    1 kept, 2 kept but "NA" (effective length < 0)
 *   d_sum_fpkm[1]    = sum of FPKM over kept isoforms of this rank (the operand
 *                    of the TPM all-reduce, alignments.cpp:1821-1824); overwritten. */
int sbgpu_abundance_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan,
                           const double *d_theta, const int32_t *d_status,
                           const int32_t *d_length,
                           const sbgpu_abundance_params_t *params,
                           double *d_fpkm, double *d_frac, int32_t *d_keep,
                           double *d_sum_fpkm, void *stream);

/* TPM = 1e6 * FPKM / total_fpkm (alignments.cpp:1825-1829).  d_total_fpkm[1] is
 * the GLOBAL sum: after the RCCL all-reduce when loci are sharded over ranks.    */
int sbgpu_tpm_device(sbgpu_ctx_t *ctx, int64_t n_iso, const double *d_fpkm,
                     const int32_t *d_keep, const double *d_total_fpkm,
                     double *d_tpm, void *stream);

/* ---- the collective: loci sharded over one process per GPU -------------------------------
 * Replaces the two cross-locus sums of the reference -- `_total_mapped_reads +=`
 * (src/alignments.cpp:1372, an atomic<int> the locus threads add to) and the FPKM total
 * of Sample::procSample (src/alignments.cpp:1821-1824) -- by all-reduce(sum) over the
 * ranks: RCCL over xGMI, a few bytes, once before and once after the EM.  No locus data
 * ever crosses ranks.  Bootstrapping is the caller's (no MPI in the library): rank 0
 * makes an id with sbgpu_comm_unique_id and hands its 128 bytes to the other ranks by
 * whatever channel the driver has (a file, a socket, argv); every rank then calls
 * sbgpu_comm_init(ctx, rank, world, id) -- a collective call -- on the GPU of its ctx.
 * world == 1 needs no id (NULL) and no RCCL: its all-reduce is the identity.  (With
 * SBGPU_COMM_FORCE_RCCL=1 in the environment a world of one takes the RCCL path all the
 * same -- its own id, ncclCommInitRank(1), ncclAllReduce -- so that a one-GPU box can
 * exercise the binding; sbgpu_comm_rccl_ranks then reports 1 instead of 0.)
 * The all-reduces are in place, on device buffers, asynchronous on `stream`.             */
#define SBGPU_COMM_ID_BYTES 128
typedef struct sbgpu_comm sbgpu_comm_t;
int sbgpu_comm_unique_id(uint8_t id_out[SBGPU_COMM_ID_BYTES]);
int sbgpu_comm_init(sbgpu_ctx_t *ctx, int rank, int world, const uint8_t id[SBGPU_COMM_ID_BYTES],
                    sbgpu_comm_t **comm_out);
int sbgpu_comm_info(const sbgpu_comm_t *comm, int *rank, int *world);
/* ranks in the RCCL communicator behind `comm` (ncclCommCount); 0 when the communicator is a
 * world of one that never opened RCCL.                                                     */
int sbgpu_comm_rccl_ranks(const sbgpu_comm_t *comm, int *ranks);
int sbgpu_comm_destroy(sbgpu_comm_t *comm);
int sbgpu_allreduce_sum_f64(sbgpu_comm_t *comm, double *d_buf, int64_t n, void *stream);
int sbgpu_allreduce_sum_i64(sbgpu_comm_t *comm, int64_t *d_buf, int64_t n, void *stream);
/* The same for HOST buffers of up to 512 values (what a driver that keeps its totals on the
 * host calls: `_total_mapped_reads`, the FPKM total): staged through device memory on the
 * context's stream; returns when the result is in `buf`.                                 */
int sbgpu_allreduce_sum_f64_host(sbgpu_comm_t *comm, double *buf, int64_t n);
int sbgpu_allreduce_sum_i64_host(sbgpu_comm_t *comm, int64_t *buf, int64_t n);
/* all-reduce(max): what lets the ranks agree on the LENGTH of an array they are about to sum -- the histogram of the
 * empirical insert-size law (sbgpu_quantify_resident), whose length is the longest locus of any rank's shard.      */
int sbgpu_allreduce_max_i64(sbgpu_comm_t *comm, int64_t *d_buf, int64_t n, void *stream);
int sbgpu_allreduce_max_i64_host(sbgpu_comm_t *comm, int64_t *buf, int64_t n);
/* A communicator whose exchange is the CALLER's (a driver that already has MPI, sockets or -- the tests -- gloo, or whose
 * ranks share a GPU, which RCCL does not serve): `fn(user, buf, n, is_f64, op)` must all-reduce the n 8-byte values of the
 * HOST buffer `buf` in place over the ranks (is_f64: doubles, else int64; op 0 = sum, 1 = max) and return 0.  Every
 * sbgpu_allreduce_* call on such a communicator stages its buffer through host memory and synchronises `stream`.      */
typedef int (*sbgpu_host_allreduce_fn)(void *user, void *buf, int64_t n, int32_t is_f64, int32_t op);
int sbgpu_comm_init_host(sbgpu_ctx_t *ctx, int rank, int world, sbgpu_host_allreduce_fn fn, void *user,
                         sbgpu_comm_t **comm_out);

/* ---- bin-weight model: what fills F ----------------------------
 * Replaces LocusContext::set_theory_bin_weight, src/estimate.cpp:201-234, with
 * ExonBin::effective_len (include/isoform.h:419-516) and InsertSize::emp_dist_pdf
 * (src/read.cpp:274-297).  One work item per (exon bin, isoform) pair:
 *   seg_lens[seg_off[p] .. seg_off[p+1])  lengths of the isoform's segments the bin
 *                                         spans (<= 32), as returned through
 *                                         ExonBin::bin_under_iso (isoform.h:363-411)
 *   implicit_mask[p]                      bit k set: segment k is implicit (mate gap)
 *   iso_len[p]                            exonic length L_j (estimate.hpp:98)
 *   out_index[p]                          element of `F` that receives the weight
 *                                         (NULL: F[p]) -- lets the kernel write
 *                                         straight into an EM batch's F array      */
typedef struct {
   double mean, sd;        /* InsertSize::_mean, _sd                                   */
   int32_t use_emp;        /* InsertSize::_use_emp                                     */
   int32_t start_offset;   /* InsertSize::_start_offset (use_emp only)                 */
   int32_t end_offset;     /* InsertSize::_end_offset                                  */
   int32_t total_reads;    /* InsertSize::_total_reads                                 */
   const double *emp_hist; /* InsertSize::_emp_dist[end_offset-start_offset+1], host   */
   int32_t read_len;       /* ReadTable::read_len_mode(), include/read.hpp:150-160     */
   int32_t long_read;      /* long_read_sample: F = 1/L_j (estimate.cpp:236-247)       */
} sbgpu_insert_t;

/* pdf_out[fl] = InsertSize::emp_dist_pdf(fl) for fl in [0, n) (host arrays).      */
int sbgpu_insert_pdf_table(const sbgpu_insert_t *ins, int32_t n, double *pdf_out);

/* Device-resident form.  d_pdf[pdf_len] must cover every fragment length up to
 * the largest sum of a pair's segment lengths.  Asynchronous on `stream`.         */
int sbgpu_binweight_device(sbgpu_ctx_t *ctx, int64_t n_pairs, const int64_t *d_seg_off,
                           const uint32_t *d_seg_lens, const uint32_t *d_implicit_mask,
                           const int32_t *d_iso_len, const int64_t *d_out_index,
                           const double *d_pdf, int32_t pdf_len, int32_t read_len,
                           int32_t lmin_base, int32_t long_read, double *d_F, void *stream);

/* Host-buffer convenience form: builds the pdf table, uploads, runs, downloads
 * weight_out[p] for every pair (out_index is not used), synchronises.            */
int sbgpu_binweight_host(sbgpu_ctx_t *ctx, int64_t n_pairs, const int64_t *seg_off,
                         const uint32_t *seg_lens, const uint32_t *implicit_mask,
                         const int32_t *iso_len, const sbgpu_insert_t *ins, double *weight_out);

/* ---- exon-bin assignment, integer part --------------------------
 * Replaces the two interval tests LocusContext::assign_exon_bin (src/estimate.cpp:135-198)
 * makes for every (fragment, isoform) of a locus:
 *   Contig::is_compatible(hit, isoform)      src/contig.cpp:547-599
 *   LocusContext::overlap_exons(segs, hit)   src/estimate.cpp:115-131
 * The bookkeeping on their results (LocusContext::set_maps, include/estimate.hpp:29-52:
 * bins keyed by the set of touched segments) is host work in the caller.
 *
 * Annotation, CSR:  locus l owns isoforms iso_off[l]..iso_off[l+1]; isoform i owns exons
 * exon_off[i]..exon_off[i+1] (closed coordinates, sorted: Contig::_genomic_feats' S_MATCH
 * entries; its introns are the gaps between consecutive exons); locus l owns the disjoint
 * exon segments seg_off[l]..seg_off[l+1] (LocusContext::_exon_segs, estimate.hpp:80-91).
 * Hits, CSR: hit h belongs to locus hit_locus[h] and owns features feat_off[h]..feat_off[h+1]
 * exactly as Contig::Contig(const PairedHit&) lays them out (src/contig.cpp:216-267):
 * feat_code 0 = S_MATCH, 1 = S_INTRON, 2 = S_GAP (include/contig.h:26-31), closed
 * feat_left..feat_right, sorted; first and last are S_MATCH.
 * Results, bit words with a fixed stride per hit:
 *   compat[h*compat_words + w] bit b  <=>  is_compatible(hit h, isoform 32*w+b of its locus)
 *   key[h*key_words + w]       bit b  <=>  hit h overlaps segment 32*w+b of its locus
 * compat_words / key_words must cover the widest locus (ceil(n/32)); bits past a locus' own
 * isoforms / segments are 0.  A hit without features gets all-zero words.                 */
typedef struct {
   int64_t n_loci;
   const int64_t *iso_off;     /* [n_loci + 1]                     */
   const int64_t *exon_off;    /* [iso_off[n_loci] + 1]            */
   const uint32_t *exon_left;  /* [exon_off[n_iso]]                */
   const uint32_t *exon_right;
   const int64_t *seg_off;     /* [n_loci + 1]                     */
   const uint32_t *seg_left;   /* [seg_off[n_loci]]                */
   const uint32_t *seg_right;
} sbgpu_annotation_t;

typedef struct {
   int64_t n_hits;
   const int32_t *hit_locus;   /* [n_hits]                         */
   const int64_t *feat_off;    /* [n_hits + 1]                     */
   const uint8_t *feat_code;   /* [feat_off[n_hits]]               */
   const uint32_t *feat_left;
   const uint32_t *feat_right;
} sbgpu_hits_t;

/* Device-resident form: every pointer inside the two structs and d_compat / d_key are device
 * pointers (the structs themselves live on the host).  Asynchronous on `stream`.         */
int sbgpu_exonbin_device(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                         int32_t compat_words, int32_t key_words, uint32_t *d_compat,
                         uint32_t *d_key, void *stream);

/* Host-buffer convenience form: validates the CSR arrays (SBGPU_EINVAL / SBGPU_ESHAPE when
 * the word counts do not cover a locus), uploads, runs, downloads, synchronises.         */
int sbgpu_exonbin_host(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                       int32_t compat_words, int32_t key_words, uint32_t *compat_out,
                       uint32_t *key_out);

/* ---- exon-bin bookkeeping on the host (the callers either side) --------
 * Plain host code (no GPU work): what the reference does per locus with std::map / std::set
 * between the interval tests above and the inputs of the bin-weight and EM kernels.        */

/* The disjoint exon segments of every locus: sort + unique over the isoforms' exons, then
 * IRanges::disjoint (include/estimate.hpp:80-91, include/interval.hpp:150-191).  Fills
 * seg_off[n_loci+1] and up to `cap` entries of seg_left/seg_right (either may be NULL to
 * size the arrays first); returns the total number of segments, or a negative SBGPU_E*.   */
int64_t sbgpu_segments_host(int64_t n_loci, const int64_t *iso_off, const int64_t *exon_off,
                            const uint32_t *exon_left, const uint32_t *exon_right, int64_t *seg_off,
                            uint32_t *seg_left, uint32_t *seg_right, int64_t cap);

/* The feature list of one fragment from its mates' features (each mate: its CIGAR as
 * MATCH / INTRON features, readhit_2_genomicFeats, src/contig.cpp:12-53), as
 * Contig::Contig(const PairedHit&) builds it (src/contig.cpp:216-267): a GAP feature when the
 * mates are apart, sort + merge_genomicFeats (include/contig.h:111-137) when they touch or
 * overlap; n_left or n_right may be 0 (single read).  The out arrays need room for
 * n_left + n_right + 1 features.  Returns the number of features, 0 when the reference
 * rejects the pair ("paired reads ... are not compatible", estimate.hpp:71-79), negative
 * SBGPU_E* on a bad argument.                                                              */
int sbgpu_hit_features(int n_left, const uint8_t *lcode, const uint32_t *lleft, const uint32_t *lright,
                       int n_right, const uint8_t *rcode, const uint32_t *rleft, const uint32_t *rright,
                       uint8_t *code_out, uint32_t *left_out, uint32_t *right_out);

/* The sample of the empirical insert-size distribution, Sample::fragLenDist's inner loop
 * (src/alignments.cpp:1381-1407): frag_len_out[h] = Contig::exonic_overlaps_len(t, hit.left(),
 * hit.right()) (src/contig.cpp:412-426) when hit h is compatible with exactly ONE transcript t of
 * its locus, else -1.  `compat` is the kernel's result (host copy).  Returns how many hits got a
 * length; InsertSize(frag_lens) (src/read.cpp:238-262) takes them in hit order.              */
int64_t sbgpu_frag_lens_host(const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                             int32_t compat_words, const uint32_t *compat, int32_t *frag_len_out);

/* ---- from aligned read pairs to unique hits (host code) ----------------------
 * HitCluster::collapseAndFilterHits (src/alignments.cpp:656-703) followed by Contig(PairedHit) for
 * every unique hit, for the clusters (loci) of a batch:
 *   - pairs of a locus are ordered by (left end, right end) of the pair (src/read.cpp:917-923); the
 *     reference uses std::sort there, ties keep their input order here;
 *   - a pair one of whose mates spans more than mean + 15.45 sd of the locus' mate spans is skipped
 *     (phi((len - mean) / (5 sd)) > 0.999, :667-682; spans of all mates, population sd, common.h:100-110);
 *   - the others add their raw mass to the cluster's mass (:683-684) and are collapsed with the
 *     previous unique hit when both mates are equal -- same start, same CIGAR (:685-697,
 *     src/read.cpp:196-207,897-910) -- summing the masses in double;
 *   - every unique hit becomes features through sbgpu_hit_features; a rejected one (0 features) is
 *     dropped, its mass stays in the cluster's mass.
 * A mate is its MATCH / INTRON features (readhit_2_genomicFeats); a missing mate has no features.
 * pair_mass[p] is the pair's raw mass: 0.5 / NH per mate of a proper pair, 1 / NH for a singleton
 * (src/read.cpp:49-53,116-123).                                                                  */
typedef struct {
   int64_t n_pairs;
   const int32_t *pair_locus;  /* [n_pairs]                                  */
   const double *pair_mass;    /* [n_pairs]                                  */
   const int64_t *left_off;    /* [n_pairs + 1] into the left mates' features  */
   const uint8_t *left_code;
   const uint32_t *left_left, *left_right;
   const int64_t *right_off;   /* [n_pairs + 1] into the right mates' features */
   const uint8_t *right_code;
   const uint32_t *right_left, *right_right;
} sbgpu_pairs_t;
typedef struct sbgpu_uniq sbgpu_uniq_t;
int sbgpu_collapse_pairs_host(int64_t n_loci, const sbgpu_pairs_t *pairs, sbgpu_uniq_t **out);
void sbgpu_uniq_destroy(sbgpu_uniq_t *u);
/* info: 0 unique hits kept, 1 their features, 2 pairs skipped by the span filter, 3 unique hits
 * rejected by Contig(PairedHit), 4 total mapped reads = sum over loci of (int) cluster mass
 * (src/alignments.cpp:1372).                                                                 */
int sbgpu_uniq_info(const sbgpu_uniq_t *u, int64_t info[8]);
/* The unique hits as an sbgpu_hits_t's arrays (+ hit_mass = (float) collapse mass, cluster_mass
 * [n_loci] in double); NULL = skip.                                                           */
int sbgpu_uniq_export(const sbgpu_uniq_t *u, int32_t *hit_locus, int64_t *feat_off, uint8_t *feat_code,
                      uint32_t *feat_left, uint32_t *feat_right, float *hit_mass, double *cluster_mass);

/* The same on the GPU (csrc/collapse_flat.h): the pairs' arrays of `d_pairs` are DEVICE pointers (pair_locus is
 * not read), grouped by locus as locus_pair_off[n_loci + 1] (host) says; the unique hits stay in HBM in
 * sbgpu_hits_t layout -- sbgpu_uniq_dev_hits hands them to sbgpu_exonbin_device / sbgpu_quantify_device -- and
 * only the per-locus offsets and cluster masses come back.  All clusters of the call at once: one stable device-wide
 * radix sort (two where its key would not fit 64 bits) gives the (left, right) order with ties in input order; the span
 * filter is decided from the spans' exact
 * integer moments (the reference's running sum of squared deviations is taken where a decision could depend on its
 * rounding); equal neighbours collapse, their masses added in double in that order (in any order where every mass
 * of the cluster is a multiple of 2^-20: the sums are then exact); Contig(PairedHit)'s features per unique hit.
 * Up to 2^31 pairs per call and mates of up to 512 features; beyond: SBGPU_EUNSUPPORTED (use
 * sbgpu_collapse_pairs_host).  Synchronises on `stream`.
 * The span filter evaluates phi() with the device's exp(): a pair exactly on the 0.999 boundary could fall on the
 * other side than with the host's libm (not observed).                                                        */
typedef struct sbgpu_uniq_dev sbgpu_uniq_dev_t;
int sbgpu_collapse_pairs_device(sbgpu_ctx_t *ctx, int64_t n_loci, const sbgpu_pairs_t *d_pairs,
                                const int64_t *locus_pair_off, void *stream, sbgpu_uniq_dev_t **out);
void sbgpu_uniq_dev_destroy(sbgpu_uniq_dev_t *u);
/* info as sbgpu_uniq_info */
int sbgpu_uniq_dev_info(const sbgpu_uniq_dev_t *u, int64_t info[8]);
/* The unique hits where they are: *d_hits gets device pointers, *d_hit_mass the (float) collapse masses
 * (device), *locus_hit_off [n_loci + 1] (host): the arguments of sbgpu_quantify_device.  Owned by the handle. */
int sbgpu_uniq_dev_hits(const sbgpu_uniq_dev_t *u, sbgpu_hits_t *d_hits, const float **d_hit_mass,
                        const int64_t **locus_hit_off);
/* Host copies (as sbgpu_uniq_export; NULL = skip). */
int sbgpu_uniq_dev_export(const sbgpu_uniq_dev_t *u, int32_t *hit_locus, int64_t *feat_off, uint8_t *feat_code,
                          uint32_t *feat_left, uint32_t *feat_right, float *hit_mass, double *cluster_mass);

/* ---- cluster streaming: which cluster does an alignment record belong to ---------------
 * Sample::nextClusterRefDemand (src/alignments.cpp:1145-1187, quant mode: the clusters are the annotation's genes, in
 * annotation order = sorted by (reference, left)): ONE forward pass over the position-sorted records.  For cluster k
 * the pass resumes where cluster k - 1 stopped; a record that ends before the cluster begins (or lies on an earlier
 * reference) is skipped for good (hit_lt_cluster, :32-37); a record that begins behind the cluster's end (or on a
 * later reference) ends the cluster and is looked at again for the next one (hit_gt_cluster, :39-49); of the others,
 * those whose transcription strand (XS) is known and differs from the cluster's are dropped, the rest join the
 * cluster (addOpenHit).  A record is therefore offered to exactly one cluster -- the first whose end it does not
 * lie behind -- even where genes overlap.
 *   clusters (HOST arrays): reference id, [left, right] and strand (1 +, 2 -, 0 unknown) of every cluster, in order;
 *   records: reference id, first and last aligned base, flags (bits 2-3: XS strand as in sbgpu_reads_t), sorted by
 *   (reference, left) as the BAM is.
 * Out: read_cluster[i] = the record's cluster or -1, and cluster_read_off[n_clusters + 1] (host): cluster k was offered
 * the records [off[k], off[k + 1]) -- the ones with read_cluster == k among them are its members, in arrival order;
 * with `flags_inout` given, the others get SBGPU_READ_SKIP set, so that range is sbgpu_pair_mates_*'s input as it
 * stands.  Device form: one binary search per cluster, a prefix maximum on the host (clusters are few), one binary
 * search per record.                                                                                            */
typedef struct {
   int64_t n_clusters;
   const int32_t *ref;
   const uint32_t *left, *right;
   const uint8_t *strand;
} sbgpu_clusters_t;
#define SBGPU_READ_SKIP 16u /* (sbgpu_reads_t.flags) the record is not this cluster's: sbgpu_pair_mates_* pass over it */
int sbgpu_assign_reads_host(const sbgpu_clusters_t *clusters, int64_t n_reads, const int32_t *read_ref, const uint32_t *read_left,
                            const uint32_t *read_right, uint8_t *flags_inout, int32_t *read_cluster, int64_t *cluster_read_off);
int sbgpu_assign_reads_device(sbgpu_ctx_t *ctx, const sbgpu_clusters_t *clusters, int64_t n_reads, const int32_t *d_read_ref,
                              const uint32_t *d_read_left, const uint32_t *d_read_right, uint8_t *d_flags_inout,
                              int32_t *d_read_cluster, int64_t *cluster_read_off, void *stream);

/* ---- mate pairing: alignment records -> read pairs --------------------------------------
 * HitCluster::addOpenHit + addHit (src/alignments.cpp:423-655): the records of a cluster, in the order the
 * position-sorted BAM gives them, become PairedHits.
 *   - a record whose span exceeds kMaxFragSpan (1 000 000, src/common.cpp:17) is refused (:512-518);
 *   - a record without a partner (partner_pos 0) or with its partner on another reference is a hit of its own: the
 *     RIGHT mate of a pair without a left one when it is on the reverse strand, else the left mate (:535-545);
 *   - otherwise the cluster's open mates of the same read id are searched, oldest first, for one that starts where
 *     this record's partner starts, expects its partner where this record starts and whose strand (XS) agrees or is
 *     unknown on either side (:590-623): the pair is complete and joins the cluster's hits NOW (the order of the hits
 *     = the order in which pairs are completed); else the record waits as an open mate -- the left one when its
 *     partner lies behind it, the right one when before it; a record whose partner starts where it starts is
 *     refused (:559-585, 630-641);
 *   - what still waits when the cluster is closed is dropped (clearOpenMates, :653).
 * Pair mass: the two reads' masses, 0.5 / NH each; a single read's 1 / NH (src/read.cpp:49-53).
 * The result has the layout of sbgpu_pairs_t -- mates as MATCH / INTRON feature lists (readhit_2_genomicFeats, src/contig.cpp:12-53:
 * an INTRON between two blocks, none where they touch -- an insertion in the read) --:
 * the input of sbgpu_collapse_pairs_host / _device.  One difference a caller should know: the reference's cluster
 * keeps the span of EVERY accepted record for its span filter (:527), the collapse here sees the spans of the
 * mates of the pairs only -- records that never find their mate do not count.                                   */
typedef struct {
   int64_t n_reads;
   const uint64_t *read_id;      /* [n_reads] ReadTable::get_id(read name): the mates of a pair share it      */
   const int64_t *block_off;     /* [n_reads + 1] the record's aligned blocks (the M runs of an M / N CIGAR)  */
   const uint32_t *block_left, *block_right; /* closed coordinates, ascending                                 */
   const uint32_t *partner_pos;  /* [n_reads] where the mate starts; 0: none                                  */
   const uint8_t *flags;         /* [n_reads] bit 0: reverse strand (BAM_FREVERSE); bit 1: the partner lies on
                                    another reference; bits 2-3: transcription strand (XS) 0 unknown, 1 +, 2 - */
   const int32_t *nh;            /* [n_reads] NH tag                                                          */
} sbgpu_reads_t;
#define SBGPU_READ_REVERSE 1u
#define SBGPU_READ_PARTNER_ELSEWHERE 2u
typedef struct sbgpu_matepairs sbgpu_matepairs_t;
/* Host form: `reads` host arrays, the records of cluster l are [locus_read_off[l], locus_read_off[l + 1]). */
int sbgpu_pair_mates_host(int64_t n_loci, const sbgpu_reads_t *reads, const int64_t *locus_read_off, sbgpu_matepairs_t **out);
/* Device form (csrc/matepair_flat.h): `d_reads` device arrays, locus_read_off host.  All clusters of the call at once:
 * one stable device-wide radix sort on a 32-bit key (a group of neighbouring clusters, then a hash of (cluster, read id))
 * brings a read id's records together in arrival order, the first record of every read id walks its group with the
 * reference's open-mate rules (any number of mates of one read id may wait), a compaction of the completing records in
 * arrival order ranks the pairs, and the pairs are written where sbgpu_collapse_pairs_device reads them -- nothing but
 * per-cluster offsets and four counters comes back.
 * Up to 2^31 records and 2^23 clusters per call; beyond: SBGPU_EUNSUPPORTED.                                        */
int sbgpu_pair_mates_device(sbgpu_ctx_t *ctx, int64_t n_loci, const sbgpu_reads_t *d_reads, const int64_t *locus_read_off,
                            void *stream, sbgpu_matepairs_t **out);
void sbgpu_matepairs_destroy(sbgpu_matepairs_t *m);
/* info: 0 pairs (single reads included), 1 complete pairs, 2 single reads, 3 records refused, 4 records that never
 * found their mate, 5 features of the left mates, 6 of the right mates, 7: 0 host arrays; else bit 0 set (the arrays live on
 * the device), bit 1: the positional matching served the call (no sort: the records of every cluster ascend by position and
 * no read id is aligned twice in a cluster), else bits 2.. say why the sorted form did: 1 records not in position order,
 * 2 a read id with more than one fitting mate (0: SBGPU_PAIR_FORCE_SORT).                                                */
int sbgpu_matepairs_info(const sbgpu_matepairs_t *m, int64_t info[8]);
/* The pairs where they are (host or device arrays, see info[7]) + locus_pair_off [n_loci + 1] (host): the arguments
 * of sbgpu_collapse_pairs_host / _device.  pair_locus is set for the host form only.  Owned by the handle.      */
int sbgpu_matepairs_pairs(const sbgpu_matepairs_t *m, sbgpu_pairs_t *pairs, const int64_t **locus_pair_off);
/* Host copies of everything (NULL = skip): pair_mass [pairs], left_off / right_off [pairs + 1], the feature arrays. */
int sbgpu_matepairs_export(const sbgpu_matepairs_t *m, double *pair_mass, int64_t *left_off, uint8_t *left_code,
                           uint32_t *left_left, uint32_t *left_right, int64_t *right_off, uint8_t *right_code,
                           uint32_t *right_left, uint32_t *right_right);

/* ---- BAM alignment records -> the read stream (replaces BAMHitFactory::getHitFromBuf) --------
 * /root/reference/src/read.cpp:480-715: a BAM record becomes a ReadHit -- or is refused -- on its flag word, its CIGAR,
 * the XS / NM / NH tags and four option globals.  In: the UNCOMPRESSED record stream behind the BAM header (what
 * samtools' bam_read1 reads after BGZF inflate: the BGZF section below): per record int32 block_size, the 32-byte
 * core, read name, CIGAR, sequence, qualities, tags.  Out: the accepted records, in file order, as the arrays
 * sbgpu_assign_reads_* and sbgpu_pair_mates_* take, plus why each of the others was refused.
 *   - refused: unmapped (flag 0x4 or no reference); a CIGAR operation of length 0; an operation other than M I D N S H P;
 *     an N outside [min_intron, max_intron]; an I or D that is not between two M, or that is among the first two operations
 *     the reference keeps (H and P are not kept: "10M2I10M" is refused, "3S10M2I10M" is not -- the reference's `i-1 <= 0`,
 *     :594); at most one aligned base; NH > 1 or a secondary alignment while unique_only;
 *   - interval [pos + 1, pos + M + D + N lengths], 1-based closed; blocks = the M runs, a D extends the block before it,
 *     an I leaves two blocks that touch (readhit_2_genomicFeats, src/contig.cpp:12-53: no INTRON between them);
 *   - flags as sbgpu_reads_t's: bit 0 reverse (the record's 0x10), bit 1 partner on another reference (the mate's id differs;
 *     no mate reference included), bits 2-3 the strand: from XS:A ('+' / '-'), else from the library type and the
 *     first-in-pair / reverse bits (:636-651);
 *   - read id = FNV-1 of the read name (ReadTable::get_id, include/read.hpp:164-173); reference id = the file's (the
 *     reference numbers the @SQ lines in order); partner_pos = mate position + 1 (0: none); NH 1 when absent; NM as the
 *     reference keeps it (through an unsigned char); read_len = M + S + I (ReadHit::read_len);
 *   - tags are found as samtools 0.1.19 finds them (external/samtools-0.1.19/bam_aux.c:28-47): a `d` value is stepped over as
 *     if it had no payload; no read leaves the record (a record whose own lengths exceed its block_size: TRUNCATED).  */
typedef struct {
   int32_t min_intron;  /* kMinIntronLength, 20 (src/common.cpp:21; -j)                     */
   int32_t max_intron;  /* kMaxIntronLength, 300000 (src/common.cpp:20; -J)                 */
   int32_t unique_only; /* use_only_unique_hits, 1 (src/common.cpp:67; --allow-multimapped-hits: 0)   */
   int32_t library;     /* 0 unstranded, 1 fr_strand, 2 rf_strand (src/common.cpp:68-69)    */
   int32_t n_ref;       /* references in the header: a larger id is refused; 0: not checked */
} sbgpu_bam_opts_t;
enum {
   SBGPU_BAM_OK = 0,
   SBGPU_BAM_UNMAPPED = 1,
   SBGPU_BAM_BAD_REF = 2,
   SBGPU_BAM_ZERO_OP = 3,
   SBGPU_BAM_OP = 4,
   SBGPU_BAM_INTRON_LONG = 5,
   SBGPU_BAM_INTRON_SHORT = 6,
   SBGPU_BAM_INDEL = 7,
   SBGPU_BAM_SHORT = 8,
   SBGPU_BAM_MULTI = 9,
   SBGPU_BAM_TRUNCATED = 10
};
typedef struct sbgpu_bamreads sbgpu_bamreads_t;
/* The records' offsets in the stream: rec_off[0 .. n] (rec_off[n] = n_bytes).  Returns n, or -1 (sbgpu_last_error) when
 * the stream ends inside a record or `cap` records are not enough.  A caller that inflates BGZF blocks itself can note
 * the offsets as it goes instead.                                                                                     */
int64_t sbgpu_bam_index_host(const uint8_t *bytes, int64_t n_bytes, int64_t *rec_off, int64_t cap);
/* Host form: host arrays in, host arrays in the handle. */
int sbgpu_bam_decode_host(const uint8_t *bytes, int64_t n_bytes, const int64_t *rec_off, int64_t n_records,
                          const sbgpu_bam_opts_t *opts, sbgpu_bamreads_t **out);
/* Device form (csrc/bamdecode_device.h): `d_bytes` and `d_rec_off` device arrays; one lane per record decides and counts
 * its blocks, two scans over the waves' totals place the accepted records and their blocks, a second pass writes them.  The
 * handle's arrays stay on the device: sbgpu_bamreads_reads hands them to sbgpu_assign_reads_device /
 * sbgpu_pair_mates_device as they are.  A record whose offsets do not ascend inside [0, n_bytes] is TRUNCATED, not read.                                                                                */
int sbgpu_bam_decode_device(sbgpu_ctx_t *ctx, const uint8_t *d_bytes, int64_t n_bytes, const int64_t *d_rec_off, int64_t n_records,
                            const sbgpu_bam_opts_t *opts, void *stream, sbgpu_bamreads_t **out);
void sbgpu_bamreads_destroy(sbgpu_bamreads_t *b);
/* info: 0 records, 1 accepted, 2 aligned blocks of the accepted, 3: 1 when some record that got as far as the
 * reference's :605 carries the paired flag (the reference then clears SINGLE_END_EXP), 4: 1 when the arrays live on the
 * device, 5 + s: records of status s (SBGPU_BAM_OK .. SBGPU_BAM_TRUNCATED).                                            */
int sbgpu_bamreads_info(const sbgpu_bamreads_t *b, int64_t info[16]);
/* The accepted records where they are (host or device, info[4]): `reads` for sbgpu_pair_mates_*, and reference id /
 * first / last aligned base for sbgpu_assign_reads_*.  Owned by the handle.                                            */
int sbgpu_bamreads_reads(const sbgpu_bamreads_t *b, sbgpu_reads_t *reads, const int32_t **read_ref, const uint32_t **read_left,
                         const uint32_t **read_right);
/* Host copies (NULL = skip): status [records]; per accepted record its index in the stream, read id, reference, interval,
 * partner_pos, flags, NH, NM, read_len, the record's flag word; block_off [accepted + 1], the blocks.                  */
int sbgpu_bamreads_export(const sbgpu_bamreads_t *b, uint8_t *status, int64_t *record, uint64_t *read_id, int32_t *ref, uint32_t *left,
                          uint32_t *right, uint32_t *partner_pos, uint8_t *flags, int32_t *nh, int32_t *nm, int32_t *read_len,
                          uint32_t *sam_flag, int64_t *block_off, uint32_t *block_left, uint32_t *block_right);

/* ---- BGZF: a BAM file's own bytes -> the inflated stream and its records (csrc/bgzf_device.h, bgzf_host.cpp, bgzf_api.hip) ----
 * A BGZF file is a chain of independent gzip members of at most 64 KiB, each with its compressed size in its header (BSIZE)
 * and its inflated size in its footer (ISIZE): samtools 0.1.19 bgzf.c.  The library inflates them itself -- no zlib is
 * linked -- with one RFC 1951 decoder (stored, fixed and dynamic blocks, any number of blocks per member, distances up to
 * 32768, matches that overlap their own output) that runs per host thread or per wave of the device.
 *
 * The block table: blk_off[0 .. n] where every member starts in the file (blk_off[n] = n_bytes), out_off[0 .. n] the running
 * sum of the ISIZE words: where every member's bytes land in the inflated stream.  Returns n, or -1 (sbgpu_last_error) when a
 * header fails the reference's check_header (bgzf.c:240-246: magic 31 139 8, FLG & 4, XLEN == 6, subfield 'B' 'C' of length 2;
 * those tests and no others), when the file ends inside a member, when ISIZE > 65536 or BSIZE leaves no room for the
 * 8-byte footer, or when there are more than `cap` members.  A member with ISIZE 0 (the EOF marker) is an ordinary entry.  */
int64_t sbgpu_bgzf_index_host(const uint8_t *file, int64_t n_bytes, int64_t *blk_off, int64_t *out_off, int64_t cap);
/* Inflate.  Member b's payload is file[blk_off[b] + 18 .. blk_off[b + 1] - 8); its bytes go to out[out_off[b] .. out_off[b + 1])
 * (`out` is the origin of the out_off coordinates, whichever members a call covers).  A member is SBGPU_BGZF_OK iff zlib's raw
 * inflate of the same payload reaches the end of the stream AND gives exactly out_off[b + 1] - out_off[b] bytes; otherwise its
 * status says why.  The reference (bgzf.c:214-238) accepts a member whose ISIZE lies; this library lays the output out by
 * ISIZE and refuses it (SBGPU_BGZF_ESIZE).  Neither checks the CRC-32 word, and bytes of the payload behind the final block
 * are ignored, as zlib ignores them.  A failed member never writes outside its own output range and never reads outside its
 * own bytes of the file; its neighbours are unaffected.  Host and device form take the same decisions (the same decoder),
 * statuses included.  The calls return SBGPU_OK when members failed -- the statuses are the report -- and SBGPU_EINVAL for
 * bad arguments.                                                                                                          */
enum {
   SBGPU_BGZF_OK = 0,
   SBGPU_BGZF_EBTYPE = 1,   /* a block of the reserved type 3                                                              */
   SBGPU_BGZF_ESTORED = 2,  /* a stored block whose LEN and NLEN disagree                                                  */
   SBGPU_BGZF_ECODELEN = 3, /* a dynamic block's code lengths: over-subscribed or incomplete set, more than 286 / 30 codes,
                               a repeat with nothing to repeat or past the last length, no end-of-block code               */
   SBGPU_BGZF_ESYMBOL = 4,  /* a code that stands for no symbol, length symbol 286 / 287, distance symbol 30 / 31           */
   SBGPU_BGZF_EDIST = 5,    /* a distance that reaches before the member's first byte                                      */
   SBGPU_BGZF_EINPUT = 6,   /* the payload ran out (also: a member shorter than header + footer or longer than 65536)      */
   SBGPU_BGZF_ESIZE = 7     /* the output is not ISIZE bytes (also: an out_off range that is negative or exceeds 65536)    */
};
/* Host form: members first_block .. first_block + n_blocks - 1 on host threads (SBGPU_HOST_THREADS, default min(16,
 * hardware threads)); status[0 .. n_blocks) belongs to those members in order.                                            */
int sbgpu_bgzf_inflate_host(const uint8_t *file, int64_t n_bytes, const int64_t *blk_off, const int64_t *out_off, int64_t first_block,
                            int64_t n_blocks, uint8_t *out, uint8_t *status);
/* Device form: all arrays in device memory, one member per wave, launched on `stream` (NULL: the context's).  *n_failed
 * (host; may be NULL) is the number of members with a nonzero status: asking for it makes the call wait for the stream,
 * without it the call returns when the kernel is launched.                                                               */
int sbgpu_bgzf_inflate_device(sbgpu_ctx_t *ctx, const uint8_t *d_file, int64_t n_bytes, const int64_t *d_blk_off,
                              const int64_t *d_out_off, int64_t n_blocks, uint8_t *d_out, void *stream, uint8_t *d_status,
                              int64_t *n_failed);
/* The records' offsets of an inflated stream that lives on the device: what sbgpu_bam_index_host gives on the bytes from
 * `first_record` (the header's length) on -- d_rec_off[0 .. n] are RELATIVE to first_record, d_rec_off[n] = n_bytes -
 * first_record, so sbgpu_bam_decode_device takes d_bytes + first_record with them -- including the -1 when the chain meets a
 * negative size word, ends inside a record, or holds more than `cap` records.  Exact for any input.  `d_guess[0 .. n_guess)`
 * (ascending; NULL: every 65536 bytes) are offsets in d_bytes where a record PROBABLY starts -- the out_off of the block table:
 * samtools starts every member on a record boundary -- and only buy speed: the chain of size words is cut there and every
 * segment is walked in parallel from its guess.  Then, round after round, a segment whose entry is not where its predecessor's
 * walk ended is walked again from there, provided that predecessor's own entry was right in the same sense (the exit of a
 * segment that is itself about to be walked again is noise and is not passed on); a round that repairs nothing has found the
 * true chain, and after 8 repairing rounds one lane walks what is left in order (slow, exact).  Waits for the stream.     */
int64_t sbgpu_bam_index_device(sbgpu_ctx_t *ctx, const uint8_t *d_bytes, int64_t n_bytes, int64_t first_record, const int64_t *d_guess,
                               int64_t n_guess, int64_t *d_rec_off, int64_t cap, void *stream);
/* About this thread's last sbgpu_bam_index_device call: info[0] rounds of walks (1: every guess was right), info[1] segments,
 * info[2] walks repeated, info[3] the segment the sequential walker started at (-1: it did not run); info[4 .. 8) zero.    */
void sbgpu_bam_index_device_info(int64_t *info);

/* LocusContext::assign_exon_bin + set_maps (src/estimate.cpp:135-198, estimate.hpp:29-52)
 * on the kernel's results (host copies of compat / key), hits visited in input order inside
 * each locus (= HitCluster::uniq_hits() order):
 *   - a hit with no compatible isoform is dropped;
 *   - bins are keyed by `key` and numbered in order of first appearance
 *     (UniqPushAndReturnIdx);
 *   - a bin's count is ExonBin::read_count (include/isoform.h:285-296): fragments with the
 *     same (offset, length) feature sequence count once (std::set<Contig>, first one wins),
 *     masses are added in float in that set's order and truncated to int (estimate.cpp:288);
 *   - a bin is paired with every isoform some hit of it is compatible with; for each pair
 *     ExonBin::bin_under_iso (include/isoform.h:363-411) yields the bin-weight kernel's
 *     segment lengths and implicit mask, and pair_out_index its element of the EM batch's F.
 * hit_mass[h] = (float) PairedHit::collapse_mass().  The handle owns the results.          */
typedef struct sbgpu_bins sbgpu_bins_t;
int sbgpu_bins_create(const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits, const float *hit_mass,
                      int32_t compat_words, int32_t key_words, const uint32_t *compat,
                      const uint32_t *key, sbgpu_bins_t **out);
/* The same bins with the per-hit work on the GPU (csrc/bins_device.h): one workgroup per locus
 * groups its hits through a hash table in LDS, ranks the bins by first appearance, accumulates
 * compat unions and masses; only the per-bin arrays come back to the host, where the (bin, isoform)
 * pairs are made as in sbgpu_bins_create.  `annot` holds HOST pointers (the pairs need the
 * annotation on the host); d_hits' pointers, d_hit_mass, d_compat and d_key are DEVICE pointers
 * (the kernel's inputs and results never leave HBM); locus_hit_off[n_loci+1] (host) says where each
 * locus' hits start -- hits must be grouped by locus.  d_hit_bin (device, [n_hits], may be NULL)
 * receives the global bin of every hit; the handle's own hit_bin stays empty.
 * The device form is exact only where the order of the reference's float accumulation cannot
 * matter, and it checks that: hits of a locus sorted by (left end, right end) (HitCluster's order),
 * whole-number masses below 2^24 per bin (the reference's default: no multi-mapped reads), at most
 * 5600 bins per locus.  Otherwise it returns SBGPU_EUNSUPPORTED and the caller uses
 * sbgpu_bins_create.  Synchronises on `stream`.                                                  */
int sbgpu_bins_create_device(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                             const float *d_hit_mass, const int64_t *locus_hit_off, int32_t compat_words,
                             int32_t key_words, const uint32_t *d_compat, const uint32_t *d_key,
                             int64_t *d_hit_bin, void *stream, sbgpu_bins_t **out);
void sbgpu_bins_destroy(sbgpu_bins_t *bins);
/* info: 0 n_loci, 1 n_iso, 2 n_bins, 3 n_elem (= f_off[n_loci]), 4 n_pairs, 5 total pair
 * segments, 6 hits that landed in a bin, 7 key_words.                                      */
int sbgpu_bins_info(const sbgpu_bins_t *bins, int64_t info[8]);
/* Which grouping made the handle's bins: *on_device = 1 the device kernels (sbgpu_bins_create_device, or the device stage of
 * sbgpu_quantify_host / _device), 0 the library's host code (sbgpu_bins_create).  sbgpu_quantify_host takes the host code
 * when the device form declines (SBGPU_EUNSUPPORTED above); *why_host (optional) then points at the reason, a string owned
 * by the handle ("" when the host code was simply what the caller called).  The results are the same either way; the
 * host path is slower, so a caller that cares can tell.                                                              */
int sbgpu_bins_grouping(const sbgpu_bins_t *bins, int32_t *on_device, const char **why_host);
/* Copies out what the caller asks for (NULL = skip).  The first five arrays are exactly an
 * sbgpu_batch_t minus F (row_off/iso_off/f_off [n_loci+1], count [n_bins]) plus iso_len
 * [n_iso]; bin_key [n_bins*key_words], bin_compat [n_bins*compat_words], hit_bin [n_hits]
 * (global bin of each hit, -1 = dropped); the pair arrays are sbgpu_binweight_device's
 * inputs ([n_pairs+1], [total pair segments], [n_pairs] x3).                               */
int sbgpu_bins_export(const sbgpu_bins_t *bins, int64_t *row_off, int64_t *iso_off, int64_t *f_off,
                      int32_t *count, int32_t *iso_len, uint32_t *bin_key, uint32_t *bin_compat,
                      int64_t *hit_bin, int64_t *pair_seg_off, uint32_t *pair_seg_lens,
                      uint32_t *pair_implicit_mask, int32_t *pair_iso_len, int64_t *pair_out_index);

/* ---- the whole path in one call: fragments -> exon bins -> bin weights -> EM ------------------
 * LocusContext's constructor + the EM of estimate_abundances for every locus of a batch
 * (include/estimate.hpp:60-103, src/estimate.cpp:279-308), host buffers in, host buffers out:
 * uploads the annotation and the hits once, runs sbgpu_exonbin_device, groups the hits into bins
 * on the device (with the library's host code, sbgpu_bins_create, when the device form declines --
 * hits that do not come grouped by locus, ...: same bins, slower; sbgpu_bins_grouping says which ran
 * and why), builds the pairs, runs
 * sbgpu_binweight_device straight into the EM batch's F, plans and runs sbgpu_em_run_device.
 * Nothing but the per-bin arrays, theta and (on request) F comes back over PCIe.
 *   annot          host arrays incl. the segments (sbgpu_segments_host)
 *   hits, hit_mass host arrays; hits grouped by locus and, inside a locus, in uniq_hits() order
 *   insert         the insert-size law (-i); NULL = none given: the empirical distribution is built
 *                  from the hits first (Sample::fragLenDist, src/alignments.cpp:1363-1407,
 *                  Strawberry.cpp:345-355) and written to *insert_used with emp_hist pointing into
 *                  the returned handle
 *   theta_out [n_iso], status_out / iters_out [n_loci]   as sbgpu_em_batch
 *   compat_out [n_hits * ceil(max isoforms / 32)]  optional (NULL): the kernel's compat words
 *   *bins_out      the bins (sbgpu_bins_info / _export, incl. hit_bin; sbgpu_bins_export_weights
 *                  for F); destroy with sbgpu_bins_destroy
 * The caller applies the reference's own epilogue to theta (src/estimate.cpp:310-355).          */
int sbgpu_quantify_host(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                        const float *hit_mass, const sbgpu_insert_t *insert, int32_t read_len,
                        int32_t long_read, double *theta_out, int32_t *status_out, int32_t *iters_out,
                        uint32_t *compat_out, sbgpu_insert_t *insert_used, sbgpu_bins_t **bins_out);
/* Keep an annotation resident.  The reference reads its GTF once and streams the reads past it
 * (src/Strawberry.cpp:245-275: one GffReader, loadRefmRNAs; :359: Sample::procSample over every cluster); a driver that calls
 * sbgpu_quantify_host / _device batch after batch against the same annotation pins it once: the arrays are uploaded
 * now, the tables the chain makes of an annotation alone (the isoforms' segment lists, the widest locus) are made
 * now, and every later call on this context that is given an annotation with the SAME counts and array addresses uses
 * them instead of uploading 10+ MB and rebuilding the tables per call.  The caller must not change the arrays while
 * they are pinned (they are not compared).  One annotation per context: pinning another replaces it; unpin (or
 * sbgpu_destroy) releases it.  Results are those of the unpinned call, bit for bit.                                    */
int sbgpu_annotation_pin(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot);
int sbgpu_annotation_unpin(sbgpu_ctx_t *ctx);
/* The owner's form of unpin: releases the context's pin only if it is the pin of THESE arrays (addresses and counts; the
 * arrays are not read).  Several objects may share a context and each pin its own annotation, the later pin replacing
 * the earlier: the earlier owner's release must then leave the later pin alone (sbgpu_annotation_unpin would drop it and
 * every later call would quietly go back to uploading the annotation).  *released (may be NULL): 1 if a pin went.      */
int sbgpu_annotation_unpin_matching(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, int32_t *released);
/* The same chain for hits that are in HBM already (a driver that decodes or collapses on the device, or
 * that quantifies the same fragments again): d_hits' arrays and d_hit_mass are DEVICE pointers, grouped by
 * locus as locus_hit_off[n_loci + 1] (host) says and sorted inside a locus like HitCluster's uniq_hits();
 * `annot` holds host pointers; insert == NULL builds the empirical law on the device (see sbgpu_quantify_resident, which
 * also returns it).  The hits take the device grouping
 * (sbgpu_bins_create_device) -- where that declines (fractional masses, ...) the call returns
 * SBGPU_EUNSUPPORTED and the caller uses sbgpu_quantify_host.  theta_out / status_out / iters_out are host
 * arrays; the handle holds the bins (no per-hit bin indices and no weights: sbgpu_bins_export_weights on it
 * fails with SBGPU_EINVAL -- a caller that wants F uses sbgpu_quantify_host).                                       */
int sbgpu_quantify_device(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                          const float *d_hit_mass, const int64_t *locus_hit_off, const sbgpu_insert_t *insert,
                          int32_t read_len, int32_t long_read, double *theta_out, int32_t *status_out,
                          int32_t *iters_out, sbgpu_bins_t **bins_out);
/* The resident path end to end: sbgpu_quantify_device's chain with pass 1 in front of it and the epilogue behind it, the
 * path's collectives INSIDE the call -- what Sample::preProcess + Sample::procSample compute between the unique hits and
 * the numbers print2gtf prints (src/alignments.cpp:1189-1232, 1736-1834), without theta, F or a per-hit array crossing PCIe:
 *   insert == NULL   the reference's DEFAULT mode (no -i): Sample::fragLenDist (alignments.cpp:1363-1410) on the device -- the
 *                    hits that are compatible with exactly one transcript, Contig::exonic_overlaps_len (contig.cpp:412-426),
 *                    an integer histogram --, all-reduced over `comm`, then InsertSize(frag_lens) (read.cpp:238-262) from
 *                    it: every rank holds the law of the WHOLE sample; returned in *insert_used (emp_hist points into the
 *                    handle).  sbgpu_quantify_host / _device with insert == NULL build their law the same way.
 *                    With long_read = 1 it is the reference's long-read workflow instead (Strawberry.cpp:335-337): no law
 *                    is built, every weight is 1/L (as with a given law), *insert_used is all zeros (use_emp = 0,
 *                    emp_hist NULL), n_frag_lens is 0 and pass 1 only all-reduces the mapped-read total.
 *                    params->effective_len_norm needs the law's mean, so it is refused there (SBGPU_EINVAL).
 *   mapped_reads     this rank's part of Sample::total_mapped_reads(): sum over its clusters of (int) weighted_mass()
 *                    (alignments.cpp:1372; sbgpu_uniq_dev_info's info[4]); all-reduced over `comm`
 *   params           the reference's globals; total_mapped_reads and insert_mean are NOT read (the call fills them in
 *                    from the all-reduced total and the law in use)
 *   comm             NULL (or a world of one): no exchange.  Otherwise every rank of the communicator must make this
 *                    call: all-reduce(max) of one int64 and all-reduce(sum) of the histogram (empirical mode only),
 *                    all-reduce(sum) of the mapped-read total, and -- the one collective per step of north_star --
 *                    all-reduce(sum) of the ranks' FPKM totals between abundance_kernel and tpm_kernel
 *                    (estimate.cpp:314-345, alignments.cpp:1821-1829)
 *   out              host arrays to fill (any may be NULL) and, on return, the device arrays of all of them -- the
 *                    context's own memory, valid until its next sbgpu_quantify_* call -- plus the totals
 * Declines like sbgpu_quantify_device (SBGPU_EUNSUPPORTED: the caller uses sbgpu_quantify_host).                        */
typedef struct {
   double *theta, *fpkm, *frac, *tpm; /* in: host [n_iso], or NULL                                    */
   int32_t *keep;                     /* in: host [n_iso], or NULL: 0 erased, 1 kept, 2 kept "NA"    */
   int32_t *status, *iters;           /* in: host [n_loci], or NULL                                   */
   const double *d_theta, *d_fpkm, *d_frac, *d_tpm; /* out: device [n_iso]                            */
   const int32_t *d_keep;                           /* out: device [n_iso]                            */
   const int32_t *d_status, *d_iters;               /* out: device [n_loci]                           */
   int64_t total_mapped_reads;        /* out: Sample::total_mapped_reads(), all ranks                 */
   double total_fpkm;                 /* out: the FPKM total TPM divides by, all ranks                */
   int64_t n_frag_lens;               /* out: size of the empirical sample, all ranks (0: a law was given) */
} sbgpu_abundances_t;
int sbgpu_quantify_resident(sbgpu_ctx_t *ctx, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                            const float *d_hit_mass, const int64_t *locus_hit_off, const sbgpu_insert_t *insert,
                            int32_t read_len, int32_t long_read, int64_t mapped_reads,
                            const sbgpu_abundance_params_t *params, sbgpu_comm_t *comm, sbgpu_insert_t *insert_used,
                            sbgpu_abundances_t *out, sbgpu_bins_t **bins_out);
/* ---- records in HOST memory -> abundances, chunk by chunk, with a bounded footprint on the device -------------------------
 * The reference streams: Sample::nextClusterRefDemand / procSample hold one cluster's reads at a time
 * (src/alignments.cpp:1145-1187, 1736-1811).  The device entries above take a whole sample's records resident; a caller that
 * inflates a BAM file on the host, or holds the file's own bytes there (push_bgzf below), uses this instead (csrc/front_stream_api.hip):
 *   begin   the clusters of quant mode (sorted by (reference, left), as sbgpu_assign_reads_*; cluster k = locus k of the
 *           annotation given to end), the decoder's options, and the most bytes one chunk will hold: two device buffers of
 *           twice that (a chunk + room for the records carried over from the chunk before)
 *   push    the next chunk of the inflated record stream -- WHOLE records, in file order -- from host memory, with the records'
 *           offsets in the chunk (rec_off[0 .. n_records], rec_off[n_records] = n_bytes; NULL: found here with
 *           sbgpu_bam_index_host).  The bytes start their way to the device, and while they travel the chunk pushed BEFORE is
 *           decoded, assigned to the clusters, and the clusters it completes (a record behind their end has been seen) are
 *           paired, collapsed, and their unique hits added to the stream's store on the device; the records of the first
 *           incomplete cluster onward are decoded again with the next chunk.  The caller must leave the bytes AND the offsets
 *           of a push untouched until the NEXT push (or end) returns.  From page-locked memory (hipHostMalloc, cudaHostRegister'ed
 *           buffers a driver inflates into) the upload runs beside the kernels; from pageable memory it is staged by the
 *           runtime before the call computes (correct, no overlap).  A cluster whose records exceed a chunk: SBGPU_ESHAPE (the
 *           records carried from one window to the next -- the first incomplete cluster's onward -- may hold chunk_bytes
 *           bytes, not one more); an empty push is allowed (no chunk).
 *   end     the last chunk, then ONE sbgpu_quantify_resident over the store (arguments as there; mapped_reads is the
 *           stream's own count): the empirical insert-size law is the whole sample's, TPM needs every locus.
 * Results: those of sbgpu_bam_decode_device .. sbgpu_quantify_resident on the whole sample at once, bit for bit.
 * info: 0 records pushed, 1 accepted records consumed, 2 pairs, 3 unique hits, 4 their features, 5 pairs the span filter
 * dropped, 6 mapped reads, 7 chunks (non-empty pushes), 8 clusters finished, 9 most bytes carried over, 10 records decoded twice, 11 the LEAST free
 * device memory seen since begin (bytes, hipMemGetInfo after every chunk and after the last stage: blocks the library's pool
 * holds idle count as used), 12 chunk_bytes (the capacity of a chunk and of a carry), 13: 1 once ended, 14 free device memory at begin, 15 compressed bytes pushed (push_bgzf). */
typedef struct sbgpu_front_stream sbgpu_front_stream_t;
int sbgpu_front_stream_begin(sbgpu_ctx_t *ctx, const sbgpu_clusters_t *clusters, const sbgpu_bam_opts_t *opts, int64_t chunk_bytes,
                             sbgpu_front_stream_t **out);
int sbgpu_front_stream_push(sbgpu_front_stream_t *fs, const uint8_t *bytes, int64_t n_bytes, const int64_t *rec_off, int64_t n_records);
int sbgpu_front_stream_end(sbgpu_front_stream_t *fs, const sbgpu_annotation_t *annot, const sbgpu_insert_t *insert, int32_t read_len,
                           int32_t long_read, const sbgpu_abundance_params_t *params, sbgpu_comm_t *comm, sbgpu_insert_t *insert_used,
                           sbgpu_abundances_t *out, sbgpu_bins_t **bins_out);
int sbgpu_front_stream_info(const sbgpu_front_stream_t *fs, int64_t info[16]);
/* push_bgzf: the next chunk as the file's own bytes -- WHOLE BGZF members in file order, from host memory under the rules of
 * push (page-locked: the upload runs beside the kernels).  file_bytes[0 .. n_bytes) are the members blk_off[0] .. blk_off[n_blocks]
 * of the block table (sbgpu_bgzf_index_host; blk_off / out_off point at the push's first member, n_bytes = blk_off[n_blocks] -
 * blk_off[0]; the two tables are copied before the call returns).  The compressed bytes are uploaded; when the chunk's turn
 * comes -- in the NEXT push, or in end -- it is inflated on the device where an inflated chunk would have landed, behind the
 * carried bytes, the window's records are found there (sbgpu_bam_index_device's scheme with the members' starts as guesses), and
 * the per-chunk work of push runs unchanged.  Members need not end on record boundaries: the bytes of a record the chunk's end
 * cuts join the carry and the next chunk's bytes complete it.  first_record: how many of the push's inflated bytes belong to the
 * BAM header (nonzero for the pushes up to the one that holds the header's end; a push that is all header passes at least its
 * span).  chunk_bytes of begin keeps meaning INFLATED bytes: a push whose out_off span exceeds it is SBGPU_ESHAPE, as is a stream
 * that ends inside a record (from end).  A member with a nonzero SBGPU_BGZF status fails the call that computes its chunk with
 * SBGPU_EINVAL and the member's offset (blk_off[k]) in sbgpu_last_error; the stream can then only be destroyed.  Results: those of
 * the same records through push and through the resident entries, bit for bit.  push and push_bgzf are not mixed in one stream
 * (SBGPU_EINVAL).  sbgpu_front_stream_info: info[15] is the compressed bytes pushed.                                          */
int sbgpu_front_stream_push_bgzf(sbgpu_front_stream_t *fs, const uint8_t *file_bytes, int64_t n_bytes, const int64_t *blk_off,
                                 const int64_t *out_off, int64_t n_blocks, int64_t first_record);
/* the store: the unique hits of the clusters finished so far (device arrays, the stream's), their masses, and where every
 * cluster's hits begin (host, [n_clusters + 1]; complete after end)                                                            */
int sbgpu_front_stream_hits(const sbgpu_front_stream_t *fs, sbgpu_hits_t *d_hits, const float **d_hit_mass, const int64_t **locus_hit_off);
void sbgpu_front_stream_destroy(sbgpu_front_stream_t *fs);
/* F of the EM batch a handle from sbgpu_quantify_host holds: F_out[info[3]] (row-major per locus). */
int sbgpu_bins_export_weights(const sbgpu_bins_t *bins, double *F_out);

/* ---- the fragment-context table (-f) as arrays ------------------------------------------------
 * Sample::printContext (src/alignments.cpp:1549-1639) up to the formatting: which bins of every locus get a row, in
 * which order, with how many hits and which conditional probabilities.  With kept(j) = keep[j] != 0 after the
 * expression filter (estimate.cpp:346-355):
 *   - a hit QUALIFIES if it landed in a bin and is compatible with a kept isoform of its locus; a locus whose status is
 *     SBGPU_EM_INIT_EMPTY, or with no kept isoform, has no qualifying hit and no row;
 *   - row_hits is a bin's number of qualifying hits (path_count); a bin without one has no row; locus_hits is their sum
 *     over the locus (gene_frag_count; summed in 32 bits as the reference's uint is);
 *   - a row holds, for EVERY isoform j of its locus (the caller picks the kept ones, as for FPKM and Frac), the bin's raw
 *     weight F where the bin's LAST qualifying hit -- the one of the largest index: eb_prob_map[...] = ... overwrites --
 *     is compatible with j, else 0.0 (estimate.hpp:173-197: that hit's isoforms, not the bin's union);
 *   - rows of a locus come in std::map order of the bins' coordinate sets (csrc/context_rules.h: ctx_key_less).
 * The struct: host arrays to fill (any may be NULL) and, on return, the row count and -- device form only -- the device
 * arrays of all five (the context's memory: valid until its next sbgpu_quantify_* or sbgpu_context_table_device call). */
typedef struct {
   int64_t  *locus_row_off;   /* in: [n_loci + 1]  rows of locus l = [off[l], off[l+1])                               */
   uint32_t *locus_hits;      /* in: [n_loci]      gene_frag_count                                                     */
   int64_t  *row_bin;         /* in: [n_bins]      global bin of row r (indexes the bin keys, sbgpu_binseq_*'s stats)  */
   uint32_t *row_hits;        /* in: [n_bins]      path_count                                                          */
   double   *row_prob;        /* in: [n_elem]      row r of locus l: niso(l) values at                                 */
                              /*                   f_off[l] + (r - locus_row_off[l]) * niso(l); 0.0 behind a locus' rows */
   int64_t n_rows;            /* out */
   const int64_t *d_locus_row_off; const uint32_t *d_locus_hits; const int64_t *d_row_bin; /* out: device form only    */
   const uint32_t *d_row_hits; const double *d_row_prob;
} sbgpu_context_table_t;
/* Host form, the plain statement of the arithmetic: `bins` holds hit -> bin (sbgpu_bins_create, sbgpu_quantify_host),
 * compat[n_hits * compat_words] are the hits' compat words (sbgpu_exonbin_*, sbgpu_quantify_host's compat_out), F[n_elem]
 * the bin weights (NULL: the handle's own, sbgpu_quantify_host), keep[n_iso] and status[n_loci] the epilogue's and the
 * EM's (NULL: everything kept / every locus started).                                                              */
int sbgpu_context_table_host(const sbgpu_bins_t *bins, const uint32_t *compat, int32_t compat_words, const double *F,
                             const int32_t *keep, const int32_t *status, sbgpu_context_table_t *out);
/* on != 0: the context's LATER sbgpu_quantify_resident / sbgpu_front_stream_end calls keep what the table needs -- hit ->
 * bin as the grouping's 4-byte ranks (made, where the grouping would have left it out), the compat words, F, keep and
 * status, all where the call had them anyway: nothing is copied, and theta, FPKM, Frac, TPM, keep, status and iters are
 * the same bits.  Off (the default): those calls are unchanged.                                                    */
int sbgpu_context_table_keep(sbgpu_ctx_t *ctx, int32_t on);
/* Device form (csrc/context_device.h): right after such a call, on the handle it returned, before the context's next
 * call that works in its scratch memory -- every sbgpu_quantify_*, sbgpu_bins_create_device and the other multi-stage
 * device entries; sbgpu_context_table_device itself and the readers of a handle do not --:
 * SBGPU_EINVAL otherwise -- a handle made without retention, or a stale one; sbgpu_last_error says which.  One pass over the hits, a sort per locus, a
 * gather; only the five per-bin / per-locus arrays cross PCIe, whatever the number of hits.  Synchronises on `stream`
 * (NULL: the context's own).  Loci of more than 4096 isoforms: SBGPU_ESHAPE.                                        */
int sbgpu_context_table_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, void *stream, sbgpu_context_table_t *out);

/* ---- fragment assignment: which isoform a fragment came from, and how sure that is -------------------
 * The posterior U(i,j) that EmSolver::run computes per bin and discards (src/estimate.cpp:449-458), per HIT: hits of one bin
 * differ in their compat words, so they differ in their candidates.  The rule (csrc/assign_rules.h, shared by both forms,
 * compiled under -ffp-contract=off), for locus l with bins b, isoforms j, raw weights F[b][j], the caller's theta, keep, status:
 *   - kept(j): keep[j] != 0, and nothing is kept in a locus whose status is SBGPU_EM_INIT_EMPTY (as for the -f table);
 *   - a bin is LIVE if some F[b][j] > SBGPU_EM_ROW_EPS (the row drop of EmSolver::init, estimate.cpp:377-384);
 *   - the column scale c_j is the sum of F[b][j] over the locus' live bins in ascending bin order -- the normalisation the EM
 *     runs on from its second iteration (estimate.cpp:466-475); the model weight is W[b][j] = F[b][j] / c_j, 0 where c_j == 0;
 *   - the gain g_j = theta[j] / c_j, exactly 0.0 where j is not kept or c_j == 0;
 *   - the CANDIDATES of hit h are compat(h) & kept(l); n_cand[h] is their number -- a fact of the words alone, defined for
 *     every hit;
 *   - numerator num_j = theta[j] * W[b][j], evaluated as g_j * F[b][j], for each candidate; the denominator den is the sum of
 *     the numerators over the candidates in ascending j; the posterior p(j|h) = num_j / den;
 *   - h is UNASSIGNED -- map_iso = -1, map_prob = 0.0 -- when it has no bin (hit -> bin < 0), its bin is not live, it has no
 *     candidate, or den is not > 0;
 *   - otherwise map_iso[h] is the candidate of the largest numerator, the lowest j on a tie (strict > in ascending order), as
 *     the index inside the locus, and map_prob[h] is its p;
 *   - per isoform, over the ASSIGNED hits of its locus, m_h the hit's mass (1.0 where no masses are given):
 *       unique_mass[j] = sum of m_h over the hits with n_cand == 1 and candidate j,
 *       map_mass[j]    = sum of m_h over the hits with map_iso == j,
 *       post_mass[j]   = sum of m_h * p(j|h);
 *   - per locus, unassigned[l] is the number of its unassigned hits.
 * The struct: host arrays to fill (any may be NULL) with, where one of the three per-hit arrays is given, n_hits saying how
 * many hits they hold (another count than the call's own: SBGPU_EINVAL, nothing is written) and, on return, the hit count
 * and -- device form only -- the device arrays of all seven (the context's memory: valid until its next sbgpu_quantify_* or sbgpu_fragment_assign_device call). */
typedef struct {
   int32_t *map_iso;          /* in: [n_hits]  the MAP isoform's index inside the hit's locus, -1: unassigned */
   double  *map_prob;         /* in: [n_hits]  its posterior, 0.0: unassigned                                  */
   int32_t *n_cand;           /* in: [n_hits]                                                                  */
   double  *unique_mass, *map_mass, *post_mass; /* in: [n_iso]                                                 */
   int64_t *unassigned;       /* in: [n_loci]                                                                  */
   int64_t n_hits;            /* in: the per-hit arrays' length (read where one is given); out: the hits */
   const int32_t *d_map_iso; const double *d_map_prob; const int32_t *d_n_cand; /* out: device form only       */
   const double *d_unique_mass, *d_map_mass, *d_post_mass; const int64_t *d_unassigned;
} sbgpu_fragment_assign_t;
/* Host form, the plain statement of the arithmetic; every sum runs in hit order.  `bins` holds hit -> bin (sbgpu_bins_create,
 * sbgpu_quantify_host; a handle that holds none: SBGPU_EINVAL), compat[n_hits * compat_words] the hits' compat words, F[n_elem]
 * the bin weights (NULL: the handle's own), theta[n_iso] the abundances the posterior is taken under (NULL: SBGPU_EINVAL),
 * keep[n_iso] / status[n_loci] as for sbgpu_context_table_host (NULL: everything kept / every locus started), hit_mass[n_hits]
 * the hits' masses (NULL: 1.0 each).  A hit without a bin belongs to the locus the hits' grouping says; a handle whose hits
 * did not come grouped by locus and that holds such a hit: SBGPU_EINVAL.                                              */
int sbgpu_fragment_assign_host(const sbgpu_bins_t *bins, const uint32_t *compat, int32_t compat_words, const double *F,
                               const double *theta, const int32_t *keep, const int32_t *status, const float *hit_mass,
                               sbgpu_fragment_assign_t *out);
/* Device form (csrc/assign_device.h): under the conditions of sbgpu_context_table_device -- right after a resident call or an
 * sbgpu_front_stream_end made with sbgpu_context_table_keep on, on that call's handle; SBGPU_EINVAL for a handle made without
 * retention or a stale one -- from what the call kept (hit -> bin, compat words, F, keep, status: nothing more is retained).
 * d_theta: any device [n_iso] array -- normally the call's d_theta; a bootstrap mean serves as well; d_hit_mass: the array the
 * resident call was given, or NULL for unit masses.  One pass over F (live bins, gains), one over the hits.  The per-hit
 * results are the host form's bits; the per-isoform sums are added in another order (integers in doubles for unit masses:
 * exact; post_mass: within the rounding of a sum of its non-negative terms).  The results live in a scratch slot of their
 * own: the table and the assignment may be asked for in either order, repeatedly.  Only what the caller asked for crosses
 * PCIe.  Synchronises on `stream` (NULL: the context's own).  Loci of more than 4096 isoforms or more than 5632 bins:
 * SBGPU_ESHAPE.                                                                                                       */
int sbgpu_fragment_assign_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const double *d_theta, const float *d_hit_mass,
                                 void *stream, sbgpu_fragment_assign_t *out);

/* ---- isoform-resolved coverage: per-exon depth and junction support ----------------------------------
 * Where along an isoform its fragments lie: what is built from the fragment assignment above and the hits' features.  The rule
 * (csrc/coverage_rules.h, shared by both forms, compiled under -ffp-contract=off).  Who is assigned, its candidates J(h) and
 * the posterior p(j|h) ARE the fragment assignment's, under the same theta, keep, status and weights.  For locus l, an assigned
 * hit h of mass m_h (a float; 1.0 where no masses are given) and a candidate j:
 *   - WEIGHT  w(h,j) = (double)m_h * p(j|h), multiplied in that order;
 *   - OVERLAP for an exon e = [L_e, R_e] of isoform j (exon_off, closed coordinates): ov(h,e) is the sum over the hit's S_MATCH
 *     features f of max(0, min(R_e, f.right) - max(L_e, f.left) + 1), an integer; S_GAP and S_INTRON features add nothing:
 *     only sequenced bases count;
 *   - exon_bases[e] = sum over the assigned hits h of l with j in J(h) of w(h,j) * (double)ov(h,e); indexed as exon_left is;
 *   - junction_mass[e], for an exon that is not its isoform's last: the sum of w(h,j) over the assigned hits with j in J(h)
 *     that own an S_INTRON feature with left == R_e + 1 and right == L_{e+1} - 1 -- a pair whose unsequenced gap spans the
 *     intron does not support it; exactly 0.0 for an isoform's last exon;
 *   - iso_bases[j] = the finished exon_bases[e] of the isoform's exons, added in ascending e: a function of exon_bases' bits;
 *   - unexplained_bases[l] = sum over the UNASSIGNED hits of l of (double)m_h * (double)matchlen(h), matchlen(h) the total
 *     length of the hit's S_MATCH features.
 * An isoform that is not kept, and a locus whose status is SBGPU_EM_INIT_EMPTY, get zeros; all hits of such a locus are
 * unassigned, so they count as unexplained.  Depth is the caller's division: exon_bases[e] / (R_e - L_e + 1) per exon,
 * iso_bases[j] / the isoform's length per isoform.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device form only -- the device arrays of all four (the
 * context's memory: valid until its next sbgpu_quantify_* or sbgpu_isoform_coverage_device call). */
typedef struct {
   double *exon_bases;        /* in: [exon_off[n_iso]]                                          */
   double *junction_mass;     /* in: [exon_off[n_iso]]                                          */
   double *iso_bases;         /* in: [n_iso]                                                    */
   double *unexplained_bases; /* in: [n_loci]                                                   */
   const double *d_exon_bases, *d_junction_mass, *d_iso_bases, *d_unexplained_bases; /* out: device form only */
} sbgpu_isoform_coverage_t;
/* Host form, the plain statement of the rule: hits in index order, inside a hit the candidates in ascending j, inside a candidate
 * the exons in ascending order.  `bins`, compat, F, theta, keep, status, hit_mass: as for sbgpu_fragment_assign_host, with its
 * refusals (theta NULL, a handle that holds no hit -> bin, a bin-less hit among hits that did not come grouped by locus:
 * SBGPU_EINVAL).  annot, hits: the host arrays the handle was made from; hits->n_hits or the annotation's loci / isoforms other
 * than the handle's: SBGPU_EINVAL, sbgpu_last_error says which.                                                        */
int sbgpu_isoform_coverage_host(const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                                const uint32_t *compat, int32_t compat_words, const double *F, const double *theta,
                                const int32_t *keep, const int32_t *status, const float *hit_mass, sbgpu_isoform_coverage_t *out);
/* Device form (csrc/coverage_device.h): valid exactly where sbgpu_fragment_assign_device is -- same handles, same refusals --
 * and nothing more is retained by a resident call.  annot: HOST pointers (the context's pinned copy is used where it matches,
 * otherwise the exon arrays are uploaded); d_hits: the DEVICE arrays the resident call was given, or sbgpu_front_stream_hits'
 * (another n_hits than the retained call's: SBGPU_EINVAL); d_theta, d_hit_mass: as for sbgpu_fragment_assign_device.  The
 * assignment's column pass, one pass over the hits, one over the isoforms.  The sums are added in another order than the host
 * form's: equal within the rounding of a sum of non-negative terms, exactly where every term is an integer; iso_bases is the
 * ascending sum of the device's own exon_bases.  The results live in a scratch slot of their own: table, assignment and
 * coverage may be asked for in any order, repeatedly.  Only the arrays the caller gave pointers for cross PCIe.  Synchronises
 * on `stream` (NULL: the context's own).  Loci of more than 4096 isoforms or more than 5632 bins: SBGPU_ESHAPE.       */
int sbgpu_isoform_coverage_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                                  const double *d_theta, const float *d_hit_mass, void *stream, sbgpu_isoform_coverage_t *out);
/* The device form's thresholds (csrc/coverage_device.h), for callers and tests that want a locus on either side of each:
 * out[0] hits of one work item, [1] annotated exons of a locus up to which its exon table and sums live in LDS, [2] the same
 * number again (the isoforms that LDS has room for: no threshold of its own, an isoform owns an exon), [3] isoforms and [4] exons
 * up to which the sums are kept in copies, [5] the copies, [6] the most bins and [7] the most isoforms of one locus.          */
int sbgpu_isoform_coverage_limits(int64_t out[8]);

/* ---- model fit: likelihood, bin residuals, isoform scores ---------------------------------------------
 * How well theta explains a locus' bin counts, and how converged theta is: made from the mixture mass of every exon bin, which
 * EmSolver::run (estimate.cpp:449-476) computes each iteration and discards.  The rule (csrc/fit_rules.h, shared by both forms,
 * compiled under -ffp-contract=off).  One locus: bins b with counts n_b (int32 >= 0), isoforms j, raw weights F[b][j], the
 * caller's theta, keep, status.
 *    1. kept(j), the live bins, the column scale c_j (the column's sum over the live bins in ascending order) and the gain
 *       g_j = theta_j / c_j ARE the fragment assignment's above (ctx_kept_word, asg_row_live, asg_gain).
 *    2. d_b = the sum over the kept j, ascending, of g_j * F[b][j] for a live bin, 0.0 otherwise: the bin's mixture mass in count
 *       units, the `den` of a hit compatible with every kept isoform.
 *    3. A live bin is POSSIBLE when d_b > 0.
 *    4. n_live[l] = sum of n_b over the live bins; n_dropped[l] = the same over the bins that are not live (the rows
 *       EmSolver::init drops); n_impossible[l] = the same over the live bins that are not possible (fragments to which the kept
 *       isoforms give probability zero: after the expression filter erased an isoform, or under SBGPU_EM_DENOM_ZERO);
 *       M = n_live - n_impossible; D = sum of d_b over the possible bins.
 *    5. expected[b] = (double)M * (d_b / D) for a possible bin, 0.0 otherwise.
 *    6. resid[b] = ((double)n_b - expected[b]) / sqrt(expected[b]) where expected[b] > 0, 0.0 otherwise.
 *    7. loglik[l] = sum of (double)n_b * log(d_b / D) over the possible bins with n_b > 0: the multinomial log-likelihood
 *       without its constant.
 *    8. deviance[l] = 2 * sum of (double)n_b * log((double)n_b / expected[b]) over the same bins.
 *    9. pearson[l] = sum of resid[b]^2 over the possible bins: a function of resid's bits.
 *   10. dof[l] = max(0, P - 1 - max(0, A - 1)), P the number of possible bins, A the number of isoforms with g_j > 0.
 *   11. worst_bin[l] = the locus-local index of the possible bin of largest |resid| under strict > in ascending order (the
 *       lowest index wins a tie; a NaN never wins); -1 when there is none.
 *   12. score[j] = (sum over the possible b, ascending, of ((double)n_b / d_b) * F[b][j]) / c_j for a kept isoform with
 *       c_j != 0, 0.0 otherwise; the ratio first, then the product, the division by c_j last.  theta[j] * score[j] is the
 *       M-step's next theta[j] on the column-normalised F, so score[j] = 1 for every theta[j] > 0 at the optimum, and
 *       || theta o score - theta ||_2 per locus is the distance the reference's stopping rule (SBGPU_EM_THETA_CHANGE_LIMIT)
 *       looks at.
 * A locus whose status is SBGPU_EM_INIT_EMPTY, or with nothing kept: all zeros, dof 0, worst_bin -1, and n_dropped counts ALL
 * its fragments, live row or not: none of them entered a fit.  p-values are the caller's: dof and the two statistics are what
 * they need.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device forms only -- the device arrays of all of them:
 * the context's memory, in a scratch slot of their own, valid until the context's next sbgpu_quantify_* or fit call.        */
typedef struct {
   double *expected, *resid;                       /* in: [n_bins]  */
   double *score;                                  /* in: [n_iso]   */
   double *loglik, *deviance, *pearson;            /* in: [n_loci]  */
   int64_t *n_live, *n_dropped, *n_impossible;     /* in: [n_loci]  */
   int32_t *dof, *worst_bin;                       /* in: [n_loci]  */
   const double *d_expected, *d_resid, *d_score, *d_loglik, *d_deviance, *d_pearson; /* out: device forms only */
   const int64_t *d_n_live, *d_n_dropped, *d_n_impossible;
   const int32_t *d_dof, *d_worst_bin;
} sbgpu_em_fit_t;
/* Host form (csrc/fit_host.cpp; no GPU needed), the plain statement of the rule: every sum in ascending order.  theta [n_iso];
 * keep [n_iso] or NULL: everything kept; status [n_loci] or NULL: every locus started.  SBGPU_EINVAL, with the reason in
 * sbgpu_last_error: a NULL theta, a negative count, malformed offsets (not beginning at 0, not ascending, f_off not rows x
 * isoforms), NULL count / F where there are bins / weights.                                                             */
int sbgpu_em_fit_host(const sbgpu_batch_t *batch, const double *theta, const int32_t *keep, const int32_t *status, sbgpu_em_fit_t *out);
/* Device form (csrc/fit_device.h) for any batch sbgpu_em_run_device solves: the plan, d_count and d_F as given to it; d_theta:
 * any device [n_iso] array (the EM's, or a bootstrap mean); d_keep / d_status: device arrays or NULL, as above.  The
 * assignment's column pass (unchanged), then one pass that reads F twice: a wave per locus of at most out[0] weights of
 * sbgpu_em_fit_limits, a workgroup per larger locus.  d_b and the score's inner sum run in the rule's order: the integer arrays,
 * the zeros and which bins are possible are the host form's exactly; D, loglik, deviance and pearson are added along a fixed
 * tree (csrc/fit_device.h states it): equal to the host form within the rounding of another order, the same bits from call to
 * call; pearson is that tree over the device's own resid, worst_bin the argmax of the device's own resid.  Only the arrays
 * the caller gave pointers for cross PCIe.  Synchronises on `stream` (NULL: the context's own).  Loci of more than 4096
 * isoforms or more than 5632 bins: SBGPU_ESHAPE.  A NULL d_theta: SBGPU_EINVAL.                                          */
int sbgpu_em_fit_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const double *d_theta,
                        const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_fit_t *out);
/* The same right after a resident call or an sbgpu_front_stream_end made with sbgpu_bootstrap_keep on, from that record (the
 * call's plan, counts and weights): nothing more is retained, and the call's seven results are the same bits with and without a
 * fit call behind it.  A handle made without retention, or a stale one: SBGPU_EINVAL, as for
 * sbgpu_abundance_bootstrap_device.  Fit, table, assignment and coverage may be asked for in any order.                  */
int sbgpu_model_fit_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const double *d_theta, const int32_t *d_keep, const int32_t *d_status,
                           void *stream, sbgpu_em_fit_t *out);
/* The device form's thresholds (csrc/fit_device.h), for callers and tests that want a locus on either side of each: out[0]
 * weights (and bins, and isoforms) of a locus up to which a wave serves it, a workgroup beyond; [1] weights up to which the
 * workgroup form stages F in LDS, global memory beyond; [2] loci per workgroup in the wave form; [3] workgroups per CU a launch's
 * grid is capped at; [4] threads of a workgroup; [5] of a wave (the reduction tree's two levels); [6] the most bins and [7] the
 * most isoforms of one locus.                                                                                              */
int sbgpu_em_fit_limits(int64_t out[8]);

/* ---- isoform information: identifiability and analytic covariance ----------------------------------------
 * Which isoforms of a locus the counted bins can tell apart, which are confounded with which, and how strongly: the observed
 * information matrix of the locus' mixture at theta, its factorisation, and the covariance of theta that follows -- one pass
 * over arrays a batch holds anyway, where a bootstrap costs one EM solve per replicate and cannot report rank deficiency.  The
 * rule (csrc/info_rules.h, shared by both forms, compiled under -ffp-contract=off).  One locus: bins b with counts n_b, isoforms
 * j, raw weights F[b][j], the caller's theta, keep, status.  Every sum starts from 0.0 and adds in ascending index unless said.
 *    1. kept(j), the live bins, c_j, g_j, d_b and "possible" ARE the assignment's and the fit's above (ctx_kept_word,
 *       asg_row_live, asg_gain, fit_bin_mass, fit_possible): called, not restated.
 *    2. w_b = ((double)n_b / d_b) / d_b for a possible bin (fit_ratio, then one more division), 0.0 otherwise.
 *    3. j is FREE when it is kept, c_j != 0 and g_j > 0 (a NaN is not free); n_free counts the free isoforms.
 *    4. For free j <= k: H_jk = (S_jk / c_j) / c_k, the information matrix in theta units.  S_jk is the WAVE-ORDER sum over the
 *       locus' bins of (w_b * F[b][j]) * F[b][k]: partial[t], t = 0 .. 63, is the ascending sum of the terms of the bins
 *       b = t (mod 64), 0.0 where there are none; then for s = 32, 16, ..., 1: partial[i] += partial[i + s] for i < s; the
 *       result is partial[0].  (A wave's natural reduction: lane i adds lane i + s.  Both forms run this order.)
 *    5. A free j with !(H_jj > 0) is UNOBSERVED -- no counted bin carries it -- and is left out of everything below.
 *    6. dg_j = sqrt(H_jj); C_jk = (H_jk / dg_j) / dg_k.  C_jj is taken as computed, not set to 1.
 *    7. C is factorised without pivoting, in ascending j over the observed free isoforms; R is the set retained so far.
 *       piv_j = C_jj - sum over k in R of L_jk * L_jk.  If !(piv_j > SBGPU_INFO_PIVOT_EPS), j is ALIASED: on the observed
 *       bins its column is a combination of the retained ones; it does not join R, and alias_of[j] is the k in R of largest
 *       |L_jk| (strict > in ascending k; a NaN never wins; -1 where there is none).  Otherwise j joins R with
 *       L_jj = sqrt(piv_j) and, for every later observed i, L_ij = (C_ij - sum over k in R, k < j, of L_ik * L_jk) / L_jj.
 *       rank = |R|; min_pivot = the smallest retained piv_j, 0.0 where R is empty.
 *    8. Y = L_R^-1, a column at a time: Y_jj = 1 / L_jj, Y_ij = -(sum over k in R, j <= k < i, of L_ik * Y_kj) / L_ii.
 *       V_ij = sum over k in R, k >= max(i, j), of Y_ki * Y_kj.  Hinv_ij = (V_ij / dg_i) / dg_j.
 *    9. The covariance of theta GIVEN THE LOCUS' TOTAL (on the simplex): u_i = sum over j in R of Hinv_ij; t = sum over i in R of
 *       u_i; cov_ij = Hinv_ij - (u_i * u_j) / t where t > 0, Hinv_ij otherwise; se[j] = sqrt(max(cov_jj, 0.0)).  In a locus
 *       whose rank is below its number of observed free isoforms these describe the model WITH THE ALIASED ISOFORMS HELD
 *       FIXED at the caller's theta: the data say nothing about moving mass between an aliased isoform and its alias_of.
 *       This is normal theory at an interior point; for a theta_j near 0 it is one-sided (theta_j cannot go below 0) and
 *       se[j] overstates the spread downwards.  Intervals and p-values are the caller's.
 *   10. For j in R: corr_jk = cov_jk / (se_j * se_k) where both are > 0; partner[j] is the k in R, k != j, of largest |corr_jk|
 *       (strict > in ascending k; -1 where there is none); partner_corr[j] is that signed value, 0.0 where there is none.
 *   11. ident[j]: SBGPU_INFO_IDENTIFIED (j in R), _ALIASED, _UNOBSERVED, _NOT_FREE, or _SKIPPED (its locus was not analysed).
 *       alias_of and partner are locus-local isoform indices.
 *   12. info_status[l]: SBGPU_INFO_OK; SBGPU_INFO_EMPTY -- status SBGPU_EM_INIT_EMPTY, nothing kept, or n_free == 0: every
 *       isoform is _NOT_FREE, everything else zero or -1; SBGPU_INFO_TOO_WIDE -- n_free exceeds out[0] of sbgpu_em_info_limits,
 *       or (device forms only) the locus exceeds the assignment's shape limits: every isoform is _SKIPPED, everything else zero
 *       or -1.  A status, not a refusal of the call.
 *   13. cov (optional): packed by locus, the upper triangle over ALL of the locus' niso isoforms in row-major order -- entry
 *       (j, k), j <= k, at cov_off[l] + j * niso - j (j - 1) / 2 + (k - j) -- zero where either isoform is not in R.
 *       cov_off[l + 1] - cov_off[l] = niso (niso + 1) / 2 for niso <= out[0] of sbgpu_em_info_limits, 0 beyond;
 *       sbgpu_em_info_cov_offsets fills it, so that the caller can size cov before the call.
 * Out of this rule: pivoted factorisations, loci of more free isoforms than the limit, boundary corrections.
 * The struct: host arrays to fill (any may be NULL; cov needs cov_off) and, on return -- device forms only -- the device arrays
 * of all of them: the context's memory, in a scratch slot of their own, valid until the context's next sbgpu_quantify_* or
 * info call.                                                                                                               */
#define SBGPU_INFO_PIVOT_EPS 1e-9
#define SBGPU_INFO_IDENTIFIED 0
#define SBGPU_INFO_ALIASED 1
#define SBGPU_INFO_UNOBSERVED 2
#define SBGPU_INFO_NOT_FREE 3
#define SBGPU_INFO_SKIPPED 4
#define SBGPU_INFO_OK 0
#define SBGPU_INFO_EMPTY 1
#define SBGPU_INFO_TOO_WIDE 2
typedef struct {
   double *se, *partner_corr;                      /* in: [n_iso]   */
   int32_t *ident, *alias_of, *partner;            /* in: [n_iso]   */
   double *min_pivot;                              /* in: [n_loci]  */
   int32_t *rank, *n_free, *info_status;           /* in: [n_loci]  */
   double *cov;                                    /* in: [cov_off[n_loci]], or NULL */
   const int64_t *cov_off;                         /* in: [n_loci + 1], needed where cov is given (sbgpu_em_info_cov_offsets) */
   const double *d_se, *d_partner_corr;            /* out: device forms only */
   const int32_t *d_ident, *d_alias_of, *d_partner;
   const double *d_min_pivot;
   const int32_t *d_rank, *d_n_free, *d_info_status;
   const double *d_cov;
   const int64_t *d_cov_off;
} sbgpu_em_info_t;
/* cov_off [n_loci + 1] from iso_off [n_loci + 1] (rule 13).  SBGPU_EINVAL: a NULL array, n_loci < 0, offsets that do not ascend. */
int sbgpu_em_info_cov_offsets(const int64_t *iso_off, int64_t n_loci, int64_t *cov_off);
/* Host form (csrc/info_host.cpp; no GPU needed, free of HIP), the plain statement of the rule.  Arguments and refusals as
 * sbgpu_em_fit_host's; further SBGPU_EINVAL: cov given without cov_off, or a cov_off that is not rule 13's.                 */
int sbgpu_em_info_host(const sbgpu_batch_t *batch, const double *theta, const int32_t *keep, const int32_t *status, sbgpu_em_info_t *out);
/* Device form (csrc/info_device.h) for any batch sbgpu_em_run_device solves; arguments as sbgpu_em_fit_device's.  The
 * assignment's column pass (unchanged), then one pass per locus: a wave per locus of at most out[1] weights and out[2] isoforms
 * of sbgpu_em_info_limits, a workgroup per larger locus.  Every sum runs in the rule's order (S_jk along the wave's own
 * reduction), there are no floating-point atomics: every array is the host form's, bit for bit, and two calls give the same
 * bits.  A locus beyond the assignment's shape limits (4096 isoforms, 5632 bins) is SBGPU_INFO_TOO_WIDE, not a refusal.  Only
 * the arrays the caller gave pointers for cross PCIe.  Synchronises on `stream` (NULL: the context's own).                  */
int sbgpu_em_info_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const double *d_theta,
                         const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_info_t *out);
/* The same right after a resident call or an sbgpu_front_stream_end made with sbgpu_bootstrap_keep on, from that record, as
 * sbgpu_model_fit_device: nothing more is retained, the call's seven results are the same bits with and without it, and info,
 * fit, table, assignment and coverage may be asked for in any order.                                                     */
int sbgpu_model_info_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const double *d_theta, const int32_t *d_keep, const int32_t *d_status,
                            void *stream, sbgpu_em_info_t *out);
/* The thresholds (csrc/info_rules.h, csrc/info_device.h; reasoned from LDS sizes, not tuned): out[0] the most free isoforms of
 * an analysed locus (both forms; also the niso up to which cov has room); [1] weights (and bins) and [2] isoforms of a locus up
 * to which a wave serves it, a workgroup beyond; [3] bins up to which the workgroup form keeps w_b, and weights up to which it
 * stages F, in LDS (global memory beyond); [4] loci per workgroup in the wave form; [5] workgroups per CU a launch's grid is
 * capped at; [6] the most bins and [7] the most isoforms of one locus the device form analyses.  A workgroup is 256 threads.  */
int sbgpu_em_info_limits(int64_t out[8]);

/* ---- isoform support: drop-one likelihood-ratio statistics ------------------------------------------------
 * Do the fragments of a locus need isoform j, or do its neighbours explain them as well?  Drop j, solve the locus again, compare
 * the likelihoods.  The information pass above is one-sided exactly where this question lives (theta_j near 0), and a bootstrap
 * costs B solves and only spreads a dispensable isoform's mass around.  The rule (csrc/loo_rules.h, shared by both forms,
 * compiled under -ffp-contract=off).  One locus: bins b with counts n_b, isoforms j, raw weights F[b][j], keep (NULL: all kept;
 * kept(j) is ctx_kept_word's bit under status SBGPU_EM_OK).  K is the number of kept isoforms.
 *    1. loo_status[l]: SBGPU_LOO_EMPTY when K = 0; SBGPU_LOO_TOO_WIDE when K > SBGPU_LOO_MAX_KEPT -- a status, not a refusal of
 *       the call: the neighbours are untouched; SBGPU_LOO_OK otherwise.  A locus beyond the fit's shape limits (5632 bins, 4096
 *       isoforms) refuses the call with SBGPU_ESHAPE, as the fit does.
 *    2. The sub-problems of an OK locus, in this order: the BASE -- the kept columns, ascending -- then, when K >= 2, one per kept
 *       j, ascending: the kept columns without j.  Each is a locus of its own: the same bins and counts, F compacted row-major to
 *       its columns.  The sub-problems of all loci are numbered consecutively (a sub-batch).  A K = 1 locus has the base only.
 *    3. Each sub-problem is solved as sbgpu_em_run_device solves any locus (theta_0, the row drop, the statuses, the iteration
 *       contract); the fit above then runs on it with nothing erased (keep NULL, status the solve's): loglik, n_live, n_dropped
 *       and n_impossible are its rules 4 and 7.  The base is always solved inside the call, never taken from the caller: a locus
 *       solved again alone does not always return a batch's theta bits.
 *    4. n_unique[j] = (n_dropped + n_impossible) of j's sub-problem - the same of the base: the fragments no other kept isoform
 *       explains.  An integer: exact.
 *    5. lr_stat[j] = +inf when n_unique[j] > 0, else 2.0 * (loglik_base - loglik_without_j): one subtraction and one product.
 *       Both solves stop at SBGPU_EM_THETA_CHANGE_LIMIT, not at the optimum: small negative values are real and are reported
 *       raw.  The isoform of a K = 1 locus is SOLE: +inf, and its n_unique is the base's n_live - n_impossible.
 *    6. heir[j] = the locus-local index of the kept k != j of largest theta_without_j[k] - theta_refit[k] under strict > in
 *       ascending k, -1 when no gain is > 0 (a NaN never wins); heir_gain[j] is that difference, 0.0 where there is none: where
 *       j's fragments go.
 *    7. theta_refit [n_iso]: the base's theta scattered back, 0.0 for an isoform that is not kept or whose locus is not OK.
 *       status_without[j], iters_without[j]: the sub-problem's, -1 for an isoform that is not TESTED.  support[j]:
 *       SBGPU_LOO_NOT_KEPT, _TESTED, _SOLE, or _LOCUS_SKIPPED (kept, in a TOO_WIDE locus).  An isoform that is not TESTED or
 *       SOLE has lr_stat 0.0, n_unique 0, heir -1, heir_gain 0.0.
 *    8. Per locus: loo_status, and the base's loglik_base, status_base, iters_base (0.0, -1, -1 where the locus is not OK).
 *    9. theta_without (optional) is packed: for a TESTED j, the K - 1 values of the other kept isoforms, ascending, at
 *       without_off[j]; sbgpu_em_loo_offsets fills without_off [n_iso + 1], so that the caller can size it before the call.
 * p-values are the caller's (the boundary mixture 1/2 chi2_0 + 1/2 chi2_1; strawberry_amd/support.py has one).
 * Out of this rule: warm starts, loci of more kept isoforms than the limit, sets of isoforms, multiple-testing corrections.
 * The struct: host arrays to fill (any may be NULL; theta_without needs without_off) and, on return -- device forms only -- the
 * device arrays of all of them: the context's memory, in a scratch slot of their own, valid until the context's next
 * sbgpu_quantify_* or support call.                                                                                       */
#define SBGPU_LOO_MAX_KEPT 64
#define SBGPU_LOO_OK 0
#define SBGPU_LOO_EMPTY 1
#define SBGPU_LOO_TOO_WIDE 2
#define SBGPU_LOO_NOT_KEPT 0
#define SBGPU_LOO_TESTED 1
#define SBGPU_LOO_SOLE 2
#define SBGPU_LOO_LOCUS_SKIPPED 3
typedef struct {
   double *lr_stat, *heir_gain, *theta_refit;                       /* in: [n_iso]   */
   int64_t *n_unique;                                               /* in: [n_iso]   */
   int32_t *heir, *status_without, *iters_without, *support;        /* in: [n_iso]   */
   double *loglik_base;                                             /* in: [n_loci]  */
   int32_t *loo_status, *status_base, *iters_base;                  /* in: [n_loci]  */
   double *theta_without;                                           /* in: [without_off[n_iso]], or NULL */
   const int64_t *without_off;                                      /* in: [n_iso + 1], needed where theta_without is given */
   const double *d_lr_stat, *d_heir_gain, *d_theta_refit;           /* out: device forms only */
   const int64_t *d_n_unique;
   const int32_t *d_heir, *d_status_without, *d_iters_without, *d_support;
   const double *d_loglik_base;
   const int32_t *d_loo_status, *d_status_base, *d_iters_base;
   const double *d_theta_without;
   const int64_t *d_without_off;
   int32_t *sub_count;                                              /* in, device forms only: [sizes[1]] and [sizes[3]] of the shapes  */
   double *sub_F;                                                   /* call, or NULL: the expanded sub-batch, for a caller that checks it */
} sbgpu_em_loo_t;
typedef struct {
   int64_t max_bytes; /* device scratch one chunk of sub-problems may take; 0: 1 GiB.  Any positive value is legal: consecutive
                         whole loci form a chunk, and a locus above the budget is a chunk alone */
   int64_t reserved;  /* 0 */
} sbgpu_loo_params_t;
/* without_off [n_iso + 1] from iso_off [n_loci + 1] and keep ([n_iso] or NULL) (rule 9).  SBGPU_EINVAL: a NULL array, n_loci < 0,
 * offsets that do not begin at 0 or do not ascend.                                                                        */
int sbgpu_em_loo_offsets(const int64_t *iso_off, const int32_t *keep, int64_t n_loci, int64_t *without_off);
/* Host form (csrc/loo_host.cpp; no GPU needed, free of HIP) in three calls, because the library has no CPU EM: the caller solves
 * the sub-batch between the second and the third.
 * Shapes (rules 1, 2): sizes[4] = the sub-problems, their bins, isoforms and weights together -- always filled; every other
 * output may be NULL (sizes first, then fill): loo_status [n_loci]; sub_locus, sub_drop [sizes[0]]: the parent locus, and the
 * locus-local index of the dropped isoform, -1 for a base; sub_row_off, sub_iso_off, sub_f_off [sizes[0] + 1].  SBGPU_EINVAL:
 * NULL offsets, n_loci < 0, offsets that do not begin at 0 or do not ascend; SBGPU_ESHAPE: rule 1.                          */
int sbgpu_em_loo_shapes_host(int64_t n_loci, const int64_t *row_off, const int64_t *iso_off, const int32_t *keep, int64_t sizes[4],
                             int32_t *loo_status, int32_t *sub_locus, int32_t *sub_drop, int64_t *sub_row_off, int64_t *sub_iso_off,
                             int64_t *sub_f_off);
/* Expansion (rule 2): the sub-batch's counts [sizes[1]] and weights [sizes[3]], a copy of the parent's.  Refusals as
 * sbgpu_em_fit_host's for the batch.                                                                                      */
int sbgpu_em_loo_expand_host(const sbgpu_batch_t *batch, const int32_t *keep, int32_t *sub_count, double *sub_F);
/* Statistics (rules 4-9) from the sub-batch's solve -- sub_theta [sizes[2]], sub_status, sub_iters [sizes[0]] -- and its fit --
 * sub_loglik, sub_n_live, sub_n_dropped, sub_n_impossible [sizes[0]].  SBGPU_EINVAL: a NULL input, malformed offsets,
 * theta_without given without without_off, or a without_off that is not sbgpu_em_loo_offsets' for this batch.              */
int sbgpu_em_loo_stat_host(int64_t n_loci, const int64_t *iso_off, const int32_t *keep, const double *sub_theta, const int32_t *sub_status,
                           const int32_t *sub_iters, const double *sub_loglik, const int64_t *sub_n_live, const int64_t *sub_n_dropped,
                           const int64_t *sub_n_impossible, sbgpu_em_loo_t *out);
/* Device form (csrc/loo_device.h) for any batch sbgpu_em_run_device solves: the plan, d_count and d_F as given to it; d_keep: a
 * device [n_iso] array or NULL; params: NULL for the defaults.  keep is read back once (the shapes are made on the host); then
 * per chunk of loci: a plan for the chunk's sub-batch, loo_expand_kernel -- a workgroup per (locus, row tile), the tile's kept
 * columns staged in LDS once and every sub-copy written from there: bitwise the host expansion, because it is a copy --, the EM
 * through sbgpu_em_run_device, the fit's three launches in this stage's scratch (an earlier fit result of the caller stays
 * valid), loo_stat_kernel.  No atomics.  The integer arrays, support, and which statistics are +inf are the host form's given
 * the same solves; the doubles follow the device EM and the device fit.  Only the arrays the caller gave pointers for cross
 * PCIe.  Synchronises on `stream` (NULL: the context's own).  SBGPU_ESHAPE: rule 1; SBGPU_EINVAL: a NULL argument, counts or
 * weights that are not on the device, theta_without without without_off, a wrong without_off, a negative max_bytes.          */
int sbgpu_em_loo_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const int32_t *d_keep,
                        const sbgpu_loo_params_t *params, void *stream, sbgpu_em_loo_t *out);
/* The same right after a resident call or an sbgpu_front_stream_end made with sbgpu_bootstrap_keep on, from that record, as
 * sbgpu_model_fit_device: nothing more is retained, the call's seven results are the same bits with and without it, and support,
 * info, fit, table, assignment and coverage may be asked for in any order.                                               */
int sbgpu_model_loo_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const int32_t *d_keep, const sbgpu_loo_params_t *params, void *stream,
                           sbgpu_em_loo_t *out);
/* The thresholds (csrc/loo_rules.h, csrc/loo_device.h; reasoned from LDS sizes, not tuned): out[0] the most kept isoforms of a
 * locus whose isoforms are tested; [1] weights of one row tile of the expand kernel (its LDS), [2] the most rows of one tile: a
 * locus of K kept isoforms is cut into tiles of min(out[2], out[1] / K) rows; [3] threads of a workgroup; [4] workgroups per CU
 * a launch's grid is capped at; [5] the default scratch budget in bytes; [6] the most bins and [7] the most isoforms of a locus. */
int sbgpu_em_loo_limits(int64_t out[8]);

/* ---- differential isoform usage: two samples, a pooled-solve likelihood ratio ------------------------------
 * Did isoform usage at a locus change between two samples?  Solve each sample, solve both under ONE shared theta, compare the
 * likelihoods: the question the drop-one support asks of an isoform, asked of a pair of samples.  Two bootstrap intervals cost
 * 2 B solves and have no joint null; a Wald test from two information matrices is one-sided at theta_j near 0.  The rule
 * (csrc/diff_rules.h, shared by both forms, compiled under -ffp-contract=off).  Two batches A and B over the same annotation:
 * the same n_loci and identical iso_off (anything else is SBGPU_EINVAL); each has its own row_off, f_off, count and F; keep_a
 * and keep_b are [n_iso] or NULL.  Every sum starts from 0.0 and adds in ascending index.
 *    1. kept(j) = kept in A OR kept in B (loo_kept's bit on each side; a NULL side keeps everything); K = the kept isoforms of
 *       the locus.  diff_status[l] before the solves: SBGPU_DIFF_EMPTY when K = 0; SBGPU_DIFF_SOLE when K = 1: no solve, lr_stat
 *       0.0 exactly, dof 0, usage 1.0 for the kept isoform in every sample that placed a fragment (a count > 0 in one of the
 *       sample's bins of the locus), 0.0 otherwise; SBGPU_DIFF_TOO_WIDE when K > SBGPU_DIFF_MAX_KEPT (the EM plan's own limit);
 *       SBGPU_DIFF_TOO_DEEP when nb_A + nb_B > SBGPU_DIFF_MAX_POOLED_BINS (the fit's bin limit, for the pooled problem);
 *       SBGPU_DIFF_OK otherwise, tested in this order.  TOO_WIDE and TOO_DEEP are statuses, not refusals of the call: the
 *       neighbours are untouched.  A single sample's locus beyond the fit's limits (5632 bins, 4096 isoforms) refuses the call
 *       with SBGPU_ESHAPE, as the fit does.
 *    2. An OK locus gets three sub-problems, in this order, numbered consecutively over the call (a sub-batch): A -- A's bins and
 *       counts, the kept columns compacted row-major; B -- likewise; POOLED -- A's rows then B's rows, nb_A + nb_B of them, the
 *       counts as they are and the weights SCALED by rule 3.
 *    3. A row of sample s is LIVE when asg_row_live holds on its KEPT weights (what the EM will decide on the compacted
 *       sub-problem).  c^s_j = the sum of kept column j over the live rows of s, in ascending row order.
 *       alpha^s_j = 0.5 * ((c^A_j + c^B_j) / c^s_j) where c^s_j != 0, and 1.0 otherwise: the sum first, then the quotient, then
 *       the product.  A pooled weight is F[b][j] * alpha^s_j.
 *       Why: EmSolver::run renormalises every column over the live rows, so the EM's model for a stacked matrix is
 *       p((s, b) | j) = F~_bj / sum F~_.j.  Stacked raw, isoform j's mass would split between the samples as c^A_j : c^B_j, a
 *       ratio that differs from isoform to isoform (c^s_j depends on which bins sample s observed): a shared theta would NOT be
 *       the joint maximum-likelihood theta.  With alpha every column puts half of its mass in each sample, the responsibilities
 *       are those of the two samples' own column-normalised models, the M-step sums both samples' fragments, and the stacked
 *       solve is the joint MLE under one theta.  When c^A_j ~ c^B_j, alpha ~ 1: the weights keep their raw magnitude and the
 *       1e-5 row threshold keeps its meaning.
 *    4. Each sub-problem is solved as sbgpu_em_run_device solves any locus; the bases are ALWAYS solved inside the call (a locus
 *       solved again alone does not always return a batch's theta bits).  Two fits run with nothing erased (keep NULL): the OWN
 *       fit -- every sub-problem at its own theta and status; the CROSS fit -- sub-problems A and B at the POOLED theta, under
 *       the pooled solve's status.  The fit's loglik is invariant to theta's scale: the pooled theta sums to N_A + N_B and is
 *       used as it is.
 *    5. lr_stat[l] = 2.0 * ((ll_A(theta_A) - ll_A(theta_P)) + (ll_B(theta_B) - ll_B(theta_P))): two subtractions, one sum, one
 *       product -- what each sample's own likelihood loses when both must share theta_P.  It carries no constants and does not
 *       depend on how the pooled matrix was scaled.  dof[l] = K - 1.  All solves stop at SBGPU_EM_THETA_CHANGE_LIMIT, not at
 *       the optimum: small negative values are real and are reported raw.
 *    6. Integers, exact: n_a, n_b = n_live - n_impossible of each base's own fit.  With lost = n_dropped + n_impossible,
 *       lost_shift[l] = lost(POOLED) - lost(A) - lost(B) + (lost(A cross) - lost(A)) + (lost(B cross) - lost(B)).  Non-zero: the
 *       scaling, or the shared theta, moved fragments across the row threshold or made them impossible; lr_stat is still
 *       reported raw, but does not compare like with like.
 *    7. After the solves an OK locus becomes SBGPU_DIFF_ONE_SAMPLE when n_a or n_b is 0 or a base ended SBGPU_EM_INIT_EMPTY;
 *       else SBGPU_DIFF_UNSOLVED when any of the three solves ended SBGPU_EM_DENOM_ZERO.  For a status other than OK or SOLE
 *       every double of the locus and of its isoforms is 0.0, n_a, n_b, lost_shift and dof are 0, and the one index, top_iso,
 *       is -1.  status_a / _b / _pooled and iters_a / _b / _pooled are STILL REPORTED, as the solves left them, for every locus
 *       that had sub-problems -- ONE_SAMPLE and UNSOLVED included: they say why -- and are -1 where it had none (EMPTY, SOLE,
 *       TOO_WIDE, TOO_DEEP).
 *    8. Per isoform: theta_a, theta_b, theta_pooled scattered back, 0.0 where the isoform is not kept or the locus is not OK;
 *       usage_x[j] = theta_x[j] / (the ascending sum of the locus' kept theta_x), 0.0 where that sum is 0;
 *       delta_usage[j] = usage_b[j] - usage_a[j].
 *    9. Per locus: the four log-likelihoods (loglik_a, loglik_b own; loglik_a_pooled, loglik_b_pooled cross), the three statuses
 *       and iteration counts, and top_iso: the locus-local index of the kept isoform of largest |delta_usage| under strict > in
 *       ascending order from -1.0 (a NaN never wins), -1 when there is none.  At K = 2 the usages of each sample sum to 1, so
 *       the two |delta_usage| are equal up to a rounding and top_iso is whichever the roundings favour: read delta_usage there.
 * p-values are the caller's (chi-squared with dof degrees of freedom; strawberry_amd/diff.py has one).
 * CAVEAT.  theta in the reference's model is a share among the bins a sample OBSERVED: the column scale runs over live bins
 * only.  Two samples of very different depth observe different bin sets, and part of a usage difference is then that difference
 * of conditioning; the resident path keeps only observed bins, so two retained samples' bin tables were not built to match.  The
 * rule allows zero counts: both batches on one shared bin table, zero-count rows included, give the test without that
 * difference.  sbgpu_bins_merge_* below builds that table from two samples' bins by key, and sbgpu_model_diff_merged_device runs
 * this rule on it for two retained samples (ChainQuantifier.differential_usage(other, shared_bins=True)); this entry and its
 * default stay as they are.  Out of this rule: more than two samples, replicates and dispersion, multiple-testing
 * corrections, warm starts, multi-rank wiring, columns in the parity writers.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device forms only -- the device arrays of all of them:
 * the (first) context's memory, in a scratch slot of their own, valid until that context's next sbgpu_quantify_* or diff call. */
#define SBGPU_DIFF_MAX_KEPT 512
#define SBGPU_DIFF_MAX_POOLED_BINS 5632
#define SBGPU_DIFF_OK 0
#define SBGPU_DIFF_EMPTY 1
#define SBGPU_DIFF_SOLE 2
#define SBGPU_DIFF_TOO_WIDE 3
#define SBGPU_DIFF_TOO_DEEP 4
#define SBGPU_DIFF_ONE_SAMPLE 5
#define SBGPU_DIFF_UNSOLVED 6
#define SBGPU_DIFF_KIND_A 0
#define SBGPU_DIFF_KIND_B 1
#define SBGPU_DIFF_KIND_POOLED 2
typedef struct {
   double *theta_a, *theta_b, *theta_pooled, *usage_a, *usage_b, *usage_pooled, *delta_usage;   /* in: [n_iso]  */
   double *lr_stat, *loglik_a, *loglik_b, *loglik_a_pooled, *loglik_b_pooled;                    /* in: [n_loci] */
   int64_t *n_a, *n_b, *lost_shift;                                                              /* in: [n_loci] */
   int32_t *dof, *diff_status, *top_iso, *status_a, *status_b, *status_pooled, *iters_a, *iters_b, *iters_pooled; /* in: [n_loci] */
   const double *d_theta_a, *d_theta_b, *d_theta_pooled, *d_usage_a, *d_usage_b, *d_usage_pooled, *d_delta_usage; /* out: device forms only */
   const double *d_lr_stat, *d_loglik_a, *d_loglik_b, *d_loglik_a_pooled, *d_loglik_b_pooled;
   const int64_t *d_n_a, *d_n_b, *d_lost_shift;
   const int32_t *d_dof, *d_diff_status, *d_top_iso, *d_status_a, *d_status_b, *d_status_pooled, *d_iters_a, *d_iters_b, *d_iters_pooled;
   int32_t *sub_count;                          /* in, device forms only: [sizes[1]] and [sizes[3]] of the shapes call, or NULL: the */
   double *sub_F;                               /* expanded sub-batch, for a caller that checks it */
} sbgpu_em_diff_t;
typedef struct {
   int64_t max_bytes; /* device scratch one chunk of sub-problems may take; 0: 1 GiB.  Any positive value is legal: consecutive
                         whole loci form a chunk, and a locus above the budget is a chunk alone */
   int64_t reserved;  /* 0 */
} sbgpu_diff_params_t;
/* Host form (csrc/diff_host.cpp; no GPU needed, free of HIP) in three calls, because the library has no CPU EM: the caller solves
 * the sub-batch between the second and the third, and fits it twice (sbgpu_em_fit_host: own and cross, rule 4).
 * Shapes (rules 1, 2): sizes[4] = the sub-problems, their bins, isoforms and weights together -- always filled; every other
 * output may be NULL (sizes first, then fill): diff_status [n_loci] (before the solves); sub_locus, sub_kind [sizes[0]]: the
 * parent locus and SBGPU_DIFF_KIND_*; sub_row_off, sub_iso_off, sub_f_off [sizes[0] + 1].  SBGPU_EINVAL: NULL offsets,
 * n_loci < 0, offsets that do not begin at 0 or do not ascend; SBGPU_ESHAPE: rule 1.                                         */
int sbgpu_em_diff_shapes_host(int64_t n_loci, const int64_t *row_off_a, const int64_t *row_off_b, const int64_t *iso_off, const int32_t *keep_a,
                              const int32_t *keep_b, int64_t sizes[4], int32_t *diff_status, int32_t *sub_locus, int32_t *sub_kind,
                              int64_t *sub_row_off, int64_t *sub_iso_off, int64_t *sub_f_off);
/* Expansion (rules 2, 3): the sub-batch's counts [sizes[1]] and weights [sizes[3]].  Refusals as sbgpu_em_fit_host's for each
 * batch; SBGPU_EINVAL also where the two batches' n_loci or iso_off differ.                                                */
int sbgpu_em_diff_expand_host(const sbgpu_batch_t *batch_a, const sbgpu_batch_t *batch_b, const int32_t *keep_a, const int32_t *keep_b,
                              int32_t *sub_count, double *sub_F);
/* Statistics (rules 5-9) from the sub-batch's solve -- sub_theta [sizes[2]], sub_status, sub_iters [sizes[0]] --, its own fit --
 * own_loglik, own_n_live, own_n_dropped, own_n_impossible [sizes[0]] -- and its cross fit -- cross_loglik, cross_n_dropped,
 * cross_n_impossible [sizes[0]]; the POOLED entries of the cross arrays are not read.  Of the batches the offsets and the
 * counts are read (F may be NULL).  SBGPU_EINVAL: a NULL input, malformed or differing offsets.                              */
int sbgpu_em_diff_stat_host(const sbgpu_batch_t *batch_a, const sbgpu_batch_t *batch_b, const int32_t *keep_a, const int32_t *keep_b,
                            const double *sub_theta, const int32_t *sub_status, const int32_t *sub_iters, const double *own_loglik,
                            const int64_t *own_n_live, const int64_t *own_n_dropped, const int64_t *own_n_impossible, const double *cross_loglik,
                            const int64_t *cross_n_dropped, const int64_t *cross_n_impossible, sbgpu_em_diff_t *out);
/* Device form (csrc/diff_device.h) for two batches sbgpu_em_run_device solves, both on ctx's device: each plan, d_count and d_F
 * as given to it; d_keep_a, d_keep_b: device [n_iso] arrays or NULL; params: NULL for the defaults.  The keeps are read back once
 * (the shapes are made on the host, by the function the host form calls); then per chunk of loci: a plan for the chunk's
 * sub-batch, diff_colscale_kernel (rule 3's live rows, c and alpha, the column sums in ascending row order), diff_expand_kernel
 * (a workgroup per row tile; own copies are stores of loaded values, a pooled weight is one product: bitwise the host
 * expansion), the EM through sbgpu_em_run_device, diff_cross_kernel, the fit's three launches twice in this stage's scratch (an
 * earlier fit result of the caller stays valid), diff_stat_kernel.  No atomics.  Every integer, every status and -- given the
 * same solves and fits -- every double are the host form's.  Only the arrays the caller gave pointers for cross PCIe.
 * Synchronises on `stream` (NULL: the context's own).  SBGPU_ESHAPE: rule 1; SBGPU_EINVAL: a NULL argument, plans that differ in
 * n_loci or iso_off, counts or weights that are not on the device, a negative max_bytes.                                    */
int sbgpu_em_diff_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan_a, const int32_t *d_count_a, const double *d_F_a, const sbgpu_plan_t *plan_b,
                         const int32_t *d_count_b, const double *d_F_b, const int32_t *d_keep_a, const int32_t *d_keep_b,
                         const sbgpu_diff_params_t *params, void *stream, sbgpu_em_diff_t *out);
/* The same from what two contexts' resident calls (or sbgpu_front_stream_end) kept with sbgpu_bootstrap_keep on: sample A is
 * ctx_a's record, sample B ctx_b's; each handle is checked against its context's record as sbgpu_model_loo_device checks one.
 * The two contexts must be on the same device (SBGPU_EINVAL otherwise); ctx_b's own stream is synchronised before its arrays
 * are read; the work, the sub-batch's plan and the scratch are ctx_a's.  Neither record changes: both calls' seven results are
 * the same bits with and without it, and every other stage still answers on both contexts, in any order.                    */
int sbgpu_model_diff_device(sbgpu_ctx_t *ctx_a, const sbgpu_bins_t *bins_a, sbgpu_ctx_t *ctx_b, const sbgpu_bins_t *bins_b, const int32_t *d_keep_a,
                            const int32_t *d_keep_b, const sbgpu_diff_params_t *params, void *stream, sbgpu_em_diff_t *out);
/* The thresholds (csrc/diff_rules.h, csrc/diff_device.h; reasoned from LDS sizes, not tuned): out[0] the most kept isoforms of
 * a tested locus; [1] the most pooled bins; [2] weights of one row tile of the expand kernel, [3] the most rows of one tile: a
 * locus of K kept isoforms is cut into tiles of max(1, min(out[3], out[2] / K)) rows; [4] kept isoforms up to which the
 * column-scale kernel serves a locus with a group of lanes (several loci to a workgroup), a whole workgroup beyond; [5] threads
 * of a workgroup; [6] workgroups per CU a launch's grid is capped at; [7] the default scratch budget in bytes.              */
int sbgpu_em_diff_limits(int64_t out[8]);

/* ---- differential isoform usage between two GROUPS of replicate samples -------------------------------------
 * A one-sample against one-sample likelihood ratio has no estimate of biological variation: two samples whose shares were
 * drawn independently reject almost every locus.  Experiments come as two conditions with a few replicates each, and the
 * question is whether usage differs between the conditions by MORE than it differs among replicates.  The pooled-solve rule
 * above generalises: a pool of P samples gives every sample 1/P of each column's mass.  The rule (csrc/gdiff_rules.h, shared by
 * both forms, compiled under -ffp-contract=off):
 * Group A holds n_a >= 1 batches and group B n_b >= 1; S = n_a + n_b <= SBGPU_GDIFF_MAX_SAMPLES (anything else, 0 samples in a
 * group included, is SBGPU_EINVAL).  All batches are over one annotation: the same n_loci and identical iso_off, else
 * SBGPU_EINVAL; each has its own row_off, f_off, count, F and optional keep.  Samples are numbered A's first, in the caller's
 * order.  Every sum starts from its first term and adds in ascending index.
 *    1. kept(j) = kept in ANY sample (loo_kept's bit per sample; a NULL keep keeps everything); K = the kept isoforms of the
 *       locus.  Sample s is PRESENT at a locus when it has at least one bin there (nb_s > 0): decided from offsets alone.  p_a
 *       and p_b are the present samples of the two groups.  gdiff_status[l] before the solves, tested in this order:
 *       SBGPU_DIFF_EMPTY when K = 0; SBGPU_DIFF_SOLE when K = 1: no solve, both statistics 0.0, both dofs 0, usage 1.0 for
 *       the kept isoform in every present sample that placed a fragment (a count > 0), in every group one of whose samples
 *       did, and in ALL where any did, 0.0 otherwise; SBGPU_DIFF_TOO_WIDE when K > SBGPU_DIFF_MAX_KEPT;
 *       SBGPU_GDIFF_ONE_GROUP when p_a = 0 or p_b = 0; SBGPU_DIFF_TOO_DEEP when the present samples' bins together exceed
 *       SBGPU_DIFF_MAX_POOLED_BINS; SBGPU_DIFF_OK otherwise.  These are statuses, not refusals of the call.  A single sample's
 *       locus beyond the fit's limits (5632 bins, 4096 isoforms) refuses the call with SBGPU_ESHAPE, as the fit does.
 *    2. The sub-problems of an OK locus, in this order, numbered consecutively over the call (a sub-batch): one OWN
 *       sub-problem per present sample, in sample order -- the kept columns compacted, row-major; GROUP_A, if p_a >= 2 -- A's
 *       present samples' rows stacked in sample order, scaled by rule 3; GROUP_B, if p_b >= 2; ALL -- every present sample's
 *       rows, A's then B's, scaled.  A group with ONE present sample has no group sub-problem: its group theta, status and
 *       group-level fit ARE that sample's own -- the same numbers, not a second solve.
 *    3. Row liveness (asg_row_live on the kept weights) and c^s_j are exactly rule 3 of the two-sample test.  For a pool P of
 *       present samples, alpha^{s,P}_j = ((sum over t in P of c^t_j) / c^s_j) / (double)|P| where c^s_j != 0, and 1.0 otherwise:
 *       the sum first, in ascending sample order, then the quotient, then the division.  At |P| = 2 this is the two-sample
 *       alpha bit for bit.  Why: the EM renormalises every column over the live rows, so with alpha every column puts 1/|P| of
 *       its mass in each sample of the pool, the responsibilities are those of the samples' own column-normalised models, the
 *       M-step sums all their fragments, and the stacked solve is the joint MLE under one theta -- the two-sample argument.
 *    4. Every sub-problem is solved inside the call as sbgpu_em_run_device solves any locus.  Three fits run over the
 *       sub-batch with nothing erased: OWN -- every sub-problem at its own theta and status; GROUP cross -- every OWN
 *       sub-problem at its group's theta and status; ALL cross -- every OWN sub-problem at ALL's theta and status.
 *    5. For a present sample s let own_s = ll_s(theta_s), grp_s = ll_s(theta_g(s)), all_s = ll_s(theta_ALL).
 *       lr_between = 2.0 * sum_s (grp_s - all_s), dof_between = K - 1: what the groups lose when they must share one theta.
 *       lr_within = 2.0 * sum_s (own_s - grp_s), dof_within = (p_a + p_b - 2)(K - 1): what the replicates lose when each
 *       group shares one -- the estimate of biological variation, on the same scale.  Each loss is one subtraction, the sum
 *       runs over the present samples in order, there is one product.  A singleton group's samples contribute exactly 0.0 to
 *       lr_within.  Both are reported raw: every solve stops at SBGPU_EM_THETA_CHANGE_LIMIT, so small negatives are real.
 *    6. Integers, exact: n_frag[s] = n_live - n_impossible of s's own fit.  With lost(.) = n_dropped + n_impossible,
 *       lost_shift = (lost(ALL) - sum_s lost(s)) + sum over the groups with a sub-problem (lost(G) - sum_{s in G} lost(s))
 *       + sum_s (lost(s at its group's theta) - lost(s)) + sum_s (lost(s at ALL's theta) - lost(s)).  At 1 + 1 samples this is
 *       the two-sample expression.
 *    7. After the solves an OK locus becomes SBGPU_GDIFF_THIN when a present sample has n_frag = 0 or its solve ended
 *       SBGPU_EM_INIT_EMPTY; otherwise SBGPU_DIFF_UNSOLVED when any solve of the locus ended SBGPU_EM_DENOM_ZERO.  For a status
 *       other than OK or SOLE every double of the locus and of its isoforms is 0.0, n_frag, lost_shift and the dofs are 0,
 *       top_iso is -1.  p_a and p_b are always reported.  The statuses and iteration counts of the sub-problems are STILL
 *       REPORTED where sub-problems existed (a singleton group's are its sample's), and are -1 where none existed and for an
 *       absent sample.
 *    8. Per isoform: theta_sample [S x n_iso], sample-major, 0.0 for an absent sample; theta_group [2 x n_iso]; theta_all
 *       [n_iso]; the usages likewise, each theta over the ascending sum of its sub-problem's theta (0.0 where that is 0);
 *       delta_usage = usage_group[B] - usage_group[A].
 *    9. Per locus: the two statistics and dofs, p_a, p_b, loglik_own, loglik_group, loglik_all and n_frag [S x n_loci]
 *       (sample-major), lost_shift, the final status, top_iso -- the two-sample rule 9 on the two GROUP usages, with the same
 *       K = 2 remark --, status_sample / iters_sample [S x n_loci], status_group / iters_group [2 x n_loci], status_all /
 *       iters_all [n_loci].
 * THE ANCHOR.  With n_a = n_b = 1 and both samples present at a locus the sub-batch is the two-sample A, B, POOLED in the same
 * order; lr_between, every theta, usage, log-likelihood, integer and top_iso are sbgpu_em_diff_device's bits; lr_within is 0.0
 * and dof_within 0.  Where a sample is absent the two-sample rule says ONE_SAMPLE and this one ONE_GROUP; where a present
 * sample placed nothing, ONE_SAMPLE there is THIN here.
 * p-values are the caller's (strawberry_amd/gdiff.py: chi-squared on lr_between, or the quasi-likelihood F test
 * F = (lr_between / dof_between) / max(1, lr_within / dof_within) on (dof_between, dof_within) degrees of freedom).  The CAVEAT
 * of the two-sample rule holds per sample: each is tested on the bins it observed.  Out of this rule: more than two groups, an
 * N-way merge onto one bin table (shared_bins for groups), multiple-testing correction, warm starts, multi-rank wiring, columns
 * in the parity writers.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device forms only -- the device arrays of all of them:
 * the (first) context's memory, in a scratch slot of their own, valid until that context's next sbgpu_quantify_* or gdiff call. */
#define SBGPU_GDIFF_MAX_SAMPLES 16
#define SBGPU_GDIFF_ONE_GROUP 7
#define SBGPU_GDIFF_THIN 8
#define SBGPU_GDIFF_KIND_OWN 0
#define SBGPU_GDIFF_KIND_GROUP_A 1
#define SBGPU_GDIFF_KIND_GROUP_B 2
#define SBGPU_GDIFF_KIND_ALL 3
typedef struct {
   double *theta_sample, *theta_group, *theta_all, *usage_sample, *usage_group, *usage_all, *delta_usage; /* in: [S | 2 | 1 x n_iso] */
   double *lr_between, *lr_within, *loglik_own, *loglik_group, *loglik_all;                                /* in: [n_loci]; loglik_*: [S x n_loci] */
   int64_t *n_frag, *lost_shift;                                                                           /* in: [S x n_loci], [n_loci] */
   int32_t *dof_between, *dof_within, *p_a, *p_b, *gdiff_status, *top_iso;                                 /* in: [n_loci] */
   int32_t *status_sample, *iters_sample, *status_group, *iters_group, *status_all, *iters_all;           /* in: [S | 2 | 1 x n_loci] */
   const double *d_theta_sample, *d_theta_group, *d_theta_all, *d_usage_sample, *d_usage_group, *d_usage_all, *d_delta_usage; /* out: device forms only */
   const double *d_lr_between, *d_lr_within, *d_loglik_own, *d_loglik_group, *d_loglik_all;
   const int64_t *d_n_frag, *d_lost_shift;
   const int32_t *d_dof_between, *d_dof_within, *d_p_a, *d_p_b, *d_gdiff_status, *d_top_iso;
   const int32_t *d_status_sample, *d_iters_sample, *d_status_group, *d_iters_group, *d_status_all, *d_iters_all;
   int32_t *sub_count;                          /* in, device forms only: [sizes[1]] and [sizes[3]] of the shapes call, or NULL: the */
   double *sub_F;                               /* expanded sub-batch, for a caller that checks it */
} sbgpu_em_gdiff_t;
typedef struct {
   int64_t max_bytes; /* device scratch one chunk of sub-problems may take; 0: 1 GiB.  Any positive value is legal: consecutive
                         whole loci form a chunk, and a locus above the budget is a chunk alone */
   int64_t reserved;  /* 0 */
} sbgpu_gdiff_params_t;
/* Host form (csrc/gdiff_host.cpp; no GPU needed, free of HIP) in three calls around a solver the caller brings, as the
 * two-sample one: the caller solves the sub-batch between the second and the third and fits it three times
 * (sbgpu_em_fit_host: own, group cross, ALL cross; rule 4).  Samples are given as arrays of S = n_a + n_b pointers, A's first.
 * Shapes (rules 1, 2): row_off [S] pointers to [n_loci + 1] arrays; keep [S] pointers to [n_iso] arrays, any of them or the
 * array itself NULL.  sizes[4] = the sub-problems, their bins, isoforms and weights together -- always filled; every other
 * output may be NULL: gdiff_status [n_loci] (before the solves); sub_locus, sub_kind (SBGPU_GDIFF_KIND_*), sub_sample (-1 for a
 * group's and ALL's) [sizes[0]]; sub_row_off, sub_iso_off, sub_f_off [sizes[0] + 1].  SBGPU_EINVAL: the group sizes, NULL
 * offsets, n_loci < 0, offsets that do not begin at 0 or do not ascend; SBGPU_ESHAPE: rule 1.                              */
int sbgpu_em_gdiff_shapes_host(int64_t n_loci, int32_t n_a, int32_t n_b, const int64_t *const *row_off, const int64_t *iso_off,
                               const int32_t *const *keep, int64_t sizes[4], int32_t *gdiff_status, int32_t *sub_locus, int32_t *sub_kind,
                               int32_t *sub_sample, int64_t *sub_row_off, int64_t *sub_iso_off, int64_t *sub_f_off);
/* Expansion (rules 2, 3): the sub-batch's counts [sizes[1]] and weights [sizes[3]].  Refusals as sbgpu_em_fit_host's for each
 * batch; SBGPU_EINVAL also where the batches' n_loci or iso_off differ.                                                    */
int sbgpu_em_gdiff_expand_host(int32_t n_a, int32_t n_b, const sbgpu_batch_t *const *batches, const int32_t *const *keep, int32_t *sub_count,
                               double *sub_F);
/* Statistics (rules 5-9) from the sub-batch's solve -- sub_theta [sizes[2]], sub_status, sub_iters [sizes[0]] --, its own fit --
 * own_loglik, own_n_live, own_n_dropped, own_n_impossible [sizes[0]] -- and its two cross fits -- group_* and all_*: loglik,
 * n_dropped, n_impossible [sizes[0]]; only the OWN sub-problems' entries of the cross arrays are read.  Of the batches the
 * offsets and the counts are read (F may be NULL).  SBGPU_EINVAL: a NULL input, malformed or differing offsets.            */
int sbgpu_em_gdiff_stat_host(int32_t n_a, int32_t n_b, const sbgpu_batch_t *const *batches, const int32_t *const *keep, const double *sub_theta,
                             const int32_t *sub_status, const int32_t *sub_iters, const double *own_loglik, const int64_t *own_n_live,
                             const int64_t *own_n_dropped, const int64_t *own_n_impossible, const double *group_loglik,
                             const int64_t *group_n_dropped, const int64_t *group_n_impossible, const double *all_loglik,
                             const int64_t *all_n_dropped, const int64_t *all_n_impossible, sbgpu_em_gdiff_t *out);
/* Device form (csrc/gdiff_device.h) for S batches sbgpu_em_run_device solves, all on ctx's device: plans, d_count, d_F: host
 * arrays of S entries, each as given to it; d_keep: a host array of S device [n_iso] arrays (any NULL), or NULL; params: NULL
 * for the defaults.  The keeps are read back once (the shapes are made on the host, by the function the host form calls); the
 * samples' arrays reach the kernels through a small device table indexed by sample, not through kernel arguments.  Per chunk
 * of consecutive whole loci: a plan for the chunk's sub-batch, gdiff_colscale_kernel (rule 3's live rows, c, the pools' sums
 * and the two alphas), gdiff_expand_kernel (a workgroup per row tile of one sample; a weight is loaded once and stored up to
 * three times: bitwise the host expansion), the EM through sbgpu_em_run_device, gdiff_cross_kernel and the fit's launches for
 * the group level, the same for ALL, the own fit, gdiff_stat_kernel, one synchronisation.  No atomics.  Every integer, every
 * status and -- given the same solves and fits -- every double are the host form's.  Only the arrays the caller gave pointers
 * for cross PCIe.  Synchronises on `stream` (NULL: the context's own).  SBGPU_ESHAPE: rule 1; SBGPU_EINVAL: a NULL argument,
 * the group sizes, plans that differ in n_loci or iso_off, counts or weights that are not on the device, a negative max_bytes. */
int sbgpu_em_gdiff_device(sbgpu_ctx_t *ctx, int32_t n_a, int32_t n_b, const sbgpu_plan_t *const *plans, const int32_t *const *d_count,
                          const double *const *d_F, const int32_t *const *d_keep, const sbgpu_gdiff_params_t *params, void *stream,
                          sbgpu_em_gdiff_t *out);
/* The same from what S contexts' resident calls (or sbgpu_front_stream_end) kept with sbgpu_bootstrap_keep on: sample s is
 * ctxs[s]'s record; each handle is checked against its context's record as sbgpu_model_loo_device checks one.  All contexts
 * must be on one device (SBGPU_EINVAL otherwise); every other context's own stream is synchronised before its arrays are read;
 * the work, the sub-batch's plan and the scratch are the first context's.  No record changes: every call's seven results are
 * the same bits with and without it, and every other stage still answers on every context, in any order.                   */
int sbgpu_model_gdiff_device(int32_t n_a, int32_t n_b, sbgpu_ctx_t *const *ctxs, const sbgpu_bins_t *const *bins, const int32_t *const *d_keep,
                             const sbgpu_gdiff_params_t *params, void *stream, sbgpu_em_gdiff_t *out);
/* The thresholds (csrc/gdiff_rules.h, csrc/gdiff_device.h; the two-sample kernels' shapes are kept): out[0] the most kept
 * isoforms of a tested locus; [1] the most bins of the present samples together; [2] weights of one row tile of the expand
 * kernel, [3] the most rows of one tile; [4] kept isoforms up to which the column-scale kernel serves a locus with a group of
 * lanes; [5] threads of a workgroup; [6] workgroups per CU a launch's grid is capped at; [7] the default scratch budget in
 * bytes; [8] the most samples of a call.                                                                                    */
int sbgpu_em_gdiff_limits(int64_t out[9]);

/* ---- two samples on ONE bin table: the merge of two bin tables by key ---------------------------------------
 * The differential usage above conditions each sample on the bins it observed.  The merge gives both samples the union of their
 * bins, with zero counts where a sample saw nothing, so that the unchanged rule above tests them on one bin set.  The rule
 * (csrc/merge_rules.h, shared by both forms):
 *    1. Two samples A and B over the same annotation: the same n_loci, identical iso_off and the same key_words >= 1 (anything
 *       else is SBGPU_EINVAL); each has row_off [n_loci + 1], key [n_bins * key_words], count [n_bins] and F [n_elem], row-major,
 *       n_elem = the sum of bins x isoforms over the loci.  Two keys are equal when all key_words words are.  Keys are unique
 *       inside a sample's locus: a duplicate in either sample is SBGPU_EINVAL and sbgpu_last_error names the (lowest such) locus,
 *       in both forms.
 *    2. The union rows of locus l are A's bins in A's order, then the bins of B whose key does not occur among A's, in B's
 *       order: nb_U = nb_A + #(B-only).  row_a[r] / row_b[r] = the GLOBAL bin of union row r in A / in B, or -1.  row_off_u and
 *       f_off_u are the union's offsets over the same iso_off; both samples share them.
 *    3. count_u_s[r] = count_s[row_s[r]], 0 where row_s[r] is -1.  F_u_s[r][j] = F_s[row_s[r]][j] where the sample has the row:
 *       its own bits.  Otherwise F_u_s[r][j] = X_s[row_other[r]][j], where X_s has the OTHER sample's shape: the other sample's
 *       bins weighed under THIS sample's insert law.  X NULL: the other sample's own weights are taken -- exact when both samples
 *       were given one law, and for long reads, where a weight does not depend on the law.
 *    4. LIMITATION.  Which isoforms a bin is paired with is the union of compatibilities over the hits of the sample that
 *       observed it.  A bin both samples observed keeps, in each sample, that sample's own pair set; a bin only one sample
 *       observed hands its pair set to the other.  Uniting the pair sets of shared bins is out of this rule.
 *    5. A single sample's locus beyond 5632 bins or 4096 isoforms, or a union of more than 5632 rows, refuses the call with
 *       SBGPU_ESHAPE, naming the locus, as the fit does.  2 * nb_U > SBGPU_DIFF_MAX_POOLED_BINS is NOT a refusal: the
 *       differential rule reports SBGPU_DIFF_TOO_DEEP for that locus.
 *    6. The deep form of the device match files keys under h = 0x811C9DC5; per word h = (h ^ word) * 0x01000193 (mod 2^32);
 *       slot = (h ^ (h >> 15)) mod out[1] of sbgpu_bins_merge_limits; a hash match is confirmed on all words, so the hash is
 *       no part of the result.
 * Footprint: the merged arrays of a whole sample pair are held at once -- 2 * n_elem_U * 8 bytes of weights, n_bins_U * 16 of
 * row maps and counts, roughly twice one sample's F -- beside n_bins_A * 4 + n_bins_B * 4 of match results; there is no chunking. */
typedef struct {
   int64_t n_loci;
   const int64_t *iso_off, *row_off; /* host, [n_loci + 1] in every form */
   int32_t key_words;
   int32_t reserved;                 /* 0 */
   const uint32_t *key;              /* [n_bins * key_words] */
   const int32_t *count;             /* [n_bins] */
   const double *F;                  /* [n_elem] */
   const double *X;                  /* [n_elem of the OTHER sample] or NULL (rule 3) */
} sbgpu_merge_sample_t;
typedef struct {
   int64_t n_bins, n_elem;                                      /* out: the union's rows and weights */
   int64_t *row_off, *f_off;                                    /* in: host [n_loci + 1] to fill, or NULL */
   const int32_t *d_row_a, *d_row_b, *d_count_a, *d_count_b;    /* out: device [n_bins] */
   const double *d_F_a, *d_F_b;                                 /* out: device [n_elem] */
} sbgpu_bins_merged_t;
/* Host form (csrc/merge_host.cpp; no GPU needed, free of HIP).  Shapes: sizes[2] = n_bins_U, n_elem_U -- always filled; every
 * other output may be NULL (sizes first, then fill): row_off_u, f_off_u [n_loci + 1]; row_a, row_b [sizes[0]].  Of the samples
 * the offsets and the keys are read.  Fill: count_a, count_b [sizes[0]], F_a, F_b [sizes[1]] (each may be NULL).               */
int sbgpu_bins_merge_shapes_host(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, int64_t sizes[2], int64_t *row_off_u,
                                 int64_t *f_off_u, int32_t *row_a, int32_t *row_b);
int sbgpu_bins_merge_fill_host(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, int32_t *count_a, int32_t *count_b, double *F_a,
                               double *F_b);
/* Device form (csrc/merge_device.h): the samples' key, count, F and X are device arrays on ctx's device, the offsets host arrays.
 * The match (merge_match_small_kernel: a group of lanes of one wave per locus, no LDS; merge_match_deep_kernel: a workgroup
 * per locus, A's keys in an LDS table of open addressing), one read-back of the per-locus B-only counts (a duplicate key is
 * reported through them), the offsets on the host by the function the host form calls, the fill (merge_fill_kernel: a
 * workgroup per tile of union rows, every output element written by exactly one thread; no global atomics), one
 * synchronisation on `stream` (NULL: the context's own).  Every integer and every double is the host form's.  The device
 * arrays lie in a scratch slot of their own and are valid until that context's next sbgpu_quantify_* or merge call.          */
int sbgpu_bins_merge_device(sbgpu_ctx_t *ctx, const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, void *stream,
                            sbgpu_bins_merged_t *out);
/* Copies the arrays the caller names (each may be NULL) of a merge that is still valid to host buffers sized from its n_bins
 * and n_elem; synchronises on `stream`.                                                                                       */
int sbgpu_bins_merge_fetch(sbgpu_ctx_t *ctx, const sbgpu_bins_merged_t *merged, int32_t *row_a, int32_t *row_b, int32_t *count_a,
                           int32_t *count_b, double *F_a, double *F_b, void *stream);
/* The thresholds (csrc/merge_rules.h, csrc/merge_device.h; from sizes -- a wave, the CU's 160 KB of LDS --, not tuned): out[0]
 * bins of one sample up to which a locus takes the small form of the match (both samples at or below it; a lane per bin inside
 * one wave64), the deep form beyond; [1] slots of the deep form's LDS table (the power of two at or above twice [2]: 64 KB, two
 * workgroups to a CU); [2] the most rows of a union, and bins of one sample's locus; [3] weights of one tile of the fill, [4] the
 * most rows of one tile: a locus of K isoforms is cut into tiles of max(1, min(out[4], out[3] / K)) rows; [5] threads of a
 * workgroup; [6] workgroups per CU a launch's grid is capped at; [7] key words a lane of the small form holds in registers.   */
int sbgpu_bins_merge_limits(int64_t out[8]);
/* The differential usage of two RETAINED samples on one bin table: what sbgpu_model_diff_device takes, checked as it checks
 * them (the same refusals).  Needs the handles' bin keys and (bin, isoform) pairs on the device: SBGPU_EUNSUPPORTED for a handle
 * whose bins were grouped on the host (one from sbgpu_quantify_host is one); SBGPU_ESHAPE for a pair wider than 32 segments
 * under a law that is not long_read.  Each record holds a host copy of the insert-size law its call weighed its bins under.
 * The work: each law's table (sbgpu_insert_pdf_table) is built and uploaded; X_A = ALL of B's pairs weighed under A's law into a
 * zeroed [n_elem_B] array by one sbgpu_binweight_device launch over B's own out_index, X_B likewise (a launch each, about the
 * cost of a sample's own weight stage, and no pair compaction: the rows the fill does not read are the price); the merge
 * above; ONE plan over the union's offsets, which serves both samples; sbgpu_em_diff_device on (count_u_A, F_u_A) and
 * (count_u_B, F_u_B), unchanged.  Neither record changes; the work and the scratch are ctx_a's; ctx_b's stream is synchronised
 * before its arrays are read.  merged_out (optional): the merge, as sbgpu_bins_merge_device reports it.  out NULL (merged_out
 * given): the merge alone -- sbgpu_last_stage_ms then lists merge_xweights_a, merge_xweights_b, merge_match, merge_fill.        */
int sbgpu_model_diff_merged_device(sbgpu_ctx_t *ctx_a, const sbgpu_bins_t *bins_a, sbgpu_ctx_t *ctx_b, const sbgpu_bins_t *bins_b,
                                   const int32_t *d_keep_a, const int32_t *d_keep_b, const sbgpu_diff_params_t *params, void *stream,
                                   sbgpu_em_diff_t *out, sbgpu_bins_merged_t *merged_out);

/* ---- the EM bootstrap: how far theta can be trusted -------------------------
 * The reference prints theta with no statement of its spread.  The bootstrap resamples every locus' fragments over its
 * bins, solves again, and reports mean and variance of theta over the replicates.
 *
 * The resampling rule (csrc/bootstrap_rules.h; the host form and the kernels call the same functions).  A locus has a
 * global id g, rows with counts n_i >= 0, N = sum n_i and prefix sums P_i = n_0 + ... + n_{i-1}.  Replicate r (0 <= r <
 * 2^24) under seed s makes N draws d = 0 .. N-1: with q = d >> 1, Philox4x32-10 (Random123 constants) runs on the counter
 * (q & 0xffffffff, (q >> 32) | (r << 8), g & 0xffffffff, g >> 32) under the key (s & 0xffffffff, s >> 32); an even d
 * takes u = o0 | o1 << 32 of its four output words, an odd d takes u = o2 | o3 << 32; t = (u * N) >> 64, and the draw lands
 * on the row i with P_i <= t < P_{i+1}.  The replicate's count of a row is the number of draws that land on it.  So: a
 * replicate's total is N, a zero row stays zero, and the result depends on (g, r, s) and the locus' counts only -- not on
 * the batch the locus sits in, its place there, the number of replicates of the call, or how the work is split.
 * A locus of N >= 2^40: SBGPU_ESHAPE.  A negative count, a replicate number outside [0, 2^24), n_rep < 1: SBGPU_EINVAL.  */
typedef struct {
   int32_t n_rep;            /* B >= 1 replicates, numbered rep_first .. rep_first + B - 1 */
   int32_t rep_first;
   uint64_t seed;
   const int64_t *locus_id;  /* HOST [n_loci] global ids, or NULL: the locus' index in the batch */
} sbgpu_bootstrap_params_t;

/* One replicate's counts, host arrays (csrc/bootstrap_host.cpp; no GPU needed).  row_off: HOST [n_loci + 1].            */
int sbgpu_bootstrap_counts_host(int64_t n_loci, const int64_t *row_off, const int32_t *count,
                                const int64_t *locus_id, uint64_t seed, int32_t rep, int32_t *count_out);
/* n_rep replicates' counts on the device: d_count_out[n_rep][row_off[n_loci]], bit for bit the host form's; d_count is
 * not written.  row_off: HOST.  Returns once `stream` has finished them.                                               */
int sbgpu_bootstrap_counts_device(sbgpu_ctx_t *ctx, int64_t n_loci, const int64_t *row_off, const int32_t *d_count,
                                  const sbgpu_bootstrap_params_t *params, int32_t *d_count_out, void *stream);
/* Resample -> EM for every replicate -> statistics.  Replicate k is exactly sbgpu_em_run_device on the counts of
 * replicate rep_first + k and d_F: the same kernels, the same status and iteration contract, failures reported through
 * sbgpu_synchronize.  d_mean / d_var [n_iso]: Welford's recurrence over the replicates in replicate order,
 *    m_k = m_{k-1} + (x_k - m_{k-1}) / k,  M2_k = M2_{k-1} + (x_k - m_{k-1}) (x_k - m_k),  var = M2_B / (B - 1)  (0 for B = 1).
 * Every replicate enters, whatever its status (a DENOM_ZERO replicate carries theta_0, as in the reference; an INIT_EMPTY
 * locus depends on F alone and has that status in all replicates).  d_status_count [n_loci][4]: replicates per SBGPU_EM_*
 * status.  d_theta_rep [n_rep][n_iso], d_status_rep / d_iters_rep [n_rep][n_loci]: every replicate's results, each may be
 * NULL.  Nothing depends on how the call schedules its replicates; d_count, d_F and the plan are left as they were (the
 * replicates' counts live in the context's pooled scratch, two sets: replicate k + 1 is resampled and solved while the
 * statistics of replicate k run).  The call waits once, at its start, for `stream` and the counts' totals (a negative
 * count or a locus of 2^40 fragments is reported by the call itself); the replicates are then queued: asynchronous on
 * `stream`.  One bootstrap per context at a time (a second call's work queues behind the first's).                     */
int sbgpu_em_bootstrap_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                              const sbgpu_bootstrap_params_t *params,
                              double *d_mean, double *d_var,          /* [n_iso] */
                              int32_t *d_status_count,                /* [n_loci][4] */
                              double *d_theta_rep,                    /* [n_rep][n_iso] or NULL */
                              int32_t *d_status_rep, int32_t *d_iters_rep, /* [n_rep][n_loci] or NULL */
                              void *stream);

/* ---- the bootstrap of the resident path: FPKM / TPM mean, spread and intervals -----------------------------
 * Statistics over the replicates of one column (csrc/bootstrap_rules.h; the host form and boot_interval_kernel call the same
 * functions).  x[n_rep][n] is replicate-major.  For column j: mean and var are Welford's recurrence in replicate order, as
 * above; lo[j] / hi[j] are the elements at the 0-based positions rank_lo / rank_hi of the column sorted ascending under <,
 * NaNs last: pure order statistics, no interpolation, so lo and hi are bits of input elements (ties: -0.0 sorts in front of
 * +0.0; a NaN comes back with its sign bit cleared), and the ranks are integers, so no rounding decides which replicate is
 * picked.  SBGPU_EINVAL unless n_rep >= 1 and 0 <= rank_lo <= rank_hi < n_rep.  mean / var / lo / hi: [n], each may be NULL.
 * Device form: device pointers, asynchronous on `stream`; n_rep <= 1024 (a wave sorts a column in its registers), above:
 * SBGPU_ESHAPE.  The host form has no cap.                                                                                 */
int sbgpu_replicate_stats_host(int32_t n_rep, int64_t n, const double *x, int32_t rank_lo, int32_t rank_hi,
                               double *mean, double *var, double *lo, double *hi);
int sbgpu_replicate_stats_device(sbgpu_ctx_t *ctx, int32_t n_rep, int64_t n, const double *d_x, int32_t rank_lo, int32_t rank_hi,
                                 double *d_mean, double *d_var, double *d_lo, double *d_hi, void *stream);
/* on != 0: the context's LATER sbgpu_quantify_resident / sbgpu_front_stream_end calls leave what
 * sbgpu_abundance_bootstrap_device needs: the call's EM plan (the context owns it from then on: destroyed by its next
 * sbgpu_quantify_* call and by sbgpu_finalize) and device pointers the call had anyway -- the bins' counts, the bin weights,
 * the isoforms' lengths -- with the epilogue's parameters as the call filled them in.  Nothing is copied, and theta, FPKM,
 * Frac, TPM, keep, status and iters are the same bits.  Off (the default): those calls are unchanged.  May be on together
 * with sbgpu_context_table_keep.                                                                                            */
int sbgpu_bootstrap_keep(sbgpu_ctx_t *ctx, int32_t on);
/* Right after such a call, on the handle it returned (which must still live), before the context's next call that works in
 * its scratch memory (as for sbgpu_context_table_device): SBGPU_EINVAL otherwise -- a handle made without retention, or a
 * stale one; sbgpu_last_error says which.  The call itself works in the context's bootstrap scratch and pooled blocks only:
 * sbgpu_context_table_device stays valid before and after it, and it may be repeated.
 * For replicate k (number rep_first + k; seed, locus_id and the double buffering as sbgpu_em_bootstrap_device): resample,
 * the EM, step k of theta's statistics and the status counts, then the reference's epilogue (abundance_kernel, the call's
 * retained parameters) on this replicate's theta and status: FPKM into row k of d_fpkm_rep, keep into row k of d_keep_rep
 * (one int32 per isoform, 0 / 1 / 2 as sbgpu_abundances_t's keep: not packed), this rank's kept-FPKM sum into entry k of the
 * totals.  total_mapped_reads and the insert law are the SAMPLE's and are not resampled.  After the last replicate: ONE
 * all-reduce(sum) of the n_rep totals over `comm` (NULL: a world of one; otherwise every rank of the communicator makes this
 * call with the same n_rep; argument checks and every allocation happen before the first kernel, so a rank that is going to
 * fail fails before its peers wait), then the statistics above over the columns of d_fpkm_rep, twice:
 *    fpkm_*  on x_k = fpkm_rep[k][j], whatever keep says;
 *    tpm_*   on x_k = keep_rep[k][j] ? 1e6 * fpkm_rep[k][j] / total[k] : 0.0 (tpm_kernel's expression; no TPM matrix is written),
 *            and keep_count[j] = the number of k with keep_rep[k][j] != 0.
 * theta_mean / theta_var / status_count are sbgpu_em_bootstrap_device's d_mean / d_var / d_status_count.
 * The struct: host arrays to fill (any may be NULL) and, on return, the device arrays of all of them and the replicates' own:
 * one pooled block of the context's, valid until its next sbgpu_abundance_bootstrap_device or sbgpu_quantify_* call.  The
 * replicates' matrices take n_rep * n_iso * (8 + 4) bytes (+ n_rep * n_iso * 8 with keep_theta_rep): SBGPU_ENOMEM when they do
 * not fit.  SBGPU_EINVAL: n_rep < 1, ranks outside 0 <= rank_lo <= rank_hi < n_rep, a NULL `out`.  SBGPU_ESHAPE: n_rep > 1024.
 * Returns synchronised on `stream` (NULL: the context's own).  Nothing depends on how the replicates are scheduled.        */
typedef struct {
   double *theta_mean, *theta_var, *fpkm_mean, *fpkm_var, *fpkm_lo, *fpkm_hi,
          *tpm_mean, *tpm_var, *tpm_lo, *tpm_hi;        /* in: host [n_iso], or NULL                                  */
   int32_t *keep_count;                                 /* in: host [n_iso], or NULL: replicates with keep != 0       */
   int32_t *status_count;                               /* in: host [n_loci][4], or NULL                              */
   double *total_fpkm_rep;                              /* in: host [n_rep], or NULL: the total TPM divided by, all ranks */
   double *fpkm_rep;                                    /* in: host [n_rep][n_iso], or NULL: every replicate's FPKM       */
   int32_t *keep_rep;                                   /* in: host [n_rep][n_iso], or NULL: every replicate's keep       */
   double *theta_rep;                                   /* in: host [n_rep][n_iso], or NULL (filled with keep_theta_rep)  */
   const double *d_theta_mean, *d_theta_var, *d_fpkm_mean, *d_fpkm_var, *d_fpkm_lo, *d_fpkm_hi,
                *d_tpm_mean, *d_tpm_var, *d_tpm_lo, *d_tpm_hi; /* out: device [n_iso]                                 */
   const int32_t *d_keep_count, *d_status_count;        /* out: device [n_iso], [n_loci][4]                           */
   const double *d_total_fpkm_rep;                      /* out: device [n_rep]                                        */
   const double *d_fpkm_rep;                            /* out: device [n_rep][n_iso]                                 */
   const int32_t *d_keep_rep;                           /* out: device [n_rep][n_iso]                                 */
   const double *d_theta_rep;                           /* out: device [n_rep][n_iso], or NULL unless keep_theta_rep  */
   int64_t n_iso, n_loci;                               /* out */
   int32_t n_rep, reserved;                             /* out */
} sbgpu_abundance_bootstrap_t;
int sbgpu_abundance_bootstrap_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const sbgpu_bootstrap_params_t *params,
                                     int32_t rank_lo, int32_t rank_hi, int32_t keep_theta_rep, sbgpu_comm_t *comm, void *stream,
                                     sbgpu_abundance_bootstrap_t *out);

/* ---- abundances per locus, and the bootstrap of Frac and of the loci's FPKM / TPM ------------------------------
 * A locus is what Strawberry calls a gene (gene_id, gene_frag_count).  The rule (csrc/bootstrap_rules.h: boot_locus_sum,
 * boot_locus_tpm; the host form and boot_locus_sum_kernel call the same functions, compiled with -ffp-contract=off).  For one
 * abundance vector -- fpkm[n_iso], keep[n_iso], total_fpkm -- and locus l with the isoforms iso_off[l] .. iso_off[l+1]-1:
 *    locus_fpkm[l]  starts at 0.0 and adds fpkm[j] over the isoforms with keep[j] != 0, in isoform order: the isoforms the
 *                   epilogue's own kept-FPKM sum takes, so that over all loci locus_fpkm adds up to the total TPM divides by
 *                   (not to its bits: the order differs);
 *    locus_kept[l]  the number of those isoforms (int32);
 *    locus_tpm[l]   = locus_kept[l] ? 1e6 * locus_fpkm[l] / total_fpkm : 0.0, the expression of sbgpu_tpm_device;
 *    a locus without isoforms gives 0.0, 0, 0.0.
 * Any output may be NULL.  SBGPU_EINVAL: n_loci < 0, NULL iso_off, offsets that decrease or start below 0, NULL fpkm / keep with
 * isoforms present.  Host form: host arrays, no GPU needed.  Device form: device arrays -- the d_* arrays of
 * sbgpu_quantify_resident's result as they stand, d_iso_off the caller's upload of the annotation's iso_off, d_total_fpkm one
 * double on the device (needed for d_locus_tpm only) --, not checked beyond NULL; one launch, asynchronous on `stream`.        */
int sbgpu_locus_abundance_host(int64_t n_loci, const int64_t *iso_off, const double *fpkm, const int32_t *keep, double total_fpkm,
                               double *locus_fpkm, double *locus_tpm, int32_t *locus_kept);
int sbgpu_locus_abundance_device(sbgpu_ctx_t *ctx, int64_t n_loci, const int64_t *d_iso_off, const double *d_fpkm, const int32_t *d_keep,
                                 const double *d_total_fpkm, double *d_locus_fpkm, double *d_locus_tpm, int32_t *d_locus_kept, void *stream);
/* sbgpu_abundance_bootstrap_device, and beside it the replicates' Frac and the loci's abundances.  Preconditions, argument
 * checks, the n_rep <= 1024 cap, the replicates, the ONE all-reduce of the n_rep totals, schedule independence and "returns
 * synchronised" are that call's; what it fills in `out` (may be NULL here) is bit for bit what that call fills for the same
 * arguments.  A NULL `locus_out`: SBGPU_EINVAL.  It also keeps, per replicate k:
 *    frac_rep[k][j]        the Frac abundance_kernel wrote for replicate k: the bits of sbgpu_abundance_device's d_frac on that
 *                          replicate's theta and status under the retained parameters (an INIT_EMPTY locus: 0.0; an "NA"
 *                          isoform: 0.0; a locus whose FPKM are all zero: what the kernel gives, NaN);
 *    locus_fpkm_rep[k][l], locus_kept_rep[k][l]   the rule above on row k of fpkm_rep / keep_rep (one more small kernel behind the
 *                          replicate's epilogue).
 * After the totals' all-reduce the statistics of sbgpu_replicate_stats_device run at rank_lo / rank_hi over the columns of
 *    frac_*        x_k = frac_rep[k][j], whatever keep says (a NaN sorts last);
 *    locus_fpkm_*  x_k = locus_fpkm_rep[k][l];
 *    locus_tpm_*   x_k = locus_kept_rep[k][l] ? 1e6 * locus_fpkm_rep[k][l] / total[k] : 0.0 (made while staging: no locus-TPM matrix
 *                  is written), and locus_kept_count[l] = the number of k with locus_kept_rep[k][l] != 0.
 * A locus lives on one rank: no collective beyond the totals'.  The struct: host arrays to fill (any may be NULL) and, on return,
 * the device arrays of all of them, in the same pooled block as `out`'s (valid until the context's next bootstrap or
 * sbgpu_quantify_* call).  On top of sbgpu_abundance_bootstrap_device's footprint the block takes n_rep * (8 n_iso + 12 n_loci)
 * bytes for the three matrices (and 32 n_iso + 68 n_loci for the statistics); it is allocated before the first kernel:
 * SBGPU_ENOMEM when it does not fit.                                                                                         */
typedef struct {
   double *frac_mean, *frac_var, *frac_lo, *frac_hi;                         /* in: host [n_iso], or NULL  */
   double *locus_fpkm_mean, *locus_fpkm_var, *locus_fpkm_lo, *locus_fpkm_hi; /* in: host [n_loci], or NULL */
   double *locus_tpm_mean, *locus_tpm_var, *locus_tpm_lo, *locus_tpm_hi;     /* in: host [n_loci], or NULL */
   int32_t *locus_kept_count;                           /* in: host [n_loci], or NULL: replicates with a kept isoform      */
   double *frac_rep;                                    /* in: host [n_rep][n_iso], or NULL: every replicate's Frac          */
   double *locus_fpkm_rep;                              /* in: host [n_rep][n_loci], or NULL                               */
   int32_t *locus_kept_rep;                             /* in: host [n_rep][n_loci], or NULL                               */
   const double *d_frac_mean, *d_frac_var, *d_frac_lo, *d_frac_hi;                         /* out: device [n_iso]  */
   const double *d_locus_fpkm_mean, *d_locus_fpkm_var, *d_locus_fpkm_lo, *d_locus_fpkm_hi; /* out: device [n_loci] */
   const double *d_locus_tpm_mean, *d_locus_tpm_var, *d_locus_tpm_lo, *d_locus_tpm_hi;     /* out: device [n_loci] */
   const int32_t *d_locus_kept_count;                   /* out: device [n_loci]                                            */
   const double *d_frac_rep;                            /* out: device [n_rep][n_iso]                                      */
   const double *d_locus_fpkm_rep;                      /* out: device [n_rep][n_loci]                                     */
   const int32_t *d_locus_kept_rep;                     /* out: device [n_rep][n_loci]                                     */
   int64_t n_iso, n_loci;                               /* out */
   int32_t n_rep, reserved;                             /* out */
} sbgpu_locus_bootstrap_t;
int sbgpu_locus_bootstrap_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const sbgpu_bootstrap_params_t *params,
                                 int32_t rank_lo, int32_t rank_hi, int32_t keep_theta_rep, sbgpu_comm_t *comm, void *stream,
                                 sbgpu_abundance_bootstrap_t *out, sbgpu_locus_bootstrap_t *locus_out);

/* ---- per-bin sequence statistics ---------------------------------------
 * What the reference's "bias" option (-b genome.fa) adds to the `-f` table and nothing else
 * (src/bias.cpp holds no code): for every exon bin, over the bases of its segments concatenated
 * (ExonBin::bin_dnaseq, include/isoform.h:173-182; FaSeqGetter::fetchSeq, src/fasta.cpp:195-200),
 *   gc[b]       Kmer<string>::GCRatio            include/kmer.h:67-76    (C c G g count; exact)
 *   entropy[b]  Kmer<string>::Entropy(seq, 6)    include/kmer.h:46-65    (natural log; bytes other
 *               than ACGTacgt code as A, :106-124; fp64, ~1e-15 relative to the reference)
 *   flags[b]    bit 0..3 = Kmer<string>::HighGCStrech(seq, 20, 0.8), (20, 0.9), (40, 0.8), (40, 0.9)
 *               include/kmer.h:78-88, in the order of src/alignments.cpp:1626-1629         (exact)
 * genome[0] is base `genome_start` (1-based, the coordinates of the segments) of the chromosome,
 * genome_len bytes as they stand in the FASTA (either case, N, ...).  Bin b = segments
 * seg_off[b] .. seg_off[b+1]-1, closed coordinates, in the bin's own (sorted) order.
 * The reference aborts on bins of 40 bases or fewer (live asserts, kmer.h:20,82); here a window
 * that does not fit gives flag 0, fewer than 6 bases give entropy 0, an empty bin gives gc NaN.
 *
 * Device form: all pointers are device pointers; *d_error (caller zeroes it) gets a non-zero
 * value if a segment lies outside the genome window (that bin's outputs are then 0).
 * genome_len must be below 2^32 (SBGPU_ESHAPE otherwise).  The first call on a device uploads two
 * small tables (synchronous); after that the call is asynchronous on `stream`.              */
int sbgpu_binseq_device(sbgpu_ctx_t *ctx, const uint8_t *d_genome, int64_t genome_start, int64_t genome_len,
                        int64_t n_bins, const int64_t *d_seg_off, const uint32_t *d_seg_left,
                        const uint32_t *d_seg_right, double *d_gc, double *d_entropy, uint8_t *d_flags,
                        int32_t *d_error, void *stream);

/* Host-buffer form: validates (SBGPU_EINVAL for a segment outside the window), uploads, runs,
 * downloads, synchronises.                                                                   */
int sbgpu_binseq_host(sbgpu_ctx_t *ctx, const uint8_t *genome, int64_t genome_start, int64_t genome_len,
                      int64_t n_bins, const int64_t *seg_off, const uint32_t *seg_left,
                      const uint32_t *seg_right, double *gc_out, double *entropy_out, uint8_t *flags_out);

/* ---- output formatting, host only -------------------------------
 * The digits Strawberry prints for FPKM / Frac / TPM: std::to_string(double) (= "%f",
 * src/estimate.cpp:335,344 and src/alignments.cpp:1827) copied into a char[12] by
 * Contig::print2gtf (src/contig.cpp:678-700), i.e. the first 11 characters.           */
int sbgpu_format_value(double v, char out[12]);

/* One transcript block exactly as Contig::print2gtf writes it (src/contig.cpp:636-721):
 * the `transcript` line then one `exon` line per exon; source "Strawberry", score 1000,
 * attributes without a space after ';' and ` exon_id "k";` appended on exon lines.
 * keep: 2 ("NA") prints NA for FPKM and Frac (src/estimate.cpp:321,339).  Writes at most
 * cap-1 bytes + NUL into buf and returns the length needed (snprintf convention).       */
int sbgpu_format_gtf_transcript(char *buf, int cap, const char *chrom, char strand, const char *gene_id,
                                const char *transcript_id, const char *ref_gene_id,
                                const char *ref_gene_name, int n_exons, const int32_t *exon_left,
                                const int32_t *exon_right, double fpkm, double frac, double tpm,
                                int32_t keep);

/* One row of the `-f` context table exactly as Sample::printContext writes it
 * (src/alignments.cpp:1549-1639, columns 1-10; the six sequence columns exist only with
 * BIAS_CORRECTION and a genome FASTA: sbgpu_format_context_row_seq below): tab-separated
 *   sample, sample_frag_count (total mapped reads), gene_id, gene_frag_count, transcripts (comma
 *   list), FPKMs (std::to_string each), conditional_probabilities (the bin's weight per isoform,
 *   to_string_with_precision(.,12) = "%.12g", include/common.h:366-372; 0 for an isoform the bin's
 *   last fragment is not compatible with), class_probabilities (Frac, std::to_string),
 *   path_symbol ("[l-r]" per segment of the bin), path_count (unique hits in the bin), newline.
 * Rows of a locus come in std::map order of the bins' coordinate sets (:1552-1563).  snprintf
 * convention like sbgpu_format_gtf_transcript.                                                */
int sbgpu_format_context_row(char *buf, int cap, const char *sample, int32_t sample_frag_count,
                             const char *gene_id, uint32_t gene_frag_count, int n_iso,
                             const char *const *transcript_ids, const double *fpkm,
                             const double *cond_prob, const double *frac, int n_seg,
                             const uint32_t *seg_left, const uint32_t *seg_right, uint32_t path_count);

/* The same row of a run with `-b genome.fa`: six more columns (src/alignments.cpp:1622-1636) --
 * path_gc_content and path_hexmer_entropy (std::to_string, six decimals) and the four stretch flags
 * (std::to_string(bool): 0 / 1), from sbgpu_binseq_*'s outputs for the bin.                   */
int sbgpu_format_context_row_seq(char *buf, int cap, const char *sample, int32_t sample_frag_count,
                                 const char *gene_id, uint32_t gene_frag_count, int n_iso,
                                 const char *const *transcript_ids, const double *fpkm,
                                 const double *cond_prob, const double *frac, int n_seg,
                                 const uint32_t *seg_left, const uint32_t *seg_right, uint32_t path_count,
                                 double gc, double entropy, uint32_t flags);

/* ---- transcript-body coverage profile: posterior-weighted bases by 5' -> 3' position ---------------------------
 * Where along an isoform its fragments lie, at a fixed number of positional bins: the gene-body curve of a sample, and per
 * isoform how even its coverage is.  The rule (csrc/body_rules.h, shared by both forms, compiled under -ffp-contract=off).  Who is
 * assigned, its candidates J(h), the posterior p(j|h) and the weight w(h,j) = (double)m_h * p(j|h) ARE the isoform-resolved
 * coverage's above, under the same theta, keep, status, weights and masses.
 *   - BINS    P = n_pos, 1 <= P <= SBGPU_BODY_MAX_POS; anything else: SBGPU_EINVAL.
 *   - LENGTH  L_j = the sum of R_e - L_e + 1 over isoform j's exons (exon_off, closed coordinates), an int64.
 *   - COORDINATE  a base at genomic g inside exon e of j has t = pre_e + (g - L_e), pre_e the total length of j's exons before e.
 *   - BIN OF A BASE  q(t) = floor(t * P / L_j) in exact 64-bit integer arithmetic: bin q holds t in [ceil(q L_j / P),
 *     ceil((q + 1) L_j / P) - 1]; where L_j < P its width may be 0.
 *   - ORIENTATION  iso_strand[j] (a HOST array; NULL: all 0) is coded as the clusters' strands: 0 unknown, 1 '+', 2 '-'; a value
 *     above 2: SBGPU_EINVAL.  The reported bin is q for 0 and 1, P - 1 - q for 2: orientation changes the index only.
 *   - TERM    n(h,j,p), an integer: the bases of hit h's S_MATCH features that lie inside j's exons and fall in reported bin p
 *     (S_GAP and S_INTRON features add nothing).  body_bases[j * P + p] = sum over the assigned hits h with j in J(h) of
 *     w(h,j) * (double)n(h,j,p): one product per (hit, candidate, bin) with n != 0.
 *   - PER ISOFORM, functions of the isoform's finished bins' bits, taken in ascending p:
 *       body_total[j]   the ascending sum;
 *       body_center[j]  (sum_p bases_p * (double)(2p + 1)) / ((double)(2P) * total): 0.5 for a uniform profile, above 0.5 towards
 *                       the 3' end of a stranded isoform;
 *       body_cv[j]      over the bins of non-zero width wd_p: depth_p = bases_p / (double)wd_p, m their mean,
 *                       sqrt(mean of (depth_p - m)^2) / m;
 *       body_center[j] = body_cv[j] = -1.0 exactly where body_total[j] is exactly 0.0.
 *   - PER SAMPLE  the length class of j is c = (L_j >= 1000) + (L_j >= 2000) + (L_j >= 4000).  For every isoform with total > 0:
 *     class_profile[c * P + p] += bases_p / total and class_n[c] += 1 -- the sample's gene-body curve, every expressed isoform
 *     with the same weight.  The host form adds in ascending j.
 * An isoform that is not kept, and a locus whose status is SBGPU_EM_INIT_EMPTY, hold zeros and -1.0 and are in no class.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device form only -- the device arrays of all six (the
 * context's memory: valid until its next quantify or body-profile call).                                                    */
#define SBGPU_BODY_MAX_POS 100
typedef struct {
   double *body_bases;     /* in: [n_iso * n_pos]                                           */
   double *body_total;     /* in: [n_iso]                                                   */
   double *body_center;    /* in: [n_iso]                                                   */
   double *body_cv;        /* in: [n_iso]                                                   */
   double *class_profile;  /* in: [4 * n_pos]                                               */
   int64_t *class_n;       /* in: [4]                                                       */
   const double *d_body_bases, *d_body_total, *d_body_center, *d_body_cv, *d_class_profile; /* out: device form only */
   const int64_t *d_class_n;                                                                 /* out: device form only */
} sbgpu_body_profile_t;
/* Host form, the plain statement of the rule: hits in index order, inside a hit the candidates in ascending j.  Every argument
 * up to hit_mass is sbgpu_isoform_coverage_host's, with its NULL conventions and its refusals.                             */
int sbgpu_body_profile_host(const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                            const uint32_t *compat, int32_t compat_words, const double *F, const double *theta,
                            const int32_t *keep, const int32_t *status, const float *hit_mass, const uint8_t *iso_strand,
                            int32_t n_pos, sbgpu_body_profile_t *out);
/* Device form (csrc/body_device.h): valid exactly where sbgpu_isoform_coverage_device is -- same handles, same refusals, the
 * same annot / d_hits / d_theta / d_hit_mass -- and nothing more is retained by a resident call.  The assignment's column pass,
 * one pass over the hits, one over the isoforms.  The sums are added in another order than the host form's: equal within the
 * rounding of a sum of non-negative terms, exactly where every term is an integer; body_total, body_center and body_cv are the
 * rule's functions of the device's own body_bases; class_n is exact.  The results live in a scratch slot of their own: table,
 * assignment, coverage, fit, information, support and profile may be asked for in any order, repeatedly.  Only the arrays the
 * caller gave pointers for cross PCIe.  Synchronises on `stream` (NULL: the context's own).  Loci of more than 4096 isoforms or
 * more than 5632 bins: SBGPU_ESHAPE.                                                                                       */
int sbgpu_body_profile_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                              const double *d_theta, const float *d_hit_mass, const uint8_t *iso_strand, int32_t n_pos, void *stream,
                              sbgpu_body_profile_t *out);
/* The device form's thresholds (csrc/body_device.h; reasoned from LDS sizes, not tuned): out[0] hits of one work item; a locus
 * keeps its tables and sums in LDS where it has at most [1] annotated exons, at most [2] isoforms and niso * n_pos is at most
 * [3]; its sums are kept in [5] copies where it has at most [4] isoforms and niso * n_pos * [5] is at most [3]; [6] the most
 * bins and [7] the most isoforms of one locus.                                                                              */
int sbgpu_body_profile_limits(int64_t out[8]);

/* ---- splicing events: exon and junction inclusion (PSI) with intervals --------------------------------------
 * For one annotated exon or one annotated intron: which share of the transcripts that run across it include it.  The event
 * table is a function of the annotation alone (built once, on the host); the PSI of every event is a function of the table and
 * of one abundance row.  The rule (csrc/splice_rules.h, shared by both forms, compiled under -ffp-contract=off).  For locus l
 * with the isoforms j0 = iso_off[l] .. j1 - 1, isoform j's exons e = exon_off[j] .. exon_off[j+1] - 1, closed [L_e, R_e], ascending:
 *   - EVENTS  an exon event is a distinct pair [L_e, R_e] among the locus' exons (kind 0); an intron event is a distinct pair
 *     [R_e + 1, L_{e+1} - 1] between consecutive exons of one isoform (kind 1: the interval junction_mass of the isoform-resolved
 *     coverage stands for), made only where R_e + 1 <= L_{e+1} - 1 (abutting exons make none).  A locus' events are ordered by
 *     (left, right, kind) ascending; an exon and an intron of the same coordinates are two events.  Loci in annotation order:
 *     event_off[n_loci + 1], event_locus[n_events].
 *   - INCLUSION LIST  of event u, incl_off[u] .. incl_off[u+1] - 1: the isoforms that own that exon or intron, in ascending j;
 *     incl_iso (int32): the isoform's index inside its locus; incl_exon (int64): the global index of that exon, or of the exon
 *     upstream of the intron -- the index into exon_bases / junction_mass.  Two identical isoforms are two entries.
 *   - SPAN  isoform j spans event [a, b] iff it has an exon and L_first(j) <= a and b <= R_last(j): iso_left[j] / iso_right[j]
 *     hold the two (0xFFFFFFFF / 0 for an isoform without exons, which spans nothing); n_span[u] (int32) counts the spanning
 *     isoforms whatever keep says.  No span list is kept; inclusion implies span.  n_incl == n_span: constitutive within its span.
 *   - FLAGS  (uint8) exon events: FIRST / LAST: the exon is the first / last exon of an including isoform; INTERNAL: it is
 *     neither in some including isoform; SKIPPED: some isoform of the locus has an intron [a', b'] with a' <= L and R <= b'.
 *     Intron events: RETAINED: some isoform of the locus has an exon [L', R'] with L' <= a and b <= R'.
 *   - PSI of one abundance row x[n_iso] with keep[n_iso] (NULL: every isoform enters): inc starts at 0.0 and adds x[j] over the
 *     inclusion list in list order where keep[j] != 0; tot starts at 0.0 and adds x[j] over j = j0 .. j1 - 1 ascending where j
 *     spans the event and keep[j] != 0; psi = tot > 0.0 ? inc / tot : NaN.  defined_count[u]: the rows with tot > 0.0.  The order
 *     of the additions is the rule: for non-negative x, tot adds a superset of inc's terms in the same order and rounded addition
 *     is monotone, so inc <= tot and 0 <= psi <= 1 exactly.  A NaN among the added x gives NaN.
 *   - SUPPORT of an event from per-exon arrays: support[u] starts at 0.0 and adds v[incl_exon[i]] in list order, v = exon_bases
 *     for an exon event and junction_mass for an intron event (the posterior mass of the spliced hits over that junction, summed
 *     over the isoforms that share it); an event whose array is NULL holds 0.0.
 * The struct is used as a host table and, with device pointers, as the device table (the convention of sbgpu_hits_t).          */
#define SBGPU_SPLICE_FIRST 1
#define SBGPU_SPLICE_LAST 2
#define SBGPU_SPLICE_INTERNAL 4
#define SBGPU_SPLICE_SKIPPED 8
#define SBGPU_SPLICE_RETAINED 16
typedef struct {
   int64_t n_loci, n_iso, n_exons, n_events, n_incl;
   int64_t *event_off;      /* [n_loci + 1]                                     */
   int32_t *event_locus;    /* [n_events]                                       */
   uint8_t *event_kind;     /* [n_events]: 0 exon, 1 intron                     */
   uint32_t *event_left;    /* [n_events]                                       */
   uint32_t *event_right;   /* [n_events]                                       */
   uint8_t *event_flags;    /* [n_events]: SBGPU_SPLICE_* bits                  */
   int32_t *n_span;         /* [n_events]                                       */
   int64_t *incl_off;       /* [n_events + 1]                                   */
   int32_t *incl_iso;       /* [n_incl]                                         */
   int64_t *incl_exon;      /* [n_incl]                                         */
   int64_t *iso_off;        /* [n_loci + 1]: the annotation's                   */
   uint32_t *iso_left;      /* [n_iso]                                          */
   uint32_t *iso_right;     /* [n_iso]                                          */
} sbgpu_splice_events_t;
/* Host only, no GPU needed (csrc/splice_host.cpp).  shapes: out[0] = n_events, out[1] = n_incl.  build: `out` names arrays the
 * caller allocated at those sizes and carries the two numbers in n_events / n_incl (anything else: SBGPU_EINVAL); the call sets
 * n_loci, n_iso and n_exons and fills every array.  SBGPU_EINVAL, with the reason in sbgpu_last_error: a NULL argument or array,
 * offsets that descend, an isoform whose exons are not ascending and disjoint, more than 2^31 - 1 isoforms in one locus.       */
int sbgpu_splice_events_shapes_host(const sbgpu_annotation_t *annot, int64_t out[2]);
int sbgpu_splice_events_build_host(const sbgpu_annotation_t *annot, sbgpu_splice_events_t *out);
/* Host forms, the plain statement of the rule.  x and keep: [n_rows][n_iso], replicate-major (keep may be NULL); psi:
 * [n_rows][n_events]; defined_count [n_events] may be NULL.  support [n_events]; exon_bases / junction_mass [n_exons], either
 * may be NULL.  Both check the table: SBGPU_EINVAL for offsets that descend or do not close, an event_locus outside the loci, an
 * incl_iso outside its locus, an incl_exon outside the exons.                                                                 */
int sbgpu_splice_psi_host(const sbgpu_splice_events_t *events, int64_t n_rows, const double *x, const int32_t *keep, double *psi,
                          int32_t *defined_count);
int sbgpu_splice_support_host(const sbgpu_splice_events_t *events, const double *exon_bases, const double *junction_mass, double *support);
/* Device forms (csrc/splice_device.h): d_events is a host struct of device pointers; every array is a device array taken as it
 * stands -- not checked beyond NULL and the sizes --, one launch, asynchronous on `stream`.  No handle, no retention, no scratch
 * slot, no collective (a locus lives on one rank).  d_x / d_keep: the d_fpkm / d_keep of sbgpu_quantify_resident's result with
 * n_rows = 1, or the d_fpkm_rep / d_keep_rep of sbgpu_abundance_bootstrap_device with n_rows = n_rep; the intervals are
 * sbgpu_replicate_stats_device over d_psi[n_rep][n_events].  The results are the host forms' bits.  SBGPU_ESHAPE: more than
 * 2^31 - 1 events or rows.                                                                                                   */
int sbgpu_splice_psi_device(sbgpu_ctx_t *ctx, const sbgpu_splice_events_t *d_events, int64_t n_rows, const double *d_x, const int32_t *d_keep,
                            double *d_psi, int32_t *d_defined_count, void *stream);
int sbgpu_splice_support_device(sbgpu_ctx_t *ctx, const sbgpu_splice_events_t *d_events, const double *d_exon_bases,
                                const double *d_junction_mass, double *d_support, void *stream);
/* out[0]: an event of a locus of at most this many isoforms keeps its inclusion and span sets as two 64-bit masks (wider loci
 * test the extents and walk the list, row by row); out[1]: events of one workgroup, one thread each (the grid is not capped). */
int sbgpu_splice_limits(int64_t out[2]);

/* ---- variational Bayes: a Dirichlet prior on the isoform shares --------------------------------------------
 * A second, independent solver over the batch layout of sbgpu_em_run_device, for the loci whose likelihood is flat in some
 * direction: a symmetric Dirichlet(alpha) prior on the isoform shares and the mean-field posterior q(share) = Dirichlet(alpha +
 * c).  With alpha < 1 it empties the isoforms the data do not need; it gives a posterior spread per isoform and an evidence bound
 * (ELBO) per locus.  It calls none of the EM kernels and is NOT a parity path: the reference has no such solve.  The rule
 * (csrc/vb_rules.h, shared by both forms, compiled under -ffp-contract=off, every fused operation written as fma).  One locus:
 * bins i with counts n_i (int32 >= 0), isoforms j = 0..K-1, raw weights F[i][j], and alpha, change_limit, max_iter.
 *    1. A bin is LIVE if some F[i][j] > SBGPU_EM_ROW_EPS (asg_row_live, the row drop of EmSolver::init).  No live bin: status
 *       SBGPU_EM_INIT_EMPTY, every output 0, iters 0.
 *    2. s_j = the sum of F[i][j] over the live bins, ascending; column j is ACTIVE if s_j > 0; K_a = the active columns;
 *       A[i][j] = F[i][j] / s_j for an active column, 0 otherwise -- from the first iteration on.
 *    3. N = the integer sum of n_i over the live bins.  Start: c_j = (double)N / K_a for an active j, 0 otherwise.  A locus with
 *       N = 0 has observed nothing: status SBGPU_EM_OK, iters 1 (its one iteration does not move c), count, share, share_sd and
 *       elbo 0.
 *    4. psi(x), x > 0: s = 0; while x < 10: s -= 1/x, x += 1; y = 1/(x x); psi = log x - 0.5/x - y (1/12 - y (1/120 - y (1/252 -
 *       y (1/240 - y (1/132 - y (691/32760 - y/12)))))) + s.
 *    5. One iteration: p_j = psi(alpha + c_j) for the active j; m = max p_j; w_j = exp(p_j - m), 0 for an inactive j;
 *       d_i = sum_j A[i][j] w_j in ascending j, a chain of fma; r_i = (double)n_i / d_i where n_i > 0, 0 where n_i = 0; a live bin
 *       with n_i > 0 and d_i == 0: status SBGPU_EM_DENOM_ZERO, c stays, the solve ends; c'_j = w_j * (sum_i A[i][j] r_i over the
 *       live bins in ascending i, a chain of fma); sqrt(sum_j (c'_j - c_j)^2) < change_limit: stop with SBGPU_EM_OK and return c,
 *       not c'; otherwise c = c'.  After max_iter iterations: SBGPU_EM_MAXITER.  iters = the iterations started.
 *    6. At the returned c: a0 = K_a alpha + (double)N; lw_j = psi(alpha + c_j) - psi(a0); elbo = sum over the live bins with n_i > 0
 *       of n_i log(sum_j A[i][j] exp(lw_j)) - [lgamma(a0) - sum_j lgamma(alpha + c_j) - lgamma(K_a alpha) + K_a lgamma(alpha) +
 *       sum_j c_j lw_j], the sums over the active j; -inf where a counted bin has mixture mass 0.
 *    7. count[j] = c_j, in fragments: comparable with theta, and a valid d_theta for sbgpu_abundance_device;
 *       share[j] = (alpha + c_j) / a0 for an active j, 0 otherwise; share_sd[j] = sqrt(a_j (a0 - a_j) / (a0^2 (a0 + 1))) with
 *       a_j = alpha + c_j: the Dirichlet's standard deviation; n_active[l] = K_a; n_frag[l] = N.
 * params NULL: alpha = 0.01, change_limit = SBGPU_EM_THETA_CHANGE_LIMIT, max_iter = SBGPU_EM_MAX_ITER.  SBGPU_EINVAL: alpha
 * outside [1e-6, 1e3], change_limit <= 0, max_iter < 1.  A locus of more than 512 isoforms or more than 5632 bins: SBGPU_ESHAPE.
 * The struct: host arrays to fill (any may be NULL) and, on return -- device forms only -- the device arrays of all of them: the
 * context's memory, in a scratch slot of their own, valid until the context's next sbgpu_quantify_* or variational call.     */
typedef struct {
   double alpha;         /* the Dirichlet's concentration per isoform */
   double change_limit;  /* the step norm below which a locus stops, in fragments */
   int32_t max_iter;
   int32_t reserved;
} sbgpu_vb_params_t;
typedef struct {
   double *count, *share, *share_sd;                /* in: [n_iso]   */
   int32_t *status, *iters;                         /* in: [n_loci]  */
   double *elbo;                                    /* in: [n_loci]  */
   int32_t *n_active;                               /* in: [n_loci]  */
   int64_t *n_frag;                                 /* in: [n_loci]  */
   const double *d_count, *d_share, *d_share_sd;    /* out: device forms only */
   const int32_t *d_status, *d_iters;
   const double *d_elbo;
   const int32_t *d_n_active;
   const int64_t *d_n_frag;
} sbgpu_em_vb_t;
/* Host form (csrc/vb_host.cpp; no GPU needed), the plain statement of the rule: every sum in ascending order.  SBGPU_EINVAL,
 * with the reason in sbgpu_last_error: a negative count, malformed offsets (not beginning at 0, not ascending, f_off not rows x
 * isoforms), NULL count / F where there are bins / weights, a parameter out of range.                                     */
int sbgpu_em_vb_host(const sbgpu_batch_t *batch, const sbgpu_vb_params_t *params, sbgpu_em_vb_t *out);
/* Device form (csrc/vb_device.h) for any batch sbgpu_em_run_device solves: the plan, d_count and d_F as given to it.  A locus'
 * normalised weights are made once and stay in LDS while it iterates: a wave per locus of at most out[0] weights of
 * sbgpu_em_vb_limits, a workgroup per larger locus, which keeps A in LDS up to out[1] and reads a normalised copy in the call's
 * scratch beyond.  d_i and c'_j are the host form's operation for operation; log, exp and lgamma are the device library's, and
 * the step norm and the ELBO's sums are added along a fixed tree (csrc/vb_device.h states it): status, n_active, n_frag and
 * which outputs are zero are the host form's exactly, the rest within the rounding of those differences, the same bits from
 * call to call and wherever a locus stands in the batch.  Only the arrays the caller gave pointers for cross PCIe.  Synchronises
 * on `stream` (NULL: the context's own).                                                                                  */
int sbgpu_em_vb_device(sbgpu_ctx_t *ctx, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                       const sbgpu_vb_params_t *params, void *stream, sbgpu_em_vb_t *out);
/* The same right after a resident call or an sbgpu_front_stream_end made with sbgpu_bootstrap_keep on, from that record (the
 * call's plan, counts and weights): nothing more is retained, and the call's seven results are the same bits with and without
 * a variational call behind it.  A handle made without retention, or a stale one: SBGPU_EINVAL, as for sbgpu_model_fit_device.
 * It may be asked for in any order with the fit, the support and the other retained-result stages.                         */
int sbgpu_model_vb_device(sbgpu_ctx_t *ctx, const sbgpu_bins_t *bins, const sbgpu_vb_params_t *params, void *stream, sbgpu_em_vb_t *out);
/* The device form's thresholds (csrc/vb_device.h), for callers and tests that want a locus on either side of each: out[0]
 * weights of a locus (bins x isoforms) up to which a wave serves it, a workgroup beyond; [1] doubles of LDS the workgroup form
 * has for one locus: bins x isoforms + bins + 2 isoforms at most that: A stays in LDS, beyond: in the call's scratch; [2] loci
 * per workgroup in the wave form; [3] workgroups per CU a launch's grid is capped at; [4] threads of a workgroup; [5] of a wave
 * (the reduction tree's two levels); [6] the most bins and [7] the most isoforms of one locus.                              */
int sbgpu_em_vb_limits(int64_t out[8]);

/* ---- the annotation: a GTF file's bytes -> sbgpu_annotation_t, sbgpu_clusters_t, the isoforms' lengths and strands, the names
 * (sbgpu_gtf_*; csrc/gtf_rules.h codes the line's rule once for both forms, csrc/gtf_host.cpp the rest).
 * GffReader::readAll over GffLine::GffLine (src/gff.cpp) and Sample::addRef2Cluster (src/alignments.cpp:1025-1079), restated.
 *
 * LINES.  The input is the file's bytes.  A line ends at '\n' (the last line need not have one); one '\r' in front of the '\n'
 * is not part of the line.  Every line gets a status:
 *   SKIP           shorter than 10 bytes, or its first byte that is not isspace is '#' (gff.cpp:460-462)
 *   FIELDS         fewer than eight tabs (the line is cut at its first eight)
 *   OTHER          column 3, ASCII-lower-cased, contains "utr", or does not contain "exon" (:162-166).  Only exon lines build
 *                  transcripts from a GTF in the reference too: a `transcript` line carries no Parent, so its gene is not found
 *                  and the mRNA case breaks (:491-495)
 *   COORD          column 4 or 5 -- each the field's leading run of ASCII digits -- has no digit or a value outside
 *                  1 .. 2^31 - 1.  end < start: the two are swapped (:134-138)
 *   NO_TRANSCRIPT  no transcript_id, or an empty one.  GFF3 (ID= / Parent=) is not read: such lines end here
 *   NO_GENE        no gene_id, or an empty one (gene_name may be empty)
 *   OK             an exon line of a transcript
 * Column 6 (the score) is NOT read.  This is the one place where a well-formed file reads differently: the reference's `return`
 * at :147 stands outside its `if`, so a line with a numeric score never becomes a feature there.  Column 7: '+' is strand 1,
 * '-' is 2, anything else 0 (the clusters' strand codes).  Column 9: gene_id, transcript_id and gene_name are found as
 * GffLine::extractAttr finds them (:13-69): a key matches outside double quotes, at the column's start or behind a blank or
 * ';', its bytes compared ASCII-case-insensitively, and must be followed by a blank or the column's end; the value skips blanks
 * and one optional opening quote and runs to the closing quote, ';' or the end when it was quoted, to ';' or the end when not.
 * Each key is looked up in the column's ORIGINAL text: the reference deletes an attribute it found before the next lookup
 * (:71-77).  A NUL is a byte like any other.  A chromosome, gene or transcript name, or a gene_name, of more than 255 bytes in
 * a line that would be OK makes both forms return SBGPU_EUNSUPPORTED.
 *
 * TRANSCRIPTS.  A transcript is the set of OK lines with one key: chromosome name lower-cased, strand, transcript_id bytes.
 * Its lines may stand anywhere in the file (the reference keeps one tree per chromosome and one list per strand, and looks a
 * transcript up by walking that list: :405-448).  Its gene_id and gene_name are those of its first line in the file.  Its exons
 * are sorted by (left, right); exons that are equal, overlap or touch (next.left <= prev.right + 1) are merged into their union,
 * and the merges are counted.
 *
 * CHROMOSOMES.  With a table of names (n_ref, ref_name: a BAM header's) a chromosome's id is its index in the table, names
 * compared lower-cased as the reference lower-cases both sides (gff.cpp:118, read.cpp:964,980); a transcript on a chromosome the
 * table lacks is dropped and counted.  Without a table, ids go by first appearance in the file (alignments.cpp:846-849).
 *
 * ORDER.  Transcripts are sorted by (1) chromosome id, (2) the exon coordinates l1, r1, l2, r2, .. compared lexicographically, a
 * proper prefix first -- Contig::operator< over GenomicFeature::operator< (contig.cpp:186-193,342-347) in exon coordinates --,
 * (3) first line in the file (the reference's std::sort leaves these ties open).
 *
 * LOCI.  A locus is all kept transcripts of one (chromosome id, gene_id bytes as written), its isoforms in the sorted order; loci
 * are ordered by their first isoform's place in it, so they ascend by (chromosome, left) as sbgpu_assign_reads_* need.  The
 * reference takes consecutive runs of one gene id, then looks 100 transcripts ahead and adds same-gene transcripts without
 * consuming them, so they come back as a second cluster: where a gene's transcripts are consecutive in the sorted order the two
 * rules agree; where they interleave, this rule gives one locus per gene and no duplicate.  Per locus: chromosome, left = min and
 * right = max over its isoforms, strand = its first isoform's.  Per isoform: iso_len, the sum of its exon lengths, and
 * iso_strand.  The disjoint segments are sbgpu_segments_host's.  A file without one OK line: SBGPU_OK and zero loci.           */
#define SBGPU_GTF_OK 0
#define SBGPU_GTF_SKIP 1
#define SBGPU_GTF_FIELDS 2
#define SBGPU_GTF_OTHER 3
#define SBGPU_GTF_COORD 4
#define SBGPU_GTF_NO_TRANSCRIPT 5
#define SBGPU_GTF_NO_GENE 6
typedef struct sbgpu_gtf sbgpu_gtf_t;
typedef struct {
   int64_t n_ref;               /* 0: no table */
   const char *const *ref_name; /* [n_ref] NUL-terminated */
   int32_t hash_bits;           /* for tests: 0 means 64, otherwise the device form's key hashes are cut to that many bits */
} sbgpu_gtf_opts_t;
/* The names: CSR offsets and bytes (not NUL-separated) of gene_id and gene_name per locus, transcript_id per isoform, and the
 * chromosome name per id -- the table's where one was given, else as first written in the file.                              */
typedef struct {
   const int64_t *gene_id_off, *gene_name_off; /* [n_loci + 1] */
   const char *gene_id, *gene_name;
   const int64_t *transcript_id_off;           /* [n_iso + 1]  */
   const char *transcript_id;
   const int64_t *chrom_off;                   /* [chromosomes + 1] */
   const char *chrom;
} sbgpu_gtf_names_t;
/* Host form (csrc/gtf_host.cpp; no GPU needed): a hash map whose keys are compared byte by byte; takes a line of any length.
 * opts may be NULL (no table).  All three forms return a handle that holds HOST arrays.                                      */
int sbgpu_gtf_read_host(const uint8_t *bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, sbgpu_gtf_t **out);
/* Device form (csrc/gtf_device.h): the bytes are in HBM, at any alignment.  The line index, the parse -- one lane per line -- and
 * the grouping of lines into transcripts (two stable radix sorts, by (left, right), then by a 64-bit FNV-1a hash of the
 * transcript's key, and a pass per transcript that merges its exons and compares every member's key bytes with its first
 * member's) run on the device; the statuses, a row per transcript, the merged exons and the names come back, and the order, the
 * loci, the arrays and the segments are built on the host in the host form's code.  Every array, name, status and info word is
 * the host form's.  SBGPU_EUNSUPPORTED, and the caller uses the host form: a line longer than limits[2] of sbgpu_gtf_limits (its '\r' and '\n' not counted);
 * 2^31 - 2 lines or more; two transcripts whose keys share a hash -- the text then has the word "collision".  Synchronises on
 * `stream` (NULL: the context's own) on every way out.                                                                       */
int sbgpu_gtf_read_device(sbgpu_ctx_t *ctx, const uint8_t *d_bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, void *stream, sbgpu_gtf_t **out);
/* The device form on host bytes: uploaded through the context's pool first.                                                   */
int sbgpu_gtf_read_upload(sbgpu_ctx_t *ctx, const uint8_t *bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, void *stream, sbgpu_gtf_t **out);
/* What the handle holds; every pointer is owned by it and lives until sbgpu_gtf_destroy.  Any out argument may be NULL.
 * iso_len, iso_strand: [n_iso].                                                                                               */
int sbgpu_gtf_annotation(const sbgpu_gtf_t *g, sbgpu_annotation_t *annot, sbgpu_clusters_t *clusters, const int32_t **iso_len, const uint8_t **iso_strand);
int sbgpu_gtf_names(const sbgpu_gtf_t *g, sbgpu_gtf_names_t *names);
/* info[0] lines; [1 .. 7] lines per status SBGPU_GTF_OK .. SBGPU_GTF_NO_GENE; [8] transcripts kept; [9] loci; [10] exons; [11]
 * segments; [12] chromosomes; [13] exons the merges took away, over every transcript of the file; [14] transcripts dropped for
 * their chromosome; [15] 0.                                                                                                   */
int sbgpu_gtf_info(const sbgpu_gtf_t *g, int64_t info[16]);
/* a copy of the lines' statuses: status[info[0]] */
int sbgpu_gtf_line_status(const sbgpu_gtf_t *g, uint8_t *status);
/* The device form's thresholds (csrc/gtf_schedule.h), for tests that want an input on either side of each: limits[0] lines per
 * tile of the parse (a wave's pass); [1] bytes of a tile up to which it is staged in LDS, beyond: walked in global memory; [2]
 * the longest line the device form takes; [3] entries per round of the scan over the tiles' totals; [4] bytes per tile of the
 * line index; [5] workgroups a kernel's grid is capped at; [6] the longest name; [7] lines from which the device form refuses. */
int sbgpu_gtf_limits(int64_t limits[8]);
void sbgpu_gtf_destroy(sbgpu_gtf_t *g);

/* ---- the genome: a FASTA file's bytes -> the contigs' names, their sequences packed back to back, and a .fai index
 * (sbgpu_fasta_*; csrc/fasta_rules.h holds what both forms share, csrc/fasta_host.cpp the host form and the handle).
 * The reference cannot build an index (FaIndex::buildIndex is a stub, src/fasta.cpp:86-89; without a .fai it shells out to
 * `samtools faidx`, :286-291) and reads a sequence line by line through one (FaSeqGetter::loadSeq, :132-193).
 *
 * LINES.  The input is the file's bytes.  A line ends at '\n' (the last line need not have one); one '\r' directly in front of the
 * '\n' is the terminator's, not the line's.  A NUL is a byte like any other.
 *
 * HEADERS.  A header is a line whose first byte is '>'; it opens a contig.  The contig's name is the bytes behind '>' up to the
 * first byte for which C's isspace holds, or up to the line's end; the rest of the line is not kept.  Empty lines in front of the
 * first header are skipped; a non-empty one makes both forms return SBGPU_EINVAL, and the text carries that line's byte offset.
 * No header at all, or zero bytes: SBGPU_OK and zero contigs.
 *
 * SEQUENCE.  A contig's sequence is every byte of every line between its header and the next header (or the end), as it stands:
 * no case folding and no filtering (the bin statistics code the bytes, and loadSeq copies them raw too).  All contigs' sequences
 * are packed back to back in file order; seq_off[n_contigs + 1] bounds them, length[c] = seq_off[c + 1] - seq_off[c].
 *
 * INDEX.  Per contig the five .fai columns: the name, the length, `offset` -- the byte behind the header line's terminator --,
 * `line_bases` -- the length of the first line behind the header -- and `line_width` -- line_bases plus the terminator bytes that
 * line actually has (0, 1 or 2).
 *
 * FLAGS.  One byte per contig:
 *   EMPTY      no base; line_bases = line_width = 0 (the reference exits on these, fasta.cpp:140-143)
 *   RAGGED     the lines behind the header are NOT, in this order: k >= 0 lines of exactly line_bases bytes, each with the first
 *              line's terminator; at most one line of 1 .. line_bases bytes with any terminator or none; any number of empty
 *              lines.  (A first line of length 0 followed by bases is RAGGED.)  The sequence is still packed and exact; only the
 *              index arithmetic does not hold
 *   DUPLICATE  an earlier contig has this name under the lookup's comparison
 *   NONAME     the name is empty
 * For a contig that is neither EMPTY nor RAGGED and every p in 1 .. length,
 *   file[offset + ((p - 1) / line_bases) * line_width + (p - 1) % line_bases] == seq[seq_off[c] + p - 1]
 * which is loadSeq's arithmetic (fasta.cpp:144-146).
 *
 * LOOKUP.  sbgpu_fasta_find compares names ASCII-lower-cased on both sides, as the GTF reader compares chromosome names with a BAM
 * header's; the first match in file order wins.  This deviates from the reference, which compares the FASTA's name as written
 * with the GTF's lower-cased one: `Chr1` in a FASTA is never found there.                                                     */
#define SBGPU_FASTA_EMPTY 1
#define SBGPU_FASTA_RAGGED 2
#define SBGPU_FASTA_DUPLICATE 4
#define SBGPU_FASTA_NONAME 8
typedef struct sbgpu_fasta sbgpu_fasta_t;
/* Host form (csrc/fasta_host.cpp; no GPU needed): line by line; takes lines and headers of any length.  The packed sequence is in
 * host memory.                                                                                                               */
int sbgpu_fasta_read_host(const uint8_t *bytes, int64_t n_bytes, sbgpu_fasta_t **out);
/* Device form (csrc/fasta_device.h): the bytes are in HBM, at any alignment.  A stream compaction over tiles of limits[0] bytes:
 * the headers are counted, scanned and walked (a wave per header line); the bases are counted per tile, scanned in 64 bits and
 * packed by popcount prefix.  No array has an entry per line, and an unwrapped contig is read like a wrapped one.  The packed
 * sequence stays in HBM, owned by the handle; the index columns, flags, seq_off and names come back to the host, and every
 * array, flag, name and info word is the host form's.  SBGPU_EUNSUPPORTED, and the caller uses the host form: a header line
 * longer than limits[3] of sbgpu_fasta_limits ('>' counted, its '\r' and '\n' not) -- the text then has the words "header line"
 * --, or more than limits[4] contigs.  Synchronises on `stream` (NULL: the context's own) on every way out.                    */
int sbgpu_fasta_read_device(sbgpu_ctx_t *ctx, const uint8_t *d_bytes, int64_t n_bytes, void *stream, sbgpu_fasta_t **out);
/* The device form on host bytes: uploaded through the context's pool first.                                                   */
int sbgpu_fasta_read_upload(sbgpu_ctx_t *ctx, const uint8_t *bytes, int64_t n_bytes, void *stream, sbgpu_fasta_t **out);
/* info[0] bytes; [1] lines; [2] contigs; [3] bases; [4 .. 7] contigs with EMPTY, RAGGED, DUPLICATE, NONAME; [8] the longest
 * contig's length and [9] its index (the first of equals; -1 without a contig); [10] 1 where the sequence is on a device and
 * [11] that device (-1: the host); [12 .. 15] 0.                                                                              */
int sbgpu_fasta_info(const sbgpu_fasta_t *g, int64_t info[16]);
/* What the handle holds; every pointer is owned by it and lives until sbgpu_fasta_destroy.  Any out argument may be NULL.
 * seq_off: [contigs + 1]; offset, line_bases, line_width, flags: [contigs].  The names: CSR offsets [contigs + 1] plus bytes
 * (not NUL-separated).  The sequence: seq_off[contigs] bytes, in HBM where *on_device comes back 1.                          */
int sbgpu_fasta_index(const sbgpu_fasta_t *g, const int64_t **seq_off, const int64_t **offset, const int64_t **line_bases, const int64_t **line_width,
                      const uint8_t **flags);
int sbgpu_fasta_names(const sbgpu_fasta_t *g, const int64_t **name_off, const char **names);
int sbgpu_fasta_sequence(const sbgpu_fasta_t *g, const uint8_t **seq, int32_t *on_device);
/* *contig: the first contig of that name (name_len bytes, compared lower-cased), -1 where there is none                        */
int sbgpu_fasta_find(const sbgpu_fasta_t *g, const char *name, int64_t name_len, int64_t *contig);
/* The .fai text: one line per contig in file order, name\tlength\toffset\tline_bases\tline_width\n.  EMPTY contigs are left out
 * (the reference's loader rejects such a line, fasta.cpp:72); a RAGGED or NONAME contig makes it return SBGPU_EUNSUPPORTED, the
 * text names the contig.  *need: the text's bytes (no NUL is written); buf may be NULL to ask for it, cap < *need: SBGPU_EINVAL. */
int sbgpu_fasta_fai(const sbgpu_fasta_t *g, char *buf, int64_t cap, int64_t *need);
/* `len` bases of contig `contig` from base `start` (1-based) to host memory; from a handle on a device: a synchronous copy.  A
 * window outside the contig: SBGPU_EINVAL.                                                                                    */
int sbgpu_fasta_fetch(const sbgpu_fasta_t *g, int64_t contig, int64_t start, int64_t len, uint8_t *out);
/* The device form's thresholds (csrc/fasta_schedule.h), for tests that want an input on either side of each: limits[0] bytes per
 * tile; [1] entries per round of the scans; [2] workgroups a kernel's grid is capped at (a tile each per round); [3] the longest
 * header line the device form takes; [4] the most contigs; [5 .. 7] 0.                                                        */
int sbgpu_fasta_limits(int64_t limits[8]);
void sbgpu_fasta_destroy(sbgpu_fasta_t *g);
/* `-b genome.fa` over every chromosome of an annotation: the per-bin sequence statistics above with the genome taken from a
 * handle.  Bins run_off[r] .. run_off[r + 1] - 1 lie on contig run_contig[r] (host arrays; run_off ascends from 0 to n_bins;
 * the runs' contigs may come in any order); one launch of the same kernel per run, with the contig's packed sequence as the
 * genome (genome_start 1, genome_len its length); the per-bin arrays are advanced by run_off[r], the coordinate arrays are
 * indexed absolutely.  The handle must hold its sequence on the context's device, and a run must not lie on an EMPTY contig, else
 * SBGPU_EINVAL; a contig of 2^32 bases or more in a run: SBGPU_ESHAPE.  Asynchronous on `stream` like the entry above.         */
int sbgpu_binseq_fasta_device(sbgpu_ctx_t *ctx, const sbgpu_fasta_t *g, int64_t n_runs, const int64_t *run_off, const int32_t *run_contig, int64_t n_bins,
                              const int64_t *d_seg_off, const uint32_t *d_seg_left, const uint32_t *d_seg_right, double *d_gc, double *d_entropy,
                              uint8_t *d_flags, int32_t *d_error, void *stream);
/* The same with host arrays and either kind of handle: validates as the host-buffer form above does, and per run calls it on the
 * contig's window from the first base the run's segments touch to the last.                                                   */
int sbgpu_binseq_fasta_host(sbgpu_ctx_t *ctx, const sbgpu_fasta_t *g, int64_t n_runs, const int64_t *run_off, const int32_t *run_contig, int64_t n_bins,
                            const int64_t *seg_off, const uint32_t *seg_left, const uint32_t *seg_right, double *gc_out, double *entropy_out,
                            uint8_t *flags_out);

#ifdef __cplusplus
}
#endif
#endif /* SBGPU_H_ */
