// strawberry_amd/csrc/bgzf_api.hip -- the device forms of the BGZF layer: sbgpu_bgzf_inflate_device (bgzf_device.h: one
// member per wave) and sbgpu_bam_index_device (the record offsets of an inflated stream by validated speculation).
#include <algorithm>
#include <string>

#include "api_internal.h"
#define SB_BGZF_KERNELS
#include "bgzf_device.h"

using sb::api_fail;

namespace {
thread_local int64_t t_index_info[8] = {};
constexpr int kIndexMaxFixRounds = 8; // rounds of re-walks before the sequential walker takes the rest
} // namespace

namespace sb {
int64_t bam_index_device_impl(sbgpu_ctx_t *c, const uint8_t *d_bytes, int64_t n_bytes, int64_t first_record, const int64_t *d_guess, int64_t n_guess,
                              int64_t guess_add, const std::function<int64_t *(int64_t)> &alloc, int64_t *tail_start, void *stream)
{
   for (int64_t &v : t_index_info) v = 0;
   if (!c || n_bytes < 0 || first_record < 0 || first_record > n_bytes || n_guess < 0 || (n_bytes && !d_bytes) || (n_guess && !d_guess))
      return api_fail(SBGPU_EINVAL, "sbgpu_bam_index_device: bad argument");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   char *w = nullptr;
   size_t w_cap = 0;
   auto bail = [&](int code, const std::string &msg) {
      (void)hipStreamSynchronize(s);
      sb::dev_give(w, w_cap);
      return (int64_t)api_fail(code, "sbgpu_bam_index_device: " + msg);
   };
#define SB_TRY(expr)                                                                                                                   \
   do {                                                                                                                                \
      hipError_t e_ = (expr);                                                                                                          \
      if (e_ != hipSuccess) return bail(e_ == hipErrorOutOfMemory ? SBGPU_ENOMEM : SBGPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
   } while (0)
   SB_TRY(hipSetDevice(sb::ctx_device(c)));
   sb::bgzf::IndexArgs a = {};
   a.bytes = d_bytes, a.n_bytes = n_bytes, a.first_record = first_record;
   a.guess = d_guess, a.guess_add = guess_add;
   a.n_seg = d_guess ? n_guess + 1 : (n_bytes - first_record) / sb::bgzf::kIndexStride + 1;
   const int64_t n_blk = (a.n_seg + 255) / 256;
   if (n_blk > 0x7fffffff) return bail(SBGPU_EUNSUPPORTED, "more than 2^39 guesses");
   const size_t seg_bytes = ((size_t)a.n_seg * 8 + 255) & ~(size_t)255, sum_bytes = ((size_t)(n_blk + 1) * 8 + 255) & ~(size_t)255;
   SB_TRY(sb::dev_take(5 * seg_bytes + sum_bytes + 256, &w, &w_cap));
   a.count = (int64_t *)w, a.entry_a = (int64_t *)(w + seg_bytes), a.exit_a = (int64_t *)(w + 2 * seg_bytes);
   a.entry_b = (int64_t *)(w + 3 * seg_bytes), a.exit_b = (int64_t *)(w + 4 * seg_bytes);
   int64_t *block_sum = (int64_t *)(w + 5 * seg_bytes);
   a.word = (unsigned long long *)(w + 5 * seg_bytes + sum_bytes);
   const dim3 grid((unsigned)n_blk), block(256);
   hipLaunchKernelGGL(sb::bgzf::index_walk_kernel, grid, block, 0, s, a);
   SB_TRY(hipGetLastError());
   int64_t *entry_in = a.entry_a, *entry_out = a.entry_b, *exit_in = a.exit_a, *exit_out = a.exit_b;
   int64_t rounds = 1, walked_again = 0, sequential_from = -1;
   for (int r = 0;; ++r) {
      const unsigned long long init[2] = {0ull, ~0ull};
      unsigned long long got[2] = {};
      SB_TRY(hipMemcpyAsync(a.word, init, 16, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(sb::bgzf::index_fix_kernel, grid, block, 0, s, a, (const int64_t *)entry_in, (const int64_t *)exit_in, entry_out, exit_out);
      SB_TRY(hipGetLastError());
      SB_TRY(hipMemcpyAsync(got, a.word, 16, hipMemcpyDeviceToHost, s));
      SB_TRY(hipStreamSynchronize(s));
      std::swap(entry_in, entry_out), std::swap(exit_in, exit_out); // (in: the state as it stands)
      if (!got[0]) break; // nothing to repair: every entry is its predecessor's exit, segment 0's is known, so all are true
      ++rounds, walked_again += (int64_t)got[0];
      if (r + 1 == kIndexMaxFixRounds) {
         // the segments before the first one walked again in this round were consistent, so they are true, and so is that one now
         // (walked from a true exit); one lane takes the rest
         sequential_from = (int64_t)got[1] + 1;
         if (sequential_from < a.n_seg) {
            hipLaunchKernelGGL(sb::bgzf::index_sequential_kernel, dim3(1), dim3(64), 0, s, a, sequential_from, entry_in, exit_in);
            SB_TRY(hipGetLastError());
         }
         break;
      }
   }
   hipLaunchKernelGGL(sb::bgzf::index_block_sums_kernel, grid, block, 0, s, a, block_sum);
   SB_TRY(hipGetLastError());
   hipLaunchKernelGGL(sb::bgzf::index_scan_sums_kernel, dim3(1), block, 0, s, block_sum, n_blk);
   SB_TRY(hipGetLastError());
   int64_t n = 0, last_exit = 0;
   SB_TRY(hipMemcpyAsync(&n, block_sum + n_blk, 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipMemcpyAsync(&last_exit, exit_in + (a.n_seg - 1), 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
   t_index_info[0] = rounds, t_index_info[1] = a.n_seg, t_index_info[2] = walked_again, t_index_info[3] = sequential_from;
   if (last_exit == sb::bgzf::kIndexFault) return bail(SBGPU_ESHAPE, "a record of the stream has a negative size");
   if (last_exit != n_bytes) { // (the chain leaves the last segment at the stream's end, or it is cut there)
      if (!tail_start) return bail(SBGPU_ESHAPE, "the stream ends inside record " + std::to_string(n));
      *tail_start = last_exit - sb::bgzf::kIndexPartial;
   } else if (tail_start) *tail_start = n_bytes;
   int64_t *d_rec_off = alloc(n);
   if (!d_rec_off) return bail(SBGPU_ESHAPE, "more than `cap` records");
   hipLaunchKernelGGL(sb::bgzf::index_fill_kernel, grid, block, 0, s, a, (const int64_t *)entry_in, (const int64_t *)block_sum, d_rec_off);
   SB_TRY(hipGetLastError());
   SB_TRY(hipStreamSynchronize(s));
   sb::dev_give(w, w_cap);
   return n;
#undef SB_TRY
}
} // namespace sb

extern "C" {

int sbgpu_bgzf_inflate_device(sbgpu_ctx_t *c, const uint8_t *d_file, int64_t n_bytes, const int64_t *d_blk_off, const int64_t *d_out_off,
                              int64_t n_blocks, uint8_t *d_out, void *stream, uint8_t *d_status, int64_t *n_failed)
{
   if (!c || n_bytes < 0 || n_blocks < 0 || n_blocks > 0x7fffffff) return api_fail(SBGPU_EINVAL, "sbgpu_bgzf_inflate_device: bad argument");
   if (n_failed) *n_failed = 0;
   if (!n_blocks) return SBGPU_OK;
   if (!d_file || !d_blk_off || !d_out_off || !d_out || !d_status) return api_fail(SBGPU_EINVAL, "sbgpu_bgzf_inflate_device: null argument");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   auto hip_fail = [](hipError_t e, const char *what) {
      return api_fail(e == hipErrorOutOfMemory ? SBGPU_ENOMEM : SBGPU_EHIP, std::string("sbgpu_bgzf_inflate_device: ") + what + ": " + hipGetErrorString(e));
   };
   if (hipError_t e = hipSetDevice(sb::ctx_device(c))) return hip_fail(e, "hipSetDevice");
   char *w = nullptr;
   size_t w_cap = 0;
   if (n_failed) {
      if (hipError_t e = sb::dev_take(256, &w, &w_cap)) return hip_fail(e, "dev_take");
      if (hipError_t e = hipMemsetAsync(w, 0, 8, s)) {
         sb::dev_give(w, w_cap);
         return hip_fail(e, "hipMemsetAsync");
      }
   }
   hipLaunchKernelGGL(sb::bgzf::bgzf_inflate_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, d_file, n_bytes, d_blk_off, d_out_off, n_blocks, d_out,
                      d_status, (unsigned long long *)w);
   hipError_t e = hipGetLastError();
   if (e == hipSuccess && n_failed) {
      unsigned long long failed = 0;
      e = hipMemcpyAsync(&failed, w, 8, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      *n_failed = (int64_t)failed;
   }
   if (w) {
      if (e != hipSuccess) (void)hipStreamSynchronize(s);
      sb::dev_give(w, w_cap);
   }
   if (e != hipSuccess) return hip_fail(e, "bgzf_inflate_kernel");
   return SBGPU_OK;
}

int64_t sbgpu_bam_index_device(sbgpu_ctx_t *c, const uint8_t *d_bytes, int64_t n_bytes, int64_t first_record, const int64_t *d_guess,
                               int64_t n_guess, int64_t *d_rec_off, int64_t cap, void *stream)
{
   if (!d_rec_off || cap < 0) {
      api_fail(SBGPU_EINVAL, "sbgpu_bam_index_device: bad argument");
      return -1;
   }
   const int64_t n = sb::bam_index_device_impl(c, d_bytes, n_bytes, first_record, d_guess, n_guess, 0,
                                               [&](int64_t n_records) { return n_records <= cap ? d_rec_off : nullptr; }, nullptr, stream);
   return n < 0 ? -1 : n;
}

void sbgpu_bam_index_device_info(int64_t *info)
{
   if (info)
      for (int k = 0; k < 8; ++k) info[k] = t_index_info[k];
}

} // extern "C"
