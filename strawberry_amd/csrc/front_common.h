// strawberry_amd/csrc/front_common.h -- what the launchers of the front end share (bamdecode_api.hip, matepair_api.hip,
// collapse_api.hip, front_stream_api.hip), beside stage_common.h: the synchronise-then-fail macro, a device block that goes
// back to the pool with its scope, owning pointers for the stages' handles, and the tests' hooks read in one place.  What the
// launchers decide -- layouts, sort keys, grids, the stream's window arithmetic -- is front_schedule.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>

#include "api_internal.h"
#include "front_schedule.h"

namespace sb {

// A HIP call of a launcher whose stream is `s`: on failure the stream is synchronised first (kernels may still read what the
// scope is about to give back), then the call fails with "<expr>: <HIP's text>" -- SBGPU_ENOMEM where the device is full.
#define SB_FRONT_TRY(expr)                          \
   do {                                             \
      hipError_t e_ = (expr);                       \
      if (e_ != hipSuccess) {                       \
         (void)hipStreamSynchronize(s);             \
         return sb::api_fail_hip(e_, #expr);        \
      }                                             \
   } while (0)
#define SB_FRONT_RC(expr)              \
   do {                                \
      const int rc_ = (expr);          \
      if (rc_ != SBGPU_OK) return rc_; \
   } while (0)

// A block from the pool (dev_take) that goes back when its scope ends, on every way out: the stream that used it is
// synchronised first.
struct DevBlock {
   char *p = nullptr;
   size_t cap = 0;
   hipStream_t s;
   explicit DevBlock(hipStream_t stream) : s(stream) {}
   DevBlock(const DevBlock &) = delete;
   DevBlock &operator=(const DevBlock &) = delete;
   ~DevBlock() { give(); }
   hipError_t take(size_t bytes) { return dev_take(bytes, &p, &cap); }
   void give()
   {
      if (!p) return;
      (void)hipStreamSynchronize(s);
      dev_give(p, cap);
      p = nullptr, cap = 0;
   }
   template <class T>
   T *at(size_t off) const
   {
      return (T *)(p + off);
   }
};

// The scans' transforms: 32-bit counts summed as 64-bit words, flag bytes as 32-bit words (one type each: rocPRIM's kernels are
// instantiated per transform)
struct I32AsI64 {
   __device__ int64_t operator()(int32_t v) const { return (int64_t)v; }
};
struct U8AsI32 {
   __device__ int32_t operator()(uint8_t v) const { return (int32_t)v; }
};

// A stage's handle, destroyed with its scope unless it is released to the caller
template <auto Destroy>
struct HandleDeleter {
   template <class T>
   void operator()(T *h) const
   {
      Destroy(h);
   }
};
using BamReadsHandle = std::unique_ptr<sbgpu_bamreads_t, HandleDeleter<sbgpu_bamreads_destroy>>;
using MatePairsHandle = std::unique_ptr<sbgpu_matepairs_t, HandleDeleter<sbgpu_matepairs_destroy>>;
using UniqDevHandle = std::unique_ptr<sbgpu_uniq_dev_t, HandleDeleter<sbgpu_uniq_dev_destroy>>;

// The tests' hooks that force a route the default inputs do not take (nonzero: on), read once per call
struct FrontHooks {
   bool pair_force_sort;    // SBGPU_PAIR_FORCE_SORT: every pairing call takes the sorted form
   bool collapse_two_sorts; // SBGPU_COLLAPSE_TWO_SORTS: the collapse orders its pairs with two sorts
   bool collapse_force_seq; // SBGPU_COLLAPSE_FORCE_SEQ: every cluster takes the running sums in the reference's order
   bool bam_two_pass;       // SBGPU_BAM_TWO_PASS: the decode skips its one-pass kernel
};
static inline FrontHooks front_hooks_from_env()
{
   auto on = [](const char *name) {
      const char *v = std::getenv(name);
      return v && std::atoi(v) != 0;
   };
   return {on("SBGPU_PAIR_FORCE_SORT"), on("SBGPU_COLLAPSE_TWO_SORTS"), on("SBGPU_COLLAPSE_FORCE_SEQ"), on("SBGPU_BAM_TWO_PASS")};
}

} // namespace sb
