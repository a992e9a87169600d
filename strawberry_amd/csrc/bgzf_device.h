// strawberry_amd/csrc/bgzf_device.h -- BGZF members -> their inflated bytes: a complete RFC 1951 decoder, once.
//
// `sb::bgzf::inflate_member<P>` is the decoder: block headers, the code-length code, the two Huffman codes, the symbol
// loop and every test that ends a member in a status.  It is written against a policy P that supplies the four things
// that differ between one host thread and one wave of 64 lanes:
//   refill()            the next 32 bits of the member's payload into the bit holder (zeros behind the payload's end)
//   build(...)          the decode tables of one Huffman code from its code lengths
//   literal / match / stored   the writes to the member's output
// so the host form (bgzf_host.cpp, HostMember) and the device form (below, WaveMember) take the same decisions on the same
// bits: a member is OK in one iff it is OK in the other, and iff zlib's raw inflate reaches the end of the stream with
// exactly ISIZE bytes (the tests in tests/test_bgzf.py and tests/test_bgzf_gpu.py hold both to zlib).
//
// The device form, one member per wave (a workgroup IS one wave: every __syncthreads below is a wave-local ordering point):
//   * the decoder's state -- bit holder, positions, the symbol just decoded -- is wave-uniform: every value that comes out
//     of LDS passes through readfirstlane, so it lives in SGPRs and the symbol loop branches on the scalar unit;
//   * the payload is staged through LDS 1 KiB at a time, one aligned 16-byte load per lane (byte loads with bounds tests
//     for the granules that straddle the payload's ends; nothing is loaded from outside the payload); staging, flushing and
//     the table build are functions of their own, so that the symbol loop stays small;
//   * the tables of a deflate block are built by the wave: code lengths -> counts by ballot, canonical codes by rank among
//     the lanes of equal length, a direct-lookup table of 10 bits (literal/length) and 8 bits (distance) filled by the
//     lanes, the symbols sorted by code for the bit-by-bit path that longer codes take;
//   * literals are written by lane 0, matches and stored blocks are copied by the whole wave -- into a ring of the member's
//     latest 4 KiB of output in LDS, which goes to global memory 1 KiB at a time in aligned 16-byte stores.  A match whose
//     source the ring still holds never leaves LDS; an older source is read back from global memory (L1 / L2), behind a
//     workgroup fence that finds the flush's stores long complete.  No 32 KiB window per member: 8.5 KiB of LDS per wave
//     (tables 3.5, staging 1, ring 4), 18 waves per CU; DESIGN 3.15 has the ring sizes that were measured.
// Every write is tested against [0, ISIZE) of the member and every read against its payload first.
#pragma once

#include <stdint.h>

#include "../../include/sbgpu.h"

#if defined(__HIP__)
#define SB_BGZF_HD __host__ __device__ __forceinline__
#else
#define SB_BGZF_HD inline
#endif

namespace sb {
namespace bgzf {

constexpr int FAST_L = 10, FAST_D = 8;   // bits of the direct-lookup tables (an entry: symbol << 4 | code length; 0: take the slow path)
constexpr int N_LIT = 288, N_DIST = 32;  // symbols of the fixed codes (a dynamic block has at most 286 / 30)
constexpr int HEADER = 18, FOOTER = 8, MAX_MEMBER = 65536, MAX_ISIZE = 65536;

// The decode tables of one member (host: members of a struct; device: LDS)
struct Tables {
   uint16_t lit_fast[1 << FAST_L], dist_fast[1 << FAST_D];
   uint16_t lit_sym[N_LIT], dist_sym[N_DIST]; // symbols in canonical order (by length, then by value)
   uint16_t lit_cnt[16], dist_cnt[16];        // codes per length
   uint8_t lens[N_LIT + N_DIST];              // the code lengths a dynamic block's header spells out
};

// What every policy shares: the bit holder over a payload of `in_len` bytes and the output cursor.
// `avail` counts the payload's bits not yet consumed; it goes negative when the decoder has taken bits from behind the
// payload's end (they read as zeros), which every caller tests before it acts on what it decoded.
template <class P>
struct MemberBase {
   uint64_t hold = 0;
   int32_t nbits = 0, avail = 0, in_len = 0;
   uint32_t wpos = 0; // the next 32-bit word of the payload stream refill() takes
   int32_t pos = 0, isize = 0;
   bool have_fixed = false;

   SB_BGZF_HD P &self() { return *static_cast<P *>(this); }
   SB_BGZF_HD void fill()
   {
      if (nbits <= 32) self().refill();
   }
   SB_BGZF_HD void drop(int n) { hold >>= n, nbits -= n, avail -= n; }
   SB_BGZF_HD uint32_t bits(int n) // n <= 16
   {
      fill();
      const uint32_t v = (uint32_t)hold & ((1u << n) - 1u);
      drop(n);
      return v;
   }
   // the reader at byte `at` of the payload stream (policy's coordinates: P::lead() is where the payload starts)
   SB_BGZF_HD void seek(uint32_t at)
   {
      wpos = at >> 2, hold = 0, nbits = 0;
      self().refill();
      const int k = (int)(at & 3u) * 8;
      hold >>= k, nbits -= k;
   }
   // one symbol of a code: the direct table, or bit by bit over the canonical order (-1: no such code)
   SB_BGZF_HD int decode(const uint16_t *fast, int fast_bits, const uint16_t *cnt, const uint16_t *sym)
   {
      fill();
      const uint32_t e = P::ld16(fast + ((uint32_t)hold & ((1u << fast_bits) - 1u)));
      if (e) {
         drop((int)(e & 15u));
         return (int)(e >> 4);
      }
      int code = 0, first = 0, index = 0;
      uint32_t h = (uint32_t)hold;
      for (int l = 1; l <= 15; ++l) {
         code |= (int)(h & 1u), h >>= 1;
         const int c = (int)P::ld16(cnt + l);
         if (code - c < first) {
            drop(l);
            return (int)P::ld16(sym + index + (code - first));
         }
         index += c, first += c, first <<= 1, code <<= 1;
      }
      drop(15);
      return -1;
   }
};

// The decoder.  Returns an SBGPU_BGZF_* status; on SBGPU_BGZF_OK exactly p.isize bytes were written.
template <class P>
SB_BGZF_HD int inflate_member(P &p, Tables *t)
{
   // (the base / extra-bits tables of RFC 1951 3.2.5 as arithmetic: a table read is a trip to global memory on the device --
   // there is no scalar byte load --, two of them on the chain of every match)
   static constexpr uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
   p.seek(p.lead());
   for (;;) {
      const uint32_t hdr = p.bits(3);
      if (p.avail < 0) return SBGPU_BGZF_EINPUT;
      const uint32_t btype = hdr >> 1;
      if (btype == 3) return SBGPU_BGZF_EBTYPE;
      if (btype == 0) {
         p.drop(p.nbits & 7); // to the byte boundary: whole words enter the holder, so nbits = -(bits consumed) mod 8
         const uint32_t len = p.bits(16), nlen = p.bits(16);
         if (p.avail < 0) return SBGPU_BGZF_EINPUT;
         if (len != (nlen ^ 0xffffu)) return SBGPU_BGZF_ESTORED;
         if ((int32_t)len * 8 > p.avail) return SBGPU_BGZF_EINPUT;
         if (p.pos + (int32_t)len > p.isize) return SBGPU_BGZF_ESIZE;
         const uint32_t at = (uint32_t)(p.in_len - (p.avail >> 3)); // byte of the payload the stored bytes begin at
         p.stored(at, len);
         p.pos += (int32_t)len, p.avail -= (int32_t)len * 8;
         p.seek(p.lead() + at + len);
      } else {
         if (btype == 1) {
            if (!p.have_fixed) {
               p.fixed_lens(t);
               p.build(t->lens, N_LIT, t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym, false);
               p.build(t->lens + N_LIT, N_DIST, t->dist_fast, FAST_D, t->dist_cnt, t->dist_sym, false);
               p.have_fixed = true;
            }
         } else {
            p.have_fixed = false;
            const int nlit = (int)p.bits(5) + 257, ndist = (int)p.bits(5) + 1, ncl = (int)p.bits(4) + 4;
            if (p.avail < 0) return SBGPU_BGZF_EINPUT;
            if (nlit > 286 || ndist > 30) return SBGPU_BGZF_ECODELEN;
            // the code-length code: 19 lengths of 3 bits in the order of RFC 1951 3.2.7, decoded through the literal tables' space
            uint32_t cl[19];
            for (int k = 0; k < 19; ++k) cl[k] = k < ncl ? p.bits(3) : 0u;
            if (p.avail < 0) return SBGPU_BGZF_EINPUT;
            p.put_cl_lens(t, cl, CL_ORDER);
            if (const int st = p.build(t->lens, 19, t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym, true)) return st;
            // (the 19 lengths sat in lens[0..19): the real ones overwrite them, after the tables are built)
            int have = 0;
            uint32_t prev = 0;
            while (have < nlit + ndist) {
               const int s = p.decode(t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym);
               if (p.avail < 0) return SBGPU_BGZF_EINPUT;
               if (s < 0) return SBGPU_BGZF_ESYMBOL;
               uint32_t val = (uint32_t)s;
               int rep = 1;
               if (s == 16) {
                  if (!have) return SBGPU_BGZF_ECODELEN; // nothing to repeat
                  val = prev, rep = 3 + (int)p.bits(2);
               } else if (s == 17) val = 0, rep = 3 + (int)p.bits(3);
               else if (s == 18) val = 0, rep = 11 + (int)p.bits(7);
               if (p.avail < 0) return SBGPU_BGZF_EINPUT;
               if (have + rep > nlit + ndist) return SBGPU_BGZF_ECODELEN;
               p.put_lens(t, have, rep, val);
               have += rep, prev = val;
            }
            if (!p.len_at(t, 256)) return SBGPU_BGZF_ECODELEN; // a block that could never end
            if (const int st = p.build_dynamic(t, nlit, ndist)) return st;
         }
         for (;;) {
            int s = p.decode(t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym);
            if (p.avail < 0) return SBGPU_BGZF_EINPUT;
            if (s < 0) return SBGPU_BGZF_ESYMBOL;
            if (s < 256) {
               if (p.pos >= p.isize) return SBGPU_BGZF_ESIZE;
               p.literal((uint8_t)s);
               ++p.pos;
               continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return SBGPU_BGZF_ESYMBOL;
            const int lext = s < 8 || s == 28 ? 0 : (s - 4) >> 2;
            const int32_t len = (s == 28 ? 258 : s < 8 ? 3 + s : 3 + ((4 + (s & 3)) << lext)) + (int32_t)p.bits(lext);
            const int d = p.decode(t->dist_fast, FAST_D, t->dist_cnt, t->dist_sym);
            if (p.avail < 0) return SBGPU_BGZF_EINPUT;
            if (d < 0 || d >= 30) return SBGPU_BGZF_ESYMBOL;
            const int dext = d < 4 ? 0 : (d - 2) >> 1;
            const int32_t dist = (d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << dext)) + (int32_t)p.bits(dext);
            if (p.avail < 0) return SBGPU_BGZF_EINPUT;
            if (dist > p.pos) return SBGPU_BGZF_EDIST;
            if (p.pos + len > p.isize) return SBGPU_BGZF_ESIZE;
            p.match(len, dist);
            p.pos += len;
         }
      }
      if (hdr & 1u) break;
   }
   return p.pos == p.isize ? SBGPU_BGZF_OK : SBGPU_BGZF_ESIZE;
}

// zlib's tests of a set of code lengths (inflate_table, inftrees.c:107-139): over-subscribed is an error, incomplete is one
// unless the set is a single code of one bit (or, for the code-length code -- `strict` --, always); a set without any code is
// accepted and decodes nothing.  left: what remains of the code space after the counts cnt[1..15].
SB_BGZF_HD int check_counts(const uint32_t *cnt, bool strict)
{
   int left = 1, max = 0;
   for (int l = 1; l <= 15; ++l) {
      left <<= 1, left -= (int)cnt[l];
      if (left < 0) return SBGPU_BGZF_ECODELEN;
      if (cnt[l]) max = l;
   }
   if (max && left > 0 && (strict || max != 1)) return SBGPU_BGZF_ECODELEN;
   return SBGPU_BGZF_OK;
}
SB_BGZF_HD uint32_t bit_reverse(uint32_t code, int len)
{
   uint32_t r = 0;
   for (int k = 0; k < len; ++k) r = (r << 1) | ((code >> k) & 1u);
   return r;
}

#if defined(SB_BGZF_KERNELS) // (bgzf_api.hip alone: the host form instantiates the decoder without them)
// ---- the device form: one member per wave ---------------------------------------------------------------------------
constexpr int STAGE_BYTES = 1024; // one aligned 16-byte granule per lane
#ifndef SB_BGZF_RING // (a power of two >= 2048; -DSB_BGZF_RING=... builds the variants DESIGN 3.15 compares)
#define SB_BGZF_RING 4096
#endif
constexpr int RING = SB_BGZF_RING; // the member's latest output, kept in LDS: a match that reaches no further back reads it there
constexpr int FLUSH = 1024;       // ... and written to the member's place in global memory a KiB at a time, 16 bytes per lane
struct WaveShared {
   Tables t;
   uint4 stage[STAGE_BYTES / 16];
   uint4 ring[RING / 16];
};

struct WaveMember : MemberBase<WaveMember> {
   const uint8_t *pay;  // the payload's first byte
   const uint8_t *base; // `pay` aligned down to 16 bytes: the origin of the stream coordinates
   uint32_t lead_;      // pay - base
   uint8_t *out;
   WaveShared *sh;
   int32_t chunk = -1;  // which 1 KiB of the stream the stage holds
   int lane;
   // The output goes through a ring in LDS: position p of the member lives at ring[(align + p) mod RING], align = the low four
   // bits of its address in global memory, so that a 16-byte granule of the ring is an aligned 16 bytes there.  [0, flushed)
   // is in global memory; at most FLUSH + 15 bytes wait in front of a write, so [pos + len - RING, pos) is always in the ring.
   uint32_t align = 0;
   int32_t flushed = 0;
   __device__ __forceinline__ uint8_t *ring() const { return (uint8_t *)sh->ring; }
   __device__ __forceinline__ void flush(bool final)
   {
      flushed = __builtin_amdgcn_readfirstlane(flush_ring(out, sh->ring, align, pos, flushed, final));
   }
   static __device__ __noinline__ int32_t flush_ring(uint8_t *out, const uint4 *ring4, uint32_t align, int32_t pos, int32_t flushed, bool final)
   {
      const int lane = (int)threadIdx.x;
      const uint8_t *ring = (const uint8_t *)ring4;
      const int32_t head = (int32_t)((16u - align) & 15u); // the bytes in front of the first aligned granule
      if (flushed < head) {
         if (pos < head && !final) return flushed;
         const int32_t e = pos < head ? pos : head;
         if (lane < e - flushed) out[flushed + lane] = ring[(align + (uint32_t)(flushed + lane)) & (RING - 1)];
         flushed = e;
      }
      while (pos - flushed >= FLUSH) {
         *(uint4 *)(out + flushed + 16 * lane) = ring4[(((align + (uint32_t)flushed) & (RING - 1)) / 16 + lane) & (RING / 16 - 1)];
         flushed += FLUSH;
      }
      if (final && pos > flushed) {
         const int32_t whole = (pos - flushed) >> 4, rest = (pos - flushed) & 15;
         if (lane < whole) *(uint4 *)(out + flushed + 16 * lane) = ring4[(((align + (uint32_t)flushed) & (RING - 1)) / 16 + lane) & (RING / 16 - 1)];
         flushed += whole * 16;
         if (lane < rest) out[flushed + lane] = ring[(align + (uint32_t)(flushed + lane)) & (RING - 1)];
         flushed = pos;
      }
      return flushed;
   }
   __device__ __forceinline__ uint32_t lead() const { return lead_; }
   static __device__ __forceinline__ uint32_t ld16(const uint16_t *p) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)*p); }

   // (out of line, like flush_ring above and build_tables below: the symbol loop calls them once per KiB or per block, and their
   // bodies inlined at every place that reads bits made the loop several times the size of the instruction cache's share)
   static __device__ __noinline__ void stage_chunk(const uint8_t *base, uint32_t lead, int32_t in_len, int32_t c, uint4 *stage)
   {
      const int lane = (int)threadIdx.x;
      __syncthreads();
      const int64_t k0 = (int64_t)c * STAGE_BYTES + lane * 16, lo = lead, hi = (int64_t)lead + in_len; // the payload is [lo, hi)
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k0 >= lo && k0 + 16 <= hi) v = *(const uint4 *)(base + k0);
      else if (k0 + 16 > lo && k0 < hi) {
         uint32_t w[4] = {0u, 0u, 0u, 0u};
         for (int j = 0; j < 16; ++j)
            if (k0 + j >= lo && k0 + j < hi) w[j >> 2] |= (uint32_t)base[k0 + j] << ((j & 3) * 8);
         v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      stage[lane] = v;
      __syncthreads();
   }
   __device__ __forceinline__ void refill()
   {
      const int32_t c = (int32_t)(wpos >> 8);
      if (c != chunk) stage_chunk(base, lead_, in_len, c, sh->stage), chunk = c;
      const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)((const uint32_t *)sh->stage)[wpos & 255u]);
      hold |= (uint64_t)w << nbits, nbits += 32, ++wpos;
   }
   __device__ __forceinline__ void literal(uint8_t b)
   {
      if (pos - flushed >= FLUSH + 16) flush(false);
      if (lane == 0) ring()[(align + (uint32_t)pos) & (RING - 1)] = b;
   }
   // byte i of the match is byte pos - dist + i; where the match overlaps itself (dist < len) that is byte i mod dist of the
   // `dist` bytes in front of pos, which earlier symbols wrote: no lane reads what this match writes.  Sources the ring still
   // holds are read there; older ones come back from global memory, where flush() put them.
   __device__ __forceinline__ void match(int32_t len, int32_t dist)
   {
      if (pos - flushed >= FLUSH + 16) flush(false);
      const int32_t ring_lo = pos + len - RING; // (what this match's own bytes overwrite lies below)
      const bool far = pos - dist < ring_lo;
      if (far) __threadfence_block(); // the flushes' stores before any lane's loads
      const float inv = 1.0f / (float)dist;
      for (int32_t i = lane; i < len; i += 64) {
         int32_t r = i;
         if (dist < len) { // i mod dist for i < 258: a float quotient is off by one at most
            r = i - (int32_t)((float)i * inv) * dist;
            r += r < 0 ? dist : 0, r -= r >= dist ? dist : 0;
         }
         const int32_t src = pos - dist + r;
         uint8_t v = ring()[(align + (uint32_t)src) & (RING - 1)];
         if (far && src < ring_lo) v = out[src];
         ring()[(align + (uint32_t)(pos + i)) & (RING - 1)] = v;
      }
   }
   // (a stored block may be longer than the ring: 256 bytes at a time, the cursor moved along for flush() and put back)
   __device__ __forceinline__ void stored(uint32_t at, uint32_t len)
   {
      const int32_t pos0 = pos;
      for (uint32_t i0 = 0; i0 < len; i0 += 256u) {
         if (pos - flushed >= FLUSH + 16) flush(false);
         const uint32_t n = len - i0 < 256u ? len - i0 : 256u;
         for (uint32_t i = (uint32_t)lane; i < n; i += 64u) ring()[(align + (uint32_t)pos + i) & (RING - 1)] = pay[at + i0 + i];
         pos += (int32_t)n;
      }
      pos = pos0;
   }
   __device__ __forceinline__ void fixed_lens(Tables *t)
   {
      for (int s = lane; s < N_LIT + N_DIST; s += 64) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < N_LIT ? 8 : 5);
      __syncthreads();
   }
   __device__ __forceinline__ void put_cl_lens(Tables *t, const uint32_t *cl, const uint8_t *order)
   {
      if (lane == 0)
         for (int k = 0; k < 19; ++k) t->lens[order[k]] = (uint8_t)cl[k];
      __syncthreads();
   }
   __device__ __forceinline__ void put_lens(Tables *t, int at, int n, uint32_t v)
   {
      if (lane < n) t->lens[at + lane] = (uint8_t)v; // n <= 138: three rounds at most
      if (lane + 64 < n) t->lens[at + lane + 64] = (uint8_t)v;
      if (lane + 128 < n) t->lens[at + lane + 128] = (uint8_t)v;
   }
   __device__ __forceinline__ uint32_t len_at(Tables *t, int s)
   {
      __syncthreads();
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)t->lens[s]);
   }
   __device__ __forceinline__ int build_dynamic(Tables *t, int nlit, int ndist)
   {
      if (const int st = build(t->lens, nlit, t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym, false)) return st;
      return build(t->lens + nlit, ndist, t->dist_fast, FAST_D, t->dist_cnt, t->dist_sym, false);
   }
   // the tables of one code from lens[0 .. n), n <= 288, by the whole wave.  A function of its own, not inlined: five copies of
   // its unrolled loops in the decoder's body cost the symbol loop its registers.
   __device__ __forceinline__ int build(const uint8_t *lens, int n, uint16_t *fast, int fast_bits, uint16_t *cnt, uint16_t *sym, bool strict)
   {
      return __builtin_amdgcn_readfirstlane(build_tables(lens, n, fast, fast_bits, cnt, sym, strict));
   }
   static __device__ __noinline__ int build_tables(const uint8_t *lens, int n, uint16_t *fast, int fast_bits, uint16_t *cnt, uint16_t *sym, bool strict)
   {
      const int lane = (int)threadIdx.x;
      __syncthreads();
      const uint64_t below = (1ull << lane) - 1ull;
      uint32_t c[16];
#pragma unroll
      for (int l = 0; l < 16; ++l) c[l] = 0;
      for (int s0 = 0; s0 < n; s0 += 64) {
         const int l = s0 + lane < n ? (int)lens[s0 + lane] : 0;
#pragma unroll
         for (int L = 1; L <= 15; ++L) c[L] += (uint32_t)__popcll(__ballot(l == L));
      }
      if (const int st = check_counts(c, strict)) return st;
      for (int k = lane; k < (1 << fast_bits); k += 64) fast[k] = 0;
      uint32_t off[16], next[16]; // where a length's symbols begin in `sym`; its first canonical code
      off[0] = 0, next[0] = 0, c[0] = 0;
#pragma unroll
      for (int L = 1; L <= 15; ++L) off[L] = off[L - 1] + c[L - 1], next[L] = (next[L - 1] + c[L - 1]) << 1;
#pragma unroll
      for (int L = 1; L <= 15; ++L)
         if (lane == 0) cnt[L] = (uint16_t)c[L];
      __syncthreads();
      for (int s0 = 0; s0 < n; s0 += 64) {
         const int s = s0 + lane, l = s < n ? (int)lens[s] : 0;
#pragma unroll
         for (int L = 1; L <= 15; ++L) {
            const uint64_t m = __ballot(l == L);
            if (l == L) {
               const uint32_t r = (uint32_t)__popcll(m & below);
               sym[off[L] + r] = (uint16_t)s;
               if (L <= fast_bits) {
                  const uint16_t e = (uint16_t)((s << 4) | L);
                  for (uint32_t k = bit_reverse(next[L] + r, L); k < (1u << fast_bits); k += 1u << L) fast[k] = e;
               }
            }
            const uint32_t k = (uint32_t)__popcll(m);
            off[L] += k, next[L] += k;
         }
      }
      __syncthreads();
      return SBGPU_BGZF_OK;
   }
};

// grid: one wave per member (blockDim 64).  status[b] and, for the members that failed, one add to *n_failed.
__global__ void __launch_bounds__(64, 4) bgzf_inflate_kernel(const uint8_t *__restrict__ file, int64_t n_bytes, const int64_t *__restrict__ blk_off,
                                                          const int64_t *__restrict__ out_off, int64_t n_blocks, uint8_t *out,
                                                          uint8_t *__restrict__ status, unsigned long long *n_failed)
{
   __shared__ WaveShared sh;
   const int64_t b = blockIdx.x;
   if (b >= n_blocks) return;
   const int64_t lo = blk_off[b], hi = blk_off[b + 1], o_lo = out_off[b], o_hi = out_off[b + 1];
   int st;
   if (lo < 0 || hi > n_bytes || hi - lo < HEADER + FOOTER || hi - lo > MAX_MEMBER) st = SBGPU_BGZF_EINPUT;
   else if (o_lo < 0 || o_hi < o_lo || o_hi - o_lo > MAX_ISIZE) st = SBGPU_BGZF_ESIZE;
   else {
      WaveMember m;
      m.lane = (int)threadIdx.x;
      m.pay = file + lo + HEADER;
      m.lead_ = (uint32_t)((uintptr_t)m.pay & 15u);
      m.base = m.pay - m.lead_;
      m.in_len = (int32_t)(hi - lo - HEADER - FOOTER), m.avail = m.in_len * 8;
      m.out = out + o_lo, m.isize = (int32_t)(o_hi - o_lo);
      m.align = (uint32_t)((uintptr_t)m.out & 15u);
      m.sh = &sh;
      st = inflate_member(m, &sh.t);
      m.flush(true); // (what a failed member had decoded as well: inside its own range)
   }
   if (threadIdx.x == 0) {
      if (status) status[b] = (uint8_t)st;
      if (st != SBGPU_BGZF_OK && n_failed) atomicAdd(n_failed, 1ull);
   }
}

// ---- record offsets of an inflated stream, on the device (sbgpu_bam_index_device) ------------------------------------
// The chain of block_size words is cut at guessed record starts and validated: segment i is [bound(i), bound(i + 1)),
// bound(0) = first_record, bound(i) = guess[i - 1] clamped into [first_record, n_bytes], bound(n_seg) = n_bytes.
// walk(i, e): follow the size words from entry e while the record STARTS inside the segment -> (records, exit): where the
// chain leaves the segment.  An entry at or behind the segment's end walks nothing and passes through (a record longer than
// a segment; an empty segment).  A negative size word ends the walk with exit = kIndexFault, a size word that is cut by the
// stream's end or runs past it with exit = kIndexPartial + its position; every later segment passes such an exit through.
// After the fixed point exit[last] tells what became of the TRUE chain, which is the only one whose end matters.
constexpr int64_t kIndexFault = INT64_MAX;
constexpr int64_t kIndexPartial = INT64_MAX / 2; // exit = kIndexPartial + p: the stream ends inside the record that starts at p
constexpr int64_t kIndexStride = 65536;          // the segments' length when no guesses are given
struct IndexArgs {
   const uint8_t *bytes;
   int64_t n_bytes, first_record;
   const int64_t *guess; // [n_seg - 1] or null
   int64_t guess_add;    // added to every guess (a caller whose guesses live in other coordinates)
   int64_t n_seg;
   int64_t *count, *entry_a, *exit_a, *entry_b, *exit_b; // [n_seg] each: the walks' results, and the (entry, exit) of two rounds
   unsigned long long *word;                 // [0] segments walked again this round, [1] the first of them
};
__device__ __forceinline__ int64_t index_bound(const IndexArgs &a, int64_t i)
{
   if (i <= 0) return a.first_record;
   if (i >= a.n_seg) return a.n_bytes;
   const int64_t g = a.guess ? a.guess[i - 1] + a.guess_add : a.first_record + i * kIndexStride;
   return g < a.first_record ? a.first_record : (g > a.n_bytes ? a.n_bytes : g);
}
// rec_off: null, or where the segment's offsets go (relative to first_record)
__device__ __forceinline__ void index_walk(const IndexArgs &a, int64_t end, int64_t e, int64_t *n_out, int64_t *exit_out, int64_t *rec_off)
{
   int64_t p = e, n = 0;
   while (p < end) { // (end <= n_bytes; an entry that is kIndexFault or kIndexPartial + p never enters)
      int32_t bs = 0;
      const bool cut = p + 4 > a.n_bytes;
      if (!cut) {
         const uint8_t *q = a.bytes + p;
         bs = (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
      }
      if (bs < 0) {
         p = kIndexFault;
         break;
      }
      if (cut || p + 4 + (int64_t)bs > a.n_bytes) {
         p += kIndexPartial;
         break;
      }
      if (rec_off) rec_off[n] = p - a.first_record;
      ++n, p += 4 + (int64_t)bs;
   }
   *n_out = n, *exit_out = p;
}
// round 1: every segment from its own bound
__global__ void __launch_bounds__(256) index_walk_kernel(IndexArgs a)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= a.n_seg) return;
   const int64_t e = index_bound(a, i);
   a.entry_a[i] = e;
   index_walk(a, index_bound(a, i + 1), e, &a.count[i], &a.exit_a[i], nullptr);
}
// A later round, from the state of the round before (in) to this one's (out).  A segment is CONSISTENT when its entry is its
// predecessor's exit (segment 0 always is).  An inconsistent segment is walked again from its predecessor's exit -- but only
// when that predecessor is consistent itself: the exit of an inconsistent one is garbage about to change, and a segment that
// adopted it would carry the error forward as fast as the truth follows.  So right guesses behind a wrong one stay as they
// are, the first inconsistent segment is always repaired, and a round that repairs nothing has found every segment consistent.
__global__ void __launch_bounds__(256) index_fix_kernel(IndexArgs a, const int64_t *__restrict__ entry_in, const int64_t *__restrict__ exit_in,
                                                        int64_t *__restrict__ entry_out, int64_t *__restrict__ exit_out)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= a.n_seg) return;
   const int64_t e = i ? exit_in[i - 1] : a.first_record, mine = entry_in[i];
   const bool pred_consistent = i < 2 || entry_in[i - 1] == exit_in[i - 2];
   if (mine == e || !pred_consistent) {
      entry_out[i] = mine, exit_out[i] = exit_in[i];
      return;
   }
   entry_out[i] = e;
   index_walk(a, index_bound(a, i + 1), e, &a.count[i], &exit_out[i], nullptr);
   atomicAdd(&a.word[0], 1ull);
   atomicMin(&a.word[1], (unsigned long long)i);
}
// the rounds' cap was reached: one lane walks the segments from `from` on in order (slow, exact)
__global__ void index_sequential_kernel(IndexArgs a, int64_t from, int64_t *entry_io, int64_t *exit_io)
{
   if (blockIdx.x || threadIdx.x) return;
   int64_t e = from ? exit_io[from - 1] : a.first_record;
   for (int64_t i = from; i < a.n_seg; ++i) {
      entry_io[i] = e;
      index_walk(a, index_bound(a, i + 1), e, &a.count[i], &e, nullptr);
      exit_io[i] = e;
   }
}
// counts -> where every segment's offsets begin: sums of blocks of 256, a scan of those by one workgroup, and the fill
__device__ __forceinline__ int64_t block_exclusive_scan_256(int64_t v, int64_t *total)
{
   __shared__ int64_t sh[256];
   const int t = (int)threadIdx.x;
   sh[t] = v;
   __syncthreads();
   for (int d = 1; d < 256; d <<= 1) {
      const int64_t x = t >= d ? sh[t - d] : 0;
      __syncthreads();
      sh[t] += x;
      __syncthreads();
   }
   const int64_t incl = sh[t];
   *total = sh[255];
   __syncthreads();
   return incl - v;
}
__global__ void __launch_bounds__(256) index_block_sums_kernel(IndexArgs a, int64_t *block_sum)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   int64_t total;
   block_exclusive_scan_256(i < a.n_seg ? a.count[i] : 0, &total);
   if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}
// block_sum[0 .. n) -> exclusive prefix in place, the total in block_sum[n]
__global__ void __launch_bounds__(256) index_scan_sums_kernel(int64_t *block_sum, int64_t n)
{
   int64_t carry = 0;
   for (int64_t k0 = 0; k0 < n; k0 += 256) {
      const int64_t k = k0 + threadIdx.x;
      int64_t total;
      const int64_t ex = block_exclusive_scan_256(k < n ? block_sum[k] : 0, &total);
      if (k < n) block_sum[k] = carry + ex;
      carry += total;
   }
   if (threadIdx.x == 0) block_sum[n] = carry;
}
__global__ void __launch_bounds__(256) index_fill_kernel(IndexArgs a, const int64_t *__restrict__ entry, const int64_t *__restrict__ block_sum,
                                                         int64_t *rec_off)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   int64_t total;
   const int64_t ex = block_exclusive_scan_256(i < a.n_seg ? a.count[i] : 0, &total);
   if (i >= a.n_seg) return;
   int64_t n, exit;
   index_walk(a, index_bound(a, i + 1), entry[i], &n, &exit, rec_off + block_sum[blockIdx.x] + ex);
   if (i == a.n_seg - 1) rec_off[block_sum[gridDim.x]] = (exit >= kIndexPartial ? exit - kIndexPartial : a.n_bytes) - a.first_record;
}
#endif // SB_BGZF_KERNELS

} // namespace bgzf
} // namespace sb
