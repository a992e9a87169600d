// strawberry_amd/csrc/bgzf_host.cpp -- BGZF on the host: the block table of a file (sbgpu_bgzf_index_host) and the host form
// of the inflate (sbgpu_bgzf_inflate_host): the decoder of bgzf_device.h run by one thread per member, members spread over
// host threads.  Plain C++, no zlib: the BAM header is parsed from what this returns, the CPU tests hold it to zlib, and the
// device form takes the same decisions because it is the same decoder.
#include <algorithm>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "api_internal.h"
#include "bgzf_device.h"

using sb::api_fail;

namespace {
using namespace sb::bgzf;

struct HostMember : MemberBase<HostMember> {
   const uint8_t *pay;
   uint8_t *out;

   uint32_t lead() const { return 0; }
   static uint32_t ld16(const uint16_t *p) { return *p; }
   void refill()
   {
      const int64_t at = (int64_t)wpos * 4;
      uint32_t w = 0;
      if (at + 4 <= in_len) std::memcpy(&w, pay + at, 4); // (little-endian hosts only, like the rest of the library)
      else
         for (int j = 0; j < 4; ++j)
            if (at + j < in_len) w |= (uint32_t)pay[at + j] << (8 * j);
      hold |= (uint64_t)w << nbits, nbits += 32, ++wpos;
   }
   void literal(uint8_t b) { out[pos] = b; }
   void match(int32_t len, int32_t dist)
   {
      const uint8_t *src = out + pos - dist;
      for (int32_t i = 0; i < len; ++i) out[pos + i] = src[i]; // byte by byte: an overlapping match repeats its own output
   }
   void stored(uint32_t at, uint32_t len) { std::memcpy(out + pos, pay + at, len); }
   void fixed_lens(Tables *t)
   {
      for (int s = 0; s < N_LIT + N_DIST; ++s) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < N_LIT ? 8 : 5);
   }
   void put_cl_lens(Tables *t, const uint32_t *cl, const uint8_t *order)
   {
      for (int k = 0; k < 19; ++k) t->lens[order[k]] = (uint8_t)cl[k];
   }
   void put_lens(Tables *t, int at, int n, uint32_t v) { std::memset(t->lens + at, (int)v, (size_t)n); }
   uint32_t len_at(Tables *t, int s) { return t->lens[s]; }
   int build_dynamic(Tables *t, int nlit, int ndist)
   {
      if (const int st = build(t->lens, nlit, t->lit_fast, FAST_L, t->lit_cnt, t->lit_sym, false)) return st;
      return build(t->lens + nlit, ndist, t->dist_fast, FAST_D, t->dist_cnt, t->dist_sym, false);
   }
   int build(const uint8_t *lens, int n, uint16_t *fast, int fast_bits, uint16_t *cnt, uint16_t *sym, bool strict)
   {
      uint32_t c[16] = {}, off[16], next[16];
      for (int s = 0; s < n; ++s) ++c[lens[s]];
      c[0] = 0;
      if (const int st = check_counts(c, strict)) return st;
      std::memset(fast, 0, sizeof(uint16_t) << fast_bits);
      off[0] = 0, next[0] = 0;
      for (int l = 1; l <= 15; ++l) off[l] = off[l - 1] + c[l - 1], next[l] = (next[l - 1] + c[l - 1]) << 1, cnt[l] = (uint16_t)c[l];
      for (int s = 0; s < n; ++s) {
         const int l = lens[s];
         if (!l) continue;
         sym[off[l]++] = (uint16_t)s;
         const uint32_t code = next[l]++;
         if (l <= fast_bits)
            for (uint32_t k = bit_reverse(code, l); k < (1u << fast_bits); k += 1u << l) fast[k] = (uint16_t)((s << 4) | l);
      }
      return SBGPU_BGZF_OK;
   }
};

int inflate_one(const uint8_t *file, int64_t n_bytes, int64_t lo, int64_t hi, int64_t o_lo, int64_t o_hi, uint8_t *out, Tables *t)
{
   if (lo < 0 || hi > n_bytes || hi - lo < HEADER + FOOTER || hi - lo > MAX_MEMBER) return SBGPU_BGZF_EINPUT;
   if (o_lo < 0 || o_hi < o_lo || o_hi - o_lo > MAX_ISIZE) return SBGPU_BGZF_ESIZE;
   HostMember m;
   m.pay = file + lo + HEADER;
   m.in_len = (int32_t)(hi - lo - HEADER - FOOTER), m.avail = m.in_len * 8;
   m.out = out + o_lo, m.isize = (int32_t)(o_hi - o_lo);
   return inflate_member(m, t);
}

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }
} // namespace

extern "C" {

int64_t sbgpu_bgzf_index_host(const uint8_t *file, int64_t n_bytes, int64_t *blk_off, int64_t *out_off, int64_t cap)
{
   if ((!file && n_bytes) || !blk_off || !out_off || n_bytes < 0 || cap < 0) {
      api_fail(SBGPU_EINVAL, "sbgpu_bgzf_index_host: bad argument");
      return -1;
   }
   int64_t n = 0, p = 0, o = 0;
   while (p < n_bytes) {
      const std::string where = "sbgpu_bgzf_index_host: member " + std::to_string(n) + " at byte " + std::to_string(p);
      if (p + HEADER > n_bytes) {
         api_fail(SBGPU_ESHAPE, where + ": the file ends inside the member's header");
         return -1;
      }
      const uint8_t *h = file + p;
      // the reference's check_header (samtools 0.1.19 bgzf.c:240-246), those tests and no others
      if (!(h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4) != 0 && le16(h + 10) == 6 && h[12] == 'B' && h[13] == 'C' && le16(h + 14) == 2)) {
         api_fail(SBGPU_EINVAL, where + ": not a BGZF header");
         return -1;
      }
      const int64_t size = (int64_t)le16(h + 16) + 1;
      if (size < HEADER + FOOTER) {
         api_fail(SBGPU_EINVAL, where + ": BSIZE leaves no room for the footer");
         return -1;
      }
      if (p + size > n_bytes) {
         api_fail(SBGPU_ESHAPE, where + ": the file ends inside the member");
         return -1;
      }
      const int64_t isize = (int64_t)le32(h + size - 4);
      if (isize > MAX_ISIZE) {
         api_fail(SBGPU_EINVAL, where + ": ISIZE " + std::to_string(isize) + " exceeds 65536");
         return -1;
      }
      if (n >= cap) {
         api_fail(SBGPU_ESHAPE, "sbgpu_bgzf_index_host: more than `cap` members");
         return -1;
      }
      blk_off[n] = p, out_off[n] = o, ++n;
      p += size, o += isize;
   }
   blk_off[n] = p, out_off[n] = o;
   return n;
}

int sbgpu_bgzf_inflate_host(const uint8_t *file, int64_t n_bytes, const int64_t *blk_off, const int64_t *out_off, int64_t first_block,
                            int64_t n_blocks, uint8_t *out, uint8_t *status)
{
   if (n_bytes < 0 || first_block < 0 || n_blocks < 0) return api_fail(SBGPU_EINVAL, "sbgpu_bgzf_inflate_host: bad argument");
   if (!n_blocks) return SBGPU_OK;
   if (!file || !blk_off || !out_off || !out || !status) return api_fail(SBGPU_EINVAL, "sbgpu_bgzf_inflate_host: null argument");
   unsigned nt = std::thread::hardware_concurrency();
   nt = nt ? std::min(nt, 16u) : 4u;
   if (const char *e = std::getenv("SBGPU_HOST_THREADS")) nt = (unsigned)std::atoi(e);
   nt = (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)nt, (n_blocks + 7) / 8));
   auto part = [&](unsigned t) {
      Tables tab;
      for (int64_t b = first_block + n_blocks * t / nt, e = first_block + n_blocks * (t + 1) / nt; b < e; ++b)
         status[b - first_block] = (uint8_t)inflate_one(file, n_bytes, blk_off[b], blk_off[b + 1], out_off[b], out_off[b + 1], out, &tab);
   };
   // (a thread that cannot be started must not leave joinable threads behind: its part and the ones after it run here)
   std::vector<std::thread> pool;
   unsigned started = 1;
   try {
      for (; started < nt; ++started) pool.emplace_back(part, started);
   } catch (const std::system_error &) {
   }
   part(0u);
   for (unsigned t = started; t < nt; ++t) part(t);
   for (std::thread &th : pool) th.join();
   return SBGPU_OK;
}

} // extern "C"
