// strawberry_amd/csrc/fasta_device.h -- the FASTA reader's kernels (include/sbgpu.h, sbgpu_fasta_read_device).  A
// stream compaction over the file's bytes: tiles of 16 KiB, a wave each, read with 16-byte loads (the buffer may begin anywhere:
// a chunk that leaves it is read byte by byte, nothing outside it is read).  No array has an entry per line, and no lane walks
// more bytes than its own sixteen -- but for the header lines, which are bounded (kFastaMaxHeader).
//
//   headers   fasta_count_kernel: per tile the '>' that begin a line, and the file's '\n'; fasta_scan_kernel; fasta_header_index_kernel:
//             their offsets in file order; fasta_header_walk_kernel: a wave per contig finds the header line's end and the name's;
//             fasta_names_kernel: the names into one byte buffer
//   bases     fasta_base_count_kernel: per tile the bytes of sequence lines that are no terminator, and per contig the first
//             '\n' behind its header (a guarded atomic minimum on one word per contig); fasta_first_line_kernel: line_bases,
//             line_width
//   pack      fasta_pack_kernel: the bases to their places (a popcount prefix within the wave, behind the tiles' scan), seq_off
//             where a header begins, and the two facts that make a contig RAGGED (fasta_rules.h): a base at a phase where a
//             full line has its terminator, and the first '\n' that ends no full line -- as the number of bases in front of it,
//             which the host compares with the contig's end
// Whether a byte is inside a header line is a two-state automaton over line starts; a wave resolves it with two ballots a round
// and carries it from round to round; at a tile's start it follows from the contigs' offsets.
// The launches and the arenas: fasta_api.hip; every threshold and layout: fasta_schedule.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fasta_rules.h"
#include "fasta_schedule.h"

namespace sb {

constexpr int64_t kFastaNone = 0x7f7f7f7f7f7f7f7fll; // "no such offset": what a fill with 0x7f leaves
// the words read back (FastaTileLayout::words): the file's '\n'; its last byte; the first byte of a non-empty line in front of
// the first header (kFastaNone: there is none); header lines longer than kFastaMaxHeader
enum { kFastaWordNewlines = 0, kFastaWordLast = 1, kFastaWordLeading = 2, kFastaWordLong = 3 };

// Sixteen bytes at a 16-byte aligned address, and what the rule says of each that is of the tile [t0, t1): masks with bit j for byte j
struct FastaChunk {
   uint32_t w[4];              // the bytes (those outside the buffer: 0)
   uint32_t in, nl, hs, term;  // of the tile; '\n'; '>' that begins a line; a terminator's byte
   int64_t p0;                 // byte 0's offset in the buffer (the first chunk's may be negative)
   int prev;                   // the byte in front of byte 0 ('\n' in front of the buffer)
   __device__ __forceinline__ uint8_t at(int j) const { return (uint8_t)(w[j >> 2] >> (8 * (j & 3))); }
};

__device__ __forceinline__ FastaChunk fasta_chunk(const uint8_t *bytes, int64_t n_bytes, const uint8_t *ca, int64_t t0, int64_t t1, bool live)
{
   FastaChunk k;
   k.w[0] = k.w[1] = k.w[2] = k.w[3] = 0, k.in = k.nl = k.hs = k.term = 0, k.prev = '\n';
   k.p0 = ca - bytes;
   if (!live) return k;
   const int64_t p0 = k.p0;
   if (p0 >= 0 && p0 + 16 <= n_bytes) {
      const uint4 v = *reinterpret_cast<const uint4 *>(ca);
      k.w[0] = v.x, k.w[1] = v.y, k.w[2] = v.z, k.w[3] = v.w;
   } else {
      for (int b = 0; b < 16; ++b)
         if (p0 + b >= 0 && p0 + b < n_bytes) k.w[b >> 2] |= (uint32_t)ca[b] << (8 * (b & 3));
   }
   const int64_t lo = t0 - p0 > 0 ? t0 - p0 : 0, hi = t1 - p0 < 16 ? t1 - p0 : 16;
   k.in = hi > lo ? ((hi >= 16 ? 0xffffu : (1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
   if (!k.in) return k;
   if (p0 > 0) k.prev = bytes[p0 - 1];
   const int next = p0 + 16 < n_bytes ? (int)bytes[p0 + 16] : -1;
#pragma unroll
   for (int j = 0; j < 16; ++j) {
      if (!((k.in >> j) & 1u)) continue;
      const uint8_t b = k.at(j);
      const int pb = p0 + j == 0 ? '\n' : (j ? (int)k.at(j ? j - 1 : 0) : k.prev);
      const int nb = p0 + j + 1 >= n_bytes ? -1 : (j < 15 ? (int)k.at(j < 15 ? j + 1 : 15) : next);
      if (b == '\n') k.nl |= 1u << j;
      if (b == '>' && pb == '\n') k.hs |= 1u << j;
      if (fasta_is_term(b, nb)) k.term |= 1u << j;
   }
   return k;
}

__device__ __forceinline__ int fasta_wave_sum(int v)
{
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}
__device__ __forceinline__ int fasta_wave_incl(int v, int lane)
{
#pragma unroll
   for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
   }
   return v;
}
// Whether this lane's first byte is inside a header line.  carry: the same for the round's first byte, in; for the next
// round's, out (wave-uniform).  A chunk with a line start decides the state behind it alone: inside exactly when its last
// event is a header's '>' and no '\n' follows it.
__device__ __forceinline__ bool fasta_header_state(const FastaChunk &k, int lane, bool &carry)
{
   const uint32_t ev = k.nl | k.hs;
   const bool has = ev != 0;
   const bool out = has && ((k.hs >> (31 - __clz((int)ev))) & 1u);
   const unsigned long long hasm = __ballot(has), outm = __ballot(out);
   const unsigned long long below = hasm & ((1ull << lane) - 1ull);
   const bool mine = below ? (outm >> (63 - __clzll((long long)below))) & 1ull : carry;
   carry = hasm ? (outm >> (63 - __clzll((long long)hasm))) & 1ull : carry;
   return mine;
}
__device__ __forceinline__ int64_t fasta_peek(const int64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a minimum kept in one word per contig: the atomic only where the word read (possibly stale, never too small) does not settle it
__device__ __forceinline__ void fasta_note_min(int64_t *word, int64_t v)
{
   if (fasta_peek(word) > v) atomicMin((long long *)word, (long long)v);
}

// the tiles a wave takes, and a tile's chunks
struct FastaTiles {
   int64_t n_tiles, shift;
   const uint8_t *base; // 16-byte aligned; chunk c is base + 16 c
   __device__ __forceinline__ FastaTiles(const uint8_t *bytes, int64_t n_bytes)
   {
      n_tiles = (n_bytes + kFastaTile - 1) / kFastaTile;
      shift = (int64_t)((uintptr_t)bytes & 15u);
      base = bytes - shift;
   }
};

// ------------------------------------------------------------------ the headers
// a wave per tile: tile_hdr[tile] = the '>' that begin a line; words: the '\n' of the file, its last byte
__global__ __launch_bounds__(64) void fasta_count_kernel(const uint8_t *bytes, int64_t n_bytes, int32_t *tile_hdr, int64_t *words)
{
   const int lane = (int)threadIdx.x;
   const FastaTiles T(bytes, n_bytes);
   int64_t newlines = 0;
   for (int64_t tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
      const int64_t t0 = tile * kFastaTile, t1 = t0 + kFastaTile < n_bytes ? t0 + kFastaTile : n_bytes;
      const int64_t c0 = (T.shift + t0) >> 4, c1 = (T.shift + t1 + 15) >> 4;
      int h = 0, l = 0;
      for (int64_t c = c0 + lane; c < c1; c += 64) {
         const FastaChunk k = fasta_chunk(bytes, n_bytes, T.base + 16 * c, t0, t1, true);
         h += __popc(k.hs), l += __popc(k.nl);
      }
      h = fasta_wave_sum(h), l = fasta_wave_sum(l);
      newlines += l;
      if (lane == 0) tile_hdr[tile] = h;
      if (lane == 0 && tile == T.n_tiles - 1) words[kFastaWordLast] = (int64_t)bytes[n_bytes - 1];
   }
   if (lane == 0 && newlines) atomicAdd((unsigned long long *)&words[kFastaWordNewlines], (unsigned long long)newlines);
}

// One workgroup: out[i] = in[0] + .. + in[i - 1] for i = 0 .. n (out[n]: the total), in 64 bits, kFastaScanTile entries a round
__global__ __launch_bounds__(256) void fasta_scan_kernel(const int32_t *in, int64_t *out, int64_t n)
{
   __shared__ int64_t s_wave[4];
   const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
   int64_t carry = 0;
   for (int64_t base = 0; base < n; base += kFastaScanTile) {
      const int64_t i0 = base + 4 * (int64_t)tid;
      int64_t v[4], sum = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? (int64_t)in[i0 + k] : 0, sum += v[k];
      int64_t incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
         const int64_t t = __shfl_up(incl, o);
         if (lane >= o) incl += t;
      }
      if (lane == 63) s_wave[wv] = incl;
      __syncthreads();
      int64_t run = carry + incl - sum, all = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
         if (w < wv) run += s_wave[w];
         all += s_wave[w];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
         if (i0 + k < n) out[i0 + k] = run;
         run += v[k];
      }
      carry += all;
      __syncthreads(); // (the next round overwrites s_wave)
   }
   if (tid == 0) out[n] = carry;
}

// a wave per tile again: hdr_off[k] = the k-th header's '>'; hdr_off[n_contigs] = n_bytes
__global__ __launch_bounds__(64) void fasta_header_index_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *hdr_at, int64_t *hdr_off, int64_t n_contigs)
{
   const int lane = (int)threadIdx.x;
   const FastaTiles T(bytes, n_bytes);
   if (blockIdx.x == 0 && lane == 0) hdr_off[n_contigs] = n_bytes;
   for (int64_t tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
      const int64_t t0 = tile * kFastaTile, t1 = t0 + kFastaTile < n_bytes ? t0 + kFastaTile : n_bytes;
      const int64_t c0 = (T.shift + t0) >> 4, c1 = (T.shift + t1 + 15) >> 4;
      int64_t at = hdr_at[tile];
      if (hdr_at[tile + 1] == at) continue; // (wave-uniform: nothing begins here)
      for (int64_t cb = c0; cb < c1; cb += 64) {
         const int64_t c = cb + lane;
         const FastaChunk k = fasta_chunk(bytes, n_bytes, T.base + 16 * c, t0, t1, c < c1);
         const int cnt = __popc(k.hs), incl = fasta_wave_incl(cnt, lane);
         int64_t i = at + (incl - cnt);
         uint32_t m = k.hs;
         while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1u;
            if (i < n_contigs) hdr_off[i] = k.p0 + b; // (the bytes are the caller's: a buffer that changed under the call writes nothing outside)
            ++i;
         }
         at += __shfl(incl, 63);
      }
   }
}

// A wave per contig walks its header line, 64 bytes a step and kFastaMaxHeader + 2 at most: offset (the byte behind the line's
// '\n', n_bytes without one), the name's length (up to the first isspace byte or the buffer's end), and whether the line is
// longer than the device form takes (words[kFastaWordLong] counts those; their offset is then only inside the buffer).
__global__ __launch_bounds__(256) void fasta_header_walk_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *hdr_off, int64_t n_contigs, int64_t *offset,
                                                                int32_t *name_len, int64_t *words)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
   for (int64_t c = wave; c < n_contigs; c += n_waves) {
      const int64_t h = hdr_off[c];
      if (h < 0 || h >= n_bytes) continue;
      int64_t name_end = -1, q = -1;
      bool is_long = false;
      for (int64_t base = h + 1;; base += 64) {
         const int64_t p = base + lane;
         const bool inb = p < n_bytes;
         const uint8_t b = inb ? bytes[p] : (uint8_t)0;
         const unsigned long long m_sp = __ballot(inb && fasta_isspace(b)), m_nl = __ballot(inb && b == (uint8_t)'\n'), m_end = __ballot(!inb);
         if (name_end < 0 && (m_sp | m_end)) name_end = base + (__ffsll((long long)(m_sp | m_end)) - 1);
         if (m_nl && (!m_end || __ffsll((long long)m_nl) < __ffsll((long long)m_end))) {
            q = base + (__ffsll((long long)m_nl) - 1);
            break;
         }
         if (m_end) {
            q = n_bytes;
            break;
         }
         if (base + 64 > h + kFastaMaxHeader + 2) {
            is_long = true;
            break;
         }
      }
      if (!is_long) {
         int64_t ce = q;
         if (q < n_bytes && q - 1 > h && bytes[q - 1] == (uint8_t)'\r') ce = q - 1;
         is_long = ce - h > kFastaMaxHeader;
      }
      if (lane == 0) {
         if (is_long) {
            offset[c] = h + 1 < n_bytes ? h + 1 : n_bytes, name_len[c] = 0;
            atomicAdd((unsigned long long *)&words[kFastaWordLong], 1ull);
         } else {
            offset[c] = q < n_bytes ? q + 1 : n_bytes, name_len[c] = (int32_t)(name_end - (h + 1));
         }
      }
   }
}

// a wave per contig: its name's bytes to names[name_at[c] ..]
__global__ __launch_bounds__(256) void fasta_names_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *hdr_off, const int64_t *name_at, int64_t n_contigs,
                                                          int64_t n_names, uint8_t *names)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
   for (int64_t c = wave; c < n_contigs; c += n_waves) {
      const int64_t h = hdr_off[c], at = name_at[c], len = name_at[c + 1] - at;
      if (h < 0 || at < 0 || len < 0 || at + len > n_names || h + 1 + len > n_bytes) continue;
      for (int64_t i = lane; i < len; i += 64) names[at + i] = bytes[h + 1 + i];
   }
}

// ------------------------------------------------------------------ the bases
struct FastaArgs {
   const uint8_t *bytes;
   int64_t n_bytes;
   const int64_t *hdr_at;   // [tiles + 1] headers in front of a tile
   const int64_t *hdr_off;  // [contigs + 1]
   const int64_t *offset;   // [contigs]
   int64_t n_contigs;
   // the count
   int32_t *base_cnt;       // [tiles]
   int64_t *first_nl;       // [contigs], kFastaNone to begin with
   int64_t *words;
   // the pack
   const int64_t *base_at;  // [tiles + 1] bases in front of a tile
   const int64_t *line_bases, *line_width;
   int64_t n_bases;
   uint8_t *seq;            // [n_bases]
   int64_t *seq_off;        // [contigs]: written where a header begins
   int64_t *first_odd;      // [contigs], kFastaNone to begin with: bases in front of the first '\n' that ends no full line
   int32_t *ragged;         // [contigs], 0 to begin with: a base stands out of phase
};

// the state at a tile's first byte: the headers in front of it, and whether the last of them has its line still open
__device__ __forceinline__ bool fasta_tile_in_header(const FastaArgs &a, int64_t hk, int64_t t0)
{
   return hk > 0 && hk <= a.n_contigs && t0 < a.offset[hk - 1];
}

// a wave per tile: base_cnt[tile]; first_nl[c]; words[kFastaWordLeading]
__global__ __launch_bounds__(64) void fasta_base_count_kernel(FastaArgs a)
{
   const int lane = (int)threadIdx.x;
   const FastaTiles T(a.bytes, a.n_bytes);
   int64_t leading = kFastaNone;
   for (int64_t tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
      const int64_t t0 = tile * kFastaTile, t1 = t0 + kFastaTile < a.n_bytes ? t0 + kFastaTile : a.n_bytes;
      const int64_t c0 = (T.shift + t0) >> 4, c1 = (T.shift + t1 + 15) >> 4;
      int64_t hk = a.hdr_at[tile];
      bool carry = fasta_tile_in_header(a, hk, t0);
      int cnt = 0;
      for (int64_t cb = c0; cb < c1; cb += 64) {
         const int64_t ci = cb + lane;
         const FastaChunk k = fasta_chunk(a.bytes, a.n_bytes, T.base + 16 * ci, t0, t1, ci < c1);
         bool s = fasta_header_state(k, lane, carry);
         const int hcnt = __popc(k.hs), hincl = fasta_wave_incl(hcnt, lane);
         int64_t c = hk + (hincl - hcnt) - 1, noted = -2;
#pragma unroll
         for (int j = 0; j < 16; ++j) {
            if (!((k.in >> j) & 1u)) continue;
            const bool nl = (k.nl >> j) & 1u, term = (k.term >> j) & 1u;
            if ((k.hs >> j) & 1u) ++c, s = true;
            if (c < 0) {
               if (!term && k.p0 + j < leading) leading = k.p0 + j;
            } else if (!s && c < a.n_contigs) {
               if (!term) ++cnt;
               if (nl && noted != c) fasta_note_min(&a.first_nl[c], k.p0 + j), noted = c;
            }
            if (nl) s = false;
         }
         hk += __shfl(hincl, 63);
      }
      cnt = fasta_wave_sum(cnt);
      if (lane == 0) a.base_cnt[tile] = cnt;
   }
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) {
      const int64_t t = __shfl_xor(leading, o);
      leading = t < leading ? t : leading;
   }
   if (lane == 0 && leading != kFastaNone) fasta_note_min(&a.words[kFastaWordLeading], leading);
}

// a lane per contig: the first line's two lengths from the first '\n' behind the header
__global__ __launch_bounds__(256) void fasta_first_line_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *hdr_off, const int64_t *offset, const int64_t *first_nl,
                                                               int64_t n_contigs, int64_t *line_bases, int64_t *line_width)
{
   for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_contigs; c += (int64_t)gridDim.x * blockDim.x) {
      const int64_t off = offset[c], end = hdr_off[c + 1], q = first_nl[c];
      const bool cr = q < end && q < n_bytes && q - 1 >= off && bytes[q - 1] == (uint8_t)'\r';
      int64_t lb = 0, lw = 0;
      if (off >= 0 && off <= end) fasta_first_line(off, end, q, cr, &lb, &lw);
      line_bases[c] = lb, line_width[c] = lw;
   }
}

// ------------------------------------------------------------------ the pack
// a wave per tile: every base to seq[bases in front of it]; seq_off[c] where contig c's header begins; first_odd, ragged
__global__ __launch_bounds__(64) void fasta_pack_kernel(FastaArgs a)
{
   const int lane = (int)threadIdx.x;
   const FastaTiles T(a.bytes, a.n_bytes);
   for (int64_t tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
      const int64_t t0 = tile * kFastaTile, t1 = t0 + kFastaTile < a.n_bytes ? t0 + kFastaTile : a.n_bytes;
      const int64_t c0 = (T.shift + t0) >> 4, c1 = (T.shift + t1 + 15) >> 4;
      int64_t hk = a.hdr_at[tile], at = a.base_at[tile];
      bool carry = fasta_tile_in_header(a, hk, t0);
      for (int64_t cb = c0; cb < c1; cb += 64) {
         const int64_t ci = cb + lane;
         const FastaChunk k = fasta_chunk(a.bytes, a.n_bytes, T.base + 16 * ci, t0, t1, ci < c1);
         const bool s_in = fasta_header_state(k, lane, carry);
         const int hcnt = __popc(k.hs), hincl = fasta_wave_incl(hcnt, lane);
         const int64_t c_in = hk + (hincl - hcnt) - 1;
         // this lane's bases: of a sequence line, no terminator
         uint32_t basem = 0;
         {
            bool s = s_in;
            int64_t c = c_in;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
               if (!((k.in >> j) & 1u)) continue;
               if ((k.hs >> j) & 1u) ++c, s = true;
               if (!s && c >= 0 && !((k.term >> j) & 1u)) basem |= 1u << j;
               if ((k.nl >> j) & 1u) s = false;
            }
         }
         const int bcnt = __popc(basem), bincl = fasta_wave_incl(bcnt, lane);
         int64_t idx = at + (bincl - bcnt);
         if (k.in) {
            bool s = s_in, have = false;
            int64_t c = c_in, off = 0, lb = 0, lw = 0, ph = -1;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
               if (!((k.in >> j) & 1u)) continue;
               const bool nl = (k.nl >> j) & 1u;
               const int64_t p = k.p0 + j;
               if ((k.hs >> j) & 1u) {
                  ++c, s = true, have = false;
                  if (c < a.n_contigs) a.seq_off[c] = idx;
               }
               if (!s && c >= 0 && c < a.n_contigs) {
                  if (!have) off = a.offset[c], lb = a.line_bases[c], lw = a.line_width[c], have = true, ph = -1;
                  if (ph < 0 && lw > 0) {
                     const uint64_t rel = (uint64_t)(p - off), w = (uint64_t)lw;
                     ph = rel < w ? (int64_t)rel : ((rel | w) >> 32 ? (int64_t)(rel % w) : (int64_t)((uint32_t)rel % (uint32_t)w));
                  }
                  if ((basem >> j) & 1u) {
                     if (idx < a.n_bases) a.seq[idx] = k.at(j);
                     ++idx;
                     if (lw > 0 && fasta_base_out_of_phase(ph, lb) && !a.ragged[c]) atomicOr(&a.ragged[c], 1);
                  } else if (nl && lw > 0) {
                     const int pb = j ? (int)k.at(j ? j - 1 : 0) : k.prev;
                     if (fasta_line_end_odd(ph, lb, lw, pb == '\r')) fasta_note_min(&a.first_odd[c], idx);
                  }
                  if (lw > 0 && ++ph == lw) ph = 0;
               }
               if (nl) {
                  if (s) ph = -1; // (the header's line ends: the next byte is the contig's offset)
                  s = false;
               }
            }
         }
         hk += __shfl(hincl, 63), at += __shfl(bincl, 63);
      }
   }
}

} // namespace sb
