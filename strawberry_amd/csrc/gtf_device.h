// strawberry_amd/csrc/gtf_device.h -- the GTF reader's kernels (include/sbgpu.h, sbgpu_gtf_read_device).  The
// pattern is the BAM decoder's (bamdecode_device.h): the file's bytes in, one lane per line, scans to place what is accepted.
//
//   line index   gtf_newline_count_kernel, gtf_tile_scan_kernel, gtf_line_index_kernel: the '\n' of every tile of 16 KiB, counted
//                and then placed with 16-byte loads (the buffer may begin anywhere: its first and last sixteen bytes are read
//                byte by byte, nothing outside it is read)
//   parse        gtf_parse_kernel: a wave's 64 consecutive lines are contiguous bytes -- staged into LDS with coalesced loads,
//                then every lane walks its line through 8-byte windows (gtf_rules.h: gtf_parse_line, the host form's function);
//                gtf_compact_kernel: the accepted lines' records in line order, behind a scan over the waves' totals
//   group        two stable radix sorts (by (left, right), then by the transcript key's hash: the launcher's), then
//                gtf_merge_kernel: one lane per transcript merges its exons, notes its first line and compares every member's
//                key bytes with the first member's (a difference is a hash collision: the call is refused);
//                gtf_names_kernel: the transcripts' names into one byte buffer
// The launches, the arenas and the sorts: gtf_api.hip; every threshold and layout: gtf_schedule.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtf_rules.h"
#include "gtf_schedule.h"

namespace sb {

// An accepted line.  The chromosome name begins the line; the other names' places are from the line's first byte.
struct GtfRec {
   uint64_t h_tx, h_gene, h_chrom;
   uint32_t line, left, right;
   uint16_t o_gene, o_tx, o_gname;
   uint8_t l_chrom, l_gene, l_tx, l_gname, strand, pad;
};
// A transcript: its first line's record, its merged exons xl / xr [exon_at, exon_at + n_exons), its names' place in the buffer
// (chromosome as written, gene_id, transcript_id, gene_name: behind each other)
struct GtfTx {
   uint64_t h_chrom;
   int64_t name_at;
   uint32_t first_line, first_rec, exon_at, n_exons, merges;
   uint8_t strand, l_chrom, l_gene, l_tx, l_gname, collision, pad[2];
};
// A staged line's bytes, eight at a time: the two aligned 8-byte words around p, shifted together, as the BAM decoder's
// ByteWindow reads its records (bamdecode_device.h, whose kernels this unit must not define a second time).  The buffer is LDS
// and the pointer says so (ds_read2_b64, no flat loads); up to 15 bytes beyond a line's end are the buffer's own.
struct GtfWindow {
   __device__ __forceinline__ uint64_t peek8(const uint8_t *p, const uint8_t *) const
   {
      const uintptr_t q = (uintptr_t)p;
      const __attribute__((address_space(3))) uint64_t *b = (const __attribute__((address_space(3))) uint64_t *)(uint32_t)(q & ~(uintptr_t)7);
      const uint64_t lo = b[0], hi = b[1];
      const unsigned sh = 8u * (unsigned)(q & 7u);
      return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
   }
};
static_assert(sizeof(GtfRec) == kGtfRecBytes && sizeof(GtfTx) == kGtfTxBytes, "gtf_schedule.h lays the arenas out");

// ------------------------------------------------------------------ the line index
// The sixteen bytes at the 16-byte aligned address `ca` as a mask of their '\n': bit b for byte b, and only for bytes whose
// offset in the buffer is in [t0, t1) -- the tile.  A chunk that leaves the buffer is read byte by byte.
__device__ __forceinline__ uint32_t gtf_newline_mask(const uint8_t *bytes, int64_t n_bytes, const uint8_t *ca, int64_t t0, int64_t t1)
{
   const int64_t p0 = ca - bytes; // the chunk's first byte, as an offset (negative: in front of the buffer)
   uint32_t w[4] = {0, 0, 0, 0};
   if (p0 >= 0 && p0 + 16 <= n_bytes) {
      const uint4 v = *reinterpret_cast<const uint4 *>(ca);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
   } else {
      for (int b = 0; b < 16; ++b)
         if (p0 + b >= 0 && p0 + b < n_bytes) w[b >> 2] |= (uint32_t)ca[b] << (8 * (b & 3));
   }
   uint32_t m = 0;
#pragma unroll
   for (int k = 0; k < 4; ++k) {
      const uint32_t y = w[k] ^ 0x0a0a0a0au; // a zero byte where the '\n' was
      const uint32_t z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu); // 0x80 in exactly those bytes
      m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xfu) << (4 * k); // the four flags side by side
   }
   // the bytes of the tile: offsets lo .. hi - 1 of the chunk
   const int64_t lo = t0 - p0 > 0 ? t0 - p0 : 0, hi = t1 - p0 < 16 ? t1 - p0 : 16;
   const uint32_t in = hi > lo ? ((hi >= 16 ? 0xffffu : (1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
   return m & in;
}
__device__ __forceinline__ int gtf_wave_sum(int v)
{
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}

// a wave per tile of kGtfIndexTile bytes: tile_cnt[tile] = its '\n'; words[1] = the file's last byte
__global__ __launch_bounds__(256) void gtf_newline_count_kernel(const uint8_t *bytes, int64_t n_bytes, int32_t *tile_cnt, int64_t *words)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int64_t n_tiles = (n_bytes + kGtfIndexTile - 1) / kGtfIndexTile;
   const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
   const int64_t shift = (int64_t)((uintptr_t)bytes & 15u);
   const uint8_t *base = bytes - shift; // 16-byte aligned; chunk c is base + 16 c
   for (int64_t tile = wave; tile < n_tiles; tile += n_waves) {
      const int64_t t0 = tile * kGtfIndexTile, t1 = t0 + kGtfIndexTile < n_bytes ? t0 + kGtfIndexTile : n_bytes;
      const int64_t c0 = (shift + t0) >> 4, c1 = (shift + t1 + 15) >> 4;
      int mine = 0;
      for (int64_t c = c0 + lane; c < c1; c += 64) mine += __popc(gtf_newline_mask(bytes, n_bytes, base + 16 * c, t0, t1));
      mine = gtf_wave_sum(mine);
      if (lane == 0) tile_cnt[tile] = mine;
      if (lane == 0 && tile == n_tiles - 1) words[1] = (int64_t)bytes[n_bytes - 1];
   }
}

// One workgroup: out[i] = in[0] + .. + in[i - 1] for i = 0 .. n (out[n]: the total, also to *total), kGtfScanTile entries a round
__global__ __launch_bounds__(256) void gtf_tile_scan_kernel(const int32_t *in, int64_t *out, int64_t n, int64_t *total)
{
   __shared__ int64_t s_wave[4];
   const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
   int64_t carry = 0;
   for (int64_t base = 0; base < n; base += kGtfScanTile) {
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
   if (tid == 0) {
      out[n] = carry;
      if (total) *total = carry;
   }
}

// a wave per tile again: line_off[k + 1] = the byte behind the k-th '\n'; line_off[0] = 0, line_off[n_lines] = n_bytes
__global__ __launch_bounds__(256) void gtf_line_index_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *tile_at, int64_t *line_off, int64_t n_lines)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int64_t n_tiles = (n_bytes + kGtfIndexTile - 1) / kGtfIndexTile;
   const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
   const int64_t shift = (int64_t)((uintptr_t)bytes & 15u);
   const uint8_t *base = bytes - shift;
   if (wave == 0 && lane == 0) line_off[0] = 0, line_off[n_lines] = n_bytes;
   for (int64_t tile = wave; tile < n_tiles; tile += n_waves) {
      const int64_t t0 = tile * kGtfIndexTile, t1 = t0 + kGtfIndexTile < n_bytes ? t0 + kGtfIndexTile : n_bytes;
      const int64_t c0 = (shift + t0) >> 4, c1 = (shift + t1 + 15) >> 4;
      int64_t at = tile_at[tile]; // the '\n' in front of the tile
      for (int64_t cb = c0; cb < c1; cb += 64) { // (wave-uniform)
         const int64_t c = cb + lane;
         uint32_t m = c < c1 ? gtf_newline_mask(bytes, n_bytes, base + 16 * c, t0, t1) : 0u;
         const int cnt = __popc(m);
         int incl = cnt;
#pragma unroll
         for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
         }
         int64_t k = at + (incl - cnt);
         const int64_t p0 = 16 * c - shift;
         while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1u;
            ++k;
            if (k <= n_lines) line_off[k] = p0 + b + 1; // (the bytes are the caller's: a buffer that changed under the call writes nothing outside)
         }
         at += __shfl(incl, 63);
      }
   }
}

// ------------------------------------------------------------------ the parse
struct GtfParseArgs {
   const uint8_t *bytes;
   int64_t n_bytes;
   const int64_t *line_off; // [n_lines + 1]
   int64_t n_lines;
   uint8_t *status;            // per line
   GtfRec *rec;                // per line: written for an accepted one
   int32_t *tile_cnt;          // per tile of 64 lines: the accepted ones
   unsigned long long *counts; // [16], by status
};

// One wave per workgroup, 64 lines per pass, as bam_scan_kernel: the lines' whole range goes to LDS with 16-byte loads, eight
// in flight per lane, and the lanes walk their lines there through GtfWindow; a range beyond the buffer is walked in global
// memory.  A line of more than kGtfMaxLine bytes is not read: the call is refused.
__global__ __launch_bounds__(64) void gtf_parse_kernel(GtfParseArgs a)
{
   extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
   __shared__ unsigned int cnt[16];
   const int lane = threadIdx.x;
   if (lane < 16) cnt[lane] = 0;
   __syncthreads();
   const int64_t n_tiles = (a.n_lines + 63) >> 6;
   for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t r0 = tile << 6, r1 = r0 + 64 < a.n_lines ? r0 + 64 : a.n_lines;
      const int64_t s0 = a.line_off[r0], s1 = a.line_off[r1];
      const uint8_t *g = a.bytes + s0;
      const int shift = (int)((uintptr_t)g & 15u);
      const bool staged = s0 >= 0 && s1 <= a.n_bytes && gtf_tile_staged(s0, s1); // (the launch brings kGtfStageBytes of LDS)
      if (staged) {
         const int len = (int)(s1 - s0);
         const int head = min((16 - shift) & 15, len), nbody = (len - head) >> 4, tail = len - head - (nbody << 4);
         if (lane < head) stage[shift + lane] = g[lane];
         const uint4 *src = reinterpret_cast<const uint4 *>(g + head);
         uint4 *dst = reinterpret_cast<uint4 *>(stage + shift + head);
         for (int c0 = 0; c0 < nbody; c0 += 8 * 64) {
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
               const int c = c0 + k * 64 + lane;
               v[k] = c < nbody ? src[c] : uint4{0, 0, 0, 0};
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
               const int c = c0 + k * 64 + lane;
               if (c < nbody) dst[c] = v[k];
            }
         }
         if (lane < tail) stage[shift + head + (nbody << 4) + lane] = g[head + (nbody << 4) + lane];
      }
      __syncthreads();
      const int64_t r = r0 + lane;
      bool my_ok = false;
      if (r < r1) {
         const int64_t o0 = a.line_off[r], o1 = a.line_off[r + 1];
         const bool inside = o0 >= s0 && o1 >= o0 && o1 <= s1 && o0 >= 0 && o1 <= a.n_bytes;
         GtfLine x;
         x.status = kGtfSkip;
         if (inside) {
            const uint8_t *line = staged ? stage + shift + (o0 - s0) : a.bytes + o0;
            int64_t len = o1 - o0;
            if (len > 0 && line[len - 1] == (uint8_t)'\n') --len; // (every line but the file's last ends in one)
            len = gtf_line_len(line, len);
            if (!gtf_line_fits(len)) {
               x.status = kGtfLineLong;
            } else {
               if (staged) {
                  GtfWindow rd;
                  gtf_parse_line(rd, line, len, x);
               } else {
                  GtfBytes rd;
                  gtf_parse_line(rd, line, len, x);
               }
            }
         }
         a.status[r] = x.status;
         my_ok = x.status == kGtfOk;
         if (my_ok) {
            GtfRec q;
            q.h_tx = x.h_tx, q.h_gene = x.h_gene, q.h_chrom = x.h_chrom;
            q.line = (uint32_t)r, q.left = x.left, q.right = x.right;
            q.o_gene = (uint16_t)x.o_gene, q.o_tx = (uint16_t)x.o_tx, q.o_gname = (uint16_t)x.o_gname;
            q.l_chrom = (uint8_t)x.l_chrom, q.l_gene = (uint8_t)x.l_gene, q.l_tx = (uint8_t)x.l_tx, q.l_gname = (uint8_t)x.l_gname;
            q.strand = x.strand, q.pad = 0;
            a.rec[r] = q;
         }
         atomicAdd(&cnt[x.status < kGtfStatuses ? x.status : kGtfStatuses], 1u);
      }
      const unsigned long long okm = __ballot(my_ok);
      if (lane == 0) a.tile_cnt[tile] = (int32_t)__popcll(okm);
      __syncthreads(); // (the next pass overwrites the buffer)
   }
   if (lane < 16 && cnt[lane]) atomicAdd(&a.counts[lane], (unsigned long long)cnt[lane]);
}

// a wave per tile of 64 lines: the accepted lines' records in line order, and the first sort's key and value
__global__ __launch_bounds__(256) void gtf_compact_kernel(const uint8_t *status, const GtfRec *rec, const int64_t *tile_at, int64_t n_lines, int64_t m,
                                                          GtfRec *out, unsigned long long *key, uint32_t *val)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int64_t n_tiles = (n_lines + 63) >> 6, wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
   for (int64_t tile = wave; tile < n_tiles; tile += n_waves) {
      const int64_t r = (tile << 6) + lane;
      const bool ok = r < n_lines && status[r] == kGtfOk;
      const unsigned long long okm = __ballot(ok);
      const int64_t k = tile_at[tile] + __popcll(okm & ((1ull << lane) - 1ull));
      if (!ok || k >= m) continue;
      const GtfRec q = rec[r];
      out[k] = q;
      key[k] = ((unsigned long long)q.left << 32) | q.right;
      val[k] = (uint32_t)k;
   }
}

// ------------------------------------------------------------------ the grouping
// the second sort's key: the transcript key's hash of the record at every place of the first sort's order, cut to `mask`
__global__ __launch_bounds__(256) void gtf_hash_keys_kernel(const GtfRec *rec, const uint32_t *order, int64_t m, unsigned long long mask, unsigned long long *key)
{
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) key[i] = rec[order[i]].h_tx & mask;
}
// a transcript begins where the sorted hash changes
__global__ __launch_bounds__(256) void gtf_heads_kernel(const unsigned long long *key, int64_t m, uint8_t *head)
{
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) head[i] = i == 0 || key[i] != key[i - 1];
}
// seg: the heads' inclusive scan.  tx_first[t] = where transcript t begins, tx_first[T] = m; words[0] = T
__global__ __launch_bounds__(256) void gtf_first_kernel(const uint8_t *head, const int32_t *seg, int64_t m, uint32_t *tx_first, int64_t *words)
{
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
      if (head[i]) tx_first[seg[i] - 1] = (uint32_t)i;
      if (i == m - 1) tx_first[seg[i]] = (uint32_t)m, words[0] = (int64_t)seg[i];
   }
}

// the key bytes of record q against record f's: the chromosome name without case, the strand, the transcript_id
__device__ inline bool gtf_same_key(const uint8_t *bytes, const int64_t *line_off, const GtfRec &f, const GtfRec &q)
{
   if (f.l_chrom != q.l_chrom || f.l_tx != q.l_tx || f.strand != q.strand) return false;
   const uint8_t *lf = bytes + line_off[f.line], *lq = bytes + line_off[q.line];
   bool same = true;
   for (int i = 0; i < (int)f.l_chrom; ++i) same &= gtf_lower(lf[i]) == gtf_lower(lq[i]);
   for (int i = 0; i < (int)f.l_tx; ++i) same &= lf[f.o_tx + i] == lq[q.o_tx + i];
   return same;
}

struct GtfMergeArgs {
   const uint8_t *bytes;
   const int64_t *line_off;
   const GtfRec *rec;       // [m] in line order
   const uint32_t *order;   // [m] by (hash, left, right, line)
   const uint32_t *tx_first; // [T + 1]
   int64_t n_tx;
   uint32_t *xl, *xr;       // [m]: a transcript's merged exons from tx_first[t]
   GtfTx *tx;               // [T]
   int32_t *name_len;       // [T]
   int64_t *words;          // words[2]: transcripts with a collision
};
// One lane per transcript: its members come sorted by (left, right)
__global__ __launch_bounds__(256) void gtf_merge_kernel(GtfMergeArgs a)
{
   for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.n_tx; t += (int64_t)gridDim.x * blockDim.x) {
      const uint32_t i0 = a.tx_first[t], i1 = a.tx_first[t + 1];
      const GtfRec f = a.rec[a.order[i0]];
      uint32_t first_rec = a.order[i0], first_line = f.line, n = 0, merges = 0;
      uint32_t cl = f.left, cr = f.right;
      bool collision = false;
      for (uint32_t i = i0 + 1; i < i1; ++i) {
         const uint32_t k = a.order[i];
         const GtfRec q = a.rec[k];
         collision |= !gtf_same_key(a.bytes, a.line_off, f, q);
         if (q.line < first_line) first_line = q.line, first_rec = k;
         if (gtf_exons_join(cr, q.left)) {
            cr = q.right > cr ? q.right : cr;
            ++merges;
         } else {
            a.xl[i0 + n] = cl, a.xr[i0 + n] = cr, ++n;
            cl = q.left, cr = q.right;
         }
      }
      a.xl[i0 + n] = cl, a.xr[i0 + n] = cr, ++n;
      const GtfRec h = a.rec[first_rec]; // the first line's: the gene and its name are this line's
      GtfTx o;
      o.h_chrom = h.h_chrom, o.name_at = 0;
      o.first_line = first_line, o.first_rec = first_rec, o.exon_at = i0, o.n_exons = n, o.merges = merges;
      o.strand = h.strand, o.l_chrom = h.l_chrom, o.l_gene = h.l_gene, o.l_tx = h.l_tx, o.l_gname = h.l_gname;
      o.collision = collision ? 1 : 0, o.pad[0] = o.pad[1] = 0;
      a.tx[t] = o;
      a.name_len[t] = (int32_t)h.l_chrom + (int32_t)h.l_gene + (int32_t)h.l_tx + (int32_t)h.l_gname;
      if (collision) atomicAdd((unsigned long long *)&a.words[2], 1ull);
   }
}

// One lane per transcript: its four names from its first line into the buffer, at name_at[t]
__global__ __launch_bounds__(256) void gtf_names_kernel(const uint8_t *bytes, const int64_t *line_off, const GtfRec *rec, GtfTx *tx, const int64_t *name_at,
                                                        int64_t n_tx, int64_t n_names, uint8_t *names)
{
   for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tx; t += (int64_t)gridDim.x * blockDim.x) {
      const GtfRec h = rec[tx[t].first_rec];
      const uint8_t *line = bytes + line_off[h.line];
      const int64_t at = name_at[t];
      tx[t].name_at = at;
      if (at < 0 || at + h.l_chrom + h.l_gene + h.l_tx + h.l_gname > n_names) continue;
      uint8_t *o = names + at;
      for (int i = 0; i < (int)h.l_chrom; ++i) *o++ = line[i];
      for (int i = 0; i < (int)h.l_gene; ++i) *o++ = line[h.o_gene + i];
      for (int i = 0; i < (int)h.l_tx; ++i) *o++ = line[h.o_tx + i];
      for (int i = 0; i < (int)h.l_gname; ++i) *o++ = line[h.o_gname + i];
   }
}

} // namespace sb
