// strawberry_amd/csrc/gtf_schedule.h -- what the GTF reader's device form (gtf_api.hip, gtf_device.h) decides on the host, as
// data and free of HIP: a plain C++ compiler takes this header alone.  The kernels' thresholds, the tile counts, the launch
// shapes, which of a wave's tiles is staged, and the three arenas' layouts.  The launcher issues what these functions return
// and decides nothing of this itself; tests/test_gtf_reader_cpp.py states the rules a second time.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h> // (the qualifiers of what the kernels call too; a plain C++ compiler sees none of it)
#define SB_GTF_HD __host__ __device__ inline
#else
#define SB_GTF_HD inline
#endif
#include "stage_host.h"

namespace sb {

// ---- the thresholds (sbgpu_gtf_limits reports them in this order)
constexpr int64_t kGtfTileLines = 64;        // lines per tile of the parse: one lane each, a wave's pass
constexpr int64_t kGtfStageBytes = 24 * 1024; // the parse kernel's staging buffer (LDS): six workgroups fit a CU
constexpr int64_t kGtfStageSlack = 32;       // of it, not for lines: the window reads up to 15 bytes behind a line, the copy starts up to 15 in
constexpr int64_t kGtfStageLimit = kGtfStageBytes - kGtfStageSlack; // a tile of more bytes than this is walked in global memory
constexpr int64_t kGtfMaxLine = 65535;       // the longest line the device form takes, its "\r\n" not counted (a record keeps its names' places in 16 bits)
constexpr int64_t kGtfScanTile = 1024;       // entries per round of the tile scan (one workgroup: 256 threads, four each)
constexpr int64_t kGtfIndexTile = 16 * 1024; // bytes per tile of the line index: a wave's sixteen rounds of 64 x 16 bytes
constexpr int64_t kGtfGridCap = 2048;        // workgroups of a kernel that strides over tiles
constexpr int64_t kGtfMaxLines = ((int64_t)1 << 31) - 2; // a record keeps its line in 32 bits
constexpr size_t kGtfRecBytes = 48, kGtfTxBytes = 48;    // sizeof(GtfRec), sizeof(GtfTx): gtf_device.h

inline int64_t gtf_index_tiles(int64_t n_bytes) { return (n_bytes + kGtfIndexTile - 1) / kGtfIndexTile; }
inline int64_t gtf_parse_tiles(int64_t n_lines) { return (n_lines + kGtfTileLines - 1) / kGtfTileLines; }
// a kernel that strides over `tiles` tiles, one per workgroup and round
inline unsigned gtf_grid(int64_t tiles) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, kGtfGridCap)); }
// a kernel with one thread per entry, 256 per workgroup, striding beyond the cap
inline unsigned gtf_grid256(int64_t n) { return gtf_grid((n + 255) / 256); }
// the tile of lines whose bytes are [s0, s1) is copied to LDS; otherwise its lanes walk global memory (gtf_parse_kernel asks here)
SB_GTF_HD bool gtf_tile_staged(int64_t s0, int64_t s1) { return s1 >= s0 && s1 - s0 <= kGtfStageLimit; }
// a line of `len` bytes -- neither its '\n' nor the one '\r' in front of it counted -- is one the device form takes
SB_GTF_HD bool gtf_line_fits(int64_t len) { return len <= kGtfMaxLine; }
// the lines of a file of n_bytes bytes with `newlines` '\n' whose last byte is `last`: one more where the last line has none
inline int64_t gtf_line_count(int64_t n_bytes, int64_t newlines, int last) { return newlines + (n_bytes > 0 && last != '\n' ? 1 : 0); }
// the transcript key's hash as the sorts see it: its low `hash_bits` bits (0: all 64)
inline unsigned gtf_hash_bits(int32_t hash_bits) { return hash_bits <= 0 || hash_bits > 64 ? 64u : (unsigned)hash_bits; }

// ---- the line index' arena: the tiles' newline counts, their scan, the words read back
struct GtfIndexLayout {
   int64_t tiles;
   size_t cnt, at, words, bytes; // cnt: int32 [tiles]; at: int64 [tiles + 1]; words: int64 [4] (0: newlines, 1: the last byte)
   size_t words_bytes;
};
inline GtfIndexLayout gtf_index_layout(int64_t n_bytes)
{
   Arena a;
   GtfIndexLayout L;
   L.tiles = gtf_index_tiles(n_bytes);
   L.cnt = a.take_nonempty((size_t)L.tiles * 4), L.at = a.take_nonempty(((size_t)L.tiles + 1) * 8);
   L.words_bytes = 4 * 8;
   L.words = a.take(L.words_bytes);
   L.bytes = a.size;
   return L;
}

// ---- the parse's arena: the lines' offsets and statuses, a record per line, the tiles' accepted lines and their scan, the counts
struct GtfParseLayout {
   int64_t tiles;
   size_t line_off, status, rec, cnt, at, counts, bytes; // line_off: int64 [lines + 1]; status: u8 [lines]; rec: GtfRec [lines];
   size_t counts_bytes;                                   // cnt: int32 [tiles]; at: int64 [tiles + 1]; counts: u64 [16], zeroed
};
inline GtfParseLayout gtf_parse_layout(int64_t n_lines)
{
   Arena a;
   GtfParseLayout L;
   const size_t n = (size_t)n_lines;
   L.tiles = gtf_parse_tiles(n_lines);
   L.line_off = a.take((n + 1) * 8), L.status = a.take_nonempty(n), L.rec = a.take_nonempty(n * kGtfRecBytes);
   L.cnt = a.take_nonempty((size_t)L.tiles * 4), L.at = a.take_nonempty(((size_t)L.tiles + 1) * 8);
   L.counts_bytes = 16 * 8;
   L.counts = a.take(L.counts_bytes);
   L.bytes = a.size;
   return L;
}

// ---- the grouping's arena, for m accepted lines: the records in line order, two sorts' keys and values (both ways), the
// transcripts' heads, the merged exons in place, a row per transcript (at most m), the words read back, rocPRIM's scratch
struct GtfGroupLayout {
   size_t rec, key_a, key_b, val_a, val_b, head, seg, tx_first, xl, xr, tx, name_len, name_at, words, tmp, bytes;
   size_t words_bytes; // int64 [4], zeroed: 0 transcripts, 1 the names' bytes, 2 collisions
};
inline GtfGroupLayout gtf_group_layout(int64_t m, size_t tmp_bytes)
{
   Arena a;
   GtfGroupLayout L;
   const size_t n = (size_t)m;
   L.rec = a.take_nonempty(n * kGtfRecBytes);
   L.key_a = a.take_nonempty(n * 8), L.key_b = a.take_nonempty(n * 8), L.val_a = a.take_nonempty(n * 4), L.val_b = a.take_nonempty(n * 4);
   L.head = a.take_nonempty(n), L.seg = a.take_nonempty(n * 4), L.tx_first = a.take_nonempty((n + 1) * 4);
   L.xl = a.take_nonempty(n * 4), L.xr = a.take_nonempty(n * 4), L.tx = a.take_nonempty(n * kGtfTxBytes);
   L.name_len = a.take_nonempty(n * 4), L.name_at = a.take_nonempty((n + 1) * 8);
   L.words_bytes = 4 * 8;
   L.words = a.take(L.words_bytes), L.tmp = a.take_nonempty(tmp_bytes);
   L.bytes = a.size;
   return L;
}

} // namespace sb
