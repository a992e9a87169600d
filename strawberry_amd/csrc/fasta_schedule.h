// strawberry_amd/csrc/fasta_schedule.h -- what the FASTA reader's device form (fasta_api.hip, fasta_device.h) decides on the
// host, as data and free of HIP: a plain C++ compiler takes this header alone.  The thresholds, the tile counts, the launch
// shapes and the two arenas' layouts, every size in 64 bits: the headline input is 3.1e9 bytes.  The launcher issues what
// these functions return and decides nothing of this itself; tests/test_fasta_reader_cpp.py states the rules a second time.
#pragma once

#include "stage_host.h"

namespace sb {

// ---- the thresholds (sbgpu_fasta_limits reports them in this order)
constexpr int64_t kFastaTile = 16 * 1024;     // bytes per tile: a wave's sixteen rounds of 64 x 16 bytes
constexpr int64_t kFastaScanTile = 1024;      // entries per round of the scan (one workgroup: 256 threads, four each)
constexpr int64_t kFastaGridCap = 2048;       // workgroups of a kernel that strides over tiles (one wave, one tile a round)
constexpr int64_t kFastaMaxHeader = 65535;    // the longest header line the device form takes, '>' counted, its "\r\n" not
constexpr int64_t kFastaMaxContigs = (int64_t)1 << 24; // the most contigs the device form takes
constexpr int64_t kFastaWaveContigs = 4;      // contigs per workgroup of the header walk: a wave each

inline int64_t fasta_tiles(int64_t n_bytes) { return n_bytes <= 0 ? 0 : (n_bytes + kFastaTile - 1) / kFastaTile; }
// a kernel that strides over `tiles` tiles, one per workgroup and round
inline unsigned fasta_grid(int64_t tiles) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, kFastaGridCap)); }
// the header walk: a wave per contig, kFastaWaveContigs waves a workgroup, striding beyond the cap
inline unsigned fasta_grid_contigs(int64_t n_contigs) { return fasta_grid((n_contigs + kFastaWaveContigs - 1) / kFastaWaveContigs); }
// a kernel with one thread per contig, 256 per workgroup
inline unsigned fasta_grid256(int64_t n) { return fasta_grid((n + 255) / 256); }
// rounds of the one-workgroup scan over n entries
inline int64_t fasta_scan_rounds(int64_t n) { return n <= 0 ? 0 : (n + kFastaScanTile - 1) / kFastaScanTile; }
// a header line of `len` bytes -- '>' counted, neither its '\n' nor the one '\r' in front of it -- is one the device form takes
inline bool fasta_header_fits(int64_t len) { return len <= kFastaMaxHeader; }
inline bool fasta_contigs_fit(int64_t n_contigs) { return n_contigs <= kFastaMaxContigs; }
// the lines of a file of n_bytes bytes with `newlines` '\n' whose last byte is `last`: one more where the last line has none
inline int64_t fasta_line_count(int64_t n_bytes, int64_t newlines, int last) { return newlines + (n_bytes > 0 && last != '\n' ? 1 : 0); }

// ---- the tiles' arena: per tile its headers and its bases, their scans, the words read back.  O(tiles).
struct FastaTileLayout {
   int64_t tiles;
   size_t hdr_cnt, hdr_at, base_cnt, base_at, words, bytes; // *_cnt: int32 [tiles]; *_at: int64 [tiles + 1]
   size_t words_bytes;                                      // int64 [8], see fasta_device.h: kFastaWord*
};
inline FastaTileLayout fasta_tile_layout(int64_t n_bytes)
{
   Arena a;
   FastaTileLayout L;
   L.tiles = fasta_tiles(n_bytes);
   const size_t t = (size_t)L.tiles;
   L.hdr_cnt = a.take_nonempty(t * 4), L.hdr_at = a.take((t + 1) * 8);
   L.base_cnt = a.take_nonempty(t * 4), L.base_at = a.take((t + 1) * 8);
   L.words_bytes = 8 * 8;
   L.words = a.take(L.words_bytes);
   L.bytes = a.size;
   return L;
}

// ---- the contigs' arena.  O(contigs).  hdr_off, name_at and seq_off have one entry more than there are contigs.
struct FastaContigLayout {
   size_t hdr_off, offset, name_len, name_at, hdr_len, first_nl, line_bases, line_width, seq_off, first_odd, ragged, bytes;
   size_t mins, mins_bytes; // first_nl and first_odd stand behind each other: one fill sets both to "none"
};
inline FastaContigLayout fasta_contig_layout(int64_t n_contigs)
{
   Arena a;
   FastaContigLayout L;
   const size_t n = (size_t)n_contigs;
   L.hdr_off = a.take((n + 1) * 8), L.offset = a.take_nonempty(n * 8), L.name_len = a.take_nonempty(n * 4), L.name_at = a.take((n + 1) * 8);
   L.hdr_len = a.take_nonempty(n * 8);
   L.mins = a.size;
   L.first_nl = a.take_nonempty(n * 8), L.first_odd = a.take_nonempty(n * 8);
   L.mins_bytes = a.size - L.mins;
   L.line_bases = a.take_nonempty(n * 8), L.line_width = a.take_nonempty(n * 8), L.seq_off = a.take((n + 1) * 8);
   L.ragged = a.take_nonempty(n * 4);
   L.bytes = a.size;
   return L;
}

} // namespace sb
