// strawberry_amd/csrc/fasta_rules.h -- the FASTA reader's rule where both forms need it (include/sbgpu.h, sbgpu_fasta_*; DESIGN
// 3.33): the byte classes, the first line's two lengths, and the two tests on a byte's phase against the first line's width that
// say whether the index arithmetic holds for a contig.  __host__ __device__; a plain C++ compiler takes this header alone.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SB_FASTA_HD __host__ __device__ inline
#else
#define SB_FASTA_HD inline
#endif

namespace sb {

// the flags of a contig (SBGPU_FASTA_* of include/sbgpu.h)
constexpr uint8_t kFastaEmpty = 1, kFastaRagged = 2, kFastaDuplicate = 4, kFastaNoname = 8;

// C's isspace in the "C" locale: a contig's name ends in front of the first such byte
SB_FASTA_HD bool fasta_isspace(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
// the lookup's comparison: ASCII lower case
SB_FASTA_HD uint8_t fasta_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }
// byte `c` followed by `next` (-1: the buffer ends) belongs to a line's terminator, not to the line
SB_FASTA_HD bool fasta_is_term(uint8_t c, int next) { return c == '\n' || (c == '\r' && next == '\n'); }

// The first line behind a header.  offset: its first byte; end: where the contig's lines end (the next header, or the buffer's
// end); first_nl: the first '\n' at or behind offset (>= end: there is none); cr: the byte in front of that '\n' is a '\r' and
// is the line's own (first_nl - 1 >= offset).
SB_FASTA_HD void fasta_first_line(int64_t offset, int64_t end, int64_t first_nl, bool cr, int64_t *line_bases, int64_t *line_width)
{
   if (first_nl >= end) {
      *line_bases = *line_width = end - offset;
      return;
   }
   *line_width = first_nl + 1 - offset;
   *line_bases = first_nl - offset - (cr ? 1 : 0);
}

// A contig's bytes against its first line.  phase: (the byte's offset - the contig's offset) % line_width, line_width > 0.
//   - a base at a phase >= line_bases stands where a full line has its terminator: a line is longer than the first
//   - a '\n' ends a full line exactly when it stands at phase line_width - 1 and, where the first line ends in a bare '\n', has
//     no '\r' in front of it.  Any other '\n' is fine only as long as no base follows it in the contig.
SB_FASTA_HD bool fasta_base_out_of_phase(int64_t phase, int64_t line_bases) { return phase >= line_bases; }
SB_FASTA_HD bool fasta_line_end_odd(int64_t phase, int64_t line_bases, int64_t line_width, bool cr_in_front)
{
   return phase != line_width - 1 || (line_width == line_bases + 1 && cr_in_front);
}

} // namespace sb
