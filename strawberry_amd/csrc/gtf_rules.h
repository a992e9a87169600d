// strawberry_amd/csrc/gtf_rules.h -- the GTF reader's rule for ONE LINE (include/sbgpu.h, sbgpu_gtf_*), stated once: the host
// form (gtf_host.cpp) and the parse kernel (gtf_device.h) both call gtf_parse_line.  Free of HIP under a plain C++ compiler (g++ takes it alone).
//
// A restatement, on flat bytes, of what GffLine::GffLine and GffLine::extractAttr decide (/root/reference/src/gff.cpp:13-232) and
// of the two tests GffReader::nextGffLine makes in front of them (:460-462).  Where this rule leaves the reference, the line says so:
//   - :83-93    the reference copies the line twice and cuts it in place; here the line is walked once, eight bytes per load, and
//               nothing is written.  A NUL is a byte like any other (the reference's C strings end at it).
//   - :123,129  atol: here a coordinate is the field's leading run of ASCII digits (no blanks, no sign), 1 .. 2^31 - 1.
//   - :139-148  the score column is NOT read.  The reference's `return` at :147 stands outside its `if`, so a line with a
//               numeric score never becomes a feature there; here it does.
//   - :159-166  the type is the whole of column 3 lower-cased (the reference looks at its first 127 bytes).
//   - :191-193  `ID=` / `Parent=` are not looked for: a GFF3 line has no transcript_id and ends as NO_TRANSCRIPT.
//   - :220-222  every key is looked up in the column's ORIGINAL text; the reference deletes an attribute it found before it
//               looks for the next one (:71-77), so there a key inside a deleted value can no longer be found.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h> // (the qualifiers; a plain C++ compiler sees none of it)
#endif
#include <stdint.h>

#ifndef SB_HD
#ifdef __HIPCC__
#define SB_HD __host__ __device__ __forceinline__
#else
#define SB_HD inline
#endif
#endif

namespace sb {

// a line's status (include/sbgpu.h: SBGPU_GTF_*); the last two never reach a caller: a call that meets one is refused
constexpr int kGtfOk = 0, kGtfSkip = 1, kGtfFields = 2, kGtfOther = 3, kGtfCoord = 4, kGtfNoTranscript = 5, kGtfNoGene = 6;
constexpr int kGtfNameLong = 7, kGtfLineLong = 8, kGtfStatuses = 9;
constexpr int kGtfMaxName = 255;                          // bytes of a chromosome, gene or transcript name
constexpr uint64_t kGtfFnvBasis = 0xcbf29ce484222325ull;  // 64-bit FNV-1a
constexpr uint64_t kGtfCoordMax = 0x7fffffffull;

// What a line says.  Offsets are from the line's first byte; the chromosome name begins there.  The hashes: h_chrom over the
// lower-cased chromosome name, h_tx over (that name, the strand, the transcript_id bytes) -- a transcript's key --, h_gene over
// (that name, the gene_id bytes).
struct GtfLine {
   uint64_t h_tx, h_gene, h_chrom;
   int64_t o_gene, o_tx, o_gname;
   int64_t l_chrom, l_gene, l_tx, l_gname;
   uint32_t left, right;
   uint8_t status, strand;
};

// bytes p .. p + 7 as a little-endian word, nothing at or beyond `end` read (the host, and lines walked in global memory)
struct GtfBytes {
   SB_HD uint64_t peek8(const uint8_t *p, const uint8_t *end) const
   {
      uint64_t w = 0;
      for (int i = 0; i < 8; ++i)
         if (p + i < end) w |= (uint64_t)p[i] << (8 * i);
      return w;
   }
};

SB_HD uint32_t gtf_lower(uint32_t c) { return c - (uint32_t)'A' < 26u ? c + 32u : c; }
SB_HD bool gtf_isspace(uint32_t c) { return c == (uint32_t)' ' || c - 9u < 5u; } // isspace in the C locale: blank, \t \n \v \f \r
SB_HD uint64_t gtf_fnv(uint64_t h, uint32_t c) { return (h ^ (uint64_t)c) * 1099511628211ull; }
// the hashes' starts behind the chromosome name: the strand (a word no byte can be) opens the transcript's, another the gene's
SB_HD uint64_t gtf_tx_hash_start(uint64_t h_chrom, uint32_t strand) { return gtf_fnv(h_chrom, 0x100u + strand); }
SB_HD uint64_t gtf_gene_hash_start(uint64_t h_chrom) { return gtf_fnv(h_chrom, 0x1ffu); }

// One attribute of column 9 as GffLine::extractAttr finds it (:13-69).  state: 0 the key is looked for, 1 found and the blanks
// behind it are passed over, 2 inside a bare value, 3 inside a quoted value, 4 done.
struct GtfAttr {
   int64_t off, len;
   uint64_t hash;
   int state;
};
constexpr uint32_t kGtfEnd = 0x100u; // the column's end, as a byte behind its last
// the value's part of the walk: byte `c` at offset `i` of the line
SB_HD void gtf_attr_value(GtfAttr &a, uint32_t c, int64_t i)
{
   if (a.state == 1) {
      if (c == (uint32_t)' ') return;                               // :52
      if (c == (uint32_t)'"') a.state = 3, a.off = i + 1;           // :56-59
      else if (c == (uint32_t)';' || c == kGtfEnd) a.state = 4, a.off = i; // :53 (the reference complains and goes on with an empty value)
      else a.state = 2, a.off = i, a.len = 1, a.hash = gtf_fnv(a.hash, c);
   } else if (a.state == 2) {
      if (c == (uint32_t)';' || c == kGtfEnd) a.state = 4;          // :66
      else ++a.len, a.hash = gtf_fnv(a.hash, c);
   } else if (a.state == 3) {
      if (c == (uint32_t)'"' || c == (uint32_t)';' || c == kGtfEnd) a.state = 4; // :63
      else ++a.len, a.hash = gtf_fnv(a.hash, c);
   }
}
// the key `found` just in front of byte `c` (a blank or the column's end, :37): its value begins behind it
SB_HD void gtf_attr_found(GtfAttr &a, uint32_t c, int64_t i)
{
   a.state = c == kGtfEnd ? 4 : 1;
   a.off = i;
}

// The line `line[0, len)`: `len` counts neither the '\n' that ends it nor -- the caller has taken it off -- the one '\r' in front.
// rd.peek8(p, end) reads eight bytes at p (GtfBytes; the kernel's staged lines: GtfWindow).
template <class RD>
SB_HD void gtf_parse_line(RD &rd, const uint8_t *line, int64_t len, GtfLine &out)
{
   out.h_tx = out.h_gene = 0, out.h_chrom = kGtfFnvBasis;
   out.o_gene = out.o_tx = out.o_gname = 0, out.l_chrom = out.l_gene = out.l_tx = out.l_gname = 0;
   out.left = out.right = 0, out.strand = 0, out.status = kGtfSkip;
   if (len < 10) return; // :462
   const uint8_t *end = line + len;
   int col = 0;                           // tabs so far, at most 8 (:105-113)
   bool lead = true, comment = false;     // :460-462
   bool typed = true;                     // column 3 is an exon's
   uint32_t t3 = 0;                       // column 3's last four bytes, lower-cased
   bool has_utr = false, has_exon = false;
   uint64_t v4 = 0, v5 = 0;               // columns 4 and 5: the leading run of digits
   int nd4 = 0, nd5 = 0;
   bool run4 = true, run5 = true, first7 = true;
   // column 9: the last sixteen bytes lower-cased (w0: the last eight, the newest lowest), their count, inside a quoted text
   uint64_t w0 = 0, w1 = 0;
   int64_t cnt = 0;
   bool in_str = false;
   GtfAttr gene = {0, 0, 0, 0}, tx = {0, 0, 0, 0}, gname = {0, 0, 0, 0};
   // the keys, as the window shows them: "gene_id" (7), "transcript_id" (13: "trans" + "cript_id"), "gene_name" (9: "g" + "ene_name")
   constexpr uint64_t kGeneId = 0x67656e655f6964ull, kCriptId = 0x63726970745f6964ull, kTrans = 0x7472616e73ull, kEneName = 0x656e655f6e616d65ull;
   auto attr_byte = [&](uint32_t c, int64_t i) {
      gtf_attr_value(gene, c, i), gtf_attr_value(tx, c, i), gtf_attr_value(gname, c, i);
      // :32-37 a key matches outside quotes, at the column's start or behind ' ' or ';', its bytes compared without case, and a
      // blank or the column's end behind it
      if (!in_str && (c == (uint32_t)' ' || c == kGtfEnd)) {
         auto front = [](uint32_t p) { return p == (uint32_t)' ' || p == (uint32_t)';'; };
         if (gene.state == 0 && (w0 & 0x00ffffffffffffffull) == kGeneId && (cnt == 7 || (cnt > 7 && front((uint32_t)(w0 >> 56))))) gtf_attr_found(gene, c, i);
         if (tx.state == 0 && w0 == kCriptId && (w1 & 0xffffffffffull) == kTrans && (cnt == 13 || (cnt > 13 && front((uint32_t)(w1 >> 40) & 0xffu)))) gtf_attr_found(tx, c, i);
         if (gname.state == 0 && w0 == kEneName && (w1 & 0xffu) == (uint32_t)'g' && (cnt == 9 || (cnt > 9 && front((uint32_t)(w1 >> 8) & 0xffu)))) gtf_attr_found(gname, c, i);
      }
      if (c == (uint32_t)'"') in_str = !in_str; // :26-31
      w1 = (w1 << 8) | (w0 >> 56), w0 = (w0 << 8) | (uint64_t)gtf_lower(c & 0xffu);
      ++cnt;
   };
   // (a line whose type is not an exon's is not read beyond its eighth tab -- once its first byte that is no blank has been seen)
   for (int64_t k = 0; k < len && (typed || lead) && !comment; k += 8) {
      uint64_t w = rd.peek8(line + k, end);
      const int nb = len - k < 8 ? (int)(len - k) : 8;
      for (int j = 0; j < nb; ++j, w >>= 8) {
         const uint32_t c = (uint32_t)w & 0xffu;
         if (lead && !gtf_isspace(c)) lead = false, comment = c == (uint32_t)'#';
         if (comment) break; // (SKIP: nothing more of the line matters)
         if (!typed) {
            if (!lead) break;
         } else if (col == 8) {
            attr_byte(c, k + j);
         } else if (c == (uint32_t)'\t') {
            if (++col == 8) {
               typed = has_exon && !has_utr; // :162-166: "utr" first, then "exon"
               gene.hash = gtf_gene_hash_start(out.h_chrom), tx.hash = gtf_tx_hash_start(out.h_chrom, out.strand);
            }
         } else if (col == 0) {
            out.h_chrom = gtf_fnv(out.h_chrom, gtf_lower(c)), ++out.l_chrom; // :117-118
         } else if (col == 2) {
            t3 = (t3 << 8) | gtf_lower(c);
            has_utr |= (t3 & 0xffffffu) == 0x757472u, has_exon |= t3 == 0x65786f6eu;
         } else if (col == 3) {
            if (run4 && c - (uint32_t)'0' < 10u) v4 = v4 * 10 + (c - (uint32_t)'0'), v4 = v4 > 0xffffffffull ? 0xffffffffull : v4, ++nd4;
            else run4 = false;
         } else if (col == 4) {
            if (run5 && c - (uint32_t)'0' < 10u) v5 = v5 * 10 + (c - (uint32_t)'0'), v5 = v5 > 0xffffffffull ? 0xffffffffull : v5, ++nd5;
            else run5 = false;
         } else if (col == 6) {
            if (first7) out.strand = c == (uint32_t)'+' ? 1 : (c == (uint32_t)'-' ? 2 : 0), first7 = false; // :149-156
         }
      }
   }
   if (comment) return; // (SKIP)
   if (col < 8) {       // :114
      out.status = kGtfFields;
      return;
   }
   if (!typed) {
      out.status = kGtfOther;
      return;
   }
   attr_byte(kGtfEnd, len);
   if (nd4 == 0 || nd5 == 0 || v4 < 1 || v5 < 1 || v4 > kGtfCoordMax || v5 > kGtfCoordMax) { // :124-133
      out.status = kGtfCoord;
      return;
   }
   out.left = (uint32_t)(v4 < v5 ? v4 : v5), out.right = (uint32_t)(v4 < v5 ? v5 : v4); // :134-138
   if (tx.len == 0) {
      out.status = kGtfNoTranscript;
      return;
   }
   if (gene.len == 0) {
      out.status = kGtfNoGene;
      return;
   }
   out.o_gene = gene.off, out.l_gene = gene.len, out.h_gene = gene.hash;
   out.o_tx = tx.off, out.l_tx = tx.len, out.h_tx = tx.hash;
   out.o_gname = gname.off, out.l_gname = gname.len;
   const bool name_long = out.l_chrom > kGtfMaxName || out.l_gene > kGtfMaxName || out.l_tx > kGtfMaxName || out.l_gname > kGtfMaxName;
   out.status = name_long ? kGtfNameLong : kGtfOk;
}

// the one '\r' in front of a line's '\n' is not the line's: its length without it
SB_HD int64_t gtf_line_len(const uint8_t *line, int64_t len) { return len > 0 && line[len - 1] == (uint8_t)'\r' ? len - 1 : len; }

// Exons of one transcript sorted by (left, right): `next` joins `prev` when it is equal to it, overlaps it or touches it
SB_HD bool gtf_exons_join(uint32_t prev_right, uint32_t next_left) { return (uint64_t)next_left <= (uint64_t)prev_right + 1u; }

} // namespace sb
