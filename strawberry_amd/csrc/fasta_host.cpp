// strawberry_amd/csrc/fasta_host.cpp -- sbgpu_fasta_read_host and what the handle answers (include/sbgpu.h, sbgpu_fasta_*): a
// FASTA file's bytes -> the contigs' names, the packed sequence, the five .fai columns and the flags.  The host form goes line
// by line; the step from a form's per-contig findings to the handle (fasta_finish) is the device form's too.  No kernels here,
// and nothing of HIP: a plain C++ compiler takes this file with fasta_rules.h, fasta_schedule.h and fasta_host.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "fasta_host.h"
#include "fasta_rules.h"
#include "fasta_schedule.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (api_internal.h; a stand-alone program over this file defines its own)

int fasta_fail_leading(const std::string &who, int64_t at)
{
   return api_fail(SBGPU_EINVAL, who + ": a non-empty line in front of the first header, at byte offset " + std::to_string(at));
}

static std::string lower_of(const char *p, int64_t n)
{
   std::string s((size_t)n, '\0');
   for (int64_t i = 0; i < n; ++i) s[(size_t)i] = (char)fasta_lower((uint8_t)p[i]);
   return s;
}

int fasta_finish(const std::string &who, int64_t n_bytes, int64_t n_lines, std::vector<int64_t> &&name_off, std::string &&names, std::vector<int64_t> &&offset,
                 std::vector<int64_t> &&line_bases, std::vector<int64_t> &&line_width, std::vector<int64_t> &&seq_off, const std::vector<uint8_t> &ragged,
                 sbgpu_fasta *g)
{
   const size_t n = offset.size();
   if (name_off.size() != n + 1 || seq_off.size() != n + 1 || line_bases.size() != n || line_width.size() != n || ragged.size() != n ||
       name_off[0] != 0 || name_off[n] != (int64_t)names.size() || seq_off[0] != 0)
      return api_fail(SBGPU_EHIP, who + ": the contigs' arrays disagree");
   g->name_off = std::move(name_off), g->names = std::move(names), g->offset = std::move(offset);
   g->line_bases = std::move(line_bases), g->line_width = std::move(line_width), g->seq_off = std::move(seq_off);
   g->flags.assign(n, 0);
   int64_t *info = g->info;
   std::fill(info, info + 16, (int64_t)0);
   info[0] = n_bytes, info[1] = n_lines, info[2] = (int64_t)n, info[3] = g->seq_off[n], info[9] = -1, info[11] = -1;
   for (size_t c = 0; c < n; ++c) {
      const int64_t len = g->seq_off[c + 1] - g->seq_off[c], l_name = g->name_off[c + 1] - g->name_off[c];
      if (len < 0 || l_name < 0 || g->offset[c] < 0 || g->offset[c] > n_bytes) return api_fail(SBGPU_EHIP, who + ": a contig's row points outside the file");
      uint8_t f = 0;
      if (len == 0) {
         f |= kFastaEmpty;
         g->line_bases[c] = g->line_width[c] = 0;
      } else if (ragged[c]) {
         f |= kFastaRagged;
      }
      if (l_name == 0) f |= kFastaNoname;
      if (!g->by_lower.emplace(lower_of(g->names.data() + g->name_off[c], l_name), (int64_t)c).second) f |= kFastaDuplicate;
      g->flags[c] = f;
      info[4] += (f & kFastaEmpty) != 0, info[5] += (f & kFastaRagged) != 0, info[6] += (f & kFastaDuplicate) != 0, info[7] += (f & kFastaNoname) != 0;
      if (info[9] < 0 || len > info[8]) info[8] = len, info[9] = (int64_t)c;
   }
   return SBGPU_OK;
}

namespace {

int read_host(const uint8_t *bytes, int64_t n_bytes, sbgpu_fasta *g)
{
   const std::string who = "sbgpu_fasta_read_host";
   std::vector<int64_t> name_off(1, 0), offset, line_bases, line_width, seq_off;
   std::vector<uint8_t> ragged;
   std::string names;
   std::vector<uint8_t> &seq = g->seq;
   int64_t n_lines = 0, pos = 0;
   // the contig being read: whether its first line is still to come, that line's terminator bytes, and whether a short or an
   // empty line has been seen, behind which only empty lines may stand
   bool first = false, tail = false;
   int64_t first_term = 0;
   while (pos < n_bytes) {
      const uint8_t *nl = (const uint8_t *)std::memchr(bytes + pos, '\n', (size_t)(n_bytes - pos));
      const int64_t le = nl ? nl - bytes : n_bytes, next = nl ? le + 1 : n_bytes;
      int64_t ce = le, term = nl ? 1 : 0;
      if (nl && le > pos && bytes[le - 1] == '\r') ce = le - 1, term = 2;
      const int64_t len = ce - pos;
      ++n_lines;
      if (len > 0 && bytes[pos] == '>') {
         int64_t e = pos + 1;
         while (e < ce && !fasta_isspace(bytes[e])) ++e;
         names.append((const char *)bytes + pos + 1, (size_t)(e - pos - 1));
         name_off.push_back((int64_t)names.size());
         offset.push_back(next), line_bases.push_back(0), line_width.push_back(0), ragged.push_back(0);
         seq_off.push_back((int64_t)seq.size());
         first = true, tail = false;
      } else if (offset.empty()) {
         if (len > 0) return fasta_fail_leading(who, pos);
      } else {
         int64_t &lb = line_bases.back(), &lw = line_width.back();
         if (first) {
            lb = len, lw = len + term, first_term = term, first = false;
         } else if (!tail && len == lb && term == first_term) {
            // a full line
         } else if (!tail && len <= lb) {
            tail = true; // the one short line, or the first empty one
         } else if (len > 0) {
            ragged.back() = 1;
         }
         if (len > 0) {
            if (seq.capacity() < seq.size() + (size_t)len) seq.reserve(std::max<size_t>((size_t)n_bytes, seq.size() + (size_t)len));
            seq.insert(seq.end(), bytes + pos, bytes + ce);
         }
      }
      pos = next;
   }
   seq_off.push_back((int64_t)seq.size());
   if (offset.empty()) seq_off.assign(1, 0);
   return fasta_finish(who, n_bytes, n_lines, std::move(name_off), std::move(names), std::move(offset), std::move(line_bases), std::move(line_width),
                       std::move(seq_off), ragged, g);
}

} // namespace
} // namespace sb

using sb::api_fail;

extern "C" {

int sbgpu_fasta_read_host(const uint8_t *bytes, int64_t n_bytes, sbgpu_fasta_t **out)
{
   if (!out || n_bytes < 0 || (n_bytes && !bytes)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_read_host: bad argument");
   *out = nullptr;
   try {
      std::unique_ptr<sbgpu_fasta> g(new sbgpu_fasta());
      if (const int rc = sb::read_host(bytes, n_bytes, g.get())) return rc;
      g->seq.shrink_to_fit();
      *out = g.release();
   } catch (const std::bad_alloc &) {
      return api_fail(SBGPU_ENOMEM, "sbgpu_fasta_read_host: out of memory");
   } catch (const std::exception &e) { // (std::length_error of a container: nothing C++ crosses the C ABI)
      return api_fail(SBGPU_ENOMEM, std::string("sbgpu_fasta_read_host: ") + e.what());
   }
   return SBGPU_OK;
}

void sbgpu_fasta_destroy(sbgpu_fasta_t *g)
{
   if (!g) return;
   if (g->d_seq && g->dev_free) g->dev_free(g->d_seq, g->device);
   delete g;
}

int sbgpu_fasta_info(const sbgpu_fasta_t *g, int64_t info[16])
{
   if (!g || !info) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_info: null argument");
   for (int k = 0; k < 16; ++k) info[k] = g->info[k];
   return SBGPU_OK;
}

int sbgpu_fasta_index(const sbgpu_fasta_t *g, const int64_t **seq_off, const int64_t **offset, const int64_t **line_bases, const int64_t **line_width,
                      const uint8_t **flags)
{
   if (!g) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_index: null handle");
   if (seq_off) *seq_off = g->seq_off.data();
   if (offset) *offset = g->offset.data();
   if (line_bases) *line_bases = g->line_bases.data();
   if (line_width) *line_width = g->line_width.data();
   if (flags) *flags = g->flags.data();
   return SBGPU_OK;
}

int sbgpu_fasta_names(const sbgpu_fasta_t *g, const int64_t **name_off, const char **names)
{
   if (!g) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_names: null handle");
   if (name_off) *name_off = g->name_off.data();
   if (names) *names = g->names.data();
   return SBGPU_OK;
}

int sbgpu_fasta_sequence(const sbgpu_fasta_t *g, const uint8_t **seq, int32_t *on_device)
{
   if (!g) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_sequence: null handle");
   if (seq) *seq = g->d_seq ? g->d_seq : g->seq.data();
   if (on_device) *on_device = g->d_seq ? 1 : 0;
   return SBGPU_OK;
}

int sbgpu_fasta_find(const sbgpu_fasta_t *g, const char *name, int64_t name_len, int64_t *contig)
{
   if (!g || !contig || name_len < 0 || (name_len && !name)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_find: bad argument");
   try {
      const auto it = g->by_lower.find(sb::lower_of(name, name_len));
      *contig = it == g->by_lower.end() ? -1 : it->second;
   } catch (const std::exception &) {
      return api_fail(SBGPU_ENOMEM, "sbgpu_fasta_find: out of memory");
   }
   return SBGPU_OK;
}

int sbgpu_fasta_fai(const sbgpu_fasta_t *g, char *buf, int64_t cap, int64_t *need)
{
   if (!g || (!buf && !need) || cap < 0) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_fai: bad argument");
   try {
      std::string text;
      for (size_t c = 0; c < g->flags.size(); ++c) {
         const uint8_t f = g->flags[c];
         if (f & sb::kFastaEmpty) continue;
         const std::string name(g->names.data() + g->name_off[c], (size_t)(g->name_off[c + 1] - g->name_off[c]));
         if (f & (sb::kFastaRagged | sb::kFastaNoname))
            return api_fail(SBGPU_EUNSUPPORTED, "sbgpu_fasta_fai: contig " + std::to_string(c) + " '" + name + "' " +
                                                    (f & sb::kFastaNoname ? "has no name" : "has lines of unequal length: an index cannot locate its bases"));
         text += name + "\t" + std::to_string(g->seq_off[c + 1] - g->seq_off[c]) + "\t" + std::to_string(g->offset[c]) + "\t" + std::to_string(g->line_bases[c]) +
                 "\t" + std::to_string(g->line_width[c]) + "\n";
      }
      if (need) *need = (int64_t)text.size();
      if (buf) {
         if (cap < (int64_t)text.size()) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_fai: the buffer is too small");
         std::memcpy(buf, text.data(), text.size());
      }
   } catch (const std::exception &) {
      return api_fail(SBGPU_ENOMEM, "sbgpu_fasta_fai: out of memory");
   }
   return SBGPU_OK;
}

int sbgpu_fasta_fetch(const sbgpu_fasta_t *g, int64_t contig, int64_t start, int64_t len, uint8_t *out)
{
   if (!g || contig < 0 || contig >= (int64_t)g->flags.size() || len < 0 || (len && !out)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_fetch: bad argument");
   const int64_t clen = g->seq_off[(size_t)contig + 1] - g->seq_off[(size_t)contig];
   if (start < 1 || start - 1 > clen || len > clen - (start - 1)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_fetch: the window lies outside the contig");
   if (len == 0) return SBGPU_OK;
   const int64_t at = g->seq_off[(size_t)contig] + start - 1;
   if (g->d_seq) return g->dev_fetch ? g->dev_fetch(g->d_seq + at, g->device, out, len) : api_fail(SBGPU_EINVAL, "sbgpu_fasta_fetch: the handle cannot reach its device");
   std::memcpy(out, g->seq.data() + at, (size_t)len);
   return SBGPU_OK;
}

int sbgpu_fasta_limits(int64_t limits[8])
{
   if (!limits) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_limits: null argument");
   limits[0] = sb::kFastaTile, limits[1] = sb::kFastaScanTile, limits[2] = sb::kFastaGridCap, limits[3] = sb::kFastaMaxHeader, limits[4] = sb::kFastaMaxContigs;
   limits[5] = limits[6] = limits[7] = 0;
   return SBGPU_OK;
}

} // extern "C"
