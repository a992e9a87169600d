// strawberry_amd/csrc/fasta_host.h -- what the two forms of the FASTA reader share on the host (fasta_host.cpp, fasta_api.hip):
// the handle, and the step from what a form found per contig to what the handle answers -- the flags, the names, the lookup, the
// info words.  Free of HIP: a handle whose sequence is on a device carries the two functions that reach it.
#pragma once

#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sbgpu.h"

struct sbgpu_fasta {
   std::vector<int64_t> seq_off, offset, line_bases, line_width, name_off;
   std::vector<uint8_t> flags;
   std::string names;
   std::unordered_map<std::string, int64_t> by_lower; // a name, lower-cased -> its first contig
   std::vector<uint8_t> seq;  // host form: the packed sequence
   uint8_t *d_seq = nullptr;  // device form: the same in HBM, owned
   int device = -1;
   void (*dev_free)(uint8_t *d_seq, int device) = nullptr;
   int (*dev_fetch)(const uint8_t *d_src, int device, uint8_t *dst, int64_t n) = nullptr; // SBGPU_OK, or a recorded failure
   int64_t info[16] = {};
};

namespace sb {

// What a form found: per contig the name's bytes (names, name_off), offset, the first line's two lengths, seq_off [n + 1] and
// whether the index arithmetic fails (ragged: 0 / 1).  -> the handle's arrays, flags, lookup and info words; the sequence
// itself (seq or d_seq / device) is the caller's to set, before or after.
int fasta_finish(const std::string &who, int64_t n_bytes, int64_t n_lines, std::vector<int64_t> &&name_off, std::string &&names, std::vector<int64_t> &&offset,
                 std::vector<int64_t> &&line_bases, std::vector<int64_t> &&line_width, std::vector<int64_t> &&seq_off, const std::vector<uint8_t> &ragged,
                 sbgpu_fasta *g);
// the refusal of a non-empty line in front of the first header, at byte `at`
int fasta_fail_leading(const std::string &who, int64_t at);

} // namespace sb
