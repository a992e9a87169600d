"""The C++ side of the bin-table merge.
`sanitized`: csrc/merge_host.cpp itself -- it is free of HIP -- compiled by g++ with AddressSanitizer and UBSan into a stand-alone
program with its own main (which supplies the library's error slot), run over em_c3_400 against a second sample: the shapes and
the fill into exactly sized arrays, a duplicate key and a mismatch refused: clean, and the bytes of the Python binding's; the same
program states the offsets of the device form's arenas (csrc/stage_host.h: merge_match_layout, merge_layout).  No sanitizer is
used on anything loaded into Python.
`header`: include/sbgpu_host.hpp's DifferentialUsage::device_merged compiles as C++14."""
import os
import subprocess

import numpy as np
import pytest

import merge_util as MU
from test_bins_merge import pair
from test_isoform_info_cpp import LOAD, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SANITIZED = r"""#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "SBGPU_H"
#include "stage_host.h"
static std::string last_error;
namespace sb {
int api_fail(int code, const std::string &msg)
{
   last_error = msg;
   return code;
}
}
""" + LOAD + r"""
int main(int argc, char **argv)
{
   if (argc < 2) return 2;
   {  // the device form's arenas, written out by hand: every entry rounded up to 256 bytes
      const sb::MergeMatchLayout M = sb::merge_match_layout(40, 300, 70, 33, 9, 2);
      if (M.roff_a != 0 || M.roff_b != 512 || M.ioff != 1024 || M.foff_a != 1536 || M.foff_b != 2048 || M.small != 2560 || M.items != 2816) return 10;
      if (M.deep != 3072 || M.upload_bytes != 3328 || M.b_of_a != 3328 || M.b_only != 4608 || M.n_only != 5120 || M.bytes != 5376) return 11;
      const sb::MergeLayout L = sb::merge_layout(40, 350, 1000, 45);
      if (L.roff_u != 0 || L.foff_u != 512 || L.tiles != 1024 || L.upload_bytes != 1792 || L.row_a != 1792 || L.row_b != 3328) return 12;
      if (L.count_a != 4864 || L.count_b != 6400 || L.F_a != 7936 || L.F_b != 16128 || L.bytes != 24320) return 13;
      if (sizeof(sb::MergeItem) != 16 || sizeof(sb::MergeTile) != 16) return 14;
   }
   const std::string d = std::string(argv[1]) + "/";
   const auto iso_off = load<int64_t>(d + "iso_off"), row_a = load<int64_t>(d + "row_off_a"), row_b = load<int64_t>(d + "row_off_b");
   const auto key_a = load<uint32_t>(d + "key_a"), key_b = load<uint32_t>(d + "key_b");
   const auto count_a = load<int32_t>(d + "count_a"), count_b = load<int32_t>(d + "count_b");
   const auto F_a = load<double>(d + "F_a"), F_b = load<double>(d + "F_b"), X_a = load<double>(d + "X_a"), X_b = load<double>(d + "X_b");
   const int64_t n_loci = (int64_t)iso_off.size() - 1;
   const sbgpu_merge_sample_t a = {n_loci, iso_off.data(), row_a.data(), 2, 0, key_a.data(), count_a.data(), F_a.data(), X_a.data()};
   const sbgpu_merge_sample_t b = {n_loci, iso_off.data(), row_b.data(), 2, 0, key_b.data(), count_b.data(), F_b.data(), X_b.data()};
   int64_t sizes[2];
   if (sbgpu_bins_merge_shapes_host(&a, &b, sizes, nullptr, nullptr, nullptr, nullptr) != SBGPU_OK) return 3;
   // exactly sized: a write past an array's end is the sanitizer's to see
   std::vector<int64_t> row_off((size_t)n_loci + 1), f_off((size_t)n_loci + 1);
   std::vector<int32_t> ra((size_t)sizes[0]), rb((size_t)sizes[0]), ca((size_t)sizes[0]), cb((size_t)sizes[0]);
   std::vector<double> Fa((size_t)sizes[1]), Fb((size_t)sizes[1]);
   if (sbgpu_bins_merge_shapes_host(&a, &b, sizes, row_off.data(), f_off.data(), ra.data(), rb.data()) != SBGPU_OK) return 4;
   if (row_off.back() != sizes[0] || f_off.back() != sizes[1]) return 5;
   if (sbgpu_bins_merge_fill_host(&a, &b, ca.data(), cb.data(), Fa.data(), Fb.data()) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 6;
   }
   // refusals: a duplicate key in B's last locus with bins; another key width
   std::vector<uint32_t> dup = key_b;
   int64_t l = n_loci - 1;
   while (l >= 0 && row_b[(size_t)l + 1] - row_b[(size_t)l] < 2) --l;
   if (l < 0) return 7;
   dup[(size_t)row_b[(size_t)l] * 2] = dup[(size_t)row_b[(size_t)l] * 2 + 2], dup[(size_t)row_b[(size_t)l] * 2 + 1] = dup[(size_t)row_b[(size_t)l] * 2 + 3];
   sbgpu_merge_sample_t bad = b;
   bad.key = dup.data();
   if (sbgpu_bins_merge_shapes_host(&a, &bad, sizes, nullptr, nullptr, nullptr, nullptr) != SBGPU_EINVAL ||
       last_error.find("a duplicate bin key in locus " + std::to_string(l)) == std::string::npos) return 8;
   bad = b, bad.key_words = 1;
   if (sbgpu_bins_merge_fill_host(&a, &bad, ca.data(), cb.data(), nullptr, nullptr) != SBGPU_EINVAL || last_error.find("key_words") == std::string::npos) return 9;
   print_int("row_off", row_off), print_int("f_off", f_off), print_int("row_a", ra), print_int("row_b", rb), print_int("count_a", ca), print_int("count_b", cb);
   print("F_a", Fa), print("F_b", Fb);
   return 0;
}
"""

HEADER = r"""#include "sbgpu_host.hpp"
int main()
{
   auto f = &sbgpu::DifferentialUsage::device_merged;
   sbgpu::DifferentialUsage t;
   return f != nullptr && t.merged.n_bins == 0 && t.merged_row_off.empty() ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden):
    from strawberry_amd import _lib
    _lib.load()
    a, b = pair(golden, "em_c3_400", 2)
    d = tmp_path_factory.mktemp("merge_cpp")
    for name, x, dt in (("iso_off", a.iso_off, np.int64), ("row_off_a", a.row_off, np.int64), ("row_off_b", b.row_off, np.int64), ("key_a", a.key, np.uint32),
                        ("key_b", b.key, np.uint32), ("count_a", a.count, np.int32), ("count_b", b.count, np.int32), ("F_a", a.F, np.float64),
                        ("F_b", b.F, np.float64), ("X_a", a.X, np.float64), ("X_b", b.X, np.float64)):
        np.ascontiguousarray(x, dt).tofile(str(d / name))
    return dict(dir=d, a=a, b=b)


def test_the_host_form_alone_under_the_sanitizers(case):
    """csrc/merge_host.cpp needs neither HIP nor the library: g++ builds it with ASan and UBSan beside a main of its own"""
    from strawberry_amd import merge
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(SANITIZED.replace("SBGPU_H", os.path.join(ROOT, "include", "sbgpu.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, str(src), os.path.join(csrc, "merge_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    got = parse(out.stdout)
    t = merge.merge_host(case["a"], case["b"])
    MU.assert_same(t, MU.by_hand(case["a"], case["b"]))
    for k in ("row_off", "f_off") + merge.NAMES:
        x = getattr(t, k)
        vals = np.array([float.fromhex(v) for v in got.get(k, [])]) if x.dtype == np.float64 else np.array([int(v) for v in got.get(k, [])], x.dtype)
        assert vals.astype(x.dtype).tobytes() == x.tobytes(), k
    assert (t.row_a < 0).sum() > 100 and (t.row_b < 0).sum() > 100


def test_the_header_compiles_as_cpp14(tmp_path):
    src = tmp_path / "header.cpp"
    src.write_text(HEADER)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
