"""The C++ side of the differential isoform usage.
`sanitized`: csrc/diff_host.cpp itself -- it is free of HIP -- compiled by g++ with AddressSanitizer and UBSan into a stand-alone
program with its own main (which supplies the library's error slot), run over em_c3_400 against a second sample with two filters:
the shapes, the expansion and the statistics of a made-up solve into exactly sized arrays: clean, and the bytes of the Python
binding's; the same program states the offsets of the device form's arenas (csrc/stage_host.h: diff_layout, diff_chunk_layout).
No sanitizer is used on anything loaded into Python.
`device`: a C++14 program over include/sbgpu_host.hpp: sbgpu::DifferentialUsage::device on the same batches -- the bytes of
diff.em_diff_device on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import diff_util as DU
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
      const sb::DiffLayout L = sb::diff_layout(40, 300, 70, 1000);
      if (L.lstat != 0 || L.rank != 256 || L.first != 1536 || L.koff != 2048 || L.kcol != 2560 || L.upload_bytes != 3072) return 10;
      if (L.th_a != 3072 || L.th_b != 5632 || L.delta != 18432 || L.lr != 20992 || L.ll_a != 21504 || L.shift != 24576) return 11;
      if (L.dof != 25088 || L.status != 25344 || L.it_p != 27136 || L.sum_a != 27392 || L.sum_p != 28416 || L.chunk != 28928 || L.bytes != 29952) return 12;
      const sb::DiffChunkLayout M = sb::diff_chunk_layout(3, 2, 5, 70, 9, 100, 30, 700, 512);
      if (M.tiles != 0 || M.items != 256 || M.list != 512 || M.upload_bytes != 768 || M.alpha != 768 || M.count != 2048 || M.F != 2560) return 13;
      if (M.theta != 8192 || M.status != 8448 || M.iters != 8704 || M.x_theta != 8960 || M.x_status != 9216 || M.fit != 9472 || M.x_fit != 9984) return 14;
      if (M.bytes != 10496 || sizeof(sb::DiffTile) != 16 || sizeof(sb::DiffScaleItem) != 16) return 15;
   }
   const std::string d = std::string(argv[1]) + "/";
   const auto row_a = load<int64_t>(d + "row_off_a"), row_b = load<int64_t>(d + "row_off_b"), iso_off = load<int64_t>(d + "iso_off");
   const auto f_a = load<int64_t>(d + "f_off_a"), f_b = load<int64_t>(d + "f_off_b");
   const auto count_a = load<int32_t>(d + "count_a"), count_b = load<int32_t>(d + "count_b"), keep_a = load<int32_t>(d + "keep_a"), keep_b = load<int32_t>(d + "keep_b");
   const auto F_a = load<double>(d + "F_a"), F_b = load<double>(d + "F_b");
   const int64_t n_loci = (int64_t)iso_off.size() - 1, n_iso = iso_off.back();
   int64_t sizes[4];
   if (sbgpu_em_diff_shapes_host(n_loci, row_a.data(), row_b.data(), iso_off.data(), keep_a.data(), keep_b.data(), sizes, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr) != SBGPU_OK) return 3;
   // exactly sized: a write past an array's end is the sanitizer's to see
   std::vector<int32_t> diff_status((size_t)n_loci), sub_locus((size_t)sizes[0]), sub_kind((size_t)sizes[0]), sub_count((size_t)sizes[1]);
   std::vector<int64_t> sub_row_off((size_t)sizes[0] + 1), sub_iso_off((size_t)sizes[0] + 1), sub_f_off((size_t)sizes[0] + 1);
   std::vector<double> sub_F((size_t)sizes[3]);
   if (sbgpu_em_diff_shapes_host(n_loci, row_a.data(), row_b.data(), iso_off.data(), keep_a.data(), keep_b.data(), sizes, diff_status.data(), sub_locus.data(),
                                 sub_kind.data(), sub_row_off.data(), sub_iso_off.data(), sub_f_off.data()) != SBGPU_OK) return 4;
   if (sub_row_off.back() != sizes[1] || sub_iso_off.back() != sizes[2] || sub_f_off.back() != sizes[3]) return 5;
   const sbgpu_batch_t a = {n_loci, row_a.data(), iso_off.data(), f_a.data(), count_a.data(), F_a.data()};
   const sbgpu_batch_t b = {n_loci, row_b.data(), iso_off.data(), f_b.data(), count_b.data(), F_b.data()};
   if (sbgpu_em_diff_expand_host(&a, &b, keep_a.data(), keep_b.data(), sub_count.data(), sub_F.data()) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 6;
   }
   if (sbgpu_em_diff_expand_host(&a, &b, keep_a.data(), keep_b.data(), nullptr, sub_F.data()) != SBGPU_EINVAL || last_error.find("sub_count") == std::string::npos) return 7;
   // the statistics over a made-up solve and made-up fits: exactly sized outputs
   std::vector<double> theta((size_t)sizes[2]), ll((size_t)sizes[0]), llx((size_t)sizes[0]);
   std::vector<int32_t> status((size_t)sizes[0], 0), iters((size_t)sizes[0], 7);
   std::vector<int64_t> n_live((size_t)sizes[0], 9), n_dropped((size_t)sizes[0], 1), n_imp((size_t)sizes[0], 0);
   for (size_t i = 0; i < theta.size(); ++i) theta[i] = (double)(i % 13) + 0.5;
   for (size_t i = 0; i < ll.size(); ++i) ll[i] = -(double)(i % 7) - 1.25, llx[i] = ll[i] - (double)(i % 5) * 0.5, n_imp[i] = (int64_t)(i % 3), status[i] = i % 11 == 10 ? 2 : 0;
   std::vector<double> per_iso[7], per_locus[5];
   for (auto &v : per_iso) v.assign((size_t)n_iso, -1.0);
   for (auto &v : per_locus) v.assign((size_t)n_loci, -1.0);
   std::vector<int64_t> i64[3];
   for (auto &v : i64) v.assign((size_t)n_loci, -1);
   std::vector<int32_t> i32[9];
   for (auto &v : i32) v.assign((size_t)n_loci, -7);
   sbgpu_em_diff_t out = {};
   out.theta_a = per_iso[0].data(), out.theta_b = per_iso[1].data(), out.theta_pooled = per_iso[2].data(), out.usage_a = per_iso[3].data();
   out.usage_b = per_iso[4].data(), out.usage_pooled = per_iso[5].data(), out.delta_usage = per_iso[6].data();
   out.lr_stat = per_locus[0].data(), out.loglik_a = per_locus[1].data(), out.loglik_b = per_locus[2].data(), out.loglik_a_pooled = per_locus[3].data();
   out.loglik_b_pooled = per_locus[4].data();
   out.n_a = i64[0].data(), out.n_b = i64[1].data(), out.lost_shift = i64[2].data();
   out.dof = i32[0].data(), out.diff_status = i32[1].data(), out.top_iso = i32[2].data(), out.status_a = i32[3].data(), out.status_b = i32[4].data();
   out.status_pooled = i32[5].data(), out.iters_a = i32[6].data(), out.iters_b = i32[7].data(), out.iters_pooled = i32[8].data();
   if (sbgpu_em_diff_stat_host(&a, &b, keep_a.data(), keep_b.data(), theta.data(), status.data(), iters.data(), ll.data(), n_live.data(), n_dropped.data(),
                               n_imp.data(), llx.data(), n_dropped.data(), n_imp.data(), &out) != SBGPU_OK) return 9;
   print_int("diff_status", diff_status), print_int("sub_locus", sub_locus), print_int("sub_kind", sub_kind);
   print_int("row_off", sub_row_off), print_int("iso_off", sub_iso_off), print_int("f_off", sub_f_off);
   print_int("count", sub_count), print("F", sub_F);
   print("lr_stat", per_locus[0]), print("delta_usage", per_iso[6]), print_int("final_status", i32[1]), print_int("dof", i32[0]), print_int("top_iso", i32[2]);
   return 0;
}
"""

PROGRAM = r"""#include <hip/hip_runtime_api.h>
#include <cstring>
#include <fstream>
#include "sbgpu_host.hpp"
""" + LOAD + r"""
template <class T> const T *up(const std::vector<T> &v)
{
   void *p = nullptr;
   if (hipMalloc(&p, v.size() * sizeof(T) + 8) != hipSuccess || hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("upload");
   return (const T *)p;
}
int main(int argc, char **argv)
{
   if (argc < 2) return 2;
   const std::string d = std::string(argv[1]) + "/";
   const auto row_a = load<int64_t>(d + "row_off_a"), row_b = load<int64_t>(d + "row_off_b"), iso_off = load<int64_t>(d + "iso_off");
   const auto f_a = load<int64_t>(d + "f_off_a"), f_b = load<int64_t>(d + "f_off_b");
   const auto count_a = load<int32_t>(d + "count_a"), count_b = load<int32_t>(d + "count_b"), keep_a = load<int32_t>(d + "keep_a"), keep_b = load<int32_t>(d + "keep_b");
   const auto F_a = load<double>(d + "F_a"), F_b = load<double>(d + "F_b");
   const int64_t n_loci = (int64_t)iso_off.size() - 1;
   sbgpu::Context ctx(0);
   sbgpu_plan_t *pa = nullptr, *pb = nullptr;
   sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row_a.data(), iso_off.data(), f_a.data(), &pa), "sbgpu_plan_create");
   sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row_b.data(), iso_off.data(), f_b.data(), &pb), "sbgpu_plan_create");
   sbgpu::DifferentialUsage t = sbgpu::DifferentialUsage::device(ctx, pa, up(count_a), up(F_a), pb, up(count_b), up(F_b), up(keep_a), up(keep_b));
   if (!t.raw.d_lr_stat || !t.raw.d_theta_pooled || !t.raw.d_top_iso || t.raw.lr_stat) return 3;
   sbgpu_plan_destroy(pa), sbgpu_plan_destroy(pb);
   if ((int64_t)t.theta_a.size() != iso_off.back() || (int64_t)t.lr_stat.size() != n_loci) return 4;
   print("theta_a", t.theta_a), print("theta_b", t.theta_b), print("theta_pooled", t.theta_pooled), print("usage_a", t.usage_a), print("usage_b", t.usage_b);
   print("usage_pooled", t.usage_pooled), print("delta_usage", t.delta_usage), print("lr_stat", t.lr_stat), print("loglik_a", t.loglik_a);
   print("loglik_b", t.loglik_b), print("loglik_a_pooled", t.loglik_a_pooled), print("loglik_b_pooled", t.loglik_b_pooled);
   print_int("n_a", t.n_a), print_int("n_b", t.n_b), print_int("lost_shift", t.lost_shift), print_int("dof", t.dof), print_int("diff_status", t.diff_status);
   print_int("top_iso", t.top_iso), print_int("status_a", t.status_a), print_int("status_b", t.status_b), print_int("status_pooled", t.status_pooled);
   print_int("iters_a", t.iters_a), print_int("iters_b", t.iters_b), print_int("iters_pooled", t.iters_pooled);
   return 0;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden, oracle):
    from strawberry_amd import _lib
    _lib.load()
    a, _, _ = golden("em_c3_400")
    b = DU.second_sample(a, "subset", 4, oracle.em_batch(a.row_off, a.iso_off, a.f_off, a.count, a.F)[0])
    rng = np.random.default_rng(9)
    n_iso = int(a.iso_off[-1])
    keep_a, keep_b = (rng.random(n_iso) < 0.7).astype(np.int32), (rng.random(n_iso) < 0.7).astype(np.int32)
    d = tmp_path_factory.mktemp("diff_cpp")
    for name, x, dt in (("row_off_a", a.row_off, np.int64), ("row_off_b", b.row_off, np.int64), ("iso_off", a.iso_off, np.int64), ("f_off_a", a.f_off, np.int64),
                        ("f_off_b", b.f_off, np.int64), ("count_a", a.count, np.int32), ("count_b", b.count, np.int32), ("F_a", a.F, np.float64),
                        ("F_b", b.F, np.float64), ("keep_a", keep_a, np.int32), ("keep_b", keep_b, np.int32)):
        np.ascontiguousarray(x, dt).tofile(str(d / name))
    return dict(dir=d, a=a, b=b, keep_a=keep_a, keep_b=keep_b)


def values(got, k, like):
    if like.dtype == np.float64:
        return np.array([float.fromhex(x) for x in got.get(k, [])])
    return np.array([int(x) for x in got.get(k, [])], like.dtype)


def test_the_host_form_alone_under_the_sanitizers(case):
    """csrc/diff_host.cpp needs neither HIP nor the library: g++ builds it with ASan and UBSan beside a main of its own"""
    from strawberry_amd import diff
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(SANITIZED.replace("SBGPU_H", os.path.join(ROOT, "include", "sbgpu.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, str(src), os.path.join(csrc, "diff_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    got = parse(out.stdout)
    a, b, keep_a, keep_b = case["a"], case["b"], case["keep_a"], case["keep_b"]
    sh = diff.shapes_host(a.row_off, b.row_off, a.iso_off, keep_a, keep_b)
    count, F = diff.expand_host(a, b, keep_a, keep_b, sh)
    for k, x in list(sh.items()) + [("count", count), ("F", F)]:
        assert values(got, k, x).astype(x.dtype).tobytes() == x.tobytes(), k
    assert (sh["diff_status"] == diff.EMPTY).any() and (sh["diff_status"] == diff.SOLE).any() and (sh["diff_status"] == diff.OK).sum() > 100
    final = values(got, "final_status", sh["diff_status"])
    assert (final == diff.UNSOLVED).any() and (final[sh["diff_status"] != diff.OK] == sh["diff_status"][sh["diff_status"] != diff.OK]).all()
    lr, dof = values(got, "lr_stat", F), values(got, "dof", sh["diff_status"])
    assert (lr[final != diff.OK] == 0.0).all() and (lr[final == diff.OK] >= 0.0).all() and (dof[final == diff.OK] >= 1).all()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_bytes(case):
    import torch
    from strawberry_amd import _lib, diff, em
    src, exe = case["dir"] / "diff.cpp", case["dir"] / "diff"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got = parse(out.stdout)
    ctx = em.default_context(0)
    a, b = case["a"], case["b"]
    dev = torch.device("cuda", ctx.device)
    pa, pb = em.Plan(ctx, a.row_off, a.iso_off, a.f_off), em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (a.count, a.F, b.count, b.F, case["keep_a"], case["keep_b"])]
    t = diff.em_diff_device(ctx, pa, d[0], d[1], pb, d[2], d[3], d[4], d[5])
    pa.close(), pb.close()
    for k in diff.NAMES:
        x = getattr(t, k)
        assert values(got, k, x).astype(x.dtype).tobytes() == x.tobytes(), k
