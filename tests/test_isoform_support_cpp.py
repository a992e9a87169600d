"""The C++ side of the isoform support.
`sanitized`: csrc/loo_host.cpp itself -- it is free of HIP -- compiled by g++ with AddressSanitizer and UBSan into a stand-alone
program with its own main (which supplies the library's error slot), run over em_c3_400's shapes and expansion with a filter:
clean, and the bytes of the Python binding's; the same program states the offsets of the device form's arenas
(csrc/stage_host.h: loo_layout, loo_chunk_layout).  No sanitizer is used on anything loaded into Python.
`device`: a C++14 program over include/sbgpu_host.hpp: sbgpu::IsoformSupport::device on the same batch -- the bytes of
support.em_loo_device on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

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
      const sb::LooLayout L = sb::loo_layout(40, 300, 70, 500, 1000);
      if (L.lstat != 0 || L.woff != 256 || L.rank != 2816 || L.first != 4096 || L.koff != 4608 || L.kcol != 5120 || L.upload_bytes != 5632) return 10;
      if (L.lr != 5632 || L.hgain != 8192 || L.refit != 10752 || L.nuniq != 13312 || L.heir != 15872 || L.stw != 17152 || L.itw != 18432) return 11;
      if (L.supp != 19712 || L.llb != 20992 || L.stb != 21504 || L.itb != 21760 || L.wo != 22016 || L.chunk != 26112 || L.bytes != 27136) return 12;
      const sb::LooChunkLayout M = sb::loo_chunk_layout(3, 10, 100, 30, 700, 512);
      if (M.tiles != 0 || M.upload_bytes != 256 || M.count != 256 || M.F != 768 || M.theta != 6400 || M.status != 6656 || M.iters != 6912) return 13;
      if (M.fit != 7168 || M.bytes != 7680 || sizeof(sb::LooTile) != 16) return 14;
   }
   const std::string d = std::string(argv[1]) + "/";
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto count = load<int32_t>(d + "count"), keep = load<int32_t>(d + "keep");
   const auto F = load<double>(d + "F");
   const int64_t n_loci = (int64_t)row_off.size() - 1, n_iso = iso_off.back();
   int64_t sizes[4];
   if (sbgpu_em_loo_shapes_host(n_loci, row_off.data(), iso_off.data(), keep.data(), sizes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SBGPU_OK) return 3;
   // exactly sized: a write past an array's end is the sanitizer's to see
   std::vector<int32_t> loo_status((size_t)n_loci), sub_locus((size_t)sizes[0]), sub_drop((size_t)sizes[0]), sub_count((size_t)sizes[1]);
   std::vector<int64_t> sub_row_off((size_t)sizes[0] + 1), sub_iso_off((size_t)sizes[0] + 1), sub_f_off((size_t)sizes[0] + 1), without_off((size_t)n_iso + 1);
   std::vector<double> sub_F((size_t)sizes[3]);
   if (sbgpu_em_loo_shapes_host(n_loci, row_off.data(), iso_off.data(), keep.data(), sizes, loo_status.data(), sub_locus.data(), sub_drop.data(),
                                sub_row_off.data(), sub_iso_off.data(), sub_f_off.data()) != SBGPU_OK) return 4;
   if (sub_row_off.back() != sizes[1] || sub_iso_off.back() != sizes[2] || sub_f_off.back() != sizes[3]) return 5;
   const sbgpu_batch_t b = {n_loci, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()};
   if (sbgpu_em_loo_expand_host(&b, keep.data(), sub_count.data(), sub_F.data()) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 6;
   }
   if (sbgpu_em_loo_expand_host(&b, keep.data(), nullptr, sub_F.data()) != SBGPU_EINVAL || last_error.find("sub_count") == std::string::npos) return 7;
   if (sbgpu_em_loo_offsets(iso_off.data(), keep.data(), n_loci, without_off.data()) != SBGPU_OK) return 8;
   // the statistics over a made-up solve (theta 1, 2, 3, ...): exactly sized outputs
   std::vector<double> theta((size_t)sizes[2]), loglik((size_t)sizes[0]);
   std::vector<int32_t> status((size_t)sizes[0], 0), iters((size_t)sizes[0], 7);
   std::vector<int64_t> n_live((size_t)sizes[0], 9), n_dropped((size_t)sizes[0], 1), n_imp((size_t)sizes[0], 0);
   for (size_t i = 0; i < theta.size(); ++i) theta[i] = (double)(i % 13) + 0.5;
   for (size_t i = 0; i < loglik.size(); ++i) loglik[i] = -(double)(i % 7) - 1.25, n_imp[i] = (int64_t)(i % 3);
   std::vector<double> lr((size_t)n_iso), hg((size_t)n_iso), refit((size_t)n_iso), llb((size_t)n_loci), wo((size_t)without_off.back());
   std::vector<int64_t> nu((size_t)n_iso);
   std::vector<int32_t> heir((size_t)n_iso), stw((size_t)n_iso), itw((size_t)n_iso), supp((size_t)n_iso), lst((size_t)n_loci), stb((size_t)n_loci), itb((size_t)n_loci);
   sbgpu_em_loo_t out = {};
   out.lr_stat = lr.data(), out.heir_gain = hg.data(), out.theta_refit = refit.data(), out.n_unique = nu.data(), out.heir = heir.data();
   out.status_without = stw.data(), out.iters_without = itw.data(), out.support = supp.data(), out.loglik_base = llb.data();
   out.loo_status = lst.data(), out.status_base = stb.data(), out.iters_base = itb.data(), out.theta_without = wo.data(), out.without_off = without_off.data();
   if (sbgpu_em_loo_stat_host(n_loci, iso_off.data(), keep.data(), theta.data(), status.data(), iters.data(), loglik.data(), n_live.data(),
                              n_dropped.data(), n_imp.data(), &out) != SBGPU_OK) return 9;
   print_int("loo_status", loo_status), print_int("sub_locus", sub_locus), print_int("sub_drop", sub_drop);
   print_int("row_off", sub_row_off), print_int("iso_off", sub_iso_off), print_int("f_off", sub_f_off), print_int("without_off", without_off);
   print_int("count", sub_count), print("F", sub_F);
   print("lr_stat", lr), print("heir_gain", hg), print_int("n_unique", nu), print_int("heir", heir), print_int("support", supp);
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
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto count = load<int32_t>(d + "count"), keep = load<int32_t>(d + "keep");
   const auto F = load<double>(d + "F");
   const int64_t n_loci = (int64_t)row_off.size() - 1;
   sbgpu::Context ctx(0);
   sbgpu_plan_t *plan = nullptr;
   sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row_off.data(), iso_off.data(), f_off.data(), &plan), "sbgpu_plan_create");
   sbgpu::IsoformSupport t = sbgpu::IsoformSupport::device(ctx, plan, iso_off.data(), up(count), up(F), up(keep), keep.data());
   if (!t.raw.d_lr_stat || !t.raw.d_theta_without || !t.raw.d_without_off || t.raw.lr_stat) return 3;
   sbgpu_plan_destroy(plan);
   if ((int64_t)t.lr_stat.size() != iso_off.back() || (int64_t)t.loo_status.size() != n_loci || (int64_t)t.theta_without.size() != t.without_off.back()) return 4;
   print("lr_stat", t.lr_stat), print("heir_gain", t.heir_gain), print("theta_refit", t.theta_refit), print("loglik_base", t.loglik_base);
   print("without", t.theta_without);
   print_int("n_unique", t.n_unique), print_int("heir", t.heir), print_int("status_without", t.status_without);
   print_int("iters_without", t.iters_without), print_int("support", t.support), print_int("loo_status", t.loo_status);
   print_int("status_base", t.status_base), print_int("iters_base", t.iters_base);
   for (size_t i = 0; i < t.lr_stat.size(); ++i) std::printf("p %a\n", t.p_value((int64_t)i));
   return 0;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden):
    from strawberry_amd import _lib
    _lib.load()
    b, _, _ = golden("em_c3_400")
    keep = (np.random.default_rng(9).random(int(b.iso_off[-1])) < 0.8).astype(np.int32)
    d = tmp_path_factory.mktemp("support_cpp")
    for name, a, dt in (("row_off", b.row_off, np.int64), ("iso_off", b.iso_off, np.int64), ("f_off", b.f_off, np.int64), ("count", b.count, np.int32),
                        ("F", b.F, np.float64), ("keep", keep, np.int32)):
        np.ascontiguousarray(a, dt).tofile(str(d / name))
    return dict(dir=d, b=b, keep=keep)


def values(got, k, like):
    if like.dtype == np.float64:
        return np.array([float.fromhex(x) for x in got.get(k, [])])
    return np.array([int(x) for x in got.get(k, [])], like.dtype)


def test_the_host_form_alone_under_the_sanitizers(case):
    """csrc/loo_host.cpp needs neither HIP nor the library: g++ builds it with ASan and UBSan beside a main of its own"""
    from strawberry_amd import support
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(SANITIZED.replace("SBGPU_H", os.path.join(ROOT, "include", "sbgpu.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, str(src), os.path.join(csrc, "loo_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    got = parse(out.stdout)
    b, keep = case["b"], case["keep"]
    sh = support.shapes_host(b.row_off, b.iso_off, keep)
    count, F = support.expand_host(b, keep, sh)
    for k, a in list(sh.items()) + [("count", count), ("F", F), ("without_off", support.offsets(b.iso_off, keep))]:
        assert values(got, k, a).astype(a.dtype).tobytes() == a.tobytes(), k
    assert (sh["loo_status"] == support.EMPTY).any() or (keep == 0).any()
    supp = values(got, "support", sh["sub_drop"])
    assert (supp[keep == 0] == support.NOT_KEPT).all() and (supp == support.TESTED).sum() == (sh["sub_drop"] >= 0).sum()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_bytes(case):
    import torch
    from strawberry_amd import _lib, em, support
    src, exe = case["dir"] / "support.cpp", case["dir"] / "support"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got = parse(out.stdout)
    ctx = em.default_context(0)
    b = case["b"]
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, case["keep"])]
    t = support.em_loo_device(ctx, plan, d[0], d[1], d[2])
    plan.close()
    for k in support.NAMES + ("without",):
        a = getattr(t, k)
        assert values(got, k, a).astype(a.dtype).tobytes() == a.tobytes(), k
    assert values(got, "p", t.lr_stat).tobytes() == t.p_value().tobytes()
