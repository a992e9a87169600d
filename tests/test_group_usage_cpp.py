"""The C++ side of the differential isoform usage between two groups of replicates.
`sanitized`: csrc/gdiff_host.cpp itself -- it is free of HIP -- compiled by g++ with AddressSanitizer and UBSan into a
stand-alone program with its own main (which supplies the library's error slot), run over em_c3_400 as 2 + 1 replicates (one of
them absent at every fifth locus) with three filters: the shapes, the expansion and the statistics of a made-up solve into
exactly sized arrays: clean, and the bytes of the Python binding's; the same program states the offsets of the device form's
arenas (csrc/stage_host.h: gdiff_layout, gdiff_chunk_layout), worked out by hand.  No sanitizer is used on anything loaded
into Python.
`device`: a C++14 program over include/sbgpu_host.hpp: sbgpu::GroupDifferentialUsage::device on the same batches -- the bytes of
gdiff.em_gdiff_device on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import gdiff_util as GU
from test_isoform_info_cpp import LOAD, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_A, N_B = 2, 1

READ = r"""
   const std::string d = std::string(argv[1]) + "/";
   const int n_a = 2, n_b = 1, S = 3;
   const auto iso_off = load<int64_t>(d + "iso_off");
   std::vector<int64_t> row[3], f[3];
   std::vector<int32_t> count[3], keep[3];
   std::vector<double> F[3];
   for (int s = 0; s < S; ++s) {
      const std::string x = std::to_string(s);
      row[s] = load<int64_t>(d + "row_off_" + x), f[s] = load<int64_t>(d + "f_off_" + x), count[s] = load<int32_t>(d + "count_" + x);
      keep[s] = load<int32_t>(d + "keep_" + x), F[s] = load<double>(d + "F_" + x);
   }
   const int64_t n_loci = (int64_t)iso_off.size() - 1, n_iso = iso_off.back();
"""

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
      const sb::GdiffLayout L = sb::gdiff_layout(3, 40, 300, 70, 1000);
      if (L.lstat != 0 || L.p_a != 256 || L.p_b != 512 || L.rank != 768 || L.koff != 2048 || L.kcol != 2560 || L.slot != 3072 || L.table != 5120) return 10;
      if (L.upload_bytes != 5376 || L.th_s != 5376 || L.th_g != 12800 || L.th_all != 17664 || L.us_s != 20224 || L.us_g != 27648 || L.us_all != 32512) return 11;
      if (L.delta != 35072 || L.lr_b != 37632 || L.lr_w != 38144 || L.ll_own != 38656 || L.ll_grp != 39680 || L.ll_all != 40704 || L.n_frag != 41728) return 12;
      if (L.shift != 42752 || L.dof_b != 43264 || L.dof_w != 43520 || L.status != 43776 || L.top != 44032 || L.st_s != 44288 || L.it_s != 44800) return 13;
      if (L.st_g != 45312 || L.it_g != 45824 || L.st_all != 46336 || L.it_all != 46592 || L.sum != 46848 || L.chunk != 48896 || L.bytes != 49920) return 14;
      const sb::GdiffChunkLayout M = sb::gdiff_chunk_layout(3, 3, 2, 5, 70, 9, 100, 30, 700, 512);
      if (M.tiles != 0 || M.items != 256 || M.list != 512 || M.src_g != 768 || M.src_a != 1024 || M.upload_bytes != 1280 || M.c != 1280) return 15;
      if (M.alpha_g != 3072 || M.alpha_a != 4864 || M.count != 6656 || M.F != 7168 || M.theta != 12800 || M.status != 13056 || M.iters != 13312) return 16;
      if (M.g_theta != 13568 || M.g_status != 13824 || M.a_theta != 14080 || M.a_status != 14336 || M.fit != 14592 || M.g_fit != 15104 || M.a_fit != 15616) return 17;
      if (M.bytes != 16128 || sizeof(sb::GdiffTile) != 48 || sizeof(sb::GdiffScaleItem) != 32 || sizeof(sb::GdiffSample) != 32) return 18;
   }
""" + READ + r"""
   const int64_t *rows[3] = {row[0].data(), row[1].data(), row[2].data()};
   const int32_t *keeps[3] = {keep[0].data(), nullptr, keep[2].data()};
   int64_t sizes[4];
   if (sbgpu_em_gdiff_shapes_host(n_loci, n_a, n_b, rows, iso_off.data(), keeps, sizes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SBGPU_OK)
      return 3;
   // exactly sized: a write past an array's end is the sanitizer's to see
   std::vector<int32_t> gdiff_status((size_t)n_loci), sub_locus((size_t)sizes[0]), sub_kind((size_t)sizes[0]), sub_sample((size_t)sizes[0]), sub_count((size_t)sizes[1]);
   std::vector<int64_t> sub_row_off((size_t)sizes[0] + 1), sub_iso_off((size_t)sizes[0] + 1), sub_f_off((size_t)sizes[0] + 1);
   std::vector<double> sub_F((size_t)sizes[3]);
   if (sbgpu_em_gdiff_shapes_host(n_loci, n_a, n_b, rows, iso_off.data(), keeps, sizes, gdiff_status.data(), sub_locus.data(), sub_kind.data(), sub_sample.data(),
                                  sub_row_off.data(), sub_iso_off.data(), sub_f_off.data()) != SBGPU_OK) return 4;
   if (sub_row_off.back() != sizes[1] || sub_iso_off.back() != sizes[2] || sub_f_off.back() != sizes[3]) return 5;
   sbgpu_batch_t b[3];
   const sbgpu_batch_t *bp[3];
   for (int s = 0; s < S; ++s) b[s] = {n_loci, row[s].data(), iso_off.data(), f[s].data(), count[s].data(), F[s].data()}, bp[s] = &b[s];
   if (sbgpu_em_gdiff_expand_host(n_a, n_b, bp, keeps, sub_count.data(), sub_F.data()) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 6;
   }
   if (sbgpu_em_gdiff_expand_host(n_a, n_b, bp, keeps, nullptr, sub_F.data()) != SBGPU_EINVAL || last_error.find("sub_count") == std::string::npos) return 7;
   if (sbgpu_em_gdiff_expand_host(n_a, 0, bp, keeps, sub_count.data(), sub_F.data()) != SBGPU_EINVAL || last_error.find("group without samples") == std::string::npos) return 8;
   // the statistics over a made-up solve and made-up fits: exactly sized outputs
   const size_t n_sub = (size_t)sizes[0], nl = (size_t)n_loci, ni = (size_t)n_iso;
   std::vector<double> theta((size_t)sizes[2]), ll(n_sub), llg(n_sub), lla(n_sub);
   std::vector<int32_t> status(n_sub, 0), iters(n_sub, 7);
   std::vector<int64_t> n_live(n_sub, 9), n_dropped(n_sub, 1), n_imp(n_sub, 0);
   for (size_t i = 0; i < theta.size(); ++i) theta[i] = (double)(i % 13) + 0.5;
   for (size_t i = 0; i < n_sub; ++i)
      ll[i] = -(double)(i % 7) - 1.25, llg[i] = ll[i] - (double)(i % 3) * 0.25, lla[i] = llg[i] - (double)(i % 5) * 0.5, n_imp[i] = (int64_t)(i % 3), status[i] = i % 23 == 22 ? 2 : 0;
   std::vector<double> ts(3 * ni, -1.0), us(3 * ni, -1.0), tg(2 * ni, -1.0), ug(2 * ni, -1.0), ta(ni, -1.0), ua(ni, -1.0), delta(ni, -1.0);
   std::vector<double> lr_b(nl, -1.0), lr_w(nl, -1.0), ll_own(3 * nl, -1.0), ll_grp(3 * nl, -1.0), ll_all(3 * nl, -1.0);
   std::vector<int64_t> n_frag(3 * nl, -1), shift(nl, -1);
   std::vector<int32_t> dof_b(nl, -7), dof_w(nl, -7), p_a(nl, -7), p_b(nl, -7), final_status(nl, -7), top(nl, -7), st_s(3 * nl, -7), it_s(3 * nl, -7), st_g(2 * nl, -7),
      it_g(2 * nl, -7), st_all(nl, -7), it_all(nl, -7);
   sbgpu_em_gdiff_t out = {};
   out.theta_sample = ts.data(), out.usage_sample = us.data(), out.theta_group = tg.data(), out.usage_group = ug.data(), out.theta_all = ta.data();
   out.usage_all = ua.data(), out.delta_usage = delta.data(), out.lr_between = lr_b.data(), out.lr_within = lr_w.data(), out.loglik_own = ll_own.data();
   out.loglik_group = ll_grp.data(), out.loglik_all = ll_all.data(), out.n_frag = n_frag.data(), out.lost_shift = shift.data();
   out.dof_between = dof_b.data(), out.dof_within = dof_w.data(), out.p_a = p_a.data(), out.p_b = p_b.data(), out.gdiff_status = final_status.data();
   out.top_iso = top.data(), out.status_sample = st_s.data(), out.iters_sample = it_s.data(), out.status_group = st_g.data(), out.iters_group = it_g.data();
   out.status_all = st_all.data(), out.iters_all = it_all.data();
   if (sbgpu_em_gdiff_stat_host(n_a, n_b, bp, keeps, theta.data(), status.data(), iters.data(), ll.data(), n_live.data(), n_dropped.data(), n_imp.data(), llg.data(),
                                n_dropped.data(), n_imp.data(), lla.data(), n_dropped.data(), n_imp.data(), &out) != SBGPU_OK) return 9;
   print_int("gdiff_status", gdiff_status), print_int("sub_locus", sub_locus), print_int("sub_kind", sub_kind), print_int("sub_sample", sub_sample);
   print_int("row_off", sub_row_off), print_int("iso_off", sub_iso_off), print_int("f_off", sub_f_off);
   print_int("count", sub_count), print("F", sub_F);
   print("lr_between", lr_b), print("lr_within", lr_w), print("delta_usage", delta), print_int("final_status", final_status), print_int("dof_between", dof_b);
   print_int("dof_within", dof_w), print_int("p_a", p_a), print_int("p_b", p_b), print_int("top_iso", top), print_int("status_sample", st_s), print_int("n_frag", n_frag);
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
""" + READ + r"""
   sbgpu::Context ctx(0);
   std::vector<const sbgpu_plan_t *> plans;
   std::vector<const int32_t *> d_count, d_keep;
   std::vector<const double *> d_F;
   for (int s = 0; s < S; ++s) {
      sbgpu_plan_t *p = nullptr;
      sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row[s].data(), iso_off.data(), f[s].data(), &p), "sbgpu_plan_create");
      plans.push_back(p), d_count.push_back(up(count[s])), d_F.push_back(up(F[s])), d_keep.push_back(s == 1 ? nullptr : up(keep[s]));
   }
   sbgpu::GroupDifferentialUsage t = sbgpu::GroupDifferentialUsage::device(ctx, n_a, n_b, plans, d_count, d_F, d_keep);
   if (!t.raw.d_lr_between || !t.raw.d_theta_all || !t.raw.d_top_iso || t.raw.lr_between) return 3;
   for (const sbgpu_plan_t *p : plans) sbgpu_plan_destroy(const_cast<sbgpu_plan_t *>(p));
   if ((int64_t)t.theta_sample.size() != S * n_iso || (int64_t)t.lr_between.size() != n_loci || (int64_t)t.status_group.size() != 2 * n_loci) return 4;
   print("theta_sample", t.theta_sample), print("theta_group", t.theta_group), print("theta_all", t.theta_all), print("usage_sample", t.usage_sample);
   print("usage_group", t.usage_group), print("usage_all", t.usage_all), print("delta_usage", t.delta_usage), print("lr_between", t.lr_between);
   print("lr_within", t.lr_within), print("loglik_own", t.loglik_own), print("loglik_group", t.loglik_group), print("loglik_all", t.loglik_all);
   print_int("n_frag", t.n_frag), print_int("lost_shift", t.lost_shift), print_int("dof_between", t.dof_between), print_int("dof_within", t.dof_within);
   print_int("p_a", t.p_a), print_int("p_b", t.p_b), print_int("gdiff_status", t.gdiff_status), print_int("top_iso", t.top_iso);
   print_int("status_sample", t.status_sample), print_int("iters_sample", t.iters_sample), print_int("status_group", t.status_group);
   print_int("iters_group", t.iters_group), print_int("status_all", t.status_all), print_int("iters_all", t.iters_all);
   return 0;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden, oracle):
    from strawberry_amd import _lib
    _lib.load()
    a, _, _ = golden("em_c3_400")
    ga, gb = GU.replicates(a, "absent", N_A, N_B, 4, oracle.em_batch(a.row_off, a.iso_off, a.f_off, a.count, a.F)[0])
    rng = np.random.default_rng(9)
    n_iso = int(a.iso_off[-1])
    keeps = [(rng.random(n_iso) < 0.6).astype(np.int32) for _ in range(3)]
    d = tmp_path_factory.mktemp("gdiff_cpp")
    np.ascontiguousarray(a.iso_off, np.int64).tofile(str(d / "iso_off"))
    for s, b in enumerate(ga + gb):
        for name, x, dt in (("row_off", b.row_off, np.int64), ("f_off", b.f_off, np.int64), ("count", b.count, np.int32), ("F", b.F, np.float64),
                            ("keep", keeps[s], np.int32)):
            np.ascontiguousarray(x, dt).tofile(str(d / ("%s_%d" % (name, s))))
    keeps[1] = None                                          # (the programs pass no filter for the second sample)
    return dict(dir=d, ga=ga, gb=gb, keeps=keeps)


def values(got, k, like):
    if like.dtype == np.float64:
        return np.array([float.fromhex(x) for x in got.get(k, [])])
    return np.array([int(x) for x in got.get(k, [])], like.dtype)


def test_the_host_form_alone_under_the_sanitizers(case):
    """csrc/gdiff_host.cpp needs neither HIP nor the library: g++ builds it with ASan and UBSan beside a main of its own"""
    from strawberry_amd import gdiff
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(SANITIZED.replace("SBGPU_H", os.path.join(ROOT, "include", "sbgpu.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, str(src), os.path.join(csrc, "gdiff_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    got = parse(out.stdout)
    ga, gb, keeps = case["ga"], case["gb"], case["keeps"]
    sh = gdiff.shapes_host([b.row_off for b in ga], [b.row_off for b in gb], ga[0].iso_off, keeps)
    count, F = gdiff.expand_host(ga, gb, keeps, sh)
    for k, x in list(sh.items()) + [("count", count), ("F", F)]:
        assert values(got, k, x).astype(x.dtype).tobytes() == x.tobytes(), k
    pre = sh["gdiff_status"]
    assert (pre == gdiff.SOLE).any() and (pre == gdiff.ONE_GROUP).any() and (pre == gdiff.OK).sum() > 100
    assert (sh["sub_kind"] == gdiff.KIND_GROUP_A).any() and not (sh["sub_kind"] == gdiff.KIND_GROUP_B).any()
    final = values(got, "final_status", pre)
    assert (final == gdiff.UNSOLVED).any() and (final[pre != gdiff.OK] == pre[pre != gdiff.OK]).all()
    ok = final == gdiff.OK
    lr_b, lr_w = values(got, "lr_between", F), values(got, "lr_within", F)
    dof_b, dof_w = values(got, "dof_between", pre), values(got, "dof_within", pre)
    p_a, p_b = values(got, "p_a", pre), values(got, "p_b", pre)
    assert (lr_b[~ok] == 0.0).all() and (lr_w[~ok] == 0.0).all() and (lr_b[ok] >= 0.0).all() and (lr_w[ok] >= 0.0).all() and (dof_b[ok] >= 1).all()
    assert (dof_w[ok] == (p_a + p_b - 2)[ok] * dof_b[ok]).all() and (p_a[ok] == 1).any() and (lr_w[ok & (p_a == 1)] == 0.0).all() and (lr_w[ok & (p_a == 2)] > 0.0).any()
    n_frag = values(got, "n_frag", np.zeros(1, np.int64)).reshape(3, -1)
    st = values(got, "status_sample", pre).reshape(3, -1)
    assert (n_frag[:, ~ok] == 0).all() and (st[:, pre != gdiff.OK] == -1).all() and ((st == -1) & (pre == gdiff.OK)[None, :]).any()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_bytes(case):
    import torch
    from strawberry_amd import _lib, em, gdiff
    src, exe = case["dir"] / "gdiff.cpp", case["dir"] / "gdiff"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got = parse(out.stdout)
    ctx = em.default_context(0)
    dev = torch.device("cuda", ctx.device)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    plans = [em.Plan(ctx, b.row_off, b.iso_off, b.f_off) for b in case["ga"] + case["gb"]]
    samples = [(p, up(b.count), up(b.F)) for p, b in zip(plans, case["ga"] + case["gb"])]
    t = gdiff.em_gdiff_device(ctx, samples[:N_A], samples[N_A:], [up(k) for k in case["keeps"]])
    for p in plans:
        p.close()
    for k in gdiff.NAMES:
        x = getattr(t, k)
        assert values(got, k, x).astype(x.dtype).tobytes() == x.tobytes(), k
