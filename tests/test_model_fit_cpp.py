"""The C++ layer of the model fit (include/sbgpu_host.hpp: sbgpu::ModelFit), from a C++14 program.
`host`: sbgpu::ModelFit::host on the em_random_256 golden under the oracle's theta and status -- no GPU; its arrays are the bytes
of the Python binding's (fit.em_fit_host).
`device`: the same batch uploaded, a plan, sbgpu::ModelFit::device -- its arrays are the bytes of fit.em_fit_device on the same
inputs (the device form gives the same bits from call to call)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include <hip/hip_runtime_api.h>
#include <cstring>
#include <fstream>
#include "sbgpu_host.hpp"
template <class T> std::vector<T> load(const std::string &path)
{
   std::ifstream f(path, std::ios::binary | std::ios::ate);
   if (!f) throw std::runtime_error("cannot read " + path);
   std::vector<T> v((size_t)f.tellg() / sizeof(T));
   f.seekg(0);
   f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
   return v;
}
template <class T> const T *up(const std::vector<T> &v)
{
   void *p = nullptr;
   if (hipMalloc(&p, v.size() * sizeof(T) + 8) != hipSuccess || hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("upload");
   return (const T *)p;
}
void print(const char *name, const std::vector<double> &v)
{
   for (double x : v) std::printf("%s %a\n", name, x);
}
template <class T> void print_int(const char *name, const std::vector<T> &v)
{
   for (T x : v) std::printf("%s %lld\n", name, (long long)x);
}
int main(int argc, char **argv)
{
   if (argc < 3) return 2;
   const std::string d = std::string(argv[1]) + "/";
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto count = load<int32_t>(d + "count"), status = load<int32_t>(d + "status");
   const auto F = load<double>(d + "F"), theta = load<double>(d + "theta");
   const int64_t n_loci = (int64_t)row_off.size() - 1;
   sbgpu::ModelFit t;
   if (std::strcmp(argv[2], "device") == 0) {
      sbgpu::Context ctx(0);
      sbgpu_plan_t *plan = nullptr;
      sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row_off.data(), iso_off.data(), f_off.data(), &plan), "sbgpu_plan_create");
      t = sbgpu::ModelFit::device(ctx, plan, up(count), up(F), up(theta), nullptr, up(status));
      if (!t.raw.d_expected || !t.raw.d_worst_bin || t.raw.expected) return 3;
      sbgpu_plan_destroy(plan);
   } else {
      const sbgpu_batch_t b = {n_loci, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()};
      t = sbgpu::ModelFit::host(b, theta.data(), nullptr, status.data());
      try {
         sbgpu::ModelFit::host(b, nullptr);
         return 4;
      } catch (const std::exception &e) {
         if (!std::strstr(e.what(), "theta is needed")) return 5;
      }
   }
   if ((int64_t)t.loglik.size() != n_loci || (int64_t)t.expected.size() != row_off.back() || (int64_t)t.score.size() != iso_off.back()) return 6;
   print("expected", t.expected), print("resid", t.resid), print("score", t.score);
   print("loglik", t.loglik), print("deviance", t.deviance), print("pearson", t.pearson), print("chi2", t.reduced_chi2());
   print_int("n_live", t.n_live), print_int("n_dropped", t.n_dropped), print_int("n_impossible", t.n_impossible);
   print_int("dof", t.dof), print_int("worst_bin", t.worst_bin);
   return 0;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle, golden):
    from strawberry_amd import _lib
    _lib.load()
    b, _, _ = golden("em_random_256")
    theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    d = tmp_path_factory.mktemp("fit_cpp")
    for name, a, dt in (("row_off", b.row_off, np.int64), ("iso_off", b.iso_off, np.int64), ("f_off", b.f_off, np.int64), ("count", b.count, np.int32),
                        ("F", b.F, np.float64), ("theta", theta, np.float64), ("status", status, np.int32)):
        np.ascontiguousarray(a, dt).tofile(str(d / name))
    src, exe = d / "fit.cpp", d / "fit"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return dict(dir=d, exe=exe, b=b, theta=theta, status=status)


def parse(text):
    out = {}
    for line in text.split("\n"):
        if line:
            k, v = line.split()
            out.setdefault(k, []).append(v)
    return out


def same_bytes(got, t):
    from strawberry_amd import fit
    for k in fit.NAMES:
        a = getattr(t, k)
        mine = np.array([float.fromhex(x) for x in got.get(k, [])]) if a.dtype == np.float64 else np.array([int(x) for x in got.get(k, [])], a.dtype)
        assert mine.astype(a.dtype).tobytes() == a.tobytes(), k
    chi2 = np.array([float.fromhex(x) for x in got["chi2"]])
    np.testing.assert_array_equal(chi2, t.reduced_chi2())


def test_host_program_gives_the_python_bindings_bytes(case):
    from strawberry_amd import fit
    out = subprocess.run([str(case["exe"]), str(case["dir"]), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    t = fit.em_fit_host(case["b"], case["theta"], status=case["status"])
    same_bytes(parse(out.stdout), t)
    assert t.n_live.sum() > 0 and (t.dof > 0).any()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_bytes(case):
    import torch
    from strawberry_amd import em, fit
    out = subprocess.run([str(case["exe"]), str(case["dir"]), "device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    ctx = em.default_context(0)
    b = case["b"]
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, case["theta"], case["status"])]
    t = fit.em_fit_device(ctx, plan, d[0], d[1], d[2], None, d[3])
    plan.close()
    same_bytes(parse(out.stdout), t)
