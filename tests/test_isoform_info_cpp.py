"""The C++ layer of the isoform information (include/sbgpu_host.hpp: sbgpu::IsoformInfo), from a C++14 program.
`host`: sbgpu::IsoformInfo::host on the em_c3_400 golden under the oracle's theta and status -- no GPU; its arrays are the bytes
of the Python binding's (info.em_info_host).
`sanitized`: csrc/info_host.cpp itself -- it is free of HIP -- compiled by g++ with AddressSanitizer and UBSan into a stand-alone
program with its own main (which supplies the library's error slot), run over the same golden: clean, and the same bytes again;
the same program states the offsets of the device form's arena (csrc/stage_host.h: info_layout).
`device`: the same batch uploaded, a plan, sbgpu::IsoformInfo::device -- the bytes of info.em_info_device on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOAD = r"""
template <class T> std::vector<T> load(const std::string &path)
{
   std::ifstream f(path, std::ios::binary | std::ios::ate);
   if (!f) throw std::runtime_error("cannot read " + path);
   std::vector<T> v((size_t)f.tellg() / sizeof(T));
   f.seekg(0);
   f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
   return v;
}
void print(const char *name, const std::vector<double> &v)
{
   for (double x : v) std::printf("%s %a\n", name, x);
}
template <class T> void print_int(const char *name, const std::vector<T> &v)
{
   for (T x : v) std::printf("%s %lld\n", name, (long long)x);
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
   if (argc < 3) return 2;
   const std::string d = std::string(argv[1]) + "/";
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto count = load<int32_t>(d + "count"), status = load<int32_t>(d + "status");
   const auto F = load<double>(d + "F"), theta = load<double>(d + "theta");
   const int64_t n_loci = (int64_t)row_off.size() - 1;
   sbgpu::IsoformInfo t;
   if (std::strcmp(argv[2], "device") == 0) {
      sbgpu::Context ctx(0);
      sbgpu_plan_t *plan = nullptr;
      sbgpu::check(sbgpu_plan_create(ctx.get(), n_loci, row_off.data(), iso_off.data(), f_off.data(), &plan), "sbgpu_plan_create");
      t = sbgpu::IsoformInfo::device(ctx, plan, iso_off.data(), up(count), up(F), up(theta), nullptr, up(status));
      if (!t.raw.d_se || !t.raw.d_cov || !t.raw.d_cov_off || !t.raw.d_info_status || t.raw.se) return 3;
      sbgpu_plan_destroy(plan);
   } else {
      const sbgpu_batch_t b = {n_loci, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()};
      t = sbgpu::IsoformInfo::host(b, theta.data(), nullptr, status.data());
      try {
         sbgpu::IsoformInfo::host(b, nullptr);
         return 4;
      } catch (const std::exception &e) {
         if (!std::strstr(e.what(), "theta is needed")) return 5;
      }
   }
   if ((int64_t)t.rank.size() != n_loci || (int64_t)t.se.size() != iso_off.back() || (int64_t)t.cov.size() != t.cov_off.back()) return 6;
   const int64_t n0 = iso_off[1] - iso_off[0];
   if (n0 > 0 && n0 <= 64 && t.covariance(0, n0, n0 - 1, 0) != t.cov[(size_t)(n0 - 1)]) return 7;
   print("se", t.se), print("partner_corr", t.partner_corr), print("min_pivot", t.min_pivot), print("cov", t.cov);
   print_int("ident", t.ident), print_int("alias_of", t.alias_of), print_int("partner", t.partner);
   print_int("rank", t.rank), print_int("n_free", t.n_free), print_int("info_status", t.info_status);
   return 0;
}
"""

# the stand-alone program over csrc/info_host.cpp: no library, no HIP; sb::api_fail is this file's
SANITIZED = r"""#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/sbgpu.h"
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
   {  // the device form's arena (csrc/stage_host.h: info_layout), written out by hand: every entry rounded up to 256 bytes
      const sb::InfoLayout L = sb::info_layout(40, 300, 70, 500, 30, 100, true, true);
      if (L.small != 0 || L.large != 256 || L.covoff != 768 || L.upload_bytes != 1280 || L.keep != 1280 || L.status != 1792 || L.live != 2048) return 10;
      if (L.gain != 2560 || L.w != 3328 || L.se != 5888 || L.pcorr != 6656 || L.ident != 7424 || L.alias != 7936 || L.partner != 8448) return 11;
      if (L.minpiv != 8960 || L.rank != 9472 || L.nfree != 9728 || L.istatus != 9984 || L.cov != 10240 || L.cov_bytes != 4096 || L.bytes != 14336) return 12;
      const sb::InfoLayout M = sb::info_layout(40, 300, 70, 0, 30, 100, false, false);
      if (M.keep != 1280 || M.status != 1280 || M.live != 1280 || M.cov_bytes != 256 || M.bytes != L.bytes - 512 - 256 - 3840) return 13;
   }
   const std::string d = std::string(argv[1]) + "/";
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto count = load<int32_t>(d + "count"), status = load<int32_t>(d + "status");
   const auto F = load<double>(d + "F"), theta = load<double>(d + "theta");
   const int64_t n_loci = (int64_t)row_off.size() - 1, n_iso = iso_off.back();
   std::vector<int64_t> cov_off((size_t)n_loci + 1);
   if (sbgpu_em_info_cov_offsets(iso_off.data(), n_loci, cov_off.data()) != SBGPU_OK) return 3;
   // exactly sized: a write past an array's end is the sanitizer's to see
   std::vector<double> se((size_t)n_iso), partner_corr((size_t)n_iso), min_pivot((size_t)n_loci), cov((size_t)cov_off.back());
   std::vector<int32_t> ident((size_t)n_iso), alias_of((size_t)n_iso), partner((size_t)n_iso), rank((size_t)n_loci), n_free((size_t)n_loci), info_status((size_t)n_loci);
   sbgpu_em_info_t out = {};
   out.se = se.data(), out.partner_corr = partner_corr.data(), out.ident = ident.data(), out.alias_of = alias_of.data(), out.partner = partner.data();
   out.min_pivot = min_pivot.data(), out.rank = rank.data(), out.n_free = n_free.data(), out.info_status = info_status.data();
   out.cov = cov.data(), out.cov_off = cov_off.data();
   const sbgpu_batch_t b = {n_loci, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()};
   if (sbgpu_em_info_host(&b, theta.data(), nullptr, status.data(), &out) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 4;
   }
   if (sbgpu_em_info_host(&b, nullptr, nullptr, nullptr, &out) != SBGPU_EINVAL || last_error.find("theta is needed") == std::string::npos) return 5;
   print("se", se), print("partner_corr", partner_corr), print("min_pivot", min_pivot), print("cov", cov);
   print_int("ident", ident), print_int("alias_of", alias_of), print_int("partner", partner);
   print_int("rank", rank), print_int("n_free", n_free), print_int("info_status", info_status);
   return 0;
}
"""


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle, golden):
    from strawberry_amd import _lib
    _lib.load()
    b, _, _ = golden("em_c3_400")
    theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    d = tmp_path_factory.mktemp("info_cpp")
    for name, a, dt in (("row_off", b.row_off, np.int64), ("iso_off", b.iso_off, np.int64), ("f_off", b.f_off, np.int64), ("count", b.count, np.int32),
                        ("F", b.F, np.float64), ("theta", theta, np.float64), ("status", status, np.int32)):
        np.ascontiguousarray(a, dt).tofile(str(d / name))
    return dict(dir=d, b=b, theta=theta, status=status)


@pytest.fixture(scope="module")
def program(case):
    from strawberry_amd import _lib
    src, exe = case["dir"] / "info.cpp", case["dir"] / "info"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def parse(text):
    out = {}
    for line in text.split("\n"):
        if line:
            k, v = line.split()
            out.setdefault(k, []).append(v)
    return out


def same_bytes(got, t):
    from strawberry_amd import info
    for k in info.NAMES:
        a = getattr(t, k)
        mine = np.array([float.fromhex(x) for x in got.get(k, [])]) if a.dtype == np.float64 else np.array([int(x) for x in got.get(k, [])], a.dtype)
        assert mine.astype(a.dtype).tobytes() == a.tobytes(), k


def test_host_program_gives_the_python_bindings_bytes(case, program):
    from strawberry_amd import info
    out = subprocess.run([str(program), str(case["dir"]), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    t = info.em_info_host(case["b"], case["theta"], status=case["status"])
    same_bytes(parse(out.stdout), t)
    assert (t.ident == info.ALIASED).any() and (t.rank > 1).any() and t.cov.any()


def test_the_host_form_alone_under_the_sanitizers(case):
    """csrc/info_host.cpp needs neither HIP nor the library: g++ builds it with ASan and UBSan beside a main of its own"""
    from strawberry_amd import info
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(SANITIZED.replace('"../../include/sbgpu.h"', '"%s"' % os.path.join(ROOT, "include", "sbgpu.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, str(src), os.path.join(csrc, "info_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    same_bytes(parse(out.stdout), info.em_info_host(case["b"], case["theta"], status=case["status"]))


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_bytes(case, program):
    import torch
    from strawberry_amd import em, info
    out = subprocess.run([str(program), str(case["dir"]), "device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    ctx = em.default_context(0)
    b = case["b"]
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, case["theta"], case["status"])]
    t = info.em_info_device(ctx, plan, d[0], d[1], d[2], None, d[3])
    plan.close()
    same_bytes(parse(out.stdout), t)
