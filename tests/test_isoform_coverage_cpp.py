"""The C++ layer of the isoform-resolved coverage (include/sbgpu_host.hpp: sbgpu::IsoformCoverage), from a C++14 program.
`host`: sbgpu_bins_create on one toy directory's hits and words, then sbgpu::IsoformCoverage::host under the oracle's weights,
theta, keep and status -- no GPU; its arrays are the bytes of the Python binding's (coverage.isoform_coverage_host).
`device`: a resident call with retention on, then sbgpu::IsoformCoverage::device -- its arrays against
quantify_resident(with_coverage=True)'s within the device-to-device bound (the atomics may order the two runs differently)."""
import os
import subprocess

import numpy as np
import pytest

import coverage_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL, WHICH, MIN_FRAC = 75, "E2E_FILTER", 0.05

PROGRAM = r"""#include <hip/hip_runtime_api.h>
#include <algorithm>
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
void print(const std::string &name, const std::vector<double> &v)
{
   for (double x : v) std::printf("%s %a\n", name.c_str(), x);
}
void print_all(const sbgpu::IsoformCoverage &c, const sbgpu_annotation_t &an)
{
   print("exon_bases", c.exon_bases), print("junction_mass", c.junction_mass), print("iso_bases", c.iso_bases);
   print("unexplained_bases", c.unexplained_bases), print("exon_depth", c.exon_depth(an)), print("iso_depth", c.iso_depth(an));
}
int main(int argc, char **argv)
{
   if (argc < 3) return 2;
   const std::string d = std::string(argv[1]) + "/";
   const bool on_device = std::strcmp(argv[2], "device") == 0;
   const auto iso_off = load<int64_t>(d + "iso_off"), exon_off = load<int64_t>(d + "exon_off"), seg_off = load<int64_t>(d + "seg_off");
   const auto exon_left = load<uint32_t>(d + "exon_left"), exon_right = load<uint32_t>(d + "exon_right");
   const auto seg_left = load<uint32_t>(d + "seg_left"), seg_right = load<uint32_t>(d + "seg_right");
   const auto hit_locus = load<int32_t>(d + "hit_locus");
   const auto feat_off = load<int64_t>(d + "feat_off"), hit_off = load<int64_t>(d + "hit_off");
   const auto feat_code = load<uint8_t>(d + "feat_code");
   const auto feat_left = load<uint32_t>(d + "feat_left"), feat_right = load<uint32_t>(d + "feat_right");
   const auto mass = load<float>(d + "mass");
   const int64_t n_loci = (int64_t)iso_off.size() - 1, n_hits = (int64_t)hit_locus.size(), n_iso = iso_off[(size_t)n_loci];
   const sbgpu_annotation_t an = {n_loci, iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(), seg_off.data(), seg_left.data(), seg_right.data()};
   const sbgpu_hits_t h_hits = {n_hits, hit_locus.data(), feat_off.data(), feat_code.data(), feat_left.data(), feat_right.data()};
   sbgpu_bins_t *bins = nullptr;
   if (!on_device) {
      const auto compat = load<uint32_t>(d + "compat"), key = load<uint32_t>(d + "key");
      const auto F = load<double>(d + "F"), theta = load<double>(d + "theta");
      const auto keep = load<int32_t>(d + "keep"), status = load<int32_t>(d + "status");
      const int32_t cw = (int32_t)(compat.size() / (size_t)n_hits), kw = (int32_t)(key.size() / (size_t)n_hits);
      sbgpu::check(sbgpu_bins_create(&an, &h_hits, mass.data(), cw, kw, compat.data(), key.data(), &bins), "sbgpu_bins_create");
      const sbgpu::IsoformCoverage c =
         sbgpu::IsoformCoverage::host(bins, an, h_hits, compat.data(), cw, F.data(), theta.data(), keep.data(), status.data(), mass.data());
      print_all(c, an);
      std::printf("shape %d\n", c.raw.d_exon_bases != nullptr);
      sbgpu_bins_destroy(bins);
      return 0;
   }
   sbgpu::Context ctx(0);
   const sbgpu_hits_t d_hits = {n_hits, up(hit_locus), up(feat_off), up(feat_code), up(feat_left), up(feat_right)};
   const float *d_mass = up(mass);
   sbgpu_insert_t ins = {};
   ins.mean = 250.0, ins.sd = 30.0, ins.read_len = @RL@;
   const sbgpu_abundance_params_t par = {0, 0, 1, 0, 0.0, @FRAC@};
   std::vector<double> theta((size_t)n_iso + 1);
   std::vector<int32_t> keep((size_t)n_iso + 1), status((size_t)n_loci + 1);
   sbgpu_abundances_t out = {};
   out.theta = theta.data(), out.keep = keep.data(), out.status = status.data();
   sbgpu_insert_t used = {};
   sbgpu::ContextTable::keep(ctx, true);
   sbgpu::check(sbgpu_quantify_resident(ctx.get(), &an, &d_hits, d_mass, hit_off.data(), &ins, @RL@, 0, @MAPPED@, &par, nullptr, &used, &out, &bins),
                "sbgpu_quantify_resident");
   sbgpu::ContextTable::keep(ctx, false);
   const sbgpu::IsoformCoverage c = sbgpu::IsoformCoverage::device(ctx, bins, an, d_hits, out.d_theta, d_mass);
   print_all(c, an);
   std::printf("shape %d\n", c.raw.d_exon_bases != nullptr && c.raw.d_unexplained_bases != nullptr);
   sbgpu_bins_destroy(bins);
   return 0;
}
"""
NAMES = CU.NAMES + ("exon_depth", "iso_depth")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    import e2e_util as U
    import exonbin_util as XU
    from strawberry_amd import _lib
    _lib.load()
    d_toy = getattr(U, WHICH)
    _, hits, _, _ = XU.e2e_inputs(d_toy, U.load(d_toy)[0])
    d = tmp_path_factory.mktemp("coverage_cpp")
    src, exe = d / "coverage.cpp", d / "coverage"
    src.write_text(PROGRAM.replace("@RL@", str(RL)).replace("@FRAC@", repr(MIN_FRAC)).replace("@MAPPED@", str(int(hits.total_mapped))))
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_inputs(d, annot, hits, **more):
    off = np.concatenate([[0], np.cumsum(np.bincount(hits.hit_locus, minlength=annot.n_loci))]).astype(np.int64)
    for name, dt in (("iso_off", np.int64), ("exon_off", np.int64), ("seg_off", np.int64), ("exon_left", np.uint32), ("exon_right", np.uint32),
                     ("seg_left", np.uint32), ("seg_right", np.uint32)):
        np.ascontiguousarray(getattr(annot, name)).view(dt).tofile(d / name)
    for name, dt in (("hit_locus", np.int32), ("feat_off", np.int64), ("feat_code", np.uint8), ("feat_left", np.uint32), ("feat_right", np.uint32),
                     ("mass", np.float32)):
        np.ascontiguousarray(getattr(hits, name)).view(dt).tofile(d / name)
    off.tofile(d / "hit_off")
    for name, (a, dt) in more.items():
        np.ascontiguousarray(a, dt).tofile(d / name)
    return off


def run(program, d, mode):
    out = subprocess.run(["timeout", "-k", "10", "120", str(program), str(d), mode], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = {}
    for line in out.stdout.split("\n"):
        if line:
            name, *vals = line.split()
            got.setdefault(name, []).extend(vals)
    shape = got.pop("shape")
    assert set(got) == set(NAMES)
    return {k: np.array([float.fromhex(x) for x in v]) for k, v in got.items()}, shape


def test_host_program_gives_the_python_bindings_arrays(oracle, program, tmp_path):
    from strawberry_amd import coverage
    from test_context_table import Handle, toy_inputs
    _, _, _, annot, hits, _, compat, key, bins, F, status, ab = toy_inputs(oracle, WHICH)
    theta, _, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    write_inputs(tmp_path, annot, hits, compat=(compat, np.uint32), key=(key, np.uint32), F=(F, np.float64), theta=(theta, np.float64),
                 keep=(ab["keep"], np.int32), status=(status, np.int32))
    got, shape = run(program, tmp_path, "host")
    assert shape == ["0"]                   # the host form names no device array
    with Handle(annot, hits, compat, key) as H:
        t = coverage.isoform_coverage_host(H.h, annot, hits, compat, theta, F=F, keep=ab["keep"], status=status, hit_mass=hits.mass)
    for k in CU.NAMES:
        assert got[k].tobytes() == getattr(t, k).tobytes(), k
    assert got["exon_depth"].tobytes() == t.exon_depth(annot).tobytes() and got["iso_depth"].tobytes() == t.iso_depth(annot).tobytes()
    assert (t.iso_bases > 0.0).any() and (t.junction_mass > 0.0).any() and (t.iso_bases[np.asarray(ab["keep"]) == 0] == 0.0).all()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_arrays(program, tmp_path):
    import e2e_util as U
    import exonbin_util as XU
    from strawberry_amd import em
    from strawberry_amd.quantify import InsertSize, quantify_resident
    d_toy = getattr(U, WHICH)
    annot, hits, _, _ = XU.e2e_inputs(d_toy, U.load(d_toy)[0])
    write_inputs(tmp_path, annot, hits)
    got, shape = run(program, tmp_path, "device")
    assert shape == ["1"]
    r = quantify_resident(annot, hits, InsertSize(250.0, 30.0), RL, hits.total_mapped, ctx=em.default_context(0), min_isoform_frac=MIN_FRAC,
                          with_coverage=True)
    c = r["coverage"]

    class Got:
        pass
    g = Got()
    for k in CU.NAMES:
        setattr(g, k, got[k])
    CU.compare(g, c, annot, hits.hit_locus, False, "the C++ program's device form")
    np.testing.assert_array_equal(got["iso_bases"], CU.iso_bases_of(got["exon_bases"], annot))
    assert got["exon_depth"].tobytes() == g.exon_bases.__truediv__(annot.exon_right.astype(np.float64) - annot.exon_left.astype(np.float64) + 1.0).tobytes()
    assert (c.iso_bases > 0.0).any() and (c.iso_bases[r["keep"] == 0] == 0.0).all()
