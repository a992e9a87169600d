"""The C++ layer of the fragment assignment: a C++14 program makes a resident call on one toy directory's unique hits with
retention on and runs sbgpu::FragmentAssignment::device, then sbgpu_quantify_host on the same hits and
sbgpu::FragmentAssignment::host on its handle (include/sbgpu_host.hpp).  Without a GPU it only has to compile and link; with
one it runs, and its arrays are those of the Python binding (quantify_resident(with_assignment=True), quantify_host(assignment_theta=...))."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL, WHICH, MIN_FRAC = 75, "E2E_FILTER", 0.05

PROGRAM = r"""#include <hip/hip_runtime_api.h>
#include <algorithm>
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
void print(const std::string &name, const std::vector<int32_t> &v)
{
   for (int32_t x : v) std::printf("%s %d\n", name.c_str(), x);
}
void print(const std::string &name, const std::vector<int64_t> &v)
{
   for (int64_t x : v) std::printf("%s %lld\n", name.c_str(), (long long)x);
}
void print_all(const std::string &p, const sbgpu::FragmentAssignment &a)
{
   print(p + "map_iso", a.map_iso), print(p + "n_cand", a.n_cand), print(p + "map_prob", a.map_prob);
   print(p + "unique_mass", a.unique_mass), print(p + "map_mass", a.map_mass), print(p + "post_mass", a.post_mass);
   print(p + "unassigned", a.unassigned);
}
int main(int argc, char **argv)
{
   if (argc < 2) return 2;
   const std::string d = std::string(argv[1]) + "/";
   sbgpu::Context ctx(0);
   const auto iso_off = load<int64_t>(d + "iso_off"), exon_off = load<int64_t>(d + "exon_off"), seg_off = load<int64_t>(d + "seg_off");
   const auto exon_left = load<uint32_t>(d + "exon_left"), exon_right = load<uint32_t>(d + "exon_right");
   const auto seg_left = load<uint32_t>(d + "seg_left"), seg_right = load<uint32_t>(d + "seg_right");
   const auto hit_locus = load<int32_t>(d + "hit_locus");
   const auto feat_off = load<int64_t>(d + "feat_off"), hit_off = load<int64_t>(d + "hit_off");
   const auto feat_code = load<uint8_t>(d + "feat_code");
   const auto feat_left = load<uint32_t>(d + "feat_left"), feat_right = load<uint32_t>(d + "feat_right");
   const auto mass = load<float>(d + "mass");
   const int64_t n_loci = (int64_t)iso_off.size() - 1, n_hits = (int64_t)hit_locus.size(), n_iso = iso_off[(size_t)n_loci];
   int64_t max_iso = 1;
   for (int64_t l = 0; l < n_loci; ++l) max_iso = std::max(max_iso, iso_off[(size_t)l + 1] - iso_off[(size_t)l]);
   const int32_t cw = (int32_t)((max_iso + 31) / 32);
   const sbgpu_annotation_t an = {n_loci, iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(), seg_off.data(), seg_left.data(), seg_right.data()};
   const sbgpu_hits_t d_hits = {n_hits, up(hit_locus), up(feat_off), up(feat_code), up(feat_left), up(feat_right)};
   const sbgpu_hits_t h_hits = {n_hits, hit_locus.data(), feat_off.data(), feat_code.data(), feat_left.data(), feat_right.data()};
   const float *d_mass = up(mass);
   sbgpu_insert_t ins = {};
   ins.mean = 250.0, ins.sd = 30.0, ins.read_len = @RL@;
   const sbgpu_abundance_params_t par = {0, 0, 1, 0, 0.0, @FRAC@};
   std::vector<double> theta((size_t)n_iso + 1);
   std::vector<int32_t> keep((size_t)n_iso + 1), status((size_t)n_loci + 1);
   sbgpu_abundances_t out = {};
   out.theta = theta.data(), out.keep = keep.data(), out.status = status.data();
   sbgpu_insert_t used = {};
   sbgpu_bins_t *bins = nullptr;
   sbgpu::ContextTable::keep(ctx, true);
   sbgpu::check(sbgpu_quantify_resident(ctx.get(), &an, &d_hits, d_mass, hit_off.data(), &ins, @RL@, 0, @MAPPED@, &par, nullptr, &used, &out, &bins),
                "sbgpu_quantify_resident");
   sbgpu::ContextTable::keep(ctx, false);
   const sbgpu::FragmentAssignment dev = sbgpu::FragmentAssignment::device(ctx, bins, n_hits, out.d_theta, d_mass);
   print_all("dev_", dev);
   std::printf("shape %lld %d\n", (long long)dev.raw.n_hits, dev.raw.d_post_mass != nullptr);
   sbgpu_bins_destroy(bins);
   /* the host form on the host entry's handle over the same hits, under the resident call's theta, keep and status */
   std::vector<double> theta_h((size_t)n_iso + 1);
   std::vector<int32_t> status_h((size_t)n_loci + 1), iters_h((size_t)n_loci + 1);
   std::vector<uint32_t> compat((size_t)n_hits * cw + 1);
   sbgpu::check(sbgpu_quantify_host(ctx.get(), &an, &h_hits, mass.data(), &ins, @RL@, 0, theta_h.data(), status_h.data(), iters_h.data(), compat.data(), &used,
                                    &bins),
                "sbgpu_quantify_host");
   const sbgpu::FragmentAssignment host =
      sbgpu::FragmentAssignment::host(bins, n_hits, compat.data(), cw, nullptr, theta.data(), keep.data(), status.data(), mass.data());
   print_all("host_", host);
   sbgpu_bins_destroy(bins);
   return 0;
}
"""
NAMES = ("map_iso", "n_cand", "map_prob", "unique_mass", "map_mass", "post_mass", "unassigned")


def sample():
    import e2e_util as U
    import exonbin_util as XU
    d = getattr(U, WHICH)
    ordered = U.load(d)[0]
    annot, hits, _, _ = XU.e2e_inputs(d, ordered)
    return annot, hits


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from strawberry_amd import _lib
    _lib.load()
    _, hits = sample()
    d = tmp_path_factory.mktemp("assign_cpp")
    src, exe = d / "assign.cpp", d / "assign"
    src.write_text(PROGRAM.replace("@RL@", str(RL)).replace("@FRAC@", repr(MIN_FRAC)).replace("@MAPPED@", str(int(hits.total_mapped))))
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds(program):
    assert os.path.exists(program)


@pytest.mark.gpu
def test_program_gives_the_python_bindings_arrays(program, tmp_path):
    from strawberry_amd import em
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    annot, hits = sample()
    off = np.concatenate([[0], np.cumsum(np.bincount(hits.hit_locus, minlength=annot.n_loci))]).astype(np.int64)
    for name, dt in (("iso_off", np.int64), ("exon_off", np.int64), ("seg_off", np.int64), ("exon_left", np.uint32), ("exon_right", np.uint32),
                     ("seg_left", np.uint32), ("seg_right", np.uint32)):
        np.ascontiguousarray(getattr(annot, name)).view(dt).tofile(tmp_path / name)
    for name, dt in (("hit_locus", np.int32), ("feat_off", np.int64), ("feat_code", np.uint8), ("feat_left", np.uint32), ("feat_right", np.uint32),
                     ("mass", np.float32)):
        np.ascontiguousarray(getattr(hits, name)).view(dt).tofile(tmp_path / name)
    off.tofile(tmp_path / "hit_off")
    out = subprocess.run(["timeout", "-k", "10", "120", str(program), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = {}
    for line in out.stdout.split("\n"):
        if line:
            name, *vals = line.split()
            got.setdefault(name, []).extend(vals)
    ctx = em.default_context(0)
    law = InsertSize(250.0, 30.0)
    r = quantify_resident(annot, hits, law, RL, hits.total_mapped, ctx=ctx, min_isoform_frac=MIN_FRAC, with_assignment=True)
    h = quantify_host(annot, hits, law, RL, ctx=ctx, assignment_theta=r["theta"], assignment_keep=r["keep"], assignment_status=r["status"])
    assert got["shape"] == [str(hits.n_hits), "1"]
    assert set(got) == {"shape"} | {p + k for p in ("dev_", "host_") for k in NAMES}
    for prefix, a in (("dev_", r["assignment"]), ("host_", h["assignment"])):
        for k in NAMES:
            w = getattr(a, k)
            if w.dtype == np.float64:
                # (the device form's post_mass is a sum by atomics: the C++ run and the Python run may order it differently)
                g = np.array([float.fromhex(x) for x in got[prefix + k]])
                if prefix == "dev_" and k == "post_mass":
                    hits_of = np.repeat(np.diff(off), np.diff(annot.iso_off))
                    assert (np.abs(g - w) <= (hits_of + 8) * 2.0 ** -52 * w).all(), k
                else:
                    assert g.tobytes() == w.tobytes(), prefix + k
            else:
                assert [int(x) for x in got[prefix + k]] == w.tolist(), prefix + k
    assert int((r["assignment"].n_cand == 0).sum()) == 13
