"""The C++ side of the transcript-body coverage profile.
`sanitized`: csrc/body_host.cpp's rule on plain arrays (sb::body_profile_arrays) and csrc/body_rules.h -- free of HIP -- compiled by
g++ with AddressSanitizer and UBSan into a stand-alone program with a main of its own (which supplies the library's error slot), run
over one toy directory's arrays, over an isoform shorter than its bins (L < P) and over one of 2^26 bases at P = 100
(L * P > 2^32): clean, the toy's bytes those of the Python binding's, the two others their closed forms.  Nothing is loaded into Python.
`host`: sbgpu::BodyProfile::host (include/sbgpu_host.hpp) from a C++14 program on the same toy: the bytes of body.body_profile_host.
`device`: a resident call with retention on, then sbgpu::BodyProfile::device -- against quantify_resident(with_body_profile=True)'s
within the device-to-device bound."""
import os
import subprocess

import numpy as np
import pytest

import body_util as BU
from test_isoform_coverage_cpp import MIN_FRAC, RL, WHICH, write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 20
FLOATS = ("body_bases", "body_total", "body_center", "body_cv", "class_profile")

COMMON = r"""
template <class T> std::vector<T> load(const std::string &path)
{
   std::ifstream f(path, std::ios::binary | std::ios::ate);
   if (!f) throw std::runtime_error("cannot read " + path);
   std::vector<T> v((size_t)f.tellg() / sizeof(T));
   f.seekg(0);
   f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
   return v;
}
void print(const std::string &name, const std::vector<double> &v)
{
   for (double x : v) std::printf("%s %a\n", name.c_str(), x);
}
"""

SANITIZED = r"""#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "body_rules.h"
#include "stage_host.h"
static std::string last_error;
namespace sb {
int api_fail(int code, const std::string &msg)
{
   last_error = msg;
   return code;
}
}
""" + COMMON + r"""
// exactly sized arrays: a write past an array's end is the sanitizer's to see
struct Out {
   std::vector<double> bases, total, center, cv, prof;
   std::vector<int64_t> n;
   sbgpu_body_profile_t raw{};
   Out(int64_t n_iso, int P) : bases((size_t)(n_iso * P)), total((size_t)n_iso), center((size_t)n_iso), cv((size_t)n_iso), prof((size_t)(4 * P)), n(4)
   {
      raw.body_bases = bases.data(), raw.body_total = total.data(), raw.body_center = center.data(), raw.body_cv = cv.data();
      raw.class_profile = prof.data(), raw.class_n = n.data();
   }
   void show(const std::string &tag) const
   {
      print(tag + "body_bases", bases), print(tag + "body_total", total), print(tag + "body_center", center), print(tag + "body_cv", cv);
      print(tag + "class_profile", prof);
      for (int64_t x : n) std::printf("%sclass_n %lld\n", tag.c_str(), (long long)x);
   }
};
// one locus of one isoform of one exon [1, L], one bin of weight 0.5, theta 1: the reads are single blocks
int one_exon(const std::string &tag, uint32_t L, int P, int strand, const std::vector<uint32_t> &rl, const std::vector<uint32_t> &rr)
{
   const int64_t nh = (int64_t)rl.size();
   const int64_t off2[2] = {0, 1}, hoff[2] = {0, nh};
   const uint32_t xl = 1, xr = L;
   std::vector<int64_t> hit_bin((size_t)nh, 0), feat_off((size_t)nh + 1);
   std::vector<uint8_t> code((size_t)nh, 0);
   std::vector<uint32_t> compat((size_t)nh, 1u);
   for (int64_t h = 0; h <= nh; ++h) feat_off[(size_t)h] = h;
   const double F = 0.5, theta = 1.0;
   const uint8_t s = (uint8_t)strand;
   sb::BodyHostIn in{};
   in.n_loci = 1, in.n_hits = nh, in.n_bins = 1;
   in.row_off = off2, in.iso_off = off2, in.f_off = off2, in.locus_hit_off = hoff, in.hit_bin = hit_bin.data();
   in.exon_off = off2, in.exon_left = &xl, in.exon_right = &xr;
   in.feat_off = feat_off.data(), in.feat_code = code.data(), in.feat_left = rl.data(), in.feat_right = rr.data();
   in.compat = compat.data(), in.compat_words = 1, in.F = &F, in.theta = &theta, in.iso_strand = &s, in.n_pos = P;
   Out o(1, P);
   if (sb::body_profile_arrays(in, &o.raw) != SBGPU_OK) return 1;
   o.show(tag);
   // an exon that ends before it begins is refused, not walked
   const uint32_t bad = 0;
   in.exon_right = &bad;
   if (sb::body_profile_arrays(in, &o.raw) != SBGPU_EINVAL || last_error.find("ends before it begins") == std::string::npos) return 2;
   return 0;
}
int main(int argc, char **argv)
{
   if (argc < 2) return 2;
   {  // the device form's arena (csrc/stage_host.h: body_layout), written out by hand: every entry rounded up to 256 bytes
      const sb::BodyLayout L = sb::body_layout(40, 300, 70, 500, 30, 20, true);
      if (L.roff != 0 || L.ioff != 512 || L.foff != 1024 || L.items != 1536 || L.eoff != 2304 || L.eleft != 3072 || L.eright != 5120) return 10;
      if (L.epre != 7168 || L.ilen != 11264 || L.strand != 12032 || L.upload_bytes != 12288 || L.live != 12288 || L.gain != 12800) return 11;
      if (L.bases != 13568 || L.cprof != 25088 || L.cn != 25856 || L.sums_bytes != 12544 || L.total != 26112 || L.center != 26880 || L.cv != 27648) return 12;
      if (L.bytes != 28416 || sb::body_layout(40, 300, 70, 500, 30, 20, false).bytes != L.bytes - 768 - 2048 - 2048) return 13;
   }
   const std::string d = std::string(argv[1]) + "/";
   const auto row_off = load<int64_t>(d + "row_off"), iso_off = load<int64_t>(d + "iso_off"), f_off = load<int64_t>(d + "f_off");
   const auto hit_off = load<int64_t>(d + "hit_off"), hit_bin = load<int64_t>(d + "hit_bin"), exon_off = load<int64_t>(d + "exon_off");
   const auto exon_left = load<uint32_t>(d + "exon_left"), exon_right = load<uint32_t>(d + "exon_right");
   const auto feat_off = load<int64_t>(d + "feat_off");
   const auto feat_code = load<uint8_t>(d + "feat_code"), strand = load<uint8_t>(d + "strand");
   const auto feat_left = load<uint32_t>(d + "feat_left"), feat_right = load<uint32_t>(d + "feat_right"), compat = load<uint32_t>(d + "compat");
   const auto F = load<double>(d + "F"), theta = load<double>(d + "theta");
   const auto keep = load<int32_t>(d + "keep"), status = load<int32_t>(d + "status");
   const auto mass = load<float>(d + "mass");
   sb::BodyHostIn in{};
   in.n_loci = (int64_t)iso_off.size() - 1, in.n_hits = (int64_t)hit_bin.size(), in.n_bins = row_off.back();
   in.row_off = row_off.data(), in.iso_off = iso_off.data(), in.f_off = f_off.data(), in.locus_hit_off = hit_off.data(), in.hit_bin = hit_bin.data();
   in.exon_off = exon_off.data(), in.exon_left = exon_left.data(), in.exon_right = exon_right.data();
   in.feat_off = feat_off.data(), in.feat_code = feat_code.data(), in.feat_left = feat_left.data(), in.feat_right = feat_right.data();
   in.compat = compat.data(), in.compat_words = (int32_t)(compat.size() / hit_bin.size());
   in.F = F.data(), in.theta = theta.data(), in.keep = keep.data(), in.status = status.data(), in.hit_mass = mass.data();
   in.iso_strand = strand.data(), in.n_pos = @P@;
   Out o(iso_off.back(), @P@);
   if (sb::body_profile_arrays(in, &o.raw) != SBGPU_OK) {
      std::printf("%s\n", last_error.c_str());
      return 4;
   }
   o.show("toy.");
   const uint32_t big = 1u << 26, half = 1u << 25;
   if (int rc = one_exon("short.", 7, 20, 2, {1, 3}, {7, 5})) return 20 + rc;
   if (int rc = one_exon("long.", big, 100, 0, {1, half - 32, big - 99}, {100, half + 68, big})) return 30 + rc;
   return 0;
}
"""

PROGRAM = r"""#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstring>
#include <fstream>
#include "sbgpu_host.hpp"
""" + COMMON + r"""
template <class T> const T *up(const std::vector<T> &v)
{
   void *p = nullptr;
   if (hipMalloc(&p, v.size() * sizeof(T) + 8) != hipSuccess || hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("upload");
   return (const T *)p;
}
void print_all(const sbgpu::BodyProfile &c)
{
   print("toy.body_bases", c.body_bases), print("toy.body_total", c.body_total), print("toy.body_center", c.body_center), print("toy.body_cv", c.body_cv);
   print("toy.class_profile", c.class_profile);
   for (int64_t x : c.class_n) std::printf("toy.class_n %lld\n", (long long)x);
   for (int k = 0; k < 4; ++k) print("toy.class_curve", c.class_curve(k));
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
   const auto feat_code = load<uint8_t>(d + "feat_code"), strand = load<uint8_t>(d + "strand");
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
      const sbgpu::BodyProfile c =
         sbgpu::BodyProfile::host(bins, an, h_hits, compat.data(), cw, F.data(), theta.data(), keep.data(), status.data(), mass.data(), strand.data(), @P@);
      print_all(c);
      std::printf("shape %d\n", c.raw.d_body_bases != nullptr);
      try {
         sbgpu::BodyProfile::host(bins, an, h_hits, compat.data(), cw, F.data(), theta.data(), keep.data(), status.data(), mass.data(), strand.data(), 101);
         return 4;
      } catch (const std::exception &e) {
         if (!std::strstr(e.what(), "n_pos must be 1 .. 100")) return 5;
      }
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
   const sbgpu::BodyProfile c = sbgpu::BodyProfile::device(ctx, bins, an, d_hits, out.d_theta, d_mass, strand.data(), @P@);
   print_all(c);
   std::printf("shape %d\n", c.raw.d_body_bases != nullptr && c.raw.d_class_n != nullptr && c.raw.body_bases == nullptr);
   sbgpu_bins_destroy(bins);
   return 0;
}
"""


def parse(text, tag):
    got = {}
    for line in text.split("\n"):
        if line.startswith(tag):
            name, val = line[len(tag):].split()
            got.setdefault(name, []).append(val)
    out = {k: np.array([float.fromhex(x) for x in v]) for k, v in got.items() if k != "class_n"}
    out["class_n"] = np.array([int(x) for x in got["class_n"]], np.int64)
    return out


@pytest.fixture(scope="module")
def toy(oracle, tmp_path_factory):
    from strawberry_amd import body
    from test_context_table import Handle, toy_inputs
    _, _, _, annot, hits, _, compat, key, bins, F, status, ab = toy_inputs(oracle, WHICH)
    theta, _, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    strand = BU.strands_of(annot)
    d = tmp_path_factory.mktemp("body_cpp")
    write_inputs(d, annot, hits, compat=(compat, np.uint32), key=(key, np.uint32), F=(F, np.float64), theta=(theta, np.float64), keep=(ab["keep"], np.int32),
                 status=(status, np.int32), strand=(strand, np.uint8), row_off=(bins.row_off, np.int64), f_off=(bins.f_off, np.int64),
                 hit_bin=(bins.hit_bin, np.int64))
    with Handle(annot, hits, compat, key) as H:
        t = body.body_profile_host(H.h, annot, hits, compat, theta, F=F, keep=ab["keep"], status=status, hit_mass=hits.mass, iso_strand=strand, n_pos=P)
    assert (t.body_total > 0.0).any() and (t.body_total[np.asarray(ab["keep"]) == 0] == 0.0).all() and (strand == 2).any()
    return dict(dir=d, annot=annot, hits=hits, t=t, strand=strand)


def same_bytes(got, t):
    for k in FLOATS:
        assert got[k].tobytes() == np.ascontiguousarray(getattr(t, k)).tobytes(), k
    assert got["class_n"].tolist() == t.class_n.tolist()


def test_the_rule_on_plain_arrays_under_the_sanitizers(toy):
    """csrc/body_host.cpp's body_profile_arrays and csrc/body_rules.h need neither HIP nor the library: g++ builds them with ASan and
    UBSan beside a main of its own"""
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = toy["dir"] / "sanitized.cpp", toy["dir"] / "sanitized"
    src.write_text(SANITIZED.replace("@P@", str(P)))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DSB_BODY_ARRAYS_ONLY", "-I", csrc, str(src), os.path.join(csrc, "body_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(toy["dir"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    same_bytes(parse(out.stdout, "toy."), toy["t"])
    # L = 7 < P = 20 on strand 2: the mirror image of q = 0, 2, 5, 8, 11, 14, 17 holding 1, 1, 2, 2, 2, 1, 1 bases
    short = parse(out.stdout, "short.")
    want = np.zeros(20)
    want[[0, 2, 5, 8, 11, 14, 17]] = [1, 1, 2, 2, 2, 1, 1]
    assert short["body_bases"].tolist() == want[::-1].tolist() and short["body_total"].tolist() == [10.0] and short["class_n"].tolist() == [1, 0, 0, 0]
    d = np.array([1, 1, 2, 2, 2, 1, 1], float)
    assert short["body_cv"][0] == np.sqrt(((d - d.sum() / 7.0) ** 2).sum() / 7.0) / (d.sum() / 7.0)
    # L = 2^26, P = 100: the 64-bit division; bin 50 begins at t = 2^25
    long_ = parse(out.stdout, "long.")
    b = long_["body_bases"]
    assert b[0] == 100.0 and b[99] == 100.0 and b[49] == 33.0 and b[50] == 68.0 and b.sum() == 301.0 and long_["class_n"].tolist() == [0, 0, 0, 1]


@pytest.fixture(scope="module")
def program(toy):
    import e2e_util as U
    import exonbin_util as XU
    from strawberry_amd import _lib
    _lib.load()
    d_toy = getattr(U, WHICH)
    _, hits, _, _ = XU.e2e_inputs(d_toy, U.load(d_toy)[0])
    src, exe = toy["dir"] / "body.cpp", toy["dir"] / "body"
    src.write_text(PROGRAM.replace("@RL@", str(RL)).replace("@FRAC@", repr(MIN_FRAC)).replace("@MAPPED@", str(int(hits.total_mapped))).replace("@P@", str(P)))
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(program, d, mode):
    out = subprocess.run(["timeout", "-k", "10", "120", str(program), str(d), mode], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    shape = [line.split()[1] for line in out.stdout.split("\n") if line.startswith("shape")]
    return parse(out.stdout, "toy."), shape


def test_host_program_gives_the_python_bindings_bytes(toy, program):
    got, shape = run(program, toy["dir"], "host")
    assert shape == ["0"]                   # the host form names no device array
    same_bytes(got, toy["t"])
    t = toy["t"]
    assert got["class_curve"].tobytes() == np.concatenate([t.class_curve(c) for c in range(4)]).tobytes()


@pytest.mark.gpu
def test_device_program_gives_the_python_bindings_arrays(toy, program):
    from strawberry_amd import em
    from strawberry_amd.quantify import InsertSize, quantify_resident
    annot, hits, strand = toy["annot"], toy["hits"], toy["strand"]
    got, shape = run(program, toy["dir"], "device")
    assert shape == ["1"]
    r = quantify_resident(annot, hits, InsertSize(250.0, 30.0), RL, hits.total_mapped, ctx=em.default_context(0), min_isoform_frac=MIN_FRAC,
                          with_body_profile=True, iso_strand=strand, n_pos=P)
    c = r["body_profile"]
    BU.compare(got, c, annot, hits.hit_locus, False, "the C++ program's device form", P, strand)
    assert (c.body_total > 0.0).any() and (c.body_total[r["keep"] == 0] == 0.0).all()
