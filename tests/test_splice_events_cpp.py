"""The C++ side of the splicing events.  One stand-alone C++14 program with a main of its own, through sbgpu::SpliceEvents and
sbgpu::SplicePsi::host (include/sbgpu_host.hpp), over the sample of tests/splice_util.py:
`linked`: against libsbgpu.so -- the table, PSI with and without keep, defined_count and the support are the bytes of the Python binding's;
`sanitized`: the same program together with csrc/splice_host.cpp (free of HIP; the program supplies the library's error slot), compiled by
g++ with AddressSanitizer and UBSan and run on the CPU: clean, and the same bytes.  Nothing sanitized is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import splice_util as SU
from strawberry_amd import _lib, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SMALL = 40
N_ROWS = 3
INTS = ("event_off", "event_locus", "event_kind", "event_left", "event_right", "event_flags", "n_span", "incl_off", "incl_iso", "incl_exon", "iso_off",
        "iso_left", "iso_right", "defined_keep", "defined_all")
FLOATS = ("psi_keep", "psi_all", "support", "support_exons")

PROGRAM = r"""#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "sbgpu_host.hpp"
#ifdef SB_STANDALONE
// the library's error slot, for csrc/splice_host.cpp compiled beside this file
static std::string last_error;
namespace sb {
int api_fail(int code, const std::string &msg)
{
   last_error = msg;
   return code;
}
}
extern "C" const char *sbgpu_last_error(void) { return last_error.c_str(); }
#endif
template <class T> std::vector<T> load(const std::string &path)
{
   std::ifstream f(path, std::ios::binary | std::ios::ate);
   if (!f) throw std::runtime_error("cannot read " + path);
   std::vector<T> v((size_t)f.tellg() / sizeof(T));
   f.seekg(0);
   f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
   return v;
}
template <class T> void ints(const char *name, const std::vector<T> &v)
{
   for (T x : v) std::printf("%s %lld\n", name, (long long)x);
}
void floats(const char *name, const std::vector<double> &v)
{
   for (double x : v) std::printf("%s %a\n", name, x);
}
int main(int argc, char **argv)
{
   if (argc < 2) return 2;
   const std::string d = std::string(argv[1]) + "/";
   const auto iso_off = load<int64_t>(d + "iso_off"), exon_off = load<int64_t>(d + "exon_off");
   auto exon_left = load<uint32_t>(d + "exon_left"), exon_right = load<uint32_t>(d + "exon_right");
   const auto x = load<double>(d + "x"), exon_bases = load<double>(d + "exon_bases"), junction_mass = load<double>(d + "junction_mass");
   const auto keep = load<int32_t>(d + "keep");
   const int64_t n_loci = (int64_t)iso_off.size() - 1, n_iso = iso_off[(size_t)n_loci];
   const int64_t n_rows = n_iso ? (int64_t)x.size() / n_iso : 0;
   const sbgpu_annotation_t an = {n_loci, iso_off.data(), exon_off.data(), exon_left.data(), exon_right.data(), nullptr, nullptr, nullptr};
   const sbgpu::SpliceEvents built(an);
   const sbgpu::SpliceEvents ev(built);      // (a copy names its own vectors)
   if (ev.raw.event_off != ev.event_off.data() || ev.raw.event_off == built.raw.event_off) return 3;
   ints("event_off", ev.event_off), ints("event_locus", ev.event_locus), ints("event_kind", ev.event_kind), ints("event_left", ev.event_left);
   ints("event_right", ev.event_right), ints("event_flags", ev.event_flags), ints("n_span", ev.n_span), ints("incl_off", ev.incl_off);
   ints("incl_iso", ev.incl_iso), ints("incl_exon", ev.incl_exon), ints("iso_off", ev.iso_off), ints("iso_left", ev.iso_left), ints("iso_right", ev.iso_right);
   const sbgpu::SplicePsi with_keep = sbgpu::SplicePsi::host(ev, n_rows, x.data(), keep.data()), all = sbgpu::SplicePsi::host(ev, n_rows, x.data());
   floats("psi_keep", with_keep.psi), ints("defined_keep", with_keep.defined_count);
   floats("psi_all", all.psi), ints("defined_all", all.defined_count);
   floats("support", sbgpu::SplicePsi::support_host(ev, exon_bases.data(), junction_mass.data()));
   floats("support_exons", sbgpu::SplicePsi::support_host(ev, exon_bases.data(), nullptr));
   int64_t alternative = 0;
   for (int64_t u = 0; u < ev.n_events(); ++u) alternative += ev.alternative(u);
   std::printf("counts %lld %lld %lld %lld\n", (long long)ev.raw.n_events, (long long)ev.raw.n_incl, (long long)ev.raw.n_exons, (long long)alternative);
   // no rows: nothing is written
   if (!sbgpu::SplicePsi::host(ev, 0, nullptr).psi.empty()) return 4;
   // an isoform whose second exon begins inside its first is refused, with the reason
   if (exon_left.size() > 1) {
      exon_left[1] = exon_left[0];
      try {
         sbgpu::SpliceEvents bad(an);
         return 5;
      } catch (const sbgpu::Error &e) {
         if (e.code != SBGPU_EINVAL || !std::strstr(e.what(), "not ascending and disjoint")) return 6;
      }
   }
   return 0;
}
"""


def parse(text):
    got = {}
    for line in text.split("\n"):
        if line:
            name, val = line.split(None, 1)
            got.setdefault(name, []).append(val)
    out = {k: np.array([int(v) for v in got.get(k, [])], np.int64) for k in INTS}
    out.update({k: np.array([float.fromhex(v) for v in got.get(k, [])], np.float64) for k in FLOATS})
    out["counts"] = [int(v) for v in got["counts"][0].split()]
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    annot, loci, at = SU.splice_annotation(N_SMALL)
    ev = splice.SpliceEvents.build(annot)
    x, keep = SU.random_rows(N_ROWS, ev.n_iso, 77)
    keep[:, int(annot.iso_off[at["cassette"]]):int(annot.iso_off[at["cassette"] + 1])] = 0
    x[1, int(annot.iso_off[at["W65"]]) + 2] = np.nan
    rng = np.random.default_rng(78)
    xb, jm = rng.gamma(2.0, 50.0, ev.n_exons), rng.gamma(1.0, 3.0, ev.n_exons)
    d = tmp_path_factory.mktemp("splice_cpp")
    assert loci[0] and len(loci[0][0]) > 1          # (the refusal the program provokes spoils the first isoform's second exon)
    for name, a, dt in (("iso_off", annot.iso_off, np.int64), ("exon_off", annot.exon_off, np.int64), ("exon_left", annot.exon_left, np.uint32),
                        ("exon_right", annot.exon_right, np.uint32), ("x", x, np.float64), ("keep", keep, np.int32), ("exon_bases", xb, np.float64),
                        ("junction_mass", jm, np.float64)):
        np.ascontiguousarray(a, dt).tofile(str(d / name))
    psi_keep, def_keep = splice.splice_psi_host(ev, x, keep)
    psi_all, def_all = splice.splice_psi_host(ev, x)
    want = {k: np.asarray(getattr(ev, k), np.int64) for k in INTS[:13]}
    want.update(defined_keep=def_keep.astype(np.int64), defined_all=def_all.astype(np.int64), psi_keep=psi_keep.reshape(-1), psi_all=psi_all.reshape(-1),
                support=splice.splice_support_host(ev, xb, jm), support_exons=splice.splice_support_host(ev, xb, None))
    assert np.isnan(psi_keep).any() and (def_keep != def_all).any()
    return dict(dir=d, ev=ev, want=want)


def same_as_the_binding(out, case):
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    got, want, ev = parse(out.stdout), case["want"], case["ev"]
    assert got["counts"] == [ev.n_events, ev.n_incl, ev.n_exons, int(ev.alternative().sum())]
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in FLOATS:
        SU.same_bits(got[k], want[k], k)


def test_linked_program_gives_the_python_bindings_bytes(case):
    _lib.load()
    src, exe = case["dir"] / "splice.cpp", case["dir"] / "splice"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    same_as_the_binding(subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120), case)


def test_the_program_and_the_host_form_under_the_sanitizers(case):
    """csrc/splice_host.cpp and csrc/splice_rules.h need neither HIP nor the library: g++ builds them with ASan and UBSan beside the program"""
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    src, exe = case["dir"] / "sanitized.cpp", case["dir"] / "sanitized"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSB_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", csrc, str(src), os.path.join(csrc, "splice_host.cpp"), "-o", str(exe)])
    same_as_the_binding(subprocess.run([str(exe), str(case["dir"])], capture_output=True, text=True, timeout=120), case)
