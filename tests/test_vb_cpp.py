"""The variational Bayes solve's host form (sbgpu_em_vb_host, csrc/vb_host.cpp; CPU, no GPU needed) against tests/vb_util.py's
restatement: on the five EM goldens at alpha = 0.01 and 1 -- which measures the yardstick the device's bounds are made of --
and on every other sample tests/test_vb_gpu.py uses; the rule's digamma through a stand-alone probe over csrc/vb_rules.h against
the restatement's, and against mpmath and scipy where importable; the evidence bound non-decreasing over max_iter = 1..8; the
rule's edge cases; every refusal; and a stand-alone program with its own main over vb_host.cpp, built with AddressSanitizer and
UBSan and run as a child process (nothing is preloaded)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import vb_util as V
from strawberry_amd import _lib, vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strawberry_amd", "csrc")
INC = ["-I", CSRC, "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def measured(lib, golden):
    """(golden, alpha) -> (batch, the host form's result, compare()'s figures against the restatement)"""
    out = {}
    for name in V.GOLDENS:
        b = V.golden_within_limits(golden, name)
        for alpha in V.ALPHAS:
            got = vb.em_vb_host(b, alpha=alpha)
            out[(name, alpha)] = (b, got, V.compare(got, V.solve(b, alpha=alpha), b.iso_off, V.HOST_COUNT_GAP, V.HOST_ELBO_GAP,
                                                    label="%s, alpha %g" % (name, alpha)))
    return out


@pytest.mark.parametrize("alpha", V.ALPHAS)
@pytest.mark.parametrize("name", V.GOLDENS)
def test_host_against_the_restatement_on_the_goldens(measured, name, alpha):
    b, got, worst = measured[(name, alpha)]
    print("%s, alpha %g: host against restatement |dc| / max(1, N) <= %.3e, |d elbo| / max(1, |elbo|) <= %.3e, iteration counts differ on %.2f %% of "
          "%d loci (up to %d iterations)" % (name, alpha, worst["count"], worst["elbo"], 100 * worst["differ"], b.n_loci, got.iters.max()))
    assert (got.status == V.OK).sum() > b.n_loci // 2 and (got.iters > 10).any()
    ok = got.status != V.INIT_EMPTY
    total = np.add.reduceat(np.concatenate([got.count, [0.0]]), b.iso_off[:-1])[ok]
    np.testing.assert_allclose(total, got.n_frag[ok], rtol=1e-9, atol=1e-9)          # the posterior's counts are the fragments


def test_the_yardstick_is_what_was_measured(measured):
    """HOST_COUNT_GAP and HOST_ELBO_GAP are the largest figures above, rounded up to two digits: not looser"""
    count, elbo = max(m[2]["count"] for m in measured.values()), max(m[2]["elbo"] for m in measured.values())
    print("the yardstick: count %.3e (constant %.1e), elbo %.3e (constant %.1e); the device's bounds are 100 x the constants" %
          (count, V.HOST_COUNT_GAP, elbo, V.HOST_ELBO_GAP))
    assert V.HOST_COUNT_GAP / 2 < count <= V.HOST_COUNT_GAP and V.HOST_ELBO_GAP / 2 < elbo <= V.HOST_ELBO_GAP


def test_host_against_the_restatement_on_the_other_gpu_samples(lib):
    """The threshold sample, the tiled base, the position test's pair: the iteration counts within the cap on each (here: equal).
    The yardstick is the goldens'; these samples hold shapes the goldens do not (512 isoforms in one locus), so the figures are
    printed and held to what the device is held to against the host form, 100 x the yardstick."""
    gaps = dict(count_gap=V.DEVICE_FACTOR * V.HOST_COUNT_GAP, elbo_gap=V.DEVICE_FACTOR * V.HOST_ELBO_GAP, exact_iters=True)
    b, names = V.threshold_sample()
    for alpha in V.ALPHAS:
        got, want = vb.em_vb_host(b, alpha=alpha), V.solve(b, alpha=alpha)
        print("thresholds, alpha %g:" % alpha, V.compare(got, want, b.iso_off, label="thresholds, alpha %g" % alpha, **gaps))
    at = dict(zip(names, range(len(names))))
    assert got.status[at["init empty"]] == V.INIT_EMPTY and got.iters[at["init empty"]] == 0
    assert got.status[at["no fragments"]] == V.OK and got.iters[at["no fragments"]] == 1 and got.n_active[at["inactive columns"]] == 2
    b = V.many_tiny()
    print("tiny loci:", V.compare(vb.em_vb_host(b), V.solve(b), b.iso_off, label="tiny loci", **gaps))
    b = V.from_loci([V.fast_locus(), V.slow_locus(np.random.default_rng(31))])
    got = vb.em_vb_host(b)
    print("fast and slow:", V.compare(got, V.solve(b), b.iso_off, label="fast and slow", **gaps))
    assert got.iters[0] == 2 and got.iters[1] >= 300


PROBE = r"""#include "vb_rules.h"
#include <cstdio>
int main()
{
   double x;
   while (std::scanf("%la", &x) == 1) std::printf("%a\n", sb::vb_digamma(x));
   return 0;
}
"""


@pytest.fixture(scope="module")
def rule_psi(tmp_path_factory):
    """x -> the rule's digamma (csrc/vb_rules.h compiled alone, as the library compiles it: -ffp-contract=off)"""
    d = tmp_path_factory.mktemp("vb_probe")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *INC, str(src), "-o", str(exe)])

    def f(x):
        out = subprocess.run([str(exe)], input="\n".join(float(v).hex() for v in x), capture_output=True, text=True, timeout=60, check=True)
        return np.array([float.fromhex(t) for t in out.stdout.split()])
    return f


def psi_grid():
    return np.concatenate([np.logspace(-6, 9, 601), np.arange(1, 40) / 4.0, [9.999999, 10.0, 19.999999, 20.0, 1e-6 + 0.0025]])


def test_the_rules_digamma_against_the_restatements(rule_psi):
    x = psi_grid()
    got, want = rule_psi(x), V.digamma(x)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("the rule's digamma against the restatement's: %.2e relative to max(1, |psi|)" % err.max())
    assert got.shape == x.shape and err.max() <= 3e-15


def test_the_rules_digamma_against_mpmath(rule_psi):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    x = psi_grid()
    want = np.array([float(mp.digamma(mp.mpf(float(v)))) for v in x])
    err = np.abs(rule_psi(x) - want) / np.maximum(1.0, np.abs(want))
    print("the rule's digamma against mpmath at 40 digits: %.2e relative to max(1, |psi|)" % err.max())
    assert err.max() <= 1.2e-15


def test_the_rules_digamma_against_scipy(rule_psi):
    sp = pytest.importorskip("scipy.special")
    x = psi_grid()
    want = sp.digamma(x)
    assert (np.abs(rule_psi(x) - want) / np.maximum(1.0, np.abs(want))).max() <= 3e-15


@pytest.mark.parametrize("alpha", [0.01, 0.5, 1.0])
def test_the_evidence_bound_does_not_decrease(lib, golden, alpha):
    b = V.golden_within_limits(golden, "em_random_256")
    e = np.stack([vb.em_vb_host(b, alpha=alpha, change_limit=1e-300, max_iter=k, want=("elbo", "iters", "status")).elbo for k in range(1, 9)])
    slack = 1e-12 * np.maximum(1.0, np.abs(e[:-1]))
    assert (e[1:] >= e[:-1] - slack).all(), np.nonzero((e[1:] < e[:-1] - slack).any(axis=0))[0][:8]
    assert (e[-1] > e[0]).mean() > 0.5          # (a locus of one isoform has nothing to improve)


def host_locus(locus, **kw):
    return vb.em_vb_host(V.from_loci([locus]), **kw)


def test_the_edge_cases(lib):
    t = host_locus(V.init_empty())
    assert t.status[0] == V.INIT_EMPTY and t.iters[0] == 0 and t.n_active[0] == 0 and t.n_frag[0] == 0 and t.elbo[0] == 0.0
    assert not t.count.any() and not t.share.any() and not t.share_sd.any()
    t = host_locus(V.no_fragments())
    assert t.status[0] == V.OK and t.iters[0] == 1 and t.n_frag[0] == 0 and t.n_active[0] == 2 and t.elbo[0] == 0.0
    assert not t.count.any() and not t.share.any() and not t.share_sd.any()
    t = host_locus(V.inactive_columns())
    assert t.status[0] == V.OK and t.n_active[0] == 2 and t.n_frag[0] == 51 and (t.count > 0).tolist() == [True, False, True, False]
    assert (t.share[[1, 3]] == 0).all() and (t.share_sd[[1, 3]] == 0).all() and abs(t.share.sum() - 1.0) < 1e-12
    # a zero-count bin private to an isoform that dies: no 0 / 0
    t = host_locus(V.dying_private_bin(), **V.DYING_PARAMS)
    want = V.solve_locus(*V.dying_private_bin(), **V.DYING_PARAMS)
    assert t.status[0] == V.OK and t.count[1] == 0.0 and t.count[0] == 100003.0 and np.isfinite(t.elbo[0]) and t.share[1] > 0.0
    assert not np.isnan(np.concatenate([t.count, t.share, t.share_sd])).any() and t.iters[0] == want["iters"]
    # a counted bin whose isoforms all underflow
    t = host_locus(V.underflowing_bin(), **V.UNDERFLOW_PARAMS)
    assert t.status[0] == V.DENOM_ZERO and t.iters[0] == 2 and t.elbo[0] == -math.inf and t.n_active[0] == 401 and t.n_frag[0] == 1000001
    np.testing.assert_allclose(t.count[:400], 1.0 / 400, rtol=1e-12)
    # max_iter <= 3: the iteration counts are exact
    t = host_locus(V.fast_locus(), max_iter=3)
    assert t.status[0] == V.OK and t.iters[0] == 2 and t.count.tolist() == [40.0, 60.0]
    b = V.many_tiny()
    t, want = vb.em_vb_host(b, max_iter=3), V.solve(b, max_iter=3)
    np.testing.assert_array_equal(t.iters, want["iters"])
    np.testing.assert_array_equal(t.status, want["status"])
    assert (t.status == V.MAXITER).any() and (t.iters[t.status == V.MAXITER] == 3).all()
    few = vb.em_vb_host(b, want=("count", "status"))
    assert few.share is None and few.elbo is None and few.device == {}
    np.testing.assert_array_equal(few.count, vb.em_vb_host(b).count)


def test_defaults_and_limits(lib):
    b = V.many_tiny()
    V.bitwise(vb.em_vb_host(b), vb.em_vb_host(b, alpha=0.01, change_limit=V.CHANGE_LIMIT, max_iter=V.MAX_ITER), "NULL params")
    lim = vb.limits()
    assert lim["max_bins"] == V.MAX_BINS and lim["max_iso"] == V.MAX_ISO and lim["wave"] == 64 and lim["threads"] == 256
    assert lim["wave_loci"] * lim["wave"] == lim["threads"] and lim["wave_vals"] == 512
    # the workgroup form's LDS: the buffer and the reductions' slots within the 64 KiB a kernel gets without asking, two per CU's 160 KiB
    assert lim["stage_doubles"] * 8 + 1024 <= 65536 and lim["stage_doubles"] >= V.MAX_BINS + 2 * V.MAX_ISO
    form = dict(zip(V.threshold_sample()[1], V.form_of(V.threshold_sample()[0], lim)))
    assert [form[k] for k in ("wave, full", "block, just", "staged, full", "global, just", "staged, one isoform", "global, one isoform")] == [0, 1, 1, 2, 1, 2]
    assert form["wave, one row"] == 0 and form["block, two rows"] == 1 and form["wave, one isoform"] == 0 and form["block, one isoform"] == 1
    assert form["tall"] == 2 and form["wide"] == 2 and form["1x1"] == 0
    rows, niso = V.THRESHOLD_SHAPES["staged, full"]
    assert rows * niso + rows + 2 * niso == lim["stage_doubles"]


def test_refusals(lib):
    b = V.from_loci([V.fast_locus()])

    def refused(code, text, **kw):
        with pytest.raises(_lib.SbgpuError, match=r"\(%d\).*%s" % (code, text)):
            vb.em_vb_host(b, **kw)
    for kw in (dict(alpha=0.9e-6), dict(alpha=1.1e3), dict(alpha=float("nan")), dict(change_limit=0.0), dict(change_limit=-1.0), dict(max_iter=0)):
        refused(_lib.SBGPU_EINVAL, "alpha outside", **kw)
    vb.em_vb_host(b, alpha=1e-6), vb.em_vb_host(b, alpha=1e3), vb.em_vb_host(b, max_iter=1)
    s = _lib.sbgpu_em_vb_t()
    assert lib.sbgpu_em_vb_host(None, None, C.byref(s)) == _lib.SBGPU_EINVAL and b"null argument" in lib.sbgpu_last_error()
    bt = _lib.sbgpu_batch_t(1, b.row_off.ctypes.data, b.iso_off.ctypes.data, b.f_off.ctypes.data, b.count.ctypes.data, b.F.ctypes.data)
    assert lib.sbgpu_em_vb_host(C.byref(bt), None, None) == _lib.SBGPU_EINVAL and b"null argument" in lib.sbgpu_last_error()
    assert lib.sbgpu_em_vb_limits(None) == _lib.SBGPU_EINVAL
    bad = V.from_loci([V.fast_locus()])
    bad.count = bad.count.copy()
    bad.count[1] = -1
    with pytest.raises(_lib.SbgpuError, match="a negative count"):
        vb.em_vb_host(bad)
    for field, value, text in (("row_off", [1, 3], "must begin at 0"), ("row_off", [0, -1], "do not ascend"), ("f_off", [0, 5], "not rows x isoforms")):
        off = {k: np.array(value, np.int64) if k == field else getattr(b, k) for k in ("row_off", "iso_off", "f_off")}
        bt = _lib.sbgpu_batch_t(1, off["row_off"].ctypes.data, off["iso_off"].ctypes.data, off["f_off"].ctypes.data, b.count.ctypes.data, b.F.ctypes.data)
        assert lib.sbgpu_em_vb_host(C.byref(bt), None, C.byref(s)) == _lib.SBGPU_EINVAL and text.encode() in lib.sbgpu_last_error()
    bt = _lib.sbgpu_batch_t(1, b.row_off.ctypes.data, b.iso_off.ctypes.data, b.f_off.ctypes.data, None, b.F.ctypes.data)
    assert lib.sbgpu_em_vb_host(C.byref(bt), None, C.byref(s)) == _lib.SBGPU_EINVAL and b"null count or F" in lib.sbgpu_last_error()
    # one bin or one isoform beyond the shape limits
    rng = np.random.default_rng(3)
    for shape, text in (((V.MAX_BINS + 1, 1), "more than 5632 bins"), ((1, V.MAX_ISO + 1), "more than 512 isoforms")):
        with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*" + text):
            vb.em_vb_host(V.from_loci([V.fast_locus(), V.shaped(rng, *shape)]))
    vb.em_vb_host(V.from_loci([V.shaped(rng, V.MAX_BINS, 1), V.shaped(rng, 1, V.MAX_ISO)]))


SANITIZED = r"""#include "sbgpu.h"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
namespace sb {
static std::string last;
int api_fail(int code, const std::string &msg) { last = msg; return code; }
}
struct Batch {
   std::vector<int64_t> row_off{0}, iso_off{0}, f_off{0};
   std::vector<int32_t> count;
   std::vector<double> F;
   void add(int nb, int niso, unsigned seed, double dead)
   {
      unsigned s = seed * 2654435761u + 12345u;
      auto next = [&s] { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
      for (int i = 0; i < nb; ++i) {
         count.push_back(next() < 0.2 ? 0 : (int32_t)(next() * 500));
         const bool is_dead = next() < dead;
         for (int j = 0; j < niso; ++j) F.push_back(is_dead ? 1e-7 : next() < 0.5 ? 0.0 : 0.001 + 0.3 * next());
      }
      row_off.push_back(row_off.back() + nb), iso_off.push_back(iso_off.back() + niso), f_off.push_back(f_off.back() + (int64_t)nb * niso);
   }
   sbgpu_batch_t view() const { return {(int64_t)row_off.size() - 1, row_off.data(), iso_off.data(), f_off.data(), count.data(), F.data()}; }
};
int main()
{
   Batch b;
   const int shapes[][2] = {{1, 1}, {0, 3}, {3, 0}, {0, 0}, {7, 3}, {64, 9}, {5, 512}, {5632, 2}, {33, 65}, {2, 2}};
   unsigned seed = 1;
   for (const auto &sh : shapes) b.add(sh[0], sh[1], seed++, sh[0] == 2 ? 1.0 : 0.15);
   const int64_t nl = (int64_t)b.row_off.size() - 1, ni = b.iso_off.back();
   // exact-size arrays: one entry past any of them is the sanitizer's
   std::vector<double> count((size_t)ni), share((size_t)ni), sd((size_t)ni), elbo((size_t)nl);
   std::vector<int32_t> status((size_t)nl), iters((size_t)nl), nact((size_t)nl);
   std::vector<int64_t> nfrag((size_t)nl);
   const sbgpu_batch_t v = b.view();
   for (int pass = 0; pass < 3; ++pass) {
      sbgpu_em_vb_t out = {};
      out.count = count.data(), out.share = share.data(), out.share_sd = sd.data(), out.status = status.data(), out.iters = iters.data();
      out.elbo = elbo.data(), out.n_active = nact.data(), out.n_frag = nfrag.data();
      if (pass == 2) out.share = nullptr, out.elbo = nullptr, out.iters = nullptr; // any may be NULL
      const sbgpu_vb_params_t p = {pass == 1 ? 1.0 : 1e-6, 1e-2, pass == 1 ? 5 : 1000, 0};
      CHECK(sbgpu_em_vb_host(&v, pass == 0 ? nullptr : &p, &out) == SBGPU_OK);
      CHECK(out.d_count == nullptr && out.d_n_frag == nullptr);
      for (int64_t l = 0; l < nl; ++l) {
         double total = 0.0;
         for (int64_t i = b.iso_off[l]; i < b.iso_off[l + 1]; ++i) {
            CHECK(count[i] >= 0.0 && !std::isnan(count[i]) && !std::isnan(sd[i]));
            total += count[i];
         }
         CHECK(status[l] >= 0 && status[l] <= 3);
         if (status[l] == SBGPU_EM_INIT_EMPTY) CHECK(total == 0.0 && nact[l] == 0 && nfrag[l] == 0);
         else CHECK(std::fabs(total - (double)nfrag[l]) <= 1e-9 * (1.0 + (double)nfrag[l]));
      }
      CHECK(status[1] == SBGPU_EM_INIT_EMPTY && status[2] == SBGPU_EM_INIT_EMPTY && status[3] == SBGPU_EM_INIT_EMPTY && status[9] == SBGPU_EM_INIT_EMPTY);
   }
   sbgpu_em_vb_t out = {};
   const sbgpu_vb_params_t bad = {0.0, 1e-2, 10, 0};
   CHECK(sbgpu_em_vb_host(&v, &bad, &out) == SBGPU_EINVAL && sb::last.find("alpha outside") != std::string::npos);
   CHECK(sbgpu_em_vb_host(nullptr, nullptr, &out) == SBGPU_EINVAL);
   Batch wide;
   wide.add(1, 513, 7, 0.0);
   const sbgpu_batch_t w = wide.view();
   CHECK(sbgpu_em_vb_host(&w, nullptr, &out) == SBGPU_ESHAPE);
   std::printf("ok\n");
   return 0;
}
"""


def test_the_host_form_under_the_sanitizers(tmp_path):
    """vb_host.cpp and the rule's headers with a main of their own: shapes at the limits, empty loci, NULL outputs, the refusals"""
    src, exe = tmp_path / "vb_main.cpp", tmp_path / "vb_main"
    src.write_text(SANITIZED)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *INC, str(src), os.path.join(CSRC, "vb_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
