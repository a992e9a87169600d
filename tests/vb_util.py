"""The variational Bayes solve restated (include/sbgpu.h: sbgpu_em_vb_*, rules 1-7) in numpy, for
tests/test_vb*.py: no code shared with the library, and nothing transliterated from csrc/vb_rules.h.  What differs on purpose:
digamma shifts its argument to x >= 20 and stops the series at y^5; a bin's mass is a matrix product (numpy's own summation
order, no fma); the step norm is numpy's pairwise sum; lgamma is math.lgamma.  Neither scipy nor mpmath is needed.

THE BOUNDS.  Exact in every comparison: status, n_active, n_frag, which outputs are zero, and iters under
max_iter <= 3.  Where two forms stop at the same iteration the yardstick is the host form against this restatement on the five EM
goldens: the largest |delta count| / max(1, N) and |delta elbo| / max(1, |elbo|) measured there (HOST_COUNT_GAP, HOST_ELBO_GAP --
measured on the CPU and rounded up to two digits; tests/test_vb_cpp.py asserts them).  The device gets 100 x that
against the host form, which leaves room for a device library whose log / exp / lgamma stand a few ulp from glibc's.  Where the
iteration counts differ by one the two forms stopped on either side of a step of about change_limit: || delta count ||_2 <=
2 change_limit; more than one iteration apart is a failure, and at most 1 % of a sample's loci may differ at all.
"""
import math

import numpy as np

ROW_EPS = 1e-5            # SBGPU_EM_ROW_EPS
CHANGE_LIMIT = 1e-2       # SBGPU_EM_THETA_CHANGE_LIMIT
MAX_ITER = 1000           # SBGPU_EM_MAX_ITER
OK, INIT_EMPTY, DENOM_ZERO, MAXITER = 0, 1, 2, 3
MAX_BINS, MAX_ISO = 5632, 512
GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
ALPHAS = (0.01, 1.0)
# the host form against this restatement over the goldens at both alphas (every locus stops at the same iteration in both):
# measured 1.13e-14 (em_c3_400, alpha 0.01) and 9.93e-15 (em_random_256, alpha 1); tests/test_vb_cpp.py prints and asserts them
HOST_COUNT_GAP = 1.2e-14
HOST_ELBO_GAP = 1.0e-14
DEVICE_FACTOR = 100.0
ITERS_MAY_DIFFER = 0.01


def digamma(x):
    """psi of a positive array: the recurrence up to x >= 20, then log x - 1/(2x) - sum B_2k / (2k x^2k), k = 1..5"""
    x = np.array(x, np.float64, ndmin=1)
    s = np.zeros_like(x)
    for _ in range(20):
        low = x < 20.0
        if not low.any():
            break
        s[low] -= 1.0 / x[low]
        x[low] += 1.0
    y = 1.0 / (x * x)
    series = y * (1.0 / 12.0 - y * (1.0 / 120.0 - y * (1.0 / 252.0 - y * (1.0 / 240.0 - y / 132.0))))
    return np.log(x) - 0.5 / x - series + s


def lgamma(x):
    return np.array([math.lgamma(float(v)) for v in np.atleast_1d(x)])


def elbo_of(A, n, c, active, alpha, N):
    """rule 6 at c (A: the live bins' normalised rows, n: their counts)"""
    ka = int(active.sum())
    a0 = ka * alpha + float(N)
    lw = digamma(alpha + c[active]) - digamma(a0)[0]
    with np.errstate(divide="ignore"):
        mass = A[:, active] @ np.exp(lw)
        counted = n > 0
        bins = float((n[counted] * np.log(mass[counted])).sum()) if counted.any() else 0.0
    prior = math.lgamma(a0) - lgamma(alpha + c[active]).sum() - math.lgamma(ka * alpha) + ka * math.lgamma(alpha) + float((c[active] * lw).sum())
    return bins - prior


def solve_locus(n, F, alpha=0.01, change_limit=CHANGE_LIMIT, max_iter=MAX_ITER, trace=False):
    """One locus -> dict(count, share, share_sd [K]; status, iters, elbo, n_active, n_frag); trace: also `steps`, the norm of
    every iteration's step"""
    n, F = np.asarray(n, np.int64), np.asarray(F, np.float64)
    F = F if F.ndim == 2 else F.reshape(len(n), -1)       # (a locus without bins keeps its isoforms: shape (0, K))
    K = F.shape[1]
    zero = dict(count=np.zeros(K), share=np.zeros(K), share_sd=np.zeros(K), status=INIT_EMPTY, iters=0, elbo=0.0, n_active=0, n_frag=0, steps=[])
    live = (F > ROW_EPS).any(axis=1) if K else np.zeros(len(n), bool)
    if not live.any():
        return zero
    F, n = F[live], n[live]
    s = np.zeros(K)
    for row in F:                      # (ascending, as the rule says: a column's sum decides who is active)
        s = s + row
    active = s > 0.0
    ka, N = int(active.sum()), int(n.sum())
    if N == 0:
        return dict(zero, status=OK, iters=1, n_active=ka)
    A = np.zeros_like(F)
    A[:, active] = F[:, active] / s[active]
    c = np.where(active, float(N) / ka, 0.0)
    status, iters, steps = MAXITER, 0, []
    for it in range(max_iter):
        iters = it + 1
        p = digamma(alpha + c[active])
        w = np.zeros(K)
        w[active] = np.exp(p - p.max())
        d = A @ w
        if ((n > 0) & (d == 0.0)).any():
            status = DENOM_ZERO
            break
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(n > 0, n / d, 0.0)
        c_next = w * (A.T @ r)
        step = float(np.sqrt(((c_next - c)[active] ** 2).sum()))
        steps.append(step)
        if step < change_limit:
            status = OK
            break
        c = c_next
    a0 = ka * alpha + float(N)
    a = alpha + c
    out = dict(count=np.where(active, c, 0.0), share=np.where(active, a / a0, 0.0),
               share_sd=np.where(active, np.sqrt(a * (a0 - a) / (a0 * a0 * (a0 + 1.0))), 0.0), status=status, iters=iters,
               elbo=elbo_of(A, n, c, active, alpha, N), n_active=ka, n_frag=N)
    if trace:
        out["steps"] = steps
    return out


def solve(batch, alpha=0.01, change_limit=CHANGE_LIMIT, max_iter=MAX_ITER):
    """Every locus of a batch -> dict of arrays laid out as a vb.VariationalFit's"""
    row_off, iso_off, f_off = (np.asarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    nl = len(row_off) - 1
    out = {k: np.zeros(int(iso_off[-1])) for k in ("count", "share", "share_sd")}
    out.update(status=np.zeros(nl, np.int32), iters=np.zeros(nl, np.int32), elbo=np.zeros(nl), n_active=np.zeros(nl, np.int32), n_frag=np.zeros(nl, np.int64))
    for l in range(nl):
        nb, K = int(row_off[l + 1] - row_off[l]), int(iso_off[l + 1] - iso_off[l])
        r = solve_locus(np.asarray(batch.count)[int(row_off[l]):int(row_off[l + 1])], np.asarray(batch.F)[int(f_off[l]):int(f_off[l]) + nb * K].reshape(nb, K),
                        alpha, change_limit, max_iter)
        for k in ("count", "share", "share_sd"):
            out[k][int(iso_off[l]):int(iso_off[l + 1])] = r[k]
        for k in ("status", "iters", "elbo", "n_active", "n_frag"):
            out[k][l] = r[k]
    return out


def get(x, k):
    return np.asarray(x[k] if isinstance(x, dict) else getattr(x, k))


def compare(got, want, iso_off, count_gap, elbo_gap, change_limit=CHANGE_LIMIT, label="", exact_iters=False):
    """got, want: two solves of one batch (a vb.VariationalFit or solve()'s dict) under the bounds at the head of this file ->
    dict(count, elbo: the largest gaps over the loci of equal iteration counts; differ: the share of loci whose counts differ)"""
    iso_off = np.asarray(iso_off, np.int64)
    nl = len(iso_off) - 1
    for k in ("status", "n_active", "n_frag"):
        np.testing.assert_array_equal(get(got, k), get(want, k), err_msg="%s %s" % (label, k))
    for k in ("count", "share", "share_sd"):
        np.testing.assert_array_equal(get(got, k) == 0.0, get(want, k) == 0.0, err_msg="%s %s's zeros" % (label, k))
        assert not np.isnan(get(got, k)).any(), (label, k)
    di = get(got, "iters").astype(np.int64) - get(want, "iters")
    assert np.abs(di).max(initial=0) <= 1, (label, "iteration counts more than one apart", np.nonzero(np.abs(di) > 1)[0][:8])
    if exact_iters:
        np.testing.assert_array_equal(get(got, "iters"), get(want, "iters"), err_msg=label + " iters")
    differ = float((di != 0).mean()) if nl else 0.0
    assert differ <= ITERS_MAY_DIFFER, (label, "loci whose iteration counts differ", differ)
    worst = dict(count=0.0, elbo=0.0, differ=differ)
    N = np.maximum(1.0, get(want, "n_frag").astype(np.float64))
    for l in range(nl):
        i0, i1 = int(iso_off[l]), int(iso_off[l + 1])
        dc = get(got, "count")[i0:i1] - get(want, "count")[i0:i1]
        if di[l] != 0:
            assert float(np.sqrt((dc ** 2).sum())) <= 2.0 * change_limit, (label, l, "a locus that stopped one iteration apart")
            continue
        gap = float(np.abs(dc).max(initial=0.0)) / N[l]
        assert gap <= count_gap, (label, l, "count", gap, count_gap)
        for k in ("share", "share_sd"):
            g = float(np.abs(get(got, k)[i0:i1] - get(want, k)[i0:i1]).max(initial=0.0))
            assert g <= count_gap, (label, l, k, g, count_gap)     # (shares are counts over a0 >= N)
        e0, e1 = float(get(got, "elbo")[l]), float(get(want, "elbo")[l])
        if np.isinf(e0) or np.isinf(e1):
            assert e0 == e1, (label, l, "elbo", e0, e1)
            continue
        eg = abs(e0 - e1) / max(1.0, abs(e1))
        assert eg <= elbo_gap, (label, l, "elbo", eg, elbo_gap)
        worst["count"], worst["elbo"] = max(worst["count"], gap), max(worst["elbo"], eg)
    return worst


def bitwise(a, b, label="", names=("count", "share", "share_sd", "status", "iters", "elbo", "n_active", "n_frag")):
    """every array of two VariationalFits, bit for bit"""
    for k in names:
        x, y = get(a, k), get(b, k)
        np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y,
                                      err_msg="%s %s" % (label, k))


# ---- the samples


def from_loci(loci):
    """[(count, F rows x niso), ...] -> LocusBatch"""
    from strawberry_amd.synth import from_loci as f
    return f([(np.asarray(n, np.int32), np.asarray(F, np.float64).reshape(len(n), -1)) for n, F in loci])


def select_loci(batch, idx):
    from fit_util import select_loci as f
    return f(batch, idx)


def within_limits(batch):
    """the loci the solve takes (the others are refused with SBGPU_ESHAPE)"""
    return np.nonzero((np.diff(batch.row_off) <= MAX_BINS) & (np.diff(batch.iso_off) <= MAX_ISO))[0]


def golden_within_limits(golden, name):
    full, _, _ = golden(name)
    idx = within_limits(full)
    return full if len(idx) == full.n_loci else select_loci(full, idx)


def shaped(rng, rows, niso, density=0.5, depth=60):
    """A random locus of a given shape: one row that carries every isoform, a dropped row where there are three or more"""
    F = rng.uniform(1e-3, 0.3, (rows, niso)) * (rng.random((rows, niso)) < density)
    F[rng.integers(0, rows), :] = rng.uniform(1e-3, 0.3, niso)
    if rows > 2:
        F[1, :] = 1e-6
    return rng.integers(0, depth, rows).astype(np.int32), F


def no_fragments():
    """live bins, no fragment in them (the dead bin's do not count): OK, one iteration, zeros"""
    return [0, 0, 7], [[0.2, 0.1], [0.0, 0.3], [1e-6, 1e-7]]


def init_empty():
    return [5, 3], [[1e-6, 1e-5], [0.0, 1e-7]]


def inactive_columns():
    """column 1 has no weight at all, column 3 only in a dead bin: K_a = 2"""
    return [30, 12, 9, 4], [[0.2, 0.0, 0.1, 0.0], [0.3, 0.0, 0.0, 0.0], [0.0, 0.0, 0.25, 0.0], [0.0, 0.0, 0.0, 9e-6]]


def dying_private_bin():
    """Isoform 1 shares a counted bin with isoform 0 and owns a bin WITHOUT fragments; isoform 0 owns a deep bin.  At alpha = 1e-6
    and a tight change limit isoform 1 dies (its weight underflows to 0) and its private bin's mass with it: 0 / 0 must not
    appear."""
    return [100000, 3, 0], [[0.5, 0.0], [0.2, 0.2], [0.0, 0.4]]


DYING_PARAMS = dict(alpha=1e-6, change_limit=1e-12, max_iter=400)


def underflowing_bin(k=400):
    """Bin 1 holds one fragment shared by k isoforms whose columns a fragment-less bin 0 scales down by 1e300, bin 2 a million
    fragments of isoform k's.  The first iteration leaves each of the k at 1/k of a fragment; in the second their weights are
    about exp(-k - 14) and every product with 1e-300 is 0 (k >= 100): a counted bin without mass."""
    F = np.zeros((3, k + 1))
    F[0, :k], F[1, :k], F[2, k] = 1e300, 1.0, 1.0
    return [0, 1, 1000000], F


UNDERFLOW_PARAMS = dict(alpha=1e-6)


def slow_locus(rng, rows=12, niso=4, depth=1000):
    """Isoforms whose columns are one profile times factors of 0.3 .. 1.7: hundreds of iterations at the default change limit
    (525 at alpha = 0.01, 345 at alpha = 1 under seed 31)"""
    F = rng.uniform(0.05, 0.3, rows)[:, None] * rng.uniform(0.3, 1.7, (rows, niso))
    lam = (F / F.sum(axis=0)) @ rng.dirichlet(np.ones(niso))
    return rng.multinomial(depth, lam / lam.sum()).astype(np.int32), F


def fast_locus():
    """Two isoforms with a bin each: the second iteration does not move"""
    return [40, 60], [[0.3, 0.0], [0.0, 0.2]]


# One locus on either side of every threshold of sbgpu_em_vb_limits (wave_vals = 512 weights; stage_doubles = 8064 doubles for
# bins x isoforms + bins + 2 isoforms), the extreme shapes, and the edge cases between ordinary loci
THRESHOLD_SHAPES = {"1x1": (1, 1), "wave, one row": (1, 512), "block, two rows": (2, 512), "wave, one isoform": (512, 1),
                    "block, one isoform": (513, 1), "wave, full": (16, 32), "block, just": (16, 33), "staged, full": (216, 36),
                    "global, just": (217, 36), "staged, one isoform": (4031, 1), "global, one isoform": (4032, 1), "tall": (5632, 2),
                    "wide": (40, 512), "before": (7, 3), "after": (9, 4)}
EDGE_LOCI = {"init empty": init_empty, "no fragments": no_fragments, "inactive columns": inactive_columns}


def threshold_sample():
    """-> (LocusBatch, names): THRESHOLD_SHAPES' loci with EDGE_LOCI's between "before" and "after" """
    rng = np.random.default_rng(22)
    names, loci = [], []
    for name, shape in THRESHOLD_SHAPES.items():
        if name == "after":
            for k, f in EDGE_LOCI.items():
                names.append(k), loci.append(f())
        names.append(name), loci.append(shaped(rng, *shape))
    return from_loci(loci), names


def form_of(batch, lim):
    """0: a wave serves the locus, 1: a workgroup with A in LDS, 2: a workgroup with A in the call's scratch"""
    rows, niso = np.diff(batch.row_off), np.diff(batch.iso_off)
    return np.where(rows * niso <= lim["wave_vals"], 0, np.where(rows * niso + rows + 2 * niso <= lim["stage_doubles"], 1, 2))


def tile_batch(batch, reps):
    from fit_util import tile_batch as f
    return f(batch, reps)


def many_tiny(n_wave=20, n_block=4):
    """A base of tiny loci of both forms, to be tiled past two passes of either grid"""
    rng = np.random.default_rng(41)
    loci = [shaped(rng, int(rng.integers(1, 10)), int(rng.integers(1, 5)), depth=200) for _ in range(n_wave)]
    loci += [shaped(rng, 16, 33, depth=200) for _ in range(n_block)]
    return from_loci(loci)
