"""The differential isoform usage restated (include/sbgpu.h: sbgpu_em_diff_*) in Python floats and plain loops, for
tests/test_differential_usage*.py: no code shared with the library.  The sub-matrices are made by deleting columns, alpha in
Python floats in the rule's order (sum, quotient, product), every fit -- own and cross -- by fit_util.by_hand, rules 5-9 in
Python floats.  The caller passes the theta, status and iterations of every sub-problem (the library has no CPU EM, and the
restatement has none either).

THE BOUND of a finite lr_stat = 2 ((ll_A - llx_A) + (ll_B - llx_B)): 2 x the sum of the four fits' "either form against by_hand"
loglik bounds at the head of tests/fit_util.py, each for its sub-problem's shape (the project's own bound, as support_util.py
uses it); the two subtractions, the sum and the product add roundings far below it."""
import math

import numpy as np

import fit_util as FU

MAX_KEPT, MAX_POOLED_BINS = 512, 5632
OK, EMPTY, SOLE, TOO_WIDE, TOO_DEEP, ONE_SAMPLE, UNSOLVED = range(7)
DENOM_ZERO = 2
PER_ISO = ("theta_a", "theta_b", "theta_pooled", "usage_a", "usage_b", "usage_pooled", "delta_usage")
INTS = ("n_a", "n_b", "lost_shift", "dof", "diff_status", "top_iso", "status_a", "status_b", "status_pooled", "iters_a", "iters_b", "iters_pooled")
MODES = ("same", "null", "subset", "shift")


def _locus(batch, l):
    row_off, iso_off, f_off = (np.asarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    nb, niso = int(row_off[l + 1] - row_off[l]), int(iso_off[l + 1] - iso_off[l])
    F = np.asarray(batch.F[int(f_off[l]):int(f_off[l + 1])], np.float64).reshape(nb, niso)
    return np.asarray(batch.count[int(row_off[l]):int(row_off[l + 1])], np.int32), F


def kept_columns(batch, keep_a, keep_b, l):
    i0, i1 = int(batch.iso_off[l]), int(batch.iso_off[l + 1])
    on = lambda keep, i: keep is None or int(keep[i]) != 0  # noqa: E731
    return [i - i0 for i in range(i0, i1) if on(keep_a, i) or on(keep_b, i)]


def sub_problems(batch_a, batch_b, keep_a=None, keep_b=None):
    """-> (diff_status [n_loci] before the solves, [(locus, kind, kept columns, count, F rows x K)]), alpha in Python floats"""
    status, subs = [], []
    for l in range(len(batch_a.iso_off) - 1):
        kept = kept_columns(batch_a, keep_a, keep_b, l)
        (na, Fa), (nb, Fb) = _locus(batch_a, l), _locus(batch_b, l)
        K = len(kept)
        st = EMPTY if K == 0 else SOLE if K == 1 else TOO_WIDE if K > MAX_KEPT else TOO_DEEP if len(na) + len(nb) > MAX_POOLED_BINS else OK
        status.append(st)
        if st != OK:
            continue
        niso = Fa.shape[1]
        gone = [j for j in range(niso) if j not in kept]
        own = [np.delete(Fa, gone, axis=1), np.delete(Fb, gone, axis=1)]
        c = []
        for M in own:
            cs = [0.0] * K
            for row in M:
                if any(float(w) > FU.ROW_EPS for w in row):
                    for k in range(K):
                        cs[k] += float(row[k])
            c.append(cs)
        pooled = []
        for s, M in enumerate(own):
            alpha = [0.5 * ((c[0][k] + c[1][k]) / c[s][k]) if c[s][k] != 0.0 else 1.0 for k in range(K)]
            pooled.append(np.array([[float(row[k]) * alpha[k] for k in range(K)] for row in M], np.float64).reshape(len(M), K))
        subs.append((l, 0, kept, na.copy(), own[0]))
        subs.append((l, 1, kept, nb.copy(), own[1]))
        subs.append((l, 2, kept, np.concatenate([na, nb]), np.concatenate(pooled, axis=0)))
    return np.array(status, np.int32), subs


def batch_of(loci):
    """[(count, F rows x niso), ...] -> LocusBatch; F is two-dimensional, so a locus may have no rows"""
    from strawberry_amd.synth import LocusBatch
    loci = [(np.asarray(n, np.int32).reshape(-1), np.asarray(F, np.float64)) for n, F in loci]
    assert all(F.ndim == 2 and F.shape[0] == len(n) for n, F in loci)
    cat = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)  # noqa: E731
    rows, niso = [len(n) for n, _ in loci], [F.shape[1] for _, F in loci]
    return LocusBatch(cat(rows), cat(niso), cat([r * k for r, k in zip(rows, niso)]), np.concatenate([n for n, _ in loci] + [np.zeros(0, np.int32)]),
                      np.concatenate([F.reshape(-1) for _, F in loci] + [np.zeros(0)]), np.full(int(sum(niso)), 1000, np.int32), "custom")


def sub_batch(subs):
    return batch_of([(n, F) for _, _, _, n, F in subs])


def _ll_bound(fit, q, shape):
    rows, cols = shape
    r_e = 2.0 * (rows + 8) * FU.U + 2.0 * (2.0 * (cols + 4) * FU.U) + 4.0 * FU.U
    return 2.0 * (rows + FU.K) * FU.U * float(fit["abs_loglik"][q]) + float(fit["n_live"][q]) * r_e


def by_hand(batch_a, batch_b, keep_a, keep_b, thetas, statuses, iters):
    """thetas: one array per sub-problem, in sub_problems' order; statuses, iters: the solves' -> dict of the 24 results, `bound`
    [n_loci]: the bound of lr_stat, `gap` [n_loci]: the top |delta_usage| minus the runner-up's (top_iso is compared where it
    clears a margin), `top_abs` [n_loci]: that top |delta_usage|, `subs`, `fit`, `cross`."""
    iso_off = np.asarray(batch_a.iso_off, np.int64)
    assert (iso_off == np.asarray(batch_b.iso_off, np.int64)).all()
    nl, n_iso = len(iso_off) - 1, int(iso_off[-1])
    pre, subs = sub_problems(batch_a, batch_b, keep_a, keep_b)
    assert len(thetas) == len(subs) == len(statuses) == len(iters)
    out = {k: np.zeros(n_iso) for k in PER_ISO}
    for k in ("lr_stat", "loglik_a", "loglik_b", "loglik_a_pooled", "loglik_b_pooled", "bound", "gap", "top_abs"):
        out[k] = np.zeros(nl)
    for k in ("n_a", "n_b", "lost_shift"):
        out[k] = np.zeros(nl, np.int64)
    out["dof"], out["diff_status"], out["top_iso"] = np.zeros(nl, np.int32), pre.copy(), np.full(nl, -1, np.int32)
    for k in ("status_a", "status_b", "status_pooled", "iters_a", "iters_b", "iters_pooled"):
        out[k] = np.full(nl, -1, np.int32)
    fit = cross = None
    if subs:
        sb = sub_batch(subs)
        own_theta = np.concatenate([np.asarray(t, np.float64) for t in thetas])
        x_thetas = [thetas[q - q % 3 + 2] for q in range(len(subs))]
        x_status = np.array([statuses[q - q % 3 + 2] for q in range(len(subs))], np.int32)
        fit = FU.by_hand(sb, own_theta, None, np.asarray(statuses, np.int32))
        cross = FU.by_hand(sb, np.concatenate([np.asarray(t, np.float64) for t in x_thetas]), None, x_status)
    lost = lambda f, q: int(f["n_dropped"][q]) + int(f["n_impossible"][q])  # noqa: E731

    def top_of(l, i0, kept):
        best, second, top = -1.0, -1.0, -1
        for j in kept:
            d = abs(float(out["delta_usage"][i0 + j]))
            if d > best:
                best, second, top = d, best, j
            elif d > second:
                second = d
        out["top_iso"][l], out["gap"][l], out["top_abs"][l] = top, best - max(second, 0.0), max(best, 0.0)

    for l in range(nl):
        if pre[l] != SOLE:
            continue
        i0 = int(iso_off[l])
        j = kept_columns(batch_a, keep_a, keep_b, l)[0]
        pa, pb = (float((_locus(b, l)[0] > 0).any()) for b in (batch_a, batch_b))
        out["usage_a"][i0 + j], out["usage_b"][i0 + j], out["usage_pooled"][i0 + j] = pa, pb, max(pa, pb)
        out["delta_usage"][i0 + j] = pb - pa
        top_of(l, i0, [j])
    for q in range(0, len(subs), 3):
        l, _, kept, _, _ = subs[q]
        i0, K = int(iso_off[l]), len(kept)
        A, B, P = q, q + 1, q + 2
        for x, name in ((A, "a"), (B, "b"), (P, "pooled")):
            out["status_" + name][l], out["iters_" + name][l] = statuses[x], iters[x]
        n_a = int(fit["n_live"][A]) - int(fit["n_impossible"][A])
        n_b = int(fit["n_live"][B]) - int(fit["n_impossible"][B])
        if n_a == 0 or n_b == 0 or statuses[A] == FU.INIT_EMPTY or statuses[B] == FU.INIT_EMPTY:
            out["diff_status"][l] = ONE_SAMPLE
            continue
        if DENOM_ZERO in (statuses[A], statuses[B], statuses[P]):
            out["diff_status"][l] = UNSOLVED
            continue
        ll_a, ll_b, llx_a, llx_b = float(fit["loglik"][A]), float(fit["loglik"][B]), float(cross["loglik"][A]), float(cross["loglik"][B])
        out["loglik_a"][l], out["loglik_b"][l], out["loglik_a_pooled"][l], out["loglik_b_pooled"][l] = ll_a, ll_b, llx_a, llx_b
        out["lr_stat"][l] = 2.0 * ((ll_a - llx_a) + (ll_b - llx_b))
        out["bound"][l] = 2.0 * (_ll_bound(fit, A, subs[A][4].shape) + _ll_bound(fit, B, subs[B][4].shape) +
                                 _ll_bound(cross, A, subs[A][4].shape) + _ll_bound(cross, B, subs[B][4].shape))
        out["n_a"][l], out["n_b"][l], out["dof"][l] = n_a, n_b, K - 1
        out["lost_shift"][l] = lost(fit, P) - lost(fit, A) - lost(fit, B) + (lost(cross, A) - lost(fit, A)) + (lost(cross, B) - lost(fit, B))
        for x, name in ((A, "a"), (B, "b"), (P, "pooled")):
            t = [float(v) for v in thetas[x]]
            total = 0.0
            for v in t:
                total += v
            for r, j in enumerate(kept):
                out["theta_" + name][i0 + j] = t[r]
                out["usage_" + name][i0 + j] = t[r] / total if total != 0.0 else 0.0
        for j in kept:
            out["delta_usage"][i0 + j] = float(out["usage_b"][i0 + j]) - float(out["usage_a"][i0 + j])
        top_of(l, i0, kept)
    out["subs"], out["fit"], out["cross"] = subs, fit, cross
    return out


def solve_each(oracle, subs):
    """the oracle's EM on every sub-problem by itself -> thetas, status, iters"""
    res = [oracle.em_locus(n, F) for _, _, _, n, F in subs]
    return [r[0] for r in res], np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32)


def compare(t, want, label="", exact_doubles=True, top_margin=None, restrict=()):
    """t: a diff.DifferentialUsage; want: by_hand()'s dict.  Every integer and status exact; theta / usage / delta bit for bit
    (exact_doubles); the log-likelihoods and lr_stat under the bound; top_iso where the top |delta| clears the runner-up by
    top_margin (None: everywhere, the same theta bits decide the same way) -> (the worst share of the bound, the loci of
    top_set whose top_iso was left out, the size of top_set, the two-isoform loci).
    THE SET top_iso's margin is held on (top_set): the OK loci of THREE OR MORE kept isoforms, without the loci `restrict` names.
    A locus of two kept isoforms has usages that sum to 1 in each sample, so its two |delta_usage| are equal up to a rounding by
    construction (include/sbgpu.h, rule 9) and NONE of them clears any margin, for any solver: they are counted, reported and kept
    out of the set, not out of the count of a set they cannot belong to; each is still compared where a call feeds by_hand the
    same theta bits (top_margin None)."""
    for k in INTS:
        if k != "top_iso":
            np.testing.assert_array_equal(getattr(t, k), want[k], err_msg="%s %s" % (label, k))
    if exact_doubles:
        for k in PER_ISO:
            np.testing.assert_array_equal(getattr(t, k).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (label, k))
    # (a locus whose usages do not differ at all -- identical samples -- is decided by the order, not by a rounding: the first
    # kept isoform, where the other side's differences are exact zeros too)
    tie_of_zeros = (want["top_abs"] == 0.0) & (np.add.reduceat(np.concatenate([np.abs(t.delta_usage), [0.0]]), t.iso_off[:-1]) * (np.diff(t.iso_off) > 0) == 0.0)
    clear = np.ones(len(want["gap"]), bool) if top_margin is None else (want["gap"] > top_margin) | (want["top_iso"] < 0) | tie_of_zeros
    np.testing.assert_array_equal(t.top_iso[clear], want["top_iso"][clear], err_msg=label + " top_iso")
    assert np.isfinite(t.lr_stat).all(), label
    err = np.abs(t.lr_stat - want["lr_stat"])
    assert (err[want["bound"] == 0.0] == 0.0).all(), label
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(err == 0.0, 0.0, err / want["bound"])
    assert not (err > want["bound"]).any(), (label, float(share.max()), int(np.argmax(share)))
    for k in ("loglik_a", "loglik_b", "loglik_a_pooled", "loglik_b_pooled"):
        assert (np.abs(getattr(t, k) - want[k]) <= want["bound"]).all(), (label, k)
    pair = (want["diff_status"] == OK) & (want["dof"] == 1)
    top_set = (want["diff_status"] == OK) & (want["dof"] > 1)
    top_set[list(restrict)] = False
    return (float(share.max()) if share.size else 0.0), int((~clear & top_set).sum()), int(top_set.sum()), int(pair.sum())


def second_sample(batch, mode, seed, theta=None):
    """A second sample B over batch A's annotation.  same: identical counts and weights.  null: F * 1.3, the counts multinomial
    (each locus' total as A's) from theta -- A's oracle theta -- under B's OWN column scales: p_b proportional to
    sum_j theta_j F_bj / c_j over B's live rows, the model's `expected` (fit_util.by_hand's, computed here with numpy), the null
    hypothesis in this model.  subset: a sorted random two-thirds of each locus' rows (at least one), then as null.  shift: as
    null, from A's theta reversed within the locus."""
    from strawberry_amd.synth import LocusBatch
    assert mode in MODES
    if mode == "same":
        return LocusBatch(batch.row_off.copy(), batch.iso_off.copy(), batch.f_off.copy(), batch.count.copy(), batch.F.copy(), batch.length.copy(), "same")
    rng = np.random.default_rng(seed)
    loci = []
    for l in range(batch.n_loci):
        n, F = _locus(batch, l)
        i0, i1 = int(batch.iso_off[l]), int(batch.iso_off[l + 1])
        th = np.asarray(theta[i0:i1], np.float64)
        if mode == "shift":
            th = th[::-1]
        if mode == "subset" and len(n):
            rows = np.sort(rng.choice(len(n), max(1, (2 * len(n)) // 3), replace=False))
            F = F[rows]
        F = F * 1.3
        live = (F > FU.ROW_EPS).any(axis=1) if F.size else np.zeros(len(F), bool)
        c = F[live].sum(axis=0) if F.size else np.zeros(F.shape[1])
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.where(c != 0.0, th / c, 0.0)
        d = np.where(live, F @ g, 0.0) if F.size else np.zeros(len(F))
        total = int(n.sum())
        cnt = rng.multinomial(total, d / d.sum()) if d.sum() > 0 and total else np.zeros(len(F), np.int64)
        loci.append((cnt.astype(np.int32), F))
    b = batch_of(loci)
    assert (np.asarray(b.iso_off) == np.asarray(batch.iso_off)).all()
    return b


def census(t, alpha_stat=None):
    """loci compared (OK, lost_shift 0), rejected at 0.05, negative statistics, the extremes"""
    ok = (t.diff_status == OK) & (t.lost_shift == 0)
    p = t.p_value()
    with np.errstate(invalid="ignore"):
        rej = int((p[ok] < 0.05).sum())
    return dict(loci=int(len(ok)), compared=int(ok.sum()), shifted=int(((t.diff_status == OK) & (t.lost_shift != 0)).sum()), rejected=rej,
                negative=int((t.lr_stat[ok] < 0).sum()), smallest=float(t.lr_stat[ok].min()) if ok.any() else 0.0,
                largest=float(t.lr_stat[ok].max()) if ok.any() else 0.0)
