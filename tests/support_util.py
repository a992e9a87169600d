"""The drop-one isoform support restated (include/sbgpu.h: sbgpu_em_loo_*) in Python floats and plain loops, for
tests/test_isoform_support*.py: no code shared with the library.  The sub-matrices are made by deleting columns, the statuses by
counting, the fit's three arrays by fit_util.by_hand, rules 4-9 in Python floats.  The caller passes the theta of every
sub-problem (the library has no CPU EM, and the restatement has none either).

THE BOUND of a finite lr_stat = 2 (loglik_base - loglik_sub): 2 x (bound_base + bound_sub), each the "either form against
by_hand" loglik bound at the head of tests/fit_util.py for that sub-problem's shape."""
import math

import numpy as np

import fit_util as FU

MAX_KEPT = 64
OK, EMPTY, TOO_WIDE = 0, 1, 2
NOT_KEPT, TESTED, SOLE, LOCUS_SKIPPED = 0, 1, 2, 3


def sub_problems(batch, keep=None):
    """-> (loo_status [n_loci], [(locus, dropped locus-local isoform or -1, kept columns used, count, F rows x cols)])"""
    row_off, iso_off, f_off = (np.asarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    status, subs = [], []
    for l in range(len(row_off) - 1):
        nb, niso = int(row_off[l + 1] - row_off[l]), int(iso_off[l + 1] - iso_off[l])
        kept = [j for j in range(niso) if keep is None or int(keep[int(iso_off[l]) + j]) != 0]
        status.append(EMPTY if not kept else TOO_WIDE if len(kept) > MAX_KEPT else OK)
        if status[-1] != OK:
            continue
        F = np.asarray(batch.F[int(f_off[l]):int(f_off[l + 1])], np.float64).reshape(nb, niso)
        n = np.asarray(batch.count[int(row_off[l]):int(row_off[l + 1])], np.int32)
        for drop in [-1] + (kept if len(kept) >= 2 else []):
            cols = [j for j in kept if j != drop]
            subs.append((l, drop, cols, n.copy(), np.delete(F, [j for j in range(niso) if j not in cols], axis=1)))
    return np.array(status, np.int32), subs


def sub_batch(subs):
    return FU.from_loci([(n, F) for _, _, _, n, F in subs])


def by_hand(batch, keep, thetas, sub_status=None, sub_iters=None):
    """thetas: one array per sub-problem, in sub_problems' order; sub_status / sub_iters: the solves' (for status_without,
    iters_without and the base's) -> dict of the thirteen results, `without` {global isoform: theta_without}, `bound` [n_iso]:
    the bound of a finite lr_stat, `gap` [n_iso]: top gain minus the runner-up's (heir is compared where it clears a margin),
    `theta_max` [n_iso]: max |theta| over the locus' sub-problems."""
    iso_off = np.asarray(batch.iso_off, np.int64)
    nl, n_iso = len(iso_off) - 1, int(iso_off[-1])
    loo_status, subs = sub_problems(batch, keep)
    assert len(thetas) == len(subs)
    sb = sub_batch(subs) if subs else None
    theta_cat = np.concatenate([np.asarray(t, np.float64) for t in thetas] + [np.zeros(0)])
    # the fit's status: a solve never started where no row has a weight above the row threshold
    fit_status = np.array([FU.INIT_EMPTY if not (F > FU.ROW_EPS).any() else 0 for _, _, _, _, F in subs], np.int32)
    fit = FU.by_hand(sb, theta_cat, None, fit_status) if subs else None
    out = dict(loo_status=loo_status, lr_stat=np.zeros(n_iso), heir_gain=np.zeros(n_iso), theta_refit=np.zeros(n_iso),
               n_unique=np.zeros(n_iso, np.int64), heir=np.full(n_iso, -1, np.int32), status_without=np.full(n_iso, -1, np.int32),
               iters_without=np.full(n_iso, -1, np.int32), support=np.zeros(n_iso, np.int32), loglik_base=np.zeros(nl),
               status_base=np.full(nl, -1, np.int32), iters_base=np.full(nl, -1, np.int32), without={}, bound=np.zeros(n_iso),
               gap=np.zeros(n_iso), theta_max=np.zeros(n_iso))
    for l in range(nl):
        for i in range(int(iso_off[l]), int(iso_off[l + 1])):
            if (keep is None or int(keep[i]) != 0) and loo_status[l] == TOO_WIDE:
                out["support"][i] = LOCUS_SKIPPED

    def ll_bound(q):
        rows, cols = subs[q][4].shape
        r_e = 2.0 * (rows + 8) * FU.U + 2.0 * (2.0 * (cols + 4) * FU.U) + 4.0 * FU.U
        return 2.0 * (rows + FU.K) * FU.U * float(fit["abs_loglik"][q]) + float(fit["n_live"][q]) * r_e

    q = 0
    while q < len(subs):
        l, _, kept, _, _ = subs[q]
        i0, K = int(iso_off[l]), len(kept)
        tb = [float(x) for x in thetas[q]]
        out["loglik_base"][l] = fit["loglik"][q]
        if sub_status is not None:
            out["status_base"][l], out["iters_base"][l] = sub_status[q], sub_iters[q]
        for r, j in enumerate(kept):
            out["theta_refit"][i0 + j] = tb[r]
        lost_base = int(fit["n_dropped"][q]) + int(fit["n_impossible"][q])
        if K == 1:
            i = i0 + kept[0]
            out["support"][i], out["lr_stat"][i] = SOLE, math.inf
            out["n_unique"][i] = int(fit["n_live"][q]) - int(fit["n_impossible"][q])
            q += 1
            continue
        tmax = max(max((abs(float(x)) for x in thetas[q + s]), default=0.0) for s in range(K + 1))
        for r, j in enumerate(kept):
            s, i = q + 1 + r, i0 + j
            assert subs[s][0] == l and subs[s][1] == j
            ts = [float(x) for x in thetas[s]]
            out["support"][i] = TESTED
            if sub_status is not None:
                out["status_without"][i], out["iters_without"][i] = sub_status[s], sub_iters[s]
            nu = int(fit["n_dropped"][s]) + int(fit["n_impossible"][s]) - lost_base
            out["n_unique"][i] = nu
            out["lr_stat"][i] = math.inf if nu > 0 else 2.0 * (float(fit["loglik"][q]) - float(fit["loglik"][s]))
            out["bound"][i] = 2.0 * (ll_bound(q) + ll_bound(s))
            best, second, heir = 0.0, 0.0, -1
            others = [k for k in range(K) if k != r]
            for c, k in enumerate(others):
                gain = ts[c] - tb[k]
                if gain > best:
                    best, second, heir = gain, best, kept[k]
                elif gain > second:
                    second = gain
            out["heir"][i], out["heir_gain"][i], out["gap"][i], out["theta_max"][i] = heir, best, best - second, tmax
            out["without"][i] = np.array(ts)
        q += K + 1
    out["fit"], out["subs"] = fit, subs
    return out


def compare_exact(t, want, label=""):
    """every integer array, support, which statistics are +inf"""
    for k in ("loo_status", "n_unique", "support"):
        np.testing.assert_array_equal(getattr(t, k), want[k], err_msg="%s %s" % (label, k))
    np.testing.assert_array_equal(np.isposinf(t.lr_stat), np.isposinf(want["lr_stat"]), err_msg=label + " +inf")
    assert not np.isnan(t.lr_stat).any(), label


def compare_stat(t, want, label=""):
    """the finite statistics and the base's loglik under the bound -> the worst share of it"""
    fin = np.isfinite(want["lr_stat"])
    err = np.abs(t.lr_stat[fin] - want["lr_stat"][fin])
    tested = want["support"][fin] == TESTED
    assert (err[~tested] == 0.0).all(), label
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(err == 0.0, 0.0, err / want["bound"][fin])
    assert not (err > want["bound"][fin]).any(), (label, float(share.max()), int(np.argmax(share)))
    return float(share.max()) if share.size else 0.0


def census(t):
    """candidates, +inf, statistic < 3.84, negative, TOO_WIDE loci"""
    c = t.support == TESTED
    return dict(candidates=int(c.sum()), inf=int(np.isposinf(t.lr_stat[c]).sum()), below_3_84=int((t.lr_stat[c] < 3.84).sum()),
                negative=int((t.lr_stat[c] < 0).sum()), smallest=float(t.lr_stat[c].min()) if c.any() else 0.0,
                too_wide=int((t.loo_status == TOO_WIDE).sum()))
