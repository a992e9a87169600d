"""The differential isoform usage between two groups of replicates restated (include/sbgpu.h: sbgpu_em_gdiff_*) in
Python floats and plain loops, for tests/test_group_usage*.py: no code shared with the library.  The sub-matrices are made by
deleting columns, alpha in Python floats in the rule's order (the sum in sample order from its first term, the quotient, the
division), the stacking by concatenation, every fit -- own, at the group's theta, at ALL's -- by fit_util.by_hand, rules 5-9
in Python floats.  The caller passes the theta, status and iterations of every sub-problem.

THE BOUND of a statistic: 2 x the sum, over the fits that enter it, of diff_util._ll_bound for the fit's sub-problem's shape
(the project's own "either form against by_hand" loglik bound; no new tolerance).  lr_between: every present sample's fit at
its group's theta (its own fit where the group is a singleton) and at ALL's; lr_within: the own and the group fit of every
present sample of a group with two or more present samples."""
import numpy as np

import diff_util as DU
import fit_util as FU

MAX_KEPT, MAX_POOLED_BINS, MAX_SAMPLES = 512, 5632, 16
OK, EMPTY, SOLE, TOO_WIDE, TOO_DEEP, _ONE_SAMPLE, UNSOLVED, ONE_GROUP, THIN = range(9)
OWN, GROUP_A, GROUP_B, ALL = range(4)
DENOM_ZERO = 2
PER_ISO = ("theta_sample", "theta_group", "theta_all", "usage_sample", "usage_group", "usage_all", "delta_usage")
INTS = ("n_frag", "lost_shift", "dof_between", "dof_within", "p_a", "p_b", "gdiff_status", "top_iso", "status_sample", "iters_sample", "status_group",
        "iters_group", "status_all", "iters_all")
LOGLIKS = ("loglik_own", "loglik_group", "loglik_all")
MODES = ("null", "shift", "overdispersed", "subset", "absent")


def kept_columns(batches, keeps, l):
    i0, i1 = int(batches[0].iso_off[l]), int(batches[0].iso_off[l + 1])
    keeps = keeps if keeps is not None else [None] * len(batches)
    return [i - i0 for i in range(i0, i1) if any(k is None or int(k[i]) != 0 for k in keeps)]


def sub_problems(batches, n_a, keeps=None):
    """-> (status [n_loci] before the solves, p_a, p_b [n_loci], [(locus, kind, sample or -1, kept columns, count, F rows x K)])"""
    S = len(batches)
    status, p_a, p_b, subs = [], [], [], []
    for l in range(len(batches[0].iso_off) - 1):
        kept = kept_columns(batches, keeps, l)
        loci = [DU._locus(b, l) for b in batches]
        present = [s for s in range(S) if len(loci[s][0]) > 0]
        groups = [[s for s in present if s < n_a], [s for s in present if s >= n_a]]
        K = len(kept)
        rows = sum(len(loci[s][0]) for s in present)
        st = (EMPTY if K == 0 else SOLE if K == 1 else TOO_WIDE if K > MAX_KEPT else ONE_GROUP if not groups[0] or not groups[1]
              else TOO_DEEP if rows > MAX_POOLED_BINS else OK)
        status.append(st), p_a.append(len(groups[0])), p_b.append(len(groups[1]))
        if st != OK:
            continue
        niso = loci[0][1].shape[1]
        gone = [j for j in range(niso) if j not in kept]
        own = {s: np.delete(loci[s][1], gone, axis=1) for s in present}
        c = {}
        for s in present:
            cs = [0.0] * K
            for row in own[s]:
                if any(float(w) > FU.ROW_EPS for w in row):
                    for k in range(K):
                        cs[k] += float(row[k])
            c[s] = cs
        for s in present:
            subs.append((l, OWN, s, kept, loci[s][0].copy(), own[s]))
        for kind, pool in ((GROUP_A, groups[0]), (GROUP_B, groups[1]), (ALL, present)):
            if kind != ALL and len(pool) < 2:
                continue
            total = []
            for k in range(K):
                t = c[pool[0]][k]
                for s in pool[1:]:
                    t = t + c[s][k]
                total.append(t)
            parts = []
            for s in pool:
                alpha = [(total[k] / c[s][k]) / float(len(pool)) if c[s][k] != 0.0 else 1.0 for k in range(K)]
                parts.append(np.array([[float(row[k]) * alpha[k] for k in range(K)] for row in own[s]], np.float64).reshape(len(own[s]), K))
            subs.append((l, kind, -1, kept, np.concatenate([loci[s][0] for s in pool]), np.concatenate(parts, axis=0)))
    return np.array(status, np.int32), np.array(p_a, np.int32), np.array(p_b, np.int32), subs


def sub_batch(subs):
    return DU.batch_of([(n, F) for _, _, _, _, n, F in subs])


def solve_each(oracle, subs):
    """the oracle's EM on every sub-problem by itself -> thetas, status, iters"""
    res = [oracle.em_locus(n, F) for _, _, _, _, n, F in subs]
    return [r[0] for r in res], np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32)


def by_hand(batches, n_a, keeps, thetas, statuses, iters):
    """thetas: one array per sub-problem, in sub_problems' order; statuses, iters: the solves' -> dict of the 26 results (the
    per-sample ones [S, n], the per-group ones [2, n]); `bound_between`, `bound_within`, `bound_ll` [n_loci]; `gap`, `top_abs`
    [n_loci] as diff_util.by_hand's; `subs`."""
    S = len(batches)
    iso_off = np.asarray(batches[0].iso_off, np.int64)
    nl, n_iso = len(iso_off) - 1, int(iso_off[-1])
    pre, p_a, p_b, subs = sub_problems(batches, n_a, keeps)
    assert len(thetas) == len(subs) == len(statuses) == len(iters)
    out = dict(theta_sample=np.zeros((S, n_iso)), usage_sample=np.zeros((S, n_iso)), theta_group=np.zeros((2, n_iso)), usage_group=np.zeros((2, n_iso)),
               theta_all=np.zeros(n_iso), usage_all=np.zeros(n_iso), delta_usage=np.zeros(n_iso))
    for k in ("lr_between", "lr_within", "bound_between", "bound_within", "bound_ll", "gap", "top_abs"):
        out[k] = np.zeros(nl)
    for k in LOGLIKS:
        out[k] = np.zeros((S, nl))
    out["n_frag"], out["lost_shift"] = np.zeros((S, nl), np.int64), np.zeros(nl, np.int64)
    out["dof_between"], out["dof_within"], out["p_a"], out["p_b"] = np.zeros(nl, np.int32), np.zeros(nl, np.int32), p_a, p_b
    out["gdiff_status"], out["top_iso"] = pre.copy(), np.full(nl, -1, np.int32)
    out["status_sample"], out["iters_sample"] = np.full((S, nl), -1, np.int32), np.full((S, nl), -1, np.int32)
    out["status_group"], out["iters_group"] = np.full((2, nl), -1, np.int32), np.full((2, nl), -1, np.int32)
    out["status_all"], out["iters_all"] = np.full(nl, -1, np.int32), np.full(nl, -1, np.int32)
    # ---- a locus' sub-problems by slot: its samples', its groups' (a singleton's is its sample's), ALL's
    by_locus = {}
    for q, (l, kind, s, _, _, _) in enumerate(subs):
        d = by_locus.setdefault(l, dict(own={}, group={}, all=None))
        if kind == OWN:
            d["own"][s] = q
        elif kind == ALL:
            d["all"] = q
        else:
            d["group"][kind - GROUP_A] = q
    fits = None
    if subs:
        sb = sub_batch(subs)
        src = [[], []]
        for q, (l, kind, s, _, _, _) in enumerate(subs):
            d = by_locus[l]
            src[0].append(d["group"].get(int(s >= n_a), q) if kind == OWN else q)
            src[1].append(d["all"] if kind == OWN else q)
        cat = lambda idx: np.concatenate([np.asarray(thetas[i], np.float64) for i in idx])  # noqa: E731
        st = np.asarray(statuses, np.int32)
        fits = [FU.by_hand(sb, cat(range(len(subs))), None, st), FU.by_hand(sb, cat(src[0]), None, st[src[0]]), FU.by_hand(sb, cat(src[1]), None, st[src[1]])]
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
        j = kept_columns(batches, keeps, l)[0]
        placed = [float((DU._locus(b, l)[0] > 0).any()) for b in batches]
        g = [max(placed[:n_a]), max(placed[n_a:])]
        for s in range(S):
            out["usage_sample"][s, i0 + j] = placed[s]
        out["usage_group"][0, i0 + j], out["usage_group"][1, i0 + j], out["usage_all"][i0 + j] = g[0], g[1], max(g)
        out["delta_usage"][i0 + j] = g[1] - g[0]
        top_of(l, i0, [j])
    for l, d in by_locus.items():
        own, fit, gfit, afit = d["own"], fits[0], fits[1], fits[2]
        kept = subs[d["all"]][3]
        i0, K = int(iso_off[l]), len(kept)
        single = [int(p_a[l]) < 2, int(p_b[l]) < 2]
        group_q = [d["group"].get(g, next(q for s, q in own.items() if (s >= n_a) == bool(g))) for g in (0, 1)]
        for s, q in own.items():
            out["status_sample"][s, l], out["iters_sample"][s, l] = statuses[q], iters[q]
        for g in (0, 1):
            out["status_group"][g, l], out["iters_group"][g, l] = statuses[group_q[g]], iters[group_q[g]]
        out["status_all"][l], out["iters_all"][l] = statuses[d["all"]], iters[d["all"]]
        n_frag = {s: int(fit["n_live"][q]) - int(fit["n_impossible"][q]) for s, q in own.items()}
        if any(n_frag[s] == 0 or statuses[q] == FU.INIT_EMPTY for s, q in own.items()):
            out["gdiff_status"][l] = THIN
            continue
        if DENOM_ZERO in [statuses[q] for q in list(own.values()) + list(d["group"].values()) + [d["all"]]]:
            out["gdiff_status"][l] = UNSOLVED
            continue
        between = within = None
        shift = lost(fit, d["all"])
        bb = bw = 0.0
        for s in sorted(own):
            q, g = own[s], int(s >= n_a)
            shape = subs[q][5].shape
            ll_own, ll_all = float(fit["loglik"][q]), float(afit["loglik"][q])
            ll_grp = ll_own if single[g] else float(gfit["loglik"][q])
            loss_b, loss_w = ll_grp - ll_all, 0.0 if single[g] else ll_own - ll_grp
            between = loss_b if between is None else between + loss_b
            within = loss_w if within is None else within + loss_w
            out["loglik_own"][s, l], out["loglik_group"][s, l], out["loglik_all"][s, l], out["n_frag"][s, l] = ll_own, ll_grp, ll_all, n_frag[s]
            shift += -lost(fit, q) + (0 if single[g] else lost(gfit, q) - lost(fit, q)) + (lost(afit, q) - lost(fit, q))
            b_own, b_grp, b_all = DU._ll_bound(fit, q, shape), DU._ll_bound(gfit, q, shape), DU._ll_bound(afit, q, shape)
            bb += (b_own if single[g] else b_grp) + b_all
            bw += 0.0 if single[g] else b_own + b_grp
            out["bound_ll"][l] = max(out["bound_ll"][l], b_own, b_grp, b_all)
        for g, q in d["group"].items():
            shift += lost(fit, q) - sum(lost(fit, own[s]) for s in own if (s >= n_a) == bool(g))
        out["lr_between"][l], out["lr_within"][l] = 2.0 * between, 2.0 * within
        out["bound_between"][l], out["bound_within"][l] = 2.0 * bb, 2.0 * bw
        out["lost_shift"][l], out["dof_between"][l], out["dof_within"][l] = shift, K - 1, (len(own) - 2) * (K - 1)

        def scatter(q, theta_row, usage_row):
            t = [float(v) for v in thetas[q]]
            total = 0.0
            for v in t:
                total += v
            for r, j in enumerate(kept):
                theta_row[i0 + j] = t[r]
                usage_row[i0 + j] = t[r] / total if total != 0.0 else 0.0
        for s, q in own.items():
            scatter(q, out["theta_sample"][s], out["usage_sample"][s])
        for g in (0, 1):
            scatter(group_q[g], out["theta_group"][g], out["usage_group"][g])
        scatter(d["all"], out["theta_all"], out["usage_all"])
        for j in kept:
            out["delta_usage"][i0 + j] = float(out["usage_group"][1, i0 + j]) - float(out["usage_group"][0, i0 + j])
        top_of(l, i0, kept)
    out["subs"], out["fits"] = subs, fits
    return out


def compare(t, want, label="", exact_doubles=True, top_margin=None, restrict=()):
    """t: a gdiff.GroupDifferentialUsage; want: by_hand()'s dict.  Every integer and status exact; theta / usage / delta bit for bit
    (exact_doubles); the log-likelihoods and the two statistics under their bounds; top_iso as diff_util.compare holds it: where
    the top |delta| clears the runner-up by top_margin (None: everywhere), on the OK loci of three or more kept isoforms without
    `restrict` -> (the worst share of a bound, the loci of the set left out, the set's size, the two-isoform loci)."""
    for k in INTS:
        if k != "top_iso":
            np.testing.assert_array_equal(getattr(t, k), want[k], err_msg="%s %s" % (label, k))
    if exact_doubles:
        for k in PER_ISO:
            np.testing.assert_array_equal(getattr(t, k).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (label, k))
    tie_of_zeros = (want["top_abs"] == 0.0) & (np.add.reduceat(np.concatenate([np.abs(t.delta_usage), [0.0]]), t.iso_off[:-1]) * (np.diff(t.iso_off) > 0) == 0.0)
    clear = np.ones(len(want["gap"]), bool) if top_margin is None else (want["gap"] > top_margin) | (want["top_iso"] < 0) | tie_of_zeros
    np.testing.assert_array_equal(t.top_iso[clear], want["top_iso"][clear], err_msg=label + " top_iso")
    worst = 0.0
    for name, bound in (("lr_between", "bound_between"), ("lr_within", "bound_within")):
        got = getattr(t, name)
        assert np.isfinite(got).all(), (label, name)
        err = np.abs(got - want[name])
        assert (err[want[bound] == 0.0] == 0.0).all(), (label, name)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(err == 0.0, 0.0, err / want[bound])
        assert not (err > want[bound]).any(), (label, name, float(share.max()), int(np.argmax(share)))
        worst = max(worst, float(share.max()) if share.size else 0.0)
    for k in LOGLIKS:
        assert (np.abs(getattr(t, k) - want[k]) <= want["bound_ll"][None, :]).all(), (label, k)
    pair = (want["gdiff_status"] == OK) & (want["dof_between"] == 1)
    top_set = (want["gdiff_status"] == OK) & (want["dof_between"] > 1)
    top_set[list(restrict)] = False
    return worst, int((~clear & top_set).sum()), int(top_set.sum()), int(pair.sum())


def _expected_counts(rng, F, th, total):
    """counts multinomial from theta under the sample's OWN column scales: p_b proportional to sum_j theta_j F_bj / c_j over its
    live rows -- the model's `expected`, as diff_util.second_sample draws them"""
    live = (F > FU.ROW_EPS).any(axis=1) if F.size else np.zeros(len(F), bool)
    c = F[live].sum(axis=0) if F.size else np.zeros(F.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(c != 0.0, th / c, 0.0)
    d = np.where(live, F @ g, 0.0) if F.size else np.zeros(len(F))
    return (rng.multinomial(total, d / d.sum()) if d.sum() > 0 and total else np.zeros(len(F), np.int64)).astype(np.int32)


def replicates(batch, mode, n_a, n_b, seed, theta, concentration=30.0):
    """n_a + n_b samples over batch's annotation -> (batches_a, batches_b).  Sample s has F x (1 + 0.1 s) and, per locus, the
    batch's total count, multinomial from a theta under the sample's own column scales.  null: every sample from `theta` (the
    batch's oracle theta).  shift: group B from theta reversed within the locus.  overdispersed: each sample's theta drawn
    Dirichlet(concentration x the group's shares) around the group's (both groups' is `theta`: null with biological variation).
    subset: a sorted random two-thirds of each locus' rows per sample, then as null.  absent: as null, and sample s has no bins
    at the loci l with (l + s) % 5 == 0 -- with one sample in a group, that group is absent there."""
    assert mode in MODES
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_a + n_b):
        loci = []
        for l in range(batch.n_loci):
            n, F = DU._locus(batch, l)
            i0, i1 = int(batch.iso_off[l]), int(batch.iso_off[l + 1])
            th = np.asarray(theta[i0:i1], np.float64)
            if mode == "shift" and s >= n_a:
                th = th[::-1]
            if mode == "overdispersed" and th.sum() > 0:
                a = concentration * th / th.sum()
                th = np.where(a > 0, rng.dirichlet(np.maximum(a, 1e-3)), 0.0)
            if mode == "subset" and len(n):
                F = F[np.sort(rng.choice(len(n), max(1, (2 * len(n)) // 3), replace=False))]
            if mode == "absent" and (l + s) % 5 == 0:
                F = F[:0]
            F = F * (1.0 + 0.1 * s)
            loci.append((_expected_counts(rng, F, th, int(n.sum())), F))
        b = DU.batch_of(loci)
        assert (np.asarray(b.iso_off) == np.asarray(batch.iso_off)).all()
        out.append(b)
    return out[:n_a], out[n_a:]


def census(t):
    """loci compared (OK, lost_shift 0), rejected at 0.05 under both p-values, the dispersion's median"""
    ok = (t.gdiff_status == OK) & (t.lost_shift == 0)
    out = dict(loci=int(len(ok)), compared=int(ok.sum()), shifted=int(((t.gdiff_status == OK) & (t.lost_shift != 0)).sum()))
    for method in ("chi2", "quasi"):
        p = t.p_value(method)
        with np.errstate(invalid="ignore"):
            out["rejected_" + method] = int((p[ok] < 0.05).sum())
    phi = t.dispersion()[ok]
    out["median_dispersion"] = float(np.nanmedian(phi)) if np.isfinite(phi).any() else float("nan")
    return out
