"""The model fit restated (include/sbgpu.h: sbgpu_em_fit_*) in Python floats and plain loops, for
tests/test_model_fit*.py: no code shared with the library.  The posterior scale is written as theta_j * (F / c_j), not as the
library's (theta_j / c_j) * F, so a bin's mass differs from the library's by its roundings.  by_hand() also returns, per locus,
the sum of |terms| of each signed sum and the other figures the bounds below are made of.

THE BOUNDS (derived in DESIGN 3.22; u = 2^-52, rows / niso the locus' bins and isoforms).
  device against host: both hold the same d_b, n_b / d_b, c_j bits; D and the three sums are added in another order.
    counts, dof, which bins are possible, the zeros, score          exact
    expected        relative  R_e = (rows + 8 + 4) u        (D's order; two roundings of its own in each form)
    resid           absolute  (sqrt(e) + |r|) (R_e + 6 u)   (e's error through (n - e) / sqrt(e); subtraction, sqrt, division in each form)
    pearson         (rows + 8) u pearson + 2 (R_e + 6 u) sum |r| (sqrt(e) + |r|)
    loglik          (rows + K) u sum |terms| + n_live (rows + 8) u
    deviance        (rows + K) u sum |terms| + 2 n_live R_e
  either form against by_hand: twice the summation term, and the masses' own roundings r_d = 2 (niso + 4) u:
    expected        relative  R_E = 2 (rows + 8) u + 2 r_d + 4 u
    resid           absolute  (sqrt(e) + |r|) (R_E + 6 u)
    score           relative  2 (rows + 8) u + r_d + 4 u
    pearson         2 (rows + 8) u pearson + 2 (R_E + 6 u) sum |r| (sqrt(e) + |r|)
    loglik          2 (rows + K) u sum |terms| + n_live R_E
    deviance        2 (rows + K) u sum |terms| + 2 n_live R_E
  K = the device log's error in ulps (LOG_ULP_DEVICE, measured on the MI355X run: tests/test_model_fit_gpu.py) + the host's 1 + 8.
"""
import math

import numpy as np

U = 2.0 ** -52
ROW_EPS = 1e-5          # SBGPU_EM_ROW_EPS
THETA_CHANGE_LIMIT = 1e-2
INIT_EMPTY = 1
LOG_ULP_DEVICE = 1      # largest distance seen between the device's and the host's log over these tests' arguments
K = LOG_ULP_DEVICE + 1 + 8
PER_LOCUS = ("loglik", "deviance", "pearson", "n_live", "n_dropped", "n_impossible", "dof", "worst_bin")


def by_hand(batch, theta, keep=None, status=None):
    """-> dict of numpy arrays: the eleven results; possible [n_bins] bool; per locus abs_loglik, abs_deviance (sum of |terms|),
    pearson_sens (sum of |r| (sqrt(e) + |r|)), step_norm (|| theta o score - theta ||_2), M, resid_gap (largest |resid| minus the
    second largest: a worst_bin closer than its bound is not compared)"""
    row_off, iso_off, f_off = (np.asarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count, F = [int(x) for x in batch.count], [float(x) for x in batch.F]
    theta = [float(x) for x in theta]
    nl, n_bins, n_iso = len(row_off) - 1, int(row_off[-1]), int(iso_off[-1])
    out = {k: np.zeros(n_bins) for k in ("expected", "resid")}
    out["possible"] = np.zeros(n_bins, bool)
    out["score"] = np.zeros(n_iso)
    for k in ("loglik", "deviance", "pearson", "abs_loglik", "abs_deviance", "pearson_sens", "step_norm", "resid_gap"):
        out[k] = np.zeros(nl)
    for k in ("n_live", "n_dropped", "n_impossible", "M"):
        out[k] = np.zeros(nl, np.int64)
    out["dof"], out["worst_bin"] = np.zeros(nl, np.int32), np.full(nl, -1, np.int32)
    for l in range(nl):
        b0, i0, f0 = int(row_off[l]), int(iso_off[l]), int(f_off[l])
        nb, niso = int(row_off[l + 1]) - b0, int(iso_off[l + 1]) - i0
        n = count[b0:b0 + nb]
        W = [F[f0 + b * niso:f0 + (b + 1) * niso] for b in range(nb)]
        started = status is None or int(status[l]) != INIT_EMPTY
        kept = [started and (keep is None or int(keep[i0 + j]) != 0) for j in range(niso)]
        live = [any(w > ROW_EPS for w in W[b]) for b in range(nb)]
        if not any(kept):
            out["n_dropped"][l] = sum(n)
            continue
        c = [0.0] * niso
        for j in range(niso):
            for b in range(nb):
                if live[b]:
                    c[j] += W[b][j]
        usable = [kept[j] and c[j] != 0.0 for j in range(niso)]
        d = [0.0] * nb
        for b in range(nb):
            if live[b]:
                for j in range(niso):
                    if usable[j]:
                        d[b] += theta[i0 + j] * (W[b][j] / c[j])
        possible = [live[b] and d[b] > 0.0 for b in range(nb)]
        n_live = sum(n[b] for b in range(nb) if live[b])
        n_imp = sum(n[b] for b in range(nb) if live[b] and not possible[b])
        M = n_live - n_imp
        D = 0.0
        for b in range(nb):
            if possible[b]:
                D += d[b]
        out["n_live"][l], out["n_dropped"][l], out["n_impossible"][l], out["M"][l] = n_live, sum(n) - n_live, n_imp, M
        P, A = sum(possible), sum(1 for j in range(niso) if usable[j] and theta[i0 + j] / c[j] > 0.0)
        out["dof"][l] = max(0, P - 1 - max(0, A - 1))
        ll = dev = pear = abs_ll = abs_dev = sens = 0.0
        best, second, best_b = -1.0, -1.0, -1
        for b in range(nb):
            if not possible[b]:
                continue
            e = float(M) * (d[b] / D)
            r = (float(n[b]) - e) / math.sqrt(e) if e > 0.0 else 0.0
            out["expected"][b0 + b], out["resid"][b0 + b], out["possible"][b0 + b] = e, r, True
            if n[b] > 0:
                t1 = float(n[b]) * math.log(d[b] / D)
                t2 = 2.0 * float(n[b]) * math.log(float(n[b]) / e) if e > 0.0 else math.inf
                ll, dev, abs_ll, abs_dev = ll + t1, dev + t2, abs_ll + abs(t1), abs_dev + abs(t2)
            pear += r * r
            sens += abs(r) * (math.sqrt(e) + abs(r))
            if abs(r) > best:
                best, second, best_b = abs(r), best, b
            elif abs(r) > second:
                second = abs(r)
        out["loglik"][l], out["deviance"][l], out["pearson"][l] = ll, dev, pear
        out["abs_loglik"][l], out["abs_deviance"][l], out["pearson_sens"][l] = abs_ll, abs_dev, sens
        out["worst_bin"][l], out["resid_gap"][l] = best_b, best - max(second, 0.0)
        step = 0.0
        for j in range(niso):
            s = 0.0
            for b in range(nb):
                if possible[b]:
                    s += (float(n[b]) / d[b]) * W[b][j]
            sc = s / c[j] if usable[j] else 0.0
            out["score"][i0 + j] = sc
            step += (theta[i0 + j] * sc - theta[i0 + j]) ** 2
        out["step_norm"][l] = math.sqrt(step)
    return out


def shapes(batch):
    """-> (rows, niso) per locus, and the locus of every bin and of every isoform"""
    rows, niso = np.diff(np.asarray(batch.row_off, np.int64)), np.diff(np.asarray(batch.iso_off, np.int64))
    nl = len(rows)
    return rows, niso, np.repeat(np.arange(nl), rows), np.repeat(np.arange(nl), niso)


def tree_sum(x, threads, wave=64):
    """The device's reduction tree (csrc/fit_device.h) over one locus' per-bin terms x, restated: thread t adds its bins t,
    t + threads, ... in ascending order; inside a wave lane i adds lane i + s for s = 32 .. 1; a workgroup of four waves adds
    (w0 + w1) + (w2 + w3)."""
    x = np.asarray(x, np.float64)
    p = np.zeros(threads)
    for k in range(0, len(x), threads):
        part = x[k:k + threads]
        p[:len(part)] = p[:len(part)] + part
    w = p.reshape(threads // wave, wave).copy()
    s = wave // 2
    while s >= 1:
        w[:, :s] = w[:, :s] + w[:, s:2 * s]
        s //= 2
    w = w[:, 0]
    return float(w[0]) if len(w) == 1 else float((w[0] + w[1]) + (w[2] + w[3]))


def compare(got, want, batch, against_by_hand, label="", exact_from=None):
    """got: a fit.ModelFit (host or device form); want: by_hand()'s dict, or -- against_by_hand False -- the host form's ModelFit
    with exact_from = by_hand()'s dict for the figures of the bounds.  Asserts every array under the bounds at the head of this
    file -> the worst share of each bound, for the reports."""
    rows, niso, bin_locus, iso_locus = shapes(batch)
    fig = want if against_by_hand else exact_from
    get = (lambda k: np.asarray(want[k])) if against_by_hand else (lambda k: np.asarray(getattr(want, k)))
    for k in ("n_live", "n_dropped", "n_impossible", "dof"):
        np.testing.assert_array_equal(getattr(got, k), get(k), err_msg="%s %s" % (label, k))
    possible = fig["possible"]
    assert ((got.expected != 0.0) <= possible).all() and (got.resid[~possible] == 0.0).all(), label
    np.testing.assert_array_equal(got.expected == 0.0, get("expected") == 0.0, err_msg=label + " expected's zeros")
    rd = 2.0 * (niso + 4) * U
    if against_by_hand:
        r_e = 2.0 * (rows + 8) * U + 2.0 * rd + 4.0 * U
        r_s = 2.0 * (rows + 8) * U + rd + 4.0 * U
        sum_term, log_term = 2.0 * (rows + 8) * U, 2.0 * (rows + K) * U
        ll_d = fig["n_live"] * r_e
    else:
        r_e = (rows + 12) * U
        r_s = np.zeros(len(rows))
        sum_term, log_term = (rows + 8) * U, (rows + K) * U
        ll_d = fig["n_live"] * (rows + 8) * U
    e, r = np.asarray(fig["expected"]), np.asarray(fig["resid"])
    bound = {"expected": r_e[bin_locus] * np.abs(get("expected")),
             "resid": (np.sqrt(e) + np.abs(r)) * (r_e[bin_locus] + 6.0 * U),
             "score": r_s[iso_locus] * np.abs(get("score")),
             "pearson": sum_term * fig["pearson"] + 2.0 * (r_e + 6.0 * U) * fig["pearson_sens"],
             "loglik": log_term * fig["abs_loglik"] + ll_d,
             "deviance": log_term * fig["abs_deviance"] + 2.0 * fig["n_live"] * r_e}
    share = {}
    for k, b in bound.items():
        err = np.abs(np.asarray(getattr(got, k)) - get(k))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(err == 0.0, 0.0, err / b)
        share[k] = float(s.max()) if s.size else 0.0
        assert not (err > b).any(), (label, k, share[k], int(np.argmax(s)))
    # the worst bin, where the restatement's own decision does not rest on a rounding: the gap to the runner-up clears four
    # times the largest bound of a residual of the locus
    tol = np.zeros(len(rows))
    np.maximum.at(tol, bin_locus, bound["resid"])
    clear = np.asarray(fig["resid_gap"]) > 4.0 * tol
    np.testing.assert_array_equal(np.asarray(got.worst_bin)[clear], np.asarray(fig["worst_bin"])[clear], err_msg=label + " worst_bin")
    return share


def worst_bin_of(resid, possible, row_off):
    """the rule's argmax over one's own resid bits: strict > in ascending order over the possible bins, -1 when there is none"""
    out = np.full(len(row_off) - 1, -1, np.int32)
    for l in range(len(row_off) - 1):
        best = -1.0
        for b in range(int(row_off[l]), int(row_off[l + 1])):
            if possible[b] and abs(resid[b]) > best:
                best, out[l] = abs(resid[b]), b - int(row_off[l])
    return out


def tile_batch(batch, reps):
    """the batch's loci `reps` times over, as a LocusBatch"""
    from strawberry_amd.synth import LocusBatch
    cat = lambda off: np.concatenate([[0], np.cumsum(np.tile(np.diff(off), reps))]).astype(np.int64)  # noqa: E731
    return LocusBatch(cat(batch.row_off), cat(batch.iso_off), cat(batch.f_off), np.tile(batch.count, reps), np.tile(batch.F, reps),
                      np.tile(batch.length, reps), "tiled")


def from_loci(loci):
    """[(count, F rows x niso), ...] -> LocusBatch"""
    from strawberry_amd.synth import from_loci as f
    return f([(np.asarray(n, np.int32), np.asarray(F, np.float64).reshape(len(n), -1)) for n, F in loci])


def select_loci(batch, idx):
    """the loci idx of the batch, in that order, as a LocusBatch"""
    from strawberry_amd.synth import LocusBatch
    idx = np.asarray(idx, np.int64)
    rows, niso = np.diff(batch.row_off)[idx], np.diff(batch.iso_off)[idx]
    pick = lambda off, n: np.concatenate([np.arange(int(off[l]), int(off[l]) + int(k)) for l, k in zip(idx, n)] + [np.zeros(0, np.int64)]).astype(np.int64)  # noqa: E731
    cat = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int64)  # noqa: E731
    return LocusBatch(cat(rows), cat(niso), cat(rows * niso), np.asarray(batch.count)[pick(batch.row_off, rows)],
                      np.asarray(batch.F)[pick(batch.f_off, rows * niso)], np.asarray(batch.length)[pick(batch.iso_off, niso)], "selected")


def per_locus_slices(values, off, idx):
    """values laid out by `off`, for the loci idx in that order"""
    return np.concatenate([np.asarray(values)[int(off[l]):int(off[l + 1])] for l in idx] + [np.asarray(values)[:0]])


def bitwise(a, b, label=""):
    """every array of two ModelFits, bit for bit"""
    from strawberry_amd.fit import NAMES
    for k in NAMES:
        x, y = getattr(a, k), getattr(b, k)
        np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y,
                                      err_msg="%s %s" % (label, k))
