"""The isoform information restated (include/sbgpu.h: sbgpu_em_info_*), for tests/test_isoform_info*.py: no code
shared with the library.  by_hand() makes, per locus, its own decision of who is free, observed and retained (its own
factorisation, in Python floats), and then -- given ITS retained set R -- the covariance by one of two routes:

  exact   (loci of at most EXACT_ISO isoforms and EXACT_BINS bins) fractions.Fraction throughout: the inputs are doubles, hence
          rationals; c_j, d_b, w_b, H_R, its inverse by Gauss-Jordan, u, t and cov are exact, and cov is rounded once.
  numpy   (larger loci) fp64: H from one matrix product, the inverse of C_R by np.linalg.inv.

THE BOUNDS (u = 2^-52; rows the locus' bins, k = |R|, kappa = the 2-norm condition number of the scaled matrix C_R).
  either form against by_hand, elementwise on cov:
    B = (rows + 8 + k^2) u kappa max|Hinv_R|
      -- rows + 8: the sums over the bins and the handful of roundings of w_b, c_j and the scaling in every entry of H; k^2: the
      factorisation, the triangular inverse and Y^T Y, each entry a sum of at most k products over k steps; kappa: how an
      entrywise relative error of C_R reaches its inverse; max|Hinv_R|: cov's entries are Hinv's minus a projection no larger.
    se            sqrt(B) + 2 u se          (|sqrt(a) - sqrt(b)| <= sqrt(|a - b|); the sqrt's own rounding)
    partner_corr  B / (se_j se_k) + |corr| (B / (2 cov_jj) + B / (2 cov_kk)) + 4 u |corr|   (first order through the quotient;
                  not compared where B exceeds a quarter of either variance: the first order says nothing there)
    partner       compared only where its gap to the runner-up clears four times that bound
    min_pivot     (rows + 8 + k^2) u kappa  (absolute: C has a unit diagonal, a pivot is one of its entries less a sum of k squares)
  ident, rank, alias_of, n_free, info_status: exact, except that a locus is left out of the comparison of R (and of what
  follows from R) when one of by_hand's pivots lies in [BAND_LO, BAND_HI] around SBGPU_INFO_PIVOT_EPS: there the decision rests
  on a rounding.  At most 2 % of a golden's loci may be left out.
  device against host: bitwise (tests/test_isoform_info_gpu.py).
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -52
ROW_EPS = 1e-5          # SBGPU_EM_ROW_EPS
PIVOT_EPS = 1e-9        # SBGPU_INFO_PIVOT_EPS
BAND_LO, BAND_HI = 1e-10, 1e-8
INIT_EMPTY = 1
IDENTIFIED, ALIASED, UNOBSERVED, NOT_FREE, SKIPPED = range(5)
OK, EMPTY, TOO_WIDE = range(3)
EXACT_ISO, EXACT_BINS = 8, 64
MAX_FREE = 64           # the exported limit (checked against info.limits() by the tests)


def _factorise(C):
    """C: list of lists (observed free isoforms, scaled).  The rule's factorisation without pivoting, in plain floats ->
    (retained indices, pivots of all, alias_of per index or -1)"""
    n = len(C)
    Lm = [[0.0] * n for _ in range(n)]
    R, piv, alias = [], [0.0] * n, [-1] * n
    for j in range(n):
        p = C[j][j] - sum(Lm[j][k] * Lm[j][k] for k in R)
        piv[j] = p
        if not p > PIVOT_EPS:
            best = -1.0
            for k in R:
                if abs(Lm[j][k]) > best:
                    best, alias[j] = abs(Lm[j][k]), k
            continue
        Lm[j][j] = math.sqrt(p)
        for i in range(j + 1, n):
            Lm[i][j] = (C[i][j] - sum(Lm[i][k] * Lm[j][k] for k in R)) / Lm[j][j]
        R.append(j)
    return R, piv, alias


def _gauss_jordan(M):
    """the inverse of a square matrix of Fractions (non-singular), exactly"""
    n = len(M)
    A = [list(M[i]) + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[p] = A[p], A[c]
        inv = 1 / A[c][c]
        A[c] = [x * inv for x in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    return [row[n:] for row in A]


def locus_by_hand(n, W, theta, kept, exact):
    """One locus.  n [nb] ints, W [nb][niso] floats, theta [niso] floats, kept [niso] bools -> dict(status, n_free, ident [niso],
    alias_of [niso], rank, pivots (of the observed free, in order), band (a pivot in [BAND_LO, BAND_HI]), R (isoform indices), cov
    [niso, niso], se [niso], B (the bound on cov's entries), kappa, route)"""
    nb, niso = len(n), len(theta)
    out = dict(status=EMPTY, n_free=0, ident=[NOT_FREE] * niso, alias_of=[-1] * niso, rank=0, pivots=[], band=False, R=[],
               cov=np.zeros((niso, niso)), se=np.zeros(niso), B=0.0, kappa=1.0, rows=nb, route="exact" if exact else "numpy", min_pivot=0.0)
    live = [any(w > ROW_EPS for w in W[b]) for b in range(nb)]
    c = [0.0] * niso
    for j in range(niso):
        for b in range(nb):
            if live[b]:
                c[j] += W[b][j]
    free = [j for j in range(niso) if kept[j] and c[j] != 0.0 and theta[j] / c[j] > 0.0]
    if not free:
        return out
    if len(free) > MAX_FREE:
        out.update(status=TOO_WIDE, ident=[SKIPPED] * niso)
        return out
    out.update(status=OK, n_free=len(free))
    usable = [j for j in range(niso) if kept[j] and c[j] != 0.0]
    if exact:
        cx = [sum((Fraction(W[b][j]) for b in range(nb) if live[b]), Fraction(0)) for j in range(niso)]
        wx = [Fraction(0)] * nb
        for b in range(nb):
            if live[b] and n[b] > 0:
                d = sum((Fraction(theta[j]) * Fraction(W[b][j]) / cx[j] for j in usable), Fraction(0))
                if d > 0:
                    wx[b] = Fraction(n[b]) / (d * d)
        bins = [b for b in range(nb) if wx[b] != 0]
        Hx = {(j, k): sum((wx[b] * Fraction(W[b][j]) * Fraction(W[b][k]) for b in bins), Fraction(0)) / (cx[j] * cx[k])
              for j in free for k in free if j <= k}
        H = {jk: float(v) for jk, v in Hx.items()}
    else:
        Wm, cm = np.asarray(W, np.float64).reshape(nb, niso), np.asarray(c)
        g = np.zeros(niso)
        g[usable] = np.asarray(theta)[usable] / cm[usable]
        d = Wm @ g
        ok = np.asarray(live) & (d > 0.0)
        wv = np.zeros(nb)
        wv[ok] = np.asarray(n, np.float64)[ok] / d[ok] / d[ok]
        Ff = Wm[:, free] / cm[free]
        Hm = (Ff * wv[:, None]).T @ Ff
        H = {(j, k): float(Hm[a, b]) for a, j in enumerate(free) for b, k in enumerate(free) if j <= k}
    obs = [j for j in free if H[(j, j)] > 0.0]
    for j in free:
        if j not in obs:
            out["ident"][j] = UNOBSERVED
    sym = lambda j, k: H[(j, k)] if j <= k else H[(k, j)]  # noqa: E731
    dg = {j: math.sqrt(H[(j, j)]) for j in obs}
    C = [[sym(j, k) / (dg[j] * dg[k]) for k in obs] for j in obs]
    Rl, piv, alias = _factorise(C)
    R = [obs[a] for a in Rl]
    for a, j in enumerate(obs):
        out["ident"][j] = IDENTIFIED if a in Rl else ALIASED
        if a not in Rl and alias[a] >= 0:
            out["alias_of"][j] = obs[alias[a]]
    out.update(rank=len(R), pivots=piv, R=R, band=any(BAND_LO <= p <= BAND_HI for p in piv),
               min_pivot=min((piv[a] for a in Rl), default=0.0))
    k = len(R)
    if not k:
        return out
    CR = np.array([[C[a][b] for b in Rl] for a in Rl])
    out["kappa"] = float(np.linalg.cond(CR)) if k > 1 else 1.0
    if exact:
        Hinv = _gauss_jordan([[Hx[(j, kk)] if j <= kk else Hx[(kk, j)] for kk in R] for j in R])
        u = [sum(row, Fraction(0)) for row in Hinv]
        t = sum(u, Fraction(0))
        cov = np.array([[float(Hinv[a][b] - u[a] * u[b] / t) if t > 0 else float(Hinv[a][b]) for b in range(k)] for a in range(k)])
        hmax = max(abs(float(x)) for row in Hinv for x in row)
    else:
        dgR = np.array([dg[j] for j in R])
        Hinv = np.linalg.inv(CR) / np.outer(dgR, dgR)
        u = Hinv.sum(axis=1)
        t = u.sum()
        cov = Hinv - np.outer(u, u) / t if t > 0 else Hinv
        hmax = float(np.abs(Hinv).max())
    out["B"] = (nb + 8 + k * k) * U * out["kappa"] * hmax
    out["cov"][np.ix_(R, R)] = cov
    out["se"][R] = np.sqrt(np.maximum(np.diag(cov), 0.0))
    return out


def by_hand(batch, theta, keep=None, status=None, loci=None, exact_limit=None, exact_cost=None):
    """-> list of locus_by_hand dicts (None for the loci not in `loci`).  Every locus that is small enough takes the exact route,
    unless the caller rations it for the suite's time (the rationals of a 61 x 8 locus take seconds): exact_limit: at most that
    many loci take it; exact_cost: only loci with bins x isoforms^3 up to that do.  The others take the numpy route."""
    row_off, iso_off, f_off = (np.asarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    nl = len(row_off) - 1
    out, n_exact = [None] * nl, 0
    for l in (range(nl) if loci is None else loci):
        b0, i0, f0 = int(row_off[l]), int(iso_off[l]), int(f_off[l])
        nb, niso = int(row_off[l + 1]) - b0, int(iso_off[l + 1]) - i0
        n = [int(x) for x in batch.count[b0:b0 + nb]]
        W = [[float(x) for x in batch.F[f0 + b * niso:f0 + (b + 1) * niso]] for b in range(nb)]
        started = status is None or int(status[l]) != INIT_EMPTY
        kept = [started and (keep is None or int(keep[i0 + j]) != 0) for j in range(niso)]
        exact = niso <= EXACT_ISO and nb <= EXACT_BINS and (exact_limit is None or n_exact < exact_limit) and (exact_cost is None or nb * niso ** 3 <= exact_cost)
        n_exact += exact
        out[l] = locus_by_hand(n, W, [float(x) for x in theta[i0:i0 + niso]], kept, exact)
    return out


def corr_bound(cov, se, B, j, k):
    """the bound on corr_jk (see the head of this file); inf where the first order says nothing"""
    vj, vk = cov[j, j], cov[k, k]
    if not (vj > 4.0 * B and vk > 4.0 * B):
        return math.inf
    corr = cov[j, k] / (se[j] * se[k])
    return B / (se[j] * se[k]) + abs(corr) * (B / (2.0 * vj) + B / (2.0 * vk)) + 4.0 * U * abs(corr)


def compare(got, want, batch, label="", max_left_out=0.02):
    """got: an info.IsoformInfo (either form) with every array; want: by_hand()'s list.  Asserts the decisions exactly and cov, se,
    partner_corr, partner under the bounds at the head of this file -> dict(share: the worst share of cov's bound, left_out: the
    loci whose R was not compared, n_cov: loci whose cov was compared)"""
    iso_off = np.asarray(batch.iso_off, np.int64)
    nl = len(iso_off) - 1
    worst, left_out, n_cov, where = 0.0, [], 0, None
    for l in range(nl):
        w = want[l]
        if w is None:
            continue
        i0, niso = int(iso_off[l]), int(iso_off[l + 1] - iso_off[l])
        ident = got.ident[i0:i0 + niso]
        assert got.info_status[l] == w["status"], (label, l, "info_status", int(got.info_status[l]), w["status"])
        assert got.n_free[l] == w["n_free"], (label, l, "n_free")
        free_got = [j for j in range(niso) if ident[j] not in (NOT_FREE, SKIPPED)]
        free_want = [j for j in range(niso) if w["ident"][j] not in (NOT_FREE, SKIPPED)]
        assert free_got == free_want, (label, l, "who is free")
        assert [j for j in range(niso) if ident[j] == UNOBSERVED] == [j for j in range(niso) if w["ident"][j] == UNOBSERVED], (label, l, "unobserved")
        if w["status"] != OK:
            assert (ident == (SKIPPED if w["status"] == TOO_WIDE else NOT_FREE)).all() and got.rank[l] == 0 and got.min_pivot[l] == 0.0, (label, l)
            assert not got.se[i0:i0 + niso].any() and (got.partner[i0:i0 + niso] == -1).all() and (got.alias_of[i0:i0 + niso] == -1).all(), (label, l)
            continue
        if w["band"]:
            left_out.append(l)
            continue
        assert list(ident) == w["ident"], (label, l, "ident", list(ident), w["ident"], w["pivots"])
        assert got.rank[l] == w["rank"], (label, l, "rank")
        assert list(got.alias_of[i0:i0 + niso]) == w["alias_of"], (label, l, "alias_of", list(got.alias_of[i0:i0 + niso]), w["alias_of"])
        if w["rank"]:
            assert abs(got.min_pivot[l] - w["min_pivot"]) <= (w["rows"] + 8 + w["rank"] ** 2) * U * w["kappa"], (label, l, "min_pivot")
        cov = got.covariance(l)
        R, B = w["R"], w["B"]
        if cov is not None:
            n_cov += 1
            out_R = [j for j in range(niso) if j not in R]
            assert not cov[out_R, :].any() and not cov[:, out_R].any(), (label, l, "cov outside R")
            err = np.abs(cov - w["cov"])
            if R:
                share = float(err.max() / B) if err.max() > 0 else 0.0
                if share > worst:
                    worst, where = share, (l, w["route"], len(R), w["kappa"])
                assert share <= 1.0, (label, l, "cov", share, w["route"], w["kappa"])
        se = got.se[i0:i0 + niso]
        assert (np.abs(se - w["se"]) <= math.sqrt(B) + 2.0 * U * w["se"]).all(), (label, l, "se")
        assert not se[[j for j in range(niso) if j not in R]].any(), (label, l, "se outside R")
        # the partner, where by_hand's own choice does not rest on a rounding
        for j in range(niso):
            pj, pc = int(got.partner[i0 + j]), float(got.partner_corr[i0 + j])
            if j not in R:
                assert pj == -1 and pc == 0.0, (label, l, j, "partner outside R")
                continue
            cand = []
            for k in R:
                if k != j and w["se"][j] > 0 and w["se"][k] > 0:
                    cand.append((abs(w["cov"][j, k] / (w["se"][j] * w["se"][k])), k, corr_bound(w["cov"], w["se"], B, j, k)))
            if not cand:
                continue    # (by_hand sees no candidate; a form whose se differs from 0 by a rounding may)
            cand.sort(key=lambda x: (-x[0], x[1]))
            tol = max(x[2] for x in cand)
            gap = cand[0][0] - (cand[1][0] if len(cand) > 1 else -math.inf)
            if math.isfinite(tol) and gap > 4.0 * tol:
                k = cand[0][1]
                assert pj == k, (label, l, j, "partner", pj, k)
                assert abs(pc - w["cov"][j, k] / (w["se"][j] * w["se"][k])) <= cand[0][2], (label, l, j, "partner_corr")
    assert len(left_out) <= max_left_out * nl, (label, "loci left out of the comparison of R", left_out)
    return dict(share=worst, where=where, left_out=left_out, n_cov=n_cov)


def bitwise(a, b, label="", names=None):
    """every array of two IsoformInfos, bit for bit"""
    from strawberry_amd.info import NAMES
    for k in names or NAMES:
        x, y = getattr(a, k), getattr(b, k)
        np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y,
                                      err_msg="%s %s" % (label, k))
