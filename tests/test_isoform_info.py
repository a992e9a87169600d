"""The isoform information on the host: sbgpu_em_info_host (csrc/info_host.cpp), the CPU statement of what the device form
computes, against tests/info_util.py::by_hand -- the rule of include/sbgpu.h restated without the library's code, exactly
(fractions) for small loci and in numpy for larger ones -- under the bounds at the head of info_util.py; the two
closed forms the rule implies; hand-made loci for every ident code and status; the refusals.

No GPU here: theta / status are the oracle's."""
import ctypes as C
import types

import numpy as np
import pytest

import fit_util as FU
import info_util as IU
from strawberry_amd import _lib, info

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
U = IU.U
# The goldens' loci that take the exact route: the first 60 of each whose rationals stay small (bins x isoforms^3 <= 2500: a
# few milliseconds each; a 61 x 8 locus takes four seconds); the others that are small enough take numpy's.  The hand-made loci
# below and test_exact_route_near_its_limit take the exact route unrationed.
EXACT_PER_GOLDEN, EXACT_COST = 60, 2500


@pytest.fixture(scope="module")
def G(oracle, golden):
    """name -> (batch, the oracle's theta, status, by_hand's list, the host form's IsoformInfo): computed once"""
    out = {}
    for name in GOLDENS:
        b, _, _ = golden(name)
        theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
        out[name] = (b, theta, status, IU.by_hand(b, theta, None, status, exact_limit=EXACT_PER_GOLDEN, exact_cost=EXACT_COST), info.em_info_host(b, theta, status=status))
    return out


def test_the_limits_are_the_restatements():
    lim = info.limits()
    assert lim["max_free"] == IU.MAX_FREE >= 64 and lim["max_bins"] == 5632 and lim["max_iso"] == 4096
    assert lim["wave_iso"] <= lim["max_free"] and lim["wave_vals"] <= lim["stage_vals"] and lim["wave_loci"] == 4 and lim["grid_per_cu"] >= 1
    assert info.PIVOT_EPS == IU.PIVOT_EPS


@pytest.mark.parametrize("name", GOLDENS)
def test_host_form_against_by_hand_on_the_goldens(G, name):
    b, theta, status, want, t = G[name]
    r = IU.compare(t, want, b, name)
    routes = [w["route"] for w in want]
    n_alias, n_unobs = int((t.ident == IU.ALIASED).sum()), int((t.ident == IU.UNOBSERVED).sum())
    print(name, "worst share of cov's bound %.4f at (locus, route, k, kappa) %s; exact route %d loci, numpy %d; left out %s; "
          "aliased isoforms %d in %d loci, unobserved %d, rank-deficient loci %d"
          % (r["share"], r["where"], routes.count("exact"), routes.count("numpy"), r["left_out"], n_alias,
             len({int(np.searchsorted(b.iso_off, i, side="right") - 1) for i in np.nonzero(t.ident == IU.ALIASED)[0]}), n_unobs,
             int(sum(1 for l, w in enumerate(want) if w["status"] == IU.OK and t.rank[l] < t.n_free[l]))))
    assert r["n_cov"] > 0
    # asked for alone, an array is the same; the others are not filled
    few = info.em_info_host(b, theta, status=status, want=("se", "rank"))
    assert few.cov is None and few.ident is None
    np.testing.assert_array_equal(few.se, t.se)
    np.testing.assert_array_equal(few.rank, t.rank)
    rows = list(t.rows(theta=theta))
    assert len(rows) == int(b.iso_off[-1]) and rows[0][:2] == (0, 0) and len(rows[0]) == 9
    cv = t.cv(theta)
    pos = np.asarray(theta)[:len(cv)] > 0
    np.testing.assert_array_equal(cv[pos], t.se[pos] / np.asarray(theta)[:len(cv)][pos])


def test_exact_route_near_its_limit(G):
    """One of em_c3_400's largest loci the exact route covers (7 isoforms, about 40 bins), unrationed"""
    b, theta, status, _, t = G["em_c3_400"]
    rows, niso = np.diff(b.row_off), np.diff(b.iso_off)
    ok = np.nonzero((niso == 7) & (rows <= 48) & (rows >= 32))[0]
    assert len(ok)
    l = int(ok[0])
    one, th = FU.select_loci(b, [l]), theta[b.iso_off[l]:b.iso_off[l + 1]]
    want = IU.by_hand(one, th, None, status[l:l + 1])
    assert want[0]["route"] == "exact"
    r = IU.compare(info.em_info_host(one, th, status=status[l:l + 1]), want, one, "near the limit")
    print("locus %d (%d x %d): share of cov's bound %.4f" % (l, rows[l], niso[l], r["share"]))


@pytest.mark.parametrize("name", GOLDENS)
def test_symmetry_row_sums_and_semidefiniteness(G, name):
    """cov is stored as one triangle (symmetric by construction); over R every row sums to 0 and cov is positive semi-definite,
    each within the bound B of info_util.py (a row is k entries; an eigenvalue moves by at most the matrix' norm, <= k B)."""
    b, theta, status, want, t = G[name]
    checked = 0
    for l, w in enumerate(want):
        cov = t.covariance(l)
        if w["status"] != IU.OK or w["band"] or cov is None or not w["R"]:
            continue
        R, k, B = w["R"], len(w["R"]), w["B"]
        c = cov[np.ix_(R, R)]
        assert (c == c.T).all()
        assert (np.abs(c.sum(axis=1)) <= 2 * k * B).all(), (name, l, float(np.abs(c.sum(axis=1)).max()), B)
        assert np.linalg.eigvalsh(c).min() >= -2 * k * B, (name, l)
        corr = t.correlation(l)
        seen = t.se[b.iso_off[l]:b.iso_off[l + 1]][R] > 0
        assert corr.shape == cov.shape and (np.abs(np.diag(corr)[R][seen] - 1.0) <= 4 * U).all()    # (sqrt, a product, a quotient)
        checked += 1
    assert checked > 0


def test_closed_form_one_isoform():
    """theta is the locus' total: given the total nothing can move, se = 0 up to the rounding of (x * x) / x"""
    b = FU.from_loci([([12, 18], [[0.2], [0.05]])])
    t = info.em_info_host(b, [30.0])
    want = IU.by_hand(b, [30.0])
    IU.compare(t, want, b, "one isoform")
    assert t.ident[0] == IU.IDENTIFIED and t.rank[0] == 1 and t.n_free[0] == 1 and t.partner[0] == -1 and t.partner_corr[0] == 0.0
    # Hinv = theta^2 / M = 30; cov = Hinv - (Hinv * Hinv) / Hinv: at most an ulp of Hinv away from 0
    assert abs(t.covariance(0)[0, 0]) <= 2 * U * 30.0 and t.se[0] <= np.sqrt(2 * U * 30.0)
    assert want[0]["cov"][0, 0] == 0.0 and want[0]["se"][0] == 0.0     # exactly 0 in exact arithmetic


def test_closed_form_disjoint_isoforms_is_the_multinomial():
    """Every bin is one isoform's alone and theta_j = n_j: cov = diag(n) - n n^T / M"""
    n = [3, 11, 7, 20]
    b = FU.from_loci([(n, np.diag([0.3, 0.07, 0.5, 0.011]))])
    t = info.em_info_host(b, np.asarray(n, np.float64))
    nv, M = np.asarray(n, np.float64), float(sum(n))
    want = np.diag(nv) - np.outer(nv, nv) / M
    np.testing.assert_allclose(t.covariance(0), want, rtol=0, atol=(4 + 8 + 16) * U * nv.max())
    np.testing.assert_allclose(t.se, np.sqrt(nv * (1 - nv / M)), rtol=64 * U)
    assert (t.ident == IU.IDENTIFIED).all() and t.rank[0] == 4 and t.info_status[0] == IU.OK
    np.testing.assert_allclose(t.min_pivot, 1.0, rtol=8 * U)
    # the strongest partner of each is the one of largest n_j n_k / (se_j se_k): isoform 3 for all, isoform 1 for isoform 3
    assert list(t.partner) == [3, 3, 3, 1] and (t.partner_corr < 0).all()
    IU.compare(t, IU.by_hand(b, nv), b, "disjoint")


def test_identical_columns_alias_the_later_one():
    F = [[.2, .2, 0], [.1, .1, .3], [.05, .05, .2], [0, 0, .4]]
    b = FU.from_loci([([5, 9, 4, 7], F)])
    theta = np.array([6.0, 6.0, 13.0])
    t = info.em_info_host(b, theta)
    assert list(t.ident) == [IU.IDENTIFIED, IU.ALIASED, IU.IDENTIFIED] and list(t.alias_of) == [-1, 0, -1]
    assert t.rank[0] == 2 and t.n_free[0] == 3 and t.info_status[0] == IU.OK
    cov = t.covariance(0)
    assert not cov[1, :].any() and not cov[:, 1].any() and t.se[1] == 0.0 and t.partner[1] == -1
    assert list(t.partner[[0, 2]]) == [2, 0] and t.partner_corr[0] == t.partner_corr[2] < 0
    IU.compare(t, IU.by_hand(b, theta), b, "identical columns")


def test_an_isoform_whose_bins_hold_no_count_is_unobserved():
    b = FU.from_loci([([5, 0, 9], [[.2, 0], [0, .3], [.1, 0]])])
    theta = np.array([14.0, 1e-3])
    t = info.em_info_host(b, theta)
    assert list(t.ident) == [IU.IDENTIFIED, IU.UNOBSERVED] and t.rank[0] == 1 and t.n_free[0] == 2
    assert t.se[1] == 0.0 and t.alias_of[1] == -1 and t.partner[1] == -1 and not t.covariance(0)[1].any()
    IU.compare(t, IU.by_hand(b, theta), b, "unobserved")


def test_an_erased_isoform_is_not_free():
    b = FU.from_loci([([5, 6, 7], [[.2, 0, .1], [.1, .1, .1], [0, .3, .2]])])
    theta = np.array([7.0, 5.0, 6.0])
    t = info.em_info_host(b, theta, keep=[1, 0, 1])
    assert list(t.ident) == [IU.IDENTIFIED, IU.NOT_FREE, IU.IDENTIFIED] and t.n_free[0] == 2
    cov = t.covariance(0)
    assert not cov[1, :].any() and not cov[:, 1].any() and cov[0, 0] > 0
    IU.compare(t, IU.by_hand(b, theta, [1, 0, 1]), b, "erased")
    assert info.em_info_host(b, theta).n_free[0] == 3


def test_init_empty_and_denom_zero_loci(oracle):
    from test_oracle import KATS
    loci, thetas, stats = [], [], []
    for name in ("toy", "all_dropped", "denom_zero", "toy"):
        _, n, F, _, _ = next(k for k in KATS if k[0] == name)
        loci.append((n, F))
    b = FU.from_loci(loci)
    theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    assert status[1] == IU.INIT_EMPTY and status[2] == 2
    t = info.em_info_host(b, theta, status=status)
    IU.compare(t, IU.by_hand(b, theta, None, status), b, "kats")
    assert t.info_status[1] == IU.EMPTY and (t.ident[b.iso_off[1]:b.iso_off[2]] == IU.NOT_FREE).all() and t.rank[1] == 0 and t.n_free[1] == 0
    assert t.info_status[2] == IU.OK            # DENOM_ZERO keeps its theta: the information is theta's
    # the neighbours of the two are what they are alone
    i0, i3 = slice(b.iso_off[0], b.iso_off[1]), slice(b.iso_off[3], b.iso_off[4])
    assert (t.se[i0].view(np.uint64) == t.se[i3].view(np.uint64)).all() and t.min_pivot[0] == t.min_pivot[3]


def wide_locus(nf, rng):
    """nf isoforms with a bin of their own each, plus one shared bin"""
    F = np.vstack([np.diag(rng.uniform(0.05, 0.5, nf)), rng.uniform(0.01, 0.1, (1, nf))])
    return rng.integers(1, 40, nf + 1), F


def test_a_too_wide_locus_between_two_ordinary_ones():
    rng = np.random.default_rng(5)
    lim = info.limits()["max_free"]
    small = ([5, 6, 7], [[.2, 0], [.1, .1], [0, .3]])
    b = FU.from_loci([small, wide_locus(lim + 1, rng), small, wide_locus(lim, rng)])
    theta = np.concatenate([[8.0, 10.0], np.full(lim + 1, 3.0), [8.0, 10.0], np.full(lim, 3.0)])
    t = info.em_info_host(b, theta)
    assert list(t.info_status) == [IU.OK, IU.TOO_WIDE, IU.OK, IU.OK] and list(t.n_free) == [2, 0, 2, lim] and t.rank[3] == lim
    wide = slice(b.iso_off[1], b.iso_off[2])
    assert (t.ident[wide] == IU.SKIPPED).all() and not t.se[wide].any() and (t.partner[wide] == -1).all() and t.min_pivot[1] == 0.0
    assert t.cov_off[2] == t.cov_off[1] and t.covariance(1) is None       # niso beyond the limit: no block
    alone = info.em_info_host(FU.from_loci([small]), [8.0, 10.0])
    for sl, l in ((slice(0, 2), 0), (slice(b.iso_off[2], b.iso_off[3]), 2)):
        assert (t.se[sl].view(np.uint64) == alone.se.view(np.uint64)).all() and (t.covariance(l) == alone.covariance(0)).all()
    IU.compare(t, IU.by_hand(b, theta), b, "too wide")


def test_a_tie_in_correlation_goes_to_the_lowest_index():
    """Three isoforms that are each other's mirror images: equal counts, equal weights, one bin each"""
    b = FU.from_loci([([8, 8, 8], np.diag([.25, .25, .25]))])
    t = info.em_info_host(b, [8.0, 8.0, 8.0])
    c = t.correlation(0)
    assert c[0, 1] == c[0, 2] == c[1, 2] < 0
    assert list(t.partner) == [1, 0, 0] and (t.partner_corr == c[0, 1]).all()


def test_cov_offsets():
    off = info.cov_offsets([0, 1, 1, 4, 4 + 64, 4 + 64 + 65])
    assert list(off) == [0, 1, 1, 7, 7 + 64 * 65 // 2, 7 + 64 * 65 // 2]
    assert list(info.cov_offsets([0])) == [0]
    with pytest.raises(_lib.SbgpuError, match="does not ascend"):
        info.cov_offsets([0, 3, 2])
    assert _lib.load().sbgpu_em_info_cov_offsets(None, 1, None) == _lib.SBGPU_EINVAL


def raw_host(batch_struct, theta, out=None):
    L = _lib.load()
    s = out if out is not None else _lib.sbgpu_em_info_t()
    rc = L.sbgpu_em_info_host(C.byref(batch_struct) if batch_struct is not None else None, theta, None, None, C.byref(s))
    return rc, L.sbgpu_last_error().decode()


def test_every_refusal_with_its_text():
    L = _lib.load()
    row_off, iso_off, f_off = (np.array(a, np.int64) for a in ([0, 2], [0, 1], [0, 2]))
    count, F, theta = np.array([1, 2], np.int32), np.array([.2, .1]), np.array([3.0])

    def struct(row_off=row_off, iso_off=iso_off, f_off=f_off, count=count, F=F, n=1):
        return _lib.sbgpu_batch_t(n, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, None if count is None else count.ctypes.data,
                                  None if F is None else F.ctypes.data)
    assert raw_host(struct(), theta.ctypes.data)[0] == _lib.SBGPU_OK
    for bad, text in ((dict(count=np.array([1, -2], np.int32)), "a negative count"),
                      (dict(row_off=np.array([1, 2], np.int64)), "must begin at 0"),
                      (dict(row_off=np.array([0, -1], np.int64)), "do not ascend"),
                      (dict(f_off=np.array([0, 3], np.int64)), "is not rows x isoforms"),
                      (dict(count=None), "null count or F"),
                      (dict(n=-1), "bad n_loci")):
        rc, msg = raw_host(struct(**bad), theta.ctypes.data)
        assert rc == _lib.SBGPU_EINVAL and text in msg and msg.startswith("sbgpu_em_info_host:"), (bad, rc, msg)
    rc, msg = raw_host(struct(), None)
    assert rc == _lib.SBGPU_EINVAL and "theta is needed" in msg
    rc, msg = raw_host(None, theta.ctypes.data)
    assert rc == _lib.SBGPU_EINVAL and "null argument" in msg
    # cov without its offsets, and with offsets that are not the batch's
    cov, good, bad_off = np.zeros(4), np.array([0, 1], np.int64), np.array([0, 2], np.int64)
    s = _lib.sbgpu_em_info_t()
    s.cov = cov.ctypes.data
    rc, msg = raw_host(struct(), theta.ctypes.data, s)
    assert rc == _lib.SBGPU_EINVAL and "cov is given without cov_off" in msg
    s.cov_off = bad_off.ctypes.data
    rc, msg = raw_host(struct(), theta.ctypes.data, s)
    assert rc == _lib.SBGPU_EINVAL and "cov_off is not sbgpu_em_info_cov_offsets'" in msg
    s.cov_off = good.ctypes.data
    assert raw_host(struct(), theta.ctypes.data, s)[0] == _lib.SBGPU_OK
    assert L.sbgpu_em_info_limits(None) == _lib.SBGPU_EINVAL
    with pytest.raises(_lib.SbgpuError, match="a negative count"):
        info.em_info_host(types.SimpleNamespace(row_off=row_off, iso_off=iso_off, f_off=f_off, count=[1, -2], F=F), theta)
    with pytest.raises(ValueError, match="theta holds 0 entries"):
        info.em_info_host(types.SimpleNamespace(row_off=row_off, iso_off=iso_off, f_off=f_off, count=count, F=F), [])
    with pytest.raises(ValueError, match="unknown arrays"):
        info.IsoformInfo(iso_off, want=("chi2",))
