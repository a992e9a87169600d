"""The drop-one isoform support built on the device (sbgpu_em_loo_device / sbgpu_model_loo_device, csrc/loo_device.h) against the
host form and tests/support_util.py::by_hand: on the five EM goldens (the expansion bit for bit, every sub-problem's theta against
the oracle under the EM tests' contract, the integers exactly, the statistics under the bound of support_util.py); loci on either
side of every threshold the library exports; past two passes of both grids; chunked against unchunked; two calls; every position
among the other retained-result stages; through quantify_resident and the front quantifier; the refusals."""
import ctypes as C

import numpy as np
import pytest

import fit_util as FU
import support_util as SU
from strawberry_amd import _lib, assign, context, coverage, fit, info, support
from test_em_gpu import THETA_FLOOR, THETA_RTOL

pytestmark = pytest.mark.gpu

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
DENOM_ZERO = 2
HEIR_MARGIN = 4e-9      # x max |theta| of the locus: THETA_RTOL on both sides of both terms of a gain


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def within_limits(b):
    lim = support.limits()
    idx = np.nonzero((np.diff(b.row_off) <= lim["max_bins"]) & (np.diff(b.iso_off) <= lim["max_iso"]))[0]
    return b if len(idx) == b.n_loci else FU.select_loci(b, idx)


def device_thetas(t, sh):
    """every sub-problem's theta as the device solved it, from theta_refit and the packed theta_without -> one array per sub-problem"""
    iso_off, out = t.iso_off, []
    for l, drop in zip(sh["sub_locus"], sh["sub_drop"]):
        i0, i1 = int(iso_off[l]), int(iso_off[l + 1])
        kept = np.ones(i1 - i0, bool) if t.keep is None else t.keep[i0:i1] != 0
        if drop < 0:
            out.append(t.theta_refit[i0:i1][kept])
        else:
            kept[drop] = False
            out.append(t.theta_without(l, drop)[kept])
    return out


def device_solves(t, sh):
    """status and iterations of every sub-problem"""
    st, it = [], []
    for l, drop in zip(sh["sub_locus"], sh["sub_drop"]):
        i = int(t.iso_off[l]) + drop
        st.append(t.status_base[l] if drop < 0 else t.status_without[i])
        it.append(t.iters_base[l] if drop < 0 else t.iters_without[i])
    return np.array(st, np.int32), np.array(it, np.int32)


def check_device(t, b, keep, oracle, label, heirs=True):
    """t (made with_sub_batch) against the host expansion, the oracle's solves and by_hand -> the worst share of the bound"""
    sh = t.sub
    count, F = support.expand_host(b, keep)
    np.testing.assert_array_equal(sh["count"], count, err_msg=label)
    np.testing.assert_array_equal(sh["F"].view(np.uint64), F.view(np.uint64), err_msg=label)
    o_theta, o_status, o_iters = oracle.em_batch(sh["row_off"], sh["iso_off"], sh["f_off"], count, F)
    thetas = device_thetas(t, sh)
    got = np.concatenate(thetas + [np.zeros(0)])
    err = np.abs(got - o_theta) / np.maximum(np.abs(o_theta), THETA_FLOOR)
    assert err.size == 0 or err.max() < THETA_RTOL, (label, err.max())
    st, it = device_solves(t, sh)
    np.testing.assert_array_equal(st, o_status, err_msg=label)
    dz = o_status == DENOM_ZERO
    np.testing.assert_array_equal(it[~dz], o_iters[~dz], err_msg=label)
    assert (np.abs(it[dz] - o_iters[dz]) <= 1).all(), label      # (include/sbgpu.h: unspecified by one for a failed solve)
    # by_hand fed the oracle's theta: the integers, and heir where the decision does not rest on the solvers' agreement
    split = lambda x: [x[int(a):int(c)] for a, c in zip(sh["iso_off"][:-1], sh["iso_off"][1:])]  # noqa: E731
    if heirs:
        ref = SU.by_hand(b, keep, split(o_theta), o_status, o_iters)
        SU.compare_exact(t, ref, label)
        c = ref["support"] == SU.TESTED
        clear = c & (ref["gap"] > HEIR_MARGIN * ref["theta_max"])
        np.testing.assert_array_equal(t.heir[clear], ref["heir"][clear], err_msg=label + " heir")
        left_out = int(c.sum() - clear.sum())
        assert left_out <= 0.05 * c.sum(), (label, left_out, int(c.sum()))
        print(label, "heir compared for all but %d of %d candidates" % (left_out, int(c.sum())))
    # by_hand fed the device's theta: the statistics
    want = SU.by_hand(b, keep, thetas, st, it)
    SU.compare_exact(t, want, label)
    for k in ("theta_refit", "heir_gain"):
        np.testing.assert_array_equal(getattr(t, k).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (label, k))
    np.testing.assert_array_equal(t.heir, want["heir"], err_msg=label)
    fin = np.isfinite(want["loglik_base"])
    share = SU.compare_stat(t, want, label)
    assert fin.all()
    print(label, SU.census(t), "worst share of the bound %.4f" % share)
    return share


def bitwise(a, b, label=""):
    for k in support.NAMES + ("without",):
        x, y = getattr(a, k), getattr(b, k)
        np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y,
                                      err_msg="%s %s" % (label, k))


@pytest.fixture(scope="module")
def G(ctx, golden):
    from strawberry_amd import em
    out = {}
    for name in GOLDENS:
        b = within_limits(golden(name)[0])
        s = em.EmBatchSolver(b, ctx)
        out[name] = dict(b=b, s=s, t=s.run_loo(with_sub_batch=True), again=s.run_loo())
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_device_on_the_goldens(G, oracle, name):
    g = G[name]
    check_device(g["t"], g["b"], None, oracle, name)
    assert set(g["t"].device) == set(support.NAMES) | {"theta_without", "without_off"}
    few = g["s"].run_loo(want=("lr_stat", "support"))
    assert few.heir is None and few.without is None
    np.testing.assert_array_equal(few.lr_stat.view(np.uint64), g["t"].lr_stat.view(np.uint64))


@pytest.mark.parametrize("name", GOLDENS)
def test_two_calls_are_bitwise_equal(G, name):
    bitwise(G[name]["t"], G[name]["again"], name)


def test_erased_isoforms_on_the_device(ctx, oracle, golden):
    import torch
    from strawberry_amd import em
    b = within_limits(golden("em_c3_400")[0])
    keep = (np.random.default_rng(3).random(int(b.iso_off[-1])) < 0.6).astype(np.int32)
    s = em.EmBatchSolver(b, ctx)
    t = s.run_loo(d_keep=torch.from_numpy(keep).to(s.dev), with_sub_batch=True)
    check_device(t, b, keep, oracle, "em_c3_400 with 40 % erased", heirs=False)
    assert (t.support[keep == 0] == SU.NOT_KEPT).all() and (t.loo_status == SU.EMPTY).any()


def test_loci_on_either_side_of_every_threshold(ctx, oracle):
    """the expand kernel's row tiles at +-1 row for K = 2, 63, 64; K = 65 (TOO_WIDE) between them; 5632 x 2; one isoform"""
    from strawberry_amd import em
    lim = support.limits()
    rng = np.random.default_rng(17)
    loci = []
    for K in (2, 63, 64):
        rows = min(lim["tile_rows"], lim["tile_vals"] // K)
        for nb in ((rows - 1, rows, rows + 1, 2 * rows + 1) if K == 2 else (rows, rows + 1) if K == 63 else (rows - 1, rows + 1)):
            F = (rng.random((nb, K)) + 0.05) * (rng.random((nb, K)) < 0.5)
            loci.append((rng.integers(0, 20, nb), F))
    loci.append((rng.integers(0, 20, 30), rng.random((30, 65)) + 0.05))
    loci.append((rng.integers(0, 5, lim["max_bins"]), (rng.random((lim["max_bins"], 2)) + 0.05) * (rng.random((lim["max_bins"], 2)) < 0.7)))
    loci.append((rng.integers(1, 20, 7), rng.random((7, 1)) + 0.05))
    b = FU.from_loci(loci)
    s = em.EmBatchSolver(b, ctx)
    t = s.run_loo(with_sub_batch=True)
    check_device(t, b, None, oracle, "thresholds", heirs=False)
    assert list(t.loo_status[8:]) == [SU.TOO_WIDE, SU.OK, SU.OK] and (t.loo_status[:8] == SU.OK).all()
    assert t.support[-1] == SU.SOLE and (t.support[int(b.iso_off[8]):int(b.iso_off[9])] == SU.LOCUS_SKIPPED).all()


def test_more_loci_than_two_passes_of_both_grids(ctx, golden):
    """em_c2_64's loci repeated until the expand kernel's tiles and the statistics' isoforms both exceed two passes of their
    grids.  Every repeat of a locus gets the first batch's integers exactly; its thetas within the EM's contract (a locus in
    another batch is another wave's, and does not always get the same bits); its finite statistics within
    8 THETA_RTOL n: a relative error e of theta moves every log(d_b / D) by at most 2 e, a loglik by 2 e n, and the statistic is
    twice the difference of two."""
    import torch
    from strawberry_amd import em
    lim = support.limits()
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    base = golden("em_c2_64")[0]
    reps = max(2 * lim["grid_per_cu"] * cu // base.n_loci, 2 * cu * lim["threads"] // int(base.iso_off[-1])) + 1
    b = FU.tile_batch(base, reps)
    assert b.n_loci > 2 * lim["grid_per_cu"] * cu and int(b.iso_off[-1]) > 2 * cu * lim["threads"]
    first = em.EmBatchSolver(base, ctx).run_loo()
    t = em.EmBatchSolver(b, ctx).run_loo()
    for k in ("n_unique", "support", "status_without", "iters_without", "loo_status", "status_base", "iters_base"):
        np.testing.assert_array_equal(getattr(t, k).reshape(reps, -1), np.tile(getattr(first, k), (reps, 1)), err_msg=k)
    for k in ("theta_refit", "without"):
        x, f = getattr(t, k).reshape(reps, -1), getattr(first, k)
        assert (np.abs(x - f) / np.maximum(np.abs(f), THETA_FLOOR)).max() < THETA_RTOL, k
    n = np.repeat(np.add.reduceat(base.count.astype(np.int64), base.row_off[:-1]), np.diff(base.iso_off))
    fin = np.isfinite(first.lr_stat)
    np.testing.assert_array_equal(np.isfinite(t.lr_stat).reshape(reps, -1), np.tile(fin, (reps, 1)))
    err = np.abs(t.lr_stat.reshape(reps, -1)[:, fin] - first.lr_stat[fin])
    assert (err <= 8 * THETA_RTOL * n[fin]).all(), float((err / n[fin]).max())
    assert (first.support == SU.TESTED).all() and fin.any()


def test_chunked_against_one_chunk(G, oracle):
    g = G["em_c3_400"]
    b, one = g["b"], g["t"]
    budget = 8 * int(one.sub["f_off"][-1]) // 4
    t = g["s"].run_loo(max_bytes=budget, with_sub_batch=True)
    # (at least three chunks: the weights alone are four budgets)
    np.testing.assert_array_equal(t.sub["count"], one.sub["count"])
    np.testing.assert_array_equal(t.sub["F"].view(np.uint64), one.sub["F"].view(np.uint64))
    for k in ("n_unique", "support", "loo_status", "status_without", "status_base"):
        np.testing.assert_array_equal(getattr(t, k), getattr(one, k), err_msg=k)
    check_device(t, b, None, oracle, "em_c3_400 in chunks")
    tiny = g["s"].run_loo(max_bytes=1)      # every locus a chunk alone: any positive budget is legal
    np.testing.assert_array_equal(tiny.n_unique, one.n_unique)
    np.testing.assert_array_equal(np.isposinf(tiny.lr_stat), np.isposinf(one.lr_stat))


def test_in_every_position_among_the_other_stages(ctx):
    """On a toy directory: the support asked for first, last and between the five other stages; every stage's arrays are the
    first turn's bits, and the resident call's seven outputs are the bits of the same call with nothing behind it."""
    import torch
    import info_util as IU
    import stream_util as S
    from strawberry_amd.quantify import quantify_resident
    from test_context_table_gpu import RL, RUNS, assert_same_table, law_of, toy
    from test_fragment_assign_gpu import assert_same_assignment, bits
    from test_isoform_coverage_gpu import device_hits
    import coverage_util as CU
    which = "E2E"
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    kw = dict(long_read=bool(RUNS[which][1]), ctx=ctx, min_isoform_frac=RUNS[which][2])
    plain = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, **kw)
    r = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, keep_handle=True, with_context=True, keep_bootstrap=True, **kw)
    dev = torch.device("cuda", ctx.device)
    hits_of = np.bincount(hits.hit_locus, minlength=annot.n_loci)
    with r["handle"] as handle:
        d_hits, own = device_hits(hits, dev)
        d_theta, d_keep, d_status, d_mass = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (r["theta"], r["keep"], r["status"], hits.mass))
        calls = {"support": lambda: support.model_loo_device(ctx, handle, d_keep),
                 "info": lambda: info.model_info_device(ctx, handle, d_theta, d_keep, d_status),
                 "fit": lambda: fit.model_fit_device(ctx, handle, d_theta, d_keep, d_status),
                 "table": lambda: context.context_table_device(ctx, handle),
                 "assignment": lambda: assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass),
                 "coverage": lambda: coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)}
        others = ["info", "fit", "table", "assignment", "coverage"]
        orders = [tuple(others[:p] + ["support"] + others[p:]) for p in range(6)] + [tuple(["support"] + others[::-1])]
        turns = [(order, {k: calls[k]() for k in order}) for order in orders]
        del own
    first = turns[0][1]
    assert (first["support"].support == SU.TESTED).any() and (first["support"].theta_refit > 0).any()
    for order, got in turns[1:]:
        what = " -> ".join(order)
        bitwise(got["support"], first["support"], what)
        IU.bitwise(got["info"], first["info"], what)
        FU.bitwise(got["fit"], first["fit"], what)
        assert_same_table(got["table"], first["table"], what)
        assert_same_assignment(got["assignment"], first["assignment"], np.asarray(annot.iso_off), hits_of, what)
        CU.compare(got["coverage"], first["coverage"], annot, hits.hit_locus, False, what)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    with_support = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, with_support=True, **kw)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(with_support[k]), bits(plain[k]), err_msg=k)
    bitwise(with_support["isoform_support"], first["support"], "quantify_resident(with_support=True)")


def test_quantify_resident_with_support_on_the_edge_sample(ctx):
    import torch
    import retained_util as R
    import stream_util as S
    from strawberry_amd.quantify import InsertSize, quantify_resident
    from test_fragment_assign_gpu import bits
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small = R.n_small_for(cu)
    annot, hits = R.edge_sample(n_small, grid=R.GRID_PER_CU * cu)
    law = InsertSize(*R.LAW)
    kw = dict(ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    plain = quantify_resident(annot, hits, law, R.RL, hits.n_hits, **kw)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, with_support=True, **kw)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    t = r["isoform_support"]
    at = R.edge_layout(n_small)
    np.testing.assert_array_equal(t.iso_off, annot.iso_off)
    kept = r["keep"] != 0
    assert (t.support[~kept] == SU.NOT_KEPT).all() and (t.support[kept] != SU.NOT_KEPT).all()
    K = np.add.reduceat(np.concatenate([kept.astype(np.int64), [0]]), np.asarray(annot.iso_off[:-1]))[:annot.n_loci] * (np.diff(annot.iso_off) > 0)
    np.testing.assert_array_equal(t.loo_status, np.where(K == 0, SU.EMPTY, np.where(K > 64, SU.TOO_WIDE, SU.OK)))
    assert t.loo_status[at["EMPTY"]] == SU.EMPTY and (t.support == SU.TESTED).sum() > n_small and (t.support == SU.SOLE).any()
    print("edge sample", SU.census(t))


def test_front_quantifier_isoform_support(ctx):
    """FrontQuantifier.isoform_support() after step() and after stream_step(): the same records, the same bits"""
    from strawberry_amd import front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
            plain.isoform_support()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_bootstrap=True, **kw)
    try:
        q.step()
        theta = q.theta[:q.n_iso].copy()
        f1 = q.isoform_support()
        q.abundance_bootstrap(4, 3, replicates=False)
        bitwise(q.isoform_support(), f1, "behind a bootstrap")
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        assert q.stream_step()["chunks"] > 3
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        bitwise(q.isoform_support(), f1, "through the stream")
        assert (f1.support == SU.TESTED).sum() > q.n_loci // 4 and np.isfinite(f1.lr_stat).any()
        few = q.isoform_support(want=("support",))
        assert few.lr_stat is None
        np.testing.assert_array_equal(few.support, f1.support)
    finally:
        q.close()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, null arguments, theta_without without its
    offsets, wrong offsets, a negative budget."""
    from strawberry_amd import bootstrap, chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_loo(h, out=True, s=None, par=None):
        s = s or _lib.sbgpu_em_loo_t()
        rc = L.sbgpu_model_loo_device(ctx.h, h, q._out.d_keep, C.byref(par) if par is not None else None, None, C.byref(s) if out else None)
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_loo(h0)
        assert rc == _lib.SBGPU_EINVAL and why.startswith("sbgpu_model_loo_device:") and "without retention (sbgpu_bootstrap_keep was off" in why, why
        bootstrap.bootstrap_keep(ctx, True)
        h1 = call()
        rc, why = try_loo(h1, out=False)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        rc, why = try_loo(h1, par=_lib.sbgpu_loo_params_t(-1, 0))
        assert rc == _lib.SBGPU_EINVAL and "max_bytes is negative" in why, why
        packed, bad = np.zeros(16), np.zeros(q.n_iso + 1, np.int64)
        bad[-1] = 5
        s = _lib.sbgpu_em_loo_t()
        s.theta_without = packed.ctypes.data
        rc, why = try_loo(h1, s=s)
        assert rc == _lib.SBGPU_EINVAL and "theta_without is given without without_off" in why, why
        s.without_off = bad.ctypes.data
        rc, why = try_loo(h1, s=s)
        assert rc == _lib.SBGPU_EINVAL and "without_off is not sbgpu_em_loo_offsets'" in why, why
        f1 = support.model_loo_device(ctx, h1, int(q._out.d_keep), keep=q.keep[:q.n_iso])
        h2 = call()
        rc, why = try_loo(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        f2 = support.model_loo_device(ctx, h2, int(q._out.d_keep), keep=q.keep[:q.n_iso])
        bitwise(f2, f1, "the same call twice")
        s = _lib.sbgpu_em_loo_t()
        assert L.sbgpu_em_loo_device(ctx.h, None, None, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "sbgpu_em_loo_device: null argument" in L.sbgpu_last_error().decode()
        with pytest.raises(ValueError, match="give keep"):
            support.model_loo_device(ctx, h2, int(q._out.d_keep))
    finally:
        bootstrap.bootstrap_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()
