"""The differential isoform usage built on the device (sbgpu_em_diff_device / sbgpu_model_diff_device, csrc/diff_device.h) against
the host form and tests/diff_util.py::by_hand: on the five EM goldens against three second samples (the expansion bit for bit,
every sub-problem's theta against the oracle under the EM tests' contract, the integers exactly, the statistic under the bound of
diff_util.py); loci on either side of every threshold the library exports; past two passes of every grid; chunked against
unchunked; two calls; every position among the other retained-result stages; two quantifiers on two contexts; the refusals."""
import ctypes as C

import numpy as np
import pytest

import diff_util as DU
import fit_util as FU
from strawberry_amd import _lib, diff
from test_em_gpu import THETA_FLOOR, THETA_RTOL

pytestmark = pytest.mark.gpu

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
MODES = ("same", "subset", "shift")
DENOM_ZERO = 2
TOP_MARGIN = 4e-9       # THETA_RTOL on both sides of both usages of a difference
TOP_CAP = 0.05          # of a set's loci of three or more kept isoforms, at most, may miss the margin and go uncompared
# em_edge has 9 or 10 such loci, so one that misses the margin is above the cap.  Two of them miss it with the ORACLE's theta alone,
# by their make: locus 3 (2 bins, 3 isoforms) has one isoform at theta 0 in both samples, so its two live usages sum to 1 and
# tie as a two-isoform locus' do; locus 6 (1 bin, 3 isoforms) has usages the weights alone fix, so every delta is 0 up to a
# rounding.  The set is restricted, the cap is not widened
TOP_RESTRICT = {"em_edge": [3, 6]}


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def within_limits(b):
    idx = np.nonzero((np.diff(b.row_off) <= 5632) & (np.diff(b.iso_off) <= 4096))[0]
    return b if len(idx) == b.n_loci else FU.select_loci(b, idx)


def run(ctx, a, b, keep_a=None, keep_b=None, **kw):
    """sbgpu_em_diff_device on two host batches -> DifferentialUsage"""
    import torch
    from strawberry_amd import em
    sa, sb = em.EmBatchSolver(a, ctx), em.EmBatchSolver(b, ctx)
    up = lambda k: None if k is None else torch.from_numpy(np.ascontiguousarray(k, np.int32)).to(sa.dev)  # noqa: E731
    return diff.em_diff_device(ctx, sa.plan, sa.d_count, sa.d_F, sb.plan, sb.d_count, sb.d_F, up(keep_a), up(keep_b), **kw)


def bitwise(x, y, label="", names=diff.NAMES):
    for k in names:
        p, q = getattr(x, k), getattr(y, k)
        np.testing.assert_array_equal(p.view(np.uint64) if p.dtype == np.float64 else p, q.view(np.uint64) if q.dtype == np.float64 else q,
                                      err_msg="%s %s" % (label, k))


def check_device(t, a, b, keep_a, keep_b, oracle, label, restrict=()):
    """t (made with_sub_batch) against the host expansion, the oracle's solves and by_hand -> the worst share of the bound.
    restrict: loci taken out of the set top_iso's margin is held on (diff_util.compare)"""
    sh = t.sub
    count, F = diff.expand_host(a, b, keep_a, keep_b)
    np.testing.assert_array_equal(sh["count"], count, err_msg=label)
    np.testing.assert_array_equal(sh["F"].view(np.uint64), F.view(np.uint64), err_msg=label)
    o_theta, o_status, o_iters = oracle.em_batch(sh["row_off"], sh["iso_off"], sh["f_off"], count, F)
    split = lambda x: [x[int(p):int(q)] for p, q in zip(sh["iso_off"][:-1], sh["iso_off"][1:])]  # noqa: E731
    o_thetas = split(o_theta)
    # the device's solves: statuses and iterations of every sub-problem; theta where the locus stayed OK (zeroed otherwise)
    st = np.array([(t.status_a, t.status_b, t.status_pooled)[k][l] for l, k in zip(sh["sub_locus"], sh["sub_kind"])], np.int32)
    it = np.array([(t.iters_a, t.iters_b, t.iters_pooled)[k][l] for l, k in zip(sh["sub_locus"], sh["sub_kind"])], np.int32)
    np.testing.assert_array_equal(st, o_status, err_msg=label)
    dz = o_status == DENOM_ZERO
    np.testing.assert_array_equal(it[~dz], o_iters[~dz], err_msg=label)
    assert (np.abs(it[dz] - o_iters[dz]) <= 1).all(), label      # (include/sbgpu.h: unspecified by one for a failed solve)
    thetas, worst = [], 0.0
    for q, (l, k) in enumerate(zip(sh["sub_locus"], sh["sub_kind"])):
        if t.diff_status[l] != DU.OK:
            thetas.append(o_thetas[q])
            continue
        kept = DU.kept_columns(a, keep_a, keep_b, l)
        got = (t.theta_a, t.theta_b, t.theta_pooled)[k][int(a.iso_off[l]):int(a.iso_off[l + 1])][kept]
        err = np.abs(got - o_thetas[q]) / np.maximum(np.abs(o_thetas[q]), THETA_FLOOR)
        worst = max(worst, float(err.max()))
        thetas.append(got)
    assert worst < THETA_RTOL, (label, worst)
    # by_hand fed the oracle's theta: the integers, and top_iso where the decision does not rest on the solvers' agreement; the
    # cases that miss the margin are counted, printed and capped for THIS set
    ref = DU.by_hand(a, b, keep_a, keep_b, o_thetas, o_status, o_iters)
    _, left_out, n_set, n_pair = DU.compare(t, ref, label + " (oracle's theta)", exact_doubles=False, top_margin=TOP_MARGIN, restrict=restrict)
    print(label, "top_iso: %d of %d loci of three or more kept isoforms miss the margin (%d two-isoform loci and %d named loci are not in the set)"
          % (left_out, n_set, n_pair, len(restrict)))
    assert left_out <= TOP_CAP * n_set, (label, left_out, n_set)
    # by_hand fed the device's theta: the statistics under the bound, usage, delta and every top_iso exactly
    want = DU.by_hand(a, b, keep_a, keep_b, thetas, st, it)
    share = DU.compare(t, want, label)[0]
    print(label, DU.census(t), "worst share of the bound %.4f, worst theta error %.3g" % (share, worst))
    return share


@pytest.fixture(scope="module")
def G(ctx, oracle, golden):
    out = {}
    for name in GOLDENS:
        a = within_limits(golden(name)[0])
        out[name] = dict(a=a, theta=oracle.em_batch(a.row_off, a.iso_off, a.f_off, a.count, a.F)[0])
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", GOLDENS)
def test_device_on_the_goldens(ctx, G, oracle, name, mode):
    a = G[name]["a"]
    b = DU.second_sample(a, mode, 5, G[name]["theta"])
    t = run(ctx, a, b, with_sub_batch=True)
    check_device(t, a, b, None, None, oracle, "%s %s" % (name, mode), TOP_RESTRICT.get(name, ()))
    assert set(t.device) == set(diff.NAMES)
    if mode == "same":
        np.testing.assert_array_equal(t.delta_usage, 0.0)
    if name == "em_c2_64":
        again = run(ctx, a, b)
        bitwise(again, t, "two calls in a row")
        few = run(ctx, a, b, want=("lr_stat", "diff_status"))
        assert few.theta_a is None and few.top_iso is None
        bitwise(few, t, "want", ("lr_stat", "diff_status"))


def test_filters_on_the_device(ctx, G, oracle):
    a = G["em_c3_400"]["a"]
    b = DU.second_sample(a, "subset", 9, G["em_c3_400"]["theta"])
    rng = np.random.default_rng(3)
    n_iso = int(a.iso_off[-1])
    keep_a, keep_b = (rng.random(n_iso) < 0.6).astype(np.int32), (rng.random(n_iso) < 0.6).astype(np.int32)
    t = run(ctx, a, b, keep_a, keep_b, with_sub_batch=True)
    check_device(t, a, b, keep_a, keep_b, oracle, "em_c3_400 subset, filtered")
    assert (t.diff_status == DU.EMPTY).any() and (t.diff_status == DU.SOLE).any()
    t = run(ctx, a, b, keep_a, None, with_sub_batch=True)
    check_device(t, a, b, keep_a, None, oracle, "em_c3_400 subset, A filtered")


def test_loci_on_either_side_of_every_threshold(ctx, oracle):
    """the expand kernel's row tiles at +-1 row for K = 2, 63, 64, 65 and 512 (the column-scale kernel's group / workgroup
    switch lies between 64 and 65); K = 513 (a batch's plan refuses a locus of 513 isoforms, so TOO_WIDE is the host form's
    alone: tests/test_differential_usage.py); 2816 + 2816 and 2816 + 2817 pooled bins; 5631 + 1; nb_B = 0; K = 1"""
    lim = diff.limits()
    rng = np.random.default_rng(17)
    loci_a, loci_b = [], []

    def add(na, nb, K, dense=0.5):
        for rows, out in ((na, loci_a), (nb, loci_b)):
            F = (rng.random((rows, K)) + 0.05) * (rng.random((rows, K)) < dense)
            out.append((rng.integers(0, 20, rows), F))

    for K in (2, 63, 64, 65, 512):
        rows = max(1, min(lim["tile_rows"], lim["tile_vals"] // K))
        add(rows - 1, rows + 1, K)
        add(rows, 2 * rows + 1, K)
    first_special = len(loci_a)
    add(2816, 2816, 2, 0.7)         # OK: 5632 pooled bins
    add(2816, 2817, 2, 0.7)         # TOO_DEEP
    add(5631, 1, 2, 0.7)            # OK
    add(7, 0, 3, 1.0)               # nb_B = 0: ONE_SAMPLE
    add(6, 4, 1, 1.0)               # SOLE
    add(9, 11, 4, 1.0)              # an ordinary one behind them
    a, b = DU.batch_of(loci_a), DU.batch_of(loci_b)
    t = run(ctx, a, b, with_sub_batch=True)
    check_device(t, a, b, None, None, oracle, "thresholds")
    assert (t.diff_status[:first_special] == DU.OK).all()
    assert list(t.diff_status[first_special:]) == [DU.OK, DU.TOO_DEEP, DU.OK, DU.ONE_SAMPLE, DU.SOLE, DU.OK]
    wide = DU.batch_of([(np.ones(2, np.int64), np.ones((2, 513)))])
    with pytest.raises(_lib.SbgpuError, match="more than 512 isoforms"):
        run(ctx, wide, wide)
    host = diff.em_diff_host(a, b, None, None, oracle.em_batch)
    bitwise(t, host, "device against host", ("n_a", "n_b", "lost_shift", "dof", "diff_status", "status_a", "status_b", "status_pooled"))


def test_more_work_than_two_passes_of_every_grid(ctx, golden):
    """em_c2_64's loci repeated until the expand kernel's tiles, the column-scale kernel's items and the statistics' isoforms
    all exceed two passes of their grids.  The expansion is the host form's bits; every repeat of a locus gets the first
    batch's integers exactly and its thetas within the EM's contract (a locus in another batch is another wave's, and does not
    always get the same bits)."""
    import torch
    lim = diff.limits()
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    base = golden("em_c2_64")[0]
    base_b = DU.second_sample(base, "same", 0)
    base_b.count[:] = np.random.default_rng(2).permutation(base_b.count)      # other counts on the same weights
    lanes = 64                                                               # a locus' group of lanes at most: 4 loci per item at least
    reps = max(2 * lim["grid_per_cu"] * cu * (lim["threads"] // lanes) // base.n_loci, 2 * cu * lim["threads"] // int(base.iso_off[-1])) + 1
    a, b = FU.tile_batch(base, reps), FU.tile_batch(base_b, reps)
    assert a.n_loci > 2 * lim["grid_per_cu"] * cu * (lim["threads"] // lanes) and int(a.iso_off[-1]) > 2 * cu * lim["threads"]
    first = run(ctx, base, base_b)
    t = run(ctx, a, b, with_sub_batch=True)
    count, F = diff.expand_host(a, b)
    np.testing.assert_array_equal(t.sub["count"], count)
    np.testing.assert_array_equal(t.sub["F"].view(np.uint64), F.view(np.uint64))
    for k in DU.INTS:
        if k != "top_iso":
            np.testing.assert_array_equal(getattr(t, k).reshape(reps, -1), np.tile(getattr(first, k), (reps, 1)), err_msg=k)
    for k in ("theta_a", "theta_b", "theta_pooled"):
        x, f = getattr(t, k).reshape(reps, -1), getattr(first, k)
        assert (np.abs(x - f) / np.maximum(np.abs(f), THETA_FLOOR)).max() < THETA_RTOL, k
    assert (first.diff_status == DU.OK).all()


def test_chunked_against_one_chunk(ctx, G, oracle):
    """At least four chunks against one: the expansion, every integer and every status are the same bits; theta follows the
    EM's contract (include/sbgpu.h, rule 4: a locus solved in another batch does not always return the same theta bits), so the
    chunked call is held against the oracle and by_hand as the unchunked one is.  A 1-byte budget: every locus a chunk alone."""
    a = G["em_c3_400"]["a"]
    b = DU.second_sample(a, "subset", 5, G["em_c3_400"]["theta"])
    one = run(ctx, a, b, with_sub_batch=True)
    budget = 8 * int(one.sub["f_off"][-1]) // 5       # the weights alone are five budgets
    t = run(ctx, a, b, max_bytes=budget, with_sub_batch=True)
    np.testing.assert_array_equal(t.sub["count"], one.sub["count"])
    np.testing.assert_array_equal(t.sub["F"].view(np.uint64), one.sub["F"].view(np.uint64))
    ints = [k for k in DU.INTS if k != "top_iso"]
    bitwise(t, one, "chunked", ints)
    check_device(t, a, b, None, None, oracle, "em_c3_400 in chunks")
    tiny = run(ctx, a, b, max_bytes=1)
    bitwise(tiny, one, "a 1-byte budget", ints)


def test_in_every_position_among_the_other_stages(ctx):
    """On a toy directory: the differential usage (of the sample against itself) asked for first, last and between the six other
    stages; every stage's arrays are the first turn's bits, and the resident call's seven outputs are the bits of the same call
    with nothing behind it."""
    import torch
    import info_util as IU
    import stream_util as S
    import coverage_util as CU
    from strawberry_amd import assign, context, coverage, fit, info, support
    from strawberry_amd.quantify import quantify_resident
    from test_context_table_gpu import RL, RUNS, assert_same_table, law_of, toy
    from test_fragment_assign_gpu import assert_same_assignment, bits
    from test_isoform_coverage_gpu import device_hits
    from test_isoform_support_gpu import bitwise as support_bitwise
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
        calls = {"diff": lambda: diff.model_diff_device(ctx, handle, ctx, handle, d_keep, d_keep),
                 "support": lambda: support.model_loo_device(ctx, handle, d_keep),
                 "info": lambda: info.model_info_device(ctx, handle, d_theta, d_keep, d_status),
                 "fit": lambda: fit.model_fit_device(ctx, handle, d_theta, d_keep, d_status),
                 "table": lambda: context.context_table_device(ctx, handle),
                 "assignment": lambda: assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass),
                 "coverage": lambda: coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)}
        others = ["support", "info", "fit", "table", "assignment", "coverage"]
        orders = [tuple(others[:p] + ["diff"] + others[p:]) for p in range(7)] + [tuple(["diff"] + others[::-1])]
        turns = [(order, {k: calls[k]() for k in order}) for order in orders]
        del own
    first = turns[0][1]
    assert (first["diff"].diff_status == DU.OK).any() and (first["diff"].theta_a > 0).any()
    np.testing.assert_array_equal(first["diff"].delta_usage, 0.0)
    for order, got in turns[1:]:
        what = " -> ".join(order)
        bitwise(got["diff"], first["diff"], what)
        support_bitwise(got["support"], first["support"], what)
        IU.bitwise(got["info"], first["info"], what)
        FU.bitwise(got["fit"], first["fit"], what)
        assert_same_table(got["table"], first["table"], what)
        assert_same_assignment(got["assignment"], first["assignment"], np.asarray(annot.iso_off), hits_of, what)
        CU.compare(got["coverage"], first["coverage"], annot, hits.hit_locus, False, what)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)


SEVEN = ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters")


def seven(q):
    return {k: getattr(q, k).copy() for k in SEVEN}


def test_two_quantifiers_on_two_contexts(ctx):
    """Two resident quantifiers of one annotation (the same seed, sample_seed 31 and 32) on two contexts of device 0:
    differential_usage() is sbgpu_em_diff_device on the two retained batches bit for bit -- the batches are read from the
    call's own expanded sub-batch, whose A and B sub-problems are each sample's counts and kept weights; both objects' seven
    results are unchanged; every other stage still answers on both; a third object with the first's sample_seed gives the
    `same` picture."""
    from strawberry_amd import chain, em
    kw = dict(n_loci=400, n_frags=2e5, seed=31, resident=True, keep_bootstrap=True, min_isoform_frac=0.01)
    ctx_b, ctx_c = em.Context(0), em.Context(0)
    qa, qb, qc = chain.ChainQuantifier(ctx, sample_seed=31, **kw), chain.ChainQuantifier(ctx_b, sample_seed=32, **kw), None
    try:
        np.testing.assert_array_equal(qa.annot.iso_off, qb.annot.iso_off)
        assert qa.n_hits != qb.n_hits
        qa.step(), qb.step()
        before = seven(qa), seven(qb)
        t = qa.differential_usage(qb, with_sub_batch=True)
        ok = np.flatnonzero(t.diff_status == DU.OK)
        assert len(ok) > 50 and (t.lost_shift[ok] == 0).sum() > 25
        print("two chain samples", DU.census(t))
        # ---- the same through the batch entry, on the OK loci's sub-problems A and B (compacted to the kept columns)
        sh = t.sub
        loci = [[], []]
        for q, (l, k) in enumerate(zip(sh["sub_locus"], sh["sub_kind"])):
            if k < 2:
                rows, K = int(sh["row_off"][q + 1] - sh["row_off"][q]), int(sh["iso_off"][q + 1] - sh["iso_off"][q])
                loci[k].append((sh["count"][int(sh["row_off"][q]):int(sh["row_off"][q + 1])], sh["F"][int(sh["f_off"][q]):int(sh["f_off"][q + 1])].reshape(rows, K)))
        a, b = DU.batch_of(loci[0]), DU.batch_of(loci[1])
        # (sample B is the other context's record, not the first's read twice: other bins, other counts, another theta, and --
        # the two samples' expression shares are drawn independently -- most loci rejected, none of which `same` below shows)
        assert a.count.size != b.count.size and a.count.sum() != b.count.sum() and (t.theta_a[t.theta_a > 0].size and not np.array_equal(t.theta_a, t.theta_b))
        assert DU.census(t)["rejected"] > len(ok) // 2
        u = run(ctx_c, a, b, with_sub_batch=True)
        np.testing.assert_array_equal(u.sub["F"].view(np.uint64), sh["F"].view(np.uint64))
        per_locus = [k for k in diff.NAMES if k not in diff.PER_ISO and k != "top_iso"]
        for k in per_locus:
            x, y = getattr(t, k)[ok], getattr(u, k)
            np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y, err_msg=k)
        kept = np.concatenate([int(t.iso_off[l]) + np.array(DU.kept_columns(qa.annot, qa.keep, qb.keep, l), np.int64) for l in ok])
        for k in diff.PER_ISO:
            np.testing.assert_array_equal(getattr(t, k)[kept].view(np.uint64), getattr(u, k).view(np.uint64), err_msg=k)
        # ---- neither record changed; every other stage still answers on both, and the call again gives the same bits
        for q, was in zip((qa, qb), before):
            q.model_fit(), q.isoform_information(), q.isoform_support(), q.abundance_bootstrap(4, 3, replicates=False)
            for k in SEVEN:
                np.testing.assert_array_equal(getattr(q, k).view(np.uint8), was[k].view(np.uint8), err_msg=k)
        bitwise(qa.differential_usage(qb), t, "behind the other stages")
        back = qb.differential_usage(qa)
        np.testing.assert_array_equal(back.theta_a.view(np.uint64)[kept], t.theta_b.view(np.uint64)[kept])
        # ---- a third object with the first's sample_seed: the `same` picture
        qc = chain.ChainQuantifier(ctx_c, sample_seed=31, **kw)
        qc.step()
        same = qa.differential_usage(qc)
        np.testing.assert_array_equal(same.delta_usage, 0.0)
        sok = same.diff_status == DU.OK
        assert sok.sum() > 50 and (same.lr_stat[sok] > -1.0).all() and (same.lr_stat[sok] < 3.84).all() and (same.lost_shift[sok] == 0).all()
        # ---- refusals: a stale handle (qb quantifies again behind its handle's back), no retention, null arguments
        stale, qb.context_handle = qb.context_handle, None
        try:
            qb.step()
            with pytest.raises(_lib.SbgpuError, match="stale handle"):
                diff.model_diff_device(ctx, qa.context_handle, ctx_b, stale)
        finally:
            ctx_b.L.sbgpu_bins_destroy(stale)
        s = _lib.sbgpu_em_diff_t()
        L = ctx.L
        assert L.sbgpu_model_diff_device(ctx.h, qa.context_handle, None, qb.context_handle, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "sbgpu_model_diff_device: null argument" in L.sbgpu_last_error().decode()
        assert L.sbgpu_model_diff_device(ctx.h, qa.context_handle, ctx_b.h, qb.context_handle, None, None, None, None, None) == _lib.SBGPU_EINVAL
        par = _lib.sbgpu_diff_params_t(-1, 0)
        assert L.sbgpu_model_diff_device(ctx.h, qa.context_handle, ctx_b.h, qb.context_handle, None, None, C.byref(par), None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "max_bytes is negative" in L.sbgpu_last_error().decode()
        assert L.sbgpu_em_diff_device(ctx.h, None, None, None, None, None, None, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "sbgpu_em_diff_device: null argument" in L.sbgpu_last_error().decode()
        plain = chain.ChainQuantifier(ctx_c, n_loci=400, n_frags=2e5, seed=31, resident=True)
        h = C.c_void_p()
        try:
            plain.step()
            with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
                qa.differential_usage(plain)
            # the C entry's own check of a handle made without retention, on either side
            plain._resident_call(ctx_c.L, plain._ht, plain.hits.mass.data_ptr(), plain.hits.locus_hit_off.ctypes.data, plain.n_frags, h)
            for args in ((ctx, qa.context_handle, ctx_c, h), (ctx_c, h, ctx, qa.context_handle)):
                with pytest.raises(_lib.SbgpuError, match=r"sbgpu_model_diff_device: this handle was made without retention \(sbgpu_bootstrap_keep was off"):
                    diff.model_diff_device(*args)
        finally:
            if h:
                ctx_c.L.sbgpu_bins_destroy(h)
            plain.close()
    finally:
        for q in (qa, qb, qc):
            if q is not None:
                q.close()


def test_arrays_that_are_not_on_the_device_and_contexts_of_two_devices(ctx):
    import torch
    from strawberry_amd import em
    L = ctx.L
    s = em.EmBatchSolver(DU.batch_of([(np.ones(3, np.int64), np.ones((3, 2)))]), ctx)
    out = _lib.sbgpu_em_diff_t()
    cnt, F, plan = s.d_count.data_ptr(), s.d_F.data_ptr(), s.plan.h
    for args, why in (((plan, None, F, plan, cnt, F), "counts are not on the device"), ((plan, cnt, F, plan, None, F), "counts are not on the device"),
                      ((plan, cnt, None, plan, cnt, F), "weights are not on the device"), ((plan, cnt, F, plan, cnt, None), "weights are not on the device")):
        assert L.sbgpu_em_diff_device(ctx.h, *args, None, None, None, None, C.byref(out)) == _lib.SBGPU_EINVAL
        assert ("sbgpu_em_diff_device: the " + why) in L.sbgpu_last_error().decode()
    assert L.sbgpu_em_diff_device(ctx.h, plan, cnt, F, plan, cnt, F, None, None, None, None, C.byref(out)) == _lib.SBGPU_OK
    # contexts of two devices: where the machine has two, the call; where it has one, the refusal's text in the library
    text = "the two contexts are on different devices"
    if torch.cuda.device_count() > 1:
        from strawberry_amd import chain
        kw = dict(n_loci=50, n_frags=5e3, seed=3, resident=True, keep_bootstrap=True)
        other = em.Context(1)
        qa, qb = chain.ChainQuantifier(ctx, **kw), chain.ChainQuantifier(other, **kw)
        try:
            qa.step(), qb.step()
            with pytest.raises(_lib.SbgpuError, match=text):
                qa.differential_usage(qb)
        finally:
            qa.close(), qb.close()
    else:
        assert text.encode() in open(_lib.LIB_PATH, "rb").read()


def test_mismatched_annotations_are_refused(ctx):
    a = DU.batch_of([(np.ones(3, np.int64), np.ones((3, 2)))])
    b = DU.batch_of([(np.ones(3, np.int64), np.ones((3, 3)))])
    with pytest.raises(_lib.SbgpuError, match="iso_off"):
        run(ctx, a, b)
    two = DU.batch_of([(np.ones(3, np.int64), np.ones((3, 2)))] * 2)
    with pytest.raises(_lib.SbgpuError, match="n_loci"):
        run(ctx, a, two)


def test_front_quantifier_differential_usage(ctx):
    """FrontQuantifier.differential_usage() after step() and after stream_step(): the same records, the same bits"""
    from strawberry_amd import em, front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002, keep_bootstrap=True)
    ctx_b = em.Context(0)
    qa, qb = front.FrontQuantifier(ctx, sample_seed=23, **kw), front.FrontQuantifier(ctx_b, sample_seed=24, **kw)
    try:
        qa.step(), qb.step()
        f1 = qa.differential_usage(qb)
        assert (f1.diff_status == DU.OK).sum() > qa.n_loci // 4
        qa.to_host(qa.n_bytes // 6 + 4096, pinned=False)
        assert qa.stream_step()["chunks"] > 3
        bitwise(qa.differential_usage(qb), f1, "through the stream")
    finally:
        qa.close(), qb.close()
