"""The model fit built on the device (sbgpu_em_fit_device / sbgpu_model_fit_device, csrc/fit_device.h) against the host form
(sbgpu_em_fit_host under the same theta, keep and status) and tests/fit_util.py::by_hand, under the bounds at the head of
fit_util.py: on the five EM goldens (em_edge without its one locus beyond the device form's limits, which is refused), under the
EM's theta and under a bootstrap mean; on tests/retained_util.py::edge_sample() through a resident call; on a locus on either
side of every threshold the library exports; past two passes of both kernels' grids; the exact parts bit for bit; two calls bit
for bit; all 24 orders with the table, the assignment and the coverage; through the front quantifier; the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fit_util as FU
import retained_util as R
from strawberry_amd import _lib, assign, context, coverage, fit

pytestmark = pytest.mark.gpu

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
SHARES = {}


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def note(label, share):
    SHARES[label] = share
    print(label, "worst share of each bound:", {k: round(v, 4) for k, v in share.items()})


def within_limits(b):
    lim = fit.limits()
    return np.nonzero((np.diff(b.row_off) <= lim["max_bins"]) & (np.diff(b.iso_off) <= lim["max_iso"]))[0]


def threads_of(b):
    """threads of the group that serves each locus: a wave, or a workgroup"""
    lim = fit.limits()
    rows, niso = np.diff(b.row_off), np.diff(b.iso_off)
    wave = (rows <= lim["wave_vals"]) & (niso <= lim["wave_vals"]) & (rows * niso <= lim["wave_vals"])
    return np.where(wave, lim["wave"], lim["threads"])


def exact_parts(t, b, possible, label):
    """worst_bin is the argmax of the device's own resid; pearson the documented tree over the device's own resid, bit for bit"""
    np.testing.assert_array_equal(t.worst_bin, FU.worst_bin_of(t.resid, possible, b.row_off), err_msg=label)
    T = threads_of(b)
    want = np.array([FU.tree_sum(t.resid[int(b.row_off[l]):int(b.row_off[l + 1])] ** 2, int(T[l])) for l in range(len(T))])
    np.testing.assert_array_equal(t.pearson.view(np.uint64), want.view(np.uint64), err_msg=label + " pearson")


@pytest.fixture(scope="module")
def G(ctx, golden):
    """name -> the golden (within the limits), solved on the device, with the fit under the EM's theta (twice) and under a
    bootstrap mean, the host forms of both, and by_hand under the EM's theta"""
    from strawberry_amd import em
    out = {}
    for name in GOLDENS:
        full, _, _ = golden(name)
        idx = within_limits(full)
        b = full if len(idx) == full.n_loci else FU.select_loci(full, idx)
        s = em.EmBatchSolver(b, ctx)
        s.run_em()
        r = s.results()
        t, again = s.run_fit(), s.run_fit()
        mean = s.run_bootstrap(8, 5)["mean"]
        s.synchronize()
        t_mean = s.run_fit(d_theta=mean.contiguous())
        mean = mean.cpu().numpy()
        out[name] = dict(b=b, full=full, r=r, t=t, again=again, t_mean=t_mean, mean=mean, few=s.run_fit(want=("score", "worst_bin")),
                         host=fit.em_fit_host(b, r["theta"], status=r["status"]), host_mean=fit.em_fit_host(b, mean, status=r["status"]),
                         want=FU.by_hand(b, r["theta"], None, r["status"]), want_mean=FU.by_hand(b, mean, None, r["status"]))
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_device_against_host_and_by_hand_on_the_goldens(G, name):
    g = G[name]
    b = g["b"]
    note(name + ", device against host", FU.compare(g["t"], g["host"], b, False, name, exact_from=g["want"]))
    note(name + ", device against by_hand", FU.compare(g["t"], g["want"], b, True, name))
    note(name + ", a bootstrap mean, device against host", FU.compare(g["t_mean"], g["host_mean"], b, False, name + " mean", exact_from=g["want_mean"]))
    note(name + ", a bootstrap mean, device against by_hand", FU.compare(g["t_mean"], g["want_mean"], b, True, name + " mean"))
    assert (g["mean"] != g["r"]["theta"]).any()
    # d_b and the score's sum run in the host form's order: the score is the host form's, bit for bit
    np.testing.assert_array_equal(g["t"].score.view(np.uint64), g["host"].score.view(np.uint64))
    exact_parts(g["t"], b, g["want"]["possible"], name)
    exact_parts(g["t_mean"], b, g["want_mean"]["possible"], name + " mean")
    few = g["few"]
    assert few.expected is None and few.pearson is None and set(few.device) == set(fit.NAMES)
    np.testing.assert_array_equal(few.score, g["t"].score)
    np.testing.assert_array_equal(few.worst_bin, g["t"].worst_bin)
    ruled = (g["r"]["status"] == 0) & (g["r"]["iters"] >= 2)
    norm = g["t"].step_norm(g["r"]["theta"])
    print(name, "step norm of the stopped loci up to %.4e; of the capped ones up to %.3e"
          % (norm[ruled].max(), norm[g["r"]["status"] == 3].max() if (g["r"]["status"] == 3).any() else 0.0))


@pytest.mark.parametrize("name", GOLDENS)
def test_two_calls_are_bitwise_equal(G, name):
    FU.bitwise(G[name]["t"], G[name]["again"], name)


def test_a_locus_beyond_the_limits_is_refused(ctx, G):
    from strawberry_amd import em
    full = G["em_edge"]["full"]
    assert full.n_loci == G["em_edge"]["b"].n_loci + 1 and np.diff(full.row_off).max() > fit.limits()["max_bins"]
    s = em.EmBatchSolver(full, ctx)
    with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*a locus of more than 5632 bins"):
        s.run_fit()


def test_the_device_log_is_within_the_ulps_the_bounds_assume(ctx, G):
    """K of the bounds holds the distance between the device's log and the host's over the arguments these tests use: d_b / D
    and n_b / expected[b] of every possible bin with a count, on the five goldens (a property of the math library)."""
    import torch
    worst = 0.0
    for name in GOLDENS:
        g = G[name]
        b, t = g["b"], g["host"]
        _, _, bin_locus, _ = FU.shapes(b)
        M = (t.n_live - t.n_impossible).astype(np.float64)[bin_locus]
        use = (t.expected > 0.0) & (np.asarray(b.count) > 0)
        args = np.concatenate([t.expected[use] / M[use], np.asarray(b.count, np.float64)[use] / t.expected[use]])
        dev = torch.log(torch.from_numpy(args).to(torch.device("cuda", ctx.device))).cpu().numpy()
        host = np.log(args)
        zero = host == 0.0             # (log(1.0): both give exactly 0.0, which has no ulp to count in)
        np.testing.assert_array_equal(dev[zero], host[zero])
        assert np.isfinite(dev).all() and np.isfinite(host).all() and (~zero).sum() > 100
        worst = max(worst, float((np.abs(dev[~zero] - host[~zero]) / np.spacing(np.abs(host[~zero]))).max()))
    print("largest distance between the device's and the host's log: %.2f ulp over the goldens' arguments" % worst)
    assert worst <= FU.LOG_ULP_DEVICE


def shaped(rng, rows, niso, density=0.5, empty=False):
    F = rng.uniform(1e-3, 0.3, (rows, niso)) * (rng.random((rows, niso)) < density)
    F[rng.integers(0, rows), :] = rng.uniform(1e-3, 0.3, niso)        # one row that carries every isoform
    if rows > 2:
        F[1, :] = 1e-6                                                  # a dropped row
    if empty:
        F[:] = 1e-7
    return rng.integers(0, 60, rows).astype(np.int32), F


THRESHOLD_SHAPES = {"1x1": (1, 1), "wave, one row": (1, 512), "block, one row": (2, 512), "wave, one isoform": (512, 1),
                    "block, one isoform": (513, 1), "wave, full": (16, 32), "block, just": (16, 33), "staged, full": (32, 64),
                    "global, just": (32, 65), "tall": (5632, 2), "wide": (40, 512), "before": (7, 3), "never started": (6, 3), "after": (9, 4)}


@pytest.fixture(scope="module")
def T(ctx):
    """One locus on either side of every threshold, under a made-up theta and filter (the fit takes any), with a locus that never
    started between two ordinary ones"""
    import torch
    from strawberry_amd import em
    rng = np.random.default_rng(22)
    b = FU.from_loci([shaped(rng, *shape, empty=name == "never started") for name, shape in THRESHOLD_SHAPES.items()])
    n_iso = int(b.iso_off[-1])
    theta = rng.uniform(0.5, 40.0, n_iso)
    keep = (rng.random(n_iso) < 0.9).astype(np.int32)
    keep[np.asarray(b.iso_off[:-1])] = 1
    status = np.zeros(b.n_loci, np.int32)
    status[list(THRESHOLD_SHAPES).index("never started")] = _lib.EM_INIT_EMPTY
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, theta, keep, status)]
    t = fit.em_fit_device(ctx, plan, *d)
    again = fit.em_fit_device(ctx, plan, *d)
    all_kept = fit.em_fit_device(ctx, plan, d[0], d[1], d[2])
    plan.close()
    return dict(b=b, theta=theta, keep=keep, status=status, t=t, again=again, all_kept=all_kept, host=fit.em_fit_host(b, theta, keep, status),
                host_all=fit.em_fit_host(b, theta), want=FU.by_hand(b, theta, keep, status), want_all=FU.by_hand(b, theta))


def test_a_locus_on_either_side_of_every_threshold(T):
    lim = fit.limits()
    b = T["b"]
    shapes = dict(zip(THRESHOLD_SHAPES, zip(np.diff(b.row_off), np.diff(b.iso_off))))
    T_of = dict(zip(THRESHOLD_SHAPES, threads_of(b)))
    # by the library's constants: the wave form ends at wave_vals weights, bins or isoforms; LDS staging at stage_vals
    for name in ("1x1", "wave, one row", "wave, one isoform", "wave, full", "before", "never started", "after"):
        assert T_of[name] == lim["wave"], name
    for name in ("block, one row", "block, one isoform", "block, just", "staged, full", "global, just", "tall", "wide"):
        assert T_of[name] == lim["threads"], name
    assert shapes["wave, one row"] == (1, lim["wave_vals"]) and shapes["wave, one isoform"] == (lim["wave_vals"], 1)
    assert shapes["wave, full"][0] * shapes["wave, full"][1] == lim["wave_vals"] < shapes["block, just"][0] * shapes["block, just"][1]
    assert shapes["staged, full"][0] * shapes["staged, full"][1] == lim["stage_vals"] < shapes["global, just"][0] * shapes["global, just"][1]
    assert shapes["tall"][0] == lim["max_bins"]
    note("thresholds, device against host", FU.compare(T["t"], T["host"], b, False, "thresholds", exact_from=T["want"]))
    note("thresholds, device against by_hand", FU.compare(T["t"], T["want"], b, True, "thresholds"))
    note("thresholds, everything kept, device against host", FU.compare(T["all_kept"], T["host_all"], b, False, "thresholds", exact_from=T["want_all"]))
    FU.compare(T["all_kept"], T["want_all"], b, True, "thresholds, everything kept")
    np.testing.assert_array_equal(T["t"].score.view(np.uint64), T["host"].score.view(np.uint64))
    exact_parts(T["t"], b, T["want"]["possible"], "thresholds")
    FU.bitwise(T["t"], T["again"], "thresholds")
    l = list(THRESHOLD_SHAPES).index("never started")
    t = T["t"]
    assert t.n_dropped[l] == b.count[int(b.row_off[l]):int(b.row_off[l + 1])].sum() and t.n_live[l] == 0 and t.dof[l] == 0 and t.worst_bin[l] == -1
    assert t.n_live[l - 1] > 0 and t.n_live[l + 1] > 0 and t.n_dropped.sum() > t.n_dropped[l] and (T["keep"] == 0).any()
    assert (t.n_impossible > 0).any() or (T["want"]["n_impossible"] == 0).all()


def test_more_loci_than_two_passes_of_either_grid(ctx, golden):
    """em_c3_400's loci repeated until the wave form's list and the workgroup form's both exceed two passes of their grids;
    by_hand is computed on the base and repeated."""
    import torch
    from strawberry_amd import em
    lim = fit.limits()
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    cap = lim["grid_per_cu"] * cu
    full, _, _ = golden("em_c3_400")
    large = np.nonzero(threads_of(full) == lim["threads"])[0]
    small = np.nonzero(threads_of(full) == lim["wave"])[0][:4 * lim["wave_loci"] * len(large)]
    base = FU.select_loci(full, np.sort(np.concatenate([large, small])))
    reps = 2 * cap // len(large) + 1
    b = FU.tile_batch(base, reps)
    n_large = int((threads_of(b) == lim["threads"]).sum())
    assert n_large > 2 * cap and b.n_loci - n_large > 2 * cap * lim["wave_loci"], (b.n_loci, n_large, cap)
    s0 = em.EmBatchSolver(base, ctx)
    s0.run_em()
    r0 = s0.results()
    theta, status = np.tile(r0["theta"], reps), np.tile(r0["status"], reps)
    want0 = FU.by_hand(base, r0["theta"], None, r0["status"])
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, theta, status)]
    t = fit.em_fit_device(ctx, plan, d[0], d[1], d[2], None, d[3])
    plan.close()
    host = fit.em_fit_host(b, theta, status=status)
    want = {k: np.tile(v, reps) for k, v in want0.items()}
    note("%d loci, device against host" % b.n_loci, FU.compare(t, host, b, False, "past two passes", exact_from=want))
    note("%d loci, device against by_hand" % b.n_loci, FU.compare(t, want, b, True, "past two passes"))
    first = fit.em_fit_host(base, r0["theta"], status=r0["status"])
    for k in fit.NAMES:     # every repeat of a locus gets the first one's bits
        x = getattr(t, k)
        np.testing.assert_array_equal(x.reshape(reps, -1), np.tile(x[:x.size // reps], (reps, 1)), err_msg=k)
    np.testing.assert_array_equal(t.n_live[:base.n_loci], first.n_live)


@pytest.fixture(scope="module")
def E(ctx):
    """One resident call on the edge sample with the fit behind it; on its handle a bootstrap, and the fit under the bootstrap's
    mean of theta; the same call's weights through sbgpu_quantify_host"""
    import torch
    from strawberry_amd import bootstrap
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small, grid = R.n_small_for(cu), R.GRID_PER_CU * cu
    annot, hits = R.edge_sample(n_small, grid=grid)
    law = InsertSize(*R.LAW)
    dev = torch.device("cuda", ctx.device)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_fit=True, keep_handle=True)
    with r["handle"] as handle:
        boot = bootstrap.abundance_bootstrap_device(ctx, handle, 4, 9, replicates=False)
        mean = np.ascontiguousarray(boot["theta_mean"])
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (mean, r["keep"], r["status"])]
        t_mean = fit.model_fit_device(ctx, handle, *d)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    return dict(r=r, h=h, at=R.edge_layout(n_small), annot=annot, mean=mean, t_mean=t_mean)


def test_the_edge_sample_through_a_resident_call(E):
    import types
    r, h = E["r"], E["h"]
    bins = h["bins"]
    batch = types.SimpleNamespace(row_off=bins.row_off, iso_off=bins.iso_off, f_off=bins.f_off, count=bins.count, F=h["F"], n_loci=len(bins.row_off) - 1)
    t = r["fit"]
    np.testing.assert_array_equal(t.row_off, bins.row_off)
    for what, t, theta in (("edge sample", r["fit"], r["theta"]), ("edge sample, a bootstrap mean", E["t_mean"], E["mean"])):
        host = fit.em_fit_host(batch, theta, r["keep"], r["status"])
        want = FU.by_hand(batch, theta, r["keep"], r["status"])
        note(what + ", device against host", FU.compare(t, host, batch, False, what, exact_from=want))
        note(what + ", device against by_hand", FU.compare(t, want, batch, True, what))
        np.testing.assert_array_equal(t.score.view(np.uint64), host.score.view(np.uint64))
        exact_parts(t, batch, want["possible"], what)
    t = r["fit"]
    assert (E["mean"] != r["theta"]).sum() > r["theta"].size // 2 and (E["t_mean"].expected != t.expected).any()
    at = E["at"]
    assert t.n_live[at["C"]] > 0 and t.dof[at["C"]] > 0 and t.n_live[at["EMPTY"]] == 0 and t.worst_bin[at["NOBIN"]] == -1
    assert (r["keep"] == 0).any() and t.n_dropped.sum() > 0 and (threads_of(batch) == fit.limits()["threads"]).sum() >= 4


def test_all_24_orders_of_fit_table_assignment_and_coverage(ctx):
    """Each order twice, on a toy directory: every result is the first turn's, and the resident call's seven outputs are the
    bits of the same call with nothing behind it."""
    import torch
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
        calls = {"fit": lambda: fit.model_fit_device(ctx, handle, d_theta, d_keep, d_status),
                 "table": lambda: context.context_table_device(ctx, handle),
                 "assignment": lambda: assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass),
                 "coverage": lambda: coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)}
        turns = [(order, {k: calls[k]() for k in order}) for order in itertools.permutations(sorted(calls)) for _ in range(2)]
        del own
    assert len(turns) == 48 and len({o for o, _ in turns}) == 24
    first = turns[0][1]
    assert first["fit"].n_live.sum() > 0 and (first["fit"].score > 0).any()
    for order, got in turns[1:]:
        what = " -> ".join(order)
        FU.bitwise(got["fit"], first["fit"], what)
        assert_same_table(got["table"], first["table"], what)
        assert_same_assignment(got["assignment"], first["assignment"], np.asarray(annot.iso_off), hits_of, what)
        CU.compare(got["coverage"], first["coverage"], annot, hits.hit_locus, False, what)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    with_fit = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, with_fit=True, **kw)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(with_fit[k]), bits(plain[k]), err_msg=k)
    FU.bitwise(with_fit["fit"], first["fit"], "quantify_resident(with_fit=True)")


def test_front_quantifier_model_fit(ctx):
    """FrontQuantifier.model_fit() after step() and after stream_step(): the same records, the same fit"""
    from strawberry_amd import front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
            plain.model_fit()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_bootstrap=True, **kw)
    try:
        q.step()
        theta = q.theta[:q.n_iso].copy()
        f1 = q.model_fit()
        q.abundance_bootstrap(4, 3, replicates=False)
        f2 = q.model_fit()
        FU.bitwise(f2, f1, "behind a bootstrap")
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        info = q.stream_step()
        assert info["chunks"] > 3
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        f3 = q.model_fit()
        FU.bitwise(f3, f1, "through the stream")
        assert f1.n_live.sum() > 0 and (f1.dof > 0).sum() > q.n_loci // 4 and set(f1.device) == set(fit.NAMES)
        norm = f1.step_norm(theta)
        # the stopping rule shows where the fit's model is the EM's: no isoform of the locus erased by the expression filter
        erased = np.add.reduceat(np.concatenate([q.keep[:q.n_iso] == 0, [0]]).astype(np.int64), q.annot.iso_off[:-1]) > 0
        ruled = (q.status[:q.n_loci] == 0) & (q.iters[:q.n_loci] >= 2) & ~erased
        assert ruled.sum() > q.n_loci // 4 and (norm[ruled] < FU.THETA_CHANGE_LIMIT * (1 + 1e-6)).all()
    finally:
        q.close()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, a null theta, null arguments."""
    from strawberry_amd import bootstrap, chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_fit(h, d_theta=True, out=True):
        s = _lib.sbgpu_em_fit_t()
        rc = L.sbgpu_model_fit_device(ctx.h, h, q._out.d_theta if d_theta else None, None, None, None, C.byref(s) if out else None)
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_fit(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention (sbgpu_bootstrap_keep was off" in why, why
        bootstrap.bootstrap_keep(ctx, True)
        h1 = call()
        rc, why = try_fit(h1, d_theta=False)
        assert rc == _lib.SBGPU_EINVAL and "d_theta is needed" in why, why
        rc, why = try_fit(h1, out=False)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        f1 = fit.model_fit_device(ctx, h1, int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status))
        h2 = call()
        rc, why = try_fit(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        f2 = fit.model_fit_device(ctx, h2, int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status))
        FU.bitwise(f2, f1, "the same call twice")
        s = _lib.sbgpu_em_fit_t()
        assert L.sbgpu_em_fit_device(ctx.h, None, None, None, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "null argument" in L.sbgpu_last_error().decode()
    finally:
        bootstrap.bootstrap_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()


def test_report_the_worst_share_of_each_bound():
    """(last in the file) what DESIGN 3.22 quotes: the largest share of each bound over every comparison above"""
    assert SHARES, "the comparisons above did not run"
    worst = {}
    for label, share in SHARES.items():
        for k, v in share.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, label)
    print("worst share of each bound on this device:", {k: (round(v, 4), where) for k, (v, where) in worst.items()})
    assert all(v <= 1.0 for v, _ in worst.values())
