"""The variational Bayes solve on the device (sbgpu_em_vb_device / sbgpu_model_vb_device, csrc/vb_device.h) against the host form
(sbgpu_em_vb_host) and tests/vb_util.py's restatement, under the bounds at the head of vb_util.py: on the five EM goldens at alpha
= 0.01 and 1 (em_edge without its one locus beyond the limits, which is refused); two calls bit for bit; a locus on either side of
every threshold the library exports and at the extreme shapes; past two passes of both kernels' grids; a fast and a slow locus in
one workgroup, each bitwise itself solved alone; max_iter = 3; the edge cases; the device library's log / exp / lgamma in ulps;
after tests/retained_util.py::edge_sample() through a resident call; in every order with the fit and the support; through the
front quantifier; abundance() against the oracle's epilogue; the refusals."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import vb_util as V
from strawberry_amd import _lib, vb

pytestmark = pytest.mark.gpu

DEV_COUNT, DEV_ELBO = V.DEVICE_FACTOR * V.HOST_COUNT_GAP, V.DEVICE_FACTOR * V.HOST_ELBO_GAP
# against the restatement: the device's distance from the host form and the host form's from the restatement
RES_COUNT, RES_ELBO = DEV_COUNT + V.HOST_COUNT_GAP, DEV_ELBO + V.HOST_ELBO_GAP
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def note(label, worst):
    WORST[label] = worst
    print(label, {k: float("%.3g" % v) for k, v in worst.items()})


def device_solve(ctx, b, **kw):
    """-> a VariationalFit for batch b through sbgpu_em_vb_device, with arrays of its own"""
    import torch
    from strawberry_amd import em
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d_count, d_F = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (np.asarray(b.count, np.int32), np.asarray(b.F, np.float64)))
    t = vb.em_vb_device(ctx, plan, d_count, d_F, **kw)
    plan.close()
    return t


@pytest.fixture(scope="module")
def G(ctx, golden):
    """(golden, alpha) -> the batch, the device's solve (twice), the host form's and the restatement's"""
    from strawberry_amd import em
    out = {}
    for name in V.GOLDENS:
        b = V.golden_within_limits(golden, name)
        s = em.EmBatchSolver(b, ctx)
        for alpha in V.ALPHAS:
            out[(name, alpha)] = dict(b=b, t=s.run_vb(alpha=alpha), again=s.run_vb(alpha=alpha), host=vb.em_vb_host(b, alpha=alpha),
                                      want=V.solve(b, alpha=alpha))
        out[name] = dict(few=s.run_vb(want=("count", "n_frag")), default=s.run_vb())
    return out


@pytest.mark.parametrize("alpha", V.ALPHAS)
@pytest.mark.parametrize("name", V.GOLDENS)
def test_device_against_host_and_restatement_on_the_goldens(G, name, alpha):
    g = G[(name, alpha)]
    b, label = g["b"], "%s, alpha %g" % (name, alpha)
    note(label + ", device against host", V.compare(g["t"], g["host"], b.iso_off, DEV_COUNT, DEV_ELBO, label=label))
    note(label + ", device against restatement", V.compare(g["t"], g["want"], b.iso_off, RES_COUNT, RES_ELBO, label=label))
    assert set(g["t"].device) == set(vb.NAMES) and (g["t"].iters > 10).any()
    if alpha == 0.01:
        few = G[name]["few"]
        assert few.share is None and few.elbo is None and set(few.device) == set(vb.NAMES)
        np.testing.assert_array_equal(few.count, g["t"].count)
        V.bitwise(G[name]["default"], g["t"], label + ": NULL params")


@pytest.mark.parametrize("alpha", V.ALPHAS)
@pytest.mark.parametrize("name", V.GOLDENS)
def test_two_calls_are_bitwise_equal(G, name, alpha):
    V.bitwise(G[(name, alpha)]["t"], G[(name, alpha)]["again"], name)


def test_a_locus_on_either_side_of_every_threshold(ctx):
    lim = vb.limits()
    b, names = V.threshold_sample()
    form = dict(zip(names, V.form_of(b, lim)))
    shape = dict(zip(names, zip(np.diff(b.row_off), np.diff(b.iso_off))))
    assert [form[k] for k in ("wave, full", "block, just", "staged, full", "global, just", "staged, one isoform", "global, one isoform")] == [0, 1, 1, 2, 1, 2]
    assert [form[k] for k in ("1x1", "wave, one row", "block, two rows", "wave, one isoform", "block, one isoform", "tall", "wide")] == [0, 0, 1, 0, 1, 2, 2]
    assert shape["wave, full"][0] * shape["wave, full"][1] == lim["wave_vals"] and shape["tall"] == (lim["max_bins"], 2)
    assert shape["wide"][1] == lim["max_iso"] and shape["block, two rows"] == (2, lim["max_iso"])
    r, k = shape["staged, full"]
    assert r * k + r + 2 * k == lim["stage_doubles"]
    at = dict(zip(names, range(len(names))))
    for alpha in V.ALPHAS:
        t, again, host = device_solve(ctx, b, alpha=alpha), device_solve(ctx, b, alpha=alpha), vb.em_vb_host(b, alpha=alpha)
        note("thresholds, alpha %g, device against host" % alpha, V.compare(t, host, b.iso_off, DEV_COUNT, DEV_ELBO, label="thresholds"))
        V.bitwise(t, again, "thresholds")
        assert t.status[at["init empty"]] == V.INIT_EMPTY and t.iters[at["init empty"]] == 0 and t.n_active[at["init empty"]] == 0
        assert t.status[at["no fragments"]] == V.OK and t.iters[at["no fragments"]] == 1 and t.elbo[at["no fragments"]] == 0.0
        i0 = int(b.iso_off[at["inactive columns"]])
        assert t.n_active[at["inactive columns"]] == 2 and (t.count[i0:i0 + 4] > 0).tolist() == [True, False, True, False]
        assert (t.status == V.MAXITER).any() or alpha == 1.0


def test_one_bin_or_one_isoform_beyond_the_limits_is_refused(ctx, golden):
    rng = np.random.default_rng(3)
    # (513 isoforms: the plan such a batch needs is refused already, with the same code)
    for extra, text in (((V.MAX_BINS + 1, 1), "sbgpu_em_vb_device.*a locus of more than 5632 bins"), ((1, V.MAX_ISO + 1), "more than 512 isoforms")):
        with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*" + text):
            device_solve(ctx, V.from_loci([V.fast_locus(), V.shaped(rng, *extra)]))
    full, _, _ = golden("em_edge")
    assert np.diff(full.row_off).max() > V.MAX_BINS
    with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*more than 5632 bins"):
        device_solve(ctx, full)
    b = V.from_loci([V.shaped(rng, V.MAX_BINS, 1), V.shaped(rng, 1, V.MAX_ISO)])
    V.compare(device_solve(ctx, b), vb.em_vb_host(b), b.iso_off, DEV_COUNT, DEV_ELBO, label="at the limits")


def test_more_tiny_loci_than_two_passes_of_either_grid(ctx):
    import torch
    lim = vb.limits()
    cap = lim["grid_per_cu"] * torch.cuda.get_device_properties(ctx.device).multi_processor_count
    base = V.many_tiny()
    n_block = int((V.form_of(base, lim) == 1).sum())
    reps = 2 * cap // n_block + 1
    b = V.tile_batch(base, reps)
    form = V.form_of(b, lim)
    assert (form == 1).sum() > 2 * cap and (form == 0).sum() > 2 * cap * lim["wave_loci"], (b.n_loci, cap)
    t, first = device_solve(ctx, b), vb.em_vb_host(base)
    want = {k: np.tile(getattr(first, k), reps) for k in vb.NAMES}
    note("%d loci, device against host" % b.n_loci, V.compare(t, want, b.iso_off, DEV_COUNT, DEV_ELBO, label="past two passes"))
    for k in vb.NAMES:      # every repeat of a locus gets the first one's bits
        x = getattr(t, k)
        np.testing.assert_array_equal(x.reshape(reps, -1), np.tile(x[:x.size // reps], (reps, 1)), err_msg=k)


def test_a_locus_is_solved_the_same_wherever_it_stands(ctx):
    """A 2-iteration locus and one of several hundred iterations share a workgroup of the wave form (neighbours in the list): the
    fast one is masked while the slow one runs, and each is bitwise itself solved alone"""
    fast, slow = V.fast_locus(), V.slow_locus(np.random.default_rng(31))
    alone = [device_solve(ctx, V.from_loci([x])) for x in (fast, slow)]
    assert alone[0].iters[0] == 2 and 300 <= alone[1].iters[0] < V.MAX_ITER and V.form_of(V.from_loci([fast, slow]), vb.limits()).tolist() == [0, 0]
    for order in ((0, 1), (1, 0), (0, 1, 0, 1, 1, 0, 0)):
        t = device_solve(ctx, V.from_loci([(fast, slow)[k] for k in order]))
        i = 0
        for l, k in enumerate(order):
            n = alone[k].n_iso
            for name in vb.NAMES:
                x, y = getattr(t, name), getattr(alone[k], name)
                x = x[i:i + n] if name in vb.PER_ISO else x[l:l + 1]
                np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y,
                                              err_msg="%s, locus %d of %s" % (name, l, order))
            i += n


def test_max_iter_three(ctx):
    b = V.many_tiny()
    t, host, want = device_solve(ctx, b, max_iter=3), vb.em_vb_host(b, max_iter=3), V.solve(b, max_iter=3)
    np.testing.assert_array_equal(t.iters, host.iters)
    np.testing.assert_array_equal(t.iters, want["iters"])
    np.testing.assert_array_equal(t.status, want["status"])
    assert (t.status == V.MAXITER).sum() > 4 and (t.iters[t.status == V.MAXITER] == 3).all() and (t.status == V.OK).any()
    V.compare(t, host, b.iso_off, DEV_COUNT, DEV_ELBO, label="max_iter 3", exact_iters=True)
    one = device_solve(ctx, b, max_iter=1)
    np.testing.assert_array_equal(one.iters, np.minimum(host.iters, 1))      # (a locus without a live bin starts none)
    assert (one.status[host.iters > 1] == V.MAXITER).all() and (one.iters == 1).sum() >= b.n_loci - 2


def test_the_edge_cases(ctx):
    """a zero-count bin private to an isoform that dies: no NaN; a counted bin whose isoforms all underflow: DENOM_ZERO, in the
    wave form and in the workgroup form"""
    for pad in (0, 300):       # pad: fragment-less bins without weight that push the locus into the workgroup form
        n, F = V.dying_private_bin()
        n, F = list(n) + [0] * pad, np.concatenate([np.asarray(F), np.zeros((pad, 2))])
        b = V.from_loci([V.fast_locus(), (n, F), V.fast_locus()])
        t, host = device_solve(ctx, b, **V.DYING_PARAMS), vb.em_vb_host(b, **V.DYING_PARAMS)
        V.compare(t, host, b.iso_off, DEV_COUNT, DEV_ELBO, change_limit=V.DYING_PARAMS["change_limit"], label="dying")
        assert t.status[1] == V.OK and t.count[3] == 0.0 and abs(t.count[2] - 100003.0) < 1e-6 and np.isfinite(t.elbo[1]) and t.share[3] > 0.0
        assert not np.isnan(np.concatenate([t.count, t.share, t.share_sd, t.elbo])).any()
        assert V.form_of(b, vb.limits())[1] == (1 if pad else 0)
    for k in (100, 400):       # 303 weights: a wave; 1203: a workgroup
        b = V.from_loci([V.fast_locus(), V.underflowing_bin(k), V.fast_locus()])
        t, host = device_solve(ctx, b, **V.UNDERFLOW_PARAMS), vb.em_vb_host(b, **V.UNDERFLOW_PARAMS)
        assert host.status[1] == V.DENOM_ZERO and host.iters[1] == 2 and V.form_of(b, vb.limits())[1] == (0 if k == 100 else 1)
        V.compare(t, host, b.iso_off, DEV_COUNT, DEV_ELBO, label="underflow", exact_iters=True)
        assert t.status.tolist() == [V.OK, V.DENOM_ZERO, V.OK] and t.elbo[1] == -math.inf and t.n_active[1] == k + 1 and t.iters.tolist() == [2, 2, 2]
        np.testing.assert_allclose(t.count[2:2 + k], 1.0 / k, rtol=1e-12)


def test_the_device_library_in_ulps(ctx, G):
    """What the factor of 100 allows for: the distance between the device's and the host's log, exp and lgamma over arguments of
    the kind the solve uses (a property of the math libraries; reported for DESIGN 3.31)"""
    import torch
    dev = torch.device("cuda", ctx.device)
    host = G[("em_c3_400", 0.01)]["host"]
    a = 0.01 + host.count[host.count > 0]
    args = {"log": np.concatenate([a + 10.0, np.logspace(-12, 0, 2000)]), "exp": -np.logspace(-3, 2.8, 4000), "lgamma": np.concatenate([a, [0.01, 1.0, 5.12]])}
    fn = {"log": (torch.log, np.log), "exp": (torch.exp, np.exp), "lgamma": (torch.lgamma, lambda x: np.array([math.lgamma(v) for v in x]))}
    for k, x in args.items():
        d, h = fn[k][0](torch.from_numpy(x).to(dev)).cpu().numpy(), fn[k][1](x)
        use = h != 0.0
        ulp = np.abs(d[use] - h[use]) / np.spacing(np.abs(h[use]))
        print("largest distance between the device's and the host's %s: %.2f ulp over %d arguments" % (k, ulp.max(), use.sum()))
        assert np.isfinite(d).all() and ulp.max() < V.DEVICE_FACTOR


@pytest.fixture(scope="module")
def E(ctx):
    """One resident call on the edge sample with the variational solve behind it, the same call plain, and its weights through
    sbgpu_quantify_host"""
    import torch
    import retained_util as R
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small = R.n_small_for(cu)
    annot, hits = R.edge_sample(n_small, grid=R.GRID_PER_CU * cu)
    law = InsertSize(*R.LAW)
    kw = dict(ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    plain = quantify_resident(annot, hits, law, R.RL, hits.n_hits, **kw)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, with_variational=True, **kw)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    return dict(r=r, plain=plain, h=h, at=R.edge_layout(n_small), annot=annot, hits=hits)


def test_the_edge_sample_through_a_resident_call(ctx, E, oracle):
    import types
    import stream_util as S
    from test_fragment_assign_gpu import bits
    r, h, at = E["r"], E["h"], E["at"]
    for k in S.OUT_KEYS:        # the call's seven results, bit for bit
        np.testing.assert_array_equal(bits(r[k]), bits(E["plain"][k]), err_msg=k)
    bins = h["bins"]
    b = types.SimpleNamespace(row_off=bins.row_off, iso_off=bins.iso_off, f_off=bins.f_off, count=bins.count, F=h["F"], n_loci=len(bins.row_off) - 1)
    t = r["variational"]
    np.testing.assert_array_equal(t.iso_off, bins.iso_off)
    V.bitwise(t, device_solve(ctx, b), "sbgpu_model_vb_device against sbgpu_em_vb_device on the exported bins")
    host = vb.em_vb_host(b)
    note("edge sample, device against host", V.compare(t, host, b.iso_off, DEV_COUNT, DEV_ELBO, label="edge sample"))
    # the restatement on the loci that are not small and on every 40th of the others
    some = np.unique(np.concatenate([np.array(sorted(at.values())), np.arange(0, b.n_loci, 40)]))
    sub = V.select_loci(types.SimpleNamespace(row_off=b.row_off, iso_off=b.iso_off, f_off=b.f_off, count=b.count, F=b.F, length=np.zeros(int(b.iso_off[-1]), np.int32)), some)
    pick = lambda x, off: np.concatenate([x[int(off[l]):int(off[l + 1])] for l in some])   # noqa: E731
    got = {k: pick(getattr(t, k), b.iso_off) if k in vb.PER_ISO else getattr(t, k)[some] for k in vb.NAMES}
    note("edge sample, device against restatement", V.compare(got, V.solve(sub), sub.iso_off, RES_COUNT, RES_ELBO, label="edge sample"))
    assert t.status[at["EMPTY"]] == V.INIT_EMPTY and t.status[at["NOBIN"]] == V.INIT_EMPTY and t.n_frag[at["C"]] > 0 and t.n_active[at["C"]] > 64
    assert (V.form_of(b, vb.limits()) == 2).any() and (V.form_of(b, vb.limits()) == 1).sum() >= 4
    # abundance(): the oracle's epilogue on the device's own count, and on the restatement's
    ab, lengths = r["variational_abundance"], bins.iso_len
    want = oracle.abundance(b.iso_off, t.count, t.status, lengths, r["total_mapped_reads"], min_isoform_frac=0.002)
    np.testing.assert_array_equal(ab["keep"], want["keep"])
    np.testing.assert_allclose(ab["fpkm"], want["fpkm"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ab["frac"], want["frac"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ab["tpm"], want["tpm"], rtol=1e-12, atol=0)
    assert abs(ab["total_fpkm"] - want["sum_fpkm"]) / want["sum_fpkm"] < 1e-12 and (ab["keep"] == 0).any() and (ab["fpkm"] > 0).sum() > b.n_loci


def test_abundance_against_the_restatement_through_the_oracles_epilogue(ctx, golden, oracle):
    """FPKM is linear in the count it is given: the device's count stands within RES_COUNT max(1, N) of the restatement's, so its
    FPKM within that times the isoform's FPKM per fragment (and the epilogue's own 1e-14)"""
    from strawberry_amd import em
    b = V.golden_within_limits(golden, "em_c3_400")
    s = em.EmBatchSolver(b, ctx)
    total = 3_000_000
    t = s.run_vb(abundance=vb.abundance_params(total, min_isoform_frac=0.0))
    ab = t.abundance()
    want_c = V.solve(b)
    own = oracle.abundance(b.iso_off, t.count, t.status, b.length, total, min_isoform_frac=0.0)
    np.testing.assert_array_equal(ab["keep"], own["keep"])
    np.testing.assert_allclose(ab["fpkm"], own["fpkm"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ab["tpm"], own["tpm"], rtol=1e-12, atol=0)
    want = oracle.abundance(b.iso_off, want_c["count"], want_c["status"], b.length, total, min_isoform_frac=0.0)
    same = np.repeat(t.iters == want_c["iters"], np.diff(b.iso_off))
    N = np.repeat(np.maximum(1.0, t.n_frag.astype(np.float64)), np.diff(b.iso_off))
    with np.errstate(divide="ignore", invalid="ignore"):
        per_fragment = np.where(want_c["count"] > 0, want["fpkm"] / want_c["count"], 0.0)
    tol = per_fragment * RES_COUNT * N + 1e-14 * np.abs(want["fpkm"])
    assert same.mean() >= 1.0 - V.ITERS_MAY_DIFFER and (np.abs(ab["fpkm"] - want["fpkm"])[same] <= tol[same]).all() and (ab["fpkm"] > 0).sum() > b.n_loci
    with pytest.raises(_lib.SbgpuError, match="abundance"):
        s.run_vb().abundance()


def test_any_order_with_the_fit_and_the_support(ctx):
    """Each order of variational, fit and support twice, on a toy directory: every result is the first turn's, and the resident
    call's seven outputs are the bits of the same call with nothing behind it"""
    import torch
    import fit_util as FU
    import stream_util as S
    from strawberry_amd import fit, support
    from strawberry_amd.quantify import quantify_resident
    from test_context_table_gpu import RL, RUNS, law_of, toy
    from test_fragment_assign_gpu import bits
    from test_isoform_support_gpu import bitwise as support_bitwise
    which = "E2E"
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    kw = dict(long_read=bool(RUNS[which][1]), ctx=ctx, min_isoform_frac=RUNS[which][2])
    plain = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, **kw)
    r = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, keep_handle=True, keep_bootstrap=True, **kw)
    dev = torch.device("cuda", ctx.device)
    with r["handle"] as handle:
        d_theta, d_keep, d_status = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (r["theta"], r["keep"], r["status"]))
        calls = {"variational": lambda: vb.model_vb_device(ctx, handle), "fit": lambda: fit.model_fit_device(ctx, handle, d_theta, d_keep, d_status),
                 "support": lambda: support.model_loo_device(ctx, handle, d_keep, keep=r["keep"])}
        turns = [(order, {k: calls[k]() for k in order}) for order in itertools.permutations(sorted(calls)) for _ in range(2)]
    first = turns[0][1]
    assert len(turns) == 12 and first["variational"].n_frag.sum() > 0 and (first["variational"].count > 0).any()
    for order, got in turns[1:]:
        what = " -> ".join(order)
        V.bitwise(got["variational"], first["variational"], what)
        FU.bitwise(got["fit"], first["fit"], what)
        support_bitwise(got["support"], first["support"], what)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    with_vb = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, with_variational=dict(alpha=0.01), **kw)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(with_vb[k]), bits(plain[k]), err_msg=k)
    V.bitwise(with_vb["variational"], first["variational"], "quantify_resident(with_variational=...)")


def test_front_quantifier_variational(ctx):
    """FrontQuantifier.variational() after step() and after stream_step(): the same records, the same bits; the step's results stay"""
    from strawberry_amd import front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
            plain.variational()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_bootstrap=True, **kw)
    try:
        q.step()
        theta, fpkm = q.theta[:q.n_iso].copy(), q.fpkm[:q.n_iso].copy()
        v1 = q.variational()
        ab = v1.abundance()
        q.abundance_bootstrap(4, 3, replicates=False)
        V.bitwise(q.variational(), v1, "behind a bootstrap")
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        assert q.stream_step()["chunks"] > 3
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        np.testing.assert_array_equal(q.fpkm[:q.n_iso].view(np.uint64), fpkm.view(np.uint64))
        V.bitwise(q.variational(), v1, "through the stream")
        solved = v1.status == V.OK
        assert solved.sum() > q.n_loci // 2 and set(v1.device) == set(vb.NAMES) and (v1.n_frag > 0).sum() > q.n_loci // 2
        total = np.add.reduceat(np.concatenate([v1.count, [0.0]]), q.annot.iso_off[:-1])[:q.n_loci]
        np.testing.assert_allclose(total[solved], v1.n_frag[solved], rtol=1e-9)
        print("isoforms at or above one fragment: %d under the EM, %d under alpha = 0.01" % ((theta >= 1.0).sum(), v1.supported().sum()))
        assert v1.supported().any() and (ab["fpkm"] > 0).any() and abs(ab["tpm"].sum() - 1e6) < 1.0
        rows = list(v1.rows())
        assert len(rows) == q.n_iso and len(rows[0]) == 8
        few = q.variational(alpha=1.0, want=("count",))
        assert few.share is None and (few.count != v1.count).any()
    finally:
        q.close()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, null arguments, parameters out of range, inputs
    that are not on the device"""
    from strawberry_amd import bootstrap, chain, em
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_vb(h, out=True, par=None):
        s = _lib.sbgpu_em_vb_t()
        rc = L.sbgpu_model_vb_device(ctx.h, h, C.byref(par) if par is not None else None, None, C.byref(s) if out else None)
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_vb(h0)
        assert rc == _lib.SBGPU_EINVAL and why.startswith("sbgpu_model_vb_device:") and "without retention (sbgpu_bootstrap_keep was off" in why, why
        bootstrap.bootstrap_keep(ctx, True)
        h1 = call()
        rc, why = try_vb(h1, out=False)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        for par in (_lib.sbgpu_vb_params_t(0.0, 1e-2, 10, 0), _lib.sbgpu_vb_params_t(0.01, 0.0, 10, 0), _lib.sbgpu_vb_params_t(0.01, 1e-2, 0, 0)):
            rc, why = try_vb(h1, par=par)
            assert rc == _lib.SBGPU_EINVAL and "alpha outside [1e-6, 1e3], change_limit <= 0 or max_iter < 1" in why, why
        v1 = vb.model_vb_device(ctx, h1)
        h2 = call()
        rc, why = try_vb(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        V.bitwise(vb.model_vb_device(ctx, h2), v1, "the same call twice")
        s = _lib.sbgpu_em_vb_t()
        assert L.sbgpu_em_vb_device(ctx.h, None, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "sbgpu_em_vb_device: null argument" in L.sbgpu_last_error().decode()
        b = V.many_tiny()
        plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
        assert L.sbgpu_em_vb_device(ctx.h, plan.h, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "the counts are not on the device" in L.sbgpu_last_error().decode()
        assert L.sbgpu_em_vb_device(ctx.h, plan.h, q._out.d_status, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "the weights are not on the device" in L.sbgpu_last_error().decode()
        plan.close()
    finally:
        bootstrap.bootstrap_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()


def test_report_the_worst_gaps():
    """(last in the file) what DESIGN 3.31 quotes: the largest gap of each kind over every comparison above"""
    assert WORST, "the comparisons above did not run"
    for k, bound in (("count", DEV_COUNT), ("elbo", DEV_ELBO)):
        v, where = max((w[k], label) for label, w in WORST.items() if "against host" in label)
        print("device against host, largest %s gap: %.3e of a bound of %.1e (%s)" % (k, v, bound, where))
        assert v <= bound
    print("loci whose iteration counts differ:", {label: w["differ"] for label, w in WORST.items() if w["differ"] > 0})
