"""The isoform information built on the device (sbgpu_em_info_device / sbgpu_model_info_device, csrc/info_device.h) against the
host form (sbgpu_em_info_host under the same theta, keep and status), BIT FOR BIT in every array -- the rule states the order of
every sum, the wave's reduction included -- and against tests/info_util.py::by_hand under the bounds at the head of info_util.py:
on the five EM goldens (em_edge without the one locus beyond the device's shape limits, which the host form analyses and the
device form reports as TOO_WIDE), under the EM's theta and under a bootstrap mean; on a locus on either side of every threshold
the library exports; past two passes of both kernels' grids; two calls; through the resident entries; in every position among
the fit, the table, the assignment and the coverage; the refusals."""
import ctypes as C

import numpy as np
import pytest

import fit_util as FU
import info_util as IU
import retained_util as R
from strawberry_amd import _lib, assign, context, coverage, fit, info

pytestmark = pytest.mark.gpu

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
SHARES = {}


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def within_limits(b):
    lim = info.limits()
    return np.nonzero((np.diff(b.row_off) <= lim["max_bins"]) & (np.diff(b.iso_off) <= lim["max_iso"]))[0]


def wave_form(b):
    """which loci a wave serves (the others get a workgroup)"""
    lim = info.limits()
    rows, niso = np.diff(b.row_off), np.diff(b.iso_off)
    return (rows <= lim["wave_vals"]) & (niso <= lim["wave_iso"]) & (rows * niso <= lim["wave_vals"])


def note(label, r):
    SHARES[label] = r["share"]
    print(label, "worst share of cov's bound %.4f at %s, left out %s" % (r["share"], r["where"], r["left_out"]))


@pytest.fixture(scope="module")
def G(ctx, golden):
    """name -> the golden (within the limits), solved on the device, with the information under the EM's theta (twice) and under
    a bootstrap mean, the host forms of both, and by_hand (numpy route: the exact one is the CPU tests') under the EM's theta"""
    from strawberry_amd import em
    out = {}
    for name in GOLDENS:
        full, _, _ = golden(name)
        idx = within_limits(full)
        b = full if len(idx) == full.n_loci else FU.select_loci(full, idx)
        s = em.EmBatchSolver(b, ctx)
        s.run_em()
        r = s.results()
        t, again = s.run_info(), s.run_info()
        mean = s.run_bootstrap(8, 5)["mean"]
        s.synchronize()
        t_mean = s.run_info(d_theta=mean.contiguous())
        mean = mean.cpu().numpy()
        out[name] = dict(b=b, full=full, r=r, t=t, again=again, t_mean=t_mean, mean=mean, few=s.run_info(want=("se", "rank")),
                         host=info.em_info_host(b, r["theta"], status=r["status"]), host_mean=info.em_info_host(b, mean, status=r["status"]),
                         want=IU.by_hand(b, r["theta"], None, r["status"], exact_limit=0))
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_device_is_the_host_form_bit_for_bit_on_the_goldens(G, name):
    g = G[name]
    IU.bitwise(g["t"], g["host"], name)
    IU.bitwise(g["t_mean"], g["host_mean"], name + ", a bootstrap mean")
    assert (g["mean"] != g["r"]["theta"]).any() and (g["t_mean"].se != g["t"].se).any()
    note(name + ", device against by_hand", IU.compare(g["t"], g["want"], g["b"], name))
    few = g["few"]
    assert few.cov is None and few.ident is None and set(few.device) == set(info.NAMES) | {"cov_off"}
    np.testing.assert_array_equal(few.se, g["t"].se)
    np.testing.assert_array_equal(few.rank, g["t"].rank)
    t = g["t"]
    print(name, "loci OK %d EMPTY %d TOO_WIDE %d; isoforms aliased %d unobserved %d"
          % (tuple(int((t.info_status == k).sum()) for k in range(3)) + (int((t.ident == IU.ALIASED).sum()), int((t.ident == IU.UNOBSERVED).sum()))))


@pytest.mark.parametrize("name", GOLDENS)
def test_two_calls_are_bitwise_equal(G, name):
    IU.bitwise(G[name]["t"], G[name]["again"], name)


def test_a_locus_beyond_the_shape_limits_is_too_wide_not_refused(ctx, G):
    from strawberry_amd import em
    full = G["em_edge"]["full"]
    rows = np.diff(full.row_off)
    assert full.n_loci == G["em_edge"]["b"].n_loci + 1 and rows.max() > info.limits()["max_bins"]
    big = int(np.argmax(rows))
    s = em.EmBatchSolver(full, ctx)
    s.run_em()
    r = s.results()
    t = s.run_info()
    host = info.em_info_host(full, r["theta"], status=r["status"])
    assert t.info_status[big] == IU.TOO_WIDE and host.info_status[big] != IU.TOO_WIDE
    sl = slice(int(full.iso_off[big]), int(full.iso_off[big + 1]))
    assert (t.ident[sl] == IU.SKIPPED).all() and not t.se[sl].any() and (t.partner[sl] == -1).all() and t.rank[big] == 0 and t.n_free[big] == 0
    others = [l for l in range(full.n_loci) if l != big]
    for k in ("se", "partner_corr", "ident", "alias_of", "partner"):
        np.testing.assert_array_equal(FU.per_locus_slices(getattr(t, k), full.iso_off, others), FU.per_locus_slices(getattr(host, k), full.iso_off, others), err_msg=k)
    np.testing.assert_array_equal(t.rank[others], host.rank[others])


def shaped(rng, rows, niso, density=0.5, empty=False):
    F = rng.uniform(1e-3, 0.3, (rows, niso)) * (rng.random((rows, niso)) < density)
    F[rng.integers(0, rows), :] = rng.uniform(1e-3, 0.3, niso)        # one row that carries every isoform
    if rows > 2:
        F[1, :] = 1e-6                                                  # a dropped row
    if empty:
        F[:] = 1e-7
    return rng.integers(0, 60, rows).astype(np.int32), F


def own_bin_each(rng, nf):
    """nf isoforms with a bin of their own each, plus one shared bin: all free, all identified"""
    F = np.vstack([np.diag(rng.uniform(0.05, 0.5, nf)), rng.uniform(0.01, 0.1, (1, nf))])
    return rng.integers(1, 40, nf + 1).astype(np.int32), F


def twins(rng, rows, niso):
    """columns 1 and niso - 1 are column 0's: two aliased isoforms"""
    n, F = shaped(rng, rows, niso, density=0.8)
    F[:, 1] = F[:, 0]
    F[:, niso - 1] = F[:, 0]
    return n, F


def threshold_loci(rng):
    lim = info.limits()
    wv, wi, st, mf = lim["wave_vals"], lim["wave_iso"], lim["stage_vals"], lim["max_free"]
    return {"1x1": shaped(rng, 1, 1), "wave, most bins": shaped(rng, wv, 1), "block, bins": shaped(rng, wv + 1, 1),
            "wave, most isoforms": shaped(rng, wv // wi, wi), "block, isoforms": shaped(rng, 2, wi + 1),
            "block, weights": shaped(rng, wv // wi + 1, wi), "63 bins": shaped(rng, 63, 3, 0.9), "64 bins": shaped(rng, 64, 3, 0.9),
            "65 bins": shaped(rng, 65, 3, 0.9), "most free": own_bin_each(rng, mf), "too many free": own_bin_each(rng, mf + 1),
            "w in LDS, last": shaped(rng, st, 1), "w in global memory": shaped(rng, st + 1, 1),
            "F staged, last": shaped(rng, st // 32, 32), "F from global memory": shaped(rng, st // 32 + 1, 32),
            "tall": shaped(rng, lim["max_bins"], 2), "wide, few free": shaped(rng, 12, 300, 0.3),
            "twins, wave": twins(rng, 20, 5), "twins, block": twins(rng, 700, 6),
            "before": shaped(rng, 7, 3), "never started": shaped(rng, 6, 3, empty=True), "after": shaped(rng, 9, 4)}


@pytest.fixture(scope="module")
def T(ctx):
    """One locus on either side of every threshold, under a made-up theta and filter (the information takes any), with a locus
    that never started between two ordinary ones"""
    import torch
    from strawberry_amd import em
    rng = np.random.default_rng(24)
    loci = threshold_loci(rng)
    names = list(loci)
    b = FU.from_loci(list(loci.values()))
    n_iso = int(b.iso_off[-1])
    theta = rng.uniform(0.5, 40.0, n_iso)
    keep = (rng.random(n_iso) < 0.9).astype(np.int32)
    keep[np.asarray(b.iso_off[:-1])] = 1
    for name in ("most free", "too many free", "twins, wave", "twins, block"):
        l = names.index(name)
        keep[int(b.iso_off[l]):int(b.iso_off[l + 1])] = 1
    few = names.index("wide, few free")
    keep[int(b.iso_off[few]) + 20:int(b.iso_off[few + 1])] = 0          # 300 isoforms, at most 20 of them free
    status = np.zeros(b.n_loci, np.int32)
    status[names.index("never started")] = _lib.EM_INIT_EMPTY
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, theta, keep, status)]
    t = info.em_info_device(ctx, plan, *d)
    again = info.em_info_device(ctx, plan, *d)
    all_kept = info.em_info_device(ctx, plan, d[0], d[1], d[2])
    plan.close()
    return dict(b=b, names=names, theta=theta, keep=keep, status=status, t=t, again=again, all_kept=all_kept,
                host=info.em_info_host(b, theta, keep, status), host_all=info.em_info_host(b, theta),
                want=IU.by_hand(b, theta, keep, status, exact_cost=3000))


def test_a_locus_on_either_side_of_every_threshold(T):
    lim = info.limits()
    b, names, t = T["b"], T["names"], T["t"]
    at = {k: i for i, k in enumerate(names)}
    shapes = dict(zip(names, zip(np.diff(b.row_off), np.diff(b.iso_off))))
    wave = dict(zip(names, wave_form(b)))
    for name in ("1x1", "wave, most bins", "wave, most isoforms", "63 bins", "64 bins", "65 bins", "twins, wave", "before", "never started", "after"):
        assert wave[name], name
    for name in ("block, bins", "block, isoforms", "block, weights", "most free", "too many free", "w in LDS, last", "w in global memory",
                 "F staged, last", "F from global memory", "tall", "wide, few free", "twins, block"):
        assert not wave[name], name
    assert shapes["wave, most bins"] == (lim["wave_vals"], 1) and shapes["wave, most isoforms"] == (lim["wave_vals"] // lim["wave_iso"], lim["wave_iso"])
    assert shapes["w in LDS, last"][0] == lim["stage_vals"] and shapes["F staged, last"][0] * shapes["F staged, last"][1] == lim["stage_vals"]
    assert shapes["tall"] == (lim["max_bins"], 2)
    IU.bitwise(t, T["host"], "thresholds")
    IU.bitwise(T["all_kept"], T["host_all"], "thresholds, everything kept")
    IU.bitwise(t, T["again"], "thresholds, again")
    note("thresholds, device against by_hand", IU.compare(t, T["want"], b, "thresholds"))
    assert t.info_status[at["most free"]] == IU.OK and t.n_free[at["most free"]] == t.rank[at["most free"]] == lim["max_free"]
    assert t.info_status[at["too many free"]] == IU.TOO_WIDE and t.covariance(at["too many free"]) is None
    assert t.info_status[at["never started"]] == IU.EMPTY and t.info_status[at["before"]] == t.info_status[at["after"]] == IU.OK
    assert t.info_status[at["wide, few free"]] == IU.OK and 0 < t.n_free[at["wide, few free"]] <= 20 and t.covariance(at["wide, few free"]) is None
    for name in ("twins, wave", "twins, block"):
        l = at[name]
        i0, niso = int(b.iso_off[l]), shapes[name][1]
        assert t.ident[i0] == IU.IDENTIFIED and t.ident[i0 + 1] == t.ident[i0 + niso - 1] == IU.ALIASED, name
        assert t.alias_of[i0 + 1] == t.alias_of[i0 + niso - 1] == 0 and t.rank[l] == niso - 2, name
    assert (T["keep"] == 0).any() and (t.ident == IU.NOT_FREE).any() and (t.ident == IU.SKIPPED).any()


def test_more_loci_than_two_passes_of_either_grid(ctx, golden):
    """em_c3_400's loci repeated until the wave form's list and the workgroup form's both exceed two passes of their grids:
    every repeat of a locus gets the first one's bits, and the first ones are the host form's"""
    import torch
    from strawberry_amd import em
    lim = info.limits()
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    cap = lim["grid_per_cu"] * cu
    full, _, _ = golden("em_c3_400")
    large = np.nonzero(~wave_form(full))[0]
    small = np.nonzero(wave_form(full))[0][:4 * lim["wave_loci"] * len(large)]
    base = FU.select_loci(full, np.sort(np.concatenate([large, small])))
    reps = 2 * cap // len(large) + 1
    b = FU.tile_batch(base, reps)
    n_large = int((~wave_form(b)).sum())
    assert n_large > 2 * cap and b.n_loci - n_large > 2 * cap * lim["wave_loci"], (b.n_loci, n_large, cap)
    s0 = em.EmBatchSolver(base, ctx)
    s0.run_em()
    r0 = s0.results()
    theta, status = np.tile(r0["theta"], reps), np.tile(r0["status"], reps)
    dev = torch.device("cuda", ctx.device)
    plan = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b.count, b.F, theta, status)]
    t = info.em_info_device(ctx, plan, d[0], d[1], d[2], None, d[3])
    plan.close()
    first = info.em_info_host(base, r0["theta"], status=r0["status"])
    for k in info.NAMES:
        x, f = getattr(t, k), getattr(first, k)
        view = (lambda a: a.view(np.uint64)) if x.dtype == np.float64 else (lambda a: a)
        np.testing.assert_array_equal(view(x).reshape(reps, -1), np.tile(view(f), (reps, 1)), err_msg=k)
    assert (first.ident == IU.ALIASED).any() and first.cov.any()


@pytest.fixture(scope="module")
def E(ctx):
    """One resident call on the edge sample with the information behind it; the same call's weights through sbgpu_quantify_host"""
    import torch
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small, grid = R.n_small_for(cu), R.GRID_PER_CU * cu
    annot, hits = R.edge_sample(n_small, grid=grid)
    law = InsertSize(*R.LAW)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_info=True)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    return dict(r=r, h=h, at=R.edge_layout(n_small))


def test_the_edge_sample_through_a_resident_call(E):
    import types
    r, h = E["r"], E["h"]
    bins = h["bins"]
    batch = types.SimpleNamespace(row_off=bins.row_off, iso_off=bins.iso_off, f_off=bins.f_off, count=bins.count, F=h["F"], n_loci=len(bins.row_off) - 1)
    t = r["isoform_info"]
    np.testing.assert_array_equal(t.iso_off, bins.iso_off)
    host = info.em_info_host(batch, r["theta"], r["keep"], r["status"])
    IU.bitwise(t, host, "edge sample")
    note("edge sample, device against by_hand", IU.compare(t, IU.by_hand(batch, r["theta"], r["keep"], r["status"], exact_limit=0), batch, "edge sample"))
    at = E["at"]
    # the sample's 300-isoform locus has more free isoforms than the limit; its 6- and 40-isoform ones do not
    assert t.info_status[at["EMPTY"]] == IU.EMPTY and t.info_status[at["C"]] == IU.TOO_WIDE and t.info_status[at["A"]] == IU.OK
    assert t.info_status[at["B"]] != IU.TOO_WIDE and (r["keep"] == 0).any() and (~wave_form(batch)).sum() >= 4
    assert (t.ident == IU.IDENTIFIED).any() and (t.ident == IU.NOT_FREE).any()


def test_in_every_position_among_fit_table_assignment_and_coverage(ctx):
    """On a toy directory: the information asked for first, last and between the four other stages; every stage's arrays are the
    first turn's bits, and the resident call's seven outputs are the bits of the same call with nothing behind it."""
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
        calls = {"info": lambda: info.model_info_device(ctx, handle, d_theta, d_keep, d_status),
                 "fit": lambda: fit.model_fit_device(ctx, handle, d_theta, d_keep, d_status),
                 "table": lambda: context.context_table_device(ctx, handle),
                 "assignment": lambda: assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass),
                 "coverage": lambda: coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)}
        others = ["fit", "table", "assignment", "coverage"]
        orders = [tuple(others[:p] + ["info"] + others[p:]) for p in range(5)] + [tuple(["info"] + others[::-1])]
        turns = [(order, {k: calls[k]() for k in order}) for order in orders]
        del own
    first = turns[0][1]
    assert (first["info"].ident == IU.IDENTIFIED).any() and first["info"].se.any()
    for order, got in turns[1:]:
        what = " -> ".join(order)
        IU.bitwise(got["info"], first["info"], what)
        FU.bitwise(got["fit"], first["fit"], what)
        assert_same_table(got["table"], first["table"], what)
        assert_same_assignment(got["assignment"], first["assignment"], np.asarray(annot.iso_off), hits_of, what)
        CU.compare(got["coverage"], first["coverage"], annot, hits.hit_locus, False, what)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    with_info = quantify_resident(annot, hits, law_of(which), RL, hits.total_mapped, with_info=True, **kw)
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(bits(with_info[k]), bits(plain[k]), err_msg=k)
    IU.bitwise(with_info["isoform_info"], first["info"], "quantify_resident(with_info=True)")


def test_front_quantifier_isoform_information(ctx):
    """FrontQuantifier.isoform_information() after step() and after stream_step(): the same records, the same bits"""
    from strawberry_amd import front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
            plain.isoform_information()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_bootstrap=True, **kw)
    try:
        q.step()
        theta = q.theta[:q.n_iso].copy()
        f1 = q.isoform_information()
        q.abundance_bootstrap(4, 3, replicates=False)
        IU.bitwise(q.isoform_information(), f1, "behind a bootstrap")
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        assert q.stream_step()["chunks"] > 3
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        IU.bitwise(q.isoform_information(), f1, "through the stream")
        assert (f1.info_status == IU.OK).sum() > q.n_loci // 4 and (f1.se > 0).any() and set(f1.device) == set(info.NAMES) | {"cov_off"}
        few = q.isoform_information(want=("ident",))
        assert few.se is None
        np.testing.assert_array_equal(few.ident, f1.ident)
    finally:
        q.close()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, a null theta, null arguments, a cov_off that
    is not the batch's."""
    from strawberry_amd import bootstrap, chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_info(h, d_theta=True, out=True, s=None):
        s = s or _lib.sbgpu_em_info_t()
        rc = L.sbgpu_model_info_device(ctx.h, h, q._out.d_theta if d_theta else None, None, None, None, C.byref(s) if out else None)
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_info(h0)
        assert rc == _lib.SBGPU_EINVAL and why.startswith("sbgpu_model_info_device:") and "without retention (sbgpu_bootstrap_keep was off" in why, why
        bootstrap.bootstrap_keep(ctx, True)
        h1 = call()
        rc, why = try_info(h1, d_theta=False)
        assert rc == _lib.SBGPU_EINVAL and "d_theta is needed" in why, why
        rc, why = try_info(h1, out=False)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        cov, bad = np.zeros(16), np.zeros(q.n_loci + 1, np.int64)
        s = _lib.sbgpu_em_info_t()
        s.cov = cov.ctypes.data
        rc, why = try_info(h1, s=s)
        assert rc == _lib.SBGPU_EINVAL and "cov is given without cov_off" in why, why
        s.cov_off = bad.ctypes.data
        rc, why = try_info(h1, s=s)
        assert rc == _lib.SBGPU_EINVAL and "cov_off is not sbgpu_em_info_cov_offsets'" in why, why
        f1 = info.model_info_device(ctx, h1, int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status))
        h2 = call()
        rc, why = try_info(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        f2 = info.model_info_device(ctx, h2, int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status))
        IU.bitwise(f2, f1, "the same call twice")
        s = _lib.sbgpu_em_info_t()
        assert L.sbgpu_em_info_device(ctx.h, None, None, None, None, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert "sbgpu_em_info_device: null argument" in L.sbgpu_last_error().decode()
    finally:
        bootstrap.bootstrap_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()


def test_report_the_worst_share_of_covs_bound():
    """(last in the file) what DESIGN 3.24 quotes: the largest share of cov's bound over every comparison above"""
    assert SHARES, "the comparisons above did not run"
    label = max(SHARES, key=SHARES.get)
    print("worst share of cov's bound on this device: %.4f (%s)" % (SHARES[label], label))
    assert SHARES[label] <= 1.0
