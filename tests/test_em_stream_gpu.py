"""em_stream_kernel -- the one-workgroup fallback for the loci the multi-workgroup kernel does not take -- against the oracle.

A locus of more than 64 isoforms (or more rows than the tall tile holds) is a "stream-kind" locus (locus kind 5).  The plan
gives it to em_wide_kernel when its best wide layout needs at most n_cu workgroups and it has rows; otherwise (more
workgroups, no rows, or SBGPU_NO_WIDE set when the plan is made) em_stream_kernel solves it.  Kind 5 alone cannot tell the
two apart, so every case here also asserts its route through the plan's counts: n_stream_loci (kind 5) and n_wide_loci (the
wide kernel's share).  More than 512 isoforms is not a route: the planner refuses such a locus (SBGPU_ESHAPE).

Status and iteration counts exact, theta within 1e-9 (relative, floor 1e-9 fragments) of the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
ROW_EPS = 1e-5          # src/estimate.cpp:380 (csrc/em_device.h: kRowEps): a row is kept only if its largest weight is > this


def theta_err(theta, ref):
    return np.abs(theta - ref) / np.maximum(np.abs(ref), 1e-9)


def check(r, o, what=""):
    o_theta, o_status, o_iters = o
    np.testing.assert_array_equal(r["status"], o_status, err_msg=what)
    np.testing.assert_array_equal(r["iters"], o_iters, err_msg=what)
    err = theta_err(r["theta"], o_theta)
    assert err.max() < THETA_RTOL, (what, err.max(), int(err.argmax()))


def route(plan):
    info = plan.info()
    return info["n_stream_loci"], info["n_wide_loci"]


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def solve(b, ctx, poison=True):
    from strawberry_amd import em
    s = em.EmBatchSolver(b, ctx)
    if poison:
        s.d_theta.fill_(float("nan")), s.d_status.fill_(77), s.d_iters.fill_(-5)
    s.run_em()
    return s, s.results()


def make_batch(loci):
    """synth.from_loci for loci that may have no rows (F of shape (0, niso))."""
    from strawberry_amd import synth
    nrow = np.array([np.shape(F)[0] for _, F in loci], np.int64)
    niso = np.array([np.shape(F)[1] for _, F in loci], np.int64)
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    count = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in loci])
    F = np.concatenate([np.asarray(f, np.float64).reshape(-1) for _, f in loci])
    return synth.LocusBatch(off(nrow), off(niso), off(nrow * niso), count, F, np.full(int(niso.sum()), 1000, np.int32))


def boundary_rows(ctx, niso):
    """The smallest row count at which a locus of `niso` isoforms leaves the wide kernel (its best layout would need more than
    n_cu workgroups): bisection over plans of that one locus -- the planner itself decides, no layout table is restated here."""
    from strawberry_amd import em

    def wide(nrow):
        p = em.Plan(ctx, np.array([0, nrow], np.int64), np.array([0, niso], np.int64), np.array([0, nrow * niso], np.int64))
        try:
            n_stream, n_wide = route(p)
        finally:
            p.close()
        assert n_stream == 1
        return n_wide == 1

    lo, hi = 1, 1 << 21
    assert wide(lo) and not wide(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if wide(mid):
            lo = mid
        else:
            hi = mid
    return hi


def fast_locus(nrow, niso, seed):
    """A locus that converges in a few dozen iterations however many rows it has: every row is strong on one isoform
    (round robin), weaker on the next, faint on a third; 0-3 fragments per row."""
    rng = np.random.default_rng(seed)
    i = np.arange(nrow)
    F = np.zeros((nrow, niso))
    F[i, i % niso] = rng.uniform(0.6, 1.0, nrow)
    F[i, (i + 1) % niso] += rng.uniform(0.05, 0.3, nrow)
    F[i, (7 * i + 3) % niso] += rng.uniform(0.001, 0.02, nrow)
    return rng.integers(0, 4, nrow).astype(np.int32), F


def random_locus(nrow, niso, seed, density=0.4):
    rng = np.random.default_rng(seed)
    F = np.where(rng.random((nrow, niso)) < density, rng.uniform(1e-3, .3, (nrow, niso)), 0.0)
    F[np.arange(nrow), rng.integers(0, niso, nrow)] += 0.05       # no empty row
    return rng.integers(0, 50, nrow).astype(np.int32), F


def decaying_locus(niso, decay_rows, seed):
    """test_em_gpu.py's tiny-denominator pattern, widened: isoform 1 loses its reads to isoform 0 and decays until its zero-count
    rows' denominators are exactly zero (DENOM_ZERO); two nearly equal isoforms keep the EM running that long."""
    rows, cnt = [], []

    def row(d, n):
        r = np.zeros(niso)
        for k, v in d.items():
            r[k] = v
        rows.append(r), cnt.append(n)
    row({0: 1.0, 1: 0.5}, 100), row({0: 1.0}, 100)
    for _ in range(decay_rows):
        row({1: 1.0}, 0)
    for k in range(6):
        a = 0.5 + 0.05 * k
        row({2: a, 3: a * (1 + 1e-3 * (k - 2.5))}, 50 + k)
    rng = np.random.default_rng(seed)
    for j in range(4, niso):
        row({j: 1.0}, int(rng.integers(5, 20)))
    return np.array(cnt, np.int32), np.array(rows)


def slow_locus(niso, seed):
    """Two isoforms that the data can hardly tell apart, many fragments: the EM creeps and stops at the 1000-iteration cap."""
    rng = np.random.default_rng(seed)
    rows, cnt = [], []
    for k in range(8):
        r = np.zeros(niso)
        a = 0.4 + 0.05 * k
        r[0], r[1] = a, a * (1 + 2e-4 * (k - 3.5))
        rows.append(r), cnt.append(20000 + 100 * k)
    for j in range(2, niso):
        r = np.zeros(niso)
        r[j] = 1.0
        rows.append(r), cnt.append(int(rng.integers(5, 50)))
    return np.array(cnt, np.int32), np.array(rows)


@pytest.fixture(scope="module")
def big(ctx, oracle):
    """Loci past the workgroup boundary (the streaming kernel's only route at default settings with rows), one per width class,
    with the boundary row count found from the planner; and the locus one row short of it (G = n_cu: one cooperative round
    with a workgroup on every CU).  Oracle results computed once."""
    loci, want = [], []
    for k, (niso, extra) in enumerate(((65, 0), (512, 37))):
        nb = boundary_rows(ctx, niso)
        loci.append(fast_locus(nb + extra, niso, seed=k))
        want.append("stream")
    nb65 = boundary_rows(ctx, 65)
    loci.append(fast_locus(nb65 - 1, 65, seed=9))
    want.append("wide")
    b = make_batch(loci)
    o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=len(loci))
    assert (o[1] == 0).all() and o[2].max() <= 200, o[1:]
    return loci, want, o


def test_planner_refuses_more_than_512_isoforms(ctx):
    from strawberry_amd import _lib, em
    for niso in (513, 600):
        with pytest.raises(_lib.SbgpuError):
            em.Plan(ctx, np.array([0, 3], np.int64), np.array([0, niso], np.int64), np.array([0, 3 * niso], np.int64))


def test_stream_kernel_past_the_workgroup_boundary(ctx, big):
    """The narrowest and the widest class (65, 512 isoforms) one row and more past the boundary -> streaming kernel; 65 isoforms one row
    short of it -> the wide kernel with exactly n_cu workgroups."""
    loci, want, o = big
    b = make_batch(loci)
    s, r = solve(b, ctx)
    assert (s.plan.locus_kinds() == 5).all()
    assert route(s.plan) == (len(loci), want.count("wide"))
    check(r, o, "boundary")
    # and each locus on its own: its route alone, the same answer
    for k, (l, w) in enumerate(zip(loci, want)):
        bl = make_batch([l])
        sl, rl = solve(bl, ctx)
        assert route(sl.plan) == (1, 1 if w == "wide" else 0), (k, w)
        j0, j1 = int(b.iso_off[k]), int(b.iso_off[k + 1])
        check(rl, (o[0][j0:j1], o[1][k:k + 1], o[2][k:k + 1]), "locus %d" % k)


def test_stream_kernel_zero_rows_row_drop_and_statuses(ctx, oracle, monkeypatch):
    """Through the streaming kernel (SBGPU_NO_WIDE, read when the plan is made): loci of more than 64 isoforms and no rows
    (INIT_EMPTY even without the switch); rows whose largest weight is exactly kRowEps (dropped), the next double above it
    (kept), rows of count 0, a locus whose every row is dropped (INIT_EMPTY); DENOM_ZERO; the 1000-iteration cap."""
    from strawberry_amd import em
    rng = np.random.default_rng(41)
    eps_up = np.nextafter(ROW_EPS, 1.0)

    def threshold_locus(nrow, niso, seed):
        c, F = random_locus(nrow, niso, seed)
        r = np.random.default_rng(seed + 1)
        at = r.choice(nrow, nrow // 4, replace=False)
        F[at] = 0.0
        F[at, r.integers(0, niso, len(at))] = ROW_EPS                       # dropped
        up = r.choice(np.setdiff1d(np.arange(nrow), at), nrow // 8, replace=False)
        F[up] = 0.0
        col = r.integers(0, niso, len(up))
        F[up, col] = eps_up                                                 # kept
        h = up[: len(up) // 2]
        F[h, (col[: len(h)] + 1) % niso] = ROW_EPS / 3                       # (a second, smaller weight does not change that)
        c[r.choice(nrow, nrow // 5, replace=False)] = 0                     # count 0 rows
        return c, F

    loci = [
        (np.zeros(0, np.int32), np.zeros((0, 100))),                          # no rows
        threshold_locus(300, 90, 1), threshold_locus(1000, 200, 2), threshold_locus(64, 512, 3),
        (rng.integers(1, 9, 40).astype(np.int32), np.full((40, 130), ROW_EPS)),   # every row dropped -> INIT_EMPTY
        decaying_locus(300, 9, 4), decaying_locus(512, 40, 5),
        slow_locus(70, 6),
        random_locus(5, 65, 7), random_locus(2000, 66, 8),
    ]
    b = make_batch(loci)
    o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=8)
    assert o[1][0] == 1 and o[1][4] == 1 and (o[1][5:7] == 2).all() and o[1][7] == 3, o[1]
    kept = [(b.locus(l)[1].max(axis=1) > ROW_EPS).sum() for l in (1, 2, 3)]
    assert all(0 < k < n for k, n in zip(kept, (300, 1000, 64)))
    # without the switch: the row-less locus is the only one on the streaming kernel
    p0 = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
    assert route(p0) == (len(loci), len(loci) - 1)
    p0.close()
    monkeypatch.setenv("SBGPU_NO_WIDE", "1")
    s, r = solve(b, ctx)
    assert route(s.plan) == (len(loci), 0)
    check(r, o, "stream")


def test_mixed_plan_tile_wide_and_stream_loci_shuffled(ctx, oracle, big):
    """One plan of tile loci, wide loci and streaming loci in shuffled order: the streaming kernel's loci start n_wide_loci
    entries into the stream class' list."""
    from strawberry_amd import synth
    loci, want, o_big = big
    rng = np.random.default_rng(5)
    small = synth.make_random(n_loci=300, seed=21)
    parts = [(small.locus(l), None) for l in range(small.n_loci)]
    wide = [random_locus(int(n), int(k), 100 + i) for i, (n, k) in enumerate(((40, 65), (700, 100), (90, 129), (300, 256), (200, 420)))]
    parts += [(w, None) for w in wide]
    parts += [((np.zeros(0, np.int32), np.zeros((0, 77))), None), ((np.zeros(0, np.int32), np.zeros((0, 300))), None)]
    parts += [(loci[0], 0), (loci[1], 1)]                                  # two past the workgroup boundary
    order = rng.permutation(len(parts))
    b = make_batch([parts[i][0] for i in order])
    # the oracle: the small loci here, the big ones from the fixture
    small_idx = [k for k, i in enumerate(order) if parts[i][1] is None]
    bs = b.select(small_idx)
    os_ = oracle.em_batch(bs.row_off, bs.iso_off, bs.f_off, bs.count, bs.F, threads=8)
    o_theta = np.zeros(int(b.iso_off[-1]))
    o_status = np.zeros(b.n_loci, np.int32)
    o_iters = np.zeros(b.n_loci, np.int32)
    big_ob = make_batch(loci)
    for k, i in enumerate(order):
        j0, j1 = int(b.iso_off[k]), int(b.iso_off[k + 1])
        if parts[i][1] is None:
            m = small_idx.index(k)
            o_theta[j0:j1] = os_[0][bs.iso_off[m]:bs.iso_off[m + 1]]
            o_status[k], o_iters[k] = os_[1][m], os_[2][m]
        else:
            g = parts[i][1]
            o_theta[j0:j1] = o_big[0][big_ob.iso_off[g]:big_ob.iso_off[g + 1]]
            o_status[k], o_iters[k] = o_big[1][g], o_big[2][g]
    s, r = solve(b, ctx)
    kinds = s.plan.locus_kinds()
    assert (kinds == 5).sum() == 9 and (kinds < 5).sum() == 300
    assert route(s.plan) == (9, 5)
    check(r, (o_theta, o_status, o_iters), "mixed")


def test_forced_fallback_on_the_wide_shapes(ctx, oracle, monkeypatch):
    """tools/check_wide_shapes.py's 41 shapes in one batch: on the wide kernel as planned, and on the streaming kernel with
    SBGPU_NO_WIDE=1 set for the second plan only -- the same oracle answer both times; the host entry gives the device path's
    bytes on the fallback plan.  40 of them are stream-kind loci; 700 x 40 is not: its 40 isoforms take 8 column lanes of
    5 columns, and the tall tile's 32 row lanes x 25 rows (plan.h: tile_rows(5, kBlockTallRh)) hold its 700 rows."""
    from strawberry_amd import em
    from strawberry_amd.synth import _generate
    shapes = [(64, 400), (128, 194), (256, 100), (700, 40), (300, 70), (90, 96), (500, 97), (333, 129), (40, 193), (777, 257),
              (100, 385), (64, 512), (1500, 300), (2600, 130), (3000, 500), (5000, 65), (1, 100), (7, 300),
              (300, 75), (801, 80), (900, 110), (450, 112), (1200, 150), (257, 160), (400, 210), (161, 224), (2000, 310),
              (129, 320), (800, 440), (81, 448), (513, 64), (20, 66), (577, 97), (97, 512), (4000, 400),
              (200, 128), (1500, 120), (417, 113), (300, 256), (1300, 240), (209, 225)]
    assert len(shapes) == 41
    nrow = np.array([s[0] for s in shapes], np.int64)
    niso = np.array([s[1] for s in shapes], np.int64)
    b = _generate(np.random.Generator(np.random.PCG64(5)), nrow, niso, nrow * 50)
    o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=16)
    monkeypatch.delenv("SBGPU_NO_WIDE", raising=False)
    s, r = solve(b, ctx)
    kinds = s.plan.locus_kinds()
    assert kinds[shapes.index((700, 40))] == 4 and (kinds == 5).sum() == 40
    n_stream, n_wide = route(s.plan)
    assert n_wide == n_stream == 40, (n_stream, n_wide)
    check(r, o, "wide")
    monkeypatch.setenv("SBGPU_NO_WIDE", "1")
    s2, r2 = solve(b, ctx)
    assert route(s2.plan) == (n_stream, 0)
    check(r2, o, "stream")
    theta, status, iters = em.em_batch_host(b, ctx)
    np.testing.assert_array_equal(theta, r2["theta"])
    np.testing.assert_array_equal(status, r2["status"])
    np.testing.assert_array_equal(iters, r2["iters"])


def test_bias_and_f32_entries_refuse_a_stream_fallback_plan(ctx, oracle, big):
    """sbgpu_em_run_device_bias / _f32 do not serve the streaming kernel: SBGPU_EUNSUPPORTED, and nothing is launched -- the
    plain entry afterwards still gives the oracle's answer."""
    import torch
    from strawberry_amd import _lib
    loci, _, o_big = big
    small = [random_locus(30, 8, 1), random_locus(200, 90, 2)]
    b = make_batch(small + [loci[0]])
    bs = make_batch(small)
    o_small = oracle.em_batch(bs.row_off, bs.iso_off, bs.f_off, bs.count, bs.F)
    s, _ = solve(b, ctx, poison=False)
    assert route(s.plan) == (2, 1)
    L = ctx.L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rb = torch.zeros(int(b.row_off[-1]), dtype=torch.float64, device=s.dev)
    ib = torch.zeros(int(b.iso_off[-1]), dtype=torch.float64, device=s.dev)
    s.d_theta.fill_(float("nan")), s.d_status.fill_(77), s.d_iters.fill_(-5)
    rc = L.sbgpu_em_run_device_bias(ctx.h, s.plan.h, s.d_count.data_ptr(), s.d_F.data_ptr(), rb.data_ptr(), ib.data_ptr(),
                                    s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr(), stream)
    assert rc == _lib.SBGPU_EUNSUPPORTED, rc
    F32 = s.d_F.to(torch.float32)
    th32 = torch.zeros(int(b.iso_off[-1]), dtype=torch.float32, device=s.dev)
    rc = L.sbgpu_em_run_device_f32(ctx.h, s.plan.h, s.d_count.data_ptr(), F32.data_ptr(), th32.data_ptr(),
                                   s.d_status.data_ptr(), s.d_iters.data_ptr(), stream)
    assert rc == _lib.SBGPU_EUNSUPPORTED, rc
    torch.cuda.synchronize()
    assert (s.d_status.cpu().numpy()[:3] == 77).all()      # refused before anything ran
    s.run_em()
    r = s.results()
    j = int(bs.iso_off[-1])
    o_theta = np.concatenate([o_small[0], o_big[0][:65]])
    check(r, (o_theta, np.concatenate([o_small[1], o_big[1][:1]]), np.concatenate([o_small[2], o_big[2][:1]])), "after refusals")
    assert j + 65 == len(o_theta)
