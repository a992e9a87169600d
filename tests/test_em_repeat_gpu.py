"""Consecutive runs that cannot mask each other.

A test that re-solves the same (count, F) into outputs that still hold the previous run's answer passes whatever a kernel
leaves stale: a wide-kernel exchange granule of the last run, a row-keep flag the streaming kernel wrote before, an output
set a pipelined step never wrote, the epilogue's last workgroup reading the previous launch's partial sums.  Here one plan
solves K >= 3 DIFFERENT draws of (count, F) on the same offsets -- each draw zeroes other weights and other whole rows, so
rows are dropped in one draw and kept in the next -- the outputs are poisoned before every run (theta NaN, status 77,
iterations -5), and every run is compared with the oracle on ITS draw: status and iterations exact, theta to 1e-9.  The
epilogue follows every run with another total of mapped reads, against oracle.abundance (FPKM / Frac 1e-14, TPM 1e-12)."""
import os
import re

import numpy as np
import pytest

from test_em_gpu import needs_experiments

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
K_DRAWS = 3
THREADS = max(4, min(16, os.cpu_count() or 4))


def theta_err(theta, ref):
    return np.abs(theta - ref) / np.maximum(np.abs(ref), 1e-9)


def draws(b, k, seed):
    """k draws of (count, F) on b's offsets: F keeps b's pattern minus a random 15 % of its weights, plus 3 % of the rows set
    to zero entirely (dropped by init()); counts redrawn."""
    rng = np.random.default_rng(seed)
    out = []
    n_rows = int(b.row_off[-1])
    row_of_el = np.repeat(np.arange(n_rows), np.repeat(b.niso, b.nrow))
    for _ in range(k):
        keep = rng.random(b.F.size) >= 0.15
        keep &= ~(rng.random(n_rows) < 0.03)[row_of_el]
        out.append((rng.integers(0, 60, n_rows).astype(np.int32), np.where(keep, b.F, 0.0)))
    return out


def poison(s):
    s.d_theta.fill_(float("nan")), s.d_status.fill_(77), s.d_iters.fill_(-5)
    s.d_fpkm.fill_(float("nan")), s.d_frac.fill_(float("nan")), s.d_keep.fill_(77), s.d_tpm.fill_(float("nan"))


def set_draw(s, d):
    import torch
    s.d_count = torch.from_numpy(d[0]).to(s.dev)
    s.d_F = torch.from_numpy(d[1]).to(s.dev)


def check_em(r, o, what):
    np.testing.assert_array_equal(r["status"], o[1], err_msg=what)
    np.testing.assert_array_equal(r["iters"], o[2], err_msg=what)
    err = theta_err(r["theta"], o[0])
    assert err.max() < THETA_RTOL, (what, err.max(), int(err.argmax()))


def check_epilogue(oracle, b, r, total_mapped, what):
    """The epilogue of the GPU's own theta (what it was given) against oracle.abundance at the existing tolerances."""
    o = oracle.abundance(b.iso_off, r["theta"], r["status"], b.length, total_mapped_reads=total_mapped, min_isoform_frac=0.01)
    np.testing.assert_array_equal(r["keep"], o["keep"], err_msg=what)
    np.testing.assert_allclose(r["fpkm"], o["fpkm"], rtol=1e-14, atol=0, err_msg=what)
    np.testing.assert_allclose(r["frac"], o["frac"], rtol=1e-14, atol=0, err_msg=what)
    assert abs(r["sum_fpkm"] - o["sum_fpkm"]) <= 1e-12 * abs(o["sum_fpkm"]), what
    np.testing.assert_allclose(r["tpm"], o["tpm"], rtol=1e-12, atol=0, err_msg=what)


def tile_slice():
    """A slice of the C3 law whose loci all fit the tile kinds (what the fp32 entry serves)."""
    from strawberry_amd import synth
    return synth.make_c5(n_loci=4000, total_frags=4e8 / 15)


def stream_batch():
    """Wide-shaped loci (planned with SBGPU_NO_WIDE: every one on em_stream_kernel) beside tile loci."""
    from strawberry_amd import synth
    from strawberry_amd.synth import _generate
    rng = np.random.Generator(np.random.PCG64(31))
    nrow = np.array([300, 64, 1500, 90, 700, 2000, 5, 400], np.int64)
    niso = np.array([70, 512, 130, 300, 200, 66, 100, 420], np.int64)
    wide = _generate(rng, nrow, niso, nrow * 40)
    small = synth.make_random(n_loci=50, seed=8)
    return synth.concat_batches([small, wide])


def repeat_runs(b, ctx, oracle, monkeypatch=None, env=None, seed=0, epilogue=True, expect=None, after_run=None):
    """expect(plan): the route checks; after_run(solver): called after every run, before its results are read."""
    from strawberry_amd import em
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    s = em.EmBatchSolver(b, ctx)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if expect:
        expect(s.plan)
    prev = None
    for i, d in enumerate(draws(b, K_DRAWS, seed)):
        o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, d[0], d[1], threads=THREADS)
        set_draw(s, d)
        poison(s)
        s.run_em()
        if after_run:
            after_run(s)
        r = s.results()
        check_em(r, o, "draw %d" % i)
        if prev is not None:
            assert not np.array_equal(r["theta"], prev), "two draws gave one answer: the draws do not differ"
        prev = r["theta"].copy()
        if epilogue:
            total = 10 ** 6 + 77777 * i
            s.run_abundance(total_mapped_reads=total, min_isoform_frac=0.01)
            s.run_tpm()
            check_epilogue(oracle, b, s.results(), total, "draw %d" % i)
    return s


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def test_repeat_tile_kinds(ctx, oracle):
    def expect(p):
        assert (p.locus_kinds() < 5).all() and p.info()["n_stream_loci"] == 0
    repeat_runs(tile_slice(), ctx, oracle, seed=1, expect=expect)


def test_repeat_wide_rounds(ctx, oracle):
    """Wide loci beside C3 loci in at least two cooperative rounds: a 65-isoform locus one row short of the workgroup boundary
    (test_em_stream_gpu.boundary_rows: the planner's own answer) needs exactly n_cu workgroups -- a workgroup count grows by at
    most one per row, so the last row count that stays wide has G = n_cu -- and fills a round on its own (a round holds at
    most n_cu workgroups); 20 C3-T-tail-like loci (65..200 isoforms, 200..600 bins) and 8 loci of 8064 bins x 65 isoforms need
    rounds of their own.  The exchange granules' epoch tags change every run, and a granule the previous run left must never
    be taken for this run's."""
    from strawberry_amd import synth
    from strawberry_amd.synth import _generate
    from test_em_stream_gpu import boundary_rows, fast_locus
    rng = np.random.Generator(np.random.PCG64(17))
    base = synth.make_c3(n_loci=300, total_frags=1e5, seed=17, max_niso=30, max_nrow=300)
    tail = _generate(rng, rng.integers(200, 601, 20), rng.integers(65, 201, 20), np.full(20, 20000))
    long = _generate(rng, np.full(8, 8064), np.full(8, 65), np.full(8, 8064 * 20), density=0.05)
    nb = boundary_rows(ctx, 65)
    full = synth.from_loci([fast_locus(nb - 1, 65, seed=23)])
    b = synth.concat_batches([base.select(np.arange(150)), tail, full, base.select(np.arange(150, 300)), long])

    def expect(p):
        assert p.info()["n_wide_loci"] == p.info()["n_stream_loci"] == 29
    repeat_runs(b, ctx, oracle, seed=2, expect=expect)


def test_repeat_stream_kernel(ctx, oracle, monkeypatch):
    """em_stream_kernel writes each row's keep flag in init() and reads it in every iteration: a draw that keeps a row the
    previous draw dropped (and the other way round) must not see the previous flags."""
    b = stream_batch()
    n_big = 8

    def expect(p):
        assert p.info()["n_stream_loci"] == n_big and p.info()["n_wide_loci"] == 0
    repeat_runs(b, ctx, oracle, monkeypatch, env={"SBGPU_NO_WIDE": "1"}, seed=3, expect=expect)


@needs_experiments
def test_repeat_phased(ctx, oracle, monkeypatch):
    """Phases of the wave kind: survivor counts and lists that the previous run filled.  Every run must have run the later
    phases (their device times, sbgpu_em_last_phase_ms), or this would be the tile test again."""
    from strawberry_amd import _lib, synth
    b = synth.make_c3(n_loci=3000, total_frags=1e7, seed=13)

    def phased(s):
        assert len(s.last_phase_ms()) >= 3, s.last_phase_ms()     # phase 0 and the two later phases of "8,64"
    _lib.check(ctx.L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")     # (context-wide: the phases' events are recorded)
    try:
        repeat_runs(b, ctx, oracle, monkeypatch, env={"SBGPU_PHASES": "8,64", "SBGPU_PHASE_LAMBDA": "2,0.25"}, seed=4,
                    after_run=phased)
    finally:
        ctx.L.sbgpu_set_timing(ctx.h, 0)


def test_repeat_bias_entry(ctx, oracle):
    """sbgpu_em_run_device_bias on consecutive draws against the oracle on the pre-multiplied weights (test_c5_bias_gpu.py's
    comparison: exp2 on the device against numpy's may move the last bit and with it a count), with other factors each run."""
    import torch
    from strawberry_amd import em
    b = tile_slice()
    s = em.EmBatchSolver(b, ctx)
    rng = np.random.default_rng(6)
    prev = None
    for i, d in enumerate(draws(b, K_DRAWS, 5)):
        row_bias = rng.uniform(-1, 1, int(b.row_off[-1]))
        iso_bias = rng.uniform(-1, 1, int(b.iso_off[-1]))
        Fb = d[1].copy()
        for l in range(b.n_loci):
            r0, r1, j0, j1 = b.row_off[l], b.row_off[l + 1], b.iso_off[l], b.iso_off[l + 1]
            Fb[b.f_off[l]:b.f_off[l + 1]] *= np.exp2(np.outer(row_bias[r0:r1], iso_bias[j0:j1])).reshape(-1)
        theta, status, iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, d[0], Fb, threads=THREADS)
        set_draw(s, d)
        s.set_bias(torch.from_numpy(row_bias).to(s.dev), torch.from_numpy(iso_bias).to(s.dev))
        poison(s)
        s.run_em()
        got = s.results()
        assert ((got["status"] >= 0) & (got["status"] <= 3)).all() and np.isfinite(got["theta"]).all()
        assert (got["status"] == status).mean() > 0.999 and (got["iters"] == iters).mean() > 0.995, i
        m = np.repeat((got["status"] == status) & (got["iters"] == iters), b.niso)
        assert theta_err(got["theta"][m], theta[m]).max() < THETA_RTOL, i
        if prev is not None:
            assert np.abs(got["theta"] - prev).max() > 1.0
        prev = got["theta"].copy()


def test_repeat_f32(ctx, oracle):
    """The fp32 entry (tile kinds only) on consecutive draws, theta32 poisoned: the existing loose checks against the fp64
    answer of the same draw, and finite -- not the previous draw's answer."""
    import torch
    from strawberry_amd import em
    b = tile_slice()
    s = em.EmBatchSolver(b, ctx)
    prev = None
    for i, d in enumerate(draws(b, K_DRAWS, 7)):
        set_draw(s, d)
        s.d_F32 = s.d_F.to(torch.float32)
        if getattr(s, "d_theta32", None) is None:
            s.d_theta32 = torch.zeros(max(s.n_iso, 1), dtype=torch.float32, device=s.dev)
        poison(s)
        s.run_em()
        r64 = s.results()
        o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, d[0], d[1], threads=THREADS)
        check_em(r64, o, "fp64 draw %d" % i)
        poison(s)
        s.d_theta32.fill_(float("nan"))
        s.run_em_f32()
        s.synchronize()
        th32 = s.d_theta32[:s.n_iso].cpu().numpy().astype(np.float64)
        st32 = s.d_status[:b.n_loci].cpu().numpy()
        it32 = s.d_iters[:b.n_loci].cpu().numpy()
        assert ((st32 >= 0) & (st32 <= 3)).all() and np.isfinite(th32).all() and (th32 >= 0).all()
        assert (st32 == r64["status"]).mean() > 0.97
        same = (st32 == 0) & (r64["status"] == 0) & (np.abs(it32 - r64["iters"]) <= 1)
        m = same[np.repeat(np.arange(b.n_loci), b.niso)]
        rel = np.abs(th32 - r64["theta"])[m] / np.maximum(r64["theta"][m], 1.0)
        assert same.mean() > 0.8 and np.percentile(rel, 99) < 1e-3, (i, same.mean(), np.percentile(rel, 99))
        if prev is not None:
            assert np.abs(th32 - prev).max() > 1.0
        prev = th32


@pytest.mark.parametrize("n_loci", [1, 257, 65536, 65537, 200003])
def test_epilogue_every_workgroup_count(ctx, oracle, n_loci):
    """abundance_kernel's last workgroup adds the per-workgroup sums in a loop of stride 256: batches of 1, 2, 256, 257 and
    ~800 workgroups (one-isoform loci), each run twice with another total of mapped reads and its outputs poisoned."""
    from strawberry_amd import em, synth
    rng = np.random.default_rng(n_loci)
    nrow = rng.integers(1, 3, n_loci)
    row_off = np.concatenate([[0], np.cumsum(nrow)]).astype(np.int64)
    iso_off = np.arange(n_loci + 1, dtype=np.int64)
    F = rng.uniform(0.01, 1.0, int(row_off[-1]))
    count = rng.integers(0, 30, int(row_off[-1])).astype(np.int32)
    b = synth.LocusBatch(row_off, iso_off, row_off.copy(), count, F, rng.integers(300, 5000, n_loci).astype(np.int32))
    s = em.EmBatchSolver(b, ctx)
    o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=THREADS)
    for i, total in enumerate((2 * 10 ** 6 + n_loci, 3 * 10 ** 5 + 1)):
        poison(s)
        s.run_em()
        check_em(s.results(), o, "run %d" % i)
        s.run_abundance(total_mapped_reads=total, min_isoform_frac=0.01)
        s.run_tpm()
        r = s.results()
        check_epilogue(oracle, b, r, total, "n_loci %d run %d" % (n_loci, i))


# ---------------------------------------------------------------- pipelined steps over rotating inputs

def snapshot_into(s, out):
    """Copies of the step's outputs, made on the stream the observe hook runs on."""
    def observe():
        out.append({k: getattr(s, "d_" + k)[:n].clone() for k, n in (("theta", s.n_iso), ("status", s.batch.n_loci),
                                                                       ("iters", s.batch.n_loci), ("fpkm", s.n_iso),
                                                                       ("frac", s.n_iso), ("keep", s.n_iso), ("tpm", s.n_iso))})
    return observe


def pipelined_over_rotating_inputs(ctx, oracle):
    import torch
    from strawberry_amd import dist, em
    b = tile_slice()
    sets = draws(b, 3, 11)
    d_sets = [(torch.from_numpy(c).to(ctx.device), torch.from_numpy(F).to(ctx.device)) for c, F in sets]
    kw = dict(min_isoform_frac=0.01)
    # one after the other, one input set at a time; that is the oracle's answer
    want = []
    for k, (c, F) in enumerate(sets):
        ref = em.EmBatchSolver(b, ctx)
        q0 = dist.ShardQuantifier(ref, 10 ** 7, pipelined=False, inputs=[d_sets[k]], **kw)
        got = []
        q0.step(observe=snapshot_into(ref, got))
        q0.finish()
        w = {n: t.cpu().numpy() for n, t in got[0].items()}
        check_em(w, oracle.em_batch(b.row_off, b.iso_off, b.f_off, c, F, threads=THREADS), "set %d" % k)
        want.append(w)
    for a in range(3):
        for c in range(a + 1, 3):
            assert not np.array_equal(want[a]["theta"], want[c]["theta"])
    for n_steps in (1, 2, 3, 5, 8):
        s = em.EmBatchSolver(b, ctx)
        q = dist.ShardQuantifier(s, 10 ** 7, pipelined=True, inputs=d_sets, **kw)
        assert q.pipelined
        snaps = []
        for _ in range(n_steps):
            q.step(observe=snapshot_into(s, snaps))
        q.finish()
        torch.cuda.synchronize()
        assert len(snaps) == n_steps
        for i, snap in enumerate(snaps):
            for name, w in want[i % 3].items():
                assert np.array_equal(snap[name].cpu().numpy(), w), (name, "step", i, "of", n_steps)


def chosen_wave_slot(text):
    m = re.findall(r"split runs: the wave kinds' second stream = (\d+)", text)
    assert len(m) == 1, text[-2000:]
    return int(m[0])


def test_pipelined_steps_over_rotating_inputs(oracle, monkeypatch, capfd):
    """ShardQuantifier(pipelined=True) over three input sets for 1, 2, 3, 5 and 8 steps: two buffer sets against three inputs
    give every pairing; each step's snapshot equals the unpipelined result of its own set, bit for bit.  On the shipped
    library on a context of its own: the wave slot is the probe's choice, which the test reports."""
    from strawberry_amd import em
    monkeypatch.setenv("SBGPU_HOST_TIMING", "1")
    ctx = em.Context(0)
    pipelined_over_rotating_inputs(ctx, oracle)
    slot = chosen_wave_slot(capfd.readouterr().err)
    with capfd.disabled():     # (in the run's output, not only on failure)
        print("\n[test_em_repeat_gpu] split runs: the probe chose side stream %d for the wave kinds (0: none)" % slot)


@needs_experiments
@pytest.mark.parametrize("alt", ["0", "3"])
def test_pipelined_steps_with_a_forced_wave_slot(oracle, monkeypatch, capfd, alt):
    """The same with SBGPU_WAVE_ALT: no alternation at all, and the wave kinds alternating onto side stream 3."""
    from strawberry_amd import em
    monkeypatch.setenv("SBGPU_HOST_TIMING", "1")
    monkeypatch.setenv("SBGPU_WAVE_ALT", alt)
    ctx = em.Context(0)
    pipelined_over_rotating_inputs(ctx, oracle)
    assert chosen_wave_slot(capfd.readouterr().err) == int(alt)
