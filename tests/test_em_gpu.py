"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the
reference goldens.  Tolerances: theta within 1e-9 relative (floor 1e-9 fragments)
of the reference -- five orders tighter than the 1e-4 the north star asks of
FPKM/TPM; status and iteration counts exact."""
import numpy as np
import os

import pytest

from conftest import ref_flags_to_status

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
THETA_FLOOR = 1e-9


def theta_err(theta, ref):
    return np.abs(theta - ref) / np.maximum(np.abs(ref), THETA_FLOOR)


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def solve(batch, ctx):
    from strawberry_amd import em
    s = em.EmBatchSolver(batch, ctx)
    s.run_em()
    return s, s.results()


@pytest.mark.parametrize("name", ["em_edge", "em_random_256", "em_c2_64", "em_c3_400", "em_c4_assembled"])
def test_gpu_matches_reference_goldens(ctx, oracle, golden, name):
    b, ref_theta, ref_flags = golden(name)
    _, r = solve(b, ctx)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    np.testing.assert_array_equal(r["status"], ref_flags_to_status(ref_flags, o_status))
    np.testing.assert_array_equal(r["status"], o_status)
    err = theta_err(r["theta"], ref_theta)
    assert err.max() < THETA_RTOL, (name, err.max(), int(err.argmax()))
    # iteration counts are part of the contract (absolute 1e-2 threshold, SURVEY "hard parts")
    np.testing.assert_array_equal(r["iters"], o_iters)


def test_gpu_known_answers_per_locus_adapter(ctx):
    """EmSolver-shaped adapter: init()/run()/_theta like src/estimate.cpp:305-313."""
    from strawberry_amd.em import EmSolver
    from test_oracle import KATS
    for name, n, F, status, theta in KATS:
        em = EmSolver(ctx)
        ok = em.init(len(F[0]), n, F)
        ran = em.run()
        assert ok == (status != 1), name
        assert ran == (status in (0, 3)), name
        np.testing.assert_allclose(em._theta, theta, rtol=2e-11, atol=1e-11, err_msg=name)


def test_gpu_host_buffer_entry(ctx, oracle, golden):
    """sbgpu_em_batch (host pointers in/out) == device-resident path."""
    from strawberry_amd import em
    b, ref_theta, _ = golden("em_random_256")
    theta, status, iters = em.em_batch_host(b, ctx)
    _, r = solve(b, ctx)
    np.testing.assert_array_equal(theta, r["theta"])
    np.testing.assert_array_equal(status, r["status"])
    np.testing.assert_array_equal(iters, r["iters"])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 2), (33, 3), (64, 8), (65, 8), (200, 5),
                                   (257, 8), (300, 16), (129, 32), (2000, 8), (5000, 2), (40, 33), (100, 64),
                                   (9000, 2), (1000, 20), (3000, 20), (17, 13), (500, 40), (64, 65), (30, 200),
                                   (9, 4), (50, 6), (70, 12), (33, 24), (20, 48), (90, 28), (15, 56), (400, 6), (700, 11)])
def test_gpu_every_size_class(ctx, oracle, shape):
    """One batch per (nrow, niso) shape so that each tile / workgroup / streaming
    class is exercised on its own, including its padding."""
    from strawberry_amd import synth
    nrow, niso = shape
    rng = np.random.Generator(np.random.PCG64(nrow * 1000 + niso))
    loci = []
    for _ in range(6):
        F = np.where(rng.random((nrow, niso)) < 0.5, rng.uniform(1e-3, .3, (nrow, niso)), 0.0)
        loci.append((rng.integers(0, 50, nrow).astype(np.int32), F))
    b = synth.from_loci(loci)
    _, r = solve(b, ctx)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    assert theta_err(r["theta"], o_theta).max() < THETA_RTOL


def test_gpu_empty_and_degenerate_batches(ctx):
    from strawberry_amd import em, synth
    # empty batch
    b = synth.from_loci([])
    theta, status, iters = em.em_batch_host(b, ctx)
    assert len(theta) == 0 and len(status) == 0
    # a locus with zero rows: init() false (no rows at all), theta0 = 0/niso
    b = synth.LocusBatch(np.array([0, 0, 2], np.int64), np.array([0, 3, 5], np.int64), np.array([0, 0, 4], np.int64),
                         np.array([4, 6], np.int32), np.array([.1, .2, .3, .1]), np.full(5, 1000, np.int32))
    theta, status, iters = em.em_batch_host(b, ctx)
    assert status[0] == 1 and iters[0] == 0 and (theta[:3] == 0).all()
    assert status[1] in (0, 3)


def test_gpu_c2_sample_against_oracle(ctx, oracle):
    """A 2000-locus slice of config C2 (32 bins x 8 isoforms x 1000 fragments)."""
    from strawberry_amd import synth
    b = synth.make_c2(n_loci=2000)
    _, r = solve(b, ctx)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=4)
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    assert theta_err(r["theta"], o_theta).max() < THETA_RTOL


def test_gpu_tiny_denominators_are_not_zero_denominators(ctx, oracle):
    """The tile kernels invert the PRODUCT of up to four row denominators (one v_rcp_f64 for four rows): the product
    of two tiny denominators underflows long before either is zero, and that must not be taken for the reference's
    `denom == 0` (estimate.cpp:451).  Isoform B below loses its reads to A and decays by a factor 5 per iteration;
    bins that fit only B and hold no reads then have denominators 0.4 theta_B: their pairwise product leaves the
    exponent range after ~220 iterations, theta_B itself flushes to zero -- the real zero denominator -- after 326 to
    650, depending on the locus; two nearly equal isoforms C, D keep the EM running that long."""
    from strawberry_amd import synth
    def locus(decay_rows):
        rows, cnt = [[1.0, 0.5, 0, 0], [1.0, 0.0, 0, 0]], [100, 100]
        for _ in range(decay_rows):
            rows.append([0.0, 1.0, 0, 0]); cnt.append(0)
        for k in range(6):
            a = 0.5 + 0.05 * k
            rows.append([0, 0, a, a * (1 + 1e-3 * (k - 2.5))]); cnt.append(50 + k)
        return np.array(cnt, np.int32), np.array(rows)
    # alone, eight to a wave, and with enough rows for several row lanes
    loci = [locus(2), locus(4), locus(1), locus(9), locus(30), locus(70)] + [locus(2 + k % 3) for k in range(40)]
    b = synth.from_loci(loci)
    _, r = solve(b, ctx)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=2)
    assert (o_status == 2).all() and o_iters[:3].min() > 300   # DENOM_ZERO, long after the products underflow
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    assert theta_err(r["theta"], o_theta).max() < THETA_RTOL


@pytest.mark.parametrize("config", ["c2", "c3"])
def test_gpu_full_size_configs_against_oracle(ctx, oracle, config):
    """BASELINE.json's configurations at FULL size -- C2: 10 000 loci x 8 isoforms x 1000 fragments,
    C3: 60 000 loci, 2e8 fragments -- through sbgpu_em_run_device, every locus compared with the
    oracle (a few seconds of CPU on 8 threads): status and iteration counts exact, theta to 1e-9,
    TPM (after the epilogue) to 1e-9 -- the north star asks 1e-4."""
    from strawberry_amd import synth, em
    b = synth.make_c2() if config == "c2" else synth.make_c3()
    assert b.n_loci == (10000 if config == "c2" else 60000)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    s.run_abundance(total_mapped_reads=min(b.n_frags, 2**31 - 1), min_isoform_frac=0.0)
    s.run_tpm()
    r = s.results()
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=8)
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    err = theta_err(r["theta"], o_theta)
    assert err.max() < THETA_RTOL, (config, err.max(), int(err.argmax()))
    o = oracle.abundance(b.iso_off, o_theta, o_status, b.length, total_mapped_reads=min(b.n_frags, 2**31 - 1),
                         min_isoform_frac=0.0)
    tpm_err = np.abs(r["tpm"] - o["tpm"]) / np.maximum(np.abs(o["tpm"]), 1e-6)
    assert tpm_err.max() < 1e-9, (config, tpm_err.max())


def test_gpu_full_size_properties(ctx):
    """BASELINE-size runs checked through size-independent properties: mass
    conservation (sum theta = kept counts after the first iteration), non-negativity,
    determinism (bitwise identical re-run), TPM sums to 1e6."""
    from strawberry_amd import synth, em
    for b in (synth.make_c2(), synth.make_c3(n_loci=20000, total_frags=2e8 / 3)):
        s = em.EmBatchSolver(b, ctx)
        s.run_em()
        r1 = s.results()
        s.run_em()
        s.run_abundance(total_mapped_reads=max(1, b.n_frags), min_isoform_frac=0.0)
        s.run_tpm()
        r2 = s.results()
        np.testing.assert_array_equal(r1["theta"], r2["theta"])
        np.testing.assert_array_equal(r1["iters"], r2["iters"])
        assert (r2["status"] >= 0).all() and (r2["status"] <= 3).all()
        assert (r2["theta"] >= 0).all() and np.isfinite(r2["theta"]).all()
        tot_theta = np.add.reduceat(r2["theta"], b.iso_off[:-1])
        tot_n = np.add.reduceat(b.count.astype(np.float64), b.row_off[:-1])
        ok = np.isin(r2["status"], (0, 3)) & (r2["iters"] > 1)
        # every synthetic row has a weight >= 1e-3, so no row is dropped
        assert np.abs(tot_theta[ok] - tot_n[ok]).max() < 1e-6 * max(1.0, tot_n.max())
        assert abs(r2["tpm"].sum() - 1e6) < 1e-3


def test_gpu_abundance_and_tpm_match_oracle(ctx, oracle, golden):
    from strawberry_amd import em
    b, _, _ = golden("em_c3_400")
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    total_mapped = 3_000_000
    for kw in (dict(min_isoform_frac=0.01), dict(min_isoform_frac=0.0),
               dict(effective_len_norm=True, insert_mean=700.5, min_isoform_frac=0.01)):
        s.run_abundance(total_mapped, **kw)
        s.run_tpm()
        r = s.results()
        fpkm, frac, keep = np.zeros_like(r["theta"]), np.zeros_like(r["theta"]), np.zeros(len(r["theta"]), np.int32)
        for l in range(b.n_loci):
            j0, j1 = b.iso_off[l], b.iso_off[l + 1]
            if r["status"][l] == 1:
                continue
            f, fr, k, _ = oracle.abundance_locus(r["theta"][j0:j1], b.length[j0:j1], total_mapped,
                                                 filter_by_expression=True, **kw)
            fpkm[j0:j1], frac[j0:j1], keep[j0:j1] = f, fr, k
        np.testing.assert_array_equal(r["keep"], keep)
        np.testing.assert_allclose(r["fpkm"], fpkm, rtol=1e-14, atol=0)
        np.testing.assert_allclose(r["frac"], frac, rtol=1e-14, atol=0)
        tpm, tot = oracle.tpm(fpkm, keep)
        assert abs(r["sum_fpkm"] - tot) / tot < 1e-12
        np.testing.assert_allclose(r["tpm"], tpm, rtol=1e-12, atol=0)


def test_wide_kernel_tiny_denominators_are_not_zero_denominators(ctx, oracle):
    """The same on the multi-workgroup kernel for loci of more than 64 isoforms (it checks the product's range
    before it inverts it): rows 2 and 10 -- both bins of the dying isoform -- share a wave's block of four."""
    from strawberry_amd import synth
    def wide_locus(decay_rows, extra=66):
        niso = 4 + extra
        rows, cnt = [], []
        def row(d, n):
            r = np.zeros(niso)
            for k, v in d.items():
                r[k] = v
            rows.append(r); cnt.append(n)
        row({0: 1.0, 1: 0.5}, 100); row({0: 1.0}, 100)
        for _ in range(decay_rows):
            row({1: 1.0}, 0)
        for k in range(6):
            a = 0.5 + 0.05 * k
            row({2: a, 3: a * (1 + 1e-3 * (k - 2.5))}, 50 + k)
        for k in range(extra):
            row({4 + k: 1.0}, 10 + k % 7)
        return np.array(cnt, np.int32), np.array(rows)
    b = synth.from_loci([wide_locus(9), wide_locus(12), wide_locus(40, extra=130)])
    _, r = solve(b, ctx)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=2)
    assert (o_status == 2).all() and o_iters.min() > 150
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    assert theta_err(r["theta"], o_theta).max() < THETA_RTOL


def _experiments_build():
    from strawberry_amd import _lib
    return _lib.load().sbgpu_build_id().decode().endswith("-exp")


def needs_experiments(test):
    """The schedule / phase switches are experiment switches (csrc/api_internal.h: sb::exp_env): the shipped library does not read
    them.  A test that sets them runs its body in a process that loads the EXPERIMENTS build (libsbgpu_exp.so: `make -C
    strawberry_amd/csrc experiments`, part of __graft_entry__.build()): from a process on the shipped library it starts such a
    process on itself and passes with it."""
    import functools
    import subprocess
    import sys

    @functools.wraps(test)
    def wrapper(*args, **kw):
        if _experiments_build():
            return test(*args, **kw)
        lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "strawberry_amd", "lib", "libsbgpu_exp.so")
        if not os.path.exists(lib):
            pytest.fail("the experiments build is missing: make -C strawberry_amd/csrc experiments")
        node = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        r = subprocess.run([sys.executable, "-m", "pytest", node, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"],
                           env=dict(os.environ, SBGPU_LIB=lib), capture_output=True, text=True, timeout=1800,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    return wrapper


@needs_experiments
def test_gpu_phased_execution_matches_oracle(ctx, oracle, monkeypatch):
    """Phases of the wave kind: loci still running at an iteration limit are suspended (theta and the iteration
    count are their whole state) and continue in a later launch with MORE lanes per locus (lane-rich layouts,
    another summation order).  Whatever the limits and lane weights, status and iteration counts stay exact and
    theta within 1e-9 of the oracle; a run with the same settings is bitwise reproducible."""
    from strawberry_amd import em, synth
    b = synth.make_c3(n_loci=6000, total_frags=2e7, seed=11)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=4)
    for spec, lam in (("0", None), ("8", "0"), ("3,17,64,300", "16,4,1,0"), ("64,256", "2,0.25"), ("32,128,512", None),
                      ("1000", None), ("2", "100"), ("8,64", "t,t"), ("16,100,400", "t,1,t"), ("5,50", "0,t")):
        monkeypatch.setenv("SBGPU_PHASES", spec)
        if lam is None:
            monkeypatch.delenv("SBGPU_PHASE_LAMBDA", raising=False)
        else:
            monkeypatch.setenv("SBGPU_PHASE_LAMBDA", lam)
        s1 = em.EmBatchSolver(b, ctx)
        s1.run_em()
        r1 = s1.results()
        np.testing.assert_array_equal(r1["status"], o_status, err_msg=spec)
        np.testing.assert_array_equal(r1["iters"], o_iters, err_msg=spec)
        assert theta_err(r1["theta"], o_theta).max() < THETA_RTOL, spec
        s1.run_em()
        r2 = s1.results()
        np.testing.assert_array_equal(r1["theta"], r2["theta"])
        np.testing.assert_array_equal(r1["iters"], r2["iters"])


@needs_experiments
def test_gpu_lane_rich_layouts_every_shape(ctx, oracle, monkeypatch):
    """Every lane-rich layout (1-4 columns per lane x 1-16 column lanes x 1-8 rows per lane, 1-64 lanes per
    locus) on shapes of its own: a first phase of 2 iterations hands every locus that is still running to the
    later phases' kernel, under three lane weights."""
    from strawberry_amd import em, synth
    rng = np.random.Generator(np.random.PCG64(99))
    loci = []
    for niso in (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 24, 31, 32, 33, 48, 64):
        for nrow in (1, 2, 3, 5, 8, 9, 16, 17, 31, 40, 64, 100, 128, 200, 256, 400, 512):
            if nrow * niso > 2048:
                continue
            F = np.where(rng.random((nrow, niso)) < 0.5, rng.uniform(1e-3, .3, (nrow, niso)), 0.0)
            loci.append((rng.integers(0, 50, nrow).astype(np.int32), F))
    b = synth.from_loci(loci)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=4)
    for lam in ("0", "1", "30"):
        monkeypatch.setenv("SBGPU_PHASES", "2,40")
        monkeypatch.setenv("SBGPU_PHASE_LAMBDA", lam + "," + lam)
        s = em.EmBatchSolver(b, ctx)
        s.run_em()
        r = s.results()
        np.testing.assert_array_equal(r["status"], o_status, err_msg=lam)
        np.testing.assert_array_equal(r["iters"], o_iters, err_msg=lam)
        assert theta_err(r["theta"], o_theta).max() < THETA_RTOL, lam


@needs_experiments
@pytest.mark.parametrize("env", [{"SBGPU_WAVE_RMULT": "1"}, {"SBGPU_WAVE_RMULT": "2"}, {"SBGPU_WAVE_RMULT": "4"},
                                 {"SBGPU_LIGHT_BLOCK": "1"}, {"SBGPU_MAX_WAVES": "64"}])
def test_gpu_every_schedule_gives_the_same_answer(ctx, oracle, monkeypatch, env):
    """Size-class / grid tuning knobs change the schedule, never the result beyond
    summation order (status and iteration counts stay exact)."""
    from strawberry_amd import em, synth
    b = synth.make_c3(n_loci=3000, total_frags=1e7, seed=5)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    r = s.results()
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=4)
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    assert theta_err(r["theta"], o_theta).max() < THETA_RTOL


@pytest.mark.gpu
def test_plan_is_independent_of_host_thread_count(monkeypatch):
    """sbgpu_plan_create classifies and sorts the loci on host threads; the plan (classes, their loci, the
    kernel kind of every locus) and hence the results must not depend on how many."""
    from strawberry_amd import em, synth
    b = synth.make_c3(n_loci=40000)
    ctx = em.default_context(0)
    ref = None
    for nt in ("1", "3", "16"):
        monkeypatch.setenv("SBGPU_HOST_THREADS", nt)
        p = em.Plan(ctx, b.row_off, b.iso_off, b.f_off)
        got = (p.info(), p.classes(), p.locus_kinds().tolist())
        p.close()
        if ref is None:
            ref = got
            assert got[0]["n_classes"] > 50
        else:
            assert got == ref
    monkeypatch.setenv("SBGPU_HOST_THREADS", "16")
    s16 = em.EmBatchSolver(b, ctx)
    s16.run_em()
    r16 = s16.results()
    monkeypatch.setenv("SBGPU_HOST_THREADS", "1")
    s1 = em.EmBatchSolver(b, ctx)
    s1.run_em()
    r1 = s1.results()
    np.testing.assert_array_equal(r1["theta"], r16["theta"])
    np.testing.assert_array_equal(r1["iters"], r16["iters"])


@pytest.mark.gpu
def test_wide_loci_multi_workgroup_kernel(oracle, monkeypatch):
    """Loci with more than 64 isoforms (or more rows than a workgroup's tile) run on the cooperative
    multi-workgroup kernel: several workgroups per locus, one exchange per iteration.  All three template
    widths (<= 128, <= 256, <= 512 isoforms), single- and multi-workgroup loci, next to ordinary loci in the
    same batch; status and iteration counts exact, theta to 1e-9 -- and the same through the streaming
    kernel (SBGPU_NO_WIDE=1), which stays the fallback."""
    from strawberry_amd import em, synth
    from strawberry_amd.synth import _generate
    rng = np.random.Generator(np.random.PCG64(2024))
    niso = np.array([65, 100, 128, 129, 200, 256, 300, 420, 70, 90], np.int64)
    nrow = np.array([40, 700, 1500, 90, 1100, 300, 900, 200, 3, 2500], np.int64)
    wide = _generate(rng, nrow, niso, (nrow * 40).astype(np.int64), name="wide")
    small = synth.make_random(n_loci=200, seed=77)
    loci = [wide.locus(l) for l in range(wide.n_loci)] + [small.locus(l) for l in range(small.n_loci)]
    b = synth.from_loci(loci)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=8)
    ctx = em.default_context(0)
    for no_wide in ("", "1"):
        if no_wide:
            monkeypatch.setenv("SBGPU_NO_WIDE", "1")
        else:
            monkeypatch.delenv("SBGPU_NO_WIDE", raising=False)
        s = em.EmBatchSolver(b, ctx)
        kinds = s.plan.locus_kinds()
        assert (kinds[:10] == 5).all()
        # kind 5 is "wide or stream": the route itself is the count of wide loci (the fallback leg has none)
        info = s.plan.info()
        assert info["n_stream_loci"] == 10 and info["n_wide_loci"] == (0 if no_wide else 10), (no_wide, info)
        s.run_em()
        r = s.results()
        np.testing.assert_array_equal(r["status"], o_status)
        np.testing.assert_array_equal(r["iters"], o_iters)
        err = np.abs(r["theta"] - o_theta) / np.maximum(np.abs(o_theta), 1e-9)
        assert err.max() < 1e-9, (no_wide, err.max())
    assert o_iters[:10].max() > 100


def test_c3t_tail_every_wide_locus_against_oracle(oracle):
    """The tail of bench.py's C3-T workload at full size -- 300 loci of 65..400 isoforms and 200..3000 bins, all of them
    on em_wide_kernel, about twenty cooperative rounds -- locus by locus against the oracle (it takes the CPU a few
    seconds on the GPU box's cores): status and iteration counts exact, theta to 1e-9."""
    import os
    from strawberry_amd import em, synth
    b = synth.make_c3t(n_loci=300, total_frags=1e6, n_tail=300)
    assert b.n_loci == 600
    threads = max(4, min(32, os.cpu_count() or 4))
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=threads)
    ctx = em.default_context(0)
    s = em.EmBatchSolver(b, ctx)
    assert (s.plan.locus_kinds() == 5).sum() == 300
    s.run_em()
    r = s.results()
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    err = np.abs(r["theta"] - o_theta) / np.maximum(np.abs(o_theta), 1e-9)
    assert err.max() < 1e-9, err.max()


def test_gpu_fp32_variant_is_close_and_leaves_fp64_untouched(ctx, oracle):
    """BASELINE config 5: the fp32 instantiation of the tile kernels (sbgpu_em_run_device_f32).  Not a parity path
    -- it is compared loosely (most loci keep their status, theta within 1e-3 of a fragment-floor relative error
    where both converged) -- and running it must not disturb the fp64 path: same plan, bitwise the same fp64 answer
    before and after, and that answer still matches the oracle."""
    from strawberry_amd import em, synth
    b = synth.make_c5(n_loci=4000, total_frags=4e8 / 15)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    r64 = s.results()
    s.run_em_f32()
    s.synchronize()
    th32 = s.d_theta32[:s.n_iso].cpu().numpy().astype(np.float64)
    st32 = s.d_status[:b.n_loci].cpu().numpy()
    it32 = s.d_iters[:b.n_loci].cpu().numpy()
    s.run_em()
    r64b = s.results()
    np.testing.assert_array_equal(r64["theta"], r64b["theta"])
    np.testing.assert_array_equal(r64["iters"], r64b["iters"])
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=4)
    np.testing.assert_array_equal(r64["status"], o_status)
    np.testing.assert_array_equal(r64["iters"], o_iters)
    assert theta_err(r64["theta"], o_theta).max() < THETA_RTOL
    # the fp32 answers: sane and close
    assert ((st32 >= 0) & (st32 <= 3)).all() and np.isfinite(th32).all() and (th32 >= 0).all()
    assert (st32 == r64["status"]).mean() > 0.97
    same = (st32 == 0) & (r64["status"] == 0) & (np.abs(it32 - r64["iters"]) <= 1)
    m = same[np.repeat(np.arange(b.n_loci), b.niso)]
    rel = np.abs(th32 - r64["theta"])[m] / np.maximum(r64["theta"][m], 1.0)
    assert same.mean() > 0.8 and np.percentile(rel, 99) < 1e-3, (same.mean(), np.percentile(rel, 99))


def test_bench_dump_outputs_are_the_timed_steps_results(oracle, tmp_path):
    """`bench.py --dump-outputs DIR` writes what the timed steps computed: on C2 (bench's batch, seed 0x5742) theta, status and
    iteration counts are the oracle's, and the epilogue's outputs come with them, all float64."""
    import json
    import subprocess
    import sys
    from strawberry_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c2", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert set(got) == {"theta", "status", "iters", "fpkm", "frac", "keep", "tpm", "sum_fpkm"}
    assert all(a.dtype == np.float64 for a in got.values())
    b = synth.make_c2(seed=0x5742)
    theta, status, iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    np.testing.assert_array_equal(got["status"], status)
    np.testing.assert_array_equal(got["iters"], iters)
    assert theta_err(got["theta"], theta).max() < THETA_RTOL
    assert got["tpm"].size == theta.size and abs(got["tpm"].sum() - 1e6) < 1e-3


def test_bench_plain_line_is_the_headline_and_full_adds_the_rest():
    """A plain `bench.py` run times the headline alone -- its line has the headline's fields and nothing measured beside
    them; `--full` adds the per-kernel times, the roofline and the steps one after the other, and the CPU parity where asked."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def line(*args):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c2", "--steps", "12", "--warmup", "2", *args],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    plain = line()
    assert plain["full"] is False and plain["steps"] == 12 and plain["warmup"] == 2 and plain["n_gpus"] == 1
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "loci/s" and plain["dtype"] == "f64"
    assert plain["higher_is_better"] is True and plain["config"]["loci_per_gpu"] == 10000
    assert not {"roofline", "cpu_baseline", "parity", "weak_scaling", "strong_scaling", "em_status", "chain", "front"} & set(plain)
    full = line("--full")
    assert full["full"] is True and full["metric"] == plain["metric"] and full["config"]["steps_pipelined"] == plain["config"]["steps_pipelined"]
    assert full["roofline"]["kernel_ms"] > 0 and full["config"]["ms_per_step_one_after_the_other"] > 0
    assert full["parity"]["ok"] and full["parity"]["checked_loci"] == 10000
