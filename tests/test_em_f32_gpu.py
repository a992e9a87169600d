"""The fp32 EM kernels (sbgpu_em_run_device_f32, sbgpu_em_run_device_bias_f32; csrc/em_kernels_f32.hip) per layout, kind and
group size, against the fp64 oracle under the tolerance three fp32 emulations set (tests/em_f32_util.py: compare_f32), and the
planner's switch from the base tile to the double tile of the wave kind in the shipped library, for both types.

A parameter is one isoform count -- one (CPL, CL) layout -- with one locus per row count of em_f32_util.row_counts: every
group size of the wave kind at full tiles, a single row, and both ends of the block and the tall block kind."""
import numpy as np
import pytest

import em_f32_util as FU

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
THETA_FLOOR = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def _poison(s):
    """nothing of an earlier run may pass for this one's answer"""
    s.d_status.fill_(-1)
    s.d_iters.fill_(-1)
    if getattr(s, "d_theta32", None) is not None:
        s.d_theta32.fill_(float("nan"))
    s.d_theta.fill_(float("nan"))


def _run_f32(s):
    _poison(s)
    s.run_em_f32()
    s.synchronize()
    s.torch.cuda.synchronize(s.dev)
    n = s.batch.n_loci
    return (s.d_theta32[:s.n_iso].cpu().numpy(), s.d_status[:n].cpu().numpy(), s.d_iters[:n].cpu().numpy())


def _run_f64(s):
    _poison(s)
    s.run_em()
    r = s.results()
    return r["theta"], r["status"], r["iters"]


def _assert_is_the_oracles(got, ref):
    np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[2], ref[2])
    err = np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), THETA_FLOOR)
    assert err.max() < THETA_RTOL, (err.max(), int(err.argmax()))


_runs = {}


def device_run(ctx, niso):
    """What the device makes of a parameter, once per process: the plan, an fp64 run, the fp32 run, the fp32 run with bias
    factors, and an fp64 run after them -- one solver, as a caller would use it."""
    if niso not in _runs:
        import torch
        from strawberry_amd import em
        c = FU.param_case(niso, True)
        s = em.EmBatchSolver(c["batch"], ctx)
        out = {"kinds": s.plan.locus_kinds().tolist(), "classes": s.plan.classes()}
        out["f64_before"] = _run_f64(s)
        out["f32"] = _run_f32(s)
        s.set_bias(torch.from_numpy(c["row_bias"].astype(np.float64)).to(s.dev), torch.from_numpy(c["iso_bias"].astype(np.float64)).to(s.dev))
        assert (s.d_row_bias32.cpu().numpy() == c["row_bias"]).all() and (s.d_iso_bias32.cpu().numpy() == c["iso_bias"]).all()
        out["f32_bias"] = _run_f32(s)
        s.set_bias(None, None)
        out["f64_after"] = _run_f64(s)
        _runs[niso] = out
    return _runs[niso]


def _report(what, batch, r):
    l = r["worst_locus"]
    print("fp32 EM %s: worst |theta - theta64| / T %.4f at locus %d (%d x %d), worst iteration difference %d, left out %s" % (
        what, r["worst_ratio"], l, batch.nrow[l], batch.niso[l], r["worst_iter_diff"], r["left_out"]))


@pytest.mark.parametrize("niso", FU.NISO)
def test_every_locus_lands_in_its_kind_and_class(ctx, niso):
    """A later change of the planner's limits fails here instead of thinning the coverage of the tests below."""
    run = device_run(ctx, niso)
    assert run["kinds"] == [kind for _, kind in FU.row_counts(niso)]
    assert {(c["kind"], c["C"], c["R"], c["G"]) for c in run["classes"]} == FU.expected_classes(niso)
    assert sum(c["n_loci"] for c in run["classes"]) == len(FU.row_counts(niso))


@pytest.mark.parametrize("niso", FU.NISO)
def test_f32_against_the_oracle(ctx, oracle, niso):
    c = FU.param_case(niso, False)
    theta, status, iters = device_run(ctx, niso)["f32"]
    assert theta.dtype == np.float32
    _report("niso %d" % niso, c["batch"], FU.compare_f32(theta.astype(np.float64), status, iters, c["batch"],
                                                         FU.oracle_for(oracle, niso, False), c["emulations"]))


@pytest.mark.parametrize("niso", FU.NISO)
def test_f32_with_bias_against_the_oracle(ctx, oracle, niso):
    """the emulations take F32 * exp2(outer(rb, ib)) formed in float32, the oracle the float64 product of the same values"""
    c = FU.param_case(niso, True)
    theta, status, iters = device_run(ctx, niso)["f32_bias"]
    _report("niso %d with bias" % niso, c["batch"], FU.compare_f32(theta.astype(np.float64), status, iters, c["batch"],
                                                                   FU.oracle_for(oracle, niso, True), c["emulations"]))
    plain = device_run(ctx, niso)["f32"][0]
    assert niso == 1 or np.abs(theta - plain).max() > 1e-2     # the factors are not a no-op (one isoform: theta is the count)


@pytest.mark.parametrize("niso", FU.NISO)
def test_fp64_is_untouched_by_the_f32_runs(ctx, oracle, niso):
    run = device_run(ctx, niso)
    for before, after in zip(run["f64_before"], run["f64_after"]):
        assert before.tobytes() == after.tobytes()
    _assert_is_the_oracles(run["f64_before"], FU.oracle_for(oracle, niso, False))


def test_f32_declines_a_batch_with_a_wide_locus(ctx):
    """a locus of 65 isoforms streams: the fp32 entry returns SBGPU_EUNSUPPORTED before it touches anything"""
    import torch
    from strawberry_amd import _lib, em, synth
    rng = np.random.Generator(np.random.PCG64(65))
    b = synth.from_loci([FU.make_locus(rng, 20, 8), FU.make_locus(rng, 40, 65), FU.make_locus(rng, 9, 3)])
    s = em.EmBatchSolver(b, ctx)
    assert s.plan.locus_kinds().tolist() == [FU.KIND_WAVE_BASE, FU.KIND_STREAM, FU.KIND_WAVE_BASE]
    s.d_F32 = s.d_F.to(torch.float32)
    s.d_theta32 = torch.full((s.n_iso,), -7.0, dtype=torch.float32, device=s.dev)
    with pytest.raises(em.SbgpuError) as e:
        s.run_em_f32()
    assert "(%d)" % _lib.SBGPU_EUNSUPPORTED in str(e.value)
    assert "sbgpu_em_run_device_f32: the fp32 variant covers loci of up to 64 isoforms in the tile kernels only" in str(e.value)
    torch.cuda.synchronize(s.dev)
    assert (s.d_theta32.cpu().numpy() == -7.0).all()
    assert (s.d_status.cpu().numpy() == -1).all()


def test_double_tile_switch_in_the_shipped_library(ctx, oracle):
    """plan.cpp takes the double tile (kind 2) for the wave kind when the batch would occupy more than 16 * n_cu * 256 lanes at
    the base tile.  One locus per layout of 64 lanes at the base tile, repeated: one repeat below the limit every locus is of
    kind 1, at the limit's first excess every locus is of kind 2 -- em_fused_kernel<0,4,double> and <0,4,float>.  On both sides
    every repeat has the first copy's bits, and the first copy is the oracle's (fp64) or passes compare_f32 (fp32)."""
    import torch
    from strawberry_amd import em
    c = FU.switch_case()
    base = c["batch"]
    for l in range(base.n_loci):   # 64 lanes at the base tile, 32 at the double tile (restated)
        cpl, cl = FU.layout_for(int(base.niso[l]))
        assert -(-int(base.nrow[l]) // FU.tile_rows(cpl, 2)) * cl == 64 and -(-int(base.nrow[l]) // FU.tile_rows(cpl, 4)) * cl == 32
    limit = 16 * ctx.device_info()["cus"] * 256
    reps = limit // (64 * base.n_loci) + 1
    ref = oracle.em_batch(base.row_off, base.iso_off, base.f_off, base.count, c["F64"])
    k, n = int(base.iso_off[-1]), base.n_loci
    for r, kind in ((reps - 1, FU.KIND_WAVE_BASE), (reps, FU.KIND_WAVE_DOUBLE)):
        s = em.EmBatchSolver(FU.tile_batch(base, r), ctx)
        assert (s.plan.locus_kinds() == kind).all(), (r, kind)
        for run, what in ((_run_f64, "fp64"), (_run_f32, "fp32")):
            theta, status, iters = run(s)
            for a, w in ((theta, k), (status, n), (iters, n)):
                a = a.reshape(r, w)
                assert a.tobytes() == np.broadcast_to(a[:1], a.shape).tobytes(), (what, kind)
            if what == "fp64":
                _assert_is_the_oracles((theta[:k], status[:n], iters[:n]), ref)
            else:
                _report("tile switch, %d repeats, wave kind %d" % (r, kind), base,
                        FU.compare_f32(theta[:k].astype(np.float64), status[:n], iters[:n], base, ref, c["emulations"]))
        del s
        torch.cuda.empty_cache()
