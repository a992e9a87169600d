"""GPU parity of the block form's per-row-count steady loop (em_device.h: with_rows).  A block-form locus uses RU of the
R rows a lane's register tile holds, RU = ceil(rows / row lanes); for the 4- and 6-row tiles (5-8 columns per lane) the
kernel runs a loop compiled for exactly RU rows, and the reciprocal batches group RU denominators.  Every (layout, RU)
instantiation at the first row count that needs RU rows and at the last one RU rows still hold, then the per-locus events
inside a locus with RU < R (rows the 1e-5 filter drops, zero denominators early and late, products of denominators that
underflow, an init-empty locus, the 1000-iteration cap), the split (pipelined) entry and the bias entry -- against the
oracle: status and iteration counts exact, theta within 1e-9 relative, every locus compared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
THETA_FLOOR = 1e-9
KIND_BLOCK = 3          # plan.h: ClassKind::kBlock
LOCI_PER_SHAPE = 3

# isoforms -> row counts.  The wave kind holds 64 lanes x R rows; beyond it the 256-lane block form takes over with
# 256 / CL row lanes (CL = 1, 2, 4, 8 column lanes for up to 8, 16, 32, 64 isoforms):
#    8 isoforms (8 x 1, R 4, 256 row lanes): RU 2 = 257..512, RU 3 = 513..768, RU 4 = 769..1024
#    5 isoforms (5 x 1, R 6, 256 row lanes): RU 2 = 385..512, RU 3 .. RU 6 = ..768, ..1024, ..1280, ..1536
#   16 isoforms (8 x 2, R 4, 128 row lanes): RU 2 = 129..256, RU 3 = 257..384, RU 4 = 385..512
#   22 isoforms (6 x 4, R 6,  64 row lanes): RU 2 = 97..128, RU 3 = 129..192, RU 4 .. RU 6 = ..256, ..320, ..384
#   64 isoforms (8 x 8, R 4,  32 row lanes): RU 2 = 33..64, RU 3 = 65..96, RU 4 = 97..128
SHAPES = {
    8: [257, 512, 513, 768, 769, 1024],
    5: [385, 512, 513, 768, 769, 1025, 1281, 1536],
    16: [129, 256, 257, 385, 512],
    22: [97, 128, 129, 193, 257, 321, 384],
    64: [33, 64, 65, 97, 128],
}
CASES = [(niso, nrow) for niso, rows in SHAPES.items() for nrow in rows]
# (niso, nrow) -> seed offset, for a case whose seed puts a locus so close to the threshold that the oracle's own
# iteration count moves under a one-ulp change of F.  Checked on the CPU -- every batch of this file solved by the oracle
# with each weight moved to a neighbouring double at random, four times: no count moved, no seed replaced.
SEED_BUMP = {}


def column_lanes(niso):
    return 1 if niso <= 8 else 2 if niso <= 16 else 4 if niso <= 32 else 8


def rows_used(niso, nrow):
    gr = 256 // column_lanes(niso)
    return (nrow + gr - 1) // gr


def tile_rows(niso):
    cpl = -(-niso // column_lanes(niso))
    return 6 if cpl <= 6 else 4


def theta_err(theta, ref):
    return np.abs(theta - ref) / np.maximum(np.abs(ref), THETA_FLOOR)


def random_locus(rng, nrow, niso):
    # test_em_gpu.py::test_gpu_every_size_class's draw
    F = np.where(rng.random((nrow, niso)) < 0.5, rng.uniform(1e-3, .3, (nrow, niso)), 0.0)
    return rng.integers(0, 50, nrow).astype(np.int32), F


def shape_batch(niso, nrow):
    from strawberry_amd import synth
    rng = np.random.Generator(np.random.PCG64(niso * 100000 + nrow + SEED_BUMP.get((niso, nrow), 0)))
    return synth.from_loci([random_locus(rng, nrow, niso) for _ in range(LOCI_PER_SHAPE)])


def solve_and_compare(ctx, oracle, b, F_oracle=None, solver_setup=None):
    """Solves b on the device and compares EVERY locus with the oracle; returns (solver, results, oracle's answer)."""
    from strawberry_amd import em
    s = em.EmBatchSolver(b, ctx)
    assert (s.plan.locus_kinds() == KIND_BLOCK).all(), s.plan.locus_kinds()
    if solver_setup:
        solver_setup(s)
    s.run_em()
    r = s.results()
    o = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F if F_oracle is None else F_oracle, threads=2)
    compare(r, o)
    return s, r, o


def compare(r, o):
    o_theta, o_status, o_iters = o
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    err = theta_err(r["theta"], o_theta)
    assert len(err) == len(o_theta) and err.max() < THETA_RTOL, (err.max(), int(err.argmax()))


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.mark.parametrize("niso,nrow", CASES)
def test_block_rows_every_instantiation(ctx, oracle, niso, nrow):
    assert 2 <= rows_used(niso, nrow) <= tile_rows(niso)
    solve_and_compare(ctx, oracle, shape_batch(niso, nrow))


# ---------------------------------------------------------------- per-locus events, in loci with RU < R
# (isoforms, rows): 8 x 1, R 4, RU 3 and 6 x 4, R 6, RU 5
EVENT_LAYOUTS = [(8, 600), (22, 280)]


def decay_locus(niso, nrow, b0, n_decay, w_decay, cd_scale):
    """test_em_gpu.py's tiny denominators at a block-form size.  Isoform A = 0 takes the reads of the bin it shares with
    B = niso - 1; B's weight there is b0 and B owns n_decay bins of weight w_decay that hold no reads, so after the
    column normalisation theta_B shrinks by b0 / (b0 + n_decay w_decay) per iteration and the denominators of those
    bins, w' theta_B, with it.  The decay bins are rows 2 .. 2 + n_decay: more than the tile has row lanes, so some
    lane holds two of them and multiplies their denominators in one reciprocal batch.  C = 1 and D = 2, nearly equal
    (counts scaled by cd_scale: the threshold on theta's step is absolute), keep the EM running; the other isoforms
    have bins of their own up to nrow rows."""
    a, c, d, b = 0, 1, 2, niso - 1
    F = np.zeros((nrow, niso))
    cnt = np.zeros(nrow, np.int32)
    F[0, a], F[0, b], cnt[0] = 1.0, b0, 100
    F[1, a], cnt[1] = 1.0, 100
    F[2:2 + n_decay, b] = w_decay
    i = 2 + n_decay
    for k in range(6):
        x = 0.5 + 0.05 * k
        F[i, c], F[i, d], cnt[i] = x, x * (1 + 1e-3 * (k - 2.5)), (50 + k) * cd_scale
        i += 1
    others = [j for j in range(niso) if j not in (a, b, c, d)]
    for k in range(i, nrow):
        j = others[k % len(others)]
        F[k, j], cnt[k] = 1.0, 20 + k % 7
        F[k, others[(k + 1 + k // len(others)) % len(others)]] += 0.25
    return cnt, F


def event_batch(niso, nrow):
    """name -> locus; all of one shape (nrow x niso)."""
    rng = np.random.Generator(np.random.PCG64(7000 + niso))
    gr = 256 // column_lanes(niso)
    loci = {}
    # rows the 1e-5 filter drops: only a few rows of the first slot kept (fewer kept rows than rows per lane, most
    # lanes hold none), a random 70 %, and all of the second slot (rows gr .. 2 gr - 1)
    cnt, F = random_locus(rng, nrow, niso)
    F[gr // 2:] *= 1e-6
    loci["drop_all_but_half_a_slot"] = (cnt, F)
    cnt, F = random_locus(rng, nrow, niso)
    F[rng.random(nrow) < 0.7] = 0.0
    loci["drop_random"] = (cnt, F)
    cnt, F = random_locus(rng, nrow, niso)
    F[gr:2 * gr] *= 1e-6
    loci["drop_second_slot"] = (cnt, F)
    # zero denominators of kept rows: every count zero (theta0 = 0: at the first iteration), and theta_B flushed to
    # zero after a decay by 5 per iteration (late: theta0 survives)
    cnt, F = random_locus(rng, nrow, niso)
    F[0, :] = 0.2
    loci["denominator_zero_first"] = (np.zeros(nrow, np.int32), F)
    loci["denominator_zero_late"] = decay_locus(niso, nrow, 0.5, gr + 44, 2.0 / (gr + 44), 40)
    # products of denominators that underflow while no denominator is zero: decay by 0.6 per iteration, theta_B is
    # ~1e-220 at the 1000th iteration (no zero), the product of two such denominators leaves the range after ~690
    loci["product_underflow"] = decay_locus(niso, nrow, 0.6, gr + 44, 0.4 / (gr + 44), 40)
    # init() == false: no weight above 1e-5
    cnt, F = random_locus(rng, nrow, niso)
    loci["init_empty"] = (cnt, F * 1e-5)
    # the 1000-iteration cap with every denominator and product in range: decay by 0.9 (theta_B ~1e-46 at the end)
    loci["iteration_cap"] = decay_locus(niso, nrow, 0.9, gr + 44, 0.1 / (gr + 44), 40)
    loci["plain"] = random_locus(rng, nrow, niso)
    return loci


@pytest.mark.parametrize("niso,nrow", EVENT_LAYOUTS)
def test_block_rows_events(ctx, oracle, niso, nrow):
    from strawberry_amd import synth
    assert rows_used(niso, nrow) < tile_rows(niso)
    loci = event_batch(niso, nrow)
    names = list(loci)
    b = synth.from_loci([loci[n] for n in names])
    _, r, (o_theta, o_status, o_iters) = solve_and_compare(ctx, oracle, b)
    st = dict(zip(names, o_status))
    it = dict(zip(names, o_iters))
    # the batch holds what it is meant to
    for n in ("drop_all_but_half_a_slot", "drop_random", "drop_second_slot", "plain"):
        assert st[n] in (0, 3) and it[n] > 1, (n, st[n], it[n])
    assert st["denominator_zero_first"] == 2 and it["denominator_zero_first"] == 1
    assert st["denominator_zero_late"] == 2 and it["denominator_zero_late"] > 100
    k = names.index("denominator_zero_late")
    th = r["theta"][b.iso_off[k]:b.iso_off[k + 1]]
    assert (th == th[0]).all() and th[0] > 0                     # theta0 survives
    k = names.index("product_underflow")
    th_b = o_theta[b.iso_off[k + 1] - 1]
    # theta_B is not zero, and below 1e-160 the product of two denominators w' theta_B (w' < 1) is below the smallest
    # normal double: flushed to zero in the batch, so the kernel's re-run with a division per row decided this locus
    assert st["product_underflow"] != 2 and 0 < th_b < 1e-160, (st["product_underflow"], th_b)
    assert st["init_empty"] == 1 and it["init_empty"] == 0
    assert st["iteration_cap"] == 3 and it["iteration_cap"] == 1000


# ---------------------------------------------------------------- schedules
def mixed_batch():
    """Every layout of the table at a few of its row counts, all block-form."""
    from strawberry_amd import synth
    rng = np.random.Generator(np.random.PCG64(99))
    loci = []
    for niso, rows in SHAPES.items():
        for nrow in rows[::2]:
            loci.append(random_locus(rng, nrow, niso))
    return synth.from_loci(loci)


def test_block_rows_split_entry_twice(ctx, oracle):
    """The split entry (what a pipelined bench step uses), two steps back to back: each step's outputs are the unsplit
    run's, byte for byte, and the unsplit run's are the oracle's."""
    import torch
    from strawberry_amd import dist, em
    b = mixed_batch()
    _, want, _ = solve_and_compare(ctx, oracle, b)
    s = em.EmBatchSolver(b, ctx)
    q = dist.ShardQuantifier(s, 10 ** 7, pipelined=True)
    assert q.pipelined
    snaps = []

    def observe():
        snaps.append({k: getattr(s, "d_" + k)[:n].clone() for k, n in (("theta", s.n_iso), ("status", b.n_loci),
                                                                       ("iters", b.n_loci))})
    q.step(observe=observe)
    q.step(observe=observe)
    q.finish()
    torch.cuda.synchronize()
    assert len(snaps) == 2
    for snap in snaps:
        for name, t in snap.items():
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(want[name]).tobytes(), name


def test_block_rows_bias_entry(ctx, oracle):
    """The bias arrays set (BASELINE config 5): the tile is loaded as F_ij 2^(row_bias_i iso_bias_j).  Factors in
    {-1, 0, 1}: the exponent is an integer and the factor an exact power of two on the device and in numpy alike, so
    the oracle on the pre-multiplied weights is the reference for every locus, counts included."""
    import torch
    b = mixed_batch()
    rng = np.random.default_rng(5)
    row_bias = rng.integers(-1, 2, int(b.row_off[-1])).astype(np.float64)
    iso_bias = rng.integers(-1, 2, int(b.iso_off[-1])).astype(np.float64)
    Fb = b.F.copy()
    for l in range(b.n_loci):
        r0, r1, j0, j1 = b.row_off[l], b.row_off[l + 1], b.iso_off[l], b.iso_off[l + 1]
        Fb[b.f_off[l]:b.f_off[l + 1]] *= np.exp2(np.outer(row_bias[r0:r1], iso_bias[j0:j1])).reshape(-1)
    assert not np.array_equal(Fb, b.F)

    def setup(s):
        s.set_bias(torch.from_numpy(row_bias).to(s.dev), torch.from_numpy(iso_bias).to(s.dev))
    solve_and_compare(ctx, oracle, b, F_oracle=Fb, solver_setup=setup)
