"""The yardstick of the fp32 EM kernels (tests/em_f32_util.py) checked on the CPU: the EM by hand is the oracle's EM, the three
fp32 emulations agree among themselves on nearly every locus of the GPU tests' inputs, and the comparison rule rejects two
planted errors of the kinds it is there to catch."""
import numpy as np
import pytest

import em_f32_util as FU


@pytest.mark.parametrize("name", ["em_edge", "em_random_256"])
def test_by_hand_fp64_reproduces_the_oracle(oracle, golden, name):
    b, _, _ = golden(name)
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    theta, status, iters = FU.em_batch_by_hand(b, dtype=np.float64, order="pair")
    np.testing.assert_array_equal(status, o_status)
    np.testing.assert_array_equal(iters, o_iters)
    err = np.abs(theta - o_theta) / np.maximum(np.abs(o_theta), 1e-9)
    assert err.max() < 1e-9, (name, err.max(), int(err.argmax()))


def test_row_counts_cover_every_layout_and_group_size():
    """the restated planner limits: twenty layouts, the largest locus 24576 x 1, the widest 512 x 64"""
    layouts = {FU.layout_for(n) for n in FU.NISO}
    assert layouts == {(c, 1) for c in range(1, 9)} | {(c, cl) for c in range(5, 9) for cl in (2, 4, 8)}
    assert set(range(1, 65)) == {n for n in range(1, 65) if FU.layout_for(n) in layouts}
    shapes = [(nrow, niso) for niso in FU.NISO for nrow, _ in FU.row_counts(niso)]
    assert max(shapes) == (24576, 1) and max(nrow for nrow, niso in shapes if niso == 64) == 512
    for niso in FU.NISO:
        cpl, cl = FU.layout_for(niso)
        assert len(FU.expected_classes(niso)) == 2 + (64 // cl).bit_length()


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("niso", FU.NISO)
def test_emulations_leave_few_loci_out(oracle, niso, bias):
    """The three fp32 emulations taken as the device's answer in turn: each passes the rule, and the loci left out (where the
    emulations themselves disagree with the fp64 oracle on status, or on the iteration count by more than 1) stay within 5 %."""
    c = FU.param_case(niso, bias)
    ref = FU.oracle_for(oracle, niso, bias)
    for order, emu in zip(FU.ORDERS, c["emulations"]):
        r = FU.compare_f32(*emu, c["batch"], ref, c["emulations"])
        assert r["worst_ratio"] <= 0.25 + 1e-12      # an emulation is within S_l by construction
    j = FU.judge_f32(*c["emulations"][0], c["batch"], ref, c["emulations"])
    print("niso %d %s: left out %s, loci drawn again %d, worst S_l / total count %.2e" % (
        niso, "bias" if bias else "plain", r["left_out"], sum(d > 1 for d in c["draws"]),
        (j["S"] / np.maximum(np.add.reduceat(c["batch"].count.astype(np.float64), c["batch"].row_off[:-1]), 1.0)).max()))


@pytest.fixture(scope="module")
def planted(oracle):
    """Two wrong fp32 EMs over the whole input set (no bias): the last live row that has reads left out of the M-step's
    column sums; the stopping threshold 2e-2 -> per parameter (case, oracle result, dropped-row answer, threshold answer)"""
    out = []
    for niso in FU.NISO:
        c = FU.param_case(niso, False)
        out.append((c, FU.oracle_for(oracle, niso, False),
                    FU.em_batch_by_hand(c["batch"], c["F32"], np.float32, "pair", drop_last_row=True),
                    FU.em_batch_by_hand(c["batch"], c["F32"], np.float32, "pair", limit=2e-2)))
    return out


def _whole(planted, k):
    """the parameters' batches, oracle results, emulations and the k-th planted answer as one batch"""
    from strawberry_amd import synth
    cat = lambda results: tuple(np.concatenate([r[i] for r in results]) for i in range(3))   # noqa: E731
    batch = synth.concat_batches([p[0]["batch"] for p in planted])
    emus = [cat([p[0]["emulations"][e] for p in planted]) for e in range(3)]
    return cat([p[k] for p in planted]), batch, cat([p[1] for p in planted]), emus


def test_a_dropped_row_is_rejected(planted):
    got, batch, ref, emus = _whole(planted, 2)
    with pytest.raises(AssertionError):
        FU.compare_f32(*got, batch, ref, emus)
    j = FU.judge_f32(*got, batch, ref, emus)
    judged = ~j["left_out"] & (batch.nrow > 1)
    missed = np.flatnonzero(judged & ~FU.rejected_f32(j))
    print("dropped row: caught on %d of %d loci of more than one row" % (judged.sum() - len(missed), judged.sum()))
    assert len(missed) == 0, [(int(batch.nrow[l]), int(batch.niso[l]), j["err"][l], j["tol"][l]) for l in missed]


def test_a_doubled_threshold_is_rejected(planted):
    got, batch, ref, emus = _whole(planted, 3)
    with pytest.raises(AssertionError):
        FU.compare_f32(*got, batch, ref, emus)
    j = FU.judge_f32(*got, batch, ref, emus)
    print("doubled threshold: caught on %d of %d loci" % (FU.rejected_f32(j).sum(), (~j["left_out"]).sum()))
