"""GPU tests of binweight_kernel (csrc/binweight_device.h) where the sweeps of test_binweight_gpu.py compare `0 == 0`:
effective lengths at 1..32 segments, integer-exact, through a one-point density; weights at 5..32 segments under a Gaussian
and an empirical law; a tiny density strictly inside the support (pdf_support[4], the flushing loop for every pair of the
launch); and the batch loop -- pair counts around 64, position independence inside a batch, out_index, long_read with empty
pairs, more than two passes of the grid.  The samples and their CPU references come from tests/binweight_util.py
(tests/test_binweight_util.py asserts the samples' own conditions on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import binweight_util as U
from test_binweight_gpu import check

pytestmark = pytest.mark.gpu

RTOL = 1e-12   # at most N <= 2000 non-negative terms: either summation order is within (N + 4) 2^-53 of the exact sum, the
#                two sides within 2 (N + 4) 2^-53 < 4.5e-13 of each other (the terms themselves agree: bw_div's quotient by a
#                small integer is the correctly rounded one, <= 1 ulp in a vanishing fraction of cases)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


class DevicePairs:
    """A pair list on the device, and launches of sbgpu_binweight_device over it (or over its first n pairs)."""

    def __init__(self, ctx, segs, imps, lens=None, allow_empty=False):
        import torch
        from strawberry_amd.binweight import pack_pairs
        self.ctx, self.torch, self.dev = ctx, torch, torch.device("cuda", 0)
        seg_off, seg_lens, mask = pack_pairs(segs, imps)
        assert allow_empty or (np.diff(seg_off) >= 1).all()
        assert (np.diff(seg_off) <= 32).all()
        self.n = len(segs)
        self.lmax = int(max([int(np.sum(s)) for s in segs] + [0]))
        self.d_off = self.put(seg_off, np.int64)
        self.d_seg = self.put(np.concatenate([seg_lens, [0]]).astype(np.uint32).view(np.int32), np.int32)
        self.d_mask = self.put(mask.view(np.int32), np.int32)
        self.d_len = self.put(np.zeros(self.n) if lens is None else lens, np.int32)

    def put(self, a, dt):
        return self.torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)

    def launch(self, d_pdf, pdf_len, rl, lmin_base, d_out, n=None, d_idx=None, long_read=0):
        from strawberry_amd import _lib
        assert long_read or pdf_len > self.lmax  # the table covers every fragment length of every pair
        _lib.check(self.ctx.L.sbgpu_binweight_device(
            self.ctx.h, self.n if n is None else n, self.d_off.data_ptr(), self.d_seg.data_ptr(), self.d_mask.data_ptr(),
            self.d_len.data_ptr(), d_idx.data_ptr() if d_idx is not None else None, d_pdf.data_ptr() if d_pdf is not None else None,
            pdf_len, rl, lmin_base, long_read, d_out.data_ptr(), C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)),
            "sbgpu_binweight_device")

    def weights(self, table, rl, lmin_base, n=None):
        d_pdf = self.put(table, np.float64)
        m = self.n if n is None else n
        out = self.torch.full((m,), SENTINEL, dtype=self.torch.float64, device=self.dev)
        self.launch(d_pdf, len(table), rl, lmin_base, out, n=n)
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def exact(oracle):
    U.exact_conditions(oracle)
    return U.exact_reference(oracle)[0]


@pytest.mark.parametrize("rl", U.EXACT_RLS)
def test_effective_len_is_exact_at_1_to_32_segments(ctx, exact, rl):
    """pdf[fl0] = 1 and nothing else, iso_len = fl0 for every pair: the denominator is 1, the wave sum has one non-zero
    term, and a pair's weight IS effective_len(fl0) as a double -- or 0 where fl0 lies outside its [max(rl, inner), lmax].
    One launch per fl0 from 1 to the largest lmax, over the whole pair list; equal to the oracle's scan entry by entry."""
    import torch
    segs, imps = U.exact_sample()
    E = exact[rl]
    dp = DevicePairs(ctx, segs, imps)
    n_fl = E.shape[0]
    assert n_fl == dp.lmax + 1
    d_pdf = torch.zeros(n_fl, dtype=torch.float64, device=dp.dev)
    out = torch.full((n_fl, dp.n), SENTINEL, dtype=torch.float64, device=dp.dev)
    for fl0 in range(1, n_fl):
        d_pdf[fl0 - 1] = 0.0
        d_pdf[fl0] = 1.0
        dp.d_len.fill_(fl0)
        dp.launch(d_pdf, n_fl, rl, rl, out[fl0])
    got = out.cpu().numpy()
    assert (got[0] == SENTINEL).all()   # no launch for fl0 = 0
    bad = np.argwhere(got[1:] != E[1:])
    print("rl %d: %d launches, %d cases non-zero in the reference, %d mismatches" % (rl, n_fl - 1, int((E != 0).sum()), len(bad)))
    if len(bad):
        fl0, p = int(bad[0][0]) + 1, int(bad[0][1])
        pytest.fail("%d mismatches; first: segs %s implicit %s fl %d rl %d: kernel %r, oracle %d"
                    % (len(bad), segs[p].tolist(), imps[p], fl0, rl, got[fl0, p], E[fl0, p]))
    np.testing.assert_array_equal(got[1:], E[1:])


@pytest.fixture(scope="module")
def weights_ref(oracle):
    U.weight_conditions(oracle)
    return U.weight_reference(oracle)


@pytest.mark.parametrize("name,rl,law", U.weight_laws(), ids=[l[0] for l in U.weight_laws()])
def test_weights_at_5_to_32_segments(ctx, oracle, weights_ref, name, rl, law):
    """The host entry on ~6 000 pairs of 5..32 segments with short inner segments (a third and more of the reference weights
    above 1e-30, at least 20 per segment count) and pairs of 1..4 segments among them: same zeros, 1e-12 relative."""
    from strawberry_amd.binweight import bin_weights, pack_pairs
    segs, imps, lens = U.weight_sample()
    ins, _ = U.make_laws(oracle, law)
    if law[0] == "emp":
        assert (ins.start_offset < rl) == (name == "emp_offset_below_rl") and ins.start_offset != rl
    seg_off, seg_lens, mask = pack_pairs(segs, imps)
    w = bin_weights(seg_off, seg_lens, mask, lens, ins, rl, ctx=ctx)
    ref = weights_ref[name]
    nz = ref != 0
    print(name, "non-zero %d of %d, max rel err %.3g" % (nz.sum(), len(ref), (np.abs(w[nz] - ref[nz]) / ref[nz]).max()))
    check(w, ref, RTOL)


def test_tiny_density_inside_the_support_outlier_law(ctx, oracle):
    """10^6 lengths from N(200, 25) and one of 1400: 1e-281 .. 1e-308 at fl 1096..1139 between the main mass and the
    outlier's entry, so pdf_support[4] is set and EVERY pair of the launch takes the flushing loop."""
    from strawberry_amd.binweight import bin_weights, pack_pairs
    ins, o_ins = U.outlier_laws(oracle)
    segs, imps, lens = U.outlier_sample()
    assert U.tiny_inside(ins.pdf_table(U.OUTLIER + 1))
    ref = U.oracle_weights(oracle, segs, imps, lens, U.OUTLIER_RL, o_ins)
    seg_off, seg_lens, mask = pack_pairs(segs, imps)
    w = bin_weights(seg_off, seg_lens, mask, lens, ins, U.OUTLIER_RL, ctx=ctx)
    nz = ref != 0
    print("non-zero %d of %d, below 1e-270: %d, max rel err %.3g" % (nz.sum(), len(ref), (nz & (ref < 1e-270)).sum(),
                                                                       (np.abs(w[nz] - ref[nz]) / ref[nz]).max()))
    assert (nz & (ref < 1e-270)).sum() >= 5 and (~nz).sum() >= 5
    check(w, ref, RTOL)


@pytest.mark.parametrize("name,table,start_offset", U.hand_tables(), ids=[t[0] for t in U.hand_tables()])
def test_hand_made_tables(ctx, oracle, name, table, start_offset):
    """Tables straight into sbgpu_binweight_device: holes, values of 1e-300 and smaller normals between larger ones (with
    and without a main mass), an all-zero table (support [1, 0]), one entry at index 0, one at pdf_len - 1.  The reference
    is the oracle under a one-read empirical law that IS the table."""
    segs, imps, lens = U.hand_sample()
    ref = U.oracle_weights(oracle, segs, imps, lens, 50, U.hand_insert(table, start_offset))
    w = DevicePairs(ctx, segs, imps, lens).weights(table, 50, start_offset)
    assert not (w == SENTINEL).any()
    nz = ref != 0
    print(name, "non-zero %d of %d" % (nz.sum(), len(ref)), "max rel err %.3g" % (np.abs(w[nz] - ref[nz]) / ref[nz]).max() if nz.any() else "")
    if name == "all_zero":
        np.testing.assert_array_equal(w, 0.0)
    check(w, ref, RTOL) if nz.any() else np.testing.assert_array_equal(w, ref)


# ---------------------------------------------------------------- the batch loop
LAW, RL = (320.0, 60.0), 75


def gauss_table(n):
    from strawberry_amd.binweight import InsertSize
    return InsertSize(*LAW).pdf_table(n)


@pytest.fixture(scope="module")
def batch_ref(oracle):
    segs, imps, lens = U.batch_sample()
    ref = U.oracle_weights(oracle, segs, imps, lens, RL, oracle.make_insert(*LAW))
    ref.setflags(write=False)
    assert (ref[:129] > 1e-30).sum() >= 40 and (ref > 1e-30).mean() >= 0.30
    return ref


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 127, 128, 129])
def test_pair_counts_around_a_batch(ctx, batch_ref, n_pairs):
    """One batch short by one, full, and one pair into the next; the slots past n_pairs keep their sentinel."""
    import torch
    segs, imps, lens = U.batch_sample()
    # the list starts at a pair of >= 5 segments with a weight: a launch of ONE pair is the LDS path alone, and not `0 == 0`
    p0 = next(p for p in range(len(segs)) if len(segs[p]) >= 5 and batch_ref[p] > 1e-30)
    segs, imps, lens, ref = segs[p0:p0 + 130], imps[p0:p0 + 130], lens[p0:p0 + 130], batch_ref[p0:p0 + 130]
    assert p0 < 64 and (ref[:63] > 1e-30).sum() >= 20 and ref[63] > 1e-30 and ref[128] > 1e-30  # the last pair of a batch, the first of one
    dp = DevicePairs(ctx, segs, imps, lens)
    out = torch.full((130,), SENTINEL, dtype=torch.float64, device=dp.dev)
    dp.launch(dp.put(gauss_table(dp.lmax + 1), np.float64), dp.lmax + 1, RL, RL, out, n=n_pairs)
    w = out.cpu().numpy()
    assert (w[n_pairs:] == SENTINEL).all()
    check(w[:n_pairs], ref[:n_pairs], RTOL)


@pytest.mark.parametrize("which", ["probe_12_segments", "probe_2_segments"])
def test_position_independence_inside_a_batch(ctx, oracle, which):
    """A probe pair at each of the 64 positions of a batch in turn (64 lists in one launch: every list is a batch of its
    own), its 63 neighbours alternating between the closed-form and the LDS path: the probe's weight is bitwise the same at
    every position, and every neighbour's weight is bitwise what it is in a launch without the probe."""
    nb, p12, p2 = U.probe_neighbours()
    probe = p12 if which == "probe_12_segments" else p2
    segs, imps, lens = [], [], []
    for pos in range(64):
        for x, n, p in ((segs, nb[0], probe[0]), (imps, nb[1], probe[1]), (lens, nb[2], probe[2])):
            x.extend(n[:pos] + p + n[pos:])
    assert len(segs) == 64 * 64
    table = gauss_table(max(int(s.sum()) for s in segs) + 1)
    w = DevicePairs(ctx, segs, imps, lens).weights(table, RL, RL).reshape(64, 64)
    alone = DevicePairs(ctx, *nb).weights(table, RL, RL)
    o_ins = oracle.make_insert(*LAW)
    ref_probe = oracle.bin_weight(probe[0][0], probe[1][0], probe[2][0], RL, o_ins)
    ref_nb = U.oracle_weights(oracle, *nb, RL, o_ins)
    assert ref_probe > 1e-30 and (ref_nb > 1e-30).sum() >= 20
    check(alone, ref_nb, RTOL)
    for pos in range(64):
        assert w[pos, pos].tobytes() == w[0, 0].tobytes(), pos
        np.testing.assert_array_equal(np.delete(w[pos], pos).view(np.int64), alone.view(np.int64))
    assert abs(w[0, 0] - ref_probe) / ref_probe < RTOL


@pytest.mark.parametrize("kind", ["reversed", "gaps"])
def test_out_index_scatter(ctx, batch_ref, kind):
    """out_index as a reversed permutation and with gaps: every weight lands in its slot, the others keep the sentinel."""
    import torch
    n = 200
    segs, imps, lens = (x[:n] for x in U.batch_sample())
    dp = DevicePairs(ctx, segs, imps, lens)
    idx = np.arange(n)[::-1].copy() if kind == "reversed" else 3 * np.arange(n) + 1
    size = n if kind == "reversed" else 3 * n + 2
    out = torch.full((size,), SENTINEL, dtype=torch.float64, device=dp.dev)
    dp.launch(dp.put(gauss_table(dp.lmax + 1), np.float64), dp.lmax + 1, RL, RL, out, d_idx=dp.put(idx, np.int64))
    w = out.cpu().numpy()
    check(w[idx], batch_ref[:n], RTOL)
    untouched = np.ones(size, bool)
    untouched[idx] = False
    assert (w[untouched] == SENTINEL).all() and untouched.sum() == size - n


def test_long_read_with_empty_pairs_and_no_table(ctx):
    """long_read = 1, d_pdf = NULL, pairs of 0 segments among the others (what the pairs kernels emit for a bin that spans
    more than 32 isoform segments): every weight is exactly 1 / L (estimate.cpp:236-247)."""
    import torch
    segs, imps, lens = (list(x[:150]) for x in U.batch_sample())
    for p in list(range(0, 150, 7)) + [63, 64, 149]:
        segs[p], imps[p] = np.zeros(0, np.int64), []
    dp = DevicePairs(ctx, segs, imps, lens, allow_empty=True)
    out = torch.full((150,), SENTINEL, dtype=torch.float64, device=dp.dev)
    dp.launch(None, 0, RL, RL, out, long_read=1)
    np.testing.assert_array_equal(out.cpu().numpy(), 1.0 / np.asarray(lens, np.float64))


def test_more_than_two_passes_of_the_grid(ctx, batch_ref):
    """The grid is capped at 64 x CUs workgroups of one batch (64 pairs) each: a list of 4 099 pairs tiled until it is longer
    than two full passes (about 2.1 M pairs on 256 CUs).  4 099 is no multiple of 64, so the replicas land at shifting batch
    positions: every replica is bitwise the first, and the first is the oracle's."""
    import torch
    from strawberry_amd.binweight import pack_pairs
    segs, imps, lens = U.batch_sample()
    n0 = len(segs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = (2 * 64 * 64 * cus) // n0 + 1
    n = reps * n0
    assert n > 2 * 64 * 64 * cus and n < 2 ** 31
    seg_off, seg_lens, mask = pack_pairs(segs, imps)
    dev = torch.device("cuda", 0)
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    total = int(seg_off[-1])
    d_off = (put(seg_off[:-1], np.int64)[None, :] + total * torch.arange(reps, dtype=torch.int64, device=dev)[:, None]).reshape(-1)
    d_off = torch.cat([d_off, torch.tensor([total * reps], dtype=torch.int64, device=dev)])
    d_seg = put(seg_lens.view(np.int32), np.int32).repeat(reps)
    d_mask = put(mask.view(np.int32), np.int32).repeat(reps)
    d_len = put(lens, np.int32).repeat(reps)
    assert d_off.numel() == n + 1 and d_seg.numel() == total * reps and int(d_off[-1]) == d_seg.numel()
    lmax = max(int(s.sum()) for s in segs)
    d_pdf = put(gauss_table(lmax + 1), np.float64)
    out = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
    from strawberry_amd import _lib
    _lib.check(ctx.L.sbgpu_binweight_device(ctx.h, n, d_off.data_ptr(), d_seg.data_ptr(), d_mask.data_ptr(), d_len.data_ptr(), None,
                                            d_pdf.data_ptr(), lmax + 1, RL, RL, 0, out.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "sbgpu_binweight_device")
    bits = out.view(torch.int64).reshape(reps, n0)
    same = (bits == bits[0]).all(dim=1).cpu().numpy()
    print("%d CUs, %d replicas of %d pairs = %d pairs, %.0f MB" % (cus, reps, n0, n, (d_off.numel() * 8 + d_seg.numel() * 4 + n * 16) / 1e6))
    assert same.all(), int(np.nonzero(~same)[0][0])
    check(out[:n0].cpu().numpy(), batch_ref, RTOL)
