"""The EM bootstrap's resampling rule on the host (sbgpu_bootstrap_counts_host; no GPU): the library against a Python
restatement of the rule of include/sbgpu.h / csrc/bootstrap_rules.h, which is itself checked against Philox4x32-10's known
answers first."""
import ctypes as C

import numpy as np
import pytest

M32 = 0xffffffff


def philox4x32_10(ctr, key):
    """Philox4x32-10 with the Random123 constants -> the four output words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def replicate(counts, g, r, s):
    """One locus' replicate by the rule as the header states it: draw by draw."""
    counts = [int(c) for c in counts]
    N = sum(counts)
    prefix = [0]
    for c in counts:
        prefix.append(prefix[-1] + c)
    out = [0] * len(counts)
    for d in range(N):
        q = d >> 1
        o = philox4x32_10((q & M32, (q >> 32) | (r << 8), g & M32, g >> 32), (s & M32, s >> 32))
        u = (o[0] | o[1] << 32) if d % 2 == 0 else (o[2] | o[3] << 32)
        t = (u * N) >> 64
        row = [i for i in range(len(counts)) if prefix[i] <= t < prefix[i + 1]]
        assert len(row) == 1
        out[row[0]] += 1
    return np.array(out, np.int32)


def test_philox_known_answers():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox4x32_10((M32,) * 4, (M32,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


@pytest.mark.parametrize("g,r,s,want", [(0, 0, 7, [15, 14, 31]), (1, 0, 7, [6, 25, 29]), (0, 1, 7, [12, 13, 35]), (0, 0, 8, [10, 22, 28])])
def test_known_replicates(g, r, s, want):
    from strawberry_amd import em
    np.testing.assert_array_equal(replicate([10, 20, 30], g, r, s), want)
    np.testing.assert_array_equal(em.bootstrap_counts_host([0, 3], [10, 20, 30], s, r, locus_id=[g]), want)


def _case_loci():
    """Loci of 1, 2, 5, 17 rows; every third row zero where there are more than two; N odd, N even, N = 0, N = 1"""
    rng = np.random.default_rng(0x5742)
    loci = []
    for nr in (1, 2, 5, 17):
        c = rng.integers(1, 12, nr)
        if nr > 2:
            c[2::3] = 0
        odd, even = c.copy(), c.copy()
        odd[0] += 1 - odd.sum() % 2
        even[0] += even.sum() % 2
        one = np.zeros(nr, np.int64)
        one[nr // 2 if nr <= 2 or (nr // 2) % 3 != 2 else 0] = 1
        loci += [odd, even, np.zeros(nr, np.int64), one]
        assert odd.sum() % 2 == 1 and even.sum() % 2 == 0 and one.sum() == 1
    return loci


@pytest.mark.parametrize("r", [0, 1, 2 ** 24 - 1])
def test_host_form_equals_the_restatement(r):
    from strawberry_amd import em
    loci = _case_loci()
    row_off = np.concatenate([[0], np.cumsum([len(c) for c in loci])]).astype(np.int64)
    count = np.concatenate(loci).astype(np.int32)
    seed = 0x0123456789abcdef
    for g in (0, 1, 2 ** 32 + 5):
        ids = np.full(len(loci), g, np.int64)
        got = em.bootstrap_counts_host(row_off, count, seed, r, locus_id=ids)
        want = np.concatenate([replicate(c, g, r, seed) for c in loci])
        np.testing.assert_array_equal(got, want)
    # without ids a locus' id is its index
    got = em.bootstrap_counts_host(row_off, count, seed, r)
    want = np.concatenate([replicate(c, l, r, seed) for l, c in enumerate(loci)])
    np.testing.assert_array_equal(got, want)


def test_totals_and_zero_rows_are_kept():
    from strawberry_amd import em, synth
    b = synth.make_random(64)
    for r in (0, 3):
        got = em.bootstrap_counts_host(b.row_off, b.count, 99, r)
        assert got.dtype == np.int32 and (got >= 0).all()
        np.testing.assert_array_equal(np.add.reduceat(np.append(got, 0).astype(np.int64), b.row_off[:-1])[b.nrow > 0],
                                      np.add.reduceat(np.append(b.count, 0).astype(np.int64), b.row_off[:-1])[b.nrow > 0])
        assert (got[b.count == 0] == 0).all()
        assert (got != b.count).any()


def test_replicate_mean_is_the_multinomial_mean():
    """Over 64 replicates (seed 0x5742) the mean of every row with 0 < p_i < 1 lies within 5 sqrt(N p_i (1 - p_i) / 64) of n_i:
    five standard errors of a multinomial cell's mean -- a condition of the law, not a tuned number.  Six loci of 1-64 rows,
    N = 2-1165 (the host form equals the restatement bit for bit, see above, so it stands for it here)."""
    from strawberry_amd import em
    rng = np.random.default_rng(0x5742)
    loci = [np.array([2]), np.array([1, 1]), rng.integers(0, 9, 5), rng.integers(0, 40, 17), rng.integers(0, 30, 40), rng.integers(0, 37, 64)]
    N = [int(c.sum()) for c in loci]
    assert min(N) == 2 and max(N) <= 1165 and max(len(c) for c in loci) == 64
    row_off = np.concatenate([[0], np.cumsum([len(c) for c in loci])]).astype(np.int64)
    count = np.concatenate(loci).astype(np.int32)
    reps = np.stack([em.bootstrap_counts_host(row_off, count, 0x5742, r) for r in range(64)]).astype(np.float64)
    Nrow = np.repeat(N, [len(c) for c in loci]).astype(np.float64)
    p = count / Nrow
    inner = (p > 0) & (p < 1)
    assert inner.sum() > 100
    units = np.abs(reps.mean(0) - count)[inner] / np.sqrt(Nrow * p * (1 - p) / 64)[inner]
    print("worst row: %.2f standard errors" % units.max())
    assert units.max() < 5.0
    # a row that holds all of its locus' fragments keeps them in every replicate
    assert (reps[:, p == 1] == count[p == 1]).all()


def test_a_split_batch_gives_the_whole_batch():
    from strawberry_amd import em, synth
    b = synth.make_random(64)
    whole = em.bootstrap_counts_host(b.row_off, b.count, 5, 2)
    cut = 29
    rc = int(b.row_off[cut])
    lo = em.bootstrap_counts_host(b.row_off[:cut + 1], b.count[:rc], 5, 2, locus_id=np.arange(cut))
    hi = em.bootstrap_counts_host(b.row_off[cut:] - rc, b.count[rc:], 5, 2, locus_id=np.arange(cut, b.n_loci))
    np.testing.assert_array_equal(np.concatenate([lo, hi]), whole)
    # ... and the ids are what carries it: the second half under its local indices is another draw
    assert (em.bootstrap_counts_host(b.row_off[cut:] - rc, b.count[rc:], 5, 2) != hi).any()


def test_bad_arguments_are_refused_with_a_reason():
    from strawberry_amd import _lib
    L = _lib.load()
    out = np.zeros(600, np.int32)
    ro = np.array([0, 3], np.int64)

    def host(row_off, count, rep):
        count = np.asarray(count, np.int32)
        return L.sbgpu_bootstrap_counts_host(len(row_off) - 1, row_off.ctypes.data, count.ctypes.data, None, 1, rep, out.ctypes.data)

    assert host(ro, [1, -2, 3], 0) == _lib.SBGPU_EINVAL and b"negative" in L.sbgpu_last_error()
    assert host(ro, [1, 2, 3], 2 ** 24) == _lib.SBGPU_EINVAL and b"2^24" in L.sbgpu_last_error()
    assert host(ro, [1, 2, 3], -1) == _lib.SBGPU_EINVAL and b"2^24" in L.sbgpu_last_error()
    assert host(np.array([0, 3, 2], np.int64), [1, 2, 3], 0) == _lib.SBGPU_EINVAL and b"row_off" in L.sbgpu_last_error()
    # 513 rows of 2^31 - 1 hold more than 2^40 fragments; 512 would not
    deep = np.full(513, 2 ** 31 - 1, np.int32)
    assert int(deep.astype(np.int64).sum()) >= 2 ** 40 > int(deep[:512].astype(np.int64).sum())
    assert host(np.array([0, 513], np.int64), deep, 0) == _lib.SBGPU_ESHAPE and b"2^40" in L.sbgpu_last_error()
    assert (out == 0).all()     # nothing was written
    assert L.sbgpu_bootstrap_counts_host(1, None, None, None, 1, 0, out.ctypes.data) == _lib.SBGPU_EINVAL
    # the device entries look at their parameters before they look for a device
    for n_rep, first, word in ((0, 0, b"n_rep"), (-3, 0, b"n_rep"), (1, 2 ** 24, b"2^24"), (2, 2 ** 24 - 1, b"2^24"), (1, -1, b"2^24")):
        par = _lib.sbgpu_bootstrap_params_t(n_rep, first, 1, None)
        assert L.sbgpu_bootstrap_counts_device(None, 1, ro.ctypes.data, None, C.byref(par), None, None) == _lib.SBGPU_EINVAL
        assert word in L.sbgpu_last_error()
        assert L.sbgpu_em_bootstrap_device(None, None, None, None, C.byref(par), None, None, None, None, None, None, None) == _lib.SBGPU_EINVAL
        assert word in L.sbgpu_last_error()
    assert L.sbgpu_em_bootstrap_device(None, None, None, None, None, None, None, None, None, None, None, None) == _lib.SBGPU_EINVAL
