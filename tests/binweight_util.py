"""Samples and CPU references for the bin-weight kernel (csrc/binweight_device.h) at the widths and edges the random sweeps
of tests/test_binweight_gpu.py do not reach: pairs of 5..32 segments whose inner segments are short enough for a fragment to
span them (so the interval arithmetic of the >= 5-segment branch answers something other than 0), one contiguous implicit
block at either end of the inner segments, an insert-size law with a tiny density strictly inside its support, and pair
lists that put the closed-form and the LDS path side by side in one wave batch.  tests/test_binweight_util.py checks the
samples themselves on the CPU (conditions on the reference alone), tests/test_binweight_edges_gpu.py the kernel.

Everything here is seeded and built once per process (functools.lru_cache); nothing returned may be modified."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

EXACT_RLS = (20, 75)             # one read length shorter than most runs of inner segments, and 75
EXACT_SEED, WEIGHT_SEED, OUTLIER_SEED = 41, 43, 47
INNER_SPANS = (4, 12, 40)        # inner segments of 1..4, 1..12, 1..40 bases, in turn
KIND_NONE, KIND_BLOCK, KIND_SPLIT = 0, 1, 2   # nothing implicit / one contiguous block of inner segments / not contiguous
TINY = 1e-280                    # csrc/binweight_device.h: kBwTiny
DBL_MIN = 2.2250738585072014e-308
THREADS = 8                      # ctypes releases the GIL during a foreign call


def inner_len(s):
    return int(np.sum(s[1:-1])) if len(s) > 2 else 0


def fl_range(s, lmin_base):
    """[lmin, lmax] of LocusContext::set_theory_bin_weight (estimate.cpp:214-223); empty where lmin > lmax."""
    lmax = int(np.sum(s))
    lmin = int(lmin_base)
    if len(s) > 2:
        lmin = max(lmin, inner_len(s))
    return lmin, lmax


def block_kind(nseg, imp):
    if len(imp) == 0:
        return KIND_NONE
    return KIND_BLOCK if list(imp) == list(range(imp[0], imp[-1] + 1)) and imp[0] >= 1 and imp[-1] <= nseg - 2 else KIND_SPLIT


def _block(rng, nseg, where):
    """One contiguous block of the inner segments 1 .. nseg-2: at the left edge, at the right edge, anywhere, or all."""
    ni = nseg - 2
    n = int(rng.integers(1, ni + 1))
    if where == 0:
        a = 1
    elif where == 1:
        a = ni - n + 1
    elif where == 2:
        a = int(rng.integers(1, ni - n + 2))
    else:
        a, n = 1, ni
    return list(range(a, a + n))


def _split(rng, nseg):
    """A subset of the inner segments that is not one contiguous block (nseg >= 5)."""
    ni = nseg - 2
    while True:
        imp = sorted(rng.choice(np.arange(1, ni + 1), int(rng.integers(2, ni + 1)), replace=False).tolist())
        if imp != list(range(imp[0], imp[-1] + 1)):
            return imp


def _wide_pair(rng, nseg, span, end_lo, end_hi, u, blocks_only=False):
    s = np.concatenate([rng.integers(end_lo, end_hi, 1), rng.integers(1, span + 1, nseg - 2), rng.integers(end_lo, end_hi, 1)])
    if blocks_only:
        imp = [] if u < 0.4 else _block(rng, nseg, int(rng.integers(0, 4)))
    elif u < 0.3:
        imp = []
    elif u < 0.8:
        imp = _block(rng, nseg, int(rng.integers(0, 4)))
    else:
        imp = _split(rng, nseg)
    return s.astype(np.int64), imp


SMALL_PATTERNS = {1: ([],), 2: ([],), 3: ([], [1]), 4: ([], [1], [2], [1, 2])}


def _small_pair(rng, nseg, end_lo, end_hi, span):
    """1..4 segments.  The inner segments stay below the shortest read length in use: with an inner segment longer than a
    read the reference's closed forms for 3 and 4 segments (isoform.h:435-475) go negative (-1 at [78 51 33 99], rl 20,
    fl 152), and the samples promise non-negative terms -- the bound on the summation error rests on it."""
    s = rng.integers(end_lo, end_hi, nseg)
    if nseg > 2:
        s[1:-1] = rng.integers(1, span + 1, nseg - 2)
    return s.astype(np.int64)


@functools.lru_cache(maxsize=None)
def exact_sample():
    """(segs, imps): about 1 000 pairs of 1..32 segments for the integer-exact comparison of effective lengths."""
    rng = np.random.Generator(np.random.PCG64(EXACT_SEED))
    segs, imps = [], []
    for nseg in range(1, 33):
        for k in range(30):
            if nseg <= 4:
                pats = SMALL_PATTERNS[nseg]
                segs.append(_small_pair(rng, nseg, 1, 120, 19))
                imps.append(list(pats[k % len(pats)]))
            else:
                s, imp = _wide_pair(rng, nseg, INNER_SPANS[k % 3], 1, 120, (k // 3 + 0.5) / 10.0)
                segs.append(s)
                imps.append(imp)
    # a block that reaches bit 30 at 32 segments, and blocks at either edge of the inner segments at 5 and at 32
    for nseg, imp in ((32, list(range(1, 31))), (32, [30]), (32, list(range(2, 31))), (32, [1]), (32, list(range(1, 30))),
                      (5, [1]), (5, [3]), (5, [1, 2, 3]), (5, [1, 3])):
        segs.append(np.concatenate([rng.integers(30, 120, 1), rng.integers(1, 5, nseg - 2), rng.integers(30, 120, 1)]).astype(np.int64))
        imps.append(imp)
    # ranges that are empty or as short as they get: one base, ends of one base around inner segments
    for s in ([1], [1, 1], [1, 5, 1], [1, 3, 4, 1], [1, 2, 3, 2, 1], [1] + [2] * 30 + [1], [119], [119, 1]):
        segs.append(np.asarray(s, np.int64))
        imps.append([])
    order = rng.permutation(len(segs))  # closed-form and LDS pairs side by side in every wave batch
    return [segs[i] for i in order], [imps[i] for i in order]


def _eff_args(s, imp):
    su = np.ascontiguousarray(s, np.uint32)
    mu = np.ascontiguousarray(imp if len(imp) else [0], np.uint32)
    return su, mu, len(imp)


_EXACT = {}


def exact_reference(oracle):
    """{rl: E}, E[fl, pair] = the oracle's effective_len (the scan of isoform.h:476-515 at >= 5 segments) for fl inside the
    pair's [max(rl, inner), lmax] and 0 outside; E has max(lmax) + 1 rows.  Also returns the number of (pair, fl) cases."""
    if "ref" in _EXACT:
        return _EXACT["ref"]
    segs, imps = exact_sample()
    fl_top = max(int(s.sum()) for s in segs)
    fn = oracle.L.sbo_effective_len
    out, cases = {}, 0
    for rl in EXACT_RLS:
        E = np.zeros((fl_top + 1, len(segs)), np.int32)

        def one(p, E=E, rl=rl):
            su, mu, nimp = _eff_args(segs[p], imps[p])
            lo, hi = fl_range(segs[p], rl)
            for fl in range(lo, hi + 1):
                E[fl, p] = fn(len(su), su, nimp, mu, fl, rl)
            return max(0, hi - lo + 1)

        with ThreadPoolExecutor(THREADS) as ex:
            cases += sum(ex.map(one, range(len(segs))))
        E.setflags(write=False)
        out[rl] = E
    _EXACT["ref"] = (out, cases)
    return _EXACT["ref"]


def exact_conditions(oracle):
    """What the exact sample must reach, stated on the reference alone; asserted on the CPU and again by the GPU module."""
    segs, imps = exact_sample()
    ref, cases = exact_reference(oracle)
    assert 900 <= len(segs) <= 1100, len(segs)
    assert cases <= 300000, cases
    nseg = np.array([len(s) for s in segs])
    kind = np.array([block_kind(len(s), i) for s, i in zip(segs, imps)])
    nz = sum((E != 0).sum(axis=0) for E in ref.values())          # non-zero cases per pair
    assert all((E >= 0).all() for E in ref.values())
    for n in range(1, 33):
        assert nz[nseg == n].sum() >= 50, (n, int(nz[nseg == n].sum()))
    wide = nseg >= 5
    assert nz[wide & (kind == KIND_NONE)].sum() >= 2000 and nz[wide & (kind == KIND_BLOCK)].sum() >= 2000
    assert nz[wide & (kind == KIND_SPLIT)].sum() == 0 and (wide & (kind == KIND_SPLIT)).sum() >= 100
    blocks = [(len(s), i) for s, i, k, z in zip(segs, imps, kind, nz) if len(s) >= 5 and k == KIND_BLOCK and z > 0]
    assert any(i[0] == 1 for _, i in blocks) and any(i[-1] == n - 2 for n, i in blocks)
    assert any(n == 32 and i[-1] == 30 for n, i in blocks)        # bit 30 of the mask: __clz(imask) == 1
    assert any(n == 32 and i[0] == 1 for n, i in blocks)          # __ffs(imask) == 2
    # every 3- and 4-segment implicit pattern, with a non-zero answer somewhere
    for n, pats in SMALL_PATTERNS.items():
        for pat in pats:
            assert sum(z for s, i, z in zip(segs, imps, nz) if len(s) == n and list(i) == list(pat)) > 0, (n, pat)
    # empty ranges: inner > lmax - 2 (only a single segment of one base can do that with segments of >= 1 base), a read
    # longer than the pair, and at >= 3 segments the tightest pair there is: ends of one base, lmax = inner + 2
    assert any(inner_len(s) > int(s.sum()) - 2 for s in segs)
    assert any(fl_range(s, rl)[0] > fl_range(s, rl)[1] for s in segs for rl in EXACT_RLS)
    assert any(len(s) >= 5 and int(s.sum()) == inner_len(s) + 2 for s in segs)


@functools.lru_cache(maxsize=None)
def weight_sample():
    """(segs, imps, iso_len): about 6 000 pairs of 5..32 segments (inner segments of 1..12 bases, ends of 20..199, nothing
    implicit or one contiguous block) with a few hundred pairs of 1..4 segments at random positions among them."""
    rng = np.random.Generator(np.random.PCG64(WEIGHT_SEED))
    segs, imps = [], []
    for k in range(6020):
        nseg = 5 + k % 28
        s, imp = _wide_pair(rng, nseg, 12, 20, 200, float(rng.random()), blocks_only=True)
        segs.append(s)
        imps.append(imp)
    for k in range(320):
        nseg = 1 + k % 4
        pats = SMALL_PATTERNS[nseg]
        segs.append(_small_pair(rng, nseg, 20, 200, 12))
        imps.append(list(pats[(k // 4) % len(pats)]))
    order = rng.permutation(len(segs))
    segs, imps = [segs[i] for i in order], [imps[i] for i in order]
    lens = [int(s.sum() + rng.integers(0, 2001)) for s in segs]
    return segs, imps, lens


def weight_laws():
    """(name, read length, ('gauss', mean, sd) | ('emp', frag_lens)) -- the laws the weight sample runs under.  The empirical
    one is cut so that its start offset lies below its read length once and above it once (lmin_base is the offset then)."""
    rng = np.random.Generator(np.random.PCG64(WEIGHT_SEED + 1))
    fl = np.rint(rng.normal(220, 25, 4000)).astype(np.int64)
    low = np.concatenate([fl, [40]])             # start_offset 40 < rl 50
    high = fl[fl >= 170]                         # start_offset 170 > rl 50
    return (("gauss_rl36", 36, ("gauss", 320.0, 60.0)), ("gauss_rl75", 75, ("gauss", 320.0, 60.0)),
            ("gauss_rl100", 100, ("gauss", 320.0, 60.0)), ("emp_offset_below_rl", 50, ("emp", low)),
            ("emp_offset_above_rl", 50, ("emp", high)))


def make_laws(oracle, law):
    """(strawberry_amd InsertSize, the oracle's sbo_insert_t) of one weight_laws() entry."""
    from strawberry_amd.binweight import InsertSize
    if law[0] == "gauss":
        return InsertSize(law[1], law[2]), oracle.make_insert(law[1], law[2])
    ins = InsertSize.from_frag_lens(law[1])
    return ins, oracle.make_insert(ins.mean, ins.sd, law[1])


def oracle_weights(oracle, segs, imps, lens, rl, o_ins):
    """oracle.bin_weight of every pair (sequential sum over fl, the scan at >= 5 segments), on a few threads."""
    fn = oracle.L.sbo_bin_weight
    out = np.zeros(len(segs))

    def one(p):
        su, mu, nimp = _eff_args(segs[p], imps[p])
        out[p] = fn(len(su), su, nimp, mu, int(lens[p]), int(rl), C.byref(o_ins))

    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(one, range(len(segs))))
    return out


_WEIGHTS = {}


def weight_reference(oracle):
    """{law name: reference weights of weight_sample()}, computed once."""
    if not _WEIGHTS:
        segs, imps, lens = weight_sample()
        for name, rl, law in weight_laws():
            w = oracle_weights(oracle, segs, imps, lens, rl, make_laws(oracle, law)[1])
            w.setflags(write=False)
            _WEIGHTS[name] = w
    return _WEIGHTS


def weight_conditions(oracle):
    segs, imps, lens = weight_sample()
    nseg = np.array([len(s) for s in segs])
    assert (nseg >= 5).sum() >= 6000 and 200 <= (nseg <= 4).sum() <= 400
    # the bound behind the 1e-12 of check(): at most N non-negative terms per weight, N <= 2000
    assert max(fl_range(s, 0)[1] - fl_range(s, 0)[0] + 1 for s in segs) <= 2000
    su = [_eff_args(s, i) for s, i in zip(segs, imps)]
    rng = np.random.Generator(np.random.PCG64(WEIGHT_SEED + 2))
    fn = oracle.L.sbo_effective_len
    for p in rng.choice(len(segs), 400, replace=False):  # effective lengths >= 0 (every fl of 400 pairs, both extreme rl)
        for rl in (36, 100):
            lo, hi = fl_range(segs[p], rl)
            assert all(fn(len(su[p][0]), su[p][0], su[p][2], su[p][1], fl, rl) >= 0 for fl in range(lo, hi + 1))
    for name, w in weight_reference(oracle).items():
        assert (w >= 0).all()
        for n in range(5, 33):
            assert (w[nseg == n] > 1e-30).sum() >= 20, (name, n, int((w[nseg == n] > 1e-30).sum()))
        assert (w > 1e-30).mean() >= 0.30, (name, float((w > 1e-30).mean()))
    # a wave batch of 64 consecutive pairs holds both paths
    mixed = sum(1 for b in range(0, len(segs) - 63, 64) if (nseg[b:b + 64] <= 4).any() and (nseg[b:b + 64] >= 5).any())
    assert mixed >= 0.9 * (len(segs) // 64)


# ---------------------------------------------------------------- a tiny density strictly inside the support
OUTLIER = 1400
OUTLIER_RL = 75


@functools.lru_cache(maxsize=None)
def outlier_hist():
    """(start_offset, hist) of 10^6 fragment lengths from N(200, 25) and one of 1400: the Gaussian fallback fills the
    histogram's holes, so densities below 1e-280 lie strictly between the main mass and the outlier's entry."""
    rng = np.random.Generator(np.random.PCG64(OUTLIER_SEED))
    fl = np.rint(rng.normal(200, 25, 10 ** 6)).astype(np.int64)
    lo = int(fl.min())
    hist = np.zeros(OUTLIER - lo + 1, np.int64)
    hist[:int(fl.max()) - lo + 1] = np.bincount(fl - lo)
    hist[-1] += 1
    return lo, hist


def outlier_laws(oracle):
    from strawberry_amd.binweight import InsertSize
    lo, hist = outlier_hist()
    ins = InsertSize.from_hist(lo, hist)
    frag_lens = np.repeat(np.arange(lo, lo + len(hist)), hist)
    return ins, oracle.make_insert(ins.mean, ins.sd, frag_lens)


def tiny_inside(table):
    """pdf_support[4] of csrc/binweight_device.h: a non-zero density below 1e-280 strictly between two at or above it."""
    t = np.asarray(table)
    big = np.nonzero(t >= TINY)[0]
    small = np.nonzero((t != 0) & (t < TINY))[0]
    return len(big) > 0 and bool(((small > big[0]) & (small < big[-1])).any())


@functools.lru_cache(maxsize=None)
def outlier_sample():
    """A few hundred pairs: ordinary ones (lmax <= 400), ones whose range crosses the tiny densities at fl 1096..1139, ones
    that reach the outlier at 1400, and ones whose mate gap swallows 940..985 bases: their fragments are at least that plus two
    reads long, so at OUTLIER_RL mostly tiny terms remain (from 946 bases on, only tiny ones)."""
    rng = np.random.Generator(np.random.PCG64(OUTLIER_SEED + 1))
    segs, imps = [], []

    def ends(total):
        a = int(rng.integers(1, total))
        return a, total - a

    for k in range(360):
        kind = k % 4
        nseg = 1 + (k // 4) % 10
        if kind == 0:
            total = int(rng.integers(max(nseg, 60), 401))
        elif kind == 1:
            total = int(rng.integers(1100, 1400))
        else:
            total = int(rng.integers(1400, 1700))
        if kind == 3 and nseg >= 3:      # the gap swallows the inner segments: lmin = inner, beyond the main mass
            inner = rng.multinomial(int(rng.integers(940, 986)) - (nseg - 2), np.ones(nseg - 2) / (nseg - 2)) + 1
            a, b = ends(int(rng.integers(100, 500)))
            s = np.concatenate([[a], inner, [b]])
            imp = list(range(1, nseg - 1))
        elif nseg == 1:
            s, imp = np.array([total]), []
        elif nseg == 2:
            s, imp = np.array(ends(total)), []
        else:
            inner = rng.integers(1, 13, nseg - 2)
            a, b = ends(total - int(inner.sum()))
            s = np.concatenate([[a], inner, [b]])
            if nseg <= 4:
                pats = SMALL_PATTERNS[nseg]
                imp = list(pats[int(rng.integers(0, len(pats)))])
            else:
                imp = [] if rng.random() < 0.5 else _block(rng, nseg, int(rng.integers(0, 4)))
        segs.append(s.astype(np.int64))
        imps.append(imp)
    lens = [int(s.sum() + rng.integers(0, 2001)) for s in segs]
    return segs, imps, lens


# ---------------------------------------------------------------- hand-made density tables
def hand_insert(table, start_offset):
    """The oracle's law whose density is exactly `table` (0 below start_offset): an empirical histogram of ONE read, so
    that emp_hist / total_reads is the table itself, over a Gaussian that is 0 on the whole table (its mean is far away).
    Entries must be normal doubles or 0: the library's table builder emits no subnormal, and the reference reads one as 0."""
    from oracle.lib import sbo_insert_t
    t = np.ascontiguousarray(table, np.float64)
    assert ((t == 0) | (t >= DBL_MIN)).all() and (t[:start_offset] == 0).all() and 0 <= start_offset < len(t)
    ins = sbo_insert_t()
    ins._keep = np.ascontiguousarray(t[start_offset:])
    ins.mean, ins.sd, ins.use_emp = -1e6, 1.0, 1
    ins.start_offset, ins.end_offset, ins.total_reads = int(start_offset), len(t) - 1, 1
    ins.emp_hist = ins._keep.ctypes.data_as(C.POINTER(C.c_double))
    return ins


HAND_LEN = 700


def hand_tables():
    """(name, table, start_offset): densities of normal size, exact zeros as holes, values from 1e-300 down to the smallest
    normals between larger ones (their products with an effective length stay normal, their quotients by L - fl + 1 do not
    all), an all-zero table, and a single non-zero entry at index 0 and at the last index."""
    rng = np.random.Generator(np.random.PCG64(53))
    x = np.arange(HAND_LEN, dtype=np.float64)
    bell = np.exp(-0.5 * ((x - 260.0) / 60.0) ** 2) / 150.0
    out = []
    t = bell.copy()
    t[:30] = 0
    out.append(("normal", t, 30))
    t = bell.copy()
    t[:60] = 0
    t[rng.choice(np.arange(61, HAND_LEN - 1), 250, replace=False)] = 0.0
    out.append(("holes", t, 60))
    t = bell.copy()
    t[:30] = 0
    idx = rng.choice(np.arange(31, HAND_LEN - 1), 300, replace=False)
    t[idx[:100]] = 1e-300
    t[idx[100:150]] = 1e-305
    t[idx[150:200]] = 2.5e-308
    t[idx[200:]] = 0.0
    out.append(("tiny_between", t, 30))
    t = np.zeros(HAND_LEN)                       # only tiny values and holes between two normal entries
    t[40], t[HAND_LEN - 1] = 1e-3, 1e-4
    idx = rng.choice(np.arange(41, HAND_LEN - 1), 400, replace=False)
    t[idx[:150]] = 1e-300
    t[idx[150:300]] = 1e-306
    t[idx[300:]] = 2.5e-308
    out.append(("tiny_only", t, 40))
    out.append(("all_zero", np.zeros(HAND_LEN), 0))
    t = np.zeros(HAND_LEN)
    t[0] = 0.25
    out.append(("first_entry", t, 0))
    t = np.zeros(HAND_LEN)
    t[HAND_LEN - 1] = 0.25
    out.append(("last_entry", t, 0))
    return out


@functools.lru_cache(maxsize=None)
def hand_sample():
    """About 500 pairs of 1..32 segments whose lmax stays below HAND_LEN (a table must cover every pair's lmax), some of
    them ending exactly at HAND_LEN - 1, plus single segments of one and two bases (fl 0 and 1 are in their range)."""
    rng = np.random.Generator(np.random.PCG64(59))
    segs, imps = [], []
    for k in range(480):
        nseg = 1 + k % 32
        if nseg <= 4:
            s = _small_pair(rng, nseg, 20, 170, 12)
            pats = SMALL_PATTERNS[nseg]
            imp = list(pats[(k // 32) % len(pats)])
        else:
            s, imp = _wide_pair(rng, nseg, 12, 20, 150, float(rng.random()), blocks_only=True)
        if k % 5 == 0:
            s[-1] += HAND_LEN - 1 - int(s.sum())  # lmax == HAND_LEN - 1: the table's last entry is in range
        segs.append(s)
        imps.append(imp)
    for s in ([1], [2], [1, 1], [HAND_LEN - 1]):
        segs.append(np.asarray(s, np.int64))
        imps.append([])
    assert max(int(s.sum()) for s in segs) == HAND_LEN - 1 and min(int(s.min()) for s in segs) >= 1
    order = rng.permutation(len(segs))
    segs, imps = [segs[i] for i in order], [imps[i] for i in order]
    lens = [int(s.sum() + rng.integers(0, 2001)) for s in segs]
    return segs, imps, lens


# ---------------------------------------------------------------- the batch loop
@functools.lru_cache(maxsize=None)
def batch_sample(n=4099):
    """The first n pairs of weight_sample() with every third pair replaced by one of 1..4 segments: closed-form and LDS pairs
    alternate inside every batch of 64.  4 099 is no multiple of 64, so replicas of the list land at shifting positions."""
    segs, imps, lens = weight_sample()
    small = [p for p in range(len(segs)) if len(segs[p]) <= 4]
    wide = [p for p in range(len(segs)) if len(segs[p]) >= 5]
    pick = [small[(k // 3) % len(small)] if k % 3 == 1 else wide[k] for k in range(n)]
    return [segs[p] for p in pick], [imps[p] for p in pick], [lens[p] for p in pick]


def probe_neighbours():
    """63 neighbours that alternate between pairs of at most 4 and of at least 5 segments, a 12-segment probe with one
    contiguous implicit block and a 2-segment probe; all with a weight above 1e-30 under N(320, 60) at rl 75 (asserted by
    the tests that use them)."""
    segs, imps, lens = weight_sample()
    small = [p for p in range(len(segs)) if len(segs[p]) <= 4]
    wide = [p for p in range(len(segs)) if len(segs[p]) >= 5]
    nb = [small[k // 2] if k % 2 == 0 else wide[k // 2] for k in range(63)]
    probe12 = next(p for p in wide[40:] if len(segs[p]) == 12 and len(imps[p]) > 0)
    probe2 = next(p for p in small[40:] if len(segs[p]) == 2)
    pick = lambda idx: ([segs[p] for p in idx], [imps[p] for p in idx], [lens[p] for p in idx])
    return pick(nb), pick([probe12]), pick([probe2])
