"""Record streams aimed at the places where the device decode (csrc/bamdecode_device.h) can be off by one: record counts at
a pass / wave / tile edge, 64-record ranges at the staging limit of either kernel and at every alignment, tiles that accept
nothing, a first tile that is slow, block totals at the one pass' capacity, and every way a record writes its blocks.  Built
with bam_util.record; every builder is seeded and cached (the CPU conditions in tests/test_bam_edges_util.py and the device
tests in tests/test_bamdecode_edges_gpu.py share one copy), and returns a Sample: the record bytes, their offsets and what
the CPU conditions need to see that the sample has the property it was built for."""
import functools
import struct

import numpy as np

import bam_util as B

N_REF = 3
TILE = 1024                    # kOneTile: records per tile of the one pass
GROUP = 64                     # a wave's pass, and the scan's tile


class Sample:
    def __init__(self, name, recs, **info):
        self.name = name
        self.sizes = np.fromiter((len(r) for r in recs), np.int64, len(recs))
        self.raw = np.frombuffer(b"".join(recs), np.uint8)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n = len(recs)
        self.info = info

    def __repr__(self):
        return "Sample(%s, %d records, %d bytes)" % (self.name, self.n, self.raw.size)


# ---------------------------------------------------------------- front_schedule.h, restated

def stage_limits(n, n_bytes, lds_max):
    """The largest 64-record range (bytes) that bam_onepass_kernel and bam_scan_kernel stage in LDS: `stage_bytes - 16` of
    bam_onepass_launch and bam_scan_launch (csrc/front_schedule.h) -> (one pass, scan).  A kernel without a buffer stages
    nothing: -16."""
    avg1 = n_bytes // n + 1
    one = min(max(4096, ((64 * avg1) * 26 // 25 + 512 + 255) & ~255), 32 * 1024)   # 64 average records + 4 % + 512, steps of 256
    one = max(0, min(one, (lds_max - 512) // 4)) & ~255                          # four waves share what a workgroup may ask for
    scan = 8 * 1024
    while scan < 64 * 1024 and scan < 70 * avg1:                                 # 1.1 x 64 average records, steps of 2 KB
        scan += 2 * 1024
    scan = max(0, min(scan, lds_max - 256))
    return one - 16, scan - 16


def block_cap(n):
    return 2 * n + 1024          # bam_onepass_launch


def oracle_prefix(o, n):
    """The oracle's answer for the first n records of the stream it decoded."""
    z = {}
    for k, v in o.items():
        if k in ("cig_off", "feat_off"):
            z[k] = v[:n + 1]
        elif k in ("cig_type", "cig_len"):
            z[k] = v[:o["cig_off"][n]]
        elif k in ("feat_code", "feat_left", "feat_right"):
            z[k] = v[:o["feat_off"][n]]
        elif k == "rec_off":
            z[k] = v[:n + 1]
        elif isinstance(v, np.ndarray):
            z[k] = v[:n]
    # a record with the paired bit that got as far as the tags (accepted, or refused as a multi-hit)
    z["any_paired"] = int((((z["sam_flag"] & 1) != 0) & np.isin(z["status"], (0, 9))).any())
    z["n"] = n
    return z


def blocks_per_record(o):
    """MATCH features of every record under the oracle (0 for a refused one)."""
    m = np.concatenate([[0], np.cumsum(o["feat_code"] == 0)])
    return np.diff(m[o["feat_off"]]) * (o["status"] == 0)


# ---------------------------------------------------------------- records

def spliced(n_blocks, rng, lo=20, hi=60):
    """M (N M)*: n_blocks aligned blocks, introns inside the default limits"""
    cig = [("M", int(rng.integers(5, 40)))]
    for _ in range(n_blocks - 1):
        cig += [("N", int(rng.integers(lo, hi))), ("M", int(rng.integers(5, 40)))]
    return cig


def plain(k, pos, cig=None, name=None, flag=0, tags=(("NH", "C", 1),), with_seq=False):
    return B.record(k % N_REF, pos, flag, "e%d" % k if name is None else name, cig or [("M", 30)], tags=list(tags), with_seq=with_seq)


def refused(k, pos):
    return B.record(k % N_REF, pos, 4, "u%d" % k, [("M", 30)], tags=[("NH", "C", 1)], with_seq=False)     # unmapped


def _varied(rng, k, pos, name, small):
    """The body of a sweep group: mostly unspliced, some with two to four blocks (the fourth is walked again), some refused."""
    r = rng.random()
    flag = int(rng.choice([0, 16, 99, 147]))
    if r < 0.6:
        cig = [("M", 40)]
    elif r < 0.8:
        cig = spliced(2, rng)
    elif r < 0.85:
        cig = spliced(3, rng)
    elif r < 0.9:
        cig = spliced(4, rng)
    else:
        cig, flag = [("M", 40)], flag | 4
    tags = [("NM", "C", int(rng.integers(0, 5)))] if rng.random() < 0.5 else []
    return B.record(k % N_REF, pos, flag, name, cig, mtid=k % N_REF, mpos=pos + 150, tags=tags, with_seq=not small and rng.random() < 0.7)


def group_of_length(serial, length, nh=None, nh_type="C", small=False):
    """64 records whose bytes add up to `length` exactly (the read names take up the slack).  With `nh`: the last record ends
    in an NH tag of that value and the one before it in XS:A, each flush against its record's end."""
    def build(extra):
        recs = []
        for j in range(GROUP):
            name = "g%d.%d" % (serial, j) + "x" * extra[j]
            k, pos = serial * GROUP + j, 1000 + 3 * (serial * GROUP + j)
            if nh is not None and j == GROUP - 1:
                recs.append(B.record(k % N_REF, pos, 0, name, [("M", 40)], tags=[("NM", "C", 1), ("NH", nh_type, nh)]))
            elif nh is not None and j == GROUP - 2:
                recs.append(B.record(k % N_REF, pos, 16, name, [("M", 40)], tags=[("NH", "C", 1), ("XS", "A", "-")]))
            else:
                recs.append(_varied(np.random.default_rng([serial, j]), k, pos, name, small))
        return recs
    extra = [0] * GROUP
    slack = length - sum(len(r) for r in build(extra))
    assert 0 <= slack <= GROUP * 240, (length, slack)
    for j in range(GROUP):
        extra[j] = slack // GROUP + (1 if j < slack % GROUP else 0)
    recs = build(extra)
    assert sum(len(r) for r in recs) == length
    return recs


# ---------------------------------------------------------------- the samples

SWEEP_AVERAGE = 120            # n_bytes // n of the sweep: the same limits at 64 KB and at 160 KB of LDS per workgroup
LDS_SIZES = (64 * 1024, 160 * 1024)


@functools.lru_cache(None)
def staging_sweep():
    """Whole 64-record groups.  For the staging limit T of either kernel: groups of every length T - 17 .. T + 17, and for
    each alignment s0 & 15 a group of T bytes and one of T + 1 (a small group in front sets the alignment); filler groups
    bring n_bytes // n to SWEEP_AVERAGE, at which the limits were computed.
    info: groups = [(first record, bytes, wanted s0 & 15 or None, NH of the last record or None)], limits = (one pass, scan)"""
    limits = stage_limits(1, SWEEP_AVERAGE, LDS_SIZES[0])
    assert limits == stage_limits(1, SWEEP_AVERAGE, LDS_SIZES[1]) and limits[0] != limits[1]
    recs, groups = [], []
    state = dict(bytes=0)

    def add(length, align=None, nh=None):
        serial = len(groups)
        g = group_of_length(serial, length, nh, "C" if serial % 4 < 2 else "i", small=length < 7500)
        groups.append((len(recs), length, align, nh))
        recs.extend(g)
        state["bytes"] += length

    def pad_to(align):
        add(4200 + (align - state["bytes"] - 4200) % 16)      # the next group then starts at `align` (mod 16)

    for which, T in enumerate(limits):
        for k, d in enumerate(range(-17, 18)):
            add(T + d, nh=1 + (k + which) % 2)
        for a in range(16):
            for d in (0, 1):
                pad_to(a)
                assert state["bytes"] % 16 == a
                add(T + d, align=a, nh=1 + (a + (a >> 1)) % 2)
    # fillers: n_bytes // n == SWEEP_AVERAGE, in the middle of the range that gives it
    for g in range(1, 400):
        n = len(recs) + GROUP * g
        per_group = (SWEEP_AVERAGE * n + n // 2 - state["bytes"]) // g
        if GROUP * 50 <= per_group <= GROUP * 250:
            for k in range(g):
                add(per_group)
            break
    s = Sample("staging_sweep", recs, groups=groups, limits=limits)
    assert s.raw.size // s.n == SWEEP_AVERAGE and s.n % GROUP == 0
    return s


COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65 * 1024, 65 * 1024 + 1, 66 * 1024 + 63)


@functools.lru_cache(None)
def count_edges():
    """One random_records bag (4 200 records, laid end to end until the longest count is reached: its period is no multiple
    of a pass, so no two tiles are alike); the streams are its prefixes of COUNTS records."""
    bag = B.random_records(np.random.default_rng(64), 4200)
    recs = (bag * (COUNTS[-1] // len(bag) + 1))[:COUNTS[-1]]
    return Sample("count_edges", recs, counts=COUNTS)


def _sparse(name, accepted_at, n=6 * TILE):
    rng = np.random.default_rng(len(name))
    keep = set(accepted_at)
    recs = [plain(k, 100 + 2 * k, spliced(int(rng.integers(1, 4)), rng)) if k in keep else refused(k, 100 + 2 * k) for k in range(n)]
    per_tile = [sum(1 for k in keep if k // TILE == t) for t in range(n // TILE)]
    return Sample(name, recs, per_tile=per_tile)


SPARSE_NAMES = ("tiles_0_and_5", "first_only", "last_only", "none", "only_1023", "only_1024", "only_1025")


@functools.lru_cache(None)
def sparse_tiles():
    """Six tiles, most of them without an accepted record (a zero count under a set flag).  info: per_tile = accepted records"""
    n = 6 * TILE
    return [_sparse("tiles_0_and_5", list(range(TILE)) + list(range(5 * TILE, n))),
            _sparse("first_only", [0]),
            _sparse("last_only", [n - 1]),
            _sparse("none", []),
            _sparse("only_1023", [1023]),
            _sparse("only_1024", [1024]),
            _sparse("only_1025", [1025])]


SLOW_OPS = 2000
SLOW_TAIL_TILES = 131


@functools.lru_cache(None)
def slow_head():
    """Tile 0: 1 024 accepted records whose CIGAR is one M and SLOW_OPS - 1 pads (one block each, walked in global memory:
    64 of them fit no buffer; M D M D ... would make a block per M, a million blocks that send every call to the two
    kernels, and the look-back's answer would never be looked at); behind it SLOW_TAIL_TILES tiles of minimal accepted records, which finish long before it:
    tiles 1-64 wait for tile 0, tiles 65-128 find no finished prefix among the 64 tiles in front of them and read 64 more,
    tiles 129 and up a third 64."""
    head = bytearray(B.record(0, 0, 0, "slow", [("M", 50)] + [("P", 1)] * (SLOW_OPS - 1), tags=[("NH", "C", 1)], with_seq=False))
    recs = []
    for k in range(TILE):
        head[8:12] = struct.pack("<i", 500 + 3 * k)
        recs.append(bytes(head))
    small = bytearray(B.record(1, 0, 0, "s", [("M", 25)], with_seq=False))
    for k in range(SLOW_TAIL_TILES * TILE):
        small[8:12] = struct.pack("<i", 10 + k)
        recs.append(bytes(small))
    return Sample("slow_head", recs)


CAP_N = 2048
CAPACITY_NAMES = ("A_at_capacity", "B_one_over_in_tile_0", "C_one_over_in_last_record", "D_at_capacity_then_refused")


@functools.lru_cache(None)
def capacity_edges():
    """n = 2 048: the one pass has room for 5 120 blocks.  A: exactly 5 120; B: 5 121, the extra block in tile 0; C: 5 121,
    the extra block in the last record; D: 5 120 in front of 64 refused records.  info: blocks = the intended total"""
    rng = np.random.default_rng(5120)
    kinds = np.array([3] * 1024 + [2] * 1024)
    rng.shuffle(kinds)

    def stream(name, kinds, tail_refused=0):
        recs = [plain(k, 100 + 5 * k, spliced(int(nb), np.random.default_rng([7, k]))) for k, nb in enumerate(kinds)]
        recs += [refused(len(kinds) + k, 20000 + k) for k in range(tail_refused)]
        assert len(recs) == CAP_N
        return Sample(name, recs, blocks=int(np.sum(kinds)))
    b = kinds.copy()
    b[int(np.flatnonzero(b[:TILE] == 2)[0])] = 3
    c = kinds.copy()
    c[-1] += 1
    d = np.array([3] * 1152 + [2] * 832)
    rng.shuffle(d)
    out = [stream("A_at_capacity", kinds), stream("B_one_over_in_tile_0", b), stream("C_one_over_in_last_record", c),
           stream("D_at_capacity_then_refused", d, 64)]
    assert [s.info["blocks"] for s in out] == [block_cap(CAP_N), block_cap(CAP_N) + 1, block_cap(CAP_N) + 1, block_cap(CAP_N)]
    return out


def _every_ordered_pair(k):
    """1 .. k in an order in which every ordered pair (a, b), a == b included, is adjacent once (cyclically): k * k entries"""
    seq, a = [], [0] * (2 * k)

    def db(t, p):              # the de Bruijn sequence B(k, 2) by Lyndon words
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return [x + 1 for x in seq]


BIG_OPS = 65535


@functools.lru_cache(None)
def block_counts():
    """Every way a record writes its blocks.  One tile of accepted records with 1 .. 8 blocks: a pass in which every ordered
    pair of counts is adjacent, an ascending, a descending and a shuffled one; then blocks that touch (an insertion), blocks
    that a deletion extends (the first, the second, the third inline one, and one beyond them), a leading and a trailing N,
    500 blocks, and 65 535 operations with 32 768 blocks (the top bit of the one pass' 16-bit count) -- in front of enough
    one-block records that the total stays within 2 n + 1 024.  (Every M starts a block, here as in the reference: a deletion
    between two M gives two blocks, the first the longer by it; an accepted record with a deletion and ONE block does not
    exist.)  info: big = that record's index, n_special = the records in front of the one-block ones"""
    rng = np.random.default_rng(8)
    counts = _every_ordered_pair(8) + list(range(1, 9)) * 8 + list(range(8, 0, -1)) * 8 + [int(x) for x in rng.permutation(list(range(1, 9)) * 8)]
    assert len(counts) == 4 * GROUP
    cigs = [spliced(c, rng) for c in counts]
    m, n_, d, i = (lambda x: ("M", x)), (lambda x: ("N", x)), (lambda x: ("D", x)), (lambda x: ("I", x))
    cigs += [[("S", 3), m(10), i(2), m(12)], [m(8), n_(30), m(10), i(1), m(12)],                   # blocks that touch
             [("S", 2), m(10), d(25), m(6)], [m(9), n_(40), m(7), d(30), m(5)],                    # a deletion longer than the runs: block 0, block 1
             [m(9), n_(40), m(7), n_(25), m(6), d(3), m(5)],                                       # ... block 2, four blocks: walked again
             [m(9), n_(40), m(7), n_(25), m(6), n_(21), m(4), d(3), m(5)],                         # ... block 3, beyond the inline ones
             [n_(50), m(20)], [m(20), n_(50)], [n_(50), m(20), n_(60), m(5), n_(70)],              # a leading / trailing N
             [("H", 4), ("S", 2), m(20), ("P", 1), n_(33), m(9), ("S", 1), ("H", 2)]]
    cigs += [spliced(500, rng)]
    big = [m(1)]
    for _ in range(BIG_OPS // 2):
        big += [n_(25), m(1)]
    assert len(big) == BIG_OPS
    cigs.append(big)
    recs = [plain(k, 1000 + 11 * k, c, flag=(0, 16, 99, 147)[k % 4], tags=[("NH", "C", 1), ("XS", "A", "+-"[k % 2])]) for k, c in enumerate(cigs)]
    n_special = len(recs)
    blocks = sum(sum(1 for op, _ in c if op == "M") for c in cigs)
    fill = blocks - 1024 + 2 * TILE                      # n + (blocks - n_special) <= 2 n + 1024, with room
    recs += [plain(n_special + k, 50 + k) for k in range(fill)]
    return Sample("block_counts", recs, big=n_special - 1, n_special=n_special)


def all_samples():
    """(sample, its offsets) of every stream but the count prefixes"""
    return [staging_sweep()] + sparse_tiles() + [slow_head()] + capacity_edges() + [block_counts()]


_oracle_results = {}


def oracle_of(oracle, s, **kw):
    """oracle.bam_decode of a sample, once per process and setting; nobody writes into the result"""
    key = (s.name, tuple(sorted(kw.items())))
    if key not in _oracle_results:
        _oracle_results[key] = oracle.bam_decode(s.raw, s.off, n_ref=N_REF, **kw)
    return _oracle_results[key]
