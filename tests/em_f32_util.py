"""Yardstick of the fp32 EM kernels (sbgpu_em_run_device_f32, sbgpu_em_run_device_bias_f32): the EM of oracle/em_oracle.c
restated in numpy, three fp32 emulations of it that differ only in the order of their sums, and a per-locus rule that says
how far an fp32 answer may sit from the fp64 oracle's.  numpy only: no code of the library is used here, the planner's
limits (tile_rows, kLayoutRHalf, layout_for) are restated.

The fp32 kernels flush denormals to zero; numpy does not (unless a library built with fast-math, the oracle's among them,
has switched the thread to flush-to-zero before).  A theta that decays through the denormals is below 1.2e-38
either way, and the weights of the inputs made here are 0, 1e-6 or at least 1e-3 (times a bias factor of at least 0.5): the
difference is far below the tolerance T_l, whose floor is 2e-2.  (A row whose every isoform decays that far would have its
denominator flush to zero on the device before numpy's reaches zero; a locus where an fp32 emulation meets a zero
denominator that the fp64 oracle does not is not among the inputs: draw_locus replaces it.)"""
import functools

import numpy as np

EM_OK, EM_INIT_EMPTY, EM_DENOM_ZERO, EM_MAXITER = 0, 1, 2, 3
MAX_ITER = 1000
THETA_LIMIT = 1e-2
ROW_EPS = 1e-5
ORDERS = ("fwd", "rev", "pair")


# ------------------------------------------------------------------ the EM by hand
def _sum(a, axis, dtype, order):
    """sum of a 2-D array along `axis` with every partial sum in `dtype`, in the order asked for"""
    a = a if axis == 1 else a.T
    if a.shape[1] == 0:
        return np.zeros(a.shape[0], dtype)
    if order == "pair":
        return np.ascontiguousarray(a).sum(axis=1, dtype=dtype)   # numpy's pairwise sum runs along the contiguous axis
    if order == "rev":
        a = a[:, ::-1]
    return np.cumsum(a, axis=1, dtype=dtype)[:, -1]


def em_by_hand(count, F, dtype=np.float64, order="pair", drop_last_row=False, limit=THETA_LIMIT):
    """One locus: (count[nrow], F[nrow, niso]) -> (theta[niso] as float64, status, iterations).
    dtype float32: every intermediate is float32, except that the step's norm accumulates in float64.
    drop_last_row / limit: the two planted errors of tests/test_em_f32_util.py (the last live row that has reads is left
    out of the M-step's column sums -- a row without reads adds nothing to them anyway; another stopping threshold)."""
    dtype = np.dtype(dtype).type
    count = np.asarray(count).reshape(-1)
    nrow = len(count)
    F = np.asarray(F)
    F = (F if F.ndim == 2 else F.reshape(nrow, -1)).astype(dtype)
    niso = F.shape[1]
    total = _sum(count.astype(dtype).reshape(1, -1), 1, dtype, order)[0]      # over ALL rows, before any is dropped
    theta0 = np.full(niso, total / dtype(niso), dtype)
    keep = (F > dtype(ROW_EPS)).any(axis=1)
    if not keep.any():
        return theta0.astype(np.float64), EM_INIT_EMPTY, 0
    Fw = np.ascontiguousarray(F[keep])
    obs = count[keep].astype(dtype)
    in_m_step = np.ones(len(obs), bool)
    if drop_last_row:
        with_reads = np.flatnonzero(obs > 0)
        in_m_step[with_reads[-1] if len(with_reads) else len(obs) - 1] = False
    theta = theta0.copy()
    status, iters = EM_MAXITER, 0
    for it in range(MAX_ITER):
        iters = it + 1
        denom = _sum(Fw * theta[None, :], 1, dtype, order)
        if (denom == 0).any():
            return theta0.astype(np.float64), EM_DENOM_ZERO, iters        # theta stays at theta0, as in the oracle
        U = (obs[:, None] * Fw * theta[None, :]) / denom[:, None]
        nxt = _sum(U[in_m_step], 0, dtype, order)
        if it == 0:
            # the first iteration ran on the raw F; from here on F is column-normalised, a zero column stays zero
            cs = _sum(Fw, 0, dtype, order)
            Fw = np.where(cs[None, :] == 0, dtype(0), Fw / np.where(cs == 0, dtype(1), cs)[None, :]).astype(dtype)
        d = (nxt - theta).astype(np.float64)
        if np.sqrt((d * d).sum()) < limit:
            status = EM_OK
            break                                                         # before theta = next
        theta = nxt
    return theta.astype(np.float64), status, iters


def em_batch_by_hand(batch, F=None, dtype=np.float64, order="pair", **kw):
    """em_by_hand over a batch (F: other weights than batch.F, same layout) -> (theta, status, iters)"""
    F = batch.F if F is None else F
    theta = np.zeros(int(batch.iso_off[-1]), np.float64)
    status = np.zeros(batch.n_loci, np.int32)
    iters = np.zeros(batch.n_loci, np.int32)
    for l in range(batch.n_loci):
        r0, r1, j0, j1 = batch.row_off[l], batch.row_off[l + 1], batch.iso_off[l], batch.iso_off[l + 1]
        t, s, i = em_by_hand(batch.count[r0:r1], F[batch.f_off[l]:batch.f_off[l + 1]].reshape(int(r1 - r0), int(j1 - j0)),
                             dtype, order, **kw)
        theta[j0:j1], status[l], iters[l] = t, s, i
    return theta, status, iters


# ------------------------------------------------------------------ the comparison
def judge_f32(got_theta, got_status, got_iters, batch, oracle_result, emulations):
    """Per locus: err = |theta - theta64|_inf, tol = T_l = 4 S_l + 2e-2, iteration difference, status agreement, and whether
    the locus is left out (an emulation's status differs from the oracle's, or its iteration count by more than 1)."""
    th64, st64, it64 = oracle_result
    n = batch.n_loci
    seg = lambda x: np.maximum.reduceat(x, batch.iso_off[:-1])   # noqa: E731  (every locus has at least one isoform)
    S = np.zeros(n)
    left_out = np.zeros(n, bool)
    for th, st, it in emulations:
        S = np.maximum(S, seg(np.abs(th - th64)))
        left_out |= (st != st64) | (np.abs(it.astype(np.int64) - it64) > 1)
    err = seg(np.where(np.isfinite(got_theta), np.abs(np.asarray(got_theta, np.float64) - th64), np.inf))
    return {"err": err, "tol": 4.0 * S + 2e-2, "S": S, "iter_diff": np.abs(np.asarray(got_iters, np.int64) - it64),
            "status_ok": np.asarray(got_status) == st64, "left_out": left_out}


def rejected_f32(j):
    """bool per locus: a locus that is not left out and misses one of the three conditions"""
    return ~j["left_out"] & ~(j["status_ok"] & (j["iter_diff"] <= 2) & (j["err"] <= j["tol"]))


def compare_f32(got_theta, got_status, got_iters, batch, oracle_result, emulations, max_left_out=0.05):
    """An fp32 answer against the fp64 oracle's (oracle_result: theta, status, iters on the widened fp32 inputs) under the
    tolerance the three fp32 emulations set:

        S_l = the largest |theta_emu - theta64|_inf over the emulations,      T_l = 4 S_l + 2e-2

    The kernel's order of operations is a fourth one next to the three sampled (a tree across lanes, FMA, a reciprocal
    with a Newton step instead of a division): it gets a factor of 4 over the worst of three draws.  The 2e-2 are two
    stopping thresholds: a run that stops one iteration earlier or later than every emulation moves theta by one step,
    and near the stop a step is below 1e-2.  A locus whose comparison rests on a rounding -- an emulation's status
    differs from the oracle's, or its iteration count by more than 1 -- is left out; at most max_left_out of the loci
    may be.  Everywhere else: status equal, |iters - iters64| <= 2 (the emulations' 1 plus one for the fourth order),
    |theta - theta64|_inf <= T_l.  Raises AssertionError otherwise.
    -> dict: worst_ratio (err / T_l), worst_locus, worst_iter_diff, left_out (the loci), n_loci"""
    j = judge_f32(got_theta, got_status, got_iters, batch, oracle_result, emulations)
    n = batch.n_loci
    left = np.flatnonzero(j["left_out"])
    assert len(left) <= max_left_out * n, "%d of %d loci left out: %s" % (len(left), n, left.tolist())
    use = ~j["left_out"]
    ratio = np.where(use, j["err"] / j["tol"], 0.0)
    worst = int(np.argmax(ratio)) if n else -1
    out = {"worst_ratio": float(ratio[worst]) if n else 0.0, "worst_locus": worst,
           "worst_iter_diff": int(j["iter_diff"][use].max()) if use.any() else 0, "left_out": left.tolist(), "n_loci": n}
    bad = np.flatnonzero(rejected_f32(j))
    assert len(bad) == 0, "loci %s: status ok %s, iteration differences %s, err / T %s" % (
        bad.tolist(), j["status_ok"][bad].tolist(), j["iter_diff"][bad].tolist(), (j["err"][bad] / j["tol"][bad]).tolist())
    return out


# ------------------------------------------------------------------ the planner's limits, restated
K_LAYOUT_RHALF = (8, 4, 4, 4, 3, 3, 2, 2)      # plan.h: kLayoutRHalf, by CPL - 1
KIND_WAVE_BASE, KIND_WAVE_DOUBLE, KIND_BLOCK, KIND_BLOCK_TALL, KIND_STREAM = 1, 2, 3, 4, 5
BLOCK_THREADS = 256
NISO = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 16, 17, 21, 25, 32, 33, 41, 49, 64)   # every (CPL, CL) layout_for makes


def tile_rows(cpl, rh):
    r = K_LAYOUT_RHALF[cpl - 1] * rh
    return 128 // cpl if r * cpl > 128 else r


def layout_for(niso):
    cl = 1
    while niso > 8 * cl:
        cl *= 2
    return (niso + cl - 1) // cl, cl


def row_counts(niso):
    """[(nrow, kind)] of a parameter: every group size of the wave kind and both ends of the two block kinds"""
    cpl, cl = layout_for(niso)
    r2, r12 = tile_rows(cpl, 2), tile_rows(cpl, 12)
    out = [(1, KIND_WAVE_BASE)]
    rl = 1
    while rl <= 64 // cl:
        out.append((r2 * rl, KIND_WAVE_BASE))
        rl *= 2
    out.append((r2 * (64 // cl) - 1, KIND_WAVE_BASE))
    out += [(r2 * (64 // cl) + 1, KIND_BLOCK), ((BLOCK_THREADS // cl) * r2, KIND_BLOCK)]
    out += [((BLOCK_THREADS // cl) * r2 + 1, KIND_BLOCK_TALL), ((BLOCK_THREADS // cl) * r12, KIND_BLOCK_TALL)]
    assert len({n for n, _ in out}) == len(out)
    return out


def expected_classes(niso):
    """{(kind, C, R, G)} the planner must make of row_counts(niso)"""
    cpl, cl = layout_for(niso)
    r2, r12 = tile_rows(cpl, 2), tile_rows(cpl, 12)
    out = {(KIND_BLOCK, cpl * cl, r2, BLOCK_THREADS), (KIND_BLOCK_TALL, cpl * cl, r12, BLOCK_THREADS)}
    rl = 1
    while rl <= 64 // cl:
        out.add((KIND_WAVE_BASE, cpl * cl, r2, cl * rl))
        rl *= 2
    return out


# ------------------------------------------------------------------ inputs
def make_locus(rng, nrow, niso):
    """F uniform in [1e-3, 0.3] with half the entries zeroed, one row that carries every isoform, one row of weights 1e-6
    (dropped by the EM; a locus of one row has only the first); counts uniform in 0..49 up to 512 rows and in 1..3 above:
    with larger totals fp32 cannot resolve the 1e-2 threshold, and zero counts on most rows would hide a lost partial sum."""
    val = rng.uniform(1e-3, 0.3, (nrow, niso))
    F = np.where(rng.random((nrow, niso)) < 0.5, val, 0.0)
    rows = rng.permutation(nrow)[:2]
    F[rows[0]] = val[rows[0]]
    if nrow > 1:
        F[rows[1]] = 1e-6
    count = rng.integers(0, 50, nrow) if nrow <= 512 else rng.integers(1, 4, nrow)
    return count.astype(np.int32), F.astype(np.float32).astype(np.float64)


def _batch(loci, name):
    from strawberry_amd import synth
    return synth.from_loci(loci, name=name)


def _biased(F64, rb, ib):
    """F * 2^(rb_i ib_j) -> (formed in float32 throughout, the float64 product of the same float32 values)"""
    F32 = F64.astype(np.float32)
    b32 = np.exp2(np.outer(rb, ib))
    assert F32.dtype == np.float32 and b32.dtype == np.float32
    return F32 * b32, F64 * np.exp2(np.outer(rb.astype(np.float64), ib.astype(np.float64)))


def _decisive(count, F32):
    """the three fp32 emulations of a locus, and whether they decide it: none differs from the fp64 EM in status, or in
    the iteration count by more than 1 (else compare_f32 would leave the locus out)"""
    _, st64, it64 = em_by_hand(count, F32.astype(np.float64), np.float64, "pair")
    emus = [em_by_hand(count, F32, np.float32, order) for order in ORDERS]
    return emus, all(st == st64 and abs(it - it64) <= 1 for _, st, it in emus)


MAX_DRAWS = 8


def draw_locus(seed, nrow, niso, with_bias):
    """One locus of the tests' inputs: make_locus and (with_bias) its bias factors, uniform in [-1, 1] as float32, from a
    generator of its own.  A draw that the emulations do not decide -- with bias or without -- would be left out of the
    comparison and check nothing, and a parameter is a dozen loci, of which the 5 % cap allows none: such a draw (a few per
    hundred, the loci of ~800 iterations) is replaced by the next one.  What decides is the emulations and the fp64 EM by
    hand, never the code under test.
    -> dict: count, F (float32 values, widened), rb, ib, emulations {bias: [(theta, status, iters)] * 3}, draws"""
    for draw in range(MAX_DRAWS):
        rng = np.random.Generator(np.random.PCG64([0xF32, seed, nrow, niso, draw]))
        count, F = make_locus(rng, nrow, niso)
        rb, ib = rng.uniform(-1, 1, nrow).astype(np.float32), rng.uniform(-1, 1, niso).astype(np.float32)
        emus, ok = {}, True
        for bias in ((False, True) if with_bias else (False,)):
            emus[bias], decided = _decisive(count, _biased(F, rb, ib)[0] if bias else F.astype(np.float32))
            ok = ok and decided
        if ok:
            break
    return {"count": count, "F": F, "rb": rb, "ib": ib, "emulations": emus, "draws": draw + 1}


def _assemble(loci, name, with_bias):
    """drawn loci -> {bias: case}; case: batch, row_bias, iso_bias (None without bias), F32 (what the emulations ran on),
    F64 (what the fp64 oracle takes), emulations (batch-wide), draws (per locus)"""
    batch = _batch([(d["count"], d["F"]) for d in loci], name)
    out = {}
    for bias in ((False, True) if with_bias else (False,)):
        if bias:
            both = [_biased(d["F"], d["rb"], d["ib"]) for d in loci]
            F32 = np.concatenate([x.reshape(-1) for x, _ in both])
            F64 = np.concatenate([y.reshape(-1) for _, y in both])
        else:
            F32, F64 = batch.F.astype(np.float32), batch.F
            assert (F32.astype(np.float64) == F64).all()
        emus = [(np.concatenate([d["emulations"][bias][e][0] for d in loci]),
                 np.array([d["emulations"][bias][e][1] for d in loci], np.int32),
                 np.array([d["emulations"][bias][e][2] for d in loci], np.int32)) for e in range(len(ORDERS))]
        out[bias] = {"batch": batch, "F32": F32, "F64": F64, "emulations": emus, "draws": [d["draws"] for d in loci],
                     "row_bias": np.concatenate([d["rb"] for d in loci]) if bias else None,
                     "iso_bias": np.concatenate([d["ib"] for d in loci]) if bias else None}
    return out


@functools.lru_cache(maxsize=None)
def _param_cases(niso):
    return _assemble([draw_locus(1, nrow, niso, True) for nrow, _ in row_counts(niso)], "f32-niso%d" % niso, True)


def param_case(niso, bias):
    """One test parameter's inputs and yardsticks -- the loci of row_counts(niso), in that order, with bias factors or
    without (the same batch) -- computed once per process and shared by the tests (treat as read-only).  The oracle's own
    result is added by the caller that has the oracle (oracle_for)."""
    return _param_cases(niso)[bool(bias)]


@functools.lru_cache(maxsize=None)
def switch_case():
    """one locus per layout with nrow = R2 * 64 / CL: 64 lanes of the wave kind at the base tile, 32 at the double tile"""
    loci = []
    for niso in NISO:
        cpl, cl = layout_for(niso)
        loci.append(draw_locus(2, tile_rows(cpl, 2) * (64 // cl), niso, False))
    return _assemble(loci, "f32-switch", False)[False]


def tile_batch(batch, reps):
    """the batch `reps` times over, copy after copy"""
    from strawberry_amd.synth import LocusBatch
    def offsets(off):
        off = np.asarray(off, np.int64)
        return np.concatenate([(off[:-1][None, :] + off[-1] * np.arange(reps, dtype=np.int64)[:, None]).reshape(-1), [off[-1] * reps]])
    return LocusBatch(offsets(batch.row_off), offsets(batch.iso_off), offsets(batch.f_off), np.tile(batch.count, reps),
                      np.tile(batch.F, reps), np.tile(batch.length, reps), batch.name + "x%d" % reps)


_oracle_results = {}


def oracle_for(oracle, niso, bias):
    """oracle.em_batch on a parameter's fp64 weights, once per process"""
    if (niso, bias) not in _oracle_results:
        c = param_case(niso, bias)
        b = c["batch"]
        _oracle_results[niso, bias] = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, c["F64"])
    return _oracle_results[niso, bias]
