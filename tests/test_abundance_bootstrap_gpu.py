"""The bootstrap of the resident path (sbgpu_bootstrap_keep, sbgpu_abundance_bootstrap_device, sbgpu_replicate_stats_device;
DESIGN 3.18): boot_interval_kernel against the host form, retention changing nothing, every replicate against the oracle's
EM and epilogue, the statistics against numpy, schedule independence, the record's lifetime, two ranks on one GPU, edge loci,
and a streamed sample."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from boot_util import columns, welford

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL = 75
T = 16                # csrc/bootstrap_device.h: kBootTile, the columns of a workgroup's tile
THETA_RTOL = 1e-9     # tests/test_bootstrap_gpu.py's bars for a replicate's EM
THETA_FLOOR = 1e-9
MIN_FRAC = 0.01       # so that the expression filter bites
N_REP = 4
OUT_KEYS = ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters")
STAT_KEYS = ("theta_mean", "theta_var", "fpkm_mean", "fpkm_var", "fpkm_lo", "fpkm_hi", "tpm_mean", "tpm_var", "tpm_lo", "tpm_hi")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def make_inputs(loci, hl, pairs):
    from strawberry_amd import exonbin as eb
    rows = [(l, eb.hit_features(lb, rb)) for l, (lb, rb) in zip(hl, pairs)]
    rows = [(l, f) for l, f in rows if f is not None]
    return eb.Annotation(loci), eb.Hits([l for l, _ in rows], [f for _, f in rows])


@pytest.fixture(scope="module")
def sample():
    """the input of tests/test_resident_gpu.py::test_a_given_law_and_the_other_entries"""
    from strawberry_amd import synth
    loci = synth.make_gene_models(80, seed=71)
    hl, pairs = synth.make_fragments(loci, 120, seed=72, noise=0.2)
    annot, hits = make_inputs(loci, hl, pairs)
    return loci, hl, pairs, annot, hits


def law():
    from strawberry_amd.quantify import InsertSize
    return InsertSize(250.0, 30.0)


def iso_lengths(annot):
    ex = annot.exon_right.astype(np.int64) - annot.exon_left.astype(np.int64) + 1
    return np.add.reduceat(ex, annot.exon_off[:-1]).astype(np.int32)


# ---- the kernel alone

@pytest.mark.parametrize("n_rep", [1, 2, 3, 63, 64, 65, 100, 1000, 1024])
def test_the_kernel_equals_the_host_form(ctx, n_rep):
    """lo / hi bitwise, mean / var at 1e-12 (the same IEEE operations in the same order; the bar of
    tests/test_bootstrap_gpu.py::test_statistics).  n_rep: one value per lane with and without padding, more than one value per
    lane, the cap; n: one column, around the tile width, many tiles with a ragged last one."""
    from strawberry_amd import bootstrap
    for n in (1, T - 1, T, T + 1, 1000):
        x = columns(n_rep, n, 7000 * n_rep + n)
        lo, hi = bootstrap.interval_ranks(n_rep, 0.9)
        for a, b in {(lo, hi), (0, n_rep - 1), (n_rep // 2, n_rep // 2)}:
            want = bootstrap.replicate_stats_host(x, a, b)
            got = bootstrap.replicate_stats_device(ctx, x, a, b)
            assert got["lo"].tobytes() == want["lo"].tobytes(), (n_rep, n, a)
            assert got["hi"].tobytes() == want["hi"].tobytes(), (n_rep, n, b)
            with np.errstate(invalid="ignore"):
                np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-12, atol=0)
                np.testing.assert_allclose(got["var"], want["var"], rtol=1e-12, atol=0)
    if n_rep >= 3:
        assert np.isnan(want["mean"][3]) and np.isnan(got["mean"][3])      # (the column with two NaNs was there)


def test_the_kernel_refuses(ctx):
    from strawberry_amd import _lib, bootstrap
    with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*1024 replicates"):       # SBGPU_ESHAPE
        bootstrap.replicate_stats_device(ctx, np.zeros((1025, 3)), 0, 1024)
    with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*ranks"):
        bootstrap.replicate_stats_device(ctx, np.zeros((10, 3)), 4, 3)


# ---- retention

@pytest.fixture(scope="module")
def plain(ctx, sample):
    """the resident call as it always was, under the given law and under the empirical one"""
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    return {name: quantify_resident(annot, hits, ins, RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC)
            for name, ins in (("given", law()), ("empirical", None))}


def assert_same_outputs(a, b, what):
    for k in OUT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert (a["total_fpkm"], a["total_mapped_reads"]) == (b["total_fpkm"], b["total_mapped_reads"]), what


def test_retention_changes_nothing(ctx, sample, plain):
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    for name, ins in (("given", law()), ("empirical", None)):
        r = quantify_resident(annot, hits, ins, RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC, keep_bootstrap=True)
        assert_same_outputs(r, plain[name], name)
        both = quantify_resident(annot, hits, ins, RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC, keep_bootstrap=True, with_context=True)
        assert_same_outputs(both, plain[name], name + ", both keeps")


# ---- every replicate is the reference's procedure

@pytest.fixture(scope="module")
def oracle_runs(ctx, sample, oracle):
    """Under the given law: sbgpu_quantify_host's bins and weights; then, on the CPU and from the oracle alone, the first seed
    under which some isoform is kept in some of the N_REP replicates and erased in others, with the oracle's EM of every
    replicate's counts (em.bootstrap_counts_host) and its epilogue on that theta."""
    from strawberry_amd import em
    from strawberry_amd.quantify import quantify_host
    _, _, _, annot, hits = sample
    h = quantify_host(annot, hits, law(), RL, ctx=ctx)
    b, lengths = h["bins"], iso_lengths(annot)
    count = np.asarray(b.count, np.int32)
    for seed in range(1, 200):
        reps = []
        for k in range(N_REP):
            c = em.bootstrap_counts_host(b.row_off, count, seed, k)
            theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, c, h["F"])
            reps.append((theta, status, oracle.abundance(annot.iso_off, theta, status, lengths, hits.n_hits, min_isoform_frac=MIN_FRAC)))
        kept = np.stack([r[2]["keep"] != 0 for r in reps])
        if (kept.any(0) & ~kept.all(0)).any():
            return {"seed": seed, "reps": reps, "host": h, "count": count, "lengths": lengths}
    raise AssertionError("no seed below 200 makes the filter bite in some replicates only")


@pytest.fixture(scope="module")
def boot(ctx, sample, oracle_runs):
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    r = quantify_resident(annot, hits, law(), RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC,
                          bootstrap=dict(n_rep=N_REP, seed=oracle_runs["seed"], level=0.5, keep_theta_rep=True))
    return r


def test_every_replicate_is_the_reference_procedure(sample, oracle, oracle_runs, boot, plain):
    _, _, _, annot, hits = sample
    assert_same_outputs(boot, plain["given"], "the call in front of the bootstrap")
    np.testing.assert_array_equal(np.asarray(boot["bins"].count, np.int32), oracle_runs["count"])     # the handle's exported counts
    b = boot["bootstrap"]
    mixed = np.zeros(b["keep_rep"].shape[1], bool)
    for k, (theta, status, _) in enumerate(oracle_runs["reps"]):
        err = np.abs(b["theta_rep"][k] - theta) / np.maximum(np.abs(theta), THETA_FLOOR)
        print("replicate %d: max rel theta err %.2e" % (k, err.max()))
        assert err.max() < THETA_RTOL, (k, err.max(), int(err.argmax()))
        # the oracle's epilogue on THAT theta (tests/test_em_gpu.py::test_gpu_abundance_and_tpm_match_oracle's bars)
        want = oracle.abundance(annot.iso_off, b["theta_rep"][k], status, oracle_runs["lengths"], hits.n_hits, min_isoform_frac=MIN_FRAC)
        np.testing.assert_array_equal(b["keep_rep"][k], want["keep"], err_msg="replicate %d" % k)
        np.testing.assert_allclose(b["fpkm_rep"][k], want["fpkm"], rtol=1e-14, atol=0)
        assert abs(b["total_fpkm_rep"][k] - want["sum_fpkm"]) / want["sum_fpkm"] < 1e-12
    kept = b["keep_rep"] != 0
    mixed = kept.any(0) & ~kept.all(0)
    assert mixed.any(), "the filter must bite in some replicates only"
    assert (b["theta_rep"][0] != b["theta_rep"][1]).any()


def test_statistics(ctx, sample, oracle_runs, boot):
    from strawberry_amd.quantify import LocusQuantifier
    _, _, _, annot, hits = sample
    b = boot["bootstrap"]
    f, kept, tot = b["fpkm_rep"], b["keep_rep"] != 0, b["total_fpkm_rep"]
    lo, hi = b["rank_lo"], b["rank_hi"]
    assert (lo, hi) == (1, 2)          # level 0.5 over 4 replicates
    s = np.sort(f, axis=0)
    assert b["fpkm_lo"].tobytes() == s[lo].tobytes() and b["fpkm_hi"].tobytes() == s[hi].tobytes()
    tpm = np.where(kept, 1e6 * f / tot[:, None], 0.0)
    st = np.sort(tpm, axis=0)
    np.testing.assert_allclose(b["tpm_lo"], st[lo], rtol=1e-12, atol=0)
    np.testing.assert_allclose(b["tpm_hi"], st[hi], rtol=1e-12, atol=0)
    for name, x in (("fpkm", f), ("tpm", tpm), ("theta", b["theta_rep"])):
        m, v = welford(x)
        np.testing.assert_allclose(b[name + "_mean"], m, rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(b[name + "_var"], v, rtol=1e-12, atol=0, err_msg=name)
    np.testing.assert_array_equal(b["keep_count"], kept.sum(0))
    assert 0 < (b["keep_count"] < N_REP).sum() and (b["fpkm_var"] > 0).any() and (b["tpm_hi"] >= b["tpm_lo"]).all()
    want = np.stack([np.stack([r[1] for r in oracle_runs["reps"]]) == code for code in range(4)], axis=2).sum(0)
    np.testing.assert_array_equal(b["status_count"], want)
    # theta's statistics: LocusQuantifier.bootstrap on the same input under the same law, bit for bit (test_chain_layer's bar)
    q = LocusQuantifier(annot, hits, law(), RL, ctx=ctx)
    q.assign_bins()
    q.bin_weights()
    got = q.bootstrap(N_REP, oracle_runs["seed"])
    q.solver.synchronize()
    for mine, theirs in (("theta_mean", "mean"), ("theta_var", "var")):
        x = got[theirs].cpu().numpy()
        print(mine, "max abs diff", np.abs(b[mine] - x).max())
        assert b[mine].tobytes() == x.tobytes(), mine


# ---- schedule independence, lifetime

def retained(ctx, annot, hits, **kw):
    from strawberry_amd.quantify import quantify_resident
    return quantify_resident(annot, hits, law(), RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC, keep_bootstrap=True, keep_handle=True, **kw)


def assert_same_bootstrap(a, b, what, keys=STAT_KEYS + ("keep_count", "status_count", "total_fpkm_rep", "fpkm_rep", "keep_rep")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_schedule_independence(ctx, sample, oracle_runs, boot):
    from strawberry_amd import bootstrap
    _, _, _, annot, hits = sample
    seed = oracle_runs["seed"]
    r = retained(ctx, annot, hits)
    try:
        run = lambda n, **kw: bootstrap.abundance_bootstrap_device(ctx, r["handle"], n, seed, level=0.5, **kw)    # noqa: E731
        first = run(N_REP, keep_theta_rep=True)
        assert_same_bootstrap(first, boot["bootstrap"], "another resident call", keys=STAT_KEYS + ("keep_count", "status_count", "total_fpkm_rep", "fpkm_rep", "keep_rep", "theta_rep"))
        assert_same_bootstrap(run(N_REP, keep_theta_rep=True), first, "twice")
        assert_same_bootstrap(run(N_REP), first, "without theta_rep")
        eight = run(8, keep_theta_rep=True)
        for k in ("fpkm_rep", "keep_rep", "theta_rep", "total_fpkm_rep"):
            assert eight[k][:N_REP].tobytes() == first[k].tobytes(), k
        later = run(N_REP, rep_first=4, keep_theta_rep=True)
        for k in ("fpkm_rep", "keep_rep", "theta_rep", "total_fpkm_rep"):
            assert later[k].tobytes() == eight[k][N_REP:].tobytes(), ("rep_first", k)
    finally:
        r["handle"].close()


def test_lifetime(ctx, sample, oracle_runs, plain):
    from strawberry_amd import _lib, bootstrap, context
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    seed, L = oracle_runs["seed"], ctx.L
    handles = []
    try:
        a = retained(ctx, annot, hits, with_context=True)       # both keeps on for one call
        handles.append(a["handle"])
        t0 = context.context_table_device(ctx, a["handle"])
        b0 = bootstrap.abundance_bootstrap_device(ctx, a["handle"], N_REP, seed)
        t1 = context.context_table_device(ctx, a["handle"])
        for k in ("locus_row_off", "locus_hits", "row_bin", "row_hits", "row_prob"):
            assert getattr(t0, k).tobytes() == getattr(t1, k).tobytes(), k
        assert t0.n_rows == t1.n_rows > 0
        assert_same_bootstrap(bootstrap.abundance_bootstrap_device(ctx, a["handle"], N_REP, seed), b0, "after the table")
        # a later plain call: its usual bytes, its handle refused, and the earlier handle stale
        p = quantify_resident(annot, hits, law(), RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC, keep_handle=True)
        handles.append(p["handle"])
        assert_same_outputs(p, plain["given"], "after a bootstrap")
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*without retention"):
            bootstrap.abundance_bootstrap_device(ctx, p["handle"], N_REP, seed)
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*stale handle"):
            bootstrap.abundance_bootstrap_device(ctx, a["handle"], N_REP, seed)
        # the refusals of the call itself
        c = retained(ctx, annot, hits)
        handles.append(c["handle"])
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*n_rep"):
            bootstrap.abundance_bootstrap_device(ctx, c["handle"], 0, seed, ranks=(0, 0))
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*ranks"):
            bootstrap.abundance_bootstrap_device(ctx, c["handle"], N_REP, seed, ranks=(2, 4))
        with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*1024"):
            bootstrap.abundance_bootstrap_device(ctx, c["handle"], 1025, seed)
        par = _lib.sbgpu_bootstrap_params_t(N_REP, 0, seed, None)
        assert L.sbgpu_abundance_bootstrap_device(ctx.h, c["handle"].h, C.byref(par), 0, 3, 0, None, None, None) == _lib.SBGPU_EINVAL      # null out
        assert_same_bootstrap(bootstrap.abundance_bootstrap_device(ctx, c["handle"], N_REP, seed), b0, "after the refusals")
    finally:
        for h in handles:
            h.close()


# ---- two ranks on one GPU

WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np
    import torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, os.path.join(%(root)r, "tests"))
    from strawberry_amd import dist, em, synth
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import InsertSize, quantify_resident
    import test_abundance_bootstrap_gpu as T
    rank, world, _ = dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    ctx = em.Context(0)
    comm = dist.HostComm(ctx, rank, world)
    loci = synth.make_gene_models(80, seed=71)
    hl, pairs = synth.make_fragments(loci, 120, seed=72, noise=0.2)
    ids = np.arange(40 * rank, 40 * (rank + 1))
    mine = [(l - ids[0], p) for l, p in zip(hl, pairs) if ids[0] <= l <= ids[-1]]
    annot, hits = T.make_inputs([loci[l] for l in ids], [l for l, _ in mine], [p for _, p in mine])
    r = quantify_resident(annot, hits, InsertSize(250.0, 30.0), %(rl)d, hits.n_hits, ctx=ctx, comm=comm, min_isoform_frac=%(frac)r,
                          bootstrap=dict(n_rep=%(n_rep)d, seed=%(seed)d, level=0.5, locus_id=ids, replicates=False))
    assert comm.calls == 3, comm.calls      # the mapped-read total, the FPKM total, and ONE exchange for all replicates' totals
    b = r["bootstrap"]
    np.savez(os.path.join(%(out)r, "rank%%d.npz" %% rank), **{k: v for k, v in b.items() if isinstance(v, np.ndarray)})
    dist.barrier()
""")


def test_two_ranks_on_one_gpu(tmp_path, oracle_runs, boot):
    """The sample's loci split in halves over two processes (dist.HostComm over gloo), locus_id the global indices: fpkm_*, theta_*
    and keep_count concatenate to the single process' bit for bit; the replicates' totals are the same bits on both ranks and
    within 1e-13 of the single process' (two partial sums of at most 2^20 positive terms against one tree sum: log2(n) 2^-53
    ~ 2e-15); tpm_* at 1e-12."""
    port = 29671
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "out": str(tmp_path), "rl": RL, "frac": MIN_FRAC, "n_rep": N_REP, "seed": oracle_runs["seed"]})
    procs = []
    for rank in range(2):       # fresh children, each under its own time limit
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SB_DIST_BACKEND="gloo", RANK=str(rank), LOCAL_RANK=str(rank),
                   WORLD_SIZE="2", SB_DIST_TIMEOUT_S="120")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate() for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    two = [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(2)]
    one = boot["bootstrap"]
    for k in ("theta_mean", "theta_var", "fpkm_mean", "fpkm_var", "fpkm_lo", "fpkm_hi", "keep_count", "status_count"):
        assert np.concatenate([z[k] for z in two]).tobytes() == one[k].tobytes(), k
    assert two[0]["total_fpkm_rep"].tobytes() == two[1]["total_fpkm_rep"].tobytes()
    rel = np.abs(two[0]["total_fpkm_rep"] - one["total_fpkm_rep"]) / one["total_fpkm_rep"]
    print("totals: max rel diff %.2e" % rel.max())
    assert rel.max() <= 1e-13
    for k in ("tpm_mean", "tpm_var", "tpm_lo", "tpm_hi"):
        np.testing.assert_allclose(np.concatenate([z[k] for z in two]), one[k], rtol=1e-12, atol=0, err_msg=k)


# ---- edge loci, a streamed sample

def test_edge_loci(ctx):
    """One small batch: an ordinary locus; a locus with no hits; a single-isoform locus (every replicate draws the same total, so
    the same theta and FPKM: lo == hi == mean, var == 0); a locus whose every fragment spans an exon of 1000 bases under N(250, 30)
    (no weight above 1e-5: INIT_EMPTY in every replicate).  And n_rep = 1: var == 0, lo == hi."""
    from strawberry_amd import _lib, bootstrap, synth
    g = synth.make_gene_models(1, seed=9, max_exons=6, max_isoforms=4)[0]
    base = max(r for iso in g for _, r in iso) + 5000
    e = base + 13000        # exons of 100, 1000 and 100: a pair from the first to the last spans the middle one
    loci = [g, [[(base, base + 499)]], [[(base + 6000, base + 6799)]], [[(e, e + 99), (e + 300, e + 1299), (e + 1500, e + 1599)]]]
    hl, pairs = synth.make_fragments([loci[0], loci[2]], 60, seed=8, noise=0.0, single=0.0)
    hl = [0 if l == 0 else 2 for l in hl]
    far = [([(e + i, e + i + RL - 1)], [(e + 1500 + i, e + 1500 + i + RL - 1)]) for i in range(12)]
    hl, pairs = hl + [3] * len(far), pairs + far
    annot, hits = make_inputs(loci, hl, pairs)
    assert annot.n_loci == 4 and annot.iso_off[3] - annot.iso_off[2] == 1 and len(g) > 1
    r = retained(ctx, annot, hits)
    try:
        assert list(r["status"][[1, 3]]) == [_lib.EM_INIT_EMPTY] * 2 and r["status"][2] == 0
        b = bootstrap.abundance_bootstrap_device(ctx, r["handle"], 5, 11, keep_theta_rep=True)
        one = bootstrap.abundance_bootstrap_device(ctx, r["handle"], 1, 11, rep_first=3, keep_theta_rep=True)
    finally:
        r["handle"].close()
    np.testing.assert_array_equal(b["status_count"][[1, 3]], [[0, 5, 0, 0]] * 2)
    assert b["status_count"].sum(1).tolist() == [5] * 4
    j = int(annot.iso_off[2])
    assert b["fpkm_lo"][j] == b["fpkm_hi"][j] == b["fpkm_mean"][j] == r["fpkm"][j] > 0 and b["fpkm_var"][j] == 0
    assert b["keep_count"][j] == 5 and (b["fpkm_rep"][:, j] == r["fpkm"][j]).all()
    for l in (1, 3):            # nothing is reported for a locus whose EM never started: erased everywhere
        jj = slice(int(annot.iso_off[l]), int(annot.iso_off[l + 1]))
        assert (b["keep_count"][jj] == 0).all() and (b["tpm_mean"][jj] == 0).all() and (b["tpm_hi"][jj] == 0).all()
    assert (b["fpkm_var"][:int(annot.iso_off[1])] > 0).any()
    assert (one["fpkm_var"] == 0).all() and (one["tpm_var"] == 0).all() and (one["theta_var"] == 0).all()
    for name in ("fpkm", "tpm"):
        assert one[name + "_lo"].tobytes() == one[name + "_hi"].tobytes() == one[name + "_mean"].tobytes()
    assert one["fpkm_mean"].tobytes() == one["fpkm_rep"][0].tobytes() == b["fpkm_rep"][3].tobytes()


def test_a_streamed_sample(ctx):
    """sbgpu_front_stream_end with retention on: the toy run's records through the stream give the bootstrap of the resident call
    on the run's unique hits, bit for bit; and FrontQuantifier(keep_bootstrap=True): stream_step()'s bootstrap == step()'s."""
    import stream_util as S
    import test_front_stream_gpu as F
    from strawberry_amd import _lib, bootstrap, front
    from strawberry_amd.quantify import quantify_resident
    s, g = F.toy("E2E_FILTER")
    hits = g["hits"]
    args = dict(n_rep=N_REP, seed=21, level=0.5, keep_theta_rep=True)
    want = quantify_resident(s.annot, hits, s.insert, RL, hits.total_mapped, long_read=bool(s.long_read), ctx=ctx,
                             min_isoform_frac=s.min_isoform_frac, bootstrap=args)
    L = ctx.L
    res, out, par, used = s._outputs()
    fs, h = C.c_void_p(), C.c_void_p()
    bootstrap.bootstrap_keep(ctx, True)
    try:
        _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), int(S.chunk_bytes_for(s.off, [(0, s.n)], s.past)), C.byref(fs)),
                   "sbgpu_front_stream_begin")
        try:
            ro = np.ascontiguousarray(s.off)
            _lib.check(L.sbgpu_front_stream_push(fs, s.raw.ctypes.data, int(s.raw.size), ro.ctypes.data, s.n), "sbgpu_front_stream_push")
            _lib.check(L.sbgpu_front_stream_end(fs, C.byref(s.an), C.byref(s.ins) if s.ins is not None else None, s.read_len, s.long_read,
                                                C.byref(par), None, C.byref(used), C.byref(out), C.byref(h)), "sbgpu_front_stream_end")
            try:
                got = bootstrap.abundance_bootstrap_device(ctx, h, **args)
            finally:
                L.sbgpu_bins_destroy(h)
        finally:
            L.sbgpu_front_stream_destroy(fs)
    finally:
        bootstrap.bootstrap_keep(ctx, False)
    r = s._collect(res, out, used)
    for k in OUT_KEYS:
        assert r[k].tobytes() == want[k].tobytes(), k
    keys = STAT_KEYS + ("keep_count", "status_count", "total_fpkm_rep", "fpkm_rep", "keep_rep", "theta_rep")
    assert_same_bootstrap(got, want["bootstrap"], "the toy records streamed", keys=keys)
    assert (got["keep_count"] < N_REP).any() or (got["fpkm_var"] > 0).any()

    q = front.FrontQuantifier(ctx, n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=MIN_FRAC, keep_bootstrap=True)
    try:
        q.step()
        first = q.abundance_bootstrap(N_REP, 21, keep_theta_rep=True)
        q.to_host(q.n_bytes // 4 + 4096, pinned=False)
        q.stream_step()
        assert_same_bootstrap(q.abundance_bootstrap(N_REP, 21, keep_theta_rep=True), first, "FrontQuantifier", keys=keys)
        assert (first["fpkm_var"] > 0).any()
    finally:
        q.close()
