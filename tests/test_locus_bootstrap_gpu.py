"""Abundances per locus and the bootstrap of Frac and of the loci's FPKM / TPM (sbgpu_locus_abundance_device,
sbgpu_locus_bootstrap_device): boot_locus_sum_kernel against the host form, the old call's results unchanged, every
replicate's Frac against the epilogue run on that replicate, the locus replicates against the host rule, the statistics against
sbgpu_replicate_stats_host, the variance of a locus' sum against its isoforms', schedule independence, two ranks on one GPU,
the refusals, and the quantifier layers."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import test_abundance_bootstrap_gpu as A
from test_abundance_bootstrap_gpu import ctx, oracle_runs, sample      # noqa: F401  (fixtures: the sample and the CPU-picked seed)
from test_locus_bootstrap import loop, mixed_loci

pytestmark = pytest.mark.gpu
ROOT = A.ROOT
RL, MIN_FRAC, N_REP = A.RL, A.MIN_FRAC, A.N_REP
OLD_KEYS = A.STAT_KEYS + ("keep_count", "status_count", "total_fpkm_rep", "fpkm_rep", "keep_rep", "theta_rep")


def flat(b):
    """a bootstrap dict's arrays by name, the "frac" and "locus" entries spelled out"""
    out = {k: v for k, v in b.items() if isinstance(v, np.ndarray)}
    for part in ("frac", "locus"):
        out.update({part + "." + k: v for k, v in b.get(part, {}).items()})
    return out


def assert_same(a, b, what, keys=None):
    a, b = flat(a), flat(b)
    for k in keys or sorted(a):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- abundances per locus

@pytest.mark.parametrize("n_loci", [1, 63, 64, 65, 257])
def test_locus_abundance_device_equals_the_host_form(ctx, n_loci):
    """bitwise; n_loci: one locus, around a wave's width, more than one workgroup.  The widths 0, 1, 3, 4, 5 and 70 in turn, an
    erased locus, one kept isoform, keep == 2, a NaN."""
    import torch
    from strawberry_amd import bootstrap
    iso_off, fpkm, keep = mixed_loci(n_loci, 300 + n_loci)
    total = 4321.5
    want = bootstrap.locus_abundance_host(iso_off, fpkm, keep, total)
    got = bootstrap.locus_abundance_device(ctx, iso_off, fpkm, keep, total)
    torch.cuda.synchronize()
    for k in ("fpkm", "tpm", "kept"):
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    ref = loop(iso_off, fpkm, keep, total)
    assert want["fpkm"].tobytes() == ref[0].tobytes() and want["tpm"].tobytes() == ref[1].tobytes()


def test_locus_abundance_on_a_resident_call(ctx):
    """the entry on the device arrays sbgpu_quantify_resident left (the toy chain sample), through ChainQuantifier.locus_abundance"""
    from strawberry_amd import bootstrap, chain
    q = chain.ChainQuantifier(ctx, n_loci=200, n_frags=1e5, seed=23, resident=True, min_isoform_frac=MIN_FRAC)
    try:
        q.step()
        got = q.locus_abundance()
        fpkm, keep = q.fpkm[:q.n_iso], q.keep[:q.n_iso]
        want = bootstrap.locus_abundance_host(q.annot.iso_off, fpkm, keep, q.total_fpkm)
        for k in ("fpkm", "tpm", "kept"):
            assert got[k].tobytes() == want[k].tobytes(), k
        kept_sum = fpkm[keep != 0].sum()
        assert (keep == 0).any() and kept_sum > 0
        assert abs(got["fpkm"].sum() - kept_sum) <= 1e-12 * kept_sum
        assert abs(got["fpkm"].sum() - q.total_fpkm) <= 1e-12 * q.total_fpkm
        tpm = q.tpm[:q.n_iso]
        np.testing.assert_allclose(got["tpm"], np.add.reduceat(np.where(keep != 0, tpm, 0.0), q.annot.iso_off[:-1]), rtol=1e-12, atol=0)
    finally:
        q.close()


# ---- the old call's results

def test_the_old_results_are_unchanged(ctx, sample, oracle_runs):
    from strawberry_amd import bootstrap
    _, _, _, annot, hits = sample
    seed = oracle_runs["seed"]
    r = A.retained(ctx, annot, hits)
    try:
        old = bootstrap.abundance_bootstrap_device(ctx, r["handle"], 8, seed, keep_theta_rep=True)
        new = bootstrap.locus_bootstrap_device(ctx, r["handle"], 8, seed, keep_theta_rep=True)
        again = bootstrap.abundance_bootstrap_device(ctx, r["handle"], 8, seed, keep_theta_rep=True)
        par = bootstrap._lib.sbgpu_bootstrap_params_t(8, 0, seed, None)
        lout = bootstrap._lib.sbgpu_locus_bootstrap_t()
        mean = np.zeros(int(annot.iso_off[-1]))
        lout.frac_mean = mean.ctypes.data
        assert ctx.L.sbgpu_locus_bootstrap_device(ctx.h, r["handle"].h, C.byref(par), 0, 7, 0, None, None, None, C.byref(lout)) == 0      # a NULL `out`
    finally:
        r["handle"].close()
    assert set(OLD_KEYS) <= set(old) and "frac" not in old and "locus" not in old
    assert_same(new, old, "the locus call's `out`", keys=OLD_KEYS)
    assert_same(again, old, "the old call after the locus call", keys=OLD_KEYS)
    assert mean.tobytes() == new["frac"]["mean"].tobytes() and lout.n_rep == 8 and lout.n_loci == annot.n_loci and lout.d_frac_rep


# ---- every replicate's Frac

def edge_batch():
    """tests/test_abundance_bootstrap_gpu.py::test_edge_loci's batch -- an ordinary locus, a hit-less one, a single-isoform one, one
    whose EM never starts (INIT_EMPTY) -- and two more loci: 70 isoforms (nine exons; the first and the last in all, the seven
    between them by the bits of 1 .. 70), and an isoform of 200 bases beside one of 800: shorter than the mean of N(250, 30)."""
    from strawberry_amd import synth
    g = synth.make_gene_models(1, seed=9, max_exons=6, max_isoforms=4)[0]
    base = max(r for iso in g for _, r in iso) + 5000
    e = base + 13000
    w = e + 20000
    ex = [(w + 300 * i, w + 300 * i + 99) for i in range(9)]
    wide = [[ex[0]] + [ex[1 + b] for b in range(7) if m >> b & 1] + [ex[8]] for m in range(1, 71)]
    s = w + 20000
    loci = [g, [[(base, base + 499)]], [[(base + 6000, base + 6799)]], [[(e, e + 99), (e + 300, e + 1299), (e + 1500, e + 1599)]], wide,
            [[(s, s + 799)], [(s, s + 199)]]]
    hl, pairs = synth.make_fragments([loci[0], loci[2], loci[4]], 60, seed=8, noise=0.0, single=0.0)
    rows = [((0, 2, 4)[l], p) for l, p in zip(hl, pairs)]
    rows += [(3, ([(e + i, e + i + RL - 1)], [(e + 1500 + i, e + 1500 + i + RL - 1)])) for i in range(12)]
    rows += [(5, ([(s + i, s + i + RL - 1)], [(s + 100 + i, s + 100 + i + RL - 1)])) for i in range(20)]           # fit both isoforms
    rows += [(5, ([(s + 300 + i, s + 300 + i + RL - 1)], [(s + 480 + i, s + 480 + i + RL - 1)])) for i in range(20)]  # the long one only
    rows.sort(key=lambda r: r[0])
    annot, hits = A.make_inputs(loci, [l for l, _ in rows], [p for _, p in rows])
    assert annot.n_loci == 6 and np.diff(annot.iso_off)[[1, 2, 4, 5]].tolist() == [1, 1, 70, 2] and len(g) > 1
    return annot, hits


def frac_by_the_epilogue(ctx, annot, r, theta, effective_len_norm):
    """sbgpu_abundance_device's d_frac on `theta` under the parameters the resident call `r` retained.  The status it reads: only
    INIT_EMPTY changes what the kernel does, and INIT_EMPTY depends on the weights alone -- a locus has it in all replicates or in
    none (include/sbgpu.h) --, so the resident call's own status says which loci have it in every replicate."""
    import torch
    from strawberry_amd import _lib, em, synth
    nl, niso = annot.n_loci, np.diff(annot.iso_off)
    one_row = np.arange(nl + 1, dtype=np.int64)
    f_off = np.concatenate([[0], np.cumsum(niso)]).astype(np.int64)
    s = em.EmBatchSolver(synth.LocusBatch(one_row, annot.iso_off.astype(np.int64), f_off, np.ones(nl, np.int32), np.zeros(int(f_off[-1])),
                                          A.iso_lengths(annot), "the epilogue alone"), ctx)
    s.d_status.copy_(torch.from_numpy(np.where(r["status"] == _lib.EM_INIT_EMPTY, _lib.EM_INIT_EMPTY, _lib.EM_OK).astype(np.int32)))
    out = []
    for row in theta:
        s.d_theta.copy_(torch.from_numpy(np.ascontiguousarray(row)))
        s.run_abundance(r["total_mapped_reads"], effective_len_norm=effective_len_norm, insert_mean=r["insert"]["mean"],
                        filter_by_expression=True, min_isoform_frac=MIN_FRAC)
        s.synchronize()
        out.append(s.d_frac[:s.n_iso].cpu().numpy())
    return np.stack(out)


@pytest.mark.parametrize("effective_len_norm", [False, True])
def test_every_replicate_frac_is_the_epilogue_frac(ctx, effective_len_norm):
    """frac_rep[k] == sbgpu_abundance_device's Frac on theta_rep[k], bitwise, on the edge batch.  The resident entry accepts
    effective_len_norm under a given law: with it the 200-base isoform is "NA" (FPKM and Frac 0.0 whatever theta says; Frac 0 is
    below min_isoform_frac, so the filter erases it: keep alone does not tell it from a filtered isoform)."""
    from strawberry_amd import _lib, bootstrap
    annot, hits = edge_batch()
    r = A.retained(ctx, annot, hits, effective_len_norm=effective_len_norm)
    try:
        assert list(r["status"][[1, 3]]) == [_lib.EM_INIT_EMPTY] * 2 and (r["status"][[0, 2, 4, 5]] != _lib.EM_INIT_EMPTY).all()
        b = bootstrap.locus_bootstrap_device(ctx, r["handle"], 5, 11, keep_theta_rep=True)
    finally:
        r["handle"].close()
    want = frac_by_the_epilogue(ctx, annot, r, b["theta_rep"], effective_len_norm)
    got = b["frac"]["rep"]
    assert got.shape == want.shape == (5, int(annot.iso_off[-1]))
    assert got.tobytes() == want.tobytes()
    assert want[0].tobytes() != want[1].tobytes()                       # (the replicates differ)
    off = annot.iso_off
    for l in (1, 3):                                                    # INIT_EMPTY: 0.0
        assert (got[:, off[l]:off[l + 1]] == 0).all() and (b["locus"]["kept_rep"][:, l] == 0).all() and (b["locus"]["fpkm_rep"][:, l] == 0).all()
    assert (got[:, off[2]] == 1.0).all() and (b["locus"]["kept_rep"][:, 2] == 1).all()         # a single isoform
    assert (b["locus"]["fpkm_rep"][:, 2] == b["fpkm_rep"][:, off[2]]).all()
    print("kept isoforms of the 70-isoform locus per replicate:", b["locus"]["kept_rep"][:, 4].tolist())
    assert (b["locus"]["kept_rep"][:, 4] > 0).all() and (b["locus"]["kept_rep"][:, 4] <= 70).all()
    short = int(off[5]) + 1
    if effective_len_norm:
        assert (got[:, short] == 0).all() and (b["fpkm_rep"][:, short] == 0).all() and (b["keep_rep"][:, short] == 0).all()
        print("theta of the NA isoform per replicate:", b["theta_rep"][:, short].tolist())
        assert (b["theta_rep"][:, short] > 0).any() and (got[:, short - 1] == 1.0).all()
    # the statistics of Frac take every replicate, whatever keep says
    st = bootstrap.replicate_stats_host(got, b["rank_lo"], b["rank_hi"])
    assert b["frac"]["lo"].tobytes() == st["lo"].tobytes() and b["frac"]["hi"].tobytes() == st["hi"].tobytes()


# ---- the locus replicates and the statistics

def check_replicates_and_statistics(b, iso_off):
    from strawberry_amd import bootstrap
    B, lo, hi = b["n_rep"], b["rank_lo"], b["rank_hi"]
    F, Lc, tot = b["frac"], b["locus"], b["total_fpkm_rep"]
    for k in range(B):      # the host rule on the downloaded rows
        want = bootstrap.locus_abundance_host(iso_off, b["fpkm_rep"][k], b["keep_rep"][k], tot[k])
        assert Lc["fpkm_rep"][k].tobytes() == want["fpkm"].tobytes(), k
        assert Lc["kept_rep"][k].tobytes() == want["kept"].tobytes(), k
    with np.errstate(all="ignore"):
        ltpm = np.where(Lc["kept_rep"] != 0, 1e6 * Lc["fpkm_rep"] / tot[:, None], 0.0)
    for name, x, got in (("frac", F["rep"], F), ("locus_fpkm", Lc["fpkm_rep"], {k: Lc["fpkm_" + k] for k in ("mean", "var", "lo", "hi")}),
                         ("locus_tpm", ltpm, {k: Lc["tpm_" + k] for k in ("mean", "var", "lo", "hi")})):
        want = bootstrap.replicate_stats_host(x, lo, hi)
        assert got["lo"].tobytes() == want["lo"].tobytes(), name
        assert got["hi"].tobytes() == want["hi"].tobytes(), name
        np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(got["var"], want["var"], rtol=1e-12, atol=0, err_msg=name)
    np.testing.assert_array_equal(Lc["kept_count"], (Lc["kept_rep"] != 0).sum(0))
    # the loci's FPKM of a replicate add up to the total TPM divides by (another order: 1e-12, tests/test_abundance_bootstrap.py's bar)
    assert (np.abs(Lc["fpkm_rep"].sum(1) - tot) <= 1e-12 * tot).all()


@pytest.fixture(scope="module")
def boot_locus(ctx, sample, oracle_runs):
    """the whole route: quantify_resident(bootstrap=dict(..., locus=True)) under the seed picked on the CPU"""
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    return quantify_resident(annot, hits, A.law(), RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC,
                             bootstrap=dict(n_rep=N_REP, seed=oracle_runs["seed"], level=0.5, keep_theta_rep=True, locus=True))


def test_statistics_under_the_picked_seed(sample, boot_locus):
    """the seed makes the filter erase some isoform in some replicates only: the loci's kept counts vary over the replicates"""
    _, _, _, annot, _ = sample
    b = boot_locus["bootstrap"]
    assert set(b["frac"]) == {"mean", "var", "lo", "hi", "rep"} and (b["rank_lo"], b["rank_hi"]) == (1, 2)
    check_replicates_and_statistics(b, annot.iso_off)
    kept = b["locus"]["kept_rep"]
    assert (kept.min(0) != kept.max(0)).any()
    assert (b["locus"]["fpkm_var"] > 0).any() and (b["frac"]["var"] > 0).any() and (b["locus"]["tpm_hi"] >= b["locus"]["tpm_lo"]).all()
    multi = np.diff(annot.iso_off) > 1
    live = (boot_locus["status"] == 0) & multi
    sums = np.add.reduceat(b["frac"]["rep"], annot.iso_off[:-1], axis=1)[:, live]
    np.testing.assert_allclose(sums, 1.0, rtol=1e-12, atol=0)        # Frac is a share of the locus in every replicate


@pytest.mark.parametrize("n_rep", [1, 2, 65])
def test_locus_replicates_and_statistics(ctx, sample, oracle_runs, n_rep):
    """n_rep: one replicate (var == 0, lo == hi), two, and 65: past the one-key-per-lane form of boot_interval_kernel"""
    from strawberry_amd import bootstrap
    _, _, _, annot, hits = sample
    r = A.retained(ctx, annot, hits)
    try:
        b = bootstrap.locus_bootstrap_device(ctx, r["handle"], n_rep, oracle_runs["seed"], level=0.9)
    finally:
        r["handle"].close()
    assert b["locus"]["fpkm_rep"].shape == (n_rep, annot.n_loci) and b["frac"]["rep"].shape == (n_rep, int(annot.iso_off[-1]))
    check_replicates_and_statistics(b, annot.iso_off)
    if n_rep == 1:
        for part, names in (("frac", ("",)), ("locus", ("fpkm_", "tpm_"))):
            for p in names:
                assert (b[part][p + "var"] == 0).all() and b[part][p + "lo"].tobytes() == b[part][p + "hi"].tobytes()
        assert b["locus"]["fpkm_mean"].tobytes() == b["locus"]["fpkm_rep"][0].tobytes()


# ---- the point of the feature

def test_a_locus_sum_varies_less_than_its_isoforms(ctx):
    """Two isoforms that share an exon of 1000 bases and differ in a short last exon: most fragments fall in the shared exon, the
    isoforms trade them from replicate to replicate, and the variance of the locus' FPKM is below the sum of the isoforms'
    variances (tests/test_locus_bootstrap.py shows the same with the host forms).  Their Frac add up to 1 in every replicate."""
    from strawberry_amd import bootstrap, synth
    g = synth.make_gene_models(1, seed=5, max_exons=5, max_isoforms=3)[0]
    p = max(r for iso in g for _, r in iso) + 5000
    pair = [[(p, p + 999), (p + 1300, p + 1399)], [(p, p + 999), (p + 1700, p + 1999)]]
    hl, pairs = synth.make_fragments([g, pair], 400, seed=6, noise=0.0, single=0.0)
    annot, hits = A.make_inputs([g, pair], hl, pairs)
    r = A.retained(ctx, annot, hits)
    try:
        b = bootstrap.locus_bootstrap_device(ctx, r["handle"], 64, 31)
    finally:
        r["handle"].close()
    j0, j1 = int(annot.iso_off[1]), int(annot.iso_off[1]) + 1
    assert annot.iso_off[2] == j1 + 1 and r["status"][1] == 0
    v0, v1, vl = b["fpkm_var"][j0], b["fpkm_var"][j1], b["locus"]["fpkm_var"][1]
    print("var: isoforms %.6g + %.6g, locus %.6g" % (v0, v1, vl))
    assert v0 > 0 and v1 > 0
    assert vl < v0 + v1
    f = b["frac"]["rep"][:, [j0, j1]]
    ok = ~np.isnan(f).any(1)
    assert ok.sum() == 64
    np.testing.assert_allclose(f[ok].sum(1), 1.0, rtol=1e-12, atol=0)
    assert (b["locus"]["kept_count"] == 64).all()


# ---- schedule independence

def test_schedule_independence(ctx, sample, oracle_runs, boot_locus):
    from strawberry_amd import bootstrap
    _, _, _, annot, hits = sample
    seed = oracle_runs["seed"]
    reps = ("fpkm_rep", "keep_rep", "theta_rep", "total_fpkm_rep", "frac.rep", "locus.fpkm_rep", "locus.kept_rep")
    r = A.retained(ctx, annot, hits)
    try:
        run = lambda n, **kw: bootstrap.locus_bootstrap_device(ctx, r["handle"], n, seed, level=0.5, keep_theta_rep=True, **kw)    # noqa: E731
        first = run(N_REP)
        assert_same(first, boot_locus["bootstrap"], "another resident call")
        assert_same(run(N_REP), first, "twice")
        eight = flat(run(8))
        for k in reps:
            assert eight[k][:N_REP].tobytes() == flat(first)[k].tobytes(), k
        later = flat(run(N_REP, rep_first=4))
        for k in reps:
            assert later[k].tobytes() == eight[k][N_REP:].tobytes(), ("rep_first", k)
    finally:
        r["handle"].close()


# ---- two ranks on one GPU

WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np
    import torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, os.path.join(%(root)r, "tests"))
    from strawberry_amd import dist, em, synth
    from strawberry_amd.quantify import InsertSize, quantify_resident
    import test_abundance_bootstrap_gpu as A
    import test_locus_bootstrap_gpu as T
    rank, world, _ = dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    ctx = em.Context(0)
    comm = dist.HostComm(ctx, rank, world)
    loci = synth.make_gene_models(80, seed=71)
    hl, pairs = synth.make_fragments(loci, 120, seed=72, noise=0.2)
    ids = np.arange(40 * rank, 40 * (rank + 1))
    mine = [(l - ids[0], p) for l, p in zip(hl, pairs) if ids[0] <= l <= ids[-1]]
    annot, hits = A.make_inputs([loci[l] for l in ids], [l for l, _ in mine], [p for _, p in mine])
    r = quantify_resident(annot, hits, InsertSize(250.0, 30.0), %(rl)d, hits.n_hits, ctx=ctx, comm=comm, min_isoform_frac=%(frac)r,
                          bootstrap=dict(n_rep=%(n_rep)d, seed=%(seed)d, level=0.5, locus_id=ids, locus=True))
    assert comm.calls == 3, comm.calls      # the mapped-read total, the FPKM total, and ONE exchange for all replicates' totals
    np.savez(os.path.join(%(out)r, "rank%%d.npz" %% rank), **T.flat(r["bootstrap"]))
    dist.barrier()
""")


def test_two_ranks_on_one_gpu(tmp_path, oracle_runs, boot_locus):
    """The sample's loci split in halves over two processes (dist.HostComm over gloo), locus_id the global indices: Frac's and the
    loci's FPKM arrays, replicates included, concatenate to the single process' bit for bit -- a locus lives on one rank.  The
    loci's TPM divide by the all-reduced totals: a shard's locus_tpm_lo / _hi are, bitwise, the order statistics of ITS loci's FPKM
    over the totals BOTH ranks hold, and the shards' locus_tpm_* agree with the single process' at 1e-12 (its totals are the same
    sums in another order: tests/test_abundance_bootstrap_gpu.py::test_two_ranks_on_one_gpu)."""
    from strawberry_amd import bootstrap
    port = 29673
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
    one = flat(boot_locus["bootstrap"])
    for k in ("frac.mean", "frac.var", "frac.lo", "frac.hi", "locus.fpkm_mean", "locus.fpkm_var", "locus.fpkm_lo", "locus.fpkm_hi", "locus.kept_count"):
        assert np.concatenate([z[k] for z in two]).tobytes() == one[k].tobytes(), k
    for k in ("frac.rep", "locus.fpkm_rep", "locus.kept_rep"):
        assert np.concatenate([z[k] for z in two], axis=1).tobytes() == one[k].tobytes(), k
    assert two[0]["total_fpkm_rep"].tobytes() == two[1]["total_fpkm_rep"].tobytes()
    tot = two[0]["total_fpkm_rep"]
    for z in two:
        assert z["locus.fpkm_rep"].sum() < 0.9 * tot.sum()           # (a shard's own loci do not add up to the totals it divides by)
        tpm = np.where(z["locus.kept_rep"] != 0, 1e6 * z["locus.fpkm_rep"] / tot[:, None], 0.0)
        st = bootstrap.replicate_stats_host(tpm, 1, 2)
        assert z["locus.tpm_lo"].tobytes() == st["lo"].tobytes() and z["locus.tpm_hi"].tobytes() == st["hi"].tobytes()
        np.testing.assert_allclose(z["locus.tpm_mean"], st["mean"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(z["locus.tpm_var"], st["var"], rtol=1e-12, atol=0)
    for k in ("locus.tpm_mean", "locus.tpm_var", "locus.tpm_lo", "locus.tpm_hi"):
        np.testing.assert_allclose(np.concatenate([z[k] for z in two]), one[k], rtol=1e-12, atol=0, err_msg=k)


# ---- refusals

def test_refusals(ctx, sample, oracle_runs):
    from strawberry_amd import _lib, bootstrap
    from strawberry_amd.quantify import quantify_resident
    _, _, _, annot, hits = sample
    seed, L = oracle_runs["seed"], ctx.L
    handles = []
    try:
        a = A.retained(ctx, annot, hits)
        handles.append(a["handle"])
        first = bootstrap.locus_bootstrap_device(ctx, a["handle"], N_REP, seed)
        p = quantify_resident(annot, hits, A.law(), RL, hits.n_hits, ctx=ctx, min_isoform_frac=MIN_FRAC, keep_handle=True)
        handles.append(p["handle"])
        with pytest.raises(_lib.SbgpuError, match=r"sbgpu_locus_bootstrap_device failed \(-1\).*without retention"):
            bootstrap.locus_bootstrap_device(ctx, p["handle"], N_REP, seed)
        with pytest.raises(_lib.SbgpuError, match=r"sbgpu_locus_bootstrap_device failed \(-1\).*stale handle"):
            bootstrap.locus_bootstrap_device(ctx, a["handle"], N_REP, seed)
        c = A.retained(ctx, annot, hits)
        handles.append(c["handle"])
        with pytest.raises(_lib.SbgpuError, match=r"\(-5\).*1024"):
            bootstrap.locus_bootstrap_device(ctx, c["handle"], 1025, seed)
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*n_rep"):
            bootstrap.locus_bootstrap_device(ctx, c["handle"], 0, seed, ranks=(0, 0))
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*ranks"):
            bootstrap.locus_bootstrap_device(ctx, c["handle"], N_REP, seed, ranks=(2, 4))
        par, out = _lib.sbgpu_bootstrap_params_t(N_REP, 0, seed, None), _lib.sbgpu_abundance_bootstrap_t()
        assert L.sbgpu_locus_bootstrap_device(ctx.h, c["handle"].h, C.byref(par), 0, 3, 0, None, None, C.byref(out), None) == _lib.SBGPU_EINVAL
        assert b"sbgpu_locus_bootstrap_device: null locus_out" in L.sbgpu_last_error()
        assert L.sbgpu_locus_abundance_device(ctx.h, 3, None, None, None, None, None, None, None, None) == _lib.SBGPU_EINVAL
        assert b"iso_off" in L.sbgpu_last_error()
        assert_same(bootstrap.locus_bootstrap_device(ctx, c["handle"], N_REP, seed), first, "after the refusals")
    finally:
        for h in handles:
            h.close()


# ---- the quantifier layer

def test_a_streamed_sample_through_the_front_quantifier(ctx):
    """FrontQuantifier(keep_bootstrap=True): the records through stream_step(), then abundance_bootstrap(locus=True) == the same
    behind step(), bit for bit; its old entries are abundance_bootstrap()'s."""
    from strawberry_amd import front
    q = front.FrontQuantifier(ctx, n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=MIN_FRAC, keep_bootstrap=True)
    try:
        q.step()
        first = q.abundance_bootstrap(N_REP, 21, keep_theta_rep=True, locus=True)
        q.to_host(q.n_bytes // 4 + 4096, pinned=False)
        q.stream_step()
        got = q.abundance_bootstrap(N_REP, 21, keep_theta_rep=True, locus=True)
        old = q.abundance_bootstrap(N_REP, 21, keep_theta_rep=True)
        assert_same(got, first, "FrontQuantifier")
        assert_same(got, old, "the old entries", keys=OLD_KEYS)
        check_replicates_and_statistics(got, q.annot.iso_off)
        assert (got["locus"]["fpkm_var"] > 0).any() and (got["frac"]["var"] > 0).any()
    finally:
        q.close()
