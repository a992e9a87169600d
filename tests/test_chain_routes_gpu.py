"""The routes through the one-call entries (sbgpu_quantify_host / _device / _resident, csrc/chain_api.hip) that the other
tests reach only through the staged LocusQuantifier: a device grouping that declines INSIDE the call, refusals that return
before or between the stages, and a call that follows a failed one on the same context.  Whatever a call that ended early
held -- helper threads, an EM plan, the hit -> bin arena, the record kept for the context table -- must be gone: the next call
on the context gives the bits of the same call on a fresh context.  Every comparison is bit-exact.

Covered elsewhere and not repeated: hits not grouped by locus and no hits at all through sbgpu_quantify_host
(test_exonbin_gpu.py::test_one_call_chain_equals_the_staged_chain), "Not enough reads" as an error of its own
(test_resident_gpu.py::test_a_given_law_and_the_other_entries)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RL = 75


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def on_fresh_context(call):
    from strawberry_amd import em
    fresh = em.Context(0)
    try:
        return call(fresh)
    finally:
        fresh.close()


def synth_sample(n_loci, per_locus, seed):
    from strawberry_amd import exonbin as eb
    from strawberry_amd import synth
    loci = synth.make_gene_models(n_loci, seed=seed)
    hl, pairs = synth.make_fragments(loci, per_locus, seed=seed + 1, noise=0.2)
    rows = [(l, eb.hit_features(lb, rb)) for l, (lb, rb) in zip(hl, pairs)]
    rows = [(l, f) for l, f in rows if f is not None]
    return eb.Annotation(loci), eb.Hits([l for l, _ in rows], [f for _, f in rows])


HOST_ARRAYS = ("theta", "status", "iters", "F", "compat")
RESIDENT_ARRAYS = ("theta", "status", "iters", "fpkm", "frac", "tpm", "keep")


def host_call(annot, hits, insert=True):
    from strawberry_amd.quantify import InsertSize, quantify_host
    return lambda c: quantify_host(annot, hits, InsertSize(250.0, 30.0) if insert else None, RL, ctx=c)


def bins_arrays(b):
    return [b.row_off, b.f_off, b.count, b.bin_key, b.bin_compat, np.asarray(b.hit_bin), b.pair_seg_off, b.pair_seg_lens,
            b.pair_implicit_mask, b.pair_iso_len, b.pair_out_index]


def assert_same_host_results(got, want):
    for k in HOST_ARRAYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["bins"].grouped_on_device == want["bins"].grouped_on_device
    for x, y in zip(bins_arrays(got["bins"]), bins_arrays(want["bins"])):
        np.testing.assert_array_equal(x, y)


@pytest.fixture(scope="module")
def ordinary():
    """20 ordinary loci and what sbgpu_quantify_host makes of them on a context that has done nothing else."""
    annot, hits = synth_sample(20, 60, seed=51)
    want = on_fresh_context(host_call(annot, hits))
    assert want["bins"].grouped_on_device and want["bins"].n_bins > 20 and (want["theta"] > 0).any()
    return annot, hits, want


def quantify_device_raw(ctx, annot, hits, locus_hit_off):
    """sbgpu_quantify_device on `hits` uploaded as they are, with the caller's locus_hit_off."""
    import torch
    from strawberry_amd import _lib
    from strawberry_amd.quantify import InsertSize
    dev = torch.device("cuda", ctx.device)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)  # noqa: E731
    d = {"hit_locus": up(hits.hit_locus, np.int32), "feat_off": up(hits.feat_off, np.int64), "feat_code": up(hits.feat_code, np.uint8),
         "feat_left": up(hits.feat_left, np.int32), "feat_right": up(hits.feat_right, np.int32)}
    d_mass = up(hits.mass, np.float32)
    hs = _lib.sbgpu_hits_t()
    hs.n_hits = hits.n_hits
    for k, v in d.items():
        setattr(hs, k, v.data_ptr())
    a = annot._struct()
    n_iso, nl = int(annot.iso_off[-1]), annot.n_loci
    theta, status, iters = np.zeros(n_iso + 1), np.zeros(nl + 1, np.int32), np.zeros(nl + 1, np.int32)
    off = np.ascontiguousarray(locus_hit_off, np.int64)
    ins = InsertSize(250.0, 30.0)._struct(RL)
    handle = C.c_void_p()
    torch.cuda.synchronize(dev)
    _lib.check(ctx.L.sbgpu_quantify_device(ctx.h, C.byref(a), C.byref(hs), d_mass.data_ptr(), off.ctypes.data, C.byref(ins), RL, 0,
                                           theta.ctypes.data, status.ctypes.data, iters.ctypes.data, C.byref(handle)),
               "sbgpu_quantify_device")
    ctx.L.sbgpu_bins_destroy(handle)
    return theta[:n_iso], status[:nl], iters[:nl]


def locus_offsets(annot, hits):
    return np.searchsorted(hits.hit_locus, np.arange(annot.n_loci + 1), side="left").astype(np.int64)


def many_bins_case(n_keys=12000, seed=77):
    """The loci of test_device_grouping_multiword_keys_and_table_limit -- 71 isoforms that all hold the same 130 exons, so any
    run of neighbouring exons is under every isoform -- with real fragments (the one-call entries make the words themselves):
    locus 0 gets n_keys read pairs that each cover ANOTHER set of exons (left mate: 1-3 neighbouring exons from exon a on;
    right mate: 1-3 more, 0-14 exons further on), i.e. n_keys bins, more than the device grouping's largest table holds (5 600);
    three more loci get a few hundred pairs over a few dozen bins."""
    from strawberry_amd import exonbin as eb
    rng = np.random.default_rng(seed)
    loci = [[[(1000 * (l + 1) * 200 + 100 * k, 1000 * (l + 1) * 200 + 100 * k + 49) for k in range(130)]] * 71 for l in range(4)]
    shapes = [(a, p, skip, q) for a in range(130) for p in (1, 2, 3) for skip in range(15) for q in (1, 2, 3) if a + p + skip + q <= 130]
    rows = []
    for l, n in enumerate([n_keys, 300, 300, 300]):
        base = 1000 * (l + 1) * 200
        pick = rng.choice(len(shapes), n, replace=False) if l == 0 else 97 * rng.choice(40, n)   # (locus 0: all different)
        for i in pick:
            a, p, skip, q = shapes[int(i)]
            b = a + p + skip
            o1, o2 = (int(x) for x in rng.integers(0, 20, 2))
            left = [(base + 100 * k, base + 100 * k + 49) for k in range(a, a + p)]
            left[0] = (left[0][0] + o1, left[0][1])
            right = [(base + 100 * k, base + 100 * k + 49) for k in range(b, b + q)]
            right[-1] = (right[-1][0], right[-1][0] + 20 + o2)
            f = eb.hit_features(left, right)
            assert f is not None
            rows.append((l, left[0][0], right[-1][1], tuple(map(tuple, f))))
    rows = sorted(set(rows))                                 # unique hits in the order the collapse leaves: (locus, left, right)
    masses = rng.integers(1, 4, len(rows)).astype(np.float32)
    return eb.Annotation(loci), eb.Hits([r[0] for r in rows], [r[3] for r in rows], mass=masses)


def test_a_decline_inside_one_call_takes_the_host_route_and_leaves_nothing_behind(ctx, ordinary):
    from strawberry_amd import _lib
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    annot, hits = many_bins_case()
    assert annot.compat_words == 3 and annot.key_words == 5
    one = host_call(annot, hits)(ctx)
    b = one["bins"]
    assert not b.grouped_on_device and "more bins than the LDS table holds" in b.host_grouping_reason
    assert b.row_off[1] - b.row_off[0] > 8192 and (np.diff(b.row_off)[1:] < 100).all()
    q = LocusQuantifier(annot, hits, InsertSize(250.0, 30.0), RL, ctx=ctx, device_bins=False)
    ref = q.run(hits.n_hits, min_isoform_frac=0.0)
    assert not q.bins_on_device
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(one[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(one["F"], q.d_F.cpu().numpy()[:len(one["F"])])
    for x, y in zip(bins_arrays(b), bins_arrays(q.bins)):
        np.testing.assert_array_equal(x, y)
    # the device entry has no host route: it says which entry has
    with pytest.raises(_lib.SbgpuError, match=r"\(%d\).*use sbgpu_quantify_host" % _lib.SBGPU_EUNSUPPORTED):
        quantify_device_raw(ctx, annot, hits, locus_offsets(annot, hits))
    o_annot, o_hits, want = ordinary
    assert_same_host_results(host_call(o_annot, o_hits)(ctx), want)


def test_refusals_before_and_between_the_stages_leave_the_context_usable(ctx, ordinary):
    from strawberry_amd import _lib
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import InsertSize, quantify_resident
    annot, hits, want = ordinary
    check = lambda: assert_same_host_results(host_call(annot, hits)(ctx), want)  # noqa: E731
    # before anything is uploaded: a hit of a locus that does not exist
    bad = hits.hit_locus.copy()
    bad[len(bad) // 2] = annot.n_loci
    stray = eb.Hits.from_arrays(bad, hits.feat_off, hits.feat_code, hits.feat_left, hits.feat_right, mass=hits.mass)
    with pytest.raises(_lib.SbgpuError, match="sbgpu_quantify_host: hit_locus out of range"):
        host_call(annot, stray)(ctx)
    check()
    # the device entry: offsets that stop short of the hits
    off = locus_offsets(annot, hits)
    off[-1] -= 1
    with pytest.raises(_lib.SbgpuError, match="sbgpu_quantify_device: locus_hit_off does not cover the hits"):
        quantify_device_raw(ctx, annot, hits, off)
    check()
    # the resident entry, behind the grouping with the plan made and the EM in the stream: a sample of no mapped reads
    with pytest.raises(_lib.SbgpuError, match=r"sbgpu_quantify_resident: the mapped-read total must be in \[1, 2\^31\)"):
        quantify_resident(annot, hits, InsertSize(250.0, 30.0), RL, 0, ctx=ctx)
    check()
    # and the device entry itself still agrees with the host entry
    theta, status, iters = quantify_device_raw(ctx, annot, hits, locus_offsets(annot, hits))
    np.testing.assert_array_equal(theta, want["theta"])
    np.testing.assert_array_equal(status, want["status"])
    np.testing.assert_array_equal(iters, want["iters"])


def test_the_law_does_not_depend_on_how_the_call_before_ended(ctx):
    from strawberry_amd import _lib
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import quantify_resident
    annot, hits = synth_sample(80, 120, seed=71)        # (the input of test_a_given_law_and_the_other_entries)
    call = lambda c: quantify_resident(annot, hits, None, RL, hits.n_hits, ctx=c)  # noqa: E731
    want = on_fresh_context(call)
    assert want["insert"]["use_emp"] and want["n_frag_lens"] > 1000
    with pytest.raises(_lib.SbgpuError, match="Not enough reads"):
        quantify_resident(annot, eb.Hits([], []), None, RL, 1, ctx=ctx)
    got = call(ctx)
    for k in ("mean", "sd", "start_offset", "end_offset", "total_reads"):
        assert got["insert"][k] == want["insert"][k], k
    np.testing.assert_array_equal(got["insert"]["emp_hist"], want["insert"]["emp_hist"])
    for k in RESIDENT_ARRAYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["total_fpkm"] == want["total_fpkm"] and got["total_mapped_reads"] == want["total_mapped_reads"] == hits.n_hits
