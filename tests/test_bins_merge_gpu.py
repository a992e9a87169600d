"""The bin-table merge on the device (sbgpu_bins_merge_device, csrc/merge_device.h) against the host form and
tests/merge_util.py::by_hand, bit for bit: the five EM goldens at three key widths; the adversarial key sets; loci on either side
of every limit sbgpu_bins_merge_limits exports; loci without bins; K = 1 and K = 512; more loci than two passes of each grid; the
refusals; two calls.  Then two retained samples on two contexts: differential_usage(other, shared_bins=True) against by_hand fed
the handles' exported keys and counts, the oracle's bin weights under the right law, and sbgpu_em_diff_device on the merged arrays."""
import ctypes as C

import numpy as np
import pytest

import merge_util as MU
from strawberry_amd import _lib, diff, merge
from test_binweight_gpu import RTOL
from test_bins_merge import GOLDENS, pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def device_sample(ctx, s):
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(dt).reshape(-1).copy()).to(dev)  # noqa: E731
    return merge.Sample(s.iso_off, s.row_off, up(s.key, np.int32), up(s.count, np.int32), up(s.F, np.float64), up(s.X, np.float64), key_words=s.key_words)


def run(ctx, a, b, **kw):
    return merge.merge_device(ctx, device_sample(ctx, a), device_sample(ctx, b), **kw)


def check(ctx, a, b, label=""):
    """the device form against the host form AND by_hand -> the MergedBins"""
    t = run(ctx, a, b)
    MU.assert_same(t, MU.by_hand(a, b), label + " (by hand)")
    h = merge.merge_host(a, b)
    MU.assert_same(t, {k: getattr(h, k) for k in ("row_off", "f_off") + merge.NAMES}, label + " (host form)")
    assert set(t.device) == set(merge.NAMES) or t.n_bins == 0
    return t


@pytest.mark.parametrize("kw", [1, 2, 3])
@pytest.mark.parametrize("name", GOLDENS)
def test_device_form_is_the_host_forms_bit_for_bit(ctx, golden, name, kw):
    a, b = pair(golden, name, kw)
    t = check(ctx, a, b, "%s kw=%d" % (name, kw))
    assert (t.row_a < 0).any() and (t.row_b < 0).any()
    if kw == 2:
        check(ctx, a.without_X(), b.without_X(), name + " X NULL")


def test_adversarial_key_sets(ctx):
    lim = merge.limits()
    rng = np.random.default_rng(21)
    pairs = {1: [], 2: [], 3: [], 5: []}
    for n in (40, 300):                    # the small form, the deep form
        for kw in (2, 3, 5):
            for kind in ("last", "first"):
                pairs[kw].append(MU.one_locus_pair(*MU.split_keys(MU.adversarial_keys(kind, n, kw, rng), n // 3, n // 3, rng), 3, rng))
        pairs[2].append(MU.one_locus_pair(*MU.split_keys(MU.adversarial_keys("swapped", n, 2, rng), n // 3, n // 3, rng), 2, rng))
        # (u, v) in A against (v, u) in B only: nothing matches
        u = MU.adversarial_keys("last", n, 2, rng)
        u[:, 0] = rng.permutation(9 * n)[:n] + 7 * n
        pairs[2].append(MU.one_locus_pair(u, u[:, ::-1].copy(), 2, rng))
    for kw in (1, 2):                      # every key in one slot of the deep form's table
        k = MU.adversarial_keys("collide", 240, kw, rng, lim["table_slots"])
        assert len(set(int(x) for x in MU.key_hash(k) & np.uint64(lim["table_slots"] - 1))) == 1
        pairs[kw].append(MU.one_locus_pair(*MU.split_keys(k, 80, 80, rng), 2, rng))
    for kw, ps in pairs.items():
        a, b = MU.concat(ps)
        t = check(ctx, a, b, "adversarial kw=%d" % kw)
        assert ((t.row_a >= 0) & (t.row_b >= 0)).any() or kw == 5
    a, b = pairs[2][-2]
    assert check(ctx, a, b).n_bins == len(a.count) + len(b.count)


def test_loci_on_either_side_of_the_limits(ctx):
    lim = merge.limits()
    g, top = lim["group_max_bins"], lim["max_bins"]
    assert (g, lim["table_slots"], top, lim["threads"]) == (64, 16384, 5632, 256) and lim["table_slots"] >= 2 * top > lim["table_slots"] // 2
    rng = np.random.default_rng(22)
    keys = MU.distinct_keys(rng, top + 1, 2)
    ps = []
    for na, nb in ((g, g), (g + 1, g), (g, g + 1), (g - 1, g + 1), (g + 1, 3), (1, g), (g, 1), (1, 1), (2, 3), (33, 31), (g + 1, g + 1), (257, 255), (255, 513)):
        shared = min(na, nb) // 2
        ka, kb = MU.split_keys(keys[:na + nb - shared], shared, na - shared, rng)
        assert len(ka) == na and len(kb) == nb
        ps.append(MU.one_locus_pair(ka, kb, 3, rng))
    a, b = MU.concat(ps)
    check(ctx, a, b, "class boundary")
    # 5632 union rows pass, 5633 are refused, in every split of the union between the samples
    for na, shared in ((3000, 1000), (top, top), (40, 20)):
        ka, kb = MU.split_keys(keys[:top], shared, na - shared, rng)
        t = check(ctx, *MU.one_locus_pair(ka, kb, 1, rng), "5632 rows")
        assert t.n_bins == top
        ka, kb = MU.split_keys(keys, shared, na - shared, rng)
        if len(kb) <= top:
            a, b = MU.concat([ps[3], MU.one_locus_pair(ka, kb, 1, rng)])
            with pytest.raises(_lib.SbgpuError, match=r"\(-5\): sbgpu_bins_merge_device: the union of locus 1 has more than 5632 bins"):
                run(ctx, a, b)
    a, b = MU.one_locus_pair(keys, keys[:2], 1, rng, with_X=False)
    with pytest.raises(_lib.SbgpuError, match=r"\(-5\): sbgpu_bins_merge_device: a locus of more than 5632 bins"):
        run(ctx, a, b)


def test_loci_without_bins_and_narrow_and_wide_loci(ctx):
    rng = np.random.default_rng(23)
    k = MU.distinct_keys(rng, 400, 2)
    none = np.zeros((0, 2), np.uint32)
    ps = [MU.one_locus_pair(none, k[:4], 3, rng), MU.one_locus_pair(k[:5], none, 2, rng), MU.one_locus_pair(none, none, 3, rng),
          MU.one_locus_pair(k[:3], k[2:6], 0, rng), MU.one_locus_pair(none, k[:100], 2, rng), MU.one_locus_pair(k[:100], none, 2, rng),
          MU.one_locus_pair(*MU.split_keys(k[:9], 3, 3, rng), 1, rng), MU.one_locus_pair(k[:2], k[1:3], 512, rng),
          MU.one_locus_pair(*MU.split_keys(k, 100, 150, rng), 1, rng), MU.one_locus_pair(*MU.split_keys(k[:30], 10, 10, rng), 700, rng)]
    a, b = MU.concat(ps)
    t = check(ctx, a, b, "edge shapes")
    assert np.diff(t.row_off)[7] == 3 and np.diff(a.iso_off)[7] == 512
    e, _ = MU.concat([ps[2], ps[2]])
    t = check(ctx, e, e, "nothing at all")
    assert t.n_bins == 0 and t.n_elem == 0


def test_more_loci_than_two_passes_of_each_grid(ctx):
    import torch
    lim = merge.limits()
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    rng = np.random.default_rng(24)
    # the small form: `threads` / 64 loci of 33..64 bins share a workgroup; the deep form: 2 workgroups per CU; the fill: a tile per locus here
    n_small, n_deep = 2 * cus * lim["grid_per_cu"] * (lim["threads"] // 64) + 5, 2 * cus * 2 + 3
    ps = []
    sizes = [33 + i % 2 if i < n_small else 65 + i % 7 for i in range(n_small + n_deep)]
    every = (rng.permutation(1 << 22)[:sum(n + n // 2 for n in sizes)] + 1).astype(np.uint32).reshape(-1, 1)   # distinct over all loci
    at = 0
    for i, n in enumerate(sizes):
        ps.append(MU.one_locus_pair(*MU.split_keys(every[at:at + n + n // 2], n // 2, n // 2, rng), 1 + i % 3, rng))
        at += n + n // 2
    order = rng.permutation(len(ps))
    a, b = MU.concat([ps[i] for i in order])
    t = check(ctx, a, b, "past two passes")
    assert t.n_loci > 2 * cus * lim["grid_per_cu"]
    # two calls in a row: the same bits
    MU.assert_same(run(ctx, a, b), {k: getattr(t, k) for k in ("row_off", "f_off") + merge.NAMES}, "again")


def test_duplicate_keys_and_mismatches_are_refused(ctx):
    rng = np.random.default_rng(25)
    k = MU.distinct_keys(rng, 400, 2)
    first, good = MU.one_locus_pair(k[:3], k[2:5], 2, rng), MU.one_locus_pair(*MU.split_keys(k[:20], 6, 6, rng), 3, rng)
    for n in (8, 200):                         # the small form, the deep form
        for dup_of in ("shared", "only"):
            for which in (0, 1):
                ka, kb = MU.split_keys(k[:n + n // 2], n // 2, n // 2, rng)
                mine, other = (ka, kb) if which == 0 else (kb, ka)
                in_other = np.array([tuple(x) in set(map(tuple, other)) for x in mine])
                src = np.flatnonzero(in_other if dup_of == "shared" else ~in_other)[:2]
                mine = mine.copy()
                mine[src[1]] = mine[src[0]]
                bad = MU.one_locus_pair(mine, other, 3, rng) if which == 0 else MU.one_locus_pair(other, mine, 3, rng)
                a, b = MU.concat([first, good, bad, good])
                with pytest.raises(_lib.SbgpuError, match=r"\(-1\): sbgpu_bins_merge_device: a duplicate bin key in locus 2"):
                    run(ctx, a, b)
                with pytest.raises(_lib.SbgpuError, match=r"\(-1\): sbgpu_bins_merge_shapes_host: a duplicate bin key in locus 2"):
                    merge.merge_host(a, b)
    a, b = good
    b3 = MU.Sample(b.iso_off, b.row_off, np.concatenate([b.key, b.key[:, :1]], axis=1), b.count, b.F)
    for x, y, text in ((a.without_X(), b3, "key_words"), (a.without_X(), MU.concat([first, good])[1].without_X(), "n_loci"),
                       (a.without_X(), MU.Sample([0, 4], b.row_off, b.key, b.count, np.zeros(4 * len(b.count))), "iso_off")):
        with pytest.raises(_lib.SbgpuError, match=r"\(-1\): sbgpu_bins_merge_device: the two samples differ in " + text):
            run(ctx, x, y)
    check(ctx, a, b, "behind the refusals")


def export(L, handle, kw):
    """keys, counts and pairs of a live handle (it stays alive)"""
    n_loci, n_iso, n_bins, n_elem, n_pairs, n_segs = (int(x) for x in diff.bins_info(L, handle)[:6])
    z = lambda n, dt: np.zeros(max(n, 1), dt)  # noqa: E731
    o = dict(row_off=z(n_loci + 1, np.int64), iso_off=z(n_loci + 1, np.int64), f_off=z(n_loci + 1, np.int64), count=z(n_bins, np.int32),
             key=np.zeros((max(n_bins, 1), kw), np.uint32), seg_off=z(n_pairs + 1, np.int64), seg_lens=z(n_segs, np.uint32), mask=z(n_pairs, np.uint32),
             iso_len=z(n_pairs, np.int32), out_index=z(n_pairs, np.int64))
    p = lambda k: o[k].ctypes.data  # noqa: E731
    _lib.check(L.sbgpu_bins_export(handle, p("row_off"), p("iso_off"), p("f_off"), p("count"), None, p("key"), None, None, p("seg_off"), p("seg_lens"),
                                   p("mask"), p("iso_len"), p("out_index")), "sbgpu_bins_export")
    o["count"], o["key"], o["n_elem"], o["n_pairs"] = o["count"][:n_bins], o["key"][:n_bins], n_elem, n_pairs
    return o


def oracle_weights(oracle, e, ins, read_len):
    """the oracle's bin weight of every exported pair under `ins`, scattered by out_index into a zeroed [n_elem]"""
    F = np.zeros(e["n_elem"])
    for p in range(e["n_pairs"]):
        segs = e["seg_lens"][e["seg_off"][p]:e["seg_off"][p + 1]]
        imps = [k for k in range(len(segs)) if (int(e["mask"][p]) >> k) & 1]
        F[e["out_index"][p]] = oracle.bin_weight(segs, imps, int(e["iso_len"][p]), read_len, ins)
    return F


SEVEN = ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters")


def host_grouped_handle(ctx):
    """A few synthetic loci through the exon-bin kernel, their words brought to the host and grouped there (sbgpu_bins_create): a
    live handle with bins whose keys and pairs are host memory"""
    from strawberry_amd import exonbin as eb, synth
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    loci = synth.make_gene_models(24, seed=3)
    hl, pairs = synth.make_fragments(loci, 80, seed=4)
    feats = [(l, eb.hit_features(lb, rb)) for l, (lb, rb) in zip(hl, pairs)]
    feats = [(l, f) for l, f in feats if f is not None]
    annot, hits = eb.Annotation(loci), eb.Hits([l for l, _ in feats], [f for _, f in feats])
    q = LocusQuantifier(annot, hits, InsertSize(250.0, 30.0), 75, ctx=ctx)
    q.assign_bins()
    compat = np.ascontiguousarray(q.d_compat.cpu().numpy().view(np.uint32)[:hits.n_hits].reshape(hits.n_hits, -1))
    key = np.ascontiguousarray(q.d_key.cpu().numpy().view(np.uint32)[:hits.n_hits].reshape(hits.n_hits, -1))
    a, h = annot._struct(), hits._struct()
    handle = C.c_void_p()
    _lib.check(ctx.L.sbgpu_bins_create(C.byref(a), C.byref(h), hits.mass.ctypes.data, compat.shape[1], key.shape[1], compat.ctypes.data, key.ctypes.data,
                                       C.byref(handle)), "sbgpu_bins_create")
    info = diff.bins_info(ctx.L, handle)
    assert info[2] > 0
    return handle


def bitwise(x, y, label, names=diff.NAMES):
    for k in names:
        p, q = getattr(x, k), getattr(y, k)
        np.testing.assert_array_equal(p.view(np.uint64) if p.dtype == np.float64 else p, q.view(np.uint64) if q.dtype == np.float64 else q,
                                      err_msg="%s %s" % (label, k))


def test_two_retained_samples_on_one_bin_table(ctx, oracle):
    from strawberry_amd import chain, em
    kw = dict(n_loci=400, n_frags=2e5, seed=31, resident=True, keep_bootstrap=True, min_isoform_frac=0.01)
    ctx_b, ctx_c = em.Context(0), em.Context(0)
    # two laws: A is given a Gaussian one, B builds the empirical law of its own hits (what the record must copy, histogram included)
    qa, qb, qc = chain.ChainQuantifier(ctx, sample_seed=31, **kw), chain.ChainQuantifier(ctx_b, sample_seed=32, empirical=True, **kw), None
    try:
        qa.step(), qb.step()
        before = [{k: getattr(q, k).copy() for k in SEVEN} for q in (qa, qb)]
        t = qa.differential_usage(qb, shared_bins=True, merged_want=None)
        m = t.merged
        # ---- maps and counts: by_hand fed the two handles' exported keys and counts
        ea, eb = export(ctx.L, qa.context_handle, qa.annot.key_words), export(ctx_b.L, qb.context_handle, qb.annot.key_words)
        lb = qb.law
        assert lb["use_emp"] == 1 and qa.law["use_emp"] == 0
        hist = lb["emp_hist"].astype(np.int64)
        assert hist[0] > 0 and hist[-1] > 0 and int(hist.sum()) == lb["total_reads"]
        law = {"a": oracle.make_insert(qa.insert.mean, qa.insert.sd),
               "b": oracle.make_insert(lb["mean"], lb["sd"], np.repeat(np.arange(lb["start_offset"], lb["end_offset"] + 1), hist))}
        w = {(x, y): oracle_weights(oracle, e, law[y], qa.read_len) for x, e in (("a", ea), ("b", eb)) for y in "ab"}   # (whose bins, whose law)
        sa = MU.Sample(ea["iso_off"], ea["row_off"], ea["key"], ea["count"], w["a", "a"], w["b", "a"])
        sb = MU.Sample(eb["iso_off"], eb["row_off"], eb["key"], eb["count"], w["b", "b"], w["a", "b"])
        want = MU.by_hand(sa, sb)
        # the laws tell: on the one-sided rows a sample's X is not the other sample's own weight
        for x, y, e, rows in (("b", "a", eb, m.row_b[m.row_a < 0]), ("a", "b", ea, m.row_a[m.row_b < 0])):
            K = np.repeat(np.diff(e["iso_off"]), np.diff(e["row_off"]))
            first = np.concatenate([[0], np.cumsum(K)])
            differs = [not np.array_equal(w[x, y][first[r]:first[r + 1]], w[x, x][first[r]:first[r + 1]]) for r in rows]
            assert len(rows) > 0 and sum(differs) > len(rows) // 2, (x, y, sum(differs), len(rows))
        for k in ("row_off", "f_off", "row_a", "row_b", "count_a", "count_b"):
            np.testing.assert_array_equal(getattr(m, k), want[k], err_msg=k)
        only_a, only_b = int(((m.row_b < 0)).sum()), int((m.row_a < 0).sum())
        print("union: %d rows, %d A-only, %d B-only" % (m.n_bins, only_a, only_b))
        assert only_a > 0 and only_b > 0
        loci_with = np.unique(np.searchsorted(m.row_off, np.flatnonzero((m.row_a < 0) | (m.row_b < 0)), side="right") - 1)
        assert len(loci_with) >= 1
        # ---- the weights: the oracle's, under the right sample's law; the zeros exact
        for k in ("F_a", "F_b"):
            got, ref = getattr(m, k), want[k]
            np.testing.assert_array_equal(got == 0.0, ref == 0.0, err_msg=k)
            nz = ref != 0.0
            err = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
            print(k, "worst relative error %.3g of %g" % (err.max(), RTOL))
            assert (err <= RTOL).all(), (k, float(err.max()))
        # ---- the differential result: sbgpu_em_diff_device on the merged device arrays, with a plan of the test's own
        plan = em.Plan(ctx_c, m.row_off, m.iso_off, m.f_off)
        d = m.device
        u = diff.em_diff_device(ctx_c, plan, d["count_a"], d["F_a"], plan, d["count_b"], d["F_b"], int(qa._out.d_keep), int(qb._out.d_keep))
        plan.close()
        bitwise(t, u, "the composition")
        assert (t.diff_status == diff.OK).sum() > 50
        # ---- neither record changed: the seven results, and every other stage still answers
        for q, was in zip((qa, qb), before):
            q.model_fit(), q.isoform_information(), q.isoform_support(), q.abundance_bootstrap(4, 3, replicates=False)
            for k in SEVEN:
                np.testing.assert_array_equal(getattr(q, k).view(np.uint8), was[k].view(np.uint8), err_msg=k)
        bitwise(qa.differential_usage(qb, shared_bins=True), t, "behind the other stages")
        # ---- a third object with the first's sample_seed: identity maps, and every result is shared_bins=False's
        qc = chain.ChainQuantifier(ctx_c, sample_seed=31, **kw)
        qc.step()
        same = qa.differential_usage(qc, shared_bins=True, merged_want=("row_a", "row_b"))
        np.testing.assert_array_equal(same.merged.row_a, np.arange(len(ea["count"])))
        np.testing.assert_array_equal(same.merged.row_b, np.arange(len(ea["count"])))
        bitwise(same, qa.differential_usage(qc), "identical samples")
        # ---- refusals: no retention (the existing text); a handle whose bins, keys and pairs are on the host
        plain = chain.ChainQuantifier(ctx_c, n_loci=400, n_frags=2e5, seed=31, resident=True)
        h = C.c_void_p()
        try:
            plain.step()
            with pytest.raises(_lib.SbgpuError, match="keep_bootstrap=True"):
                qa.differential_usage(plain, shared_bins=True)
            plain._resident_call(ctx_c.L, plain._ht, plain.hits.mass.data_ptr(), plain.hits.locus_hit_off.ctypes.data, plain.n_frags, h)
            for args in ((ctx, qa.context_handle, ctx_c, h), (ctx_c, h, ctx, qa.context_handle)):
                with pytest.raises(_lib.SbgpuError, match=r"\(-1\): sbgpu_model_diff_merged_device: this handle was made without retention \(sbgpu_bootstrap_keep was off"):
                    diff.model_diff_merged_device(*args)
        finally:
            if h:
                ctx_c.L.sbgpu_bins_destroy(h)
            plain.close()
        # a handle grouped on the host (sbgpu_bins_create) has neither keys nor pairs in HBM: refused on either side, and the caller's
        # struct keeps no device pointer of an earlier call
        hosted = host_grouped_handle(ctx_c)
        try:
            for args in ((ctx_c, hosted, ctx, qa.context_handle), (ctx, qa.context_handle, ctx_c, hosted)):
                with pytest.raises(_lib.SbgpuError, match=r"\(-6\): sbgpu_model_diff_merged_device: the handle's bin keys or \(bin, isoform\) pairs are not on the device"):
                    diff.model_diff_merged_device(*args)
            s, ms = _lib.sbgpu_em_diff_t(), _lib.sbgpu_bins_merged_t()
            s.d_lr_stat, ms.d_F_a, ms.n_bins = 8, 8, 3
            assert ctx.L.sbgpu_model_diff_merged_device(ctx.h, qa.context_handle, ctx_c.h, hosted, None, None, None, None, C.byref(s), C.byref(ms)) == _lib.SBGPU_EUNSUPPORTED
            assert not s.d_lr_stat and not ms.d_F_a and ms.n_bins == 0
        finally:
            ctx_c.L.sbgpu_bins_destroy(hosted)
        s = _lib.sbgpu_em_diff_t()
        assert ctx.L.sbgpu_model_diff_merged_device(ctx.h, qa.context_handle, ctx_b.h, qb.context_handle, None, None, None, None, None, None) == _lib.SBGPU_EINVAL
        assert ctx.L.sbgpu_model_diff_merged_device(ctx.h, None, ctx_b.h, qb.context_handle, None, None, None, None, C.byref(s), None) == _lib.SBGPU_EINVAL
        assert "sbgpu_model_diff_merged_device: null argument" in ctx.L.sbgpu_last_error().decode()
    finally:
        for q in (qa, qb, qc):
            if q is not None:
                q.close()
