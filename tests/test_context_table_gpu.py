"""The `-f` fragment-context table built on the device (sbgpu_context_table_keep / sbgpu_context_table_device,
csrc/context_device.h) from what a resident call leaves in HBM: against the reference's ctx.tsv files byte for byte,
against the host form (sbgpu_context_table_host on the handle of sbgpu_quantify_host over the same hits) array for array,
through the chunked stream, and the retention switch itself (off: the resident call is unchanged; on: the same bits)."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_util as B
import e2e_util as U
import exonbin_util as XU
import stream_util as S
from strawberry_amd import _lib, context
from strawberry_amd import exonbin as eb

pytestmark = pytest.mark.gpu
RL, MEAN, SD = 75, 250.0, 30.0
# run -> (law: "i" = -i 250/30, "se" = N(200, 80), None = empirical; long_read; min_isoform_frac), as the golden runs' command lines
RUNS = {"E2E": ("i", 0, 0.0), "E2E_LONG": ("i", 0, 0.0), "E2E_MASS": ("i", 0, 0.0), "E2E_FILTER": ("i", 0, 0.05), "E2E_EMP": (None, 0, 0.0),
        "E2E_SINGLE": ("se", 0, 0.0), "E2E_LONGREAD": ("se", 1, 0.0), "E2E_MINUS": ("i", 0, 0.0), "E2E_CHROMS": ("i", 0, 0.0),
        "E2E_BIAS": ("i", 0, 0.0)}
# unit masses, hits in uniq_hits() order: none of the device grouping's decline conditions can apply
MUST_BE_RESIDENT = ("E2E", "E2E_LONG", "E2E_EMP", "E2E_FILTER", "E2E_MINUS", "E2E_CHROMS")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def law_of(which):
    from strawberry_amd.quantify import InsertSize
    return {"i": InsertSize(MEAN, SD), "se": InsertSize(200.0, 80.0), None: None}[RUNS[which][0]]


def assert_same_table(a, b, what=""):
    assert a.n_rows == b.n_rows, what
    for k in ("locus_row_off", "locus_hits", "row_bin", "row_hits"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg="%s %s" % (what, k))
    # bitwise: every element is a copy of one (bin, isoform) weight of the same binweight_kernel, or 0.0
    np.testing.assert_array_equal(a.row_prob.view(np.uint64), b.row_prob.view(np.uint64), err_msg="%s row_prob" % what)


def text_of(t, bins, g, total_mapped, fpkm, frac, keep, seq_stats=None):
    names, ordered = g["names"], g["ordered"]
    coords = [c for l in range(bins.n_loci) for c in bins.bin_coords(l)]
    return context.format_table(t, "toy", total_mapped, names, [[n for n, _ in ordered[x]] for x in names], bins.row_off, bins.iso_off,
                                bins.f_off, lambda b: coords[b], fpkm, frac, keep=keep, seq_stats=seq_stats)


def toy(which):
    d = getattr(U, which)
    ordered, rows, gtf, theta_log = U.load(d)
    annot, hits, names, _ = XU.e2e_inputs(d, ordered)
    return dict(d=d, ordered=ordered, rows=rows, annot=annot, hits=hits, names=names)


def host_route(ctx, g, which, want):
    """A directory the resident entry declined: the chain stage by stage (LocusQuantifier), the host form on sbgpu_bins_create's handle."""
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    annot, hits = g["annot"], g["hits"]
    law = law_of(which)
    q = LocusQuantifier(annot, hits, law if law is not None else InsertSize(MEAN, SD), RL, long_read=bool(RUNS[which][1]), ctx=ctx)
    bins = q.assign_bins()
    compat = q.d_compat.cpu().numpy().view(np.uint32)[:hits.n_hits].reshape(hits.n_hits, -1)
    key = q.d_key.cpu().numpy().view(np.uint32)[:hits.n_hits].reshape(hits.n_hits, -1)
    if law is None:
        q.insert = InsertSize.from_frag_lens(eb.frag_lens(annot, hits, compat))
    F = q.bin_weights().cpu().numpy()
    res = q.solve(hits.total_mapped, min_isoform_frac=RUNS[which][2])
    a, h = annot._struct(), hits._struct()
    handle = C.c_void_p()
    _lib.check(ctx.L.sbgpu_bins_create(C.byref(a), C.byref(h), hits.mass.ctypes.data, compat.shape[1], key.shape[1], compat.ctypes.data,
                                       key.ctypes.data, C.byref(handle)), "sbgpu_bins_create")
    try:
        t = context.context_table_host(handle, compat, F=F, keep=res["keep"], status=res["status"])
    finally:
        ctx.L.sbgpu_bins_destroy(handle)
    host_bins = eb.LocusBins(annot, hits, compat, key)
    assert text_of(t, host_bins, g, hits.total_mapped, res["fpkm"], res["frac"], res["keep"]) == want


@pytest.mark.parametrize("which", list(RUNS))
def test_device_table_reproduces_the_reference_files(ctx, which):
    """Each golden run's unique hits through sbgpu_quantify_resident with retention on, sbgpu_context_table_device, the
    formatter: the reference's ctx.tsv byte for byte (E2E_BIAS: with sbgpu_binseq_device's statistics indexed through row_bin)."""
    from strawberry_amd.quantify import quantify_host, quantify_resident
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    law, long_read, min_frac = law_of(which), bool(RUNS[which][1]), RUNS[which][2]
    want = open(os.path.join(g["d"], "ctx.tsv")).read()
    try:
        r = quantify_resident(annot, hits, law, RL, hits.total_mapped, long_read=long_read, ctx=ctx, min_isoform_frac=min_frac, with_context=True)
    except _lib.SbgpuError as e:
        if "sbgpu_quantify_resident failed (-6)" not in str(e):
            raise
        # the device grouping may decline (fractional masses next to another obstacle, ...): the resident entry then says so
        # and the directory goes through the host form
        assert which not in MUST_BE_RESIDENT, (which, str(e))
        assert "the device grouping does not cover these hits" in str(e) and "use sbgpu_quantify_host" in str(e), str(e)
        host_route(ctx, g, which, want)
        return
    t, bins = r["context"], r["bins"]
    assert bins.grouped_on_device and t.n_rows == len(g["rows"])
    stats = None
    if which == "E2E_BIAS":
        import torch
        from strawberry_amd.binseq import bin_segments, bin_sequence_stats_device
        from test_binseq_oracle import load_bias_run
        genome, _ = load_bias_run()
        dev = torch.device("cuda", ctx.device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)   # noqa: E731
        off, sl, sr = bin_segments(bins)
        gc, ent, fl, err = bin_sequence_stats_device(up(np.frombuffer(genome, np.uint8).copy(), np.uint8), 1, up(off.astype(np.int64), np.int64),
                                                     up(sl, np.int32), up(sr, np.int32), device=ctx.device)
        torch.cuda.synchronize(dev)
        assert int(err.item()) == 0
        stats = (gc.cpu().numpy(), ent.cpu().numpy(), fl.cpu().numpy())
    assert text_of(t, bins, g, r["total_mapped_reads"], r["fpkm"], r["frac"], r["keep"], stats) == want
    if which == "E2E_FILTER":
        assert (r["keep"] == 0).sum() == 5
    # and the host form on the host entry's handle over the same hits: the same arrays
    h = quantify_host(annot, hits, law, RL, long_read=long_read, ctx=ctx, context_keep=r["keep"], context_status=r["status"])
    assert_same_table(t, h["context"], which)


def test_device_table_equals_host_table_on_the_chain_sample(ctx):
    """A few thousand loci of the chain workload with isoforms erased (min_isoform_frac 0.01): locus_row_off, locus_hits, row_bin,
    row_hits exactly and row_prob bitwise equal to the host form's on sbgpu_quantify_host over the same hits."""
    from strawberry_amd import chain
    from strawberry_amd.quantify import InsertSize, quantify_host
    q = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01, keep_context=True)
    try:
        q.step()
        t = q.context_table()
        keep, status = q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        assert (keep == 0).sum() > 20 and t.n_rows > 10000
        t2 = q.context_table()                  # (the table call leaves what it read alone)
        assert_same_table(t, t2, "again")
        hits = q.hits.host_hits(q.n_loci)
        h = quantify_host(q.annot, hits, InsertSize(250.0, 30.0), 75, ctx=ctx, context_keep=keep, context_status=status)
        np.testing.assert_array_equal(h["theta"], q.theta[:q.n_iso])
        assert_same_table(t, h["context"], "chain sample")
        assert int(t.locus_hits.sum()) <= hits.n_hits and int(t.row_hits.sum()) == int(t.locus_hits.sum())
        # the host entry was this context's next quantify call: what the resident call kept is gone, and the call says so
        with pytest.raises(_lib.SbgpuError, match="stale handle"):
            q.context_table()
    finally:
        q.close()


def wide_sample():
    """One locus of 70 segments whose fragments make > 1000 bins from > 16384 hits (key words: 3; several count work items; the
    sort above the all-pairs threshold), one locus of 40 isoforms (compat words: 2), five narrow loci."""
    rng = np.random.default_rng(2718)
    loci, hl, feats = [], [], []
    # locus 0: one isoform of 70 exons of 30 bases, 100 apart
    base = 100000
    ex = [(base + 130 * k, base + 130 * k + 29) for k in range(70)]
    loci.append([ex])

    def mate(i, a, o1, o2):
        """a read over exons i .. i + a: from o1 bases into the first to o2 bases before the end of the last"""
        if a == 0:
            return [(ex[i][0] + o1, ex[i][1] - o2)]
        return [(ex[i][0] + o1, ex[i][1])] + [ex[k] for k in range(i + 1, i + a)] + [(ex[i + a][0], ex[i + a][1] - o2)]
    combos = set()
    while len(combos) < 1500:
        i, a, gap, b = int(rng.integers(0, 60)), int(rng.integers(0, 3)), int(rng.integers(1, 6)), int(rng.integers(0, 3))
        if i + a + gap + b < 70:
            combos.add((i, a, i + a + gap, b))
    for (i, a, j, b) in sorted(combos):
        for _ in range(14):
            f = eb.hit_features(mate(i, a, int(rng.integers(0, 12)), int(rng.integers(0, 6))), mate(j, b, int(rng.integers(0, 6)), int(rng.integers(0, 12))))
            assert f is not None
            hl.append(0)
            feats.append(f)
    # locus 1: 8 exons, 40 isoforms (distinct subsets that keep the first and the last)
    base = 300000
    ex8 = [(base + 400 * k, base + 400 * k + 119) for k in range(8)]
    isos = []
    while len(isos) < 40:
        pick = [e for k, e in enumerate(ex8) if k in (0, 7) or rng.random() < 0.6]
        if pick not in isos:
            isos.append(pick)
    loci.append(isos)
    for _ in range(3000):
        iso = isos[int(rng.integers(0, 40))]
        k = int(rng.integers(0, len(iso) - 1))
        x, y = iso[k], iso[k + 1]
        o = int(rng.integers(0, 30))
        f = eb.hit_features([(x[1] - 40 - o, x[1]), (y[0], y[0] + 33 - o)], [(y[0] + 50, y[0] + 100 + o)])
        if f is not None:
            hl.append(1)
            feats.append(f)
    # loci 2 .. 6: two isoforms each
    for l in range(2, 7):
        base = 300000 + 100000 * l
        a_iso = [(base, base + 199), (base + 500, base + 699), (base + 1000, base + 1199)]
        loci.append([a_iso, [a_iso[0], a_iso[2]]])
        for _ in range(150):
            o = int(rng.integers(0, 120))
            two = rng.random() < 0.5
            f = eb.hit_features([(base + 100 + o // 2, base + 199), (base + 1000 if two else base + 500, (base + 1000 if two else base + 500) + 30 + o // 3)],
                                [((base + 1000) + 60 + o // 2, base + 1000 + 130 + o // 2)])
            if f is not None:
                hl.append(l)
                feats.append(f)
    annot = eb.Annotation(loci)
    keyed = sorted(set((hl[i], feats[i][1][0], feats[i][2][-1], tuple(map(tuple, feats[i]))) for i in range(len(hl))))
    hits = eb.Hits([k[0] for k in keyed], [tuple(list(x) for x in k[3]) for k in keyed])
    return annot, hits


def test_wide_keys_many_isoforms_a_split_locus_and_the_sort(ctx):
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    annot, hits = wide_sample()
    assert annot.key_words == 3 and annot.compat_words == 2
    in_wide = int((hits.hit_locus == 0).sum())
    assert in_wide > 16384          # csrc/context_device.h: kCtxItemHits -- the locus is several count work items
    law = InsertSize(150.0, 60.0)      # (the wide locus' fragments are 60 .. 300 bases long)
    r = quantify_resident(annot, hits, law, RL, hits.n_hits, ctx=ctx, min_isoform_frac=0.05, with_context=True)
    t, bins = r["context"], r["bins"]
    assert bins.row_off[1] - bins.row_off[0] > 1000 and bins.grouped_on_device
    assert (r["keep"][annot.iso_off[1]:annot.iso_off[2]] == 0).any()          # isoforms of the 40 were erased
    h = quantify_host(annot, hits, law, RL, ctx=ctx, context_keep=r["keep"], context_status=r["status"])
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    assert_same_table(t, h["context"], "wide")
    assert t.locus_row_off[1] > 1000 and (np.diff(t.locus_row_off) > 0).all()
    # the wide locus' rows, independently: Python's order of the coordinate tuples; every hit of it qualifies
    coords = bins.bin_coords(0)
    got = [tuple(coords[b]) for b in t.row_bin[:t.locus_row_off[1]].tolist()]
    assert got == sorted(got) and len(set(got)) == len(got) == bins.row_off[1]
    assert int(t.locus_hits[0]) == in_wide == int(t.row_hits[:t.locus_row_off[1]].sum())


def stream_table(s, ctx, feed, chunk_bytes):
    """s (stream_util.Sample) through sbgpu_front_stream_*, `feed(L, fs)` making the pushes, retention on:
    -> (table, LocusBins, outputs) of sbgpu_front_stream_end's handle."""
    L = ctx.L
    res, out, par, used = s._outputs()
    fs, h = C.c_void_p(), C.c_void_p()
    context.context_table_keep(ctx, True)
    try:
        _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), int(chunk_bytes), C.byref(fs)), "sbgpu_front_stream_begin")
        try:
            alive = feed(L, fs)     # noqa: F841  (the pushes' bytes stay alive until the stream is gone)
            _lib.check(L.sbgpu_front_stream_end(fs, C.byref(s.an), C.byref(s.ins) if s.ins is not None else None, s.read_len, s.long_read,
                                                C.byref(par), None, C.byref(used), C.byref(out), C.byref(h)), "sbgpu_front_stream_end")
            r = s._collect(res, out, used)
            try:
                t = context.context_table_device(ctx, h)
            except Exception:
                L.sbgpu_bins_destroy(h)
                raise
            dh = _lib.sbgpu_hits_t()
            _lib.check(L.sbgpu_front_stream_hits(fs, C.byref(dh), None, None), "sbgpu_front_stream_hits")
            bins = eb.LocusBins.__new__(eb.LocusBins)
            bins._export(L, s.annot, h, int(dh.n_hits), s.annot.compat_words, s.annot.key_words, with_hit_bin=False)   # destroys the handle
        finally:
            L.sbgpu_front_stream_destroy(fs)
    finally:
        context.context_table_keep(ctx, False)
    return t, bins, r


@pytest.mark.parametrize("which", ["E2E_FILTER", "E2E_EMP"])
def test_stream_end_keeps_the_table_inputs(ctx, which):
    """sbgpu_front_stream_end with retention on: the table of the resident entry on the whole sample's unique hits, from
    records pushed inflated (two schedules) and as BGZF members, and the reference's file."""
    import test_front_stream_gpu as T
    from strawberry_amd import bam
    from strawberry_amd.quantify import quantify_resident
    s, g = T.toy(which)
    hits = g["hits"]
    want = quantify_resident(s.annot, hits, s.insert, RL, hits.total_mapped, long_read=bool(s.long_read), ctx=ctx,
                             min_isoform_frac=s.min_isoform_frac, with_context=True)
    want_text = open(os.path.join(g["d"], "ctx.tsv")).read()
    assert text_of(want["context"], want["bins"], g, want["total_mapped_reads"], want["fpkm"], want["frac"], want["keep"]) == want_text

    def pushes_of(pushes):
        def feed(L, fs):
            alive = []
            for a, b in pushes:
                part = np.ascontiguousarray(s.raw[s.off[a]:s.off[b]])
                ro = np.ascontiguousarray(s.off[a:b + 1] - s.off[a])
                alive.append((part, ro))
                _lib.check(L.sbgpu_front_stream_push(fs, part.ctypes.data if part.size else None, int(part.size), ro.ctypes.data, int(b - a)),
                           "sbgpu_front_stream_push")
            return alive
        return feed
    schedules = dict(S.schedules(s.n, s.first, s.past, seed=3))
    for name in ("one", "starts"):
        pushes = schedules[name]
        t, bins, r = stream_table(s, ctx, pushes_of(pushes), S.chunk_bytes_for(s.off, pushes, s.past))
        assert_same_table(t, want["context"], "%s push %s" % (which, name))
        for k in S.OUT_KEYS:
            np.testing.assert_array_equal(r[k], want[k], err_msg=k)
        assert text_of(t, bins, g, r["total_mapped_reads"], r["fpkm"], r["frac"], r["keep"]) == want_text
    head = B.header_bytes([(c, 10_000_000) for c in g["chroms"]])
    file = np.frombuffer(B.bgzf_compress(head + s.raw.tobytes(), block=6000), np.uint8)
    blk, out = bam.bgzf_index(file)
    _, first = bam.read_header(file, (blk, out))
    n = blk.size - 1

    def feed_bgzf(L, fs):
        alive = []
        for a, b in ((0, n // 2), (n // 2, n)):
            part = np.ascontiguousarray(file[blk[a]:blk[b]])
            tb, to = blk[a:b + 1].copy(), out[a:b + 1].copy()
            alive.append((part, tb, to))
            _lib.check(L.sbgpu_front_stream_push_bgzf(fs, part.ctypes.data if part.size else None, int(part.size), tb.ctypes.data, to.ctypes.data,
                                                      int(b - a), max(0, first - int(out[a]))), "sbgpu_front_stream_push_bgzf")
        return alive
    t, bins, r = stream_table(s, ctx, feed_bgzf, max(S.MIN_CHUNK, len(head) + int(s.raw.size)))
    assert_same_table(t, want["context"], "%s push_bgzf" % which)
    assert text_of(t, bins, g, r["total_mapped_reads"], r["fpkm"], r["frac"], r["keep"]) == want_text


# the kernel stages of a resident call under a given law, in stream order, as they were before retention existed
STAGES = ["exonbin_kernel", "bins_accum_kernel", "bins_scan_*_kernel<rows> + bins_pack_kernel",
          "bins_pairs_kernel<count> + bins_scan_*_kernel<pairs>", "bins_pairs_kernel<fill>", "binweight_kernel", "em kernels", "abundance + tpm"]


def test_retention_switch(ctx):
    """Off (the default): the resident call's stages are the list above and the table call refuses its handle.  On: theta, FPKM,
    Frac, TPM, keep, status and iters are the same bits; resident + table twice on one context give the same arrays (nothing
    stale in the per-bin scratch); a handle whose call is no longer the context's last is refused."""
    from strawberry_amd import chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=600, n_frags=600 * 250, seed=12, resident=True, min_isoform_frac=0.01)
    outs = lambda: {k: getattr(q, k)[:(q.n_loci if k in ("status", "iters") else q.n_iso)].copy() for k in S.OUT_KEYS}   # noqa: E731

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        return h

    def table(h):
        s = _lib.sbgpu_context_table_t()
        return L.sbgpu_context_table_device(ctx.h, h, None, C.byref(s)), L.sbgpu_last_error().decode()
    handles = []
    try:
        assert list(q.stage_ms()) == STAGES
        h0 = call()
        handles.append(h0)
        off = outs()
        rc, why = table(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
        context.context_table_keep(ctx, True)
        assert list(q.stage_ms()) == STAGES             # (hit -> bin is made by a kernel outside the timed stages)
        h1 = call()
        handles.append(h1)
        on = outs()
        for k in S.OUT_KEYS:
            np.testing.assert_array_equal(on[k].view(np.uint64 if on[k].dtype == np.float64 else np.int32),
                                          off[k].view(np.uint64 if off[k].dtype == np.float64 else np.int32), err_msg=k)
        rc, why = table(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
        t1 = context.context_table_device(ctx, h1)
        h2 = call()
        handles.append(h2)
        rc, why = table(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        t2 = context.context_table_device(ctx, h2)
        assert_same_table(t1, t2, "twice")
        assert t1.n_rows > 3000
        context.context_table_keep(ctx, False)          # off: later calls keep nothing; what the last one kept stays until then
        assert_same_table(context.context_table_device(ctx, h2), t1, "after switching off")
        h3 = call()
        handles.append(h3)
        for h, why_want in ((h2, "stale handle"), (h3, "without retention")):
            rc, why = table(h)
            assert rc == _lib.SBGPU_EINVAL and why_want in why, why
    finally:
        context.context_table_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()


def test_another_entry_in_the_contexts_scratch_ends_what_was_kept(ctx):
    """Not only sbgpu_quantify_* reuses the context's scratch: a device grouping of another sample on the same context
    (sbgpu_bins_create_device) between the resident call and the table call makes the handle stale too -- SBGPU_EINVAL, not a
    table read from reused memory.  And a quantifier's keep_context leaves the shared context's switch as it found it."""
    from strawberry_amd import chain, exonbin as eb, synth
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=9, resident=True, keep_context=True)
    plain = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=9, resident=True, pin=False)
    try:
        q.step()
        assert q.context_table().n_rows > 300
        loci = synth.make_gene_models(6, seed=3)
        hl, pairs = synth.make_fragments(loci, 40, seed=4)
        feats = [(l, eb.hit_features(lb, rb)) for l, (lb, rb) in zip(hl, pairs)]
        feats = [(l, f) for l, f in feats if f is not None]
        other = LocusQuantifier(eb.Annotation(loci), eb.Hits([l for l, _ in feats], [f for _, f in feats]), InsertSize(250.0, 30.0), 75, ctx=ctx)
        other.assign_bins()
        with pytest.raises(_lib.SbgpuError, match="stale handle"):
            q.context_table()
        # the switch was on for q's own call only: a plain quantifier on the same context keeps nothing
        h = C.c_void_p()
        plain._resident_call(L, plain._ht, plain.hits.mass.data_ptr(), plain.hits.locus_hit_off.ctypes.data, plain.n_frags, h)
        s = _lib.sbgpu_context_table_t()
        rc, why = L.sbgpu_context_table_device(ctx.h, h, None, C.byref(s)), L.sbgpu_last_error().decode()
        L.sbgpu_bins_destroy(h)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
    finally:
        plain.close()
        q.close()
