"""The chunked record stream (sbgpu_front_stream_begin / push / end, csrc/front_stream_api.hip) at its chunk edges and on the
reference program's own runs.  The stream carries a cluster's records from one window to the next; its results must be those
of the resident entries over the whole sample, bit for bit, whatever the cuts: one push, one record per push, cuts at every
cluster's first record and around its last, random cuts, chunks that complete nothing, empty pushes anywhere, the caller's
record offsets or none.  The toy runs (tests/golden/e2e_toy*) pin the results to the reference's theta log and GTF; records
the reference drops are spliced in where the stream cuts; a cluster larger than 64 KB meets the capacity edge; a 2 500-locus
sample and a two-reference stream check the same at scale.  Helpers: tests/stream_util.py."""
import numpy as np
import pytest

import bam_util as B
import e2e_util as U
import exonbin_util as XU
import stream_util as S

pytestmark = pytest.mark.gpu
RL, MEAN, SD = 75, 250.0, 30.0

# run -> (unique_only, law: "i" = -i 250/30, "se" = N(200, 80) (a single-end or long-read library), None = the empirical law
# the stream builds; long_read; min_isoform_frac), as oracle/sbgpu_front_shim.cpp passes them for the golden runs' command lines
RUNS = {
    "E2E": (True, "i", 0, 0.0),
    "E2E_LONG": (True, "i", 0, 0.0),
    "E2E_MASS": (False, "i", 0, 0.0),          # --allow-multimapped-hits
    "E2E_FILTER": (True, "i", 0, 0.05),        # -e 0.05
    "E2E_EMP": (True, None, 0, 0.0),
    "E2E_SINGLE": (True, "se", 0, 0.0),
    "E2E_LONGREAD": (True, "se", 1, 0.0),
    "E2E_MINUS": (True, "i", 0, 0.0),
    "E2E_CHROMS": (True, "i", 0, 0.0),
}


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def toy(which, extra_refs=0):
    """-> (Sample of the run's records, the run's goldens and unique hits)."""
    from strawberry_amd import bam
    from strawberry_amd.quantify import InsertSize
    d = getattr(U, which)
    unique_only, law, long_read, min_frac = RUNS[which]
    ordered, rows, gtf, theta_log = U.load(d)
    annot, hits, names, _ = XU.e2e_inputs(d, ordered)
    raw, chroms, clusters = B.toy_run_as_bam_records(d, names)
    insert = {"i": InsertSize(MEAN, SD), "se": InsertSize(200.0, 80.0), None: None}[law]
    s = S.Sample(raw, bam.index(raw), clusters, len(chroms) + extra_refs, annot, insert, RL, long_read, unique_only, min_frac)
    return s, dict(d=d, ordered=ordered, rows=rows, gtf=gtf, theta_log=theta_log, hits=hits, names=names, chroms=chroms, clusters=clusters)


def check_info(s, r, pushes, one_push=False, accepted=None):
    i = r["info"]
    assert i["records"] == s.n and i["clusters_finished"] == s.n_loci and i["ended"] == 1, i
    assert i["chunks"] == sum(1 for a, b in pushes if s.off[b] > s.off[a]), i
    assert i["most_bytes_carried"] <= r["chunk_bytes"] == i["chunk_bytes"], i
    if one_push:
        assert i["records_decoded_twice"] == 0, i
    if accepted is not None:
        assert i["accepted_records"] == accepted, i


def check_reference_run(which, r, g):
    """r's store and abundances against the reference's run: the unique hits exactly, theta within 1e-6 of its log, FPKM /
    Frac / TPM and the kept set against its GTF (the bars of test_chain_from_fragments_reproduces_reference_run)."""
    hits, h = g["hits"], r["hits"]
    for k in S.HIT_KEYS:
        np.testing.assert_array_equal(h[k], getattr(hits, k), err_msg="%s %s" % (which, k))
    assert r["info"]["mapped_reads"] == g["rows"][0]["total_mapped"] == r["total_mapped_reads"]
    names, ordered, gtf = g["names"], g["ordered"], g["gtf"]
    iso_off = np.concatenate([[0], np.cumsum([len(ordered[n]) for n in names])])
    for l, ref_theta in enumerate(g["theta_log"]):
        th = r["theta"][iso_off[l]:iso_off[l + 1]]
        assert np.abs(th - np.array(ref_theta)).max() < 1e-6, (which, names[l], th, ref_theta)
    tx = [t for n in names for t, _ in ordered[n]]
    assert set(gtf) == set(t for t, k in zip(tx, r["keep"]) if k), which
    assert (r["keep"] == 0).sum() == (5 if which == "E2E_FILTER" else 0)
    for t, f, fr, tp, k in zip(tx, r["fpkm"], r["frac"], r["tpm"], r["keep"]):
        if k:
            assert abs(f - float(gtf[t][0])) <= 1e-5 * max(1.0, f), (which, t)
            assert abs(fr - float(gtf[t][1])) < 2e-6, (which, t)
            assert abs(tp - float(gtf[t][2])) <= 1e-5 * max(1.0, tp), (which, t)


@pytest.mark.parametrize("which", list(RUNS))
def test_reference_runs_through_the_stream_under_every_schedule(ctx, which):
    """Each run's records, pushed whole, give the reference's unique hits, theta, FPKM, Frac, TPM and kept set, and every
    array of the resident pass bit for bit (E2E, E2E_EMP: also sbgpu_quantify_resident on the stream's own store, the law
    included); every schedule, with the caller's offsets and without, gives the one-push results bit for bit.
    Catches: a cluster finished before a read behind its end was seen, carried records' offsets not rebased, an empty push or a
    window of the carry alone mis-served, the library's own record index (rec_off NULL) differing from the caller's, an empty
    push counted as a chunk (info[7]; fixed with these tests)."""
    s, g = toy(which)
    one_pushes = [(0, s.n)]
    one = s.run_stream(ctx, one_pushes)
    check_info(s, one, one_pushes, one_push=True, accepted=s.n)
    check_reference_run(which, one, g)
    res = s.resident_pass(ctx)
    S.assert_same(one, res, "%s resident" % which)
    assert res["info"]["accepted_records"] == s.n
    if which in ("E2E", "E2E_EMP"):
        from strawberry_amd import exonbin as eb
        from strawberry_amd.quantify import quantify_resident
        h = one["hits"]
        hits = eb.Hits.from_arrays(h["hit_locus"], h["feat_off"], h["feat_code"], h["feat_left"], h["feat_right"], h["mass"])
        q = quantify_resident(s.annot, hits, s.insert, RL, one["info"]["mapped_reads"], long_read=bool(s.long_read), ctx=ctx,
                              min_isoform_frac=s.min_isoform_frac)
        for k in S.OUT_KEYS:
            np.testing.assert_array_equal(q[k], one[k], err_msg=k)
        assert (q["total_fpkm"], q["total_mapped_reads"]) == (one["total_fpkm"], one["total_mapped_reads"])
        law = dict(q["insert"], use_emp=int(q["insert"]["use_emp"]))
        S.assert_same_law(law, one["law"], which)
        if which == "E2E_EMP":
            assert one["law"]["use_emp"] == 1 and one["law"]["total_reads"] > 1000
    for name, pushes in S.schedules(s.n, s.first, s.past, seed=list(RUNS).index(which)):
        for give_off in (True, False):
            r = s.run_stream(ctx, pushes, give_off=give_off)
            what = "%s %s rec_off=%s" % (which, name, give_off)
            S.assert_same(r, one, what)
            check_info(s, r, pushes, one_push=name == "one", accepted=s.n)
            if name in ("ends", "each", "starts"):
                assert r["info"]["records_decoded_twice"] > 0, what


@pytest.mark.parametrize("which", ["E2E_EMP", "E2E_CHROMS"])
def test_dropped_and_outside_records_at_chunk_edges(ctx, oracle, which):
    """Records the reference drops (unmapped with a placed mate, unmapped at the tail, secondary, QC-fail -- which ones are
    dropped is the oracle decoder's word) and records outside every cluster (intergenic pairs, pairs on a reference without
    clusters) spliced into the run, cut at every schedule: the resident pass over the same records bit for bit; the accepted
    count the oracle's; where the spliced records are dropped or outside every cluster, the clean run's hits, theta and law.
    Catches: a carry that starts at a dropped record, reads behind the last cluster left out of accepted_records (info[1];
    fixed with these tests) or carried wrongly, an empty last push behind reads that every cluster is finished before."""
    clean, g = toy(which)
    want_clean = clean.resident_pass(ctx)
    n_chroms = len(g["chroms"])
    c_ref, c_left, c_right, _ = g["clusters"]
    raw, off, kinds = S.splice(clean.raw, c_ref, c_left, c_right, n_chroms, seed=7)
    unique_only = RUNS[which][0]
    o = oracle.bam_decode(raw, off, n_ref=n_chroms + 1, unique_only=unique_only)
    accepted = o["status"] == 0
    spliced = np.array([k is not None for k in kinds])
    assert set(k for k in kinds if k) >= {"unmapped-mate", "secondary", "qcfail", "intergenic", "no-cluster-ref", "unmapped-tail"}
    assert not accepted[np.array([k in ("unmapped-mate", "unmapped-tail") for k in kinds])].any()
    assert accepted[np.array([k in ("intergenic", "no-cluster-ref") for k in kinds])].all()
    s = S.Sample(raw, off, g["clusters"], n_chroms + 1, clean.annot, clean.insert, RL, clean.long_read, unique_only, clean.min_isoform_frac)
    res = s.resident_pass(ctx)
    assert res["info"]["accepted_records"] == int(accepted.sum())
    # inside a cluster and accepted: may change the cluster's hits (the rest must not)
    keys = s.keys
    inside = np.zeros(s.n, bool)
    for r_, lo, hi in zip(c_ref, c_left, c_right):
        inside |= (keys >= ((int(r_) << 32) | int(lo))) & (keys <= ((int(r_) << 32) | int(hi)))
    benign = ~spliced | ~accepted | ~inside
    if benign.all():
        S.assert_same(res, want_clean, "%s spliced vs clean" % which)
    else:
        keep = np.flatnonzero(benign)
        part = np.concatenate([raw[off[i]:off[i + 1]] for i in keep])
        from strawberry_amd import bam
        b = S.Sample(part, bam.index(part), g["clusters"], n_chroms + 1, clean.annot, clean.insert, RL, clean.long_read, unique_only,
                     clean.min_isoform_frac)
        S.assert_same(b.resident_pass(ctx), want_clean, "%s benign spliced vs clean" % which)
        S.assert_same(b.run_stream(ctx, S.from_cuts(b.n, [b.n // 3, b.n])), want_clean, "%s benign spliced stream vs clean" % which)
    for name, pushes in S.schedules(s.n, s.first, s.past, seed=11):
        chunk = S.chunk_bytes_for(s.off, pushes, s.past, accepted)
        for give_off in (True, False):
            r = s.run_stream(ctx, pushes, give_off=give_off, chunk_bytes=chunk)
            what = "%s spliced %s rec_off=%s" % (which, name, give_off)
            S.assert_same(r, res, what)
            check_info(s, r, pushes, one_push=name == "one", accepted=int(accepted.sum()))


def test_trailing_clusters_without_reads(ctx):
    """E2E with one more cluster (and locus) behind its last record: a cluster no read is ever offered to.  Pushed whole, whole
    then an empty push, and under every schedule: the resident pass over the same records bit for bit, the store's cluster
    offsets included -- the read-less cluster ends where the store ends.  (Every window before the last carries the last
    cluster's reads, which no read behind it completes, so the read-less cluster is finished by the last window.)"""
    from strawberry_amd import exonbin as eb
    base, g = toy("E2E")
    names, ordered = g["names"], g["ordered"]
    c_ref, c_left, c_right, c_strand = (list(x) for x in g["clusters"])
    shift = max(c_right) + 1_000_000 - min(e[0] for _, ex in ordered[names[-1]] for e in ex)
    extra = [[(a + shift, b + shift) for a, b in ex] for _, ex in ordered[names[-1]]]
    annot = eb.Annotation([[ex for _, ex in ordered[n]] for n in names] + [extra])
    clusters = (c_ref + [c_ref[-1]], c_left + [min(e[0] for ex in extra for e in ex)], c_right + [max(e[1] for ex in extra for e in ex)],
                c_strand + [c_strand[-1]])
    s = S.Sample(base.raw, base.off, clusters, base.opts.n_ref, annot, base.insert, RL)
    assert s.first[-1] == s.past[-1] == s.n                  # nothing offered to the last cluster
    res = s.resident_pass(ctx)
    n_hits = len(res["hits"]["hit_locus"])
    assert res["hits"]["locus_hit_off"][-2] == res["hits"]["locus_hit_off"][-1] == n_hits > 0
    sch = dict(S.schedules(s.n, s.first, s.past, seed=23))
    for name in ("one", "all-then-empty", "empty-first-middle-last", "ends", "random0"):
        for give_off in (True, False):
            r = s.run_stream(ctx, sch[name], give_off=give_off)
            S.assert_same(r, res, "read-less last cluster, %s rec_off=%s" % (name, give_off))
            check_info(s, r, sch[name], one_push=name == "one", accepted=s.n)


@pytest.mark.parametrize("pushes", ["none", "empty", "refused-then-empty"])
def test_stream_without_accepted_reads_finishes_every_cluster(ctx, pushes):
    """The only way to a last window of nothing (no carry, an empty or no last push) with clusters left over: no accepted read
    before it -- a window that holds reads always carries some while a cluster is left.  The stream has no hits and no mapped
    reads, so end() refuses the pass as sbgpu_quantify_resident does; but every cluster is finished with an empty hit range.
    Catches: the last window of nothing returning with the clusters unfinished (info[8] was 0; fixed with these tests)."""
    import ctypes as C
    from strawberry_amd import _lib
    base, _ = toy("E2E")
    L = ctx.L
    raw = np.frombuffer(b"".join(B.record(-1, -1, 1 | 4 | 8 | (0x40 if j % 2 else 0x80), "unplaced%d" % j, []) for j in range(6)), np.uint8).copy()
    from strawberry_amd import bam
    off = bam.index(raw)
    plan = {"none": [], "empty": [(0, 0), (0, 0)], "refused-then-empty": [(0, off.size - 1), (off.size - 1, off.size - 1)]}[pushes]
    s = S.Sample(raw, off, (base.c_ref, base.c_left, base.c_right, base.c_strand), base.opts.n_ref, base.annot, base.insert, RL)
    with pytest.raises(_lib.SbgpuError):
        s.resident_pass(ctx)
    res, out, par, used = s._outputs()
    fs, h = C.c_void_p(), C.c_void_p()
    _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), S.MIN_CHUNK, C.byref(fs)), "sbgpu_front_stream_begin")
    try:
        keep = []
        for a, b in plan:
            part, ro = np.ascontiguousarray(raw[off[a]:off[b]]), np.ascontiguousarray(off[a:b + 1] - off[a])
            keep.append((part, ro))
            _lib.check(L.sbgpu_front_stream_push(fs, part.ctypes.data if part.size else None, int(part.size), ro.ctypes.data, int(b - a)),
                       "sbgpu_front_stream_push")
        rc = L.sbgpu_front_stream_end(fs, C.byref(s.an), C.byref(s.ins), s.read_len, 0, C.byref(par), None, C.byref(used), C.byref(out), C.byref(h))
        assert rc != 0, "a pass without mapped reads is refused"
        info = (C.c_int64 * 16)()
        _lib.check(L.sbgpu_front_stream_info(fs, info), "sbgpu_front_stream_info")
        hoff = C.c_void_p()
        _lib.check(L.sbgpu_front_stream_hits(fs, None, None, C.byref(hoff)), "sbgpu_front_stream_hits")
        hit_off = np.ctypeslib.as_array(C.cast(hoff, C.POINTER(C.c_int64)), shape=(s.n_loci + 1,)).copy()
    finally:
        L.sbgpu_front_stream_destroy(fs)
    n = off.size - 1 if pushes == "refused-then-empty" else 0
    assert (info[0], info[1], info[3], info[7], info[13]) == (n, 0, 0, 1 if n else 0, 1)
    assert info[8] == s.n_loci, "clusters finished: %d of %d" % (info[8], s.n_loci)
    np.testing.assert_array_equal(hit_off, np.zeros(s.n_loci + 1, np.int64))


def test_carry_of_exactly_the_chunk_capacity_and_recovery(ctx):
    """One cluster of more than 64 KB of records (a toy gene's pairs tiled with fresh names), pushed in pieces of ~20 KB: the
    cluster is complete only at the end, so the last carry is every byte before the last push.  chunk_bytes equal to that carry
    is served (bit for bit the one-push results); one byte less is SBGPU_ESHAPE ("exceed a chunk") and the stream can still be
    destroyed; a fresh stream and a resident pass on the same context are right afterwards.
    Catches: a carry of exactly chunk_bytes refused, or one byte more served (the capacity was rounded up to 256 bytes; fixed
    with these tests)."""
    from strawberry_amd import _lib, bam
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import InsertSize
    base, g = toy("E2E")
    want_base = base.run_stream(ctx, [(0, base.n)])
    gene = g["names"][0]
    one_copy, _ = S.tiled_gene_records(U.E2E, gene, 1)
    copies = (150_000 // max(one_copy.size, 1)) + 1
    raw, off = S.tiled_gene_records(U.E2E, gene, copies)
    exons = [e for _, ex in g["ordered"][gene] for e in ex]
    clusters = ([0], [min(e[0] for e in exons)], [max(e[1] for e in exons)], [1 if U.gene_strands(U.E2E)[gene] == "+" else 2])
    annot = eb.Annotation([[ex for _, ex in g["ordered"][gene]]])
    s = S.Sample(raw, off, clusters, 1, annot, InsertSize(MEAN, SD), RL)
    assert s.first[0] == 0 and s.past[0] == s.n          # one cluster, nothing behind it
    cuts = np.unique(np.searchsorted(off, np.arange(20_000, int(off[-1]) - 20_000, 20_000)))
    pushes = S.from_cuts(s.n, cuts)
    carry = int(off[cuts[-1]])
    assert carry > S.MIN_CHUNK + 1 and max(int(off[b] - off[a]) for a, b in pushes) < carry - 1
    want = s.run_stream(ctx, [(0, s.n)])
    assert want["hits"]["mass"].sum() > 0 and (want["keep"] >= 0).all()
    for give_off in (True, False):
        r = s.run_stream(ctx, pushes, give_off=give_off, chunk_bytes=carry)
        S.assert_same(r, want, "carry == chunk_bytes")
        assert r["info"]["most_bytes_carried"] == carry == r["info"]["chunk_bytes"]
        with pytest.raises(_lib.SbgpuError, match="exceed a chunk"):
            s.run_stream(ctx, pushes, give_off=give_off, chunk_bytes=carry - 1)
    # the context serves a fresh stream and a resident pass afterwards
    S.assert_same(base.run_stream(ctx, S.schedules(base.n, base.first, base.past, seed=3)[3][1]), want_base, "after ESHAPE")
    S.assert_same(base.resident_pass(ctx), want_base, "resident after ESHAPE")
    S.assert_same(s.run_stream(ctx, pushes, chunk_bytes=carry), want, "again")
    assert bam.index(raw).size == s.n + 1


def test_streams_and_resident_pass_repeated_on_one_context(ctx):
    """Two streams back to back with different schedules, outputs poisoned (-1) before each, then a resident pass, on one
    context: every result identical (pooled memory reused between them)."""
    s, _ = toy("E2E_EMP")
    sch = dict(S.schedules(s.n, s.first, s.past, seed=5))
    a = s.run_stream(ctx, sch["random0"])
    b = s.run_stream(ctx, sch["ends"], give_off=False)
    c = s.resident_pass(ctx)
    d = s.run_stream(ctx, sch["empty-first-middle-last"])
    for x, what in ((b, "second stream"), (c, "resident"), (d, "third stream")):
        S.assert_same(x, a, what)


def _irregular_chunks(q, seed, n_pieces=45):
    """FrontQuantifier.h_chunks cut at seeded irregular record indices (pieces between a quarter and twice the mean size),
    and the chunk size they need (the largest piece or the largest possible carry)."""
    import torch
    rng = np.random.default_rng(seed)
    off = q.h_rec_off
    n = q.n_records
    w = rng.uniform(0.25, 2.0, n_pieces)
    cuts = np.unique(np.clip((np.cumsum(w)[:-1] / w.sum() * n).astype(np.int64), 1, n - 1))
    pushes = S.from_cuts(n, cuts)
    raw = q.h_bytes.numpy()
    keys = S.record_keys(raw, off)
    first, past = S.cluster_edges(keys, q._c_ref, q._c_left, q._c_right)
    q.h_chunks = [(a, b, int(off[a]), int(off[b]), torch.from_numpy(off[a:b + 1] - off[a])) for a, b in pushes]
    q.chunk_bytes = S.chunk_bytes_for(off, pushes, past)
    return pushes


def test_at_scale_irregular_cuts_and_a_chunk_across_references(ctx):
    """The 2 500-locus sample of test_records_from_host_in_chunks_equal_the_resident_pass under irregular seeded cuts: step()'s
    resident results bit for bit.  Then two samples on references 0 and 1 as ONE stream with a chunk that crosses the switch of
    reference: stream_parts' results (which never cut across it) bit for bit."""
    from strawberry_amd import front
    from strawberry_amd.exonbin import Annotation
    q = front.FrontQuantifier(ctx, n_loci=2500, n_frags=2.5e6, seed=44, resident=True, empirical=True)
    q.step()
    size = {"theta": q.n_iso, "fpkm": q.n_iso, "frac": q.n_iso, "tpm": q.n_iso, "keep": q.n_iso, "status": q.n_loci, "iters": q.n_loci}
    want = {k: getattr(q, k)[:n].copy() for k, n in size.items()}
    want_law, want_off, want_tot = dict(q.law), q.front_hit_off.copy(), (q.total_fpkm, q.total_mapped_reads)
    q.to_host(q.n_bytes // 20 + 4096, pinned=False)
    pushes = _irregular_chunks(q, seed=19)
    assert len(set(b - a for a, b in pushes)) > 10
    for k in want:
        getattr(q, k)[:] = -1
    info = q.stream_step()
    assert info["records"] == q.n_records and info["chunks"] == len(pushes) and info["clusters_finished"] == q.n_loci
    assert info["accepted_records"] == q.n_records and info["most_bytes_carried"] <= info["chunk_bytes"] and info["records_decoded_twice"] > 0
    np.testing.assert_array_equal(q.front_hit_off, want_off)
    for k, v in want.items():
        np.testing.assert_array_equal(getattr(q, k)[:size[k]], v, err_msg=k)
    assert (q.total_fpkm, q.total_mapped_reads) == want_tot
    S.assert_same_law(dict(q.law, emp_hist=q.law.get("emp_hist")), dict(want_law, emp_hist=want_law.get("emp_hist")), "at scale")
    q.close()

    parts = []
    for ref_id, seed in ((0, 61), (1, 62)):
        p = front.FrontQuantifier(ctx, n_loci=300, n_frags=2e5, seed=seed, resident=True, empirical=True)
        p.to_host(p.n_bytes // 5 + 4096, pinned=False, ref_id=ref_id)
        parts.append(p)
    want = front.FrontQuantifier.stream_parts(parts)
    raw = np.concatenate([p.h_bytes.numpy() for p in parts])
    off = np.concatenate([parts[0].h_rec_off, parts[1].h_rec_off[1:] + parts[0].h_rec_off[-1]])
    clusters = tuple(np.concatenate([getattr(p, k) for p in parts]) for k in ("_c_ref", "_c_left", "_c_right", "_c_strand"))
    annot = Annotation.concat([p.annot for p in parts])
    s = S.Sample(raw, off, clusters, 2, annot, None, parts[0].read_len)
    n0 = parts[0].n_records
    assert S.record_keys(raw, off)[n0 - 1] >> 32 == 0 and S.record_keys(raw, off)[n0] >> 32 == 1
    cuts = [n0 // 2, n0 - 3 * n0 // 20, n0 + parts[1].n_records // 7, n0 + parts[1].n_records // 2]    # the second chunk crosses the switch
    r = s.run_stream(ctx, S.from_cuts(s.n, cuts))
    for k in S.OUT_KEYS:
        np.testing.assert_array_equal(r[k], want[k], err_msg="two references: %s" % k)
    assert (r["total_fpkm"], r["total_mapped_reads"]) == (want["total_fpkm"], want["total_mapped_reads"])
    assert want["law"]["use_emp"] == 1
    S.assert_same_law(r["law"], want["law"], "two references")
    np.testing.assert_array_equal(r["hits"]["locus_hit_off"], want["locus_hit_off"])
    # the store itself: the resident pass over the same two-reference records (stream_parts does not export it)
    S.assert_same(r, s.resident_pass(ctx), "two references, resident")
    assert r["info"]["clusters_finished"] == annot.n_loci and r["info"]["records"] == s.n
    for p in parts:
        p.close()
