"""Helpers for the tests of the chunked record stream (sbgpu_front_stream_begin / push / end, tests/test_front_stream_gpu.py):

  record_keys(raw, off)          (reference, 1-based start) of every record as one sortable key
  cluster_edges(...)             per cluster: its first record, the first record behind its end
  from_cuts(n, cuts)             record-index cut points -> pushes [(a, b)]; a repeated cut is an empty push
  schedules(...)                 the deterministic, seeded push schedules every record set goes through
  chunk_bytes_for(...)           the chunk size a schedule needs (its largest push, its largest possible carry, 64 KB at least)
  splice(...)                    records the reference drops (or that lie outside every cluster) inserted in coordinate order
  run_stream / resident_pass     one sample through the stream under a schedule / through the resident entries at once
"""
import ctypes as C

import numpy as np

import bam_util as B

MIN_CHUNK = 1 << 16          # sbgpu_front_stream_begin's smallest chunk
TAIL = 1 << 40               # the key of an unplaced record (refID -1): behind every placed one, as a sorted BAM puts it
OUT_KEYS = ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters")
LAW_KEYS = ("mean", "sd", "use_emp", "start_offset", "end_offset", "total_reads")
HIT_KEYS = ("hit_locus", "feat_off", "feat_code", "feat_left", "feat_right", "mass")


def record_keys(raw, off):
    """-> int64 [n]: refID << 32 | (pos + 1) per record (TAIL for refID -1)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    at = np.asarray(off[:-1], np.int64)
    ref = raw[(at + 4)[:, None] + np.arange(4)].copy().view("<i4").reshape(-1).astype(np.int64)
    pos = raw[(at + 8)[:, None] + np.arange(4)].copy().view("<i4").reshape(-1).astype(np.int64)
    return np.where(ref < 0, TAIL, (ref << 32) | (pos + 1))


def cluster_edges(keys, c_ref, c_left, c_right):
    """-> (first, past): cluster k's records start at first[k]; past[k] is the first record that starts behind its end
    (sbgpu_assign_reads_*'s bound: a read with key > (ref, right) completes the cluster)."""
    c_ref = np.asarray(c_ref, np.int64)
    first = np.searchsorted(keys, (c_ref << 32) | np.asarray(c_left, np.int64), side="left")
    past = np.searchsorted(keys, (c_ref << 32) | (np.asarray(c_right, np.int64) + 1), side="left")      # (the first key > (ref, right))
    return first.astype(np.int64), np.maximum.accumulate(past).astype(np.int64)


def from_cuts(n, cuts):
    """Cut points (record indices in [0, n], repeats allowed) -> consecutive pushes [(a, b)] covering [0, n)."""
    bounds = [0] + sorted(int(c) for c in cuts) + [n]
    assert all(0 <= c <= n for c in bounds)
    return list(zip(bounds[:-1], bounds[1:]))


def schedules(n, first, past, seed, n_random=20):
    """-> [(name, pushes)]: one push; one record per push; cuts at every cluster's first record; right behind every
    cluster's last record and one record either side; n_random seeded random cut sets (some with empty pushes); a chunk
    that completes no cluster; empty pushes first, in the middle and last; everything then an empty push."""
    inner = lambda cs: sorted(set(int(c) for c in cs if 0 < c < n))  # noqa: E731
    out = [("one", from_cuts(n, [])),
           ("each", from_cuts(n, range(1, n))),
           ("starts", from_cuts(n, inner(first))),
           ("ends", from_cuts(n, inner(past))),
           ("ends-1", from_cuts(n, inner(past - 1))),
           ("ends+1", from_cuts(n, inner(past + 1)))]
    for r in range(n_random):
        rng = np.random.default_rng([seed, r])
        m = int(rng.integers(1, max(2, min(n - 1, 60))))
        cuts = list(rng.choice(np.arange(1, n), size=min(m, n - 1), replace=False)) if n > 1 else []
        if rng.random() < 0.3 and cuts:
            cuts.append(cuts[int(rng.integers(0, len(cuts)))])         # an empty push somewhere
        out.append(("random%d" % r, from_cuts(n, cuts)))
    big = int(np.argmax(past - first))
    if past[big] - first[big] >= 3:
        # the middle chunk holds records of one cluster only, none behind its end: it completes nothing
        out.append(("completes-none", from_cuts(n, inner([first[big] + 1, past[big] - 1]))))
    mid = inner(past)[len(inner(past)) // 2] if inner(past) else n // 2
    out.append(("empty-first-middle-last", from_cuts(n, [0, mid, mid, n])))
    out.append(("all-then-empty", from_cuts(n, [n])))
    return out


def chunk_bytes_for(off, pushes, past, accepted=None):
    """The larger of 64 KB and what the schedule needs: its largest push, and the largest carry any window can hold -- the
    records from the first one offered to a cluster (behind the cluster before) up to the first ACCEPTED record behind its
    end, the last cluster's up to the stream's end.  accepted: bool per record (None: every record is)."""
    off = np.asarray(off, np.int64)
    n = off.size - 1
    acc_idx = np.arange(n) if accepted is None else np.flatnonzero(accepted)
    begin = np.concatenate([[0], past[:-1]]).astype(np.int64)
    k = np.searchsorted(acc_idx, past, side="left")
    nxt = np.full(len(past), n, np.int64)
    nxt[k < acc_idx.size] = acc_idx[k[k < acc_idx.size]]
    carry = int((off[nxt] - off[begin]).max()) if len(past) else 0
    carry = max(carry, int(off[n] - off[past[-1]]) if len(past) else int(off[n]))     # (the reads behind the last cluster)
    push = max((int(off[b] - off[a]) for a, b in pushes), default=0)
    return max(MIN_CHUNK, push, carry)


def check_schedule(n, pushes):
    """Every record is pushed exactly once, in order, in whole records."""
    assert pushes[0][0] == 0 and pushes[-1][1] == n
    for (a, b), (c, _) in zip(pushes[:-1], pushes[1:]):
        assert a <= b == c
    assert sum(b - a for a, b in pushes) == n


# ---- records the reference drops, or that lie outside every cluster, spliced into a toy run's stream

def splice(raw, c_ref, c_left, c_right, n_chroms, seed):
    """-> (records as uint8, rec_off, kinds [n] (None for the run's own records)).  Inserted, keeping coordinate order:
    unmapped records with a placed mate inside clusters (0x4, at the mate's position), secondary (0x100) and QC-fail (0x200)
    alignments inside clusters, intergenic pairs between clusters that are far enough apart, pairs on a reference without
    clusters (id n_chroms: the options must allow n_chroms + 1 references), and unmapped records (refID -1) at the tail."""
    from strawberry_amd import bam
    rng = np.random.default_rng(seed)
    off = bam.index(raw)
    own = [bytes(raw[off[i]:off[i + 1]]) for i in range(off.size - 1)]
    keys = record_keys(raw, off)
    extra = []          # (key, kind, record bytes)

    def add(kind, tid, pos, flag, cig, mtid=-1, mpos=-1, tags=(("NH", "C", 1), ("XS", "A", "+"))):
        name = "sp%s%d" % (kind[:3], len(extra))
        r = B.record(tid, pos - 1, flag, name, cig, mtid=mtid, mpos=mpos - 1 if mpos > 0 else -1, tags=list(tags))
        extra.append((((tid << 32) | pos) if tid >= 0 else TAIL, kind, r))
    nc = len(c_left)
    for k in sorted(rng.choice(nc, size=min(nc, 6), replace=False).tolist()):
        ref, lo, hi = int(c_ref[k]), int(c_left[k]), int(c_right[k])
        p = int(rng.integers(lo, max(lo + 1, hi - 60)))
        add("unmapped-mate", ref, p, 1 | 4 | 0x80, [], mtid=ref, mpos=p)
        add("secondary", ref, p, 1 | 2 | 0x40 | 0x100, [("M", 40)], mtid=ref, mpos=p + 80)
        add("qcfail", ref, p + 1, 1 | 2 | 0x80 | 0x200 | 0x10, [("M", 40)], mtid=ref, mpos=p + 1)
    reach = {}           # per reference: the furthest end of the clusters so far
    for k in range(nc):
        ref = int(c_ref[k])
        if ref in reach and int(c_left[k]) - reach[ref] > 400:
            g = reach[ref] + 50
            add("intergenic", ref, g, 1 | 2 | 0x20 | 0x40, [("M", 40)], mtid=ref, mpos=g + 150)
            add("intergenic", ref, g + 150, 1 | 2 | 0x10 | 0x80, [("M", 40)], mtid=ref, mpos=g)
        reach[ref] = max(reach.get(ref, 0), int(c_right[k]))
    for j in range(3):
        add("no-cluster-ref", n_chroms, 1000 + 500 * j, 1 | 2 | 0x20 | 0x40, [("M", 50)], mtid=n_chroms, mpos=1200 + 500 * j)
        add("no-cluster-ref", n_chroms, 1200 + 500 * j, 1 | 2 | 0x10 | 0x80, [("M", 50)], mtid=n_chroms, mpos=1000 + 500 * j)
    for j in range(4):
        add("unmapped-tail", -1, 0, 1 | 4 | 8 | (0x40 if j % 2 else 0x80), [], tags=())
    # merge, stable: the run's own records before spliced ones of the same key
    allk = np.concatenate([keys, np.array([e[0] for e in extra], np.int64)])
    src = np.concatenate([np.zeros(len(own), np.int64), np.ones(len(extra), np.int64)])
    order = np.lexsort((np.arange(allk.size), src, allk))
    recs, kinds = [], []
    for i in order.tolist():
        if i < len(own):
            recs.append(own[i]), kinds.append(None)
        else:
            recs.append(extra[i - len(own)][2]), kinds.append(extra[i - len(own)][1])
    out = np.frombuffer(b"".join(recs), np.uint8).copy()
    return out, bam.index(out), kinds


# ---- running a sample

def _hip():
    from strawberry_amd import _lib
    _lib.load()              # (the HIP runtime torch loaded, and the library links against)
    h = C.CDLL("libamdhip64.so.7")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemcpy.restype = C.c_int
    return h


def _d2h(ptr, n, dtype):
    out = np.zeros(max(n, 0), dtype)
    if n > 0:
        rc = _hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)     # hipMemcpyDeviceToHost
        assert rc == 0, "hipMemcpy: %d" % rc
    return out


class Sample:
    """What the stream and the resident pass need of one record set: bytes, offsets, clusters, options, annotation, law."""

    def __init__(self, raw, off, clusters, n_ref, annot, insert=None, read_len=75, long_read=0, unique_only=True, min_isoform_frac=0.0):
        from strawberry_amd import _lib, bam
        self.raw = np.ascontiguousarray(raw, np.uint8)
        self.off = np.ascontiguousarray(off, np.int64)
        self.n = self.off.size - 1
        self.c_ref, self.c_left, self.c_right = (np.ascontiguousarray(x, t) for x, t in zip(clusters[:3], (np.int32, np.uint32, np.uint32)))
        self.c_strand = np.ascontiguousarray(clusters[3], np.uint8)
        self.n_loci = len(self.c_ref)
        self.cl = _lib.sbgpu_clusters_t(self.n_loci, self.c_ref.ctypes.data, self.c_left.ctypes.data, self.c_right.ctypes.data,
                                        self.c_strand.ctypes.data)
        self.opts = bam.BamOptions(unique_only=unique_only, n_ref=n_ref).c()
        self.annot, self.an = annot, annot._struct()
        self.n_iso = int(annot.iso_off[-1])
        self.insert, self.read_len, self.long_read, self.min_isoform_frac = insert, int(read_len), int(long_read), float(min_isoform_frac)
        self.ins = insert._struct(read_len, long_read) if insert is not None else None
        self.keys = record_keys(self.raw, self.off)
        self.first, self.past = cluster_edges(self.keys, self.c_ref, self.c_left, self.c_right)

    def _outputs(self):
        from strawberry_amd import _lib
        res = {k: np.full(self.n_iso + 1, -1.0) for k in ("theta", "fpkm", "frac", "tpm")}     # poisoned: every value must be written
        res["keep"] = np.full(self.n_iso + 1, -1, np.int32)
        res["status"], res["iters"] = np.full(self.n_loci + 1, -1, np.int32), np.full(self.n_loci + 1, -1, np.int32)
        out = _lib.sbgpu_abundances_t()
        for k, v in res.items():
            setattr(out, k, v.ctypes.data)
        par = _lib.sbgpu_abundance_params_t(0, 0, 1, 0, 0.0, self.min_isoform_frac)
        return res, out, par, _lib.sbgpu_insert_t()

    def _collect(self, res, out, used):
        r = {k: (v[:self.n_iso] if k not in ("status", "iters") else v[:self.n_loci]).copy() for k, v in res.items()}
        law = {k: getattr(used, k) for k in LAW_KEYS}
        law["emp_hist"] = (np.ctypeslib.as_array(used.emp_hist, shape=(used.end_offset - used.start_offset + 1,)).copy()
                           if used.use_emp else None)
        r.update(law=law, total_fpkm=float(out.total_fpkm), total_mapped_reads=int(out.total_mapped_reads))
        return r

    def _hits(self, dh, d_mass, hoff):
        n = int(dh.n_hits)
        foff = _d2h(dh.feat_off, n + 1, np.int64) if n else np.zeros(1, np.int64)
        nf = int(foff[-1])
        return {"hit_locus": _d2h(dh.hit_locus, n, np.int32), "feat_off": foff, "feat_code": _d2h(dh.feat_code, nf, np.uint8),
                "feat_left": _d2h(dh.feat_left, nf, np.uint32), "feat_right": _d2h(dh.feat_right, nf, np.uint32),
                "mass": _d2h(d_mass.value if isinstance(d_mass, C.c_void_p) else d_mass, n, np.float32),
                "locus_hit_off": np.ctypeslib.as_array(C.cast(hoff, C.POINTER(C.c_int64)), shape=(self.n_loci + 1,)).copy()}

    def run_stream(self, ctx, pushes, give_off=True, chunk_bytes=None):
        """The record set through sbgpu_front_stream_* pushed as `pushes` (record ranges), with the caller's offsets or
        NULL.  -> dict: outputs, law, totals, info, the store (hits, exported after end), chunk_bytes."""
        from strawberry_amd import _lib
        L = ctx.L
        chunk = chunk_bytes or chunk_bytes_for(self.off, pushes, self.past)
        res, out, par, used = self._outputs()
        fs, h = C.c_void_p(), C.c_void_p()
        _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(self.cl), C.byref(self.opts), int(chunk), C.byref(fs)), "sbgpu_front_stream_begin")
        try:
            # the pushes' bytes and offsets stay alive (and untouched) until the stream is gone
            keep = []
            for a, b in pushes:
                part = np.ascontiguousarray(self.raw[self.off[a]:self.off[b]])
                ro = np.ascontiguousarray(self.off[a:b + 1] - self.off[a])
                keep.append((part, ro))
                _lib.check(L.sbgpu_front_stream_push(fs, part.ctypes.data if part.size else None, int(part.size),
                                                     ro.ctypes.data if give_off else None, int(b - a)), "sbgpu_front_stream_push")
            _lib.check(L.sbgpu_front_stream_end(fs, C.byref(self.an), C.byref(self.ins) if self.ins is not None else None, self.read_len,
                                                self.long_read, C.byref(par), None, C.byref(used), C.byref(out), C.byref(h)), "sbgpu_front_stream_end")
            r = self._collect(res, out, used)
            L.sbgpu_bins_destroy(h)
            dh, d_mass, hoff = _lib.sbgpu_hits_t(), C.c_void_p(), C.c_void_p()
            _lib.check(L.sbgpu_front_stream_hits(fs, C.byref(dh), C.byref(d_mass), C.byref(hoff)), "sbgpu_front_stream_hits")
            r["hits"] = self._hits(dh, d_mass, hoff)
            info = (C.c_int64 * 16)()
            _lib.check(L.sbgpu_front_stream_info(fs, info), "sbgpu_front_stream_info")
        finally:
            L.sbgpu_front_stream_destroy(fs)
        keys = ("records", "accepted_records", "pairs", "unique_hits", "features", "pairs_dropped_by_the_span_filter", "mapped_reads",
                "chunks", "clusters_finished", "most_bytes_carried", "records_decoded_twice", "least_free_device_bytes", "chunk_bytes",
                "ended", "free_device_bytes_at_begin")
        r["info"] = {k: int(info[i]) for i, k in enumerate(keys)}
        r["chunk_bytes"] = int(chunk)
        return r

    def resident_pass(self, ctx):
        """The whole record set at once through the resident entries: sbgpu_bam_decode_device -> sbgpu_assign_reads_device ->
        sbgpu_pair_mates_device -> sbgpu_collapse_pairs_device -> sbgpu_quantify_resident.  -> the same dict as run_stream
        (info: accepted records and mapped reads)."""
        import torch
        from strawberry_amd import _lib
        L = ctx.L
        dev = torch.device("cuda", ctx.device)
        d_raw = torch.from_numpy(self.raw.copy() if self.raw.size else np.zeros(1, np.uint8)).to(dev)
        d_off = torch.from_numpy(self.off).to(dev)
        hb, hm, hu, h = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        try:
            _lib.check(L.sbgpu_bam_decode_device(ctx.h, d_raw.data_ptr(), int(self.raw.size), d_off.data_ptr(), self.n, C.byref(self.opts), None,
                                                 C.byref(hb)), "sbgpu_bam_decode_device")
            rs = _lib.sbgpu_reads_t()
            d_ref, d_left, d_right = C.c_void_p(), C.c_void_p(), C.c_void_p()
            _lib.check(L.sbgpu_bamreads_reads(hb, C.byref(rs), C.byref(d_ref), C.byref(d_left), C.byref(d_right)), "sbgpu_bamreads_reads")
            n_reads = int(rs.n_reads)
            d_cluster = torch.empty(max(n_reads, 1), dtype=torch.int32, device=dev)
            roff = np.zeros(self.n_loci + 1, np.int64)
            _lib.check(L.sbgpu_assign_reads_device(ctx.h, C.byref(self.cl), n_reads, d_ref, d_left, d_right, rs.flags, d_cluster.data_ptr(),
                                                   roff.ctypes.data, None), "sbgpu_assign_reads_device")
            rs.n_reads = int(roff[-1])          # (reads behind the last cluster are no cluster's: pairing takes the clusters' reads)
            _lib.check(L.sbgpu_pair_mates_device(ctx.h, self.n_loci, C.byref(rs), roff.ctypes.data, None, C.byref(hm)), "sbgpu_pair_mates_device")
            dp, poff = _lib.sbgpu_pairs_t(), C.c_void_p()
            _lib.check(L.sbgpu_matepairs_pairs(hm, C.byref(dp), C.byref(poff)), "sbgpu_matepairs_pairs")
            _lib.check(L.sbgpu_collapse_pairs_device(ctx.h, self.n_loci, C.byref(dp), poff, None, C.byref(hu)), "sbgpu_collapse_pairs_device")
            ui = (C.c_int64 * 8)()
            _lib.check(L.sbgpu_uniq_dev_info(hu, ui), "sbgpu_uniq_dev_info")
            dh, d_mass, hoff = _lib.sbgpu_hits_t(), C.c_void_p(), C.c_void_p()
            _lib.check(L.sbgpu_uniq_dev_hits(hu, C.byref(dh), C.byref(d_mass), C.byref(hoff)), "sbgpu_uniq_dev_hits")
            res, out, par, used = self._outputs()
            _lib.check(L.sbgpu_quantify_resident(ctx.h, C.byref(self.an), C.byref(dh), d_mass, hoff, C.byref(self.ins) if self.ins is not None else None,
                                                 self.read_len, self.long_read, int(ui[4]), C.byref(par), None, C.byref(used), C.byref(out),
                                                 C.byref(h)), "sbgpu_quantify_resident")
            r = self._collect(res, out, used)
            r["hits"] = self._hits(dh, d_mass, hoff)
            r["info"] = {"accepted_records": n_reads, "mapped_reads": int(ui[4]), "unique_hits": int(ui[0])}
            torch.cuda.synchronize(dev)
        finally:
            for fn, x in ((L.sbgpu_bins_destroy, h), (L.sbgpu_uniq_dev_destroy, hu), (L.sbgpu_matepairs_destroy, hm), (L.sbgpu_bamreads_destroy, hb)):
                if x.value:
                    fn(x)
        return r


def assert_same(a, b, what="", law=True, hits=True):
    """Every output array, the law, the totals and the store of two runs: bit for bit."""
    for k in OUT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))
    assert (a["total_fpkm"], a["total_mapped_reads"]) == (b["total_fpkm"], b["total_mapped_reads"]), what
    if law:
        assert_same_law(a["law"], b["law"], what)
    if hits:
        for k in HIT_KEYS + ("locus_hit_off",):
            np.testing.assert_array_equal(a["hits"][k], b["hits"][k], err_msg="%s %s" % (what, k))


def assert_same_law(a, b, what=""):
    for k in LAW_KEYS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    if a["use_emp"]:
        np.testing.assert_array_equal(a["emp_hist"], b["emp_hist"], err_msg="%s emp_hist" % what)


def tiled_gene_records(d, gene, copies):
    """One toy gene's read pairs (reads.npz), `copies` times over with fresh names, as BAM records in coordinate order ->
    (bytes, rec_off).  Same positions: the copies are PCR duplicates of the gene's pairs, one cluster whose records can
    exceed a chunk."""
    import os
    import e2e_util as U
    from strawberry_amd import bam
    z = dict(np.load(os.path.join(d, "reads.npz")))
    genes = list(U.parse_annotation(os.path.join(d, "toy.gtf")))
    strands = U.gene_strands(d)
    xs = "+" if strands[gene] == "+" else "-"
    gi = genes.index(gene)

    def cigar(blocks):
        out = []
        for i, (a, b) in enumerate(blocks):
            if i:
                out.append(("N", a - blocks[i - 1][1] - 1))
            out.append(("M", b - a + 1))
        return out
    recs, serial = [], 0
    for k in np.flatnonzero(z["gene"] == gi).tolist():
        left = list(zip(z["left_l"][z["left_off"][k]:z["left_off"][k + 1]].tolist(), z["left_r"][z["left_off"][k]:z["left_off"][k + 1]].tolist()))
        right = list(zip(z["right_l"][z["right_off"][k]:z["right_off"][k + 1]].tolist(), z["right_r"][z["right_off"][k]:z["right_off"][k + 1]].tolist()))
        for _ in range(copies):
            serial += 1
            name = "tile%d" % serial
            tags = [("NH", "C", 1), ("XS", "A", xs)]
            recs.append((left[0][0], B.record(0, left[0][0] - 1, 1 | 2 | 0x20 | 0x40, name, cigar(left), mtid=0, mpos=right[0][0] - 1, tags=tags)))
            recs.append((right[0][0], B.record(0, right[0][0] - 1, 1 | 2 | 0x10 | 0x80, name, cigar(right), mtid=0, mpos=left[0][0] - 1, tags=tags)))
    recs.sort(key=lambda r: r[0])
    raw = np.frombuffer(b"".join(r[1] for r in recs), np.uint8).copy()
    return raw, bam.index(raw)
