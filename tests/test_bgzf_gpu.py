"""BGZF on the device: sbgpu_bgzf_inflate_device against zlib and against the host form, on the corpus and the damaged members of
tests/test_bgzf.py; sbgpu_bam_index_device against sbgpu_bam_index_host on streams whose members do and do not start on record
boundaries; a BAM file's bytes -> reads on the device (bam.decode_file); and the chunked stream fed with compressed members
(sbgpu_front_stream_push_bgzf) against the same records through push and through the resident entries."""
import ctypes as C
import struct

import numpy as np
import pytest

import bam_util as B
import bgzf_util as Z
import stream_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus(np.random.default_rng(20))


def run_device(ctx, members):
    """sbgpu_bgzf_inflate_device over `members` laid out as one file, the output between guards of 0xA5 -> (status, per-member
    output bytes, guards intact, *n_failed)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    file = np.frombuffer(b"".join(m.bytes() for m in members), np.uint8)
    blk, off = Z.walk(file.tobytes())
    n = len(members)
    d_file, d_blk, d_off = torch.from_numpy(file.copy()).to(dev), torch.from_numpy(blk).to(dev), torch.from_numpy(off).to(dev)
    d_buf = torch.full((Z.GUARD + int(off[-1]) + Z.GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    failed = C.c_int64(-1)
    torch.cuda.synchronize(dev)
    rc = ctx.L.sbgpu_bgzf_inflate_device(ctx.h, d_file.data_ptr(), file.size, d_blk.data_ptr(), d_off.data_ptr(), n, d_buf.data_ptr() + Z.GUARD,
                                         None, d_status.data_ptr(), C.byref(failed))
    assert rc == 0, ctx.L.sbgpu_last_error()
    buf = d_buf.cpu().numpy()
    return d_status.cpu().numpy()[:n], Z.split_output(buf, off), Z.guards_intact(buf), failed.value


def test_inflate_equals_zlib_on_the_corpus(ctx, corpus):
    members, _ = corpus
    status, got, guards, failed = run_device(ctx, members)
    assert guards and failed == 0
    for m, s, g in zip(members, status, got):
        assert s == 0 and g == m.data, (m.label, s)


def damaged_layout(members):
    rng = np.random.default_rng(21)
    small = [m for m in members if m.isize <= 257] + [m for m in members if m.isize > 257][::7]
    bad = Z.damaged(rng, small, 2400)
    good = [m for m in members if 0 < m.isize <= 0xff00][::5]
    return Z.interleave(good, bad)


def test_damaged_members_as_zlib_and_as_the_host_form(ctx, corpus):
    members, _ = corpus
    laid = damaged_layout(members)
    status, got, guards, failed = run_device(ctx, laid)
    h_status, h_got, h_guards = Z.run_host(ctx.L, laid)
    assert guards and h_guards
    np.testing.assert_array_equal(status, h_status)            # the same decoder: the same verdicts, reasons included
    assert failed == int((status != 0).sum()) > 100
    for k, (m, s, g) in enumerate(zip(laid, status, got)):
        if k % 2 == 0:
            assert s == 0 and g == m.data, ("neighbour", m.label)
            continue
        ok, want = Z.expect(m)
        assert (s == 0) == ok, (m.label, int(s), ok)
        if ok:
            assert g == want, m.label
    # an ISIZE that lies, one too small and one too large
    picks = [m for m in members if m.isize in (2, 257, 0xff00)][::9]
    for delta in (-1, 1):
        laid = Z.interleave(picks, [Z.Member(m.payload, m.isize + delta, None, m.label) for m in picks])
        status, got, guards, failed = run_device(ctx, laid)
        assert guards and (status[0::2] == 0).all() and (status[1::2] == 7).all() and failed == len(picks)
        assert all(g == m.data for m, g in zip(laid[0::2], got[0::2]))


def test_twenty_thousand_members_at_once(ctx, corpus):
    """Every CU holds several members at once; undamaged and damaged ones side by side in random order."""
    members, _ = corpus
    rng = np.random.default_rng(23)
    pool = [m for m in members if m.isize <= 257] + [m for m in members if m.isize > 257][::4] + damaged_layout(members)[1::2][:1500]
    want = [Z.expect(m) for m in pool]
    order = rng.integers(0, len(pool), 21000)
    laid = [pool[int(k)] for k in order]
    status, got, guards, failed = run_device(ctx, laid)
    assert guards
    n_bad = 0
    for k, s, g in zip(order, status, got):
        ok, data = want[int(k)]
        assert (s == 0) == ok, (pool[int(k)].label, int(s))
        n_bad += not ok
        if ok:
            assert g == data, pool[int(k)].label
    assert failed == n_bad > 1000


def test_no_members_and_bad_arguments(ctx):
    failed = C.c_int64(-1)
    assert ctx.L.sbgpu_bgzf_inflate_device(ctx.h, None, 0, None, None, 0, None, None, None, C.byref(failed)) == 0 and failed.value == 0
    assert ctx.L.sbgpu_bgzf_inflate_device(ctx.h, None, 0, None, None, 0, None, None, None, None) == 0
    assert ctx.L.sbgpu_bgzf_inflate_device(ctx.h, None, 10, None, None, 1, None, None, None, None) == -1
    assert ctx.L.sbgpu_bgzf_inflate_device(None, None, 0, None, None, 0, None, None, None, None) == -1


# ---- record offsets on the device

def members_at_record_boundaries(head, records, target=0xff00):
    """The way bam_write1 writes (bam.c:238: a flush before a record that would not fit): the header in members of its own, every
    member begins with a record; a record longer than a member is cut."""
    parts, cur = [head[i:i + target] for i in range(0, len(head), target)], b""
    for r in records:
        if cur and len(cur) + len(r) > target:
            parts.append(cur)
            cur = b""
        cur += r
        while len(cur) > target:
            parts.append(cur[:target])
            cur = cur[target:]
    if cur:
        parts.append(cur)
    return b"".join(B._bgzf_block(p) for p in parts) + B._bgzf_block(b"")


def blind_members(data, rng, lo, hi, first=()):
    """Members of lo .. hi bytes cut without regard to records (the first ones of the sizes `first`)."""
    out, p, first = [], 0, list(first)
    while p < len(data):
        k = first.pop(0) if first else int(rng.integers(lo, hi + 1))
        out.append(B._bgzf_block(data[p:p + k]))
        p += k
    return b"".join(out) + B._bgzf_block(b"")


def index_both(ctx, file, with_guesses=True, cap_delta=None):
    """-> (host result or None, device result or None, info) on the file's inflated stream behind its header."""
    import torch
    from strawberry_amd import _lib, bam
    table = bam.bgzf_index(file)
    raw = bam.inflate(file, table=table)
    _, first = bam.header_length(raw)
    try:
        want = bam.index(raw[first:])
    except _lib.SbgpuError:
        want = None
    d_raw = bam.inflate(file, device=ctx, table=table)
    assert d_raw.cpu().numpy().tobytes() == raw.tobytes()
    d_guess = torch.from_numpy(table[1]).to(d_raw.device) if with_guesses else None
    cap = None if cap_delta is None else want.size - 1 + cap_delta
    try:
        d_off, info = bam.index_device(d_raw, first, d_guess, ctx, cap=cap)
        got = d_off.cpu().numpy()
    except _lib.SbgpuError:
        got = None
        info = (C.c_int64 * 8)()
        ctx.L.sbgpu_bam_index_device_info(info)
        info = [int(v) for v in info[:4]]
    return want, got, info


def test_index_device_equals_index_host(ctx):
    rng = np.random.default_rng(24)
    head = B.header_bytes(B.REFS)
    recs = B.random_records(rng, 6000)
    assert len(b"".join(recs)) > 6 * 0xff00
    # (a) members cut at record boundaries: every guess is right, one round
    want, got, info = index_both(ctx, members_at_record_boundaries(head, recs))
    np.testing.assert_array_equal(got, want)
    assert want.size == 6001 and info[0] == 1 and info[1] >= 8 and info[2] == 0 and info[3] == -1, info
    # (b) blind cuts every 0xff00 bytes
    want, got, info = index_both(ctx, B.bgzf_compress(head + b"".join(recs)))
    np.testing.assert_array_equal(got, want)
    assert info[0] > 1, info
    # (c) one record longer than two members, among records at member starts
    long_rec = struct.pack("<i", 150_000) + rng.integers(0, 256, 150_000, dtype=np.uint8).tobytes()
    want, got, info = index_both(ctx, members_at_record_boundaries(head, recs[:2000] + [long_rec] + recs[2000:]))
    np.testing.assert_array_equal(got, want)
    assert want.size == 6002 and int(np.diff(want).max()) == 150_004 and info[3] == -1, info
    # (d) members of 100-300 bytes: most guesses are wrong, the rounds' cap is reached and the sequential walker finishes
    want, got, info = index_both(ctx, blind_members(head + b"".join(recs[:1500]), rng, 100, 300))
    np.testing.assert_array_equal(got, want)
    assert info[0] == 9 and info[3] > 0 and info[1] > 1000, info
    # (e) no guesses
    want, got, info = index_both(ctx, B.bgzf_compress(head + b"".join(recs)), with_guesses=False)
    np.testing.assert_array_equal(got, want)
    # (f) a stream that ends inside a record
    for cut in (1, 3, 4, 5, 40):
        want, got, info = index_both(ctx, members_at_record_boundaries(head, recs[:3000] + [recs[3000][:-cut]]))
        assert want is None and got is None, cut
    # (g) cap: exactly enough, one too small
    file = members_at_record_boundaries(head, recs)
    want, got, info = index_both(ctx, file, cap_delta=0)
    np.testing.assert_array_equal(got, want)
    want, got, info = index_both(ctx, file, cap_delta=-1)
    assert want is not None and got is None
    assert b"cap" in ctx.L.sbgpu_last_error()
    # (h) a record of the true chain with a negative size word
    broken = list(recs)
    broken[4000] = struct.pack("<i", -8) + broken[4000][4:]
    for f in (members_at_record_boundaries(head, broken), B.bgzf_compress(head + b"".join(broken))):
        want, got, info = index_both(ctx, f)
        assert want is None and got is None
    # (i) noise behind valid size words: walks from wrong entries meet anything
    noise = B.garbage_records(rng, 5000)
    for f in (B.bgzf_compress(head + b"".join(noise)), blind_members(head + b"".join(noise), rng, 2000, 9000),
              members_at_record_boundaries(head, noise, 5000)):
        want, got, info = index_both(ctx, f)
        np.testing.assert_array_equal(got, want)
        assert want.size == 5001
    # nothing behind the header; nothing at all behind first_record
    want, got, info = index_both(ctx, B.bgzf_compress(head))
    np.testing.assert_array_equal(got, want)
    assert got.tolist() == [0]


# ---- a file's bytes -> reads

READ_ARRAYS = ("status", "record", "read_id", "ref", "nh", "nm", "read_len", "left", "right", "partner_pos", "sam_flag", "flags", "block_off",
               "block_left", "block_right")


def assert_same_reads(a, b, what):
    assert (a.n_records, a.n_reads, a.n_blocks, a.any_paired, a.by_status) == (b.n_records, b.n_reads, b.n_blocks, b.any_paired, b.by_status), what
    for k in READ_ARRAYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg="%s %s" % (what, k))


def test_decode_file_equals_decode_of_the_inflated_records(ctx, tmp_path):
    import test_front_stream_gpu as T
    from strawberry_amd import bam
    rng = np.random.default_rng(25)
    files = {}
    for n in (0, 1, 3000):
        path = str(tmp_path / ("r%d.bam" % n))
        B.write_bam(path, B.REFS, B.random_records(rng, n) + B.garbage_records(rng, n // 3))
        files["random %d" % n] = (path, bam.BamOptions(n_ref=len(B.REFS)))
    for which in T.RUNS:
        s, g = T.toy(which)
        path = str(tmp_path / (which + ".bam"))
        open(path, "wb").write(members_at_record_boundaries(B.header_bytes([(c, 10_000_000) for c in g["chroms"]]),
                                                            [s.raw[s.off[k]:s.off[k + 1]].tobytes() for k in range(s.n)], 3000))
        files[which] = (path, bam.BamOptions(unique_only=T.RUNS[which][0], n_ref=len(g["chroms"])))
    for what, (path, opts) in files.items():
        refs, rec = B.read_bam_records(path)
        want = bam.decode(rec, options=opts, device=ctx)
        got = bam.decode_file(open(path, "rb").read(), opts, device=ctx)
        assert_same_reads(got, want, what)
        assert_same_reads(bam.decode_file(open(path, "rb").read(), opts), bam.decode(rec, options=opts), what + " (host)")
        assert want.n_records == (rec.size and bam.index(rec).size - 1)


# ---- the chunked stream fed with compressed members

def run_stream_bgzf(s, ctx, file, groups, chunk_bytes, spoil=None):
    """`file` (header + s.raw as BGZF) through sbgpu_front_stream_push_bgzf, members grouped as `groups` ([(a, b)] member ranges)
    -> the dict of Sample.run_stream (info with the compressed bytes pushed)."""
    from strawberry_amd import _lib, bam
    L = ctx.L
    f = np.frombuffer(file, np.uint8)
    blk, out = bam.bgzf_index(f)
    _, first = bam.read_header(f, (blk, out))
    res, outs, par, used = s._outputs()
    fs, h = C.c_void_p(), C.c_void_p()
    _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), int(chunk_bytes), C.byref(fs)), "sbgpu_front_stream_begin")
    try:
        keep = []
        for a, b in groups:
            part = np.ascontiguousarray(f[blk[a]:blk[b]])
            tb, to = blk[a:b + 1].copy(), out[a:b + 1].copy()
            keep.append(part)
            _lib.check(L.sbgpu_front_stream_push_bgzf(fs, part.ctypes.data if part.size else None, int(part.size), tb.ctypes.data, to.ctypes.data,
                                                      int(b - a), max(0, first - int(out[a]))), "sbgpu_front_stream_push_bgzf")
            tb[:], to[:] = -1, -1                     # (the tables are the caller's again once the push returns)
            if spoil is not None:
                spoil(L, fs)
        _lib.check(L.sbgpu_front_stream_end(fs, C.byref(s.an), C.byref(s.ins) if s.ins is not None else None, s.read_len, s.long_read,
                                            C.byref(par), None, C.byref(used), C.byref(outs), C.byref(h)), "sbgpu_front_stream_end")
        r = s._collect(res, outs, used)
        L.sbgpu_bins_destroy(h)
        dh, d_mass, hoff = _lib.sbgpu_hits_t(), C.c_void_p(), C.c_void_p()
        _lib.check(L.sbgpu_front_stream_hits(fs, C.byref(dh), C.byref(d_mass), C.byref(hoff)), "sbgpu_front_stream_hits")
        r["hits"] = s._hits(dh, d_mass, hoff)
        info = (C.c_int64 * 16)()
        _lib.check(L.sbgpu_front_stream_info(fs, info), "sbgpu_front_stream_info")
    finally:
        L.sbgpu_front_stream_destroy(fs)
    r["info"] = {"records": int(info[0]), "accepted_records": int(info[1]), "clusters_finished": int(info[8]), "ended": int(info[13]),
                 "compressed_bytes": int(info[15])}
    return r


def groupings(n, out, first, rec_starts, seed):
    """name -> member ranges covering [0, n): the schedules the stream must not care about."""
    rng = np.random.default_rng(seed)
    g = {"each": [(k, k + 1) for k in range(n)], "one": [(0, n)]}
    for r in range(3):
        cuts = np.unique(np.concatenate([rng.choice(np.arange(1, n), min(n - 1, int(rng.integers(1, 8))), replace=False), [n]]))
        g["random%d" % r] = S.from_cuts(n, cuts)
    inside_record = [k for k in range(1, n) if out[k] > first and out[k] < out[n] and int(out[k] - first) not in rec_starts]
    inside_header = [k for k in range(1, n) if 0 < out[k] < first]
    assert inside_record and inside_header
    g["inside a record"] = S.from_cuts(n, [inside_record[len(inside_record) // 2], n])
    g["inside the header"] = S.from_cuts(n, [inside_header[0], inside_header[-1], n])
    g["empty pushes"] = [(0, 0), (0, n // 2), (n // 2, n // 2), (n // 2, n), (n, n)]
    return g


def stream_cases(s, ctx, head, what, lo=400, hi=7000):
    want = s.run_stream(ctx, [(0, s.n)])
    S.assert_same(s.resident_pass(ctx), want, what + " resident vs push")
    rng = np.random.default_rng(26)
    rec_starts = set(int(v) for v in s.off)
    chunk = max(S.MIN_CHUNK, len(head) + int(s.raw.size))
    for layout, file in (("blind", blind_members(head + s.raw.tobytes(), rng, lo, hi, first=(25, 20, 10))),
                         ("records", members_at_record_boundaries(b"", [head[:len(head) // 2], head[len(head) // 2:]] +
                                                                  [s.raw[s.off[k]:s.off[k + 1]].tobytes() for k in range(s.n)], 9000))):
        from strawberry_amd import bam
        blk, out = bam.bgzf_index(file)
        n = blk.size - 1
        gs = groupings(n, out, len(head), rec_starts, 27) if layout.startswith("blind") else {"each": [(k, k + 1) for k in range(n)], "one": [(0, n)]}
        for name, groups in gs.items():
            r = run_stream_bgzf(s, ctx, file, groups, chunk)
            S.assert_same(r, want, "%s %s %s" % (what, layout, name))
            assert r["info"]["records"] == s.n and r["info"]["clusters_finished"] == s.n_loci and r["info"]["ended"] == 1, r["info"]
            assert r["info"]["compressed_bytes"] == len(file)
    return want


@pytest.mark.parametrize("which", ["E2E", "E2E_LONG", "E2E_MASS", "E2E_FILTER", "E2E_EMP", "E2E_SINGLE", "E2E_LONGREAD", "E2E_MINUS", "E2E_CHROMS"])
def test_compressed_members_through_the_stream_on_reference_runs(ctx, which):
    import test_front_stream_gpu as T
    s, g = T.toy(which)
    head = B.header_bytes([(c, 10_000_000) for c in g["chroms"]])
    want = stream_cases(s, ctx, head, which)
    T.check_reference_run(which, want, g)


def test_compressed_members_through_the_stream_on_a_spliced_sample(ctx):
    import test_front_stream_gpu as T
    clean, g = T.toy("E2E")
    n_chroms = len(g["chroms"])
    c_ref, c_left, c_right, _ = g["clusters"]
    raw, off, kinds = S.splice(clean.raw, c_ref, c_left, c_right, n_chroms, seed=7)
    s = S.Sample(raw, off, g["clusters"], n_chroms + 1, clean.annot, clean.insert, T.RL, clean.long_read, True, clean.min_isoform_frac)
    assert s.n > clean.n
    # (members of 40-700 bytes: nearly every member boundary cuts a record, many records span several members)
    stream_cases(s, ctx, B.header_bytes([(c, 10_000_000) for c in g["chroms"]] + [("other", 1000)]), "spliced", lo=40, hi=700)


def test_stream_refuses_mixing_and_damaged_members_and_recovers(ctx):
    import test_front_stream_gpu as T
    from strawberry_amd import _lib, bam
    s, g = T.toy("E2E")
    want = s.run_stream(ctx, [(0, s.n)])
    head = B.header_bytes([(c, 10_000_000) for c in g["chroms"]])
    file = blind_members(head + s.raw.tobytes(), np.random.default_rng(28), 500, 2000)
    blk, out = bam.bgzf_index(file)
    n = blk.size - 1
    chunk = max(S.MIN_CHUNK, int(out[-1]))
    each = [(k, k + 1) for k in range(n)]
    # push into a stream of compressed members, and the other way round
    def push_records(L, fs):
        part = np.ascontiguousarray(s.raw[:s.off[1]])
        assert L.sbgpu_front_stream_push(fs, part.ctypes.data, int(part.size), None, 0) == -1        # SBGPU_EINVAL
        assert b"not mixed" in L.sbgpu_last_error()
    S.assert_same(run_stream_bgzf(s, ctx, file, [(0, n // 2), (n // 2, n)], chunk, spoil=push_records), want, "push refused, stream goes on")
    fs = C.c_void_p()
    _lib.check(ctx.L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), chunk, C.byref(fs)), "begin")
    part = np.ascontiguousarray(s.raw[:s.off[1]])
    assert ctx.L.sbgpu_front_stream_push(fs, part.ctypes.data, int(part.size), None, 0) == 0
    f = np.frombuffer(file, np.uint8)
    assert ctx.L.sbgpu_front_stream_push_bgzf(fs, f.ctypes.data, int(blk[1]), blk.ctypes.data, out.ctypes.data, 1, 0) == -1
    assert b"not mixed" in ctx.L.sbgpu_last_error()
    ctx.L.sbgpu_front_stream_destroy(fs)
    # a push that inflates to more than a chunk
    fs = C.c_void_p()
    _lib.check(ctx.L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), S.MIN_CHUNK, C.byref(fs)), "begin")
    big = B.bgzf_compress(bytes(70000))
    bb, bo = bam.bgzf_index(big)
    fb = np.frombuffer(big, np.uint8)
    assert ctx.L.sbgpu_front_stream_push_bgzf(fs, fb.ctypes.data, fb.size, bb.ctypes.data, bo.ctypes.data, bb.size - 1, 0) == -5     # SBGPU_ESHAPE
    ctx.L.sbgpu_front_stream_destroy(fs)
    # a damaged member: SBGPU_EINVAL naming its offset in the file; the stream is destroyed, the context goes on
    k = n // 2
    x = bytearray(file)
    x[int(blk[k]) + 18] |= 0x06                      # the first block's type becomes the reserved one
    with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*member at byte %d of the file" % int(blk[k])):
        run_stream_bgzf(s, ctx, bytes(x), each, chunk)
    with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*member at byte %d of the file" % int(blk[k])):
        run_stream_bgzf(s, ctx, bytes(x), [(0, n)], chunk)
    # a file that ends inside a record
    cut = blind_members((head + s.raw.tobytes())[:-7], np.random.default_rng(29), 500, 2000)
    cb = bam.bgzf_index(cut)[0]
    with pytest.raises(_lib.SbgpuError, match="ends inside a record"):
        run_stream_bgzf(s, ctx, cut, [(0, cb.size - 1)], chunk)
    S.assert_same(s.resident_pass(ctx), want, "resident after the failures")
    S.assert_same(run_stream_bgzf(s, ctx, file, each, chunk), want, "stream after the failures")
