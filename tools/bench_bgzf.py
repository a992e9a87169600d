#!/usr/bin/env python3
"""BGZF on the device, measured: inflate rate, record-index time, and the chunked records -> TPM pass fed with the file's
compressed members (sbgpu_front_stream_push_bgzf) against the same pass fed with the inflated bytes (sbgpu_front_stream_push:
the path that exists without this layer, the yardstick), same process, same sample, alternating.

Input: the c3-front record generator (strawberry_amd/front.py::pack_bam_records) at SB_FRONT_LOCI / SB_FRONT_FRAGS (default
60000 loci, 4e6 read pairs: 8e6 records, ~1.5 GB inflated, compressed here by 16 threads in a few seconds).  The generator's
constant sequence and quality bytes would compress 20-fold; they are overwritten with random nibbles and qualities from a
skewed distribution, and the achieved ratio is reported (real RNA-seq BAMs: 3-5 x).  Compressed by zlib at level 6 in members
that begin on record boundaries, as samtools writes them.

Prints one JSON line (and writes it to --out).  --kernels-only: inflate and index a few times and nothing else (for a
rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
MEMBER = 0xff00


def member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return HEAD + np.uint16(len(comp) + 25).tobytes() + comp + np.array([zlib.crc32(data) & 0xffffffff, len(data)], "<u4").tobytes()


def randomise_payload(torch, d_bytes, d_rec_off, read_len, seed):
    """Sequence nibbles uniform, qualities from a skewed law (most bases at the top few values), in place."""
    g = torch.Generator(device=d_bytes.device)
    g.manual_seed(seed)
    n = int(d_rec_off.numel()) - 1
    seq_len = (read_len + 1) // 2
    # (binned qualities as current sequencers write them: four values, most bases at the top one)
    law = torch.tensor([0.86, 0.08, 0.04, 0.02], device=d_bytes.device)
    qual_of = torch.tensor([37, 25, 11, 2], dtype=torch.uint8, device=d_bytes.device)
    step = 1 << 20
    for a in range(0, n, step):
        at = d_rec_off[a:min(n, a + step)]
        m = int(at.numel())
        n_cig = d_bytes[at + 16].to(torch.int64) | (d_bytes[at + 17].to(torch.int64) << 8)
        seq0 = at + 36 + d_bytes[at + 12].to(torch.int64) + 4 * n_cig
        idx = (seq0.unsqueeze(1) + torch.arange(seq_len, device=at.device).unsqueeze(0)).reshape(-1)
        nib = torch.randint(0, 4, (idx.numel(), 2), generator=g, device=at.device)
        d_bytes[idx] = ((1 << nib[:, 0]) * 16 + (1 << nib[:, 1])).to(torch.uint8)          # A C G T = 1 2 4 8
        idx = (seq0.unsqueeze(1) + seq_len + torch.arange(read_len, device=at.device).unsqueeze(0)).reshape(-1)
        d_bytes[idx] = qual_of[torch.multinomial(law, idx.numel(), replacement=True, generator=g)]
        del idx, nib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, bam, em, front
    if not torch.cuda.is_available():
        raise SystemExit("bench_bgzf.py: no GPU (nothing here is measured on a CPU)")
    n_loci = int(float(os.environ.get("SB_FRONT_LOCI", "60000")))
    n_frags = float(os.environ.get("SB_FRONT_FRAGS", "4e6"))
    chunk = int(float(os.environ.get("SB_FRONT_CHUNK_MB", "128")) * (1 << 20))
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", 0)
    q = front.FrontQuantifier(ctx, n_loci=n_loci, n_frags=n_frags, seed=31, resident=True, empirical=True)
    randomise_payload(torch, q.d_bytes, q.d_rec_off, q.read_len, 5)
    torch.cuda.synchronize(dev)
    host = q.to_host(chunk, pinned=True)
    q.unpin()
    raw = q.h_bytes.numpy()
    rec_off = q.h_rec_off
    # ---- the file: the header in a member of its own, then members that begin on record boundaries
    head = b"BAM\1" + np.int32(0).tobytes() + np.int32(1).tobytes() + np.int32(5).tobytes() + b"chr1\0" + np.int32(2**31 - 1).tobytes()
    cuts, i = [0], 0
    while i < q.n_records:
        j = int(np.searchsorted(rec_off, rec_off[i] + MEMBER, side="right")) - 1
        j = max(j, i + 1)
        cuts.append(j)
        i = j
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:       # (zlib releases the interpreter lock while it compresses)
        parts = list(pool.map(lambda k: member(raw[rec_off[cuts[k]]:rec_off[cuts[k + 1]]].tobytes()), range(len(cuts) - 1), chunksize=64))
    compress_s = time.perf_counter() - t0
    file_bytes = b"".join([member(head)] + parts + [member(b"")])
    del parts
    file = torch.empty(len(file_bytes), dtype=torch.uint8, pin_memory=True)
    file.numpy()[:] = np.frombuffer(file_bytes, np.uint8)
    del file_bytes
    f = file.numpy()
    blk, out = bam.bgzf_index(f)
    n_members, first = blk.size - 1, len(head)
    assert int(out[-1]) == first + raw.size
    ratio = (first + raw.size) / f.size
    # ---- inflate and index on the device, alone
    d_file, d_blk, d_out = file.to(dev), torch.from_numpy(blk).to(dev), torch.from_numpy(out).to(dev)
    d_raw = torch.empty(int(out[-1]), dtype=torch.uint8, device=dev)
    d_status = torch.zeros(n_members, dtype=torch.uint8, device=dev)
    d_off = torch.empty(q.n_records + 1, dtype=torch.int64, device=dev)
    failed = C.c_int64(0)

    def inflate():
        _lib.check(L.sbgpu_bgzf_inflate_device(ctx.h, d_file.data_ptr(), f.size, d_blk.data_ptr(), d_out.data_ptr(), n_members, d_raw.data_ptr(), None,
                                               d_status.data_ptr(), C.byref(failed)), "sbgpu_bgzf_inflate_device")
        assert failed.value == 0

    def index():
        n = L.sbgpu_bam_index_device(ctx.h, d_raw.data_ptr(), int(out[-1]), first, d_out.data_ptr(), n_members + 1, d_off.data_ptr(), q.n_records, None)
        assert n == q.n_records, (n, L.sbgpu_last_error())
        info = (C.c_int64 * 8)()
        L.sbgpu_bam_index_device_info(info)
        return int(info[0])

    def timed(fn, reps):
        fn(), fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t) * 1e3)
        return ts, r
    inflate_ms, _ = timed(inflate, 2 if args.kernels_only else 7)
    index_ms, rounds = timed(index, 2 if args.kernels_only else 7)
    if args.kernels_only:
        print(json.dumps({"kernels_only": True, "inflate_ms": inflate_ms, "index_ms": index_ms}))
        return
    assert torch.equal(d_raw[first:].cpu(), q.h_bytes), "the device inflate does not reproduce the records"
    assert np.array_equal(d_off.cpu().numpy(), rec_off), "the device index does not reproduce the records' offsets"
    del d_file, d_raw, d_off, d_status
    torch.cuda.empty_cache()
    # ---- the host form on 16 threads
    os.environ["SBGPU_HOST_THREADS"] = "16"
    h_raw, h_status = np.empty(int(out[-1]), np.uint8), np.zeros(n_members, np.uint8)
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        _lib.check(L.sbgpu_bgzf_inflate_host(f.ctypes.data, f.size, blk.ctypes.data, out.ctypes.data, 0, n_members, h_raw.ctypes.data, h_status.ctypes.data),
                   "sbgpu_bgzf_inflate_host")
        host_ms.append((time.perf_counter() - t) * 1e3)
    assert not h_status.any() and np.array_equal(h_raw[first:], raw)
    del h_raw
    # ---- the streaming pass: inflated bytes through push (the yardstick) and compressed members through push_bgzf, alternating
    groups, a = [], 0
    while a < n_members:
        b = int(np.searchsorted(out, out[a] + chunk, side="right")) - 1
        groups.append((a, b))
        a = b
    bg = (file, blk, out, first, groups)
    names = ("theta", "fpkm", "frac", "tpm", "keep")
    results = {}
    times = {"push": [], "push_bgzf": []}
    for rep in range(args.steps + 1):            # (the first round warms both up: the pool gets its blocks)
        for kind in ("push", "push_bgzf"):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            info = q.stream_step(bgzf=bg if kind == "push_bgzf" else None)
            torch.cuda.synchronize(dev)
            if rep:
                times[kind].append((time.perf_counter() - t) * 1e3)
            results[kind] = ({k: getattr(q, k)[:q.n_iso].copy() for k in names}, q.front_hit_off.copy(), info)
    same = all(np.array_equal(results["push"][0][k], results["push_bgzf"][0][k]) for k in names) and \
        np.array_equal(results["push"][1], results["push_bgzf"][1])
    gb = (first + raw.size) / 1e9
    med = lambda v: float(np.median(v))      # noqa: E731
    line = {
        "metric": "BGZF inflate on the device, GB/s of inflated output", "value": gb / (med(inflate_ms) * 1e-3), "unit": "GB/s",
        "build_id": L.sbgpu_build_id().decode(),
        "input": {"generator": "c3-front (strawberry_amd/front.py::pack_bam_records), sequence and quality bytes randomised", "loci": n_loci,
                  "read_pairs": int(q.n_frags), "records": q.n_records, "inflated_bytes": first + int(raw.size), "compressed_bytes": int(f.size),
                  "compression_ratio": ratio, "members": n_members, "zlib_level": 6, "members_begin_on_record_boundaries": True,
                  "compress_s_16_threads": compress_s, "host_memory": "page-locked" if host["pinned"] else "pageable"},
        "inflate_device_ms": inflate_ms, "inflate_device_gb_per_s": gb / (med(inflate_ms) * 1e-3),
        "index_device_ms": index_ms, "index_rounds": rounds,
        "inflate_host_16_threads_ms": host_ms, "inflate_host_16_threads_gb_per_s": gb / (min(host_ms) * 1e-3),
        "stream": {"chunk_bytes": chunk, "pushes_inflated": len(q.h_chunks), "pushes_compressed": len(groups),
                   "push_inflated_ms": times["push"], "push_bgzf_ms": times["push_bgzf"],
                   "push_bgzf_over_push": med(times["push_bgzf"]) / med(times["push"]), "results_identical": bool(same),
                   "compressed_bytes_pushed": results["push_bgzf"][2]["compressed_bytes_pushed"]},
        "warmup": "2 calls (kernels), 1 pass of each kind (streams)", "repeats": {"kernels": 7, "streams": args.steps},
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(s + "\n")
    if not same:
        raise SystemExit("bench_bgzf.py: the compressed pass and the inflated pass disagree")


if __name__ == "__main__":
    main()
