#!/usr/bin/env python
"""What reading a genome costs (sbgpu_fasta_*): a generated genome at human scale -- 3.1e9 bases in 25 contigs at 60
bases a line, built on the device by repeating a block of random lines -- read by the device form stage by stage, and by the host
form on one thread beside it.

  python tools/bench_fasta.py --out profiles/fasta_bench.json

  upload_ms            the file's bytes host -> device (a torch copy of a pageable array, device events around it)
  device_call_ms       sbgpu_fasta_read_device on bytes that are in HBM, host clock around the call (it synchronises): `reps` calls
                       after a warm-up, median with min - max
  stage_ms             with sbgpu_set_timing on, the call's launches as stages of their own: fasta_count (the headers per tile
                       and their scan), fasta_headers (their offsets, the walk of the header lines, the scan of the names),
                       fasta_base_count (the bases per tile, their scan, the first lines), fasta_pack, fasta_names_copy_back
  host_ms              device_call_ms minus the stages: the allocation of the packed sequence, the handle, the call's waits
  host_form_ms         sbgpu_fasta_read_host, one thread, one call
  pack_fraction_of_copy_rate
                       the pack stage's bytes read plus bytes written per second over the rate of a device copy kernel
                       (6.29 TB/s measured for a 16-byte-per-lane copy on this part)
It records and gates nothing."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12


def generate(dev, n_bases, n_contigs, width, seed=0x6661):
    """The file as a uint8 tensor on the device."""
    import torch
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    block_lines = 1 << 20
    alphabet = torch.tensor(list(b"ACGTacgtN"), dtype=torch.uint8, device=dev)
    block = alphabet[torch.randint(0, 9, (block_lines, width + 1), device=dev, generator=gen)]
    block[:, width] = 10
    block = block.reshape(-1)
    parts = []
    for c in range(n_contigs):
        n = n_bases // n_contigs + (1 if c < n_bases % n_contigs else 0)
        full, rest = divmod(n, width)
        parts.append(torch.tensor(list(b">chr%d generated contig %d\n" % (c + 1, c)), dtype=torch.uint8, device=dev))
        body = block.repeat(full // block_lines + 1)[:full * (width + 1)]
        parts.append(body)
        if rest:
            parts.append(torch.cat([block[:rest], torch.tensor([10], dtype=torch.uint8, device=dev)]))
    return torch.cat(parts)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def stages(ctx):
    ms, names = (C.c_float * 16)(), (C.c_char_p * 16)()
    n = ctx.L.sbgpu_last_stage_ms(ctx.h, 16, ms, names)
    return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3.1e9)
    ap.add_argument("--contigs", type=int, default=25)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host form and the upload (the file then never leaves the device)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, em, fasta
    ctx = em.default_context(0)
    L, dev = ctx.L, torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    d = generate(dev, int(args.bases), args.contigs, args.width)
    torch.cuda.synchronize(dev)
    doc = {"tool": "tools/bench_fasta.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "bases": int(args.bases), "contigs": args.contigs, "line_bases": args.width, "file_bytes": int(d.numel()), "generate_s": time.perf_counter() - t0,
           "limits": fasta.limits(), "copy_rate_bytes_per_s": COPY_RATE}
    h = C.c_void_p()

    def call():
        t = time.perf_counter()
        _lib.check(L.sbgpu_fasta_read_device(ctx.h, d.data_ptr(), int(d.numel()), None, C.byref(h)), "sbgpu_fasta_read_device")
        ms = (time.perf_counter() - t) * 1e3
        L.sbgpu_fasta_destroy(h)
        return ms
    g_dev = fasta.read_fasta(d, ctx=ctx)
    doc["info"] = g_dev.info
    assert g_dev.info["bases"] == int(args.bases) and g_dev.info["contigs"] == args.contigs and g_dev.info["ragged"] == 0
    if not args.no_host:
        host_arr = d.cpu().numpy()
        t = time.perf_counter()
        g_host = fasta.read_fasta(host_arr)
        doc["host_form_ms"] = (time.perf_counter() - t) * 1e3
        # the results first: the device form's are the host form's
        for name in ("seq_off", "offset", "line_bases", "line_width", "flags"):
            assert np.array_equal(getattr(g_dev, name), getattr(g_host, name)), name
        assert g_dev.names == g_host.names and all(g_dev.info[k] == g_host.info[k] for k in fasta.INFO_KEYS[:10])
        for c in (0, args.contigs // 2, args.contigs - 1):
            n = int(g_host.length[c])
            for start in (1, n // 2, n - 9999):
                assert g_dev.fetch(c, start, 10000) == g_host.fetch(c, start, 10000), (c, start)
        doc["device_equals_host"] = "index, flags, names, info; windows of three contigs"
        del g_host
        up = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d2 = torch.from_numpy(host_arr).to(dev)
            e1.record()
            torch.cuda.synchronize(dev)
            up.append(e0.elapsed_time(e1))
            del d2
        doc["upload_ms"] = stats(up[1:])
        del host_arr
    del g_dev
    call()
    doc["device_call_ms"] = stats([call() for _ in range(args.reps)])
    _lib.check(L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per, walls = {}, []
        for _ in range(args.reps):
            walls.append(call())
            for k, v in stages(ctx).items():
                per.setdefault(k, []).append(v)
    finally:
        L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: stats(v) for k, v in per.items()}
    doc["timed_call_ms"] = stats(walls)
    doc["host_ms"] = float(np.median(walls)) - sum(float(np.median(v)) for v in per.values())
    doc["bytes_per_s_device_call"] = int(d.numel()) / (doc["device_call_ms"]["median"] * 1e-3)
    if "host_form_ms" in doc:
        doc["bytes_per_s_host_form"] = int(d.numel()) / (doc["host_form_ms"] * 1e-3)
    if "fasta_pack" in per:
        moved = int(d.numel()) + int(args.bases)
        doc["pack_bytes_read_plus_written"] = moved
        doc["pack_bytes_per_s"] = moved / (float(np.median(per["fasta_pack"])) * 1e-3)
        doc["pack_fraction_of_copy_rate"] = doc["pack_bytes_per_s"] / COPY_RATE
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in doc if k not in ("limits", "tool")}))


if __name__ == "__main__":
    main()
