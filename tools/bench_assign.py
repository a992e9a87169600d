#!/usr/bin/env python
"""The fragment assignment on the chain sample: what sbgpu_fragment_assign_device costs beside the `-f` table's call on the same
retained inputs and beside the resident step itself.

  python tools/bench_assign.py --loci 60000 --frags 2e8 --out profiles/assign_bench.json

ChainQuantifier, resident, keep_context=True.  After a warm-up of every call it times, with device events on a stream of its
own that both calls are given (they synchronise on it before they return, so an event pair brackets the whole call: the upload
of the offsets and work items, the kernels, and -- the table only -- the download its row count sizes):
  assign_device_ms   sbgpu_fragment_assign_device, no host array asked for (nothing but the call's own synchronisation crosses PCIe)
  assign_download_ms the same with all seven arrays brought to the host (16 bytes per hit)
  table_device_ms    sbgpu_context_table_device with no host array asked for: existing code whose count pass reads the same
                     per-hit bytes (bin rank 4 + compat words 4 cw) -- the yardstick
  resident_stage_ms  the resident step's kernel stages from the library's own events (sbgpu_set_timing), and resident_wall_ms
                     the host clock around the synchronising step
hit_pass_bytes is the assignment's algorithmic traffic computed from the shapes: per hit the bin rank, the compat words, the
mass and the three results (4 + 4 cw + 4 + 16), per work item its 24-byte record, once F (8 bytes per weight) and the gains.
--kernel-loop N: only N x (resident + assignment), for a `rocprofv3 --kernel-trace --stats` run of its own; --kernel-stats FILE
merges that run's per-kernel averages into the JSON and derives the hit pass' GB/s over hit_pass_bytes."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITEM_HITS = 16384       # csrc/assign_device.h: kAsgItemHits
ITEM_BYTES = 24         # sizeof(sb::HitItem), csrc/stage_host.h


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(x, 4) for x in ms]}


def kernel_stats(path):
    """rocprofv3's *_kernel_stats.csv -> {kernel: (calls, average us)} for the assignment's and the table's kernels"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "asg_" in name or "ctx_" in name:
            out[name.split("(")[0].split("::")[-1]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        ks = kernel_stats(args.kernel_stats)
        doc["kernels"] = ks
        if "asg_hit_kernel" in ks:
            doc["hit_pass"] = {"algorithmic_bytes": doc["hit_pass_bytes"], "GBps": doc["hit_pass_bytes"] / (ks["asg_hit_kernel"]["avg_us"] * 1e-6) / 1e9}
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps({k: doc[k] for k in ("kernels", "hit_pass") if k in doc}))
        return
    import torch
    from strawberry_amd import _lib, assign, chain, em
    ctx = em.default_context(0)
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_context=True)
    try:
        if args.kernel_loop:
            for _ in range(args.kernel_loop):
                q.step()
                q.fragment_assignment(want=())
            print(json.dumps({"kernel_loop": args.kernel_loop, "n_hits": q.n_hits}))
            return
        stream = torch.cuda.Stream(device=q.dev)
        sp = C.c_void_p(stream.cuda_stream)

        def device_ms(fn, reps):
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return out
        t0 = time.perf_counter()
        q.step()
        q.step()
        wall = []
        for _ in range(5):
            t = time.perf_counter()
            q.step()        # (synchronises: its results are downloaded)
            wall.append((time.perf_counter() - t) * 1e3)
        stages = q.stage_ms()
        d_theta, d_mass = int(q._out.d_theta), q.hits.mass.data_ptr()
        h = q.context_handle
        empty_t = _lib.sbgpu_context_table_t()

        def assign_none():
            assign.fragment_assign_device(ctx, h, d_theta, q.n_hits, d_hit_mass=d_mass, stream=sp, want=())

        def assign_all():
            assign.fragment_assign_device(ctx, h, d_theta, q.n_hits, d_hit_mass=d_mass, stream=sp)

        def table_none():
            _lib.check(L.sbgpu_context_table_device(ctx.h, h, sp, C.byref(empty_t)), "sbgpu_context_table_device")
        for fn in (assign_none, assign_all, table_none):      # warm-up: code objects, the scratch slots' first allocation
            fn(), fn()
        doc = {"tool": "tools/bench_assign.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(q.dev),
               "n_loci": q.n_loci, "n_iso": q.n_iso, "n_hits": q.n_hits, "n_frags": int(q.n_frags), "compat_words": q.annot.compat_words,
               "n_bins": q.info["n_bins"], "n_elem": q.info["n_elem"], "min_isoform_frac": args.min_isoform_frac, "reps": args.reps}
        # alternating, so that a drift of the machine falls on all three alike
        ms = {"assign_device_ms": [], "table_device_ms": [], "assign_download_ms": []}
        for _ in range(args.reps):
            ms["assign_device_ms"] += device_ms(assign_none, 1)
            ms["table_device_ms"] += device_ms(table_none, 1)
            ms["assign_download_ms"] += device_ms(assign_all, 1)
        doc.update({k: summary(v) for k, v in ms.items()})
        per_locus = np.diff(np.asarray(q.hits.locus_hit_off[:q.n_loci + 1], np.int64))
        items = int(((per_locus + ITEM_HITS - 1) // ITEM_HITS).sum())
        cw = q.annot.compat_words
        doc["work_items"] = items
        doc["hit_pass_bytes"] = int(q.n_hits * (4 + 4 * cw + 4 + 16) + ITEM_BYTES * items + 8 * q.info["n_elem"] + 8 * q.n_iso)
        doc["count_pass_bytes_of_the_table"] = int(q.n_hits * (4 + 4 * cw) + ITEM_BYTES * items)
        doc["assign_call_GBps_over_hit_pass_bytes"] = doc["hit_pass_bytes"] / (doc["assign_device_ms"]["median"] * 1e-3) / 1e9
        doc["assign_d2h_bytes_all_arrays"] = int(16 * q.n_hits + 24 * q.n_iso + 8 * q.n_loci)
        doc["resident_stage_ms"] = {k: round(v, 4) for k, v in stages.items()}
        doc["resident_stage_sum_ms"] = float(sum(stages.values()))
        doc["resident_wall_ms"] = summary(wall)
        a = assign.fragment_assign_device(ctx, h, d_theta, q.n_hits, d_hit_mass=d_mass, stream=sp)
        doc["assigned_hits"] = int((a.map_iso >= 0).sum())
        doc["ambiguous_hits"] = int((a.n_cand > 1).sum())
        doc["total_s"] = time.perf_counter() - t0
        print(json.dumps(doc), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)
    finally:
        q.close()


if __name__ == "__main__":
    main()
