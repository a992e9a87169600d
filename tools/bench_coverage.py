#!/usr/bin/env python
"""The isoform-resolved coverage on the chain sample: what sbgpu_isoform_coverage_device costs beside the fragment assignment's and
the `-f` table's calls on the same retained inputs.

  python tools/bench_coverage.py --loci 60000 --frags 2e8 --out profiles/coverage_bench.json

ChainQuantifier, resident, keep_context=True.  After a warm-up of every call it times, with device events on a stream of its
own that all three calls are given (they synchronise on it before they return, so an event pair brackets the whole call: the
upload of the offsets and work items, the memset, the kernels), alternating so that a drift of the machine falls on all alike:
  coverage_device_ms  sbgpu_isoform_coverage_device, no host array asked for
  assign_device_ms    sbgpu_fragment_assign_device, no host array asked for -- the yardstick: the coverage pass does its work
                      (the posterior of every hit) plus one merge walk per (hit, candidate)
  table_device_ms     sbgpu_context_table_device, no host array asked for
  coverage_download_ms the coverage with all four arrays brought to the host (16 bytes per annotated exon, 8 per isoform and locus)
hit_pass_bytes is the coverage's algorithmic traffic computed from the shapes: per hit the bin rank, the compat words, the mass,
its two feature offsets' share (8) and 9 bytes per feature; per work item its 24-byte record; once F and the gains (8 bytes
each), the exon table (8 bytes per isoform, 8 per exon) and the results (16 bytes per exon, 8 per isoform and per locus).
--kernel-loop N: only N x (resident + coverage), for a `rocprofv3 --kernel-trace --stats` run of its own; --kernel-stats FILE
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

ITEM_BYTES = 24         # sizeof(sb::HitItem), csrc/stage_host.h


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(x, 4) for x in ms]}


def kernel_stats(path):
    """rocprofv3's *_kernel_stats.csv -> {kernel: (calls, average us)} for the coverage's kernels (and the column pass it launches)"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "cov_" in name or "asg_" in name:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        ks = kernel_stats(args.kernel_stats)
        doc["kernels"] = ks
        if "cov_hit_kernel" in ks:
            doc["hit_pass"] = {"algorithmic_bytes": doc["hit_pass_bytes"], "GBps": doc["hit_pass_bytes"] / (ks["cov_hit_kernel"]["avg_us"] * 1e-6) / 1e9}
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps({k: doc[k] for k in ("kernels", "hit_pass") if k in doc}))
        return
    import torch
    from strawberry_amd import _lib, assign, chain, coverage, em
    ctx = em.default_context(0)
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_context=True)
    try:
        if args.kernel_loop:
            for _ in range(args.kernel_loop):
                q.step()
                q.isoform_coverage(want=())
            print(json.dumps({"kernel_loop": args.kernel_loop, "n_hits": q.n_hits}))
            return
        stream = torch.cuda.Stream(device=q.dev)
        sp = C.c_void_p(stream.cuda_stream)

        def device_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        t0 = time.perf_counter()
        q.step()
        q.step()
        d_theta, d_mass = int(q._out.d_theta), q.hits.mass.data_ptr()
        h = q.context_handle
        empty_t = _lib.sbgpu_context_table_t()

        def coverage_none():
            coverage.isoform_coverage_device(ctx, h, q.annot, q._ht, d_theta, d_hit_mass=d_mass, stream=sp, want=())

        def coverage_all():
            return coverage.isoform_coverage_device(ctx, h, q.annot, q._ht, d_theta, d_hit_mass=d_mass, stream=sp)

        def assign_none():
            assign.fragment_assign_device(ctx, h, d_theta, q.n_hits, d_hit_mass=d_mass, stream=sp, want=())

        def table_none():
            _lib.check(L.sbgpu_context_table_device(ctx.h, h, sp, C.byref(empty_t)), "sbgpu_context_table_device")
        for fn in (coverage_none, coverage_all, assign_none, table_none):      # warm-up: code objects, the scratch slots' first allocation
            fn(), fn()
        n_exon, n_feat = int(np.asarray(q.annot.exon_off)[-1]), int(q.hits.feat_off[-1])
        doc = {"tool": "tools/bench_coverage.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(q.dev),
               "n_loci": q.n_loci, "n_iso": q.n_iso, "n_exon": n_exon, "n_hits": q.n_hits, "n_features": n_feat, "n_frags": int(q.n_frags),
               "compat_words": q.annot.compat_words, "n_bins": q.info["n_bins"], "n_elem": q.info["n_elem"], "min_isoform_frac": args.min_isoform_frac,
               "reps": args.reps, "limits": coverage.limits()}
        ms = {"coverage_device_ms": [], "assign_device_ms": [], "table_device_ms": [], "coverage_download_ms": []}
        for _ in range(args.reps):
            ms["coverage_device_ms"].append(device_ms(coverage_none))
            ms["assign_device_ms"].append(device_ms(assign_none))
            ms["table_device_ms"].append(device_ms(table_none))
            ms["coverage_download_ms"].append(device_ms(coverage_all))
        doc.update({k: summary(v) for k, v in ms.items()})
        doc["coverage_over_assign"] = doc["coverage_device_ms"]["median"] / doc["assign_device_ms"]["median"]
        per_locus = np.diff(np.asarray(q.hits.locus_hit_off[:q.n_loci + 1], np.int64))
        item_hits = doc["limits"]["item_hits"]
        items = int(((per_locus + item_hits - 1) // item_hits).sum())
        cw = q.annot.compat_words
        doc["work_items"] = items
        doc["hit_pass_bytes"] = int(q.n_hits * (4 + 4 * cw + 4 + 8) + 9 * n_feat + ITEM_BYTES * items + 8 * q.info["n_elem"] + 8 * q.n_iso
                                    + 8 * q.n_iso + 8 * n_exon + 16 * n_exon + 8 * q.n_iso + 8 * q.n_loci)
        doc["coverage_call_GBps_over_hit_pass_bytes"] = doc["hit_pass_bytes"] / (doc["coverage_device_ms"]["median"] * 1e-3) / 1e9
        c = coverage_all()
        iso_off, exon_off = np.asarray(q.annot.iso_off, np.int64), np.asarray(q.annot.exon_off, np.int64)
        niso, nex = np.diff(iso_off), np.diff(exon_off[iso_off])
        lim = doc["limits"]
        doc["loci_with_copies"] = int(((niso <= lim["narrow_iso"]) & (nex <= lim["copy_exons"])).sum())
        doc["loci_beyond_lds"] = int(((niso > lim["lds_iso"]) | (nex > lim["lds_exons"])).sum())
        doc["covered_exons"] = int((c.exon_bases > 0.0).sum())
        doc["supported_junctions"] = int((c.junction_mass > 0.0).sum())
        doc["unexplained_share"] = float(c.unexplained_bases.sum() / (c.unexplained_bases.sum() + c.iso_bases.sum()))
        doc["total_s"] = time.perf_counter() - t0
        print(json.dumps(doc), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)
    finally:
        q.close()


if __name__ == "__main__":
    main()
