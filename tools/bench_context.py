#!/usr/bin/env python
"""The `-f` fragment-context table on the chain sample: what retention costs the resident step, what the device table
costs, and what the parent's only route to the same table costs.

  python tools/bench_context.py --loci 60000 --frags 2e8 --depths 1,0.25 --out profiles/context_table_bench.json

Per depth (the same annotation, fewer read pairs) it times, with the wall clock around calls that synchronise:
  resident_off_ms     sbgpu_quantify_resident, retention off (what the parent commit runs: compare with --label parent there)
  resident_on_ms      the same with sbgpu_context_table_keep on
  table_device_ms     sbgpu_context_table_device incl. its download; d2h_bytes is what it brings over
  host_route_ms       sbgpu_quantify_host from the same hits in host memory (compat_out asked for) + the export of hit -> bin +
                      the per-hit walk on one host thread (sbgpu_context_table_host): the route a caller had before
--kernel-loop N: only N x (resident + table), for a `rocprofv3 --kernel-trace --stats` run of its own; --kernel-stats FILE
merges that run's per-kernel averages (the *_kernel_stats.csv) into the JSON and derives the count pass' GB/s over its
algorithmic bytes (per hit: bin rank 4 + compat words 4 cw; per work item: its 24-byte record, which names the locus).
--resident-only: the resident step alone, in a process of its own; the same file run at the parent commit (--label parent,
several times for the run-to-run spread) and at this one, then --merge-resident FILES records them in the JSON.
table_d2h_bytes is computed from the array sizes the call copies (context_api.hip), not measured on the bus."""
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


COUNT_ITEM_HITS = 16384     # csrc/context_device.h: kCtxItemHits
COUNT_ITEM_BYTES = 24       # sizeof(sb::HitItem), csrc/stage_host.h


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(x, 3) for x in ms]}


def one_depth(ctx, n_loci, n_frags, reps, host_route, min_frac):
    from strawberry_amd import _lib, chain, context
    from strawberry_amd.quantify import InsertSize
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=n_loci, n_frags=n_frags, resident=True, min_isoform_frac=min_frac)
    r = {"n_loci": q.n_loci, "n_hits": q.n_hits, "n_frags": q.n_frags, "compat_words": q.annot.compat_words}
    per_locus = np.diff(np.asarray(q.hits.locus_hit_off[:q.n_loci + 1], np.int64))
    r["count_items"] = int(((per_locus + COUNT_ITEM_HITS - 1) // COUNT_ITEM_HITS).sum())   # the count pass' work items (context_api.hip)
    try:
        r["resident_off_ms"] = summary(timed(q.step, reps, warmup=2))
        off = (q.theta.copy(), q.keep.copy())
        q.keep_context = True            # (every step switches retention on for its own call)
        r["resident_on_ms"] = summary(timed(q.step, reps, warmup=2))
        r["retention_changes_no_bit"] = bool((q.theta.view(np.uint64) == off[0].view(np.uint64)).all() and (q.keep == off[1]).all())
        last = {}
        r["table_device_ms"] = summary(timed(lambda: last.update(t=q.context_table()), reps))
        t = last["t"]
        r.update(n_bins=q.info["n_bins"], n_elem=q.info["n_elem"], n_rows=t.n_rows, erased_isoforms=int((q.keep[:q.n_iso] == 0).sum()))
        r["table_d2h_bytes"] = int(8 * (q.n_loci + 1) + 4 * q.n_loci + 12 * t.n_rows + 8 * q.info["n_elem"] + 8)
        r["resident_plus_table_ms"] = r["resident_on_ms"]["median"] + r["table_device_ms"]["median"]
        if host_route:
            keep, status = q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
            hits = q.hits.host_hits(q.n_loci)
            a, h = q.annot._struct(), hits._struct()
            cw = q.annot.compat_words
            theta, st, it = np.zeros(q.n_iso + 1), np.zeros(q.n_loci + 1, np.int32), np.zeros(q.n_loci + 1, np.int32)
            compat = np.zeros((hits.n_hits, cw), np.uint32)
            ins, used = InsertSize(250.0, 30.0)._struct(q.read_len), _lib.sbgpu_insert_t()
            parts = {"quantify_host": [], "table_host": []}

            def route():
                handle = C.c_void_p()
                t0 = time.perf_counter()
                _lib.check(L.sbgpu_quantify_host(ctx.h, C.byref(a), C.byref(h), hits.mass.ctypes.data, C.byref(ins), q.read_len, 0, theta.ctypes.data,
                                                 st.ctypes.data, it.ctypes.data, compat.ctypes.data, C.byref(used), C.byref(handle)), "sbgpu_quantify_host")
                t1 = time.perf_counter()
                try:
                    th = context.context_table_host(handle, compat, keep=keep, status=status)   # (exports hit -> bin: 8 bytes per hit)
                finally:
                    L.sbgpu_bins_destroy(handle)
                parts["quantify_host"].append((t1 - t0) * 1e3)
                parts["table_host"].append((time.perf_counter() - t1) * 1e3)
                return th
            th = None
            ms = []
            for k in range(3):
                t0 = time.perf_counter()
                th = route()
                ms.append((time.perf_counter() - t0) * 1e3)
            r["host_route_ms"] = summary(ms[1:])
            r["host_route_parts_ms"] = {k: summary(v[1:]) for k, v in parts.items()}
            r["host_route_d2h_bytes_per_hit_arrays"] = int(hits.n_hits * (8 + 4 * cw))
            r["host_route_h2d_hit_bytes"] = int(sum(getattr(hits, k).nbytes for k in ("hit_locus", "feat_off", "feat_code", "feat_left", "feat_right", "mass")))
            same = all((getattr(t, k) == getattr(th, k)).all() for k in ("locus_row_off", "locus_hits", "row_bin", "row_hits")) and \
                bool((t.row_prob.view(np.uint64) == th.row_prob.view(np.uint64)).all())
            r["device_table_equals_host_table_bitwise"] = bool(same)
    finally:
        context.context_table_keep(ctx, False)
        q.close()
    return r


def resident_only(ctx, n_loci, n_frags, reps, min_frac):
    """The resident step alone, retention never touched: runs unchanged on a commit without the table (the parent)."""
    from strawberry_amd import chain
    q = chain.ChainQuantifier(ctx, n_loci=n_loci, n_frags=n_frags, resident=True, min_isoform_frac=min_frac)
    try:
        return {"n_loci": q.n_loci, "n_hits": q.n_hits, "resident_ms": summary(timed(q.step, reps, warmup=2))}
    finally:
        q.close()


def kernel_stats(path):
    """rocprofv3's *_kernel_stats.csv -> {kernel: (calls, average ns)} for the table's kernels"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "ctx_" in name:
            out[name.split("(")[0].split("::")[-1]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--depths", default="1,0.25")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident-only", action="store_true", help="time the resident step alone (works on the parent commit too)")
    ap.add_argument("--merge-resident", nargs="+", default=None, help="--resident-only results to record in --out as resident_step_runs")
    args = ap.parse_args()
    if args.merge_resident:
        doc = json.load(open(args.out))
        runs = [json.load(open(f)) for f in args.merge_resident]
        doc["resident_step_runs"] = runs
        par = [x["resident_ms"]["median"] for x in runs if x["label"] == "parent"]
        this = [x["resident_ms"]["median"] for x in runs if x["label"] != "parent"]
        if par and this:
            doc["resident_step_parent_vs_this"] = {"parent_medians_ms": par, "this_medians_ms": this, "parent_run_to_run_spread_ms": max(par) - min(par),
                                                   "this_minus_parent_ms": float(np.median(this) - np.median(par))}
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps(doc.get("resident_step_parent_vs_this")))
        return
    if args.kernel_stats:
        doc = json.load(open(args.out))
        ks = kernel_stats(args.kernel_stats)
        doc["kernels"] = ks
        d0 = doc["depths"][0]
        if "ctx_count_kernel" in ks:
            alg = d0["n_hits"] * (4 + 4 * d0["compat_words"]) + COUNT_ITEM_BYTES * d0["count_items"]
            doc["count_pass"] = {"algorithmic_bytes": int(alg), "GBps": alg / (ks["ctx_count_kernel"]["avg_us"] * 1e-6) / 1e9}
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps({k: doc[k] for k in ("kernels", "count_pass") if k in doc}))
        return
    from strawberry_amd import chain, em
    ctx = em.default_context(0)
    if args.resident_only:
        doc = {"tool": "tools/bench_context.py --resident-only", "label": args.label, "build_id": ctx.L.sbgpu_build_id().decode(),
               "min_isoform_frac": args.min_isoform_frac}
        doc.update(resident_only(ctx, args.loci, args.frags, args.reps, args.min_isoform_frac))
        print(json.dumps(doc), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
        return
    if args.kernel_loop:
        q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_context=True)
        for _ in range(args.kernel_loop):
            q.step()
            q.context_table()
        q.close()
        print(json.dumps({"kernel_loop": args.kernel_loop, "n_hits": q.n_hits}))
        return
    doc = {"tool": "tools/bench_context.py", "label": args.label, "build_id": ctx.L.sbgpu_build_id().decode(), "loci": args.loci, "frags": args.frags,
           "min_isoform_frac": args.min_isoform_frac, "depths": []}
    for d in [float(x) for x in args.depths.split(",")]:
        doc["depths"].append(dict(depth=d, **one_depth(ctx, args.loci, args.frags * d, args.reps, not args.no_host_route, args.min_isoform_frac)))
        print(json.dumps(doc["depths"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
