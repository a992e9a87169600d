#!/usr/bin/env python
"""The EM bootstrap on the C3 batch: what a replicate costs beyond one plain solve, and what the route a caller had before
costs.

  python tools/bench_bootstrap.py --loci 60000 --reps 100 --out profiles/bootstrap_bench.json [--plain-tree PARENT_CHECKOUT]

Device events around windows that end in a synchronisation, after a warm-up window:
  plain_split_ms_per_batch   sbgpu_em_run_device_split, batch after batch on the same batch (two output sets): the cost of one plain
                             solve in a run of batches.  Measured in a child process per build -- this tree and, with
                             --plain-tree, another built checkout of the project (the parent commit's) --, the builds alternating
  bootstrap_ms_per_replicate sbgpu_em_bootstrap_device with B = --reps, the whole call (its one wait at the start included) / B
  counts_ms_per_replicate    sbgpu_bootstrap_counts_device with B = --count-reps: the resampling alone (prefix sums once per call)
  host_route_ms_per_replicate  numpy multinomial per locus, upload, sbgpu_em_run_device, download theta, numpy Welford: the route
                             without this entry (wall clock; --host-reps replicates)
--resident: the bootstrap of the resident path on the chain sample (bench.py --workload c3-chain's generator):
  resident_bootstrap_ms_per_replicate  sbgpu_abundance_bootstrap_device on the handle of one sbgpu_quantify_resident call, the whole
                             call (its wait, the collective-free epilogues, the two statistics passes, the downloads) / B
  em_bootstrap_ms_per_replicate  sbgpu_em_bootstrap_device on the same batch (the handle's bins, sbgpu_quantify_host's weights) in
                             the same process: code the parent commit has too, the baseline
  with --kernel-loop N only N calls of the resident bootstrap, for the kernel trace.
--resident --locus: the locus bootstrap beside it, in one process on one resident call's handle:
  locus_bootstrap_ms_per_replicate     sbgpu_locus_bootstrap_device, the whole call / B
  resident_bootstrap_ms_per_replicate  sbgpu_abundance_bootstrap_device, the whole call / B: code the parent commit has too, the baseline
  with --kernel-loop N only N calls of the locus bootstrap, for the kernel trace (boot_locus_sum_kernel, boot_interval_kernel).
--kernel-loop N: only N bootstrap calls of B replicates, for a `rocprofv3 --kernel-trace --stats` run of its own;
--kernel-stats FILE merges that run's per-kernel averages (the *_kernel_stats.csv) into --out."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(float(x), 4) for x in ms]}


def event_window(torch, dev, fn):
    """fn() queues work on the current stream; -> device milliseconds between two events around it, synchronised"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1)


def plain_split(solver, steps):
    """`steps` split runs, outputs alternating between two sets, completion joined into a second stream -> ms per batch"""
    torch = solver.torch
    epi = torch.cuda.Stream(device=solver.dev)
    sets = [(solver.d_theta, solver.d_status, solver.d_iters),
            (torch.zeros_like(solver.d_theta), torch.full_like(solver.d_status, -1), torch.zeros_like(solver.d_iters))]

    def window():
        main = torch.cuda.current_stream(solver.dev)
        done = [None, None]
        for i in range(steps):
            k = i & 1
            solver.d_theta, solver.d_status, solver.d_iters = sets[k]
            if done[k] is not None:
                main.wait_event(done[k])
            solver.run_em(join_stream=epi)
            done[k] = torch.cuda.Event()
            done[k].record(epi)
        main.wait_stream(epi)
    return lambda: event_window(torch, solver.dev, window) / steps


def host_route(solver, batch, n_rep, seed):
    """What a caller did without the entry: resample on the host, upload, solve, download, accumulate -> (ms per replicate, parts)"""
    torch = solver.torch
    rng = np.random.default_rng(seed)
    nrow = batch.nrow
    N = np.add.reduceat(np.append(batch.count, 0).astype(np.int64), batch.row_off[:-1]) * (nrow > 0)
    parts = {"resample": [], "upload_solve_download": [], "statistics": []}
    m, q = np.zeros(solver.n_iso), np.zeros(solver.n_iso)
    keep = solver.d_count
    total = []
    for k in range(n_rep):
        t0 = time.perf_counter()
        rep = np.zeros_like(batch.count)
        for l in range(batch.n_loci):
            if N[l] > 0:
                r0, r1 = batch.row_off[l], batch.row_off[l + 1]
                rep[r0:r1] = rng.multinomial(N[l], batch.count[r0:r1] / N[l])
        t1 = time.perf_counter()
        solver.d_count = torch.from_numpy(rep).to(solver.dev)
        solver.run_em()
        solver.synchronize()
        x = solver.d_theta[:solver.n_iso].cpu().numpy()
        t2 = time.perf_counter()
        d = x - m
        m = m + d / (k + 1)
        q = q + d * (x - m)
        t3 = time.perf_counter()
        parts["resample"].append((t1 - t0) * 1e3), parts["upload_solve_download"].append((t2 - t1) * 1e3), parts["statistics"].append((t3 - t2) * 1e3)
        total.append((t3 - t0) * 1e3)
    solver.d_count = keep
    return summary(total), {k: summary(v) for k, v in parts.items()}


def resident_leg(args):
    """-> the --resident document (or, with --kernel-loop, just the calls)"""
    from strawberry_amd import chain, em, synth
    from strawberry_amd.quantify import quantify_host
    ctx = em.default_context(0)
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=2e8 * args.loci / 60000.0, resident=True, min_isoform_frac=0.01, keep_bootstrap=True)
    torch = q.torch
    q.step()
    run = lambda: q.abundance_bootstrap(args.reps, args.seed, level=0.95, replicates=False, locus=args.locus)  # noqa: E731
    if args.kernel_loop:
        for _ in range(args.kernel_loop):
            run()
        print(json.dumps({"kernel_loop": args.kernel_loop, "reps": args.reps, "resident": True, "locus": args.locus}))
        q.close()
        return None
    if args.locus:
        doc = {"tool": "tools/bench_bootstrap.py --resident --locus", "build_id": ctx.L.sbgpu_build_id().decode(), "n_loci": q.n_loci,
               "n_iso": q.n_iso, "n_hits": q.n_hits, "n_frags": q.n_frags, "reps": args.reps, "measured": True}
        old = lambda: q.abundance_bootstrap(args.reps, args.seed, level=0.95, replicates=False)  # noqa: E731
        first, before = run(), old()
        if any(first[k].tobytes() != before[k].tobytes() for k in ("fpkm_mean", "fpkm_var", "tpm_lo", "tpm_hi", "keep_count", "total_fpkm_rep")):
            raise RuntimeError("the locus call's isoform results differ from the old call's")
        doc["same_isoform_results_in_both_legs"] = True
        doc["loci_kept_in_all_replicates"] = int((first["locus"]["kept_count"] == args.reps).sum())
        doc["loci_kept_in_some_replicates"] = int(((first["locus"]["kept_count"] > 0) & (first["locus"]["kept_count"] < args.reps)).sum())
        a, b = [], []
        for _ in range(args.windows):       # the legs alternate: a drift of the clocks hits both
            a.append(event_window(torch, q.dev, run) / args.reps)
            b.append(event_window(torch, q.dev, old) / args.reps)
        doc["locus_bootstrap_ms_per_replicate"], doc["resident_bootstrap_ms_per_replicate"] = summary(a), summary(b)
        doc["added_ms_per_replicate"] = doc["locus_bootstrap_ms_per_replicate"]["median"] - doc["resident_bootstrap_ms_per_replicate"]["median"]
        print(json.dumps({k: doc[k] for k in ("locus_bootstrap_ms_per_replicate", "resident_bootstrap_ms_per_replicate", "added_ms_per_replicate")}), flush=True)
        q.close()
        return doc
    doc = {"tool": "tools/bench_bootstrap.py --resident", "build_id": ctx.L.sbgpu_build_id().decode(), "n_loci": q.n_loci, "n_iso": q.n_iso,
           "n_hits": q.n_hits, "n_frags": q.n_frags, "reps": args.reps, "measured": True}
    first = run()
    doc["kept_in_all_replicates"] = int((first["keep_count"] == args.reps).sum())
    doc["kept_in_some_replicates"] = int(((first["keep_count"] > 0) & (first["keep_count"] < args.reps)).sum())
    boot = lambda: event_window(torch, q.dev, run) / args.reps  # noqa: E731
    doc["resident_bootstrap_ms_per_replicate"] = summary([boot() for _ in range(args.windows)])
    print(json.dumps({"resident_bootstrap_ms_per_replicate": doc["resident_bootstrap_ms_per_replicate"]}), flush=True)
    # the same batch by hand: the bins of the sample's hits and the host entry's weights
    h = quantify_host(q.annot, q.hits.host_hits(q.n_loci), q.insert, q.read_len, ctx=ctx)
    b = h["bins"]
    mine = q.step(keep=True)     # one more resident step, its handle exported: both legs must solve the same batch
    if not (np.array_equal(mine.row_off, b.row_off) and np.array_equal(np.asarray(mine.count), np.asarray(b.count))):
        raise RuntimeError("the host entry's bins differ from the resident call's: the two legs would not solve the same batch")
    doc["same_bins_in_both_legs"] = True
    s = em.EmBatchSolver(synth.LocusBatch(b.row_off, b.iso_off, b.f_off, np.asarray(b.count, np.int32), h["F"], b.iso_len, "chain sample"), ctx)
    doc["n_rows"] = int(b.row_off[-1])
    base = lambda: event_window(torch, s.dev, lambda: s.run_bootstrap(args.reps, args.seed)) / args.reps  # noqa: E731
    base()
    doc["em_bootstrap_ms_per_replicate"] = summary([base() for _ in range(args.windows)])
    doc["added_ms_per_replicate"] = doc["resident_bootstrap_ms_per_replicate"]["median"] - doc["em_bootstrap_ms_per_replicate"]["median"]
    print(json.dumps({"em_bootstrap_ms_per_replicate": doc["em_bootstrap_ms_per_replicate"], "added_ms_per_replicate": doc["added_ms_per_replicate"]}), flush=True)
    q.close()
    return doc


def kernel_stats(path):
    """rocprofv3's *_kernel_stats.csv -> {kernel: calls, average us} for the bootstrap's kernels and the EM's"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        short = name.split("(")[0].split("::")[-1].split("<")[0]
        if "boot_" in name or "fused" in name or "em_" in name or "wide" in name or "abundance" in name:
            out[short] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--count-reps", type=int, default=8)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--plain-steps", type=int, default=50)
    ap.add_argument("--plain-tree", default=None, help="another built checkout (the parent commit's) for the plain split runs")
    ap.add_argument("--child-plain", default=None, metavar="TREE", help="(internal) the plain split runs alone, with the package of TREE")
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5742)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident", action="store_true", help="the bootstrap of the resident path on the chain sample")
    ap.add_argument("--locus", action="store_true", help="with --resident: sbgpu_locus_bootstrap_device beside sbgpu_abundance_bootstrap_device")
    args = ap.parse_args()
    if args.kernel_stats:
        doc = json.load(open(args.out))
        doc["kernels"] = kernel_stats(args.kernel_stats)
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps(doc["kernels"]))
        return
    if args.resident:
        doc = resident_leg(args)
        if doc is not None and args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
        return
    if args.child_plain:
        sys.path.insert(0, os.path.abspath(args.child_plain))
    from strawberry_amd import em, synth
    ctx = em.default_context(0)
    batch = synth.make_c3(n_loci=args.loci, total_frags=2e8 * args.loci / 60000.0)
    s = em.EmBatchSolver(batch, ctx)
    torch = s.torch
    if args.child_plain:
        f = plain_split(s, args.plain_steps)
        f()
        print(json.dumps({"build_id": ctx.L.sbgpu_build_id().decode(), "plain_split_ms_per_batch": summary([f() for _ in range(args.windows)])}))
        return
    if args.kernel_loop:
        for _ in range(args.kernel_loop):
            s.run_bootstrap(args.reps, args.seed)
            s.synchronize()
        print(json.dumps({"kernel_loop": args.kernel_loop, "reps": args.reps}))
        return
    doc = {"tool": "tools/bench_bootstrap.py", "build_id": ctx.L.sbgpu_build_id().decode(), "n_loci": batch.n_loci, "n_rows": int(batch.row_off[-1]),
           "n_iso": s.n_iso, "n_frags": batch.n_frags, "reps": args.reps, "measured": True}
    # the whole call, B replicates
    boot = lambda: event_window(torch, s.dev, lambda: s.run_bootstrap(args.reps, args.seed)) / args.reps  # noqa: E731
    boot()
    doc["bootstrap_ms_per_replicate"] = summary([boot() for _ in range(args.windows)])
    doc["draws_per_second"] = batch.n_frags / (doc["bootstrap_ms_per_replicate"]["median"] * 1e-3)
    cnt = lambda: event_window(torch, s.dev, lambda: s.bootstrap_counts(args.count_reps, args.seed)) / args.count_reps  # noqa: E731
    cnt()
    doc["counts_ms_per_replicate"] = summary([cnt() for _ in range(args.windows)])
    f = plain_split(s, args.plain_steps)
    f()
    doc["plain_split_ms_per_batch_in_process"] = summary([f() for _ in range(args.windows)])
    doc["replicate_over_plain_solve"] = doc["bootstrap_ms_per_replicate"]["median"] / doc["plain_split_ms_per_batch_in_process"]["median"]
    print(json.dumps({k: doc[k] for k in ("bootstrap_ms_per_replicate", "counts_ms_per_replicate", "plain_split_ms_per_batch_in_process")}), flush=True)
    if args.host_reps:
        doc["host_route_ms_per_replicate"], doc["host_route_parts_ms"] = host_route(s, batch, args.host_reps, args.seed)
        print(json.dumps({"host_route_ms_per_replicate": doc["host_route_ms_per_replicate"]}), flush=True)
    # the plain split runs in processes of their own, the builds alternating (this one, the other, this one, ...)
    del s
    torch.cuda.synchronize()
    trees = [("this", ROOT)] + ([("other", os.path.abspath(args.plain_tree))] if args.plain_tree else [])
    runs = []
    for _ in range(2 if args.plain_tree else 1):
        for label, tree in trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-plain", tree, "--loci", str(args.loci), "--windows", str(args.windows),
                                  "--plain-steps", str(args.plain_steps)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("the plain run under %s failed (%d): %s" % (label, out.returncode, out.stderr[-2000:]))
            runs.append(dict(label=label, **json.loads(out.stdout.strip().split("\n")[-1])))
    doc["plain_split_runs"] = runs
    print(json.dumps(runs), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
