#!/usr/bin/env python
"""The splicing events' PSI on the chain sample: what the event table's host build, its upload, sbgpu_splice_psi_device at one row and
at a bootstrap's rows, and the statistics pass over the PSI matrix cost, beside two yardsticks of the same process.

  python tools/bench_splice.py --loci 60000 --frags 2e8 --n-rep 100 --out profiles/splice_bench.json

ChainQuantifier, resident, keep_bootstrap=True: one step, then one bootstrap of --n-rep replicates whose d_fpkm_rep / d_keep_rep the
PSI kernel reads as they stand.  Host work is timed on the wall clock; device work with device events on a stream of its own around
windows that end in a synchronisation, `reps` times in turns so that a drift of the machine falls on all alike:
  build_host_ms            SpliceEvents.build (both host calls: shapes, then build)
  upload_ms                SpliceEvents.to_device, synchronised (wall clock)
  psi_rows1_ms             sbgpu_splice_psi_device on the step's d_fpkm / d_keep
  psi_rowsB_ms             sbgpu_splice_psi_device on the bootstrap's d_fpkm_rep / d_keep_rep (n_rows = n_rep)
  psi_rowsB_nokeep_ms      the same without keep
  stats_ms                 sbgpu_replicate_stats_device over d_psi[n_rep][n_events]
  support_ms               sbgpu_splice_support_device on two per-exon arrays
  locus_abundance_ms       one sbgpu_locus_abundance_device launch -- the yardstick of a one-row pass over the isoforms
  bootstrap_per_rep_ms     sbgpu_abundance_bootstrap_device over n_rep replicates, per replicate -- what one more row of PSI rides on
Reported, not asserted: the census (events, alternative, skipped, retained), the bytes each PSI call reads and writes, the share of
defined events and the median interval width of the alternative ones."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--n-rep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--boot-reps", type=int, default=2)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, bootstrap, chain, em, splice
    ctx = em.default_context(0)
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    try:
        t0 = time.perf_counter()
        stream = torch.cuda.Stream(device=q.dev)
        sp = C.c_void_p(stream.cuda_stream)

        def device_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def wall_ms(fn):
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(q.dev)
            return (time.perf_counter() - t) * 1e3, r
        build_ms, upload_ms = [], []
        for _ in range(3):
            ms, ev = wall_ms(lambda: splice.SpliceEvents.build(q.annot))
            build_ms.append(ms)
            ms, d_ev = wall_ms(lambda: ev.to_device(ctx))
            upload_ms.append(ms)
        q.step()
        q.step()
        B, nu, n_iso = args.n_rep, ev.n_events, q.n_iso
        lo, hi = bootstrap.interval_ranks(B, 0.95)

        last = {}

        def boot():
            last.update(q.abundance_bootstrap(B, 11, replicates=False, stream=sp))
        boot()                  # warm-up; then timed, before anything reads the replicates (a later bootstrap may move them)
        boot_ms = [device_ms(boot) / B for _ in range(args.boot_reps)]
        d_fpkm_rep, d_keep_rep = last["device"]["fpkm_rep"], last["device"]["keep_rep"]
        d_fpkm, d_keep = int(q._out.d_fpkm), int(q._out.d_keep)
        dev = q.dev
        psi1 = torch.zeros((1, nu), dtype=torch.float64, device=dev)
        psiB = torch.zeros((B, nu), dtype=torch.float64, device=dev)
        defined = torch.zeros(nu, dtype=torch.int32, device=dev)
        stats = [torch.zeros(nu, dtype=torch.float64, device=dev) for _ in range(4)]
        rng = np.random.default_rng(3)
        d_xb, d_jm = (torch.from_numpy(rng.gamma(2.0, 50.0, ev.n_exons)).to(dev) for _ in range(2))
        support = torch.zeros(nu, dtype=torch.float64, device=dev)
        d_iso_off = torch.from_numpy(np.ascontiguousarray(q.annot.iso_off, np.int64)).to(dev)
        d_total = torch.tensor([q.total_fpkm], dtype=torch.float64, device=dev)
        loc = [torch.zeros(q.n_loci, dtype=torch.float64, device=dev), torch.zeros(q.n_loci, dtype=torch.float64, device=dev),
               torch.zeros(q.n_loci, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize(dev)
        s = d_ev.struct

        def psi(n_rows, x, keep, out):
            return lambda: _lib.check(L.sbgpu_splice_psi_device(ctx.h, C.byref(s), n_rows, x, keep, out.data_ptr(), defined.data_ptr(), sp), "sbgpu_splice_psi_device")
        calls = {
            "psi_rows1_ms": psi(1, d_fpkm, d_keep, psi1),
            "psi_rowsB_ms": psi(B, d_fpkm_rep, d_keep_rep, psiB),
            "psi_rowsB_nokeep_ms": psi(B, d_fpkm_rep, None, psiB),
            "stats_ms": lambda: _lib.check(L.sbgpu_replicate_stats_device(ctx.h, B, nu, psiB.data_ptr(), lo, hi, *(t.data_ptr() for t in stats), sp),
                                           "sbgpu_replicate_stats_device"),
            "support_ms": lambda: _lib.check(L.sbgpu_splice_support_device(ctx.h, C.byref(s), d_xb.data_ptr(), d_jm.data_ptr(), support.data_ptr(), sp),
                                             "sbgpu_splice_support_device"),
            "locus_abundance_ms": lambda: _lib.check(L.sbgpu_locus_abundance_device(ctx.h, q.n_loci, d_iso_off.data_ptr(), d_fpkm, d_keep, d_total.data_ptr(),
                                                                                    loc[0].data_ptr(), loc[1].data_ptr(), loc[2].data_ptr(), sp),
                                                     "sbgpu_locus_abundance_device"),
        }
        for fn in calls.values():       # warm-up: code objects
            fn(), fn()
        stream.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                ms[k].append(device_ms(fn))
        # the PSI matrix once more (the no-keep call wrote it last), for the census of what it says
        calls["psi_rowsB_ms"]()
        calls["stats_ms"]()
        stream.synchronize()
        niso = np.diff(np.asarray(q.annot.iso_off, np.int64))[ev.event_locus]
        n_incl = ev.n_incl_of.astype(np.int64)
        table_bytes = int(nu * (4 + 1 + 4 + 4 + 16) + ev.n_incl * 4 + 8 * q.n_loci + 8 * n_iso)
        census = ev.census()
        census.update(n_incl=int(ev.n_incl), loci=q.n_loci, isoforms=n_iso, exons=int(ev.n_exons), widest_locus=int(niso.max(initial=0)),
                      events_in_wide_loci=int((niso > splice.limits()["mask_iso"]).sum()), mean_span=float(ev.n_span.mean()), mean_incl=float(n_incl.mean()))
        dcount = defined.cpu().numpy()
        width = (stats[3] - stats[2]).cpu().numpy()
        alt = ev.alternative() & (dcount == B)
        doc = {"tool": "tools/bench_splice.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "n_rep": B,
               "rank_lo": lo, "rank_hi": hi, "reps": args.reps, "boot_reps": args.boot_reps, "n_frags": int(q.n_frags), "n_hits": q.n_hits,
               "min_isoform_frac": args.min_isoform_frac, "limits": splice.limits(), "census": census,
               "build_host_ms": summary(build_ms), "upload_ms": summary(upload_ms), "table_bytes": table_bytes,
               # the distinct bytes a call touches: every row of x and keep once (the lanes of a locus share them), the table, the matrix
               "bytes_rows1": {"read": int(12 * n_iso + table_bytes), "written": int(8 * nu + 4 * nu)},
               "bytes_rowsB": {"read": int(12 * n_iso * B + table_bytes), "written": int(8 * nu * B + 4 * nu)},
               "psi_matrix_bytes": int(8 * nu * B), "replicate_matrices_bytes": int(12 * n_iso * B)}
        doc.update({k: summary(v) for k, v in ms.items()})
        doc["bootstrap_per_rep_ms"] = summary(boot_ms)
        doc["psi_rowsB_GBps"] = (doc["bytes_rowsB"]["read"] + doc["bytes_rowsB"]["written"]) / doc["psi_rowsB_ms"]["median"] / 1e6
        doc["psi_rows1_over_locus_abundance"] = doc["psi_rows1_ms"]["median"] / doc["locus_abundance_ms"]["median"]
        doc["psi_per_row_over_bootstrap_per_rep"] = doc["psi_rowsB_ms"]["median"] / B / doc["bootstrap_per_rep_ms"]["median"]
        doc["stats_over_bootstrap_per_rep"] = doc["stats_ms"]["median"] / B / doc["bootstrap_per_rep_ms"]["median"]
        doc["sample"] = {"defined_in_every_replicate": float((dcount == B).mean()), "never_defined": float((dcount == 0).mean()),
                         "alternative_and_defined": int(alt.sum()), "median_interval_width_there": float(np.median(width[alt])) if alt.any() else None}
        doc["total_s"] = time.perf_counter() - t0
        print(json.dumps(doc), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)
    finally:
        q.close()


if __name__ == "__main__":
    main()
