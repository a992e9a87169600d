#!/usr/bin/env python
"""The transcript-body coverage profile on the chain sample: what sbgpu_body_profile_device costs beside the isoform-resolved
coverage's and the fragment assignment's calls on the same retained inputs.

  python tools/bench_body.py --loci 60000 --frags 2e8 --out profiles/body_bench.json

ChainQuantifier, resident, keep_context=True; the sample has no strands of its own: the loci are taken as unknown, + and - in
turns (the orientation changes a flush index only).  After a warm-up of every call it times, with device events on a stream of its
own that all calls are given (they synchronise on it before they return, so an event pair brackets the whole call: the upload
of the offsets, work items and prefix lengths, the memset, the kernels), `reps` times in turns so that a drift of the machine
falls on all alike:
  body_p20_ms / body_p100_ms            sbgpu_body_profile_device at P = 20 and P = 100, no host array asked for
  body_p20_download_ms / _p100_         the same with all six arrays brought to the host (8 n_iso (P + 3) bytes)
  coverage_device_ms                    sbgpu_isoform_coverage_device, no host array asked for -- the yardstick: this pass is that
                                        walk plus the bin arithmetic
  assign_device_ms                      sbgpu_fragment_assign_device, no host array asked for
then, with sbgpu_set_timing on, the profile's three launches as stages of their own (body_column: asg_column_kernel, unchanged;
body_hit; body_iso): `stage_reps` calls at each P, medians.  Reported, not asserted: the class curves, bias_3p, the share of
expressed isoforms with body_cv above 1, how many loci keep their sums in LDS and in copies at each P."""
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


def stages(ctx):
    ms, names = (C.c_float * 16)(), (C.c_char_p * 16)()
    n = ctx.L.sbgpu_last_stage_ms(ctx.h, 16, ms, names)
    return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, assign, body, chain, coverage, em
    ctx = em.default_context(0)
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_context=True)
    try:
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
        strand = np.repeat(np.arange(q.n_loci) % 3, np.diff(np.asarray(q.annot.iso_off, np.int64))).astype(np.uint8)

        def profile(P, want):
            return lambda: body.body_profile_device(ctx, h, q.annot, q._ht, d_theta, d_hit_mass=d_mass, iso_strand=strand, n_pos=P, stream=sp, want=want)
        calls = {"body_p20_ms": profile(20, ()), "body_p100_ms": profile(100, ()), "body_p20_download_ms": profile(20, None),
                 "body_p100_download_ms": profile(100, None),
                 "coverage_device_ms": lambda: coverage.isoform_coverage_device(ctx, h, q.annot, q._ht, d_theta, d_hit_mass=d_mass, stream=sp, want=()),
                 "assign_device_ms": lambda: assign.fragment_assign_device(ctx, h, d_theta, q.n_hits, d_hit_mass=d_mass, stream=sp, want=())}
        for fn in calls.values():       # warm-up: code objects, the scratch slots' first allocation
            fn(), fn()
        n_exon, n_feat = int(np.asarray(q.annot.exon_off)[-1]), int(q.hits.feat_off[-1])
        lim = body.limits()
        doc = {"tool": "tools/bench_body.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(q.dev),
               "n_loci": q.n_loci, "n_iso": q.n_iso, "n_exon": n_exon, "n_hits": q.n_hits, "n_features": n_feat, "n_frags": int(q.n_frags),
               "compat_words": q.annot.compat_words, "n_bins": q.info["n_bins"], "n_elem": q.info["n_elem"], "min_isoform_frac": args.min_isoform_frac,
               "reps": args.reps, "stage_reps": args.stage_reps, "limits": lim}
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                ms[k].append(device_ms(fn))
        doc.update({k: summary(v) for k, v in ms.items()})
        for P in (20, 100):
            doc["body_p%d_over_coverage" % P] = doc["body_p%d_ms" % P]["median"] / doc["coverage_device_ms"]["median"]
        _lib.check(L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
        try:
            for P in (20, 100):
                per = []
                for _ in range(args.stage_reps):
                    profile(P, ())()
                    per.append(stages(ctx))
                doc["stage_ms_p%d" % P] = {k: summary([p[k] for p in per]) for k in per[0]}
        finally:
            L.sbgpu_set_timing(ctx.h, 0)
        iso_off, exon_off = np.asarray(q.annot.iso_off, np.int64), np.asarray(q.annot.exon_off, np.int64)
        niso, nex = np.diff(iso_off), np.diff(exon_off[iso_off])
        for P in (20, 100):
            in_lds = (niso <= lim["lds_iso"]) & (nex <= lim["lds_exons"]) & (niso * P <= lim["lds_sums"])
            doc["loci_in_lds_p%d" % P] = int(in_lds.sum())
            doc["loci_with_copies_p%d" % P] = int((in_lds & (niso <= lim["narrow_iso"]) & (niso * P * lim["copies"] <= lim["lds_sums"])).sum())
            t = profile(P, None)()
            some = t.body_total > 0.0
            doc["sample_p%d" % P] = {"class_n": t.class_n.tolist(), "class_curve": [t.class_curve(c).tolist() for c in range(4)],
                                     "bias_3p": t.bias_3p(), "bias_3p_by_class": [t.bias_3p(c) for c in range(4)],
                                     "expressed_isoforms": int(some.sum()), "share_cv_above_1": float((t.body_cv[some] > 1.0).mean()),
                                     "median_cv": float(np.median(t.body_cv[some])), "median_center": float(np.median(t.body_center[some]))}
        doc["total_s"] = time.perf_counter() - t0
        print(json.dumps({k: v for k, v in doc.items() if not k.startswith("sample_")}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)
    finally:
        q.close()


if __name__ == "__main__":
    main()
