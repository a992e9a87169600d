#!/usr/bin/env python
"""The differential isoform usage between two groups of replicates on six chain samples of one annotation: what
sbgpu_model_gdiff_device costs at 3 + 3 and at 1 + 1, stage by stage, beside the unchanged two-sample call
(sbgpu_model_diff_device) on the same quantifiers in the same run.

  python tools/bench_gdiff.py --out profiles/gdiff_bench.json

Six chain.ChainQuantifier (resident, keep_bootstrap=True) on six contexts of device 0: group A is sample_seed 31, replicate 0 .. 2,
group B sample_seed 32, replicate 0 .. 2; --frags fragments PER SAMPLE (the default is chosen so that six samples' records, bins and
weights lie beside each other in HBM).  By tools/bench_diff.py's method: after two warm-up calls each, `reps` times in turns, each
call bracketed by device events on a stream of its own that the call is given (it synchronises on it before it returns); no
host array asked for:
  gdiff_3_3_ms   sbgpu_model_gdiff_device on all six
  gdiff_1_1_ms   sbgpu_model_gdiff_device on the first sample of each group
  diff_ms        sbgpu_model_diff_device on the same two
with sbgpu_set_timing on, each call's launches as stages of their own: `stage_reps` calls, medians with min - max."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_info import stages, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=3e7, help="fragments per sample")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gdiff_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, chain, em, gdiff
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_gdiff.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "stage_reps": args.stage_reps, "frags_per_sample": args.frags, "limits": gdiff.limits()}
    ctxs = [ctx] + [em.Context(0) for _ in range(5)]
    kw = dict(n_loci=args.loci, n_frags=args.frags, seed=31, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    qs = [chain.ChainQuantifier(c, sample_seed=31 + s // 3, replicate=s % 3, **kw) for s, c in enumerate(ctxs)]
    try:
        for q in qs:
            q.step()
            q.step()
        arr = lambda v: (C.c_void_p * len(v))(*v)  # noqa: E731
        none, none2 = _lib.sbgpu_em_gdiff_t(), _lib.sbgpu_em_diff_t()
        pick = {"gdiff_3_3_ms": (3, 3, qs), "gdiff_1_1_ms": (1, 1, [qs[0], qs[3]])}

        def gdiff_call(n_a, n_b, group):
            c, h, k = arr([q.ctx.h for q in group]), arr([q.context_handle for q in group]), arr([int(q._out.d_keep) for q in group])

            def run(sp):
                _lib.check(L.sbgpu_model_gdiff_device(n_a, n_b, c, h, k, None, sp, C.byref(none)), "sbgpu_model_gdiff_device")
            return run

        def diff_call(sp):
            _lib.check(L.sbgpu_model_diff_device(ctx.h, qs[0].context_handle, qs[3].ctx.h, qs[3].context_handle, int(qs[0]._out.d_keep), int(qs[3]._out.d_keep),
                                                 None, sp, C.byref(none2)), "sbgpu_model_diff_device")
        calls = {k: gdiff_call(*v) for k, v in pick.items()}
        calls["diff_ms"] = diff_call
        stream = torch.cuda.Stream(device=dev)
        sp = C.c_void_p(stream.cuda_stream)

        def device_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn(sp)
                e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        for fn in calls.values():          # warm-up: code objects, the scratch slots' first allocation
            device_ms(fn), device_ms(fn)
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                ms[k].append(device_ms(fn))
        doc.update({k: summary(v) for k, v in ms.items()})
        _lib.check(L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
        try:
            doc["stage_ms"] = {}
            for k, fn in calls.items():
                per = []
                for _ in range(args.stage_reps):
                    fn(sp)
                    per.append(stages(ctx))
                doc["stage_ms"][k] = {name: summary([p[name] for p in per]) for name in per[0]}
        finally:
            L.sbgpu_set_timing(ctx.h, 0)
        import gdiff_util as GU  # (its census of a result)
        full = chain.ChainQuantifier.differential_usage_groups(qs[:3], qs[3:])
        doc.update(n_loci=qs[0].n_loci, n_iso=qs[0].n_iso, n_bins=[q.info["n_bins"] for q in qs], n_frags=[int(q.n_frags) for q in qs], census_3_3=GU.census(full),
                   status_3_3={n: int((full.gdiff_status == k).sum()) for k, n in enumerate(gdiff.STATUS_NAMES)},
                   gdiff_1_1_over_diff=doc["gdiff_1_1_ms"]["median"] / doc["diff_ms"]["median"],
                   gdiff_3_3_over_diff=doc["gdiff_3_3_ms"]["median"] / doc["diff_ms"]["median"])
    finally:
        for q in qs:
            q.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({k: v for k, v in doc.items() if k != "stage_ms"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
