#!/usr/bin/env python
"""The drop-one isoform support on the C3 batch and on the chain sample: what sbgpu_em_loo_device / sbgpu_model_loo_device cost,
stage by stage, beside one plain EM solve of the parent and a B = 100 bootstrap on the same data; and the census of what it
finds.

  python tools/bench_support.py --out profiles/support_bench.json

C3 batch (synth.make_c3, em.EmBatchSolver): after a warm-up, `reps` times in turns, each bracketed by device events on a stream
of its own that the calls are given (the support synchronises on it before it returns, so an event pair brackets the whole call):
  support_device_ms    sbgpu_em_loo_device, no host array asked for (the host's part -- shapes, the sub-batch's plan -- included)
  support_download_ms  the same with all thirteen arrays brought to the host
  em_solve_ms          one sbgpu_em_run_device on the parent's plan and arrays
then `boot_reps` times a B = 100 bootstrap (bootstrap_ms); with sbgpu_set_timing on, the support's launches as stages of their
own (loo_expand, loo_em, fit_column, fit_wave, fit_block, loo_stat; one chunk): `stage_reps` calls, medians; the expand kernel's
GB/s against the bytes it writes (the sub-batch's weights and counts); and, on the host clock, the shapes and the sub-batch's
plan (plan_host_ms), which the call makes before its first launch.
Chain sample (chain.ChainQuantifier, resident, keep_bootstrap=True): the same for sbgpu_model_loo_device /
sbgpu_abundance_bootstrap_device on the step's handle; the EM solve beside them is the "em kernels" stage of one more timed step."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_info import stages, summary  # noqa: E402


def measure(torch, ctx, dev, reps, boot_reps, stage_reps, calls, boot, none):
    from strawberry_amd import _lib
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
    for fn in calls.values():          # warm-up: code objects, the scratch slot's first allocation
        device_ms(fn), device_ms(fn)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    doc = {k: summary(v) for k, v in ms.items()}
    device_ms(boot)
    doc["bootstrap_ms"] = summary([device_ms(boot) for _ in range(boot_reps)])
    _lib.check(ctx.L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per = []
        for _ in range(stage_reps):
            none(sp)
            per.append(stages(ctx))
    finally:
        ctx.L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: summary([p[k] for p in per]) for k in per[0]}
    doc["fit_ms"] = sum(doc["stage_ms"][k]["median"] for k in ("fit_column", "fit_wave", "fit_block") if k in doc["stage_ms"])
    if "em_solve_ms" in doc:
        doc["support_over_em_solve"] = doc["support_device_ms"]["median"] / doc["em_solve_ms"]["median"]
    doc["bootstrap_over_support"] = doc["bootstrap_ms"]["median"] / doc["support_device_ms"]["median"]
    return doc


def sub_batch_figures(ctx, row_off, iso_off, keep, stage_ms, reps=5):
    """the sub-batch's sizes, the expand kernel's GB/s against what it writes, the host's part on the host clock"""
    from strawberry_amd import em, support
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sh = support.shapes_host(row_off, iso_off, keep)
        plan = em.Plan(ctx, sh["row_off"], sh["iso_off"], sh["f_off"])
        ms.append((time.perf_counter() - t0) * 1e3)
        plan.close()
    written = 8 * int(sh["f_off"][-1]) + 4 * int(sh["row_off"][-1])
    doc = {"n_sub": len(sh["sub_locus"]), "sub_rows": int(sh["row_off"][-1]), "sub_iso": int(sh["iso_off"][-1]), "sub_elem": int(sh["f_off"][-1]),
           "expand_written_bytes": written, "plan_host_ms": summary(ms)}
    if "loo_expand" in stage_ms:
        doc["expand_gb_per_s"] = written / (stage_ms["loo_expand"]["median"] * 1e-3) / 1e9
    return doc


def census(t):
    from strawberry_amd import support
    c = t.support == support.TESTED
    return {"candidates": int(c.sum()), "sole": int((t.support == support.SOLE).sum()), "inf": int(np.isposinf(t.lr_stat[c]).sum()),
            "below_3_84": int((t.lr_stat[c] < 3.84).sum()), "negative": int((t.lr_stat[c] < 0).sum()),
            "smallest": float(t.lr_stat[c].min()) if c.any() else 0.0, "too_wide_loci": int((t.loo_status == support.TOO_WIDE).sum()),
            "empty_loci": int((t.loo_status == support.EMPTY).sum()), "not_kept": int((t.support == support.NOT_KEPT).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-loci", type=int, default=60000)
    ap.add_argument("--c3-frags", type=float, default=2e8)
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--boot-reps", type=int, default=3)
    ap.add_argument("--n-rep", type=int, default=100)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "support_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, bootstrap, chain, em, support, synth
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_support.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "boot_reps": args.boot_reps, "n_rep": args.n_rep, "stage_reps": args.stage_reps, "limits": support.limits()}
    none = _lib.sbgpu_em_loo_t()
    # ---- the C3 batch
    b = synth.make_c3(args.c3_loci, args.c3_frags)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    s.synchronize()
    ptrs = [s.d_count.data_ptr(), s.d_F.data_ptr(), s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr()]

    def c3_none(sp):        # (the C entry itself: no host array asked for, no wrapper around it)
        _lib.check(L.sbgpu_em_loo_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], None, None, sp, C.byref(none)), "sbgpu_em_loo_device")

    def c3_all(sp):
        return support.em_loo_device(ctx, s.plan, ptrs[0], ptrs[1], stream=sp)

    def c3_em(sp):
        _lib.check(L.sbgpu_em_run_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], sp), "sbgpu_em_run_device")
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")

    def c3_boot(sp):        # (asynchronous on torch's current stream: measure() makes its stream current; the wait ends the bracket)
        s.run_bootstrap(args.n_rep, 7)
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
    calls = {"support_device_ms": c3_none, "support_download_ms": c3_all, "em_solve_ms": c3_em}
    doc["c3"] = measure(torch, ctx, dev, args.reps, args.boot_reps, args.stage_reps, calls, c3_boot, c3_none)
    torch.cuda.synchronize(dev)
    doc["c3"].update(n_loci=b.n_loci, n_bins=int(b.row_off[-1]), n_iso=int(b.iso_off[-1]), n_elem=int(b.f_off[-1]), census=census(c3_all(None)),
                     sub_batch=sub_batch_figures(ctx, b.row_off, b.iso_off, None, doc["c3"]["stage_ms"]))
    print(json.dumps({"c3": {k: v for k, v in doc["c3"].items() if k != "stage_ms"}}), flush=True)
    # ---- the chain sample
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    try:
        q.step()
        q.step()
        h, d_keep = q.context_handle, int(q._out.d_keep)
        keep = q.keep[:q.n_iso].copy()

        def chain_none(sp):
            _lib.check(L.sbgpu_model_loo_device(ctx.h, h, d_keep, None, sp, C.byref(none)), "sbgpu_model_loo_device")

        def chain_all(sp):
            return support.model_loo_device(ctx, h, d_keep, keep=keep, stream=sp)

        def chain_boot(sp):
            bootstrap.abundance_bootstrap_device(ctx, h, args.n_rep, 7, replicates=False, stream=sp)
            _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
        calls = {"support_device_ms": chain_none, "support_download_ms": chain_all}
        doc["chain"] = measure(torch, ctx, dev, args.reps, args.boot_reps, args.stage_reps, calls, chain_boot, chain_none)
        first = chain_all(None)
        row_off = np.zeros(q.n_loci + 1, np.int64)
        _lib.check(L.sbgpu_bins_export(h, row_off.ctypes.data, *([None] * 12)), "sbgpu_bins_export")
        doc["chain"].update(n_loci=q.n_loci, n_iso=q.n_iso, n_bins=q.info["n_bins"], n_elem=q.info["n_elem"], n_hits=q.n_hits, n_frags=int(q.n_frags),
                            census=census(first), sub_batch=sub_batch_figures(ctx, row_off, first.iso_off, keep, doc["chain"]["stage_ms"]))
        doc["chain"]["step_stage_ms"] = q.stage_ms()      # one more step, timed: its "em kernels" stage is the solve beside the support
        em_ms = doc["chain"]["step_stage_ms"].get("em kernels")
        doc["chain"]["support_over_em_solve"] = doc["chain"]["support_device_ms"]["median"] / em_ms if em_ms else None
    finally:
        q.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": {k: v for k, v in doc["chain"].items() if k != "stage_ms"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
