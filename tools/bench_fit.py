#!/usr/bin/env python
"""The model fit on the C3 batch and on the chain sample: what sbgpu_em_fit_device / sbgpu_model_fit_device cost beside one plain
EM solve and the assignment's column pass on the same data.

  python tools/bench_fit.py --out profiles/fit_bench.json

C3 batch (synth.make_c3, em.EmBatchSolver): after a warm-up, `reps` times in turns, each bracketed by device events on a stream
of its own that the calls are given (the fit synchronises on it before it returns, so an event pair brackets the whole call:
the upload of the two locus lists, the column pass, the two fit kernels):
  fit_device_ms     sbgpu_em_fit_device, no host array asked for
  em_solve_ms       one sbgpu_em_run_device on the same plan and arrays
  fit_download_ms   the fit with all eleven arrays brought to the host
then, with sbgpu_set_timing on, the fit's three launches as stages of their own (fit_column: asg_column_kernel, unchanged;
fit_wave, fit_block: the fit pass): `stage_reps` calls, medians.
Chain sample (chain.ChainQuantifier, resident, keep_bootstrap=True): the same for sbgpu_model_fit_device on the step's handle;
the EM solve beside it is the "em" stage of one more timed step.
fit_pass_bytes is the fit pass' algorithmic traffic from the shapes: F twice at most (16 bytes per weight), per bin the count
(4), the live flag (1), expected and resid (16), per isoform the gain, keep and the score (20), per locus the three offsets
(24), status (4), the list entry (4) and the eight results (56)."""
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


def fit_pass_bytes(n_elem, n_bins, n_iso, n_loci):
    return int(16 * n_elem + 21 * n_bins + 20 * n_iso + 88 * n_loci)


def stages(ctx):
    ms, names = (C.c_float * 16)(), (C.c_char_p * 16)()
    n = ctx.L.sbgpu_last_stage_ms(ctx.h, 16, ms, names)
    return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}


def measure(torch, ctx, dev, reps, stage_reps, fit_none, fit_all, em_solve, shapes):
    """-> the figures of one workload; fit_none / fit_all / em_solve take the stream's address (em_solve may be None)"""
    from strawberry_amd import _lib, fit
    stream = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(stream.cuda_stream)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn(sp)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    calls = {"fit_device_ms": fit_none, "fit_download_ms": fit_all}
    if em_solve is not None:
        calls["em_solve_ms"] = em_solve
    for fn in calls.values():          # warm-up: code objects, the scratch slot's first allocation
        device_ms(fn), device_ms(fn)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    doc = {k: summary(v) for k, v in ms.items()}
    _lib.check(ctx.L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per = []
        for _ in range(stage_reps):
            fit_none(sp)
            per.append(stages(ctx))
    finally:
        ctx.L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: summary([p[k] for p in per]) for k in per[0]}
    n_elem, n_bins, n_iso, n_loci, rows, niso = shapes
    lim = fit.limits()
    wave = (rows <= lim["wave_vals"]) & (niso <= lim["wave_vals"]) & (rows * niso <= lim["wave_vals"])
    staged = ~wave & (rows * niso <= lim["stage_vals"])
    doc.update(n_loci=int(n_loci), n_bins=int(n_bins), n_iso=int(n_iso), n_elem=int(n_elem), loci_wave_form=int(wave.sum()),
               loci_block_form_staged=int(staged.sum()), loci_block_form_global=int((~wave & ~staged).sum()),
               weights_wave_form=int((rows * niso)[wave].sum()), fit_pass_bytes=fit_pass_bytes(n_elem, n_bins, n_iso, n_loci))
    pass_ms = doc["stage_ms"]["fit_wave"]["median"] + doc["stage_ms"]["fit_block"]["median"]
    doc["fit_pass_ms"] = pass_ms
    doc["fit_pass_GBps"] = doc["fit_pass_bytes"] / (pass_ms * 1e-3) / 1e9 if pass_ms > 0 else None
    doc["fit_call_GBps_over_fit_pass_bytes"] = doc["fit_pass_bytes"] / (doc["fit_device_ms"]["median"] * 1e-3) / 1e9
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-loci", type=int, default=60000)
    ap.add_argument("--c3-frags", type=float, default=2e8)
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, chain, em, fit, synth
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_fit.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "stage_reps": args.stage_reps, "limits": fit.limits()}
    # ---- the C3 batch
    b = synth.make_c3(args.c3_loci, args.c3_frags)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    s.synchronize()
    ptrs = [s.d_count.data_ptr(), s.d_F.data_ptr(), s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr()]

    def c3_fit(want):
        return lambda sp: fit.em_fit_device(ctx, s.plan, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], stream=sp, want=want)

    def c3_em(sp):
        _lib.check(L.sbgpu_em_run_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], sp), "sbgpu_em_run_device")
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
    empty = _lib.sbgpu_em_fit_t()

    def c3_fit_none(sp):        # (the C entry itself: no host array asked for, no wrapper around it)
        _lib.check(L.sbgpu_em_fit_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], sp, C.byref(empty)), "sbgpu_em_fit_device")
    shapes = (int(b.f_off[-1]), int(b.row_off[-1]), int(b.iso_off[-1]), b.n_loci, np.diff(b.row_off), np.diff(b.iso_off))
    doc["c3"] = measure(torch, ctx, dev, args.reps, args.stage_reps, c3_fit_none, c3_fit(None), c3_em, shapes)
    t = c3_fit(None)(None)
    doc["c3"]["median_reduced_chi2"] = float(np.nanmedian(t.reduced_chi2()))
    doc["c3"]["fragments_impossible"] = int(t.n_impossible.sum())
    print(json.dumps({"c3": {k: v for k, v in doc["c3"].items() if k != "stage_ms"}}), flush=True)
    # ---- the chain sample
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    try:
        q.step()
        q.step()
        h = q.context_handle
        d_theta, d_keep, d_status = int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status)

        def chain_fit(want):
            return lambda sp: fit.model_fit_device(ctx, h, d_theta, d_keep, d_status, stream=sp, want=want)
        first = chain_fit(None)(None)
        rows, niso = np.diff(first.row_off), np.diff(first.iso_off)
        shapes = (q.info["n_elem"], q.info["n_bins"], q.n_iso, q.n_loci, rows, niso)

        def chain_fit_none(sp):
            _lib.check(L.sbgpu_model_fit_device(ctx.h, h, d_theta, d_keep, d_status, sp, C.byref(empty)), "sbgpu_model_fit_device")
        doc["chain"] = measure(torch, ctx, dev, args.reps, args.stage_reps, chain_fit_none, chain_fit(None), None, shapes)
        doc["chain"].update(n_hits=q.n_hits, n_frags=int(q.n_frags), median_reduced_chi2=float(np.nanmedian(first.reduced_chi2())),
                            fragments_impossible=int(first.n_impossible.sum()), fragments_dropped=int(first.n_dropped.sum()))
        doc["chain"]["step_stage_ms"] = q.stage_ms()      # one more step, timed: its "em" stage is the solve beside the fit
    finally:
        q.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": {k: v for k, v in doc["chain"].items() if k != "stage_ms"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
