#!/usr/bin/env python
"""The variational Bayes solve on the C3 batch and on the chain sample: what sbgpu_em_vb_device / sbgpu_model_vb_device cost
beside one plain EM solve on the same data.  It records; it gates nothing, and no ratio is promised.

  python tools/bench_vb.py --out profiles/vb_bench.json

C3 batch (synth.make_c3, em.EmBatchSolver): after a warm-up, `reps` times in turns, each bracketed by device events on a stream of
its own that the calls are given (the solve synchronises on it before it returns, so an event pair brackets the whole call):
  vb_alpha_0.01_ms, vb_alpha_1_ms   sbgpu_em_vb_device at the two priors, no host array asked for
  em_solve_ms                       one sbgpu_em_run_device on the same plan and arrays
with both solvers' total iterations, the loci by the device form that serves them, and -- with sbgpu_set_timing on -- the two
launches (vb_wave, vb_block) as stages of their own.
Chain sample (chain.ChainQuantifier, resident, keep_bootstrap=True): sbgpu_model_vb_device on the step's handle at alpha = 0.01;
the EM solve beside it is the "em" stage of one more timed step."""
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


def timed(torch, dev, calls, reps):
    """calls: name -> fn(stream address) -> name -> summary of `reps` event-bracketed calls, in turns"""
    stream = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(stream.cuda_stream)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    return {k: summary(v) for k, v in ms.items()}, sp


def forms(rows, niso, lim):
    wave = rows * niso <= lim["wave_vals"]
    staged = ~wave & (rows * niso + rows + 2 * niso <= lim["stage_doubles"])
    return {"loci_wave_form": int(wave.sum()), "loci_block_form_lds": int(staged.sum()), "loci_block_form_scratch": int((~wave & ~staged).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-loci", type=int, default=60000)
    ap.add_argument("--c3-frags", type=float, default=2e8)
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vb_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, chain, em, synth, vb
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    lim = vb.limits()
    doc = {"tool": "tools/bench_vb.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "stage_reps": args.stage_reps, "limits": lim}
    empty = _lib.sbgpu_em_vb_t()
    # ---- the C3 batch
    b = synth.make_c3(args.c3_loci, args.c3_frags)
    s = em.EmBatchSolver(b, ctx)
    ptrs = [s.d_count.data_ptr(), s.d_F.data_ptr(), s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr()]

    def c3_vb(alpha):
        par = _lib.sbgpu_vb_params_t(alpha, 1e-2, 1000, 0)
        return lambda sp: _lib.check(L.sbgpu_em_vb_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], C.byref(par), sp, C.byref(empty)), "sbgpu_em_vb_device")

    def c3_em(sp):
        _lib.check(L.sbgpu_em_run_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], sp), "sbgpu_em_run_device")
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
    c3, sp = timed(torch, dev, {"vb_alpha_0.01_ms": c3_vb(0.01), "vb_alpha_1_ms": c3_vb(1.0), "em_solve_ms": c3_em}, args.reps)
    _lib.check(L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per = []
        for _ in range(args.stage_reps):
            c3_vb(0.01)(sp)
            per.append(stages(ctx))
    finally:
        L.sbgpu_set_timing(ctx.h, 0)
    c3["stage_ms_alpha_0.01"] = {k: summary([p[k] for p in per]) for k in per[0]}
    em_iters = int(s.results()["iters"].sum())
    for alpha in (0.01, 1.0):
        t = s.run_vb(alpha=alpha)
        c3["vb_alpha_%g" % alpha] = {"iterations": int(t.iters.sum()), "status_counts": np.bincount(t.status, minlength=4).tolist(),
                                     "isoforms_at_least_one_fragment": int(t.supported().sum())}
    r = s.results()
    c3.update(n_loci=b.n_loci, n_bins=int(b.row_off[-1]), n_iso=int(b.iso_off[-1]), n_elem=int(b.f_off[-1]), em_iterations=em_iters,
              em_isoforms_at_least_one_fragment=int((r["theta"] >= 1.0).sum()), **forms(np.diff(b.row_off), np.diff(b.iso_off), lim))
    doc["c3"] = c3
    print(json.dumps({"c3": {k: v for k, v in c3.items() if not k.startswith("stage_ms")}}), flush=True)
    # ---- the chain sample
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    try:
        q.step()
        q.step()
        h = q.context_handle

        def chain_vb(sp):
            _lib.check(L.sbgpu_model_vb_device(ctx.h, h, None, sp, C.byref(empty)), "sbgpu_model_vb_device")
        ch, _ = timed(torch, dev, {"model_vb_ms": chain_vb}, args.reps)
        t = q.variational()
        ch.update(n_loci=q.n_loci, n_iso=q.n_iso, n_bins=q.info["n_bins"], n_elem=q.info["n_elem"], n_hits=q.n_hits, vb_iterations=int(t.iters.sum()),
                  em_iterations=int(q.iters[:q.n_loci].sum()), status_counts=np.bincount(t.status, minlength=4).tolist(),
                  isoforms_at_least_one_fragment=int(t.supported().sum()), em_isoforms_at_least_one_fragment=int((q.theta[:q.n_iso] >= 1.0).sum()))
        ch["step_stage_ms"] = q.stage_ms()      # one more step, timed: its "em" stage is the solve beside the variational one
        doc["chain"] = ch
    finally:
        q.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": doc["chain"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
