#!/usr/bin/env python
"""The isoform information on the C3 batch and on the chain sample: what sbgpu_em_info_device / sbgpu_model_info_device cost
beside one plain EM solve, the model fit and a B = 100 bootstrap on the same data, and how its standard errors compare with the
bootstrap's spread.

  python tools/bench_info.py --out profiles/info_bench.json

C3 batch (synth.make_c3, em.EmBatchSolver): after a warm-up, `reps` times in turns, each bracketed by device events on a stream
of its own that the calls are given (the information and the fit synchronise on it before they return, so an event pair
brackets the whole call):
  info_device_ms     sbgpu_em_info_device, no host array asked for
  info_download_ms   the same with all ten arrays brought to the host
  em_solve_ms        one sbgpu_em_run_device on the same plan and arrays
  fit_device_ms      sbgpu_em_fit_device, no host array asked for
then `boot_reps` times a B = 100 bootstrap (bootstrap_ms), and, with sbgpu_set_timing on, the information's three launches as
stages of their own (info_column: asg_column_kernel, unchanged; info_wave, info_block): `stage_reps` calls, medians.
Chain sample (chain.ChainQuantifier, resident, keep_bootstrap=True): the same for sbgpu_model_info_device / sbgpu_model_fit_device /
sbgpu_abundance_bootstrap_device on the step's handle; the EM solve beside them is the "em kernels" stage of one more timed step.
Reported, not asserted: over the loci with rank == n_free, status OK and every theta_j above 1 % of the locus' total, the median
and the 5 - 95 % range of se / (bootstrap sd); how many loci and isoforms are ALIASED / UNOBSERVED / TOO_WIDE."""
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


def measure(torch, ctx, dev, reps, boot_reps, stage_reps, calls, boot, info_none):
    """calls: name -> fn(stream address), timed in turns; boot: fn(stream address), timed boot_reps times"""
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
            info_none(sp)
            per.append(stages(ctx))
    finally:
        ctx.L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: summary([p[k] for p in per]) for k in per[0]}
    doc["info_kernels_ms"] = doc["stage_ms"]["info_wave"]["median"] + doc["stage_ms"]["info_block"]["median"]
    doc["info_over_em_solve"] = doc["info_device_ms"]["median"] / doc["em_solve_ms"]["median"] if "em_solve_ms" in doc else None
    doc["bootstrap_over_info"] = doc["bootstrap_ms"]["median"] / doc["info_device_ms"]["median"]
    return doc


def census(t, theta, boot_var):
    """the counts, and se against the bootstrap's sd where the comparison means something"""
    from strawberry_amd import info
    nl = t.n_loci
    locus_of = np.repeat(np.arange(nl), np.diff(t.iso_off))
    theta = np.asarray(theta, np.float64)[:t.n_iso]
    total = np.bincount(locus_of, weights=theta, minlength=nl)
    small = np.bincount(locus_of, weights=(theta <= 0.01 * total[locus_of]) & (t.ident == info.IDENTIFIED), minlength=nl) > 0
    good = (t.info_status == info.OK) & (t.rank == t.n_free) & ~small
    sd = np.sqrt(np.asarray(boot_var, np.float64)[:t.n_iso])
    use = good[locus_of] & (t.ident == info.IDENTIFIED) & (sd > 0) & (t.se > 0)
    ratio = t.se[use] / sd[use]
    doc = {"loci": {name: int((t.info_status == k).sum()) for k, name in enumerate(info.STATUS_NAMES)},
           "isoforms": {name: int((t.ident == k).sum()) for k, name in enumerate(info.IDENT_NAMES)},
           "loci_rank_deficient": int(((t.info_status == info.OK) & (t.rank < t.n_free)).sum()),
           "loci_compared": int(good.sum()), "isoforms_compared": int(use.sum())}
    if ratio.size:
        doc["se_over_bootstrap_sd"] = {"median": float(np.median(ratio)), "p05": float(np.percentile(ratio, 5)), "p95": float(np.percentile(ratio, 95))}
    return doc


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, bootstrap, chain, em, info, synth
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_info.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "boot_reps": args.boot_reps, "n_rep": args.n_rep, "stage_reps": args.stage_reps, "limits": info.limits()}
    no_info, no_fit = _lib.sbgpu_em_info_t(), _lib.sbgpu_em_fit_t()
    # ---- the C3 batch
    b = synth.make_c3(args.c3_loci, args.c3_frags)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    s.synchronize()
    ptrs = [s.d_count.data_ptr(), s.d_F.data_ptr(), s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr()]

    def c3_info_none(sp):        # (the C entry itself: no host array asked for, no wrapper around it)
        _lib.check(L.sbgpu_em_info_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], sp, C.byref(no_info)), "sbgpu_em_info_device")

    def c3_info_all(sp):
        return info.em_info_device(ctx, s.plan, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], stream=sp)

    def c3_em(sp):
        _lib.check(L.sbgpu_em_run_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], sp), "sbgpu_em_run_device")
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")

    def c3_fit(sp):
        _lib.check(L.sbgpu_em_fit_device(ctx.h, s.plan.h, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], sp, C.byref(no_fit)), "sbgpu_em_fit_device")
    last = {}

    def c3_boot(sp):             # (asynchronous on torch's current stream: measure() makes its stream current; the wait ends the bracket)
        last["boot"] = s.run_bootstrap(args.n_rep, 7)
        _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
    calls = {"info_device_ms": c3_info_none, "info_download_ms": c3_info_all, "em_solve_ms": c3_em, "fit_device_ms": c3_fit}
    doc["c3"] = measure(torch, ctx, dev, args.reps, args.boot_reps, args.stage_reps, calls, c3_boot, c3_info_none)
    torch.cuda.synchronize(dev)
    t = c3_info_all(None)
    doc["c3"].update(n_loci=b.n_loci, n_bins=int(b.row_off[-1]), n_iso=int(b.iso_off[-1]), n_elem=int(b.f_off[-1]),
                     census=census(t, s.d_theta.cpu().numpy(), last["boot"]["var"].cpu().numpy()))
    print(json.dumps({"c3": {k: v for k, v in doc["c3"].items() if k != "stage_ms"}}), flush=True)
    # ---- the chain sample
    q = chain.ChainQuantifier(ctx, n_loci=args.loci, n_frags=args.frags, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    try:
        q.step()
        q.step()
        h = q.context_handle
        d_theta, d_keep, d_status = int(q._out.d_theta), int(q._out.d_keep), int(q._out.d_status)

        def chain_info_none(sp):
            _lib.check(L.sbgpu_model_info_device(ctx.h, h, d_theta, d_keep, d_status, sp, C.byref(no_info)), "sbgpu_model_info_device")

        def chain_info_all(sp):
            return info.model_info_device(ctx, h, d_theta, d_keep, d_status, stream=sp)

        def chain_fit(sp):
            _lib.check(L.sbgpu_model_fit_device(ctx.h, h, d_theta, d_keep, d_status, sp, C.byref(no_fit)), "sbgpu_model_fit_device")

        def chain_boot(sp):
            last["chain_boot"] = bootstrap.abundance_bootstrap_device(ctx, h, args.n_rep, 7, replicates=False, stream=sp)
            _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
        calls = {"info_device_ms": chain_info_none, "info_download_ms": chain_info_all, "fit_device_ms": chain_fit}
        doc["chain"] = measure(torch, ctx, dev, args.reps, args.boot_reps, args.stage_reps, calls, chain_boot, chain_info_none)
        first = chain_info_all(None)
        doc["chain"].update(n_loci=q.n_loci, n_iso=q.n_iso, n_bins=q.info["n_bins"], n_elem=q.info["n_elem"], n_hits=q.n_hits, n_frags=int(q.n_frags),
                            census=census(first, q.theta[:q.n_iso], last["chain_boot"]["theta_var"]))
        doc["chain"]["step_stage_ms"] = q.stage_ms()      # one more step, timed: its "em kernels" stage is the solve beside the information
        em_ms = doc["chain"]["step_stage_ms"].get("em kernels")
        doc["chain"]["info_over_em_solve"] = doc["chain"]["info_device_ms"]["median"] / em_ms if em_ms else None
    finally:
        q.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": {k: v for k, v in doc["chain"].items() if k != "stage_ms"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
