#!/usr/bin/env python
"""The differential isoform usage on the C3 batch against a second draw of it, and on two chain samples of one annotation: what
sbgpu_em_diff_device / sbgpu_model_diff_device cost, stage by stage, beside one plain EM solve of each parent and the drop-one
support on the same parent.

  python tools/bench_diff.py --out profiles/diff_bench.json

C3 batch (synth.make_c3, em.EmBatchSolver; the second draw keeps the weights and redraws every bin's count as Poisson(count)):
after a warm-up, `reps` times in turns, each bracketed by device events on a stream of its own that the calls are given (the
calls synchronise on it before they return, so an event pair brackets the whole call):
  diff_device_ms     sbgpu_em_diff_device, no host array asked for (the host's part -- shapes, the sub-batch's plan -- included)
  diff_download_ms   the same with all 24 arrays brought to the host
  em_solve_a_ms / em_solve_b_ms   one sbgpu_em_run_device on each parent's plan and arrays
  support_device_ms  sbgpu_em_loo_device on parent A, no host array asked for
with sbgpu_set_timing on, the call's launches as stages of their own (diff_colscale, diff_expand, diff_em, diff_cross, the fit's
three twice, diff_stat; one chunk): `stage_reps` calls, medians with min - max.
Chain samples (two chain.ChainQuantifier, resident, keep_bootstrap=True, on two contexts of device 0, sample_seed 31 and 32): the
same for sbgpu_model_diff_device / sbgpu_model_loo_device on the steps' handles; the EM solve beside them is the "em kernels"
stage of one more timed step of each."""
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


def measure(torch, ctx, dev, reps, stage_reps, calls, none):
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
    _lib.check(ctx.L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per = []
        for _ in range(stage_reps):
            none(sp)
            per.append(stages(ctx))
    finally:
        ctx.L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: summary([p[k] for p in per]) for k in per[0]}
    return doc


def census(t):
    from strawberry_amd import diff
    ok = (t.diff_status == diff.OK) & (t.lost_shift == 0)
    p = t.p_value()
    with np.errstate(invalid="ignore"):
        rejected = int((p[ok] < 0.05).sum())
    return {"loci": int(t.n_loci), "compared": int(ok.sum()), "shifted": int(((t.diff_status == diff.OK) & (t.lost_shift != 0)).sum()),
            "rejected_at_0_05": rejected, "negative": int((t.lr_stat[ok] < 0).sum()), "smallest": float(t.lr_stat[ok].min()) if ok.any() else 0.0,
            "status": {n: int((t.diff_status == k).sum()) for k, n in enumerate(diff.STATUS_NAMES)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-loci", type=int, default=60000)
    ap.add_argument("--c3-frags", type=float, default=2e8)
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, chain, diff, em, synth
    ctx = em.default_context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_diff.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "stage_reps": args.stage_reps, "limits": diff.limits()}
    none, loo_none = _lib.sbgpu_em_diff_t(), _lib.sbgpu_em_loo_t()
    # ---- the C3 batch and a second draw of it
    a = synth.make_c3(args.c3_loci, args.c3_frags)
    b = synth.LocusBatch(a.row_off, a.iso_off, a.f_off, np.random.default_rng(5).poisson(a.count).astype(np.int32), a.F, a.length, "C3, second draw")
    sa, sb = em.EmBatchSolver(a, ctx), em.EmBatchSolver(b, ctx, d_F=None)
    for s in (sa, sb):
        s.run_em()
        s.synchronize()
    pa, pb = ([s.d_count.data_ptr(), s.d_F.data_ptr(), s.d_theta.data_ptr(), s.d_status.data_ptr(), s.d_iters.data_ptr()] for s in (sa, sb))

    def c3_none(sp):        # (the C entry itself: no host array asked for, no wrapper around it)
        _lib.check(L.sbgpu_em_diff_device(ctx.h, sa.plan.h, pa[0], pa[1], sb.plan.h, pb[0], pb[1], None, None, None, sp, C.byref(none)), "sbgpu_em_diff_device")

    def c3_all(sp):
        return diff.em_diff_device(ctx, sa.plan, pa[0], pa[1], sb.plan, pb[0], pb[1], stream=sp)

    def em_of(s, p):
        def run(sp):
            _lib.check(L.sbgpu_em_run_device(ctx.h, s.plan.h, p[0], p[1], p[2], p[3], p[4], sp), "sbgpu_em_run_device")
            _lib.check(L.sbgpu_synchronize(ctx.h, sp), "sbgpu_synchronize")
        return run

    def c3_support(sp):
        _lib.check(L.sbgpu_em_loo_device(ctx.h, sa.plan.h, pa[0], pa[1], None, None, sp, C.byref(loo_none)), "sbgpu_em_loo_device")
    calls = {"diff_device_ms": c3_none, "diff_download_ms": c3_all, "em_solve_a_ms": em_of(sa, pa), "em_solve_b_ms": em_of(sb, pb), "support_device_ms": c3_support}
    doc["c3"] = measure(torch, ctx, dev, args.reps, args.stage_reps, calls, c3_none)
    torch.cuda.synchronize(dev)
    m = doc["c3"]
    m.update(n_loci=a.n_loci, n_bins_a=int(a.row_off[-1]), n_bins_b=int(b.row_off[-1]), n_iso=int(a.iso_off[-1]), n_elem=int(a.f_off[-1]), census=census(c3_all(None)),
             diff_over_em_solves=m["diff_device_ms"]["median"] / (m["em_solve_a_ms"]["median"] + m["em_solve_b_ms"]["median"]),
             diff_over_support=m["diff_device_ms"]["median"] / m["support_device_ms"]["median"])
    print(json.dumps({"c3": {k: v for k, v in m.items() if k != "stage_ms"}}), flush=True)
    del sa, sb
    # ---- two chain samples of one annotation, on two contexts
    ctx_b = em.Context(0)
    kw = dict(n_loci=args.loci, n_frags=args.frags, seed=31, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    qa, qb = chain.ChainQuantifier(ctx, sample_seed=31, **kw), chain.ChainQuantifier(ctx_b, sample_seed=32, **kw)
    try:
        for q in (qa, qb):
            q.step()
            q.step()
        ha, hb, ka, kb = qa.context_handle, qb.context_handle, int(qa._out.d_keep), int(qb._out.d_keep)

        def chain_none(sp):
            _lib.check(L.sbgpu_model_diff_device(ctx.h, ha, ctx_b.h, hb, ka, kb, None, sp, C.byref(none)), "sbgpu_model_diff_device")

        def chain_all(sp):
            return diff.model_diff_device(ctx, ha, ctx_b, hb, ka, kb, stream=sp)

        def chain_support(sp):
            _lib.check(L.sbgpu_model_loo_device(ctx.h, ha, ka, None, sp, C.byref(loo_none)), "sbgpu_model_loo_device")
        calls = {"diff_device_ms": chain_none, "diff_download_ms": chain_all, "support_device_ms": chain_support}
        doc["chain"] = measure(torch, ctx, dev, args.reps, args.stage_reps, calls, chain_none)
        m = doc["chain"]
        m.update(n_loci=qa.n_loci, n_iso=qa.n_iso, n_bins_a=qa.info["n_bins"], n_bins_b=qb.info["n_bins"], n_frags_a=int(qa.n_frags), n_frags_b=int(qb.n_frags),
                 census=census(chain_all(None)), diff_over_support=m["diff_device_ms"]["median"] / m["support_device_ms"]["median"])
        m["step_stage_ms_a"], m["step_stage_ms_b"] = qa.stage_ms(), qb.stage_ms()     # one more step of each, timed: "em kernels" is the solve beside
        em_ms = [x.get("em kernels") for x in (m["step_stage_ms_a"], m["step_stage_ms_b"])]
        m["diff_over_em_solves"] = m["diff_device_ms"]["median"] / sum(em_ms) if all(em_ms) else None
    finally:
        qa.close(), qb.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": {k: v for k, v in doc["chain"].items() if k != "stage_ms"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
