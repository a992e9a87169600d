#!/usr/bin/env python
"""Two chain samples of one annotation on ONE bin table: what the merge (sbgpu_model_diff_merged_device) costs, stage
by stage, and the merged differential call beside the unmerged one on the same two quantifiers.

  python tools/bench_merge.py --out profiles/merge_bench.json

Two chain.ChainQuantifier (resident, keep_bootstrap=True, sample_seed 31 and 32, on two contexts of device 0: the pair
tools/bench_diff.py times), under that tool's method: after a warm-up, `reps` times in turns, each bracketed by device events on
a stream of its own that the calls are given (the calls synchronise on it before they return):
  merged_diff_ms     sbgpu_model_diff_merged_device, no host array asked for (the host's part included)
  unmerged_diff_ms   sbgpu_model_diff_device on the same handles
  merge_only_ms      sbgpu_model_diff_merged_device without the test (out NULL): the two cross-law weight launches, match, fill
with sbgpu_set_timing on, the merge-only call's launches as stages of their own (merge_xweights_a, merge_xweights_b, merge_match,
merge_fill): `stage_reps` calls, medians with min - max.  The union's size is reported: bins per sample, A-only and B-only bins,
loci whose status turned TOO_DEEP."""
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

from bench_diff import census, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--frags", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--min-isoform-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, chain, diff, em, merge
    ctx, ctx_b = em.default_context(0), em.Context(0)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    doc = {"tool": "tools/bench_merge.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "stage_reps": args.stage_reps, "limits": merge.limits()}
    none, merged = _lib.sbgpu_em_diff_t(), _lib.sbgpu_bins_merged_t()
    kw = dict(n_loci=args.loci, n_frags=args.frags, seed=31, resident=True, min_isoform_frac=args.min_isoform_frac, keep_bootstrap=True)
    qa, qb = chain.ChainQuantifier(ctx, sample_seed=31, **kw), chain.ChainQuantifier(ctx_b, sample_seed=32, **kw)
    try:
        for q in (qa, qb):
            q.step()
            q.step()
        ha, hb, ka, kb = qa.context_handle, qb.context_handle, int(qa._out.d_keep), int(qb._out.d_keep)

        def merged_diff(sp):
            _lib.check(L.sbgpu_model_diff_merged_device(ctx.h, ha, ctx_b.h, hb, ka, kb, None, sp, C.byref(none), C.byref(merged)), "sbgpu_model_diff_merged_device")

        def unmerged_diff(sp):
            _lib.check(L.sbgpu_model_diff_device(ctx.h, ha, ctx_b.h, hb, ka, kb, None, sp, C.byref(none)), "sbgpu_model_diff_device")

        def merge_only(sp):
            _lib.check(L.sbgpu_model_diff_merged_device(ctx.h, ha, ctx_b.h, hb, ka, kb, None, sp, None, C.byref(merged)), "sbgpu_model_diff_merged_device")
        calls = {"merged_diff_ms": merged_diff, "unmerged_diff_ms": unmerged_diff, "merge_only_ms": merge_only}
        m = doc["chain"] = measure(torch, ctx, dev, args.reps, args.stage_reps, calls, merge_only)
        t = diff.model_diff_merged_device(ctx, ha, ctx_b, hb, ka, kb, merged_want=("row_a", "row_b"))
        u = diff.model_diff_device(ctx, ha, ctx_b, hb, ka, kb)
        g = t.merged
        m.update(n_loci=qa.n_loci, n_iso=qa.n_iso, n_bins_a=qa.info["n_bins"], n_bins_b=qb.info["n_bins"], n_elem_a=qa.info["n_elem"], n_elem_b=qb.info["n_elem"],
                 n_pairs_a=qa.info["n_pairs"], n_pairs_b=qb.info["n_pairs"], n_bins_union=g.n_bins, n_elem_union=g.n_elem,
                 a_only_bins=int((g.row_b < 0).sum()), b_only_bins=int((g.row_a < 0).sum()), shared_bins=int(((g.row_a >= 0) & (g.row_b >= 0)).sum()),
                 too_deep_merged=int((t.diff_status == diff.TOO_DEEP).sum()), too_deep_unmerged=int((u.diff_status == diff.TOO_DEEP).sum()),
                 census_merged=census(t), census_unmerged=census(u),
                 # every merged weight is one 8-byte load and one 8-byte store, in both samples; per row two maps, two counts and their sources
                 fill_bytes=int(2 * 16 * g.n_elem + 32 * g.n_bins),
                 merged_over_unmerged=m["merged_diff_ms"]["median"] / m["unmerged_diff_ms"]["median"])
        # the merged call's UNSOLVED loci: which of the three solves ended DENOM_ZERO (2), and what the unmerged call said of those loci
        uns = t.diff_status == diff.UNSOLVED
        one_sided = np.add.reduceat(np.concatenate([(g.row_a < 0) | (g.row_b < 0), [False]]).astype(np.int64), g.row_off[:-1]) * (np.diff(g.row_off) > 0)
        m["unsolved_merged"] = {"loci": int(uns.sum()), "denom_zero_a": int((t.status_a[uns] == 2).sum()), "denom_zero_b": int((t.status_b[uns] == 2).sum()),
                                "denom_zero_pooled": int((t.status_pooled[uns] == 2).sum()),
                                "shifted_unmerged": int(((u.diff_status == diff.OK) & (u.lost_shift != 0) & uns).sum()),
                                "with_one_sided_rows": int((one_sided[uns] > 0).sum())}
        fill = m["stage_ms"].get("merge_fill")
        if fill and fill["median"] > 0:
            m["fill_gb_per_s"] = m["fill_bytes"] / fill["median"] / 1e6
    finally:
        qa.close(), qb.close()
    doc["total_s"] = time.perf_counter() - t0
    print(json.dumps({"chain": doc["chain"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
