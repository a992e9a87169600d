#!/usr/bin/env python3
"""GPU box: the five stages' wall times of the resident records -> theta pass (bench.py --workload c3-front's sample and
FrontQuantifier.step), step by step -- a plain bench.py line carries the pass' time only.  One JSON line per step behind the
warm-up steps; the library is SBGPU_LIB's (A/B: one process per library, alternating).
usage: front_stage_times.py [steps=8] [warmup=2]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from strawberry_amd import em, front
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ctx = em.Context(0)
q = front.FrontQuantifier(ctx, n_loci=int(float(os.environ.get("SB_FRONT_LOCI", "60000"))), n_frags=float(os.environ.get("SB_FRONT_FRAGS", "2e8")),
                          seed=31, resident=True, empirical=True)
torch.cuda.empty_cache()
for i in range(warmup + steps):
    q.step()
    if i >= warmup:
        print(json.dumps({"step": i - warmup, "stage_wall_ms": dict(q.stage_wall_ms)}), flush=True)
q.close()
