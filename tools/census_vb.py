#!/usr/bin/env python
"""False positives of the maximum-likelihood EM against the variational Bayes solve, on synthetic loci whose truth leaves some
isoforms at zero (DESIGN 3.31's table).  CPU only: the VB solve is the library's host form (sbgpu_em_vb_host); the EM beside it is
the plain maximum-likelihood iteration on the same column-normalised weights, from theta = N / K, stopped as the library's EM is
(step norm below 1e-2 fragments, 1000 iterations at most), written here in numpy.

  python tools/census_vb.py --out profiles/vb_census.json

Per class of loci (isoforms, bins, depth): `loci` loci; a share of the isoforms is expressed (Dirichlet shares), the others have no
fragment in truth; the bins' counts are one multinomial draw.  Counted per solver: isoforms reported at or above one fragment that
have none in truth (false positives), expressed isoforms reported below one fragment (misses), and the mean absolute error on the
expressed ones in fragments."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = [dict(niso=4, bins=9, depth=200), dict(niso=8, bins=24, depth=1000), dict(niso=16, bins=60, depth=3000),
           dict(niso=65, bins=200, depth=20000), dict(niso=200, bins=500, depth=50000)]


def make_locus(rng, niso, bins, depth, expressed):
    """-> (counts, F, truth in fragments): every bin is compatible with a random third of the isoforms, at least one"""
    F = rng.uniform(0.02, 0.3, (bins, niso)) * (rng.random((bins, niso)) < 1.0 / 3.0)
    F[np.arange(bins), rng.integers(0, niso, bins)] = rng.uniform(0.02, 0.3, bins)
    F[rng.integers(0, bins, niso), np.arange(niso)] = rng.uniform(0.02, 0.3, niso)      # every isoform has a bin
    on = np.zeros(niso, bool)
    on[rng.permutation(niso)[:max(1, int(round(expressed * niso)))]] = True
    share = np.zeros(niso)
    share[on] = rng.dirichlet(np.ones(int(on.sum())))
    lam = (F / F.sum(axis=0)) @ share
    return rng.multinomial(depth, lam / lam.sum()).astype(np.int32), F, share * depth


def em_ml(n, F, change_limit=1e-2, max_iter=1000):
    A = F / F.sum(axis=0)
    theta = np.full(F.shape[1], n.sum() / F.shape[1])
    for _ in range(max_iter):
        d = A @ theta
        nxt = theta * (A.T @ np.where(n > 0, n / np.where(d > 0, d, 1.0), 0.0))
        if np.sqrt(((nxt - theta) ** 2).sum()) < change_limit:
            break
        theta = nxt
    return theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=200)
    ap.add_argument("--expressed", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vb_census.json"))
    args = ap.parse_args()
    from strawberry_amd import synth, vb
    rng = np.random.default_rng(args.seed)
    doc = {"tool": "tools/census_vb.py", "loci_per_class": args.loci, "expressed_share": args.expressed, "seed": args.seed, "classes": []}
    for c in CLASSES:
        loci = [make_locus(rng, c["niso"], c["bins"], c["depth"], args.expressed) for _ in range(args.loci)]
        b = synth.from_loci([(n, F) for n, F, _ in loci])
        truth = np.concatenate([t for _, _, t in loci])
        got = {"em": np.concatenate([em_ml(n, F) for n, F, _ in loci]), "vb_alpha_0.01": vb.em_vb_host(b, alpha=0.01).count,
               "vb_alpha_1": vb.em_vb_host(b, alpha=1.0).count}
        row = dict(c, isoforms=int(truth.size), expressed=int((truth > 0).sum()))
        for k, x in got.items():
            row[k] = {"false_positives": int(((x >= 1.0) & (truth == 0)).sum()), "misses": int(((x < 1.0) & (truth >= 1.0)).sum()),
                      "mean_abs_error_expressed": float(np.abs(x - truth)[truth > 0].mean())}
        doc["classes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
