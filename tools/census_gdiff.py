#!/usr/bin/env python
"""Rejections at 0.05 of the differential usage between two groups of replicates (DESIGN 3.30's census): 3 + 3 replicates of two
EM goldens, made by tests/gdiff_util.py::replicates, solved by the oracle's EM through the host form (no GPU) -- `null` (every
sample from one theta), `overdispersed` (each sample's theta Dirichlet around the one theta: a null with biological variation)
and `shift` (group B from the reversed theta), under both p-values: chi-squared on lr_between, and the quasi-likelihood F test
that divides by the within-group dispersion.

  python tools/census_gdiff.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gdiff_util as GU  # noqa: E402
from conftest import load_golden  # noqa: E402


def main():
    from oracle import OracleLib, build
    from strawberry_amd import gdiff
    build(with_ref=False)
    oracle = OracleLib()
    for name in ("em_random_256", "em_c3_400"):
        a = load_golden(name)[0]
        theta = oracle.em_batch(a.row_off, a.iso_off, a.f_off, a.count, a.F)[0]
        out = {"set": name, "sizes": "3+3"}
        for mode in ("null", "overdispersed", "shift"):
            ga, gb = GU.replicates(a, mode, 3, 3, 5, theta)
            out[mode] = GU.census(gdiff.em_gdiff_host(ga, gb, None, oracle.em_batch))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
