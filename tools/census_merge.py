#!/usr/bin/env python
"""The calibration census of DESIGN 3.29, on the CPU with the oracle's solves: rejections at 0.05 of the differential rule on two
EM goldens against second samples, unmerged and on the merged (shared) bin table.  One JSON line per set.

  python tools/census_merge.py

subset    DESIGN 3.28's `subset` sample (tests/diff_util.py: a random two thirds of each locus' rows, counts drawn under B's own
          column scales over the rows left), unmerged; then merged: B's rows keyed by A's row, X_B = A's rows under B's law (the
          full-row weights of `null`'s model), zero counts in B's missing rows.
observed  B drawn under `null`'s model on the FULL table; then each sample keeps only the rows it observed (count > 0, what the
          resident path keeps), unmerged; then merged, a missing row's weights the full table's under the sample's own law."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diff_util as DU  # noqa: E402
import merge_util as MU  # noqa: E402
from conftest import load_golden  # noqa: E402


def rows_of(batch, l):
    n = int(batch.row_off[l + 1] - batch.row_off[l])
    return batch.F[batch.f_off[l]:batch.f_off[l + 1]].reshape(n, -1)


def subset_keys(a, b):
    """B's rows inside A's: each is A's row * 1.3, the rows ascending"""
    key = []
    for l in range(a.n_loci):
        Fa, Fb, at = rows_of(a, l) * 1.3, rows_of(b, l), 0
        for r in range(len(Fb)):
            while not np.array_equal(Fa[at], Fb[r]):
                at += 1
            key.append(at)
            at += 1
    return np.array(key, np.int64).reshape(-1, 1)


def observed(x):
    """-> (the rows with a count as a batch, their rows in the full table as keys)"""
    loci, keys = [], []
    for l in range(x.n_loci):
        k = x.count[int(x.row_off[l]):int(x.row_off[l + 1])] > 0
        loci.append((x.count[int(x.row_off[l]):int(x.row_off[l + 1])][k], rows_of(x, l)[k]))
        keys.append(np.flatnonzero(k))
    return DU.batch_of(loci), np.concatenate(keys + [np.zeros(0, np.int64)]).reshape(-1, 1)


def full_rows(full, keys, row_off):
    """the full table's weights of the rows `keys` names, per locus"""
    return np.concatenate([rows_of(full, l)[keys[int(row_off[l]):int(row_off[l + 1]), 0]].reshape(-1) for l in range(full.n_loci)] + [np.zeros(0)])


def main():
    from oracle import OracleLib, build
    from strawberry_amd import diff, merge
    build(with_ref=False)
    oracle = OracleLib()
    test = lambda x, y: DU.census(diff.em_diff_host(x, y, None, None, oracle.em_batch))  # noqa: E731
    for name in ("em_random_256", "em_c3_400"):
        a = load_golden(name)[0]
        theta = oracle.em_batch(a.row_off, a.iso_off, a.f_off, a.count, a.F)[0]
        null, sub = DU.second_sample(a, "null", 5, theta), DU.second_sample(a, "subset", 5, theta)
        out = {"set": name, "null": test(a, null), "subset unmerged": test(a, sub)}
        key_a = np.concatenate([np.arange(n) for n in np.diff(a.row_off)] + [np.zeros(0, np.int64)]).reshape(-1, 1)
        m = merge.merge_host(MU.Sample(a.iso_off, a.row_off, key_a, a.count, a.F), MU.Sample(sub.iso_off, sub.row_off, subset_keys(a, sub), sub.count, sub.F, a.F * 1.3))
        assert (m.row_a >= 0).all() and (m.row_b < 0).any()
        out["subset merged"] = test(*m.batches())
        (oa, ka), (ob, kb) = observed(a), observed(null)
        out["observed unmerged"] = test(oa, ob)
        m = merge.merge_host(MU.Sample(oa.iso_off, oa.row_off, ka, oa.count, oa.F, full_rows(a, kb, ob.row_off)),
                             MU.Sample(ob.iso_off, ob.row_off, kb, ob.count, ob.F, full_rows(null, ka, oa.row_off)))
        out["observed merged"] = test(*m.batches())
        out["rows"] = {"full": int(a.row_off[-1]), "observed_a": int(oa.row_off[-1]), "observed_b": int(ob.row_off[-1]), "union": int(m.n_bins)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
