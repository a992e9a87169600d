"""What tests/test_abundance_bootstrap.py and tests/test_abundance_bootstrap_gpu.py share: the replicate matrices with their
special columns, and the statistics' recurrence restated in numpy."""
import numpy as np


def columns(n_rep, n, seed):
    """[n_rep, n]: random columns, with -- as far as n has room -- an all-equal column, a descending one, heavy ties (three
    levels), and one with two NaNs (they sort last)"""
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, 10.0, (n_rep, n))
    special = [np.full(n_rep, 12.25), np.arange(n_rep, 0, -1, dtype=np.float64) * 0.37,
               rng.choice(np.array([0.0, 3.5, 1e6]), n_rep), rng.normal(0, 1, n_rep)]
    if n_rep >= 3:
        special[3][[0, n_rep // 2]] = np.nan
    for j, col in enumerate(special[:n] if n > 1 else special[2:3]):
        x[:, j] = col
    return x


def welford(x):
    """The header's recurrence in replicate order, in numpy's IEEE doubles"""
    B = len(x)
    m, q = np.zeros_like(x[0]), np.zeros_like(x[0])
    for k in range(B):
        d = x[k] - m
        m = m + d / float(k + 1)
        q = q + d * (x[k] - m)
    return m, (q / float(B - 1) if B > 1 else np.zeros_like(q))
