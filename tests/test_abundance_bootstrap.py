"""The replicates' statistics on the host (sbgpu_replicate_stats_host: the plain statement of what boot_interval_kernel
computes, csrc/bootstrap_rules.h) against numpy, the interval's integer ranks, and the host form's refusals.  No GPU."""
import numpy as np
import pytest

from boot_util import columns, welford

N_REPS = (1, 2, 3, 64, 65, 100, 1500)
NS = (1, 7, 300)


def check_against_numpy(got, x, lo, hi):
    """lo / hi: np.sort's elements (NaNs last), BITWISE; mean / var: 1e-12 relative -- the same IEEE operations
    (-ffp-contract=off), the bar tests/test_bootstrap_gpu.py::test_statistics uses and explains"""
    s = np.sort(x, axis=0)
    assert got["lo"].tobytes() == s[lo].tobytes()
    assert got["hi"].tobytes() == s[hi].tobytes()
    m, v = welford(x)
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(got["mean"], m, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["var"], v, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n_rep", N_REPS)
def test_host_statistics_against_numpy(n_rep):
    from strawberry_amd import bootstrap
    for n in NS:
        x = columns(n_rep, n, 1000 * n_rep + n)
        lo, hi = bootstrap.interval_ranks(n_rep, 0.9)
        for a, b in {(lo, hi), (0, n_rep - 1), (n_rep // 2, n_rep // 2)}:      # (the last: rank_lo == rank_hi)
            got = bootstrap.replicate_stats_host(x, a, b)
            check_against_numpy(got, x, a, b)
            if a == b:
                assert got["lo"].tobytes() == got["hi"].tobytes()


def test_special_columns_behave():
    from strawberry_amd import bootstrap
    x = columns(100, 7, 5)
    r = bootstrap.replicate_stats_host(x, 2, 97)
    assert r["lo"][0] == r["hi"][0] == r["mean"][0] == 12.25 and r["var"][0] == 0.0           # all equal
    assert r["lo"][1] == 3 * 0.37 and r["hi"][1] == 98 * 0.37                                  # descending
    assert r["lo"][2] in (0.0, 3.5, 1e6) and r["hi"][2] in (0.0, 3.5, 1e6)                     # ties
    assert np.isnan(r["mean"][3]) and not np.isnan(r["hi"][3])                                 # two NaNs: positions 98 and 99
    top = bootstrap.replicate_stats_host(x, 97, 98)
    assert not np.isnan(top["lo"][3]) and np.isnan(top["hi"][3])
    one = bootstrap.replicate_stats_host(x[:1], 0, 0)
    assert (one["var"] == 0).all() and one["lo"].tobytes() == one["hi"].tobytes() == one["mean"].tobytes() == x[0].tobytes()


def test_interval_ranks():
    from strawberry_amd.bootstrap import interval_ranks
    assert interval_ranks(100, 0.95) == (2, 97)
    assert interval_ranks(100, 0.9) == (5, 94)       # (0.1 / 2 * 100 in binary floating point falls short of 5)
    assert interval_ranks(40, 0.95) == (1, 38)
    for level in (0.5, 0.9, 0.95, 0.999, 1):
        assert interval_ranks(1, level) == (0, 0)
    assert interval_ranks(1000, 0.999) == (0, 999) and interval_ranks(1000, 0.99) == (5, 994)
    with pytest.raises(ValueError):
        interval_ranks(0, 0.9)
    with pytest.raises(ValueError):
        interval_ranks(10, 0)


def test_the_host_form_refuses():
    from strawberry_amd import _lib, bootstrap
    x = np.zeros((4, 3))
    for lo, hi in ((-1, 2), (3, 2), (0, 4)):
        with pytest.raises(_lib.SbgpuError, match="ranks"):
            bootstrap.replicate_stats_host(x, lo, hi)
    L = _lib.load()
    assert L.sbgpu_replicate_stats_host(0, 3, x.ctypes.data, 0, 0, None, None, None, None) == -1      # SBGPU_EINVAL
    assert L.sbgpu_replicate_stats_host(4, 3, None, 0, 0, None, None, None, None) == -1
    assert b"null matrix" in L.sbgpu_last_error()
    assert L.sbgpu_replicate_stats_host(4, 0, None, 0, 3, None, None, None, None) == 0                 # no columns: nothing to do
