"""Abundances per locus on the host (sbgpu_locus_abundance_host): the rule of csrc/bootstrap_rules.h against a plain
Python loop, its refusals, and -- with the other host forms -- the effect the locus columns of the bootstrap exist to show."""
import ctypes as C

import numpy as np
import pytest

WIDTHS = (0, 1, 3, 4, 5, 70)      # 4: the group width of the loads


def loop(iso_off, fpkm, keep, total):
    """the rule, one Python float operation per addition"""
    nl = len(iso_off) - 1
    lf, lt, lk = np.zeros(nl), np.zeros(nl), np.zeros(nl, np.int32)
    for l in range(nl):
        s, n = 0.0, 0
        for j in range(int(iso_off[l]), int(iso_off[l + 1])):
            if keep[j] != 0:
                s = s + float(fpkm[j])
                n += 1
        lf[l], lk[l] = s, n
        with np.errstate(all="ignore"):
            lt[l] = float(np.float64(1e6) * np.float64(s) / np.float64(total)) if n else 0.0
    return lf, lt, lk


def mixed_loci(n_loci, seed):
    """n_loci loci of the widths above in turn; among them (as far as n_loci has room) a locus with every isoform erased, one
    with a single kept isoform, keep == 2 entries, and one NaN FPKM on a kept isoform"""
    rng = np.random.default_rng(seed)
    width = np.array([WIDTHS[(l + 1) % len(WIDTHS)] for l in range(n_loci)], np.int64)      # (locus 0 has an isoform)
    iso_off = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    n_iso = int(iso_off[-1])
    fpkm = rng.gamma(0.7, 40.0, n_iso)
    fpkm[rng.random(n_iso) < 0.1] = 0.0
    keep = rng.choice(np.array([0, 1, 1, 1, 2], np.int32), n_iso)
    wide = [l for l in range(n_loci) if width[l] >= 3]
    if len(wide) > 0:
        keep[iso_off[wide[0]]:iso_off[wide[0] + 1]] = 0                                    # every isoform erased
    if len(wide) > 1:
        keep[iso_off[wide[1]]:iso_off[wide[1] + 1]] = 0
        keep[iso_off[wide[1]] + 1] = 1                                                     # one kept isoform
    if len(wide) > 2:
        j = int(iso_off[wide[2]]) + 2
        fpkm[j], keep[j] = np.nan, 1                                                       # a NaN enters the sum
    return iso_off, fpkm, keep.astype(np.int32)


@pytest.mark.parametrize("n_loci", [1, 6, 13, 257])
def test_the_host_form_is_the_rule(n_loci):
    from strawberry_amd import bootstrap
    iso_off, fpkm, keep = mixed_loci(n_loci, 100 + n_loci)
    if n_loci >= 13:
        assert (keep == 2).any() and np.isnan(fpkm).any()
        assert set(np.diff(iso_off).tolist()) == set(WIDTHS)
    locus_of = np.repeat(np.arange(n_loci), np.diff(iso_off))
    clean = ~np.isin(locus_of, locus_of[np.isnan(fpkm) & (keep != 0)])                   # isoforms of loci whose sum is a number
    kept_sum = float(fpkm[(keep != 0) & clean].sum())
    total = kept_sum * 1.37 + 1.0
    want_f, want_t, want_k = loop(iso_off, fpkm, keep, total)
    got = bootstrap.locus_abundance_host(iso_off, fpkm, keep, total)
    assert got["fpkm"].tobytes() == want_f.tobytes()
    assert got["tpm"].tobytes() == want_t.tobytes()
    np.testing.assert_array_equal(got["kept"], want_k)
    erased = want_k == 0
    assert (got["fpkm"][erased] == 0).all() and (got["tpm"][erased] == 0).all()
    fin = ~np.isnan(got["fpkm"])
    assert abs(got["fpkm"][fin].sum() - kept_sum) <= 1e-12 * kept_sum                     # the same terms in another order
    if n_loci >= 13:
        assert np.isnan(got["fpkm"]).sum() == 1 and erased.sum() >= 2 and (want_k == 1).any()


def test_outputs_are_optional_and_empty_inputs_pass():
    from strawberry_amd import _lib
    L = _lib.load()
    iso_off, fpkm, keep = mixed_loci(13, 5)
    want_f, want_t, want_k = loop(iso_off, fpkm, keep, 1234.5)
    f, t, k = np.zeros(13), np.zeros(13), np.zeros(13, np.int32)
    args = (13, iso_off.ctypes.data, fpkm.ctypes.data, keep.ctypes.data, C.c_double(1234.5))
    assert L.sbgpu_locus_abundance_host(*args, f.ctypes.data, None, None) == 0 and f.tobytes() == want_f.tobytes()
    assert L.sbgpu_locus_abundance_host(*args, None, t.ctypes.data, None) == 0 and t.tobytes() == want_t.tobytes()
    assert L.sbgpu_locus_abundance_host(*args, None, None, k.ctypes.data) == 0 and (k == want_k).all()
    assert L.sbgpu_locus_abundance_host(*args, None, None, None) == 0
    zero = np.zeros(1, np.int64)
    assert L.sbgpu_locus_abundance_host(0, zero.ctypes.data, None, None, C.c_double(1.0), None, None, None) == 0
    # loci without isoforms only: nothing of fpkm / keep is read
    off = np.zeros(4, np.int64)
    assert L.sbgpu_locus_abundance_host(3, off.ctypes.data, None, None, C.c_double(1.0), f.ctypes.data, t.ctypes.data, k.ctypes.data) == 0
    assert (f[:3] == 0).all() and (t[:3] == 0).all() and (k[:3] == 0).all()


def test_refusals():
    from strawberry_amd import _lib, bootstrap
    L = _lib.load()
    fpkm, keep = np.ones(5), np.ones(5, np.int32)
    with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*null iso_off"):
        bootstrap.locus_abundance_host(None, fpkm, keep, 1.0)
    with pytest.raises(_lib.SbgpuError, match=r"\(-1\).*must not decrease \(locus 1\)"):
        bootstrap.locus_abundance_host([0, 3, 2, 5], fpkm, keep, 1.0)
    off = np.array([0, 5], np.int64)
    out = np.zeros(1)
    assert L.sbgpu_locus_abundance_host(1, off.ctypes.data, None, keep.ctypes.data, C.c_double(1.0), out.ctypes.data, None, None) == _lib.SBGPU_EINVAL
    assert b"null fpkm or keep" in L.sbgpu_last_error()
    assert L.sbgpu_locus_abundance_host(-1, off.ctypes.data, fpkm.ctypes.data, keep.ctypes.data, C.c_double(1.0), None, None, None) == _lib.SBGPU_EINVAL
    neg = np.array([-1, 5], np.int64)
    assert L.sbgpu_locus_abundance_host(1, neg.ctypes.data, fpkm.ctypes.data, keep.ctypes.data, C.c_double(1.0), None, None, None) == _lib.SBGPU_EINVAL


def test_the_sum_of_a_locus_varies_less_than_its_isoforms(oracle):
    """The point of the locus columns, with the host forms alone: two isoforms that share a bin holding most of the locus' count.
    Over resampled counts (sbgpu_bootstrap_counts_host) and the oracle's EM, the isoforms trade the shared bin's fragments, so
    their FPKM are negatively correlated and the variance of the locus' FPKM (sbgpu_locus_abundance_host on every replicate,
    sbgpu_replicate_stats_host over them) stays below the sum of the isoforms' variances."""
    from strawberry_amd import bootstrap, em
    row_off, iso_off, f_off = np.array([0, 3], np.int64), np.array([0, 2], np.int64), np.array([0, 6], np.int64)
    count = np.array([900, 60, 40], np.int32)                               # shared; isoform 0 alone; isoform 1 alone
    F = np.array([1e-3, 1e-3, 1e-3, 0.0, 0.0, 1e-3])
    lengths, B = np.array([1000, 2000], np.int32), 64
    fpkm, keep = np.zeros((B, 2)), np.zeros((B, 2), np.int32)
    for k in range(B):
        c = em.bootstrap_counts_host(row_off, count, 77, k)
        assert c.sum() == 1000
        theta, status, _ = oracle.em_batch(row_off, iso_off, f_off, c, F)
        a = oracle.abundance(iso_off, theta, status, lengths, 1000, min_isoform_frac=0.0)
        fpkm[k], keep[k] = a["fpkm"], a["keep"]
    assert (keep != 0).all()
    locus = np.stack([bootstrap.locus_abundance_host(iso_off, fpkm[k], keep[k], fpkm[k].sum())["fpkm"] for k in range(B)])
    iso = bootstrap.replicate_stats_host(fpkm, 1, B - 2)
    loc = bootstrap.replicate_stats_host(locus, 1, B - 2)
    print("var: isoforms %.4g + %.4g, locus %.4g" % (iso["var"][0], iso["var"][1], loc["var"][0]))
    assert iso["var"][0] > 0 and iso["var"][1] > 0
    assert loc["var"][0] < iso["var"][0] + iso["var"][1]
