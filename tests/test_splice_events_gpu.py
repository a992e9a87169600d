"""Splicing events on the device (sbgpu_splice_psi_device, sbgpu_splice_support_device; csrc/splice_device.h) against the host forms,
bit for bit -- psi NaN for NaN, defined_count, support: the same IEEE additions and the one division in the same order, so no
tolerance is chosen.  On tests/splice_util.py's sample as a whole (N_SMALL = 1200: about 7 600 events, 30 workgroups; the launch does
not cap its grid, so there is no case beyond a cap), on annotations of exactly 0, 1, 255, 256, 257 events, on the loci of 63, 64, 65
and 300 isoforms alone (either side of the mask threshold the library exports), for 1, 2 and 65 rows, with and without keep.  Then
behind a resident call on a toy directory: PSI of the call's own FPKM / keep, the call's seven results unchanged, PSI per bootstrap
replicate and its intervals (held to sbgpu_replicate_stats_host as tests/test_abundance_bootstrap_gpu.py holds boot_interval_kernel:
lo / hi bitwise, mean / var at 1e-12), the support from the coverage, the chain and the front quantifiers, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import splice_util as SU
from strawberry_amd import _lib, bootstrap, splice
from strawberry_amd import exonbin as eb
from test_context_table_gpu import RL, RUNS, law_of, toy

pytestmark = pytest.mark.gpu
N_SMALL = 1200
ROWS = (1, 2, 65)
OUT_KEYS = ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.fixture(scope="module")
def sample(ctx):
    annot, loci, at = SU.splice_annotation(N_SMALL)
    ev = splice.SpliceEvents.build(annot)
    return dict(annot=annot, loci=loci, at=at, ev=ev, dev=ev.to_device(ctx))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def device_equals_host(ctx, ev, d_ev, n_rows, with_keep, seed, what, spoil=None):
    """PSI, defined_count and support of both forms on random rows -> the host's psi"""
    import torch
    x, keep = SU.random_rows(n_rows, ev.n_iso, seed, keep=with_keep)
    if spoil is not None:
        spoil(x, keep)
    want, wdef = splice.splice_psi_host(ev, x, keep)
    dev = d_ev.dev
    d_x = torch.from_numpy(x).to(dev)
    d_keep = None if keep is None else torch.from_numpy(keep).to(dev)
    psi, defined = splice.splice_psi_device(ctx, d_ev, d_x, d_keep)
    assert tuple(psi.shape) == (n_rows, ev.n_events) and tuple(defined.shape) == (ev.n_events,)
    SU.same_bits(psi.cpu().numpy(), want, what)
    np.testing.assert_array_equal(defined.cpu().numpy(), wdef, err_msg=what)
    rng = np.random.default_rng(seed + 1)
    xb, jm = rng.gamma(2.0, 50.0, max(ev.n_exons, 1)), rng.gamma(1.0, 3.0, max(ev.n_exons, 1))
    for a, b in ((xb, jm), (xb, None), (None, jm)):
        got = splice.splice_support_device(ctx, d_ev, None if a is None else torch.from_numpy(a).to(dev), None if b is None else torch.from_numpy(b).to(dev))
        assert got.cpu().numpy().tobytes() == splice.splice_support_host(ev, a, b).tobytes(), what
    return want


@pytest.mark.parametrize("with_keep", [True, False])
@pytest.mark.parametrize("n_rows", ROWS)
def test_device_equals_host_on_the_sample(ctx, sample, n_rows, with_keep):
    ev, annot, at = sample["ev"], sample["annot"], sample["at"]
    lim = splice.limits()
    assert ev.n_events > 20 * lim["threads"] and ev.n_events % lim["threads"] != 0
    niso = np.diff(annot.iso_off)
    assert niso[at["W64"]] == lim["mask_iso"] and niso[at["W65"]] == lim["mask_iso"] + 1 and niso[at["W300"]] == 300

    def spoil(x, keep):        # an all-erased locus (with keep), a locus of zeros, a NaN in a narrow and in a wide locus
        i0, i1 = int(annot.iso_off[at["cassette"]]), int(annot.iso_off[at["cassette"] + 1])
        if keep is not None:
            keep[:, i0:i1] = 0
        x[:, int(annot.iso_off[at["retained"]]):int(annot.iso_off[at["retained"] + 1])] = 0.0
        for name in ("W40", "W300"):
            j = int(annot.iso_off[at[name]]) + 3
            x[0, j] = np.nan
            if keep is not None:
                keep[0, j] = 1
    psi = device_equals_host(ctx, ev, sample["dev"], n_rows, with_keep, 300 + n_rows, "sample, %d rows, keep %s" % (n_rows, with_keep), spoil)
    ok = ~np.isnan(psi)
    assert ((psi[ok] >= 0.0) & (psi[ok] <= 1.0)).all() and ok.mean() > 0.5
    for name in ("retained", "W40", "W300") + (("cassette",) if with_keep else ()):
        s = slice(int(ev.event_off[at[name]]), int(ev.event_off[at[name] + 1]))
        assert np.isnan(psi[0, s]).all(), name


def test_annotations_of_0_1_255_256_257_events(ctx):
    """a locus without isoforms, a single-exon locus, 42 loci of six events, then single-exon loci: prefixes end at every count"""
    loci = [[], SU.shifted(SU.HAND["single"], 1000)]
    loci += [SU.shifted(SU.HAND["cassette"], 10000 + 2000 * k) for k in range(42)]
    loci += [SU.shifted(SU.HAND["single"], 200000 + 1000 * k) for k in range(6)]
    annot = eb.Annotation(loci)
    full = splice.SpliceEvents.build(annot)
    off = full.event_off.tolist()
    seen = []
    for n_events in (0, 1, 255, 256, 257, 259):
        n_loci = off.index(n_events)
        ev = splice.SpliceEvents.build(annot.prefix(n_loci))
        assert ev.n_events == n_events
        SU.assert_same_table(ev, SU.by_hand(loci[:n_loci]), "%d events" % n_events)
        d_ev = ev.to_device(ctx)
        for n_rows in ROWS:
            for with_keep in (True, False):
                device_equals_host(ctx, ev, d_ev, n_rows, with_keep, 17 * n_events + n_rows, "%d events, %d rows" % (n_events, n_rows))
        seen.append(n_events)
    assert seen == [0, 1, 255, 256, 257, 259] and 259 % splice.limits()["threads"] != 0


@pytest.mark.parametrize("name", ["W63", "W64", "W65", "W300"])
def test_the_wide_loci_alone(ctx, sample, name):
    loci = [sample["loci"][sample["at"][name]]]
    ev = splice.SpliceEvents.build(eb.Annotation(loci))
    want = SU.by_hand(loci)
    SU.assert_same_table(ev, want, name)
    assert ev.n_iso == int(name[1:]) and ev.alternative().mean() > 0.5
    d_ev = ev.to_device(ctx)
    for n_rows in ROWS:
        for with_keep in (True, False):
            psi = device_equals_host(ctx, ev, d_ev, n_rows, with_keep, 7 * n_rows + ev.n_iso, "%s, %d rows" % (name, n_rows))
    x, keep = SU.random_rows(ROWS[-1], ev.n_iso, 7 * ROWS[-1] + ev.n_iso, keep=False)
    by_hand, _ = SU.psi_by_hand(want, x, keep)
    SU.same_bits(psi, by_hand, name + " against the restatement")


# ---- behind a resident call

@pytest.fixture(scope="module", params=["E2E", "E2E_FILTER"])
def resident(ctx, request):
    from strawberry_amd.quantify import quantify_resident
    which = request.param
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    kw = dict(long_read=bool(RUNS[which][1]), ctx=ctx, min_isoform_frac=RUNS[which][2])
    law = law_of(which)
    ev = splice.SpliceEvents.build(annot)
    plain = quantify_resident(annot, hits, law, RL, hits.total_mapped, **kw)
    first = quantify_resident(annot, hits, law, RL, hits.total_mapped, with_splicing=True, **kw)
    full = quantify_resident(annot, hits, law, RL, hits.total_mapped, with_splicing=ev, bootstrap=dict(n_rep=8, seed=5, locus=False), with_coverage=True, **kw)
    return dict(which=which, annot=annot, ev=ev, plain=plain, first=first, full=full)


def test_resident_psi_is_the_host_form_on_the_calls_fpkm_and_keep(resident):
    r, ev = resident["first"], resident["ev"]
    s = r["splicing"]
    assert isinstance(s, splice.SplicePsi) and s.mean is None and s.support is None and s.psi.shape == (ev.n_events,)
    SU.assert_same_table(s.events, {k: getattr(ev, k) for k in SU.TABLE_ARRAYS + ("n_exons",)}, "the table built inside the call")
    want, _ = splice.splice_psi_host(ev, r["fpkm"], r["keep"])
    SU.same_bits(s.psi, want[0], resident["which"])
    assert (~np.isnan(s.psi)).sum() > 0 and "splicing" not in resident["plain"]
    for k in OUT_KEYS:          # the call's own seven results: the bytes of the same call with no PSI behind it
        np.testing.assert_array_equal(bits(r[k]), bits(resident["plain"][k]), err_msg=k)
        np.testing.assert_array_equal(bits(resident["full"][k]), bits(resident["plain"][k]), err_msg=k)


def test_resident_psi_per_replicate_and_its_intervals(resident):
    r, ev = resident["full"], resident["ev"]
    s, b = r["splicing"], r["bootstrap"]
    want, _ = splice.splice_psi_host(ev, r["fpkm"], r["keep"])
    SU.same_bits(s.psi, want[0], "behind a bootstrap and a coverage")
    assert s.rep.shape == (8, ev.n_events) and s.n_rep == 8 and (s.rank_lo, s.rank_hi) == (b["rank_lo"], b["rank_hi"])
    rep, defined = splice.splice_psi_host(ev, b["fpkm_rep"], b["keep_rep"])
    SU.same_bits(s.rep, rep, "row k of the PSI matrix")
    np.testing.assert_array_equal(s.defined_count, defined)
    assert len({row.tobytes() for row in s.rep}) > 1            # (the replicates differ)
    stats = bootstrap.replicate_stats_host(s.rep, s.rank_lo, s.rank_hi)
    assert s.lo.tobytes() == stats["lo"].tobytes() and s.hi.tobytes() == stats["hi"].tobytes()
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(s.mean, stats["mean"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(s.var, stats["var"], rtol=1e-12, atol=0)
    ok = defined == 8
    assert ok.any() and (s.lo[ok] <= s.hi[ok]).all() and (s.lo[ok] >= 0.0).all() and (s.hi[ok] <= 1.0).all()
    assert len(list(s.rows())[0]) == len(s.header()) == 14


def test_resident_support_is_the_host_form_on_the_coverage(resident):
    r, ev = resident["full"], resident["ev"]
    cov = r["coverage"]
    want = splice.splice_support_host(ev, cov.exon_bases, cov.junction_mass)
    assert r["splicing"].support.tobytes() == want.tobytes() and (want > 0.0).any()
    assert (want[ev.event_kind == 1] > 0.0).any() and (want[ev.event_kind == 0] > 0.0).any()


def test_chain_and_front_quantifiers(ctx):
    from strawberry_amd import chain, front
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01, keep_context=True, keep_bootstrap=True)
    try:
        with pytest.raises(_lib.SbgpuError, match="no resident step has run"):
            q.splice_psi()
        q.step()
        ev = splice.SpliceEvents.build(q.annot)
        want, _ = splice.splice_psi_host(ev, q.fpkm[:q.n_iso], q.keep[:q.n_iso])
        s = q.splice_psi()
        SU.same_bits(s.psi, want[0], "ChainQuantifier.splice_psi()")
        SU.same_bits(q.splice_psi(events=ev).psi, want[0], "... on a table built outside")
        b, cov = q.abundance_bootstrap(8, 11), q.isoform_coverage()
        s = q.splice_psi(bootstrap=b, coverage=cov)
        SU.same_bits(s.psi, want[0], "... with a bootstrap and a coverage")
        _, defined = splice.splice_psi_host(ev, b["fpkm_rep"], b["keep_rep"])
        np.testing.assert_array_equal(s.defined_count, defined)
        assert s.support.tobytes() == splice.splice_support_host(ev, cov.exon_bases, cov.junction_mass).tobytes()
        with pytest.raises(_lib.SbgpuError, match="replicates are not on the device"):
            q.splice_psi(bootstrap={"n_rep": 8})
        with pytest.raises(ValueError, match="SpliceEvents"):
            q.splice_psi(events=7)
    finally:
        q.close()
    f = front.FrontQuantifier(ctx, n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    try:
        f.step()
        ev = splice.SpliceEvents.build(f.annot)
        want, _ = splice.splice_psi_host(ev, f.fpkm[:f.n_iso], f.keep[:f.n_iso])
        s = f.splice_psi()
        SU.same_bits(s.psi, want[0], "FrontQuantifier.splice_psi()")
        assert (~np.isnan(s.psi)).sum() > f.n_loci and s.alternative().any()
    finally:
        f.close()


def test_refusals(ctx, sample):
    import torch
    L, d_ev, ev = ctx.L, sample["dev"], sample["ev"]
    dev = d_ev.dev
    x = torch.ones(ev.n_iso, dtype=torch.float64, device=dev)
    psi = torch.zeros(ev.n_events, dtype=torch.float64, device=dev)

    def refuse(rc, code, text):
        why = L.sbgpu_last_error().decode()
        assert rc == code and text in why, (rc, why)
    s = d_ev.struct
    refuse(L.sbgpu_splice_psi_device(None, C.byref(s), 1, x.data_ptr(), None, psi.data_ptr(), None, None), _lib.SBGPU_EINVAL, "null argument")
    refuse(L.sbgpu_splice_psi_device(ctx.h, None, 1, x.data_ptr(), None, psi.data_ptr(), None, None), _lib.SBGPU_EINVAL, "null argument")
    refuse(L.sbgpu_splice_psi_device(ctx.h, C.byref(s), 1, None, None, psi.data_ptr(), None, None), _lib.SBGPU_EINVAL, "d_x is needed")
    refuse(L.sbgpu_splice_psi_device(ctx.h, C.byref(s), 1, x.data_ptr(), None, None, None, None), _lib.SBGPU_EINVAL, "d_psi is needed")
    refuse(L.sbgpu_splice_psi_device(ctx.h, C.byref(s), -1, x.data_ptr(), None, psi.data_ptr(), None, None), _lib.SBGPU_EINVAL, "negative row count")
    refuse(L.sbgpu_splice_psi_device(ctx.h, C.byref(s), 2 ** 31, x.data_ptr(), None, psi.data_ptr(), None, None), _lib.SBGPU_ESHAPE, "2^31 - 1 rows")
    refuse(L.sbgpu_splice_support_device(ctx.h, C.byref(s), None, None, None, None), _lib.SBGPU_EINVAL, "d_support is needed")
    bad = _lib.sbgpu_splice_events_t()
    C.memmove(C.byref(bad), C.byref(s), C.sizeof(bad))
    bad.incl_iso = None
    refuse(L.sbgpu_splice_psi_device(ctx.h, C.byref(bad), 1, x.data_ptr(), None, psi.data_ptr(), None, None), _lib.SBGPU_EINVAL, "inclusion lists are needed")
    C.memmove(C.byref(bad), C.byref(s), C.sizeof(bad))
    bad.n_events = 2 ** 31
    refuse(L.sbgpu_splice_support_device(ctx.h, C.byref(bad), None, None, psi.data_ptr(), None), _lib.SBGPU_ESHAPE, "2^31 - 1 events")
    with pytest.raises(ValueError, match="torch.float64"):
        splice.splice_psi_device(ctx, d_ev, x.float())
    with pytest.raises(ValueError, match="n_rows, n_iso"):
        splice.splice_psi_device(ctx, d_ev, x[:-1].contiguous())
    with pytest.raises(ValueError, match="n_rows is needed"):
        splice.splice_psi_device(ctx, d_ev, x.data_ptr())
    # the refused calls wrote nothing
    torch.cuda.synchronize(dev)
    assert (psi == 0.0).all()
