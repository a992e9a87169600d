"""Fragment assignment built on the device (sbgpu_fragment_assign_device, csrc/assign_device.h) from what a resident call
leaves in HBM, against the host form (sbgpu_fragment_assign_host on the handle of sbgpu_quantify_host over the same hits, fed
the resident call's theta, keep and status): map_iso, n_cand, map_prob and unassigned bitwise (the rule is shared and runs in
the same order), unique_mass and map_mass bitwise (sums of whole masses: exact in any order), post_mass within
(hits of the locus + 8) * 2^-52 relative (the atomics reorder non-negative terms)."""
import ctypes as C

import numpy as np
import pytest

import stream_util as S
from strawberry_amd import _lib, assign, context
from test_context_table_gpu import MUST_BE_RESIDENT, RL, RUNS, assert_same_table, law_of, toy, wide_sample

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
EXACT = ("map_iso", "n_cand", "map_prob", "unassigned", "unique_mass", "map_mass")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_assignment(dev, host, iso_off, hits_of_locus, what=""):
    assert dev.n_hits == host.n_hits, what
    for k in EXACT:
        np.testing.assert_array_equal(bits(getattr(dev, k)), bits(getattr(host, k)), err_msg="%s %s" % (what, k))
    bound = np.repeat((np.asarray(hits_of_locus, np.float64) + 8.0) * EPS, np.diff(iso_off))
    err = np.abs(dev.post_mass - host.post_mass)
    worst = int(np.argmax(err / np.where(host.post_mass > 0.0, bound * host.post_mass, 1.0)))       # (the largest share of its bound)
    print("%s post_mass: worst isoform %d, |dev - host| = %.3e, bound = %.3e" % (what, worst, err[worst], bound[worst] * host.post_mass[worst]))
    assert (err <= bound * host.post_mass).all(), (what, worst, dev.post_mass[worst], host.post_mass[worst])


def hits_by_locus(hit_locus, n_loci):
    return np.bincount(np.asarray(hit_locus, np.int64), minlength=n_loci)


@pytest.mark.parametrize("which", MUST_BE_RESIDENT)
def test_device_assignment_equals_the_host_form_on_the_toy_directories(ctx, which):
    from strawberry_amd.quantify import quantify_host, quantify_resident
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    law, long_read, min_frac = law_of(which), bool(RUNS[which][1]), RUNS[which][2]
    r = quantify_resident(annot, hits, law, RL, hits.total_mapped, long_read=long_read, ctx=ctx, min_isoform_frac=min_frac, with_assignment=True)
    plain = quantify_resident(annot, hits, law, RL, hits.total_mapped, long_read=long_read, ctx=ctx, min_isoform_frac=min_frac)
    for k in S.OUT_KEYS:        # the call's own results: the bytes of the same call with no assignment
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    a = r["assignment"]
    assert r["bins"].grouped_on_device and a.n_hits == hits.n_hits
    h = quantify_host(annot, hits, law, RL, long_read=long_read, ctx=ctx, assignment_theta=r["theta"], assignment_keep=r["keep"],
                      assignment_status=r["status"])
    assert_same_assignment(a, h["assignment"], annot.iso_off, hits_by_locus(hits.hit_locus, annot.n_loci), which)
    assert (a.map_iso >= 0).sum() > hits.n_hits // 2 and (a.n_cand > 1).any()
    if which == "E2E_FILTER":
        assert (r["keep"] == 0).sum() == 5 and int((a.n_cand == 0).sum()) == 13 == int(a.unassigned.sum())


def test_a_split_locus_two_compat_words_and_erased_isoforms(ctx):
    """wide_sample(): a locus of more than 16384 hits (several work items: the sums are flushed by global atomics), a locus of 40
    isoforms (two compat words; wider than the copies' threshold), five narrow loci (the sums in copies), isoforms erased."""
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    annot, hits = wide_sample()
    assert annot.compat_words == 2 and int((hits.hit_locus == 0).sum()) > 16384      # csrc/assign_device.h: kAsgItemHits
    law = InsertSize(150.0, 60.0)
    r = quantify_resident(annot, hits, law, RL, hits.n_hits, ctx=ctx, min_isoform_frac=0.05, with_assignment=True, with_context=True)
    a = r["assignment"]
    erased = r["keep"][annot.iso_off[1]:annot.iso_off[2]] == 0
    assert erased.any() and not erased.all()
    h = quantify_host(annot, hits, law, RL, ctx=ctx, assignment_theta=r["theta"], assignment_keep=r["keep"], assignment_status=r["status"],
                      context_keep=r["keep"], context_status=r["status"])
    assert_same_assignment(a, h["assignment"], annot.iso_off, hits_by_locus(hits.hit_locus, annot.n_loci), "wide")
    assert_same_table(r["context"], h["context"], "wide")
    in40 = hits.hit_locus == 1
    i0 = int(annot.iso_off[1])
    assert (a.n_cand[in40] > 1).any() and ((a.post_mass[i0 + 32:i0 + 40] > 0.0).any() or erased[32:].all())     # the second compat word's isoforms
    assert not erased[a.map_iso[in40][a.map_iso[in40] >= 0]].any() and (a.post_mass[i0:i0 + 40][erased] == 0.0).all()
    in_wide = hits.hit_locus == 0       # one isoform: the split locus' items all add to it
    # ... and under this law many of its bins are dead (weight <= 1e-5): its assigned hits are those of the live bins, counted here from F
    hb = h["bins"]
    assert hb.row_off[0] == 0 and annot.iso_off[1] == 1 and r["keep"][0] != 0 and r["theta"][0] > 0.0
    live = h["F"][:hb.row_off[1]] > 1e-5
    in_live = int(live[hb.hit_bin[in_wide]].sum())
    assert 0 < in_live < int(in_wide.sum()) and not live.all()
    assert int(a.map_mass[0]) == int(a.unique_mass[0]) == int((a.map_iso[in_wide] == 0).sum()) == in_live
    assert int(a.unassigned[0]) == int(in_wide.sum()) - in_live


@pytest.fixture(scope="module")
def chain_sample(ctx):
    """2 000 loci of the chain workload, isoforms erased (min_isoform_frac 0.01): the device form under the call's theta and under
    another one (one isoform per locus zeroed), table and assignment in turns; then the host form twice."""
    import torch
    from strawberry_amd import chain
    from strawberry_amd.quantify import InsertSize, quantify_host
    q = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01, keep_context=True)
    try:
        q.step()
        theta, keep, status = q.theta[:q.n_iso].copy(), q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        other = theta.copy()
        iso_off = np.asarray(q.annot.iso_off)
        other[iso_off[:-1] + (np.arange(q.n_loci) % np.diff(iso_off))] = 0.0
        t1 = q.context_table()
        a1 = q.fragment_assignment()
        t2 = q.context_table()
        a2 = q.fragment_assignment()
        d_other = torch.from_numpy(other).to(q.dev)
        b = q.fragment_assignment(d_theta=d_other)
        few = q.fragment_assignment(want=("unassigned", "map_mass"))
        hits = q.hits.host_hits(q.n_loci)
        law = InsertSize(250.0, 30.0)
        h = quantify_host(q.annot, hits, law, 75, ctx=ctx, assignment_theta=theta, assignment_keep=keep, assignment_status=status)
        hb = quantify_host(q.annot, hits, law, 75, ctx=ctx, assignment_theta=other, assignment_keep=keep, assignment_status=status)
        np.testing.assert_array_equal(h["theta"], theta)
        with pytest.raises(_lib.SbgpuError, match="stale handle"):      # the host entry was this context's next quantify call
            q.fragment_assignment()
        return dict(iso_off=iso_off, hits_of=hits_by_locus(hits.hit_locus, q.n_loci), keep=keep, other=other, t=(t1, t2), a=(a1, a2), b=b, few=few,
                    host=h["assignment"], host_other=hb["assignment"], n_hits=hits.n_hits, mass=hits.mass)
    finally:
        q.close()


def test_device_assignment_equals_the_host_form_on_the_chain_sample(chain_sample):
    c = chain_sample
    a = c["a"][0]
    assert_same_assignment(a, c["host"], c["iso_off"], c["hits_of"], "chain sample")
    assert a.n_hits == c["n_hits"] and (c["keep"] == 0).sum() > 20 and (a.n_cand > 1).sum() > a.n_hits // 20 and (a.map_iso >= 0).sum() > a.n_hits // 2
    assert (a.post_mass[c["keep"] == 0] == 0.0).all() and (a.unique_mass <= a.map_mass).all()
    # the posterior mass of a locus is its assigned hits' mass
    assigned = np.bincount(np.repeat(np.arange(c["hits_of"].size), c["hits_of"]), weights=np.where(a.map_iso >= 0, c["mass"].astype(np.float64), 0.0),
                           minlength=c["hits_of"].size)
    got = np.add.reduceat(a.post_mass, c["iso_off"][:-1])
    assert (np.abs(got - assigned) <= (c["hits_of"] + np.diff(c["iso_off"]) + 8) * EPS * assigned).all()


def test_a_theta_that_is_not_the_calls(chain_sample):
    c = chain_sample
    assert_same_assignment(c["b"], c["host_other"], c["iso_off"], c["hits_of"], "another theta")
    zeroed = np.zeros(c["iso_off"][-1], bool)
    zeroed[c["other"] == 0.0] = True
    first = np.repeat(c["iso_off"][:-1], c["hits_of"])
    on = c["b"].map_iso >= 0
    assert not zeroed[first[on] + c["b"].map_iso[on]].any()               # theta_j = 0 is never the MAP
    assert (c["b"].map_iso != c["a"][0].map_iso).sum() > 100 and (c["b"].post_mass[zeroed] == 0.0).all()


def test_table_and_assignment_in_either_order(chain_sample):
    c = chain_sample
    assert_same_table(c["t"][0], c["t"][1], "the table around an assignment")
    assert_same_assignment(c["a"][1], c["a"][0], c["iso_off"], c["hits_of"], "the assignment around a table")
    few = c["few"]          # only what was asked for comes to the host
    assert few.map_iso is None and few.post_mass is None and few.map_prob is None
    np.testing.assert_array_equal(few.unassigned, c["a"][0].unassigned)
    np.testing.assert_array_equal(few.map_mass, c["a"][0].map_mass)
    assert set(few.device) == {"map_iso", "map_prob", "n_cand", "unique_mass", "map_mass", "post_mass", "unassigned"}


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, a null theta, per-hit arrays of another length."""
    from strawberry_amd import chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_assign(h, d_theta=True, n_hits=None):
        s = _lib.sbgpu_fragment_assign_t()
        buf = np.zeros(max(n_hits or 1, 1), np.int32)
        if n_hits is not None:
            s.map_iso, s.n_hits = buf.ctypes.data, n_hits
        rc = L.sbgpu_fragment_assign_device(ctx.h, h, q._out.d_theta if d_theta else None, None, None, C.byref(s))
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_assign(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
        context.context_table_keep(ctx, True)
        h1 = call()
        rc, why = try_assign(h1, d_theta=False)
        assert rc == _lib.SBGPU_EINVAL and "d_theta is needed" in why, why
        rc, why = try_assign(h1, n_hits=q.n_hits - 1)
        assert rc == _lib.SBGPU_EINVAL and "n_hits" in why, why
        a1 = assign.fragment_assign_device(ctx, h1, int(q._out.d_theta), q.n_hits, d_hit_mass=q.hits.mass)
        unit = assign.fragment_assign_device(ctx, h1, int(q._out.d_theta), q.n_hits)
        np.testing.assert_array_equal(unit.map_iso, a1.map_iso)
        assert unit.map_mass.sum() == (unit.map_iso >= 0).sum() and a1.map_mass.sum() == q.hits.mass.cpu().numpy().astype(np.float64)[a1.map_iso >= 0].sum()
        h2 = call()
        rc, why = try_assign(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        a2 = assign.fragment_assign_device(ctx, h2, int(q._out.d_theta), q.n_hits, d_hit_mass=q.hits.mass)
        off = np.asarray(q.hits.locus_hit_off)
        assert_same_assignment(a2, a1, np.asarray(q.annot.iso_off), np.diff(off), "the same call twice")
    finally:
        context.context_table_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()


def test_stream_end_keeps_the_assignment_inputs(ctx):
    """sbgpu_front_stream_end with retention on (E2E_FILTER, pushed inflated in one chunk and cluster by cluster): the assignment
    under the masses of sbgpu_front_stream_hits == the resident route's on the whole sample's unique hits."""
    import test_front_stream_gpu as T
    from strawberry_amd.quantify import quantify_resident
    s, g = T.toy("E2E_FILTER")
    hits = g["hits"]
    want = quantify_resident(s.annot, hits, s.insert, RL, hits.total_mapped, long_read=bool(s.long_read), ctx=ctx,
                             min_isoform_frac=s.min_isoform_frac, with_assignment=True)
    L = ctx.L
    schedules = dict(S.schedules(s.n, s.first, s.past, seed=3))
    for name in ("one", "starts"):
        pushes = schedules[name]
        res, out, par, used = s._outputs()
        fs, h = C.c_void_p(), C.c_void_p()
        context.context_table_keep(ctx, True)
        try:
            _lib.check(L.sbgpu_front_stream_begin(ctx.h, C.byref(s.cl), C.byref(s.opts), int(S.chunk_bytes_for(s.off, pushes, s.past)), C.byref(fs)),
                       "sbgpu_front_stream_begin")
            try:
                alive = []
                for a, b in pushes:
                    part = np.ascontiguousarray(s.raw[s.off[a]:s.off[b]])
                    ro = np.ascontiguousarray(s.off[a:b + 1] - s.off[a])
                    alive.append((part, ro))
                    _lib.check(L.sbgpu_front_stream_push(fs, part.ctypes.data if part.size else None, int(part.size), ro.ctypes.data, int(b - a)),
                               "sbgpu_front_stream_push")
                _lib.check(L.sbgpu_front_stream_end(fs, C.byref(s.an), C.byref(s.ins) if s.ins is not None else None, s.read_len, s.long_read,
                                                    C.byref(par), None, C.byref(used), C.byref(out), C.byref(h)), "sbgpu_front_stream_end")
                try:
                    r = s._collect(res, out, used)
                    dh, d_mass = _lib.sbgpu_hits_t(), C.c_void_p()
                    _lib.check(L.sbgpu_front_stream_hits(fs, C.byref(dh), C.byref(d_mass), None), "sbgpu_front_stream_hits")
                    assert int(dh.n_hits) == hits.n_hits
                    got = assign.fragment_assign_device(ctx, h, int(out.d_theta), int(dh.n_hits), d_hit_mass=d_mass.value)
                    table = context.context_table_device(ctx, h)
                    again = assign.fragment_assign_device(ctx, h, int(out.d_theta), int(dh.n_hits), d_hit_mass=d_mass.value)
                finally:
                    L.sbgpu_bins_destroy(h)
            finally:
                L.sbgpu_front_stream_destroy(fs)
        finally:
            context.context_table_keep(ctx, False)
        for k in S.OUT_KEYS:
            np.testing.assert_array_equal(r[k], want[k], err_msg=k)
        hits_of = hits_by_locus(hits.hit_locus, s.annot.n_loci)
        assert_same_assignment(got, want["assignment"], s.annot.iso_off, hits_of, "stream %s" % name)
        assert_same_assignment(again, got, s.annot.iso_off, hits_of, "stream %s, behind the table" % name)
        assert table.n_rows == len(g["rows"]) and int((got.n_cand == 0).sum()) == 13

