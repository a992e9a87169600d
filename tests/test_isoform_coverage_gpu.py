"""Isoform-resolved coverage built on the device (sbgpu_isoform_coverage_device, csrc/coverage_device.h) from what a resident call
leaves in HBM and the hits it was given, against the host form (sbgpu_isoform_coverage_host under the resident call's theta, keep
and status) within (hits of the locus + 8) * 2^-52 -- iso_bases: + the isoform's exons -- and against
tests/coverage_util.py::by_hand within (2 hits + niso + 16) * 2^-52; zeros exactly.  On the toy directories, on
tests/retained_util.py::edge_sample() as a whole and locus by locus (a locus on either side of every threshold of the kernel), in
the all-integer case bit for bit, under another theta, in every order with the table and the assignment, through the chain and
the front quantifiers, and the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import coverage_util as CU
import retained_util as R
import stream_util as S
from strawberry_amd import _lib, context, coverage
from strawberry_amd import exonbin as eb
from test_context_table import Handle
from test_context_table_gpu import MUST_BE_RESIDENT, RL, RUNS, assert_same_table, law_of, toy
from test_fragment_assign_gpu import assert_same_assignment, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def device_hits(hits, dev):
    """-> (the _lib.sbgpu_hits_t of device copies of the hits' arrays, the tensors that own them)"""
    import torch
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)  # noqa: E731
    d = {"hit_locus": up(hits.hit_locus, np.int32), "feat_off": up(hits.feat_off, np.int64), "feat_code": up(hits.feat_code, np.uint8),
         "feat_left": up(hits.feat_left, np.int32), "feat_right": up(hits.feat_right, np.int32)}
    hs = _lib.sbgpu_hits_t()
    hs.n_hits = hits.n_hits
    for k, v in d.items():
        setattr(hs, k, v.data_ptr())
    return hs, d


def host_forms(oracle, annot, hits, h, keep, status, *thetas, unit_masses=False):
    """sbgpu_isoform_coverage_host under each theta, on a host handle over the hits of h = quantify_host(annot, hits, ...):
    sbgpu_bins_create on the oracle's words numbers the bins as sbgpu_quantify_host did (asserted), so h["F"] are its weights."""
    compat, key = oracle.exonbin_batch(annot, hits)
    np.testing.assert_array_equal(compat, h["compat"])
    own = eb.LocusBins(annot, hits, compat, key)
    np.testing.assert_array_equal(own.hit_bin, h["bins"].hit_bin)
    np.testing.assert_array_equal(own.f_off, h["bins"].f_off)
    with Handle(annot, hits, compat, key) as H:
        return [coverage.isoform_coverage_host(H.h, annot, hits, compat, t, F=h["F"], keep=keep, status=status,
                                               hit_mass=None if unit_masses else hits.mass) for t in thetas]


@pytest.mark.parametrize("which", MUST_BE_RESIDENT)
def test_device_coverage_on_the_toy_directories(ctx, oracle, which):
    from strawberry_amd.quantify import quantify_host, quantify_resident
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    law, long_read, min_frac = law_of(which), bool(RUNS[which][1]), RUNS[which][2]
    kw = dict(long_read=long_read, ctx=ctx, min_isoform_frac=min_frac)
    r = quantify_resident(annot, hits, law, RL, hits.total_mapped, with_coverage=True, **kw)
    plain = quantify_resident(annot, hits, law, RL, hits.total_mapped, **kw)
    for k in S.OUT_KEYS:        # the call's own seven results: the bytes of the same call with no coverage behind it
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    c = r["coverage"]
    assert r["bins"].grouped_on_device
    h = quantify_host(annot, hits, law, RL, long_read=long_read, ctx=ctx)
    host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], r["theta"])
    CU.compare(c, host, annot, hits.hit_locus, False, which + ", device against host")
    want = CU.by_hand(h["bins"], annot, hits, h["compat"], h["F"], r["theta"], r["keep"], r["status"], hits.mass)
    CU.compare(c, want, annot, hits.hit_locus, True, which + ", device against the restatement")
    CU.conservation(c, want, annot, hits.hit_locus, which)
    np.testing.assert_array_equal(c.iso_bases, CU.iso_bases_of(c.exon_bases, annot))
    assert (c.iso_bases > 0.0).any() and (c.junction_mass > 0.0).any() and (c.iso_bases[r["keep"] == 0] == 0.0).all()
    assert set(c.device) == set(CU.NAMES)


@pytest.fixture(scope="module")
def E(ctx, oracle):
    """One resident call on the edge sample with the coverage behind it; on its handle the all-integer case (one-hot theta, unit
    masses); the host forms of both on a host handle over the same hits; the restatement."""
    import torch
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small, grid = R.n_small_for(cu), R.GRID_PER_CU * cu
    annot, hits = R.edge_sample(n_small, grid=grid)
    law = InsertSize(*R.LAW)
    dev = torch.device("cuda", ctx.device)
    hot = np.zeros(int(annot.iso_off[-1]))
    hot[np.asarray(annot.iso_off[:-1], np.int64)] = 1.0
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, keep_handle=True, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_coverage=True)
    with r["handle"] as handle:
        d_hits, own = device_hits(hits, dev)
        d_hot, d_theta, d_mass = torch.from_numpy(hot).to(dev), torch.from_numpy(r["theta"].copy()).to(dev), torch.from_numpy(hits.mass.copy()).to(dev)
        exact = coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_hot)
        again = coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)
        del own
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], r["theta"])
    exact_host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], hot, unit_masses=True)
    want = CU.by_hand(h["bins"], annot, hits, h["compat"], h["F"], r["theta"], r["keep"], r["status"], hits.mass)
    at = R.edge_layout(n_small)
    fig = CU.sample_conditions(annot, hits, want, nobin_locus=at["NOBIN"])
    print(fig)
    hits_of = np.bincount(hits.hit_locus, minlength=annot.n_loci)
    return dict(annot=annot, hits=hits, r=r, c=r["coverage"], again=again, exact=exact, exact_host=exact_host, h=h, host=host, want=want, at=at, cu=cu, grid=grid,
                hits_of=hits_of, nl=annot.n_loci)


def test_the_sample_lies_on_either_side_of_every_threshold(E):
    """... by the constants the library exports, and its work items exceed two passes of the grid"""
    lim = coverage.limits()
    annot, at = E["annot"], E["at"]
    niso = np.diff(annot.iso_off)
    nex = np.diff(np.asarray(annot.exon_off)[np.asarray(annot.iso_off)])
    assert lim["item_hits"] == R.ITEM_HITS and lim["copy_exons"] * lim["copies"] <= lim["lds_exons"]
    assert R.n_items(E["hits_of"]) > 2 * E["grid"] and E["nl"] > 2 * E["grid"]
    # C: on the far side of the exons-in-LDS threshold (its sums and its exon table in global memory); everybody else within
    # (lds_iso is no threshold of its own: an isoform owns an exon, so it is the same number)
    assert lim["lds_exons"] < nex[at["C"]] <= 3600 and niso[at["C"]] == 300 and lim["lds_iso"] == lim["lds_exons"]
    assert all(nex[at[k]] <= lim["lds_exons"] for k in R.SPECIAL if k != "C")
    assert 200 <= nex[at["T1024"]] <= 300 and 200 <= nex[at["T1025"]] <= 300
    # copies: A, T8 and the small loci keep them; T9 (isoforms) and T1024 / T1025 (exons) do not
    copies = (niso <= lim["narrow_iso"]) & (nex <= lim["copy_exons"])
    assert copies[at["A"]] and copies[at["T8"]] and niso[at["T8"]] == lim["narrow_iso"]
    assert not copies[at["T9"]] and niso[at["T9"]] == lim["narrow_iso"] + 1 and nex[at["T9"]] <= lim["copy_exons"]
    assert not copies[at["T1024"]] and niso[at["T1024"]] <= lim["narrow_iso"]
    assert not copies[at["T32"]] and not copies[at["T33"]] and not copies[at["B"]]
    # split loci on either side of the copies: A (three items, the last partial) and B (two)
    assert 2 * lim["item_hits"] < E["hits_of"][at["A"]] < 3 * lim["item_hits"] < 3 * E["hits_of"][at["B"]] < 6 * lim["item_hits"]


def test_device_equals_the_host_form_and_the_restatement(E):
    annot, hits = E["annot"], E["hits"]
    CU.compare(E["c"], E["host"], annot, hits.hit_locus, False, "edge sample, device against host")
    CU.compare(E["c"], E["want"], annot, hits.hit_locus, True, "edge sample, device against the restatement")
    CU.compare(E["host"], E["want"], annot, hits.hit_locus, True, "edge sample, host against the restatement")
    CU.compare(E["again"], E["c"], annot, hits.hit_locus, False, "edge sample, the same call again")
    CU.conservation(E["c"], E["want"], annot, hits.hit_locus, "edge sample")


@pytest.mark.parametrize("name", R.SPECIAL)
def test_each_shape_on_its_own(E, name):
    annot, hits, c = E["annot"], E["hits"], E["c"]
    l = E["at"][name]
    only = np.zeros(E["nl"], bool)
    only[l] = True
    i0, i1 = int(annot.iso_off[l]), int(annot.iso_off[l + 1])
    e0, e1 = int(annot.exon_off[i0]), int(annot.exon_off[i1])
    what = "locus %s (%d isoforms, %d exons, %d hits)" % (name, i1 - i0, e1 - e0, E["hits_of"][l])
    CU.compare(c, E["host"], annot, hits.hit_locus, False, what + ", device against host", loci=only)
    CU.compare(c, E["want"], annot, hits.hit_locus, True, what + ", device against the restatement", loci=only)
    erased = E["r"]["keep"][i0:i1] == 0
    assert (c.iso_bases[i0:i1][erased] == 0.0).all(), what
    if name in ("EMPTY", "NOBIN"):
        assert (c.exon_bases[e0:e1] == 0.0).all() and (c.junction_mass[e0:e1] == 0.0).all() and (c.iso_bases[i0:i1] == 0.0).all()
        assert (c.unexplained_bases[l] > 0.0) == (name == "NOBIN")
        return
    assert (c.exon_bases[e0:e1] > 0.0).sum() > 1 and (c.junction_mass[e0:e1] > 0.0).any(), what    # the sums went to several addresses
    if name == "B":
        assert erased.any() and not erased.all()
    if name == "C":         # beyond the first compat word, beyond the first stride of the staging loops
        assert (c.iso_bases[i0 + 256:i1] > 0.0).any() or erased[256:].all()


def test_the_later_passes_of_the_persistent_loop(E):
    """A workgroup's second, third, ... work item (item i is taken in pass i // grid), each pass compared as a group of its own"""
    annot, hits, grid, nl = E["annot"], E["hits"], E["grid"], E["nl"]
    item_locus = np.repeat(np.arange(nl), -(-E["hits_of"] // R.ITEM_HITS))
    item_pass = np.arange(item_locus.size) // grid
    assert item_pass.max() >= 2
    for p in range(1, int(item_pass.max()) + 1):
        group = np.zeros(nl, bool)
        group[item_locus[item_pass == p]] = True
        what = "pass %d of the grid over the work items" % (p + 1)
        CU.compare(E["c"], E["host"], annot, hits.hit_locus, False, what, loci=group)
        CU.compare(E["c"], E["want"], annot, hits.hit_locus, True, what + ", the restatement", loci=group)


def test_the_all_integer_case_is_bitwise_and_iso_bases_is_the_sum_of_the_devices_own_exons(E):
    """one-hot theta, unit masses: every term is an integer, so device and host agree bit for bit in any order"""
    CU.bitwise(E["exact"], E["exact_host"], "one-hot theta, unit masses")
    x = E["exact"]
    assert (x.exon_bases == np.round(x.exon_bases)).all() and (x.junction_mass == np.round(x.junction_mass)).all() and x.exon_bases.sum() > 0
    for what, c in (("the call's theta", E["c"]), ("again", E["again"]), ("one-hot", E["exact"])):
        np.testing.assert_array_equal(c.iso_bases.view(np.uint64), CU.iso_bases_of(c.exon_bases, E["annot"]).view(np.uint64), err_msg=what)


@pytest.fixture(scope="module")
def chain_sample(ctx, oracle):
    """2 000 loci of the chain workload with both retentions on: coverage, assignment and table in all six orders, twice each;
    the coverage under a bootstrap mean of theta; then the host forms."""
    import torch
    from strawberry_amd import chain
    from strawberry_amd.quantify import InsertSize, quantify_host
    q = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01, keep_context=True, keep_bootstrap=True)
    try:
        q.step()
        theta, keep, status = q.theta[:q.n_iso].copy(), q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        outputs = {k: getattr(q, k)[:(q.n_loci if k in ("status", "iters") else q.n_iso)].copy() for k in S.OUT_KEYS}
        calls = {"coverage": q.isoform_coverage, "assignment": q.fragment_assignment, "table": q.context_table}
        turns = []
        for order in itertools.permutations(sorted(calls)):
            for _ in range(2):
                turns.append((order, {k: calls[k]() for k in order}))
        boot = q.abundance_bootstrap(8, 11, replicates=False)
        mean = np.ascontiguousarray(boot["theta_mean"])
        behind = q.isoform_coverage(d_theta=torch.from_numpy(mean).to(q.dev))
        few = q.isoform_coverage(want=("unexplained_bases",))
        hits = q.hits.host_hits(q.n_loci)
        law = InsertSize(250.0, 30.0)
        h = quantify_host(q.annot, hits, law, 75, ctx=ctx)
        np.testing.assert_array_equal(h["theta"], theta)
        host, host_mean = host_forms(oracle, q.annot, hits, h, keep, status, theta, mean)
        with pytest.raises(_lib.SbgpuError, match="stale handle"):      # the host entry was this context's next quantify call
            q.isoform_coverage()
        plain = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01)
        try:
            plain.step()
            for k in S.OUT_KEYS:        # the call's own seven results with and without retention and what is built from it
                np.testing.assert_array_equal(bits(getattr(plain, k)[:outputs[k].size]), bits(outputs[k]), err_msg=k)
        finally:
            plain.close()
        return dict(annot=q.annot, hits=hits, theta=theta, mean=mean, keep=keep, turns=turns, behind=behind, few=few, host=host,
                    host_mean=host_mean, hits_of=np.bincount(hits.hit_locus, minlength=q.n_loci))
    finally:
        q.close()


def test_coverage_assignment_and_table_in_all_six_orders_twice(chain_sample):
    c = chain_sample
    annot, hits = c["annot"], c["hits"]
    assert len(c["turns"]) == 12 and len({o for o, _ in c["turns"]}) == 6
    first = c["turns"][0][1]
    CU.compare(first["coverage"], c["host"], annot, hits.hit_locus, False, "chain sample, device against host")
    for order, got in c["turns"][1:]:
        what = " -> ".join(order)
        CU.compare(got["coverage"], first["coverage"], annot, hits.hit_locus, False, what)
        CU.compare(got["coverage"], c["host"], annot, hits.hit_locus, False, what + ", against host")
        assert_same_assignment(got["assignment"], first["assignment"], np.asarray(annot.iso_off), c["hits_of"], what)
        assert_same_table(got["table"], first["table"], what)
    few = c["few"]          # only what was asked for comes to the host
    assert few.exon_bases is None and few.iso_bases is None and set(few.device) == set(CU.NAMES)
    np.testing.assert_array_equal(few.unexplained_bases, first["coverage"].unexplained_bases)
    cov = first["coverage"]
    assert (cov.iso_bases[c["keep"] == 0] == 0.0).all() and (c["keep"] == 0).sum() > 20 and (cov.junction_mass > 0.0).sum() > 1000


def test_a_theta_that_is_not_the_calls(chain_sample):
    """the bootstrap's mean of theta, from the same handle: the coverage under it is the host form's under it"""
    c = chain_sample
    assert (c["mean"] != c["theta"]).sum() > c["theta"].size // 2
    CU.compare(c["behind"], c["host_mean"], c["annot"], c["hits"].hit_locus, False, "a bootstrap mean")
    assert (c["behind"].exon_bases != c["turns"][0][1]["coverage"].exon_bases).sum() > 100


def front_hits(q):
    """the unique hits the last pass of a FrontQuantifier(keep_context=True) kept on the device, as host arrays (eb.Hits)"""
    dh, d_mass = q._coverage_hits()
    n = int(dh.n_hits)
    off = S._d2h(dh.feat_off, n + 1, np.int64)
    nf = int(off[-1])
    return eb.Hits.from_arrays(S._d2h(dh.hit_locus, n, np.int32), off, S._d2h(dh.feat_code, nf, np.uint8), S._d2h(dh.feat_left, nf, np.uint32),
                               S._d2h(dh.feat_right, nf, np.uint32), S._d2h(d_mass, n, np.float32))


def test_front_quantifier_isoform_coverage(ctx, oracle):
    """FrontQuantifier.isoform_coverage(): after step() on the unique hits of sbgpu_uniq_dev_hits, after stream_step() on
    sbgpu_front_stream_hits' -- the same records, the same hits, the same coverage; and the host form's on those hits."""
    from strawberry_amd import front
    from strawberry_amd.quantify import quantify_host
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
            plain.isoform_coverage()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_context=True, **kw)
    try:
        q.step()
        hits_of = np.diff(q.front_hit_off)
        hit_locus = np.repeat(np.arange(q.n_loci), hits_of)
        theta = q.theta[:q.n_iso].copy()
        keep, status = q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        c1 = q.isoform_coverage()
        a = q.fragment_assignment()
        c2 = q.isoform_coverage()
        CU.compare(c2, c1, q.annot, hit_locus, False, "behind the assignment")
        hits1 = front_hits(q)
        np.testing.assert_array_equal(hits1.hit_locus, hit_locus)
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        info = q.stream_step()
        assert info["chunks"] > 3 and info["unique_hits"] == a.n_hits
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        c3 = q.isoform_coverage()
        CU.compare(c3, c1, q.annot, hit_locus, False, "through the stream")
        hits3 = front_hits(q)
        for k in ("hit_locus", "feat_off", "feat_code", "feat_left", "feat_right", "mass"):     # the same hits in the same order
            np.testing.assert_array_equal(getattr(hits3, k), getattr(hits1, k), err_msg=k)
        np.testing.assert_array_equal(c3.iso_bases, CU.iso_bases_of(c3.exon_bases, q.annot))
        keep = q.keep[:q.n_iso]
        assert (c3.iso_bases[keep == 0] == 0.0).all() and (c3.iso_bases > 0.0).sum() > q.n_loci and (c3.junction_mass > 0.0).sum() > q.n_loci
        # the unassigned hits are the unexplained ones
        assert ((c3.unexplained_bases > 0.0) == (a.unassigned > 0)).all()
    finally:
        q.close()
    # the host form on those hits, under the pass' theta, keep and status (the pass built its insert-size law from the hits)
    h = quantify_host(q.annot, hits1, None, q.read_len, ctx=ctx)
    np.testing.assert_array_equal(h["theta"].view(np.uint64), theta.view(np.uint64))
    host, = host_forms(oracle, q.annot, hits1, h, keep, status, theta)
    CU.compare(c1, host, q.annot, hit_locus, False, "the front's hits, device against host")
    CU.compare(c3, host, q.annot, hit_locus, False, "the stream's hits, device against host")
    with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
        q.isoform_coverage()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, a null theta, hits of another count, another annotation."""
    from strawberry_amd import chain
    L = ctx.L
    q = chain.ChainQuantifier(ctx, n_loci=300, n_frags=300 * 200, seed=12, resident=True, min_isoform_frac=0.01)
    handles = []
    an = q.annot._struct()

    def call():
        h = C.c_void_p()
        q._resident_call(L, q._ht, q.hits.mass.data_ptr(), q.hits.locus_hit_off.ctypes.data, q.n_frags, h)
        handles.append(h)
        return h

    def try_cover(h, d_theta=True, n_hits=None, annot=None):
        s = _lib.sbgpu_isoform_coverage_t()
        ht = q.hits.struct()
        if n_hits is not None:
            ht.n_hits = n_hits
        rc = L.sbgpu_isoform_coverage_device(ctx.h, h, C.byref(annot or an), C.byref(ht), q._out.d_theta if d_theta else None, None, None, C.byref(s))
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = try_cover(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
        context.context_table_keep(ctx, True)
        h1 = call()
        rc, why = try_cover(h1, d_theta=False)
        assert rc == _lib.SBGPU_EINVAL and "d_theta is needed" in why, why
        rc, why = try_cover(h1, n_hits=q.n_hits - 1)
        assert rc == _lib.SBGPU_EINVAL and "d_hits->n_hits is not the retained call's" in why, why
        other = eb.Annotation([[[(1, 100), (201, 300)]]])
        rc, why = try_cover(h1, annot=other._struct())
        assert rc == _lib.SBGPU_EINVAL and "the annotation's loci or isoforms are not the handle's" in why, why
        c1 = coverage.isoform_coverage_device(ctx, h1, q.annot, q._ht, int(q._out.d_theta), d_hit_mass=q.hits.mass)
        unit = coverage.isoform_coverage_device(ctx, h1, q.annot, q._ht, int(q._out.d_theta))
        assert (unit.exon_bases > 0.0).tolist() == (c1.exon_bases > 0.0).tolist() and unit.iso_bases.sum() > 0.0
        h2 = call()
        rc, why = try_cover(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        c2 = coverage.isoform_coverage_device(ctx, h2, q.annot, q._ht, int(q._out.d_theta), d_hit_mass=q.hits.mass)
        hit_locus = np.repeat(np.arange(q.n_loci), np.diff(np.asarray(q.hits.locus_hit_off)))
        CU.compare(c2, c1, q.annot, hit_locus, False, "the same call twice")
    finally:
        context.context_table_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()
