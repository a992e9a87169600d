"""Transcript-body coverage profile built on the device (sbgpu_body_profile_device, csrc/body_device.h) from what a resident call
leaves in HBM and the hits it was given, against the host form (sbgpu_body_profile_host under the resident call's theta, keep and
status) and against tests/body_util.py::by_hand, under the bounds of that file's head; zeros, -1.0 and class_n exactly.  On the
toy directories, on tests/body_util.py::body_sample() as a whole, locus by locus (a locus on either side of every threshold of the
kernel, by the constants the library exports) and pass by pass of the grid, at P = 1, 20, 96 and 100, in the all-integer case bit
for bit, under another theta, in every position among the other retained-result stages, through the chain and the front
quantifiers, at the work-item boundary, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import body_util as BU
import coverage_util as CU
import retained_util as R
import stream_util as S
from strawberry_amd import _lib, body, context, coverage
from strawberry_amd import exonbin as eb
from test_context_table import Handle
from test_context_table_gpu import MUST_BE_RESIDENT, RL, RUNS, assert_same_table, law_of, toy
from test_fragment_assign_gpu import assert_same_assignment, bits
from test_isoform_coverage_gpu import device_hits, front_hits

pytestmark = pytest.mark.gpu
STATS = ("body_bases", "body_total", "body_center", "body_cv")
P_LIST = (1, 20, 96, 100)       # 96: 32 isoforms x 96 bins are the LDS sums' 3072, 33 x 96 are beyond


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def host_forms(oracle, annot, hits, h, keep, status, strand, calls, unit_masses=False):
    """sbgpu_body_profile_host for each (theta, n_pos) of `calls`, on a host handle over the hits of h = quantify_host(annot, hits,
    ...): sbgpu_bins_create on the oracle's words numbers the bins as sbgpu_quantify_host did (asserted), so h["F"] are its weights."""
    compat, key = oracle.exonbin_batch(annot, hits)
    np.testing.assert_array_equal(compat, h["compat"])
    own = eb.LocusBins(annot, hits, compat, key)
    np.testing.assert_array_equal(own.hit_bin, h["bins"].hit_bin)
    np.testing.assert_array_equal(own.f_off, h["bins"].f_off)
    with Handle(annot, hits, compat, key) as H:
        return [body.body_profile_host(H.h, annot, hits, compat, t, F=h["F"], keep=keep, status=status, hit_mass=None if unit_masses else hits.mass,
                                       iso_strand=strand, n_pos=P) for t, P in calls]


@pytest.mark.parametrize("which", MUST_BE_RESIDENT)
def test_device_profile_on_the_toy_directories(ctx, oracle, which):
    from strawberry_amd.quantify import quantify_host, quantify_resident
    g = toy(which)
    annot, hits = g["annot"], g["hits"]
    strand = BU.strands_of(annot)
    law, long_read, min_frac = law_of(which), bool(RUNS[which][1]), RUNS[which][2]
    kw = dict(long_read=long_read, ctx=ctx, min_isoform_frac=min_frac)
    r = quantify_resident(annot, hits, law, RL, hits.total_mapped, with_body_profile=True, iso_strand=strand, **kw)
    plain = quantify_resident(annot, hits, law, RL, hits.total_mapped, **kw)
    for k in S.OUT_KEYS:        # the call's own seven results: the bytes of the same call with no profile behind it
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    c = r["body_profile"]
    assert r["bins"].grouped_on_device and c.n_pos == 20
    h = quantify_host(annot, hits, law, RL, long_read=long_read, ctx=ctx)
    host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], strand, [(r["theta"], 20)])
    BU.compare(c, host, annot, hits.hit_locus, False, which + ", device against host", 20, strand)
    want = BU.by_hand(h["bins"], annot, hits, h["compat"], h["F"], r["theta"], r["keep"], r["status"], hits.mass, strand, 20, per_base=True)
    BU.compare(c, want, annot, hits.hit_locus, True, which + ", device against the restatement", 20, strand)
    BU.stats_of_own_bins(c, annot, strand, which)
    assert (c.body_total > 0.0).any() and (c.body_total[r["keep"] == 0] == 0.0).all() and set(c.device) == set(BU.NAMES)
    assert int(c.class_n.sum()) == int((c.body_total > 0.0).sum())


@pytest.fixture(scope="module")
def E(ctx, oracle):
    """One resident call on the body sample with the profile behind it (P = 20); on its handle the other P, the all-integer case
    (one-hot theta, unit masses), the same call again and the coverage; the host forms of all of them on a host handle over the
    same hits; the restatement at P = 20."""
    import torch
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small, grid = R.n_small_for(cu), R.GRID_PER_CU * cu
    annot, hits = BU.body_sample(n_small, grid=grid)
    strand = BU.strands_of(annot)
    law = InsertSize(*R.LAW)
    dev = torch.device("cuda", ctx.device)
    hot = np.zeros(int(annot.iso_off[-1]))
    hot[np.asarray(annot.iso_off[:-1], np.int64)] = 1.0
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, keep_handle=True, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_body_profile=True,
                          iso_strand=strand)
    dev_p = {20: r["body_profile"]}
    with r["handle"] as handle:
        d_hits, own = device_hits(hits, dev)
        d_hot, d_theta, d_mass = torch.from_numpy(hot).to(dev), torch.from_numpy(r["theta"].copy()).to(dev), torch.from_numpy(hits.mass.copy()).to(dev)
        exact = body.body_profile_device(ctx, handle, annot, d_hits, d_hot, iso_strand=strand)
        for P in P_LIST:
            if P != 20:
                dev_p[P] = body.body_profile_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass, iso_strand=strand, n_pos=P)
        again = body.body_profile_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass, iso_strand=strand)
        cov = coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)
        del own
    plain = quantify_resident(annot, hits, law, R.RL, hits.n_hits, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    for k in S.OUT_KEYS:        # the call's own seven results: the bytes of the same call with no profile behind it
        np.testing.assert_array_equal(bits(r[k]), bits(plain[k]), err_msg=k)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    hosts = host_forms(oracle, annot, hits, h, r["keep"], r["status"], strand, [(r["theta"], P) for P in P_LIST])
    exact_host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], strand, [(hot, 20)], unit_masses=True)
    want = BU.by_hand(h["bins"], annot, hits, h["compat"], h["F"], r["theta"], r["keep"], r["status"], hits.mass, strand, 20)
    at = R.edge_layout(n_small)
    print(BU.sample_conditions(annot, want, strand, 20))
    hits_of = np.bincount(hits.hit_locus, minlength=annot.n_loci)
    return dict(annot=annot, hits=hits, strand=strand, r=r, dev=dev_p, host=dict(zip(P_LIST, hosts)), again=again, exact=exact, exact_host=exact_host,
                cov=cov, want=want, at=at, cu=cu, grid=grid, hits_of=hits_of, nl=annot.n_loci)


def test_the_sample_lies_on_either_side_of_every_threshold(E):
    """... by the constants the library exports; its work items exceed two passes of the grid, its isoforms twice body_iso_kernel's"""
    lim = body.limits()
    annot, at = E["annot"], E["at"]
    niso = np.diff(annot.iso_off)
    nex = np.diff(np.asarray(annot.exon_off)[np.asarray(annot.iso_off)])
    in_lds = lambda l, P: niso[l] <= lim["lds_iso"] and nex[l] <= lim["lds_exons"] and niso[l] * P <= lim["lds_sums"]  # noqa: E731
    copies = lambda l, P: in_lds(l, P) and niso[l] <= lim["narrow_iso"] and niso[l] * P * lim["copies"] <= lim["lds_sums"]  # noqa: E731
    assert lim["item_hits"] == R.ITEM_HITS and lim["narrow_iso"] * lim["copies"] <= lim["lds_sums"]
    assert R.n_items(E["hits_of"]) > 2 * E["grid"] and E["nl"] > 2 * E["grid"]
    n_iso = int(annot.iso_off[-1])
    iso_grid = min(-(-n_iso // 256), E["grid"])
    assert n_iso > 2 * iso_grid and iso_grid > 1
    # LDS against global tables: C (300 isoforms) is beyond lds_iso at every P; B (40) and T33 leave LDS as P grows, T32 at 96 is the last that fits
    assert niso[at["C"]] == 300 > lim["lds_iso"] and all(not in_lds(at["C"], P) for P in P_LIST)
    assert in_lds(at["B"], 20) and not in_lds(at["B"], 96) and not in_lds(at["B"], 100)
    assert niso[at["T32"]] * 96 == lim["lds_sums"] and in_lds(at["T32"], 96) and not in_lds(at["T33"], 96) and not in_lds(at["T32"], 100)
    assert all(in_lds(at[k], 1) for k in R.SPECIAL if k != "C") and all(nex[at[k]] <= lim["lds_exons"] for k in R.SPECIAL if k != "C")
    # copies against no copies: T8 / T9 at P = 20; A (six isoforms, split) with copies at 20 and without at 96; the small loci (2 and 3
    # isoforms) with copies up to 96 and 64 bins, none at 100
    assert copies(at["T8"], 20) and not copies(at["T9"], 20) and in_lds(at["T9"], 20) and niso[at["T8"]] == lim["narrow_iso"]
    assert copies(at["A"], 20) and not copies(at["A"], 96) and in_lds(at["A"], 96)
    small = [l for l in range(5) if l not in at.values()]
    assert {int(niso[l]) for l in small} == {2, 3}
    assert all(copies(l, 20) and not copies(l, 100) for l in small) and any(copies(l, 96) for l in small) and not all(copies(l, 96) for l in small)
    # split loci on either side of the copies and of LDS: A (three items) and B (two)
    assert 2 * lim["item_hits"] < E["hits_of"][at["A"]] < 3 * lim["item_hits"] < 3 * E["hits_of"][at["B"]] < 6 * lim["item_hits"]


@pytest.mark.parametrize("P", P_LIST)
def test_device_equals_the_host_form_at_every_bin_count(E, P):
    annot, hits, strand = E["annot"], E["hits"], E["strand"]
    c, host = E["dev"][P], E["host"][P]
    assert c.n_pos == P and c.body_bases.shape == (int(annot.iso_off[-1]), P)
    BU.compare(c, host, annot, hits.hit_locus, False, "body sample, P = %d, device against host" % P, P, strand)
    BU.stats_of_own_bins(c, annot, strand, "P = %d" % P)
    assert c.class_n.tolist() == host.class_n.tolist() and (c.class_n > 0).all() and int(c.class_n.sum()) == int((c.body_total > 0.0).sum())
    # conservation against the coverage built on the same handle: every isoform of every locus
    hits_of, niso, iso_locus = BU.shape(annot, hits.hit_locus)
    iso_bases = E["cov"].iso_bases
    bound = (2.0 * hits_of[iso_locus] + np.diff(annot.exon_off) + P + 16.0) * BU.EPS
    sums = c.body_bases.sum(axis=1)
    assert (np.abs(sums - iso_bases) <= bound * iso_bases).all()
    np.testing.assert_array_equal(sums[iso_bases == 0.0], 0.0)


def test_device_and_host_equal_the_restatement(E):
    annot, hits, strand = E["annot"], E["hits"], E["strand"]
    BU.compare(E["dev"][20], E["want"], annot, hits.hit_locus, True, "body sample, device against the restatement", 20, strand)
    BU.compare(E["host"][20], E["want"], annot, hits.hit_locus, True, "body sample, host against the restatement", 20, strand)
    BU.compare(E["again"], E["dev"][20], annot, hits.hit_locus, False, "body sample, the same call again", 20, strand)


@pytest.mark.parametrize("name", R.SPECIAL + ("TAIL",))
def test_each_shape_on_its_own(E, name):
    annot, hits, strand = E["annot"], E["hits"], E["strand"]
    l = E["nl"] - 1 if name == "TAIL" else E["at"][name]
    only = np.zeros(E["nl"], bool)
    only[l] = True
    i0, i1 = int(annot.iso_off[l]), int(annot.iso_off[l + 1])
    what = "locus %s (%d isoforms, %d hits)" % (name, i1 - i0, E["hits_of"][l])
    for P in P_LIST:
        BU.compare(E["dev"][P], E["host"][P], annot, hits.hit_locus, False, "%s, P = %d, device against host" % (what, P), P, strand, loci=only)
    c = E["dev"][20]
    BU.compare(c, E["want"], annot, hits.hit_locus, True, what + ", device against the restatement", 20, strand, loci=only)
    erased = E["r"]["keep"][i0:i1] == 0
    assert (c.body_total[i0:i1][erased] == 0.0).all() and (c.body_cv[i0:i1][erased] == -1.0).all(), what
    if name in ("EMPTY", "NOBIN"):
        assert (c.body_bases[i0:i1] == 0.0).all() and (c.body_center[i0:i1] == -1.0).all() and (c.body_cv[i0:i1] == -1.0).all()
        return
    if name != "TAIL":      # the sums went to many addresses
        assert (c.body_bases[i0:i1] > 0.0).sum() > 20 and (E["dev"][100].body_bases[i0:i1] > 0.0).sum() > 60, what
    if name == "C":         # beyond the first compat word, beyond the first stride of the staging loops
        assert (c.body_total[i0 + 256:i1] > 0.0).any() or erased[256:].all()
    if name == "TAIL":
        assert (body.iso_lengths(annot)[i0:i1] >= 4000).any()


def test_the_later_passes_of_the_persistent_loop(E):
    """A workgroup's second, third, ... work item (item i is taken in pass i // grid), each pass compared as a group of its own"""
    annot, hits, grid, nl, strand = E["annot"], E["hits"], E["grid"], E["nl"], E["strand"]
    item_locus = np.repeat(np.arange(nl), -(-E["hits_of"] // R.ITEM_HITS))
    item_pass = np.arange(item_locus.size) // grid
    assert item_pass.max() >= 2
    for p in range(1, int(item_pass.max()) + 1):
        group = np.zeros(nl, bool)
        group[item_locus[item_pass == p]] = True
        what = "pass %d of the grid over the work items" % (p + 1)
        for P in (20, 100):
            BU.compare(E["dev"][P], E["host"][P], annot, hits.hit_locus, False, "%s, P = %d" % (what, P), P, strand, loci=group)
        BU.compare(E["dev"][20], E["want"], annot, hits.hit_locus, True, what + ", the restatement", 20, strand, loci=group)


def test_the_all_integer_case_is_bitwise(E):
    """one-hot theta, unit masses: every term is an integer, so device and host agree bit for bit in any order -- the bins, and
    with them the totals, centres and coefficients of variation; the class curves are sums of quotients: within their bound"""
    annot, hits, strand = E["annot"], E["hits"], E["strand"]
    BU.bitwise(E["exact"], E["exact_host"], "one-hot theta, unit masses", 20, names=STATS + ("class_n",))
    BU.compare(E["exact"], E["exact_host"], annot, hits.hit_locus, False, "one-hot theta, unit masses", 20, strand)
    x = E["exact"]
    assert (x.body_bases == np.round(x.body_bases)).all() and x.body_bases.sum() > 0
    for what, c in (("again", E["again"]), ("one-hot", E["exact"])):
        BU.stats_of_own_bins(c, annot, strand, what)


def test_two_bin_counts_on_one_handle_and_only_what_was_asked_for(E):
    """P = 100 ran between the call's own P = 20 and `again`: the second P = 20 is the first within the device-to-device bound"""
    assert E["again"].n_pos == 20 and E["dev"][100].body_bases.shape[1] == 100 and E["dev"][1].body_bases.shape[1] == 1
    one = E["dev"][1]
    some = one.body_total > 0.0
    assert (one.body_center[some] == 0.5).all() and (one.body_cv[some] == 0.0).all() and (one.body_total == one.body_bases[:, 0]).all()


def device_arrays_unchanged(res, what):
    """every device array a stage's result names still holds the bits that came to the host with it"""
    for name, ptr in res.device.items():
        a = getattr(res, name, None)
        if isinstance(a, np.ndarray) and a.size:
            a = np.ascontiguousarray(a).ravel()
            np.testing.assert_array_equal(bits(S._d2h(ptr, a.size, a.dtype)), bits(a), err_msg="%s: %s" % (what, name))


@pytest.fixture(scope="module")
def chain_sample(ctx, oracle):
    """2 000 loci of the chain workload with both retentions on: the profile in every position among table, assignment, coverage,
    fit, information and support, twice; under a bootstrap mean of theta; then the host forms."""
    import torch
    from strawberry_amd import chain
    from strawberry_amd.quantify import InsertSize, quantify_host
    q = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01, keep_context=True, keep_bootstrap=True)
    try:
        q.step()
        strand = BU.strands_of(q.annot)
        theta, keep, status = q.theta[:q.n_iso].copy(), q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        outputs = {k: getattr(q, k)[:(q.n_loci if k in ("status", "iters") else q.n_iso)].copy() for k in S.OUT_KEYS}
        others = [("table", q.context_table), ("assignment", q.fragment_assignment), ("coverage", q.isoform_coverage), ("fit", q.model_fit),
                  ("info", q.isoform_information), ("support", q.isoform_support)]
        first = {k: f() for k, f in others}
        profiles, later = [], {}
        for _ in range(2):
            p = q.body_profile(iso_strand=strand)                               # in front of all of them
            profiles.append(p)
            for k, f in others:
                later[k] = f()
                device_arrays_unchanged(p, "the profile across the " + k)
                p = q.body_profile(iso_strand=strand)                           # ... and behind each
                profiles.append(p)
                if k != "table":
                    device_arrays_unchanged(later[k], "the %s across the profile" % k)
        boot = q.abundance_bootstrap(8, 11, replicates=False)
        mean = np.ascontiguousarray(boot["theta_mean"])
        behind = q.body_profile(iso_strand=strand, d_theta=torch.from_numpy(mean).to(q.dev))
        few = q.body_profile(iso_strand=strand, n_pos=50, want=("class_profile", "class_n"))
        hits = q.hits.host_hits(q.n_loci)
        h = quantify_host(q.annot, hits, InsertSize(250.0, 30.0), 75, ctx=ctx)
        np.testing.assert_array_equal(h["theta"], theta)
        host, host_mean, host50 = host_forms(oracle, q.annot, hits, h, keep, status, strand, [(theta, 20), (mean, 20), (theta, 50)])
        with pytest.raises(_lib.SbgpuError, match="stale handle"):      # the host entry was this context's next quantify call
            q.body_profile()
        plain = chain.ChainQuantifier(ctx, n_loci=2000, n_frags=2000 * 300, seed=5, resident=True, min_isoform_frac=0.01)
        try:
            plain.step()
            for k in S.OUT_KEYS:        # the call's own seven results with and without retention and what is built from it
                np.testing.assert_array_equal(bits(getattr(plain, k)[:outputs[k].size]), bits(outputs[k]), err_msg=k)
        finally:
            plain.close()
        return dict(annot=q.annot, hits=hits, strand=strand, theta=theta, mean=mean, keep=keep, first=first, later=later, profiles=profiles, behind=behind,
                    few=few, host=host, host_mean=host_mean, host50=host50, hits_of=np.bincount(hits.hit_locus, minlength=q.n_loci))
    finally:
        q.close()


def test_the_profile_in_every_position_among_the_other_stages_twice(chain_sample):
    c = chain_sample
    annot, hits, strand = c["annot"], c["hits"], c["strand"]
    assert len(c["profiles"]) == 14
    for n, p in enumerate(c["profiles"]):
        what = "chain sample, profile %d" % n
        BU.compare(p, c["host"], annot, hits.hit_locus, False, what + ", against host", 20, strand)
        BU.compare(p, c["profiles"][0], annot, hits.hit_locus, False, what + ", against the first", 20, strand)
    # the others' arrays are what they were before any profile ran
    first, later = c["first"], c["later"]
    assert_same_table(later["table"], first["table"], "behind the profile")
    assert_same_assignment(later["assignment"], first["assignment"], np.asarray(annot.iso_off), c["hits_of"], "behind the profile")
    CU.compare(later["coverage"], first["coverage"], annot, hits.hit_locus, False, "coverage behind the profile")
    few = c["few"]          # only what was asked for comes to the host
    assert few.body_bases is None and few.body_total is None and set(few.device) == set(BU.NAMES) and few.class_profile.shape == (4, 50)
    assert few.class_n.tolist() == c["host50"].class_n.tolist()
    p = c["profiles"][0]
    assert (p.body_total[c["keep"] == 0] == 0.0).all() and (c["keep"] == 0).sum() > 20 and (p.body_total > 0.0).sum() > 2000


def test_a_theta_that_is_not_the_calls(chain_sample):
    """the bootstrap's mean of theta, from the same handle: the profile under it is the host form's under it"""
    c = chain_sample
    assert (c["mean"] != c["theta"]).sum() > c["theta"].size // 2
    BU.compare(c["behind"], c["host_mean"], c["annot"], c["hits"].hit_locus, False, "a bootstrap mean", 20, c["strand"])
    assert (c["behind"].body_bases != c["profiles"][0].body_bases).sum() > 100


def test_front_quantifier_body_profile(ctx, oracle):
    """FrontQuantifier.body_profile(): after step() on the unique hits of sbgpu_uniq_dev_hits, after stream_step() on
    sbgpu_front_stream_hits' -- the same hits, the same profile; and the host form's on those hits."""
    from strawberry_amd import front
    from strawberry_amd.quantify import quantify_host
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
            plain.body_profile()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_context=True, **kw)
    try:
        q.step()
        strand = BU.strands_of(q.annot)
        hit_locus = np.repeat(np.arange(q.n_loci), np.diff(q.front_hit_off))
        theta = q.theta[:q.n_iso].copy()
        keep, status = q.keep[:q.n_iso].copy(), q.status[:q.n_loci].copy()
        c1 = q.body_profile(iso_strand=strand)
        hits1 = front_hits(q)
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        info = q.stream_step()
        assert info["chunks"] > 3
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        c3 = q.body_profile(iso_strand=strand)
        BU.compare(c3, c1, q.annot, hit_locus, False, "through the stream", 20, strand)
        BU.stats_of_own_bins(c3, q.annot, strand, "through the stream")
        assert (c3.body_total[q.keep[:q.n_iso] == 0] == 0.0).all() and (c3.body_total > 0.0).sum() > q.n_loci
    finally:
        q.close()
    h = quantify_host(q.annot, hits1, None, q.read_len, ctx=ctx)
    np.testing.assert_array_equal(h["theta"].view(np.uint64), theta.view(np.uint64))
    host, = host_forms(oracle, q.annot, hits1, h, keep, status, strand, [(theta, 20)])
    BU.compare(c1, host, q.annot, hit_locus, False, "the front's hits, device against host", 20, strand)
    BU.compare(c3, host, q.annot, hit_locus, False, "the stream's hits, device against host", 20, strand)
    with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
        q.body_profile()


def test_one_item_and_one_item_plus_a_hit(ctx, oracle):
    """two loci of exactly 16384 and 16385 hits: one item that owns its results (plain stores), one locus split in two (atomics)"""
    import torch
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    from test_stage_items_gpu import COUNTS, boundary_sample
    annot, hits = boundary_sample()
    hits_of = np.bincount(hits.hit_locus, minlength=annot.n_loci)
    assert hits_of.tolist() == list(COUNTS) and body.limits()["item_hits"] == R.ITEM_HITS and R.n_items(hits_of) == 3
    law = InsertSize(*R.LAW)
    strand = np.array([1, 1, 2, 2], np.uint8)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_body_profile=True, iso_strand=strand, n_pos=100)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx)
    np.testing.assert_array_equal(h["theta"], r["theta"])
    host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], strand, [(r["theta"], 100)])
    BU.compare(r["body_profile"], host, annot, hits.hit_locus, False, "16384 and 16385 hits", 100, strand)
    assert (r["body_profile"].body_total > 0.0).all()


def test_refusals(ctx):
    """A handle made without retention, a stale one after another sbgpu_quantify_*, null arguments, a bad n_pos, a bad strand, hits of
    another count, another annotation."""
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

    def attempt(h, d_theta=True, n_hits=None, annot=None, P=20, strand=None, out=True):
        s = _lib.sbgpu_body_profile_t()
        ht = q.hits.struct()
        if n_hits is not None:
            ht.n_hits = n_hits
        rc = L.sbgpu_body_profile_device(ctx.h, h, C.byref(annot or an), C.byref(ht), q._out.d_theta if d_theta else None, None,
                                         None if strand is None else strand.ctypes.data, P, None, C.byref(s) if out else None)
        return rc, L.sbgpu_last_error().decode()
    try:
        h0 = call()
        rc, why = attempt(h0)
        assert rc == _lib.SBGPU_EINVAL and "without retention" in why, why
        context.context_table_keep(ctx, True)
        h1 = call()
        rc, why = attempt(h1, d_theta=False)
        assert rc == _lib.SBGPU_EINVAL and "d_theta is needed" in why, why
        rc, why = attempt(h1, out=False)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        for P in (0, 101):
            rc, why = attempt(h1, P=P)
            assert rc == _lib.SBGPU_EINVAL and "n_pos must be 1 .. 100" in why, why
        bad = np.zeros(q.n_iso, np.uint8)
        bad[-1] = 3
        rc, why = attempt(h1, strand=bad)
        assert rc == _lib.SBGPU_EINVAL and "iso_strand holds a value above 2" in why, why
        rc, why = attempt(h1, n_hits=q.n_hits - 1)
        assert rc == _lib.SBGPU_EINVAL and "d_hits->n_hits is not the retained call's" in why, why
        other = eb.Annotation([[[(1, 100), (201, 300)]]])
        rc, why = attempt(h1, annot=other._struct())
        assert rc == _lib.SBGPU_EINVAL and "the annotation's loci or isoforms are not the handle's" in why, why
        c1 = body.body_profile_device(ctx, h1, q.annot, q._ht, int(q._out.d_theta), d_hit_mass=q.hits.mass)
        unit = body.body_profile_device(ctx, h1, q.annot, q._ht, int(q._out.d_theta))
        assert (unit.body_bases > 0.0).tolist() == (c1.body_bases > 0.0).tolist() and unit.body_total.sum() > 0.0
        h2 = call()
        rc, why = attempt(h1)
        assert rc == _lib.SBGPU_EINVAL and "stale handle" in why, why
        c2 = body.body_profile_device(ctx, h2, q.annot, q._ht, int(q._out.d_theta), d_hit_mass=q.hits.mass)
        hit_locus = np.repeat(np.arange(q.n_loci), np.diff(np.asarray(q.hits.locus_hit_off)))
        BU.compare(c2, c1, q.annot, hit_locus, False, "the same call twice", 20)
    finally:
        context.context_table_keep(ctx, False)
        for h in handles:
            L.sbgpu_bins_destroy(h)
        q.close()
