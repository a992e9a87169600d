"""The `-f` table (csrc/context_device.h) and the fragment assignment (csrc/assign_device.h) on tests/retained_util.py::edge_sample():
more loci and more work items than twice the grid (every persistent loop takes a second and a third pass: the re-zeroing of the
LDS sums and counts, the barriers at the bottom of the loops, ctx_order_kernel's `continue`), more loci than two rounds of
ctx_scan_kernel, split loci of 6 and of 40 isoforms (the 32 LDS copies and the single copy, flushed by fp64 global atomics), a
locus of 300 isoforms (ten compat words; the column loop strides, F is not staged), and a locus on either side of every
threshold (8 / 9 and 32 / 33 isoforms, 256 / 257 and 1024 / 1025 bins).

Device against the host form as the existing tests compare them, AND against the independent restatements of
tests/test_fragment_assign.py::by_hand and tests/test_context_table.py::arrays_by_hand -- the two forms share assign_rules.h and
context_rules.h, the restatements share nothing with them."""
import numpy as np
import pytest

import retained_util as R
from strawberry_amd import _lib, assign, context
from strawberry_amd import exonbin as eb
from test_context_table import arrays_by_hand, check_arrays
from test_context_table_gpu import assert_same_table
from test_fragment_assign import by_hand
from test_fragment_assign_gpu import assert_same_assignment, bits

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
PER_HIT, PER_ISO = ("map_iso", "n_cand", "map_prob"), ("unique_mass", "map_mass", "post_mass")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


class Picked:
    """The arrays of a FragmentAssignment for some loci only (what assert_same_assignment reads)"""

    def __init__(self, a, hit_mask, iso_mask, locus_mask):
        self.n_hits = int(hit_mask.sum())
        for k in PER_HIT:
            setattr(self, k, np.ascontiguousarray(np.asarray(getattr(a, k))[hit_mask]))
        for k in PER_ISO:
            setattr(self, k, np.ascontiguousarray(np.asarray(getattr(a, k))[iso_mask]))
        self.unassigned = np.ascontiguousarray(np.asarray(a.unassigned)[locus_mask])


@pytest.fixture(scope="module")
def E(ctx):
    """One resident call with table and assignment, both again in turns on its handle, the same call once more, the host call
    under the resident call's theta / keep / status, and the two restatements on the host call's bins, words and weights."""
    import torch
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n_small, grid = R.n_small_for(cu), R.GRID_PER_CU * cu
    annot, hits = R.edge_sample(n_small, grid=grid)
    law = InsertSize(*R.LAW)
    kw = dict(ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_assignment=True, with_context=True)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, keep_handle=True, **kw)
    with r["handle"] as handle:
        dev = torch.device("cuda", ctx.device)
        d_theta, d_mass = torch.from_numpy(r["theta"].copy()).to(dev), torch.from_numpy(hits.mass.copy()).to(dev)
        turns = [assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass), context.context_table_device(ctx, handle),
                 assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass), context.context_table_device(ctx, handle)]
    again = quantify_resident(annot, hits, law, R.RL, hits.n_hits, **kw)
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx, assignment_theta=r["theta"], assignment_keep=r["keep"], assignment_status=r["status"],
                      context_keep=r["keep"], context_status=r["status"])
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    want, posterior = by_hand(h["bins"], hits.hit_locus, h["compat"], h["F"], r["theta"], r["keep"], r["status"], hits.mass)
    table_want = arrays_by_hand(h["bins"], h["compat"], h["F"], r["keep"], r["status"])
    fig = R.sample_conditions(annot, hits, h["bins"], h["F"], r["status"], r["keep"], want["n_cand"], posterior, n_small)
    assert R.device_conditions(fig, cu) == grid
    print({k: v for k, v in fig.items() if k not in ("hits_of", "hit_off")})
    nl = annot.n_loci
    niso, hits_of = np.diff(annot.iso_off), fig["hits_of"]
    return dict(annot=annot, hits=hits, r=r, a=r["assignment"], t=r["context"], turns=turns, again=again, h=h, want=want, table_want=table_want,
                fig=fig, grid=grid, nl=nl, niso=niso, hits_of=hits_of, at=R.edge_layout(n_small),
                hit_locus=np.asarray(hits.hit_locus, np.int64), mass=hits.mass.astype(np.float64))


def masks(E, loci):
    """loci: bool [n_loci] -> (hit mask, isoform mask, element mask)"""
    return loci[E["hit_locus"]], np.repeat(loci, E["niso"]), np.repeat(loci, np.diff(E["h"]["bins"].f_off))


def rows_of(t, loci):
    """the rows (global) of the loci picked, by the table's own offsets"""
    off = np.asarray(t.locus_row_off, np.int64)
    n = np.diff(off)[loci]
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    return np.repeat(off[:-1][loci] - start, n) + np.arange(int(n.sum()))


def same_assignment_on(E, a, b, loci, what):
    hm, im, _ = masks(E, loci)
    assert_same_assignment(Picked(a, hm, im, loci), Picked(b, hm, im, loci), np.concatenate([[0], np.cumsum(E["niso"][loci])]), E["hits_of"][loci], what)


def same_table_on(E, t, u, loci, what):
    np.testing.assert_array_equal(np.diff(t.locus_row_off)[loci], np.diff(u.locus_row_off)[loci], err_msg="%s rows per locus" % what)
    np.testing.assert_array_equal(t.locus_hits[loci], u.locus_hits[loci], err_msg="%s locus_hits" % what)
    rt, ru = rows_of(t, loci), rows_of(u, loci)
    for k in ("row_bin", "row_hits"):
        np.testing.assert_array_equal(getattr(t, k)[rt], getattr(u, k)[ru], err_msg="%s %s" % (what, k))
    em = masks(E, loci)[2]
    np.testing.assert_array_equal(t.row_prob[:em.size][em].view(np.uint64), u.row_prob[:em.size][em].view(np.uint64), err_msg="%s row_prob" % what)


def against_by_hand(E, a, loci, what):
    """The device assignment of the loci picked against the restatement: map_iso, n_cand, unassigned exact; unique_mass and map_mass
    exact (see test_device_equals_the_host_form); map_prob within (niso + hits + 8) 2^-52, the host test's bound; post_mass within
    (2 hits + niso + 16) 2^-52: the device-to-host bound (hits + 8) plus the host-to-restatement bound (niso + hits + 8)."""
    w = E["want"]
    hm, im, _ = masks(E, loci)
    for k in ("map_iso", "n_cand"):
        np.testing.assert_array_equal(np.asarray(getattr(a, k))[hm], np.asarray(w[k])[hm], err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(np.asarray(a.unassigned)[loci], np.asarray(w["unassigned"])[loci], err_msg="%s unassigned" % what)
    for k in ("unique_mass", "map_mass"):
        np.testing.assert_array_equal(np.asarray(getattr(a, k))[im], np.asarray(w[k], np.float64)[im], err_msg="%s %s" % (what, k))
    per_locus = (E["niso"] + E["hits_of"] + 8.0) * EPS
    worst = {}
    for k, bound, mask in (("map_prob", per_locus[E["hit_locus"]][hm], hm), ("post_mass", np.repeat(per_locus + (E["hits_of"] + 8.0) * EPS, E["niso"])[im], im)):
        got, ref = np.asarray(getattr(a, k))[mask], np.asarray(w[k], np.float64)[mask]
        err = np.abs(got - ref)
        share = err / np.where(ref > 0.0, bound * ref, 1.0)
        worst[k] = float(share.max(initial=0.0))
        print("%s %s against the restatement: worst share of its bound %.3f" % (what, k, worst[k]))
        assert (err <= bound * ref).all(), (what, k, int(np.argmax(share)), float(share.max()))
    return worst


def table_against_by_hand(E, t, loci, what):
    off, lhits, rbin, rhits, probs = E["table_want"]
    off = np.asarray(off, np.int64)
    np.testing.assert_array_equal(np.diff(t.locus_row_off)[loci], np.diff(off)[loci], err_msg="%s rows per locus" % what)
    np.testing.assert_array_equal(t.locus_hits[loci], np.asarray(lhits, np.uint32)[loci], err_msg="%s locus_hits" % what)
    rt = rows_of(t, loci)
    n = np.diff(off)[loci]
    rw = np.repeat(off[:-1][loci] - np.concatenate([[0], np.cumsum(n)])[:-1], n) + np.arange(int(n.sum()))
    np.testing.assert_array_equal(t.row_bin[rt], np.asarray(rbin, np.int64)[rw], err_msg="%s row_bin" % what)
    np.testing.assert_array_equal(t.row_hits[rt], np.asarray(rhits, np.uint32)[rw], err_msg="%s row_hits" % what)
    b = E["h"]["bins"]
    for l in np.nonzero(loci)[0]:
        for k in range(int(off[l + 1] - off[l])):
            r = int(t.locus_row_off[l]) + k
            assert t.row(l, r, b.iso_off, b.f_off).tolist() == probs[int(off[l]) + k], (what, l, k)     # exact: copies of F, or 0.0


def test_device_equals_the_host_form(E):
    """The existing comparisons, unchanged, on this sample.  unique_mass and map_mass stay EXACT under these fractional masses:
    float32 masses between 2^-3 and 1 have 24-bit mantissas, so every one of them is a multiple of 2^-26, and a sum of them
    below 2^27 is a multiple of 2^-26 below 2^53 of them: exact in double whatever the order.  If this comparison fails, the
    kernel is wrong, not the bound."""
    assert E["hits"].mass.min() >= 2.0 ** -3 and E["hits"].mass.max() <= 1.0 and E["hits"].mass.astype(np.float64).sum() < 2.0 ** 27
    assert_same_table(E["t"], E["h"]["context"], "edge sample")
    assert_same_assignment(E["a"], E["h"]["assignment"], E["annot"].iso_off, E["hits_of"], "edge sample")
    assert E["again"]["bins"].grouped_on_device and E["a"].n_hits == E["hits"].n_hits


def test_device_equals_the_restatements(E):
    every = np.ones(E["nl"], bool)
    check_arrays(E["t"], E["h"]["bins"], E["table_want"])
    against_by_hand(E, E["a"], every, "edge sample")


def invariants(E, a, t, l, mass, what):
    """What holds for one locus whatever its shape"""
    annot, b = E["annot"], E["h"]["bins"]
    i0, i1 = int(annot.iso_off[l]), int(annot.iso_off[l + 1])
    h0, h1 = int(E["fig"]["hit_off"][l]), int(E["fig"]["hit_off"][l + 1])
    on = a.map_iso[h0:h1] >= 0
    assigned = float(mass[h0:h1][on].sum())
    total = float(a.post_mass[i0:i1].sum())
    bound = (i1 - i0 + (h1 - h0) + 8) * EPS
    assert abs(total - assigned) <= bound * assigned, (what, total, assigned)        # the posterior mass is the assigned hits' mass
    assert abs(float(a.map_mass[i0:i1].sum()) - assigned) <= bound * assigned, (what, "map_mass")
    assert (a.unique_mass[i0:i1] <= a.map_mass[i0:i1]).all(), what
    erased = E["r"]["keep"][i0:i1] == 0
    for k in PER_ISO:
        assert (getattr(a, k)[i0:i1][erased] == 0.0).all(), (what, k)               # erased isoforms hold nothing
    assert not erased[a.map_iso[h0:h1][on]].any(), what
    assert int(a.unassigned[l]) == (h1 - h0) - int(on.sum()), what
    assert ((a.map_prob[h0:h1] > 0.0) == on).all() and (a.map_prob[h0:h1] <= 1.0 + bound).all(), what
    r0, r1 = int(t.locus_row_off[l]), int(t.locus_row_off[l + 1])
    coords = b.bin_coords(l)
    got = [tuple(coords[x - int(b.row_off[l])]) for x in t.row_bin[r0:r1].tolist()]
    assert got == sorted(got) and len(set(got)) == len(got), what                    # rows in the order of Python's sorted coordinate tuples
    assert int(t.row_hits[r0:r1].sum()) == int(t.locus_hits[l]) <= h1 - h0 and (t.row_hits[r0:r1] > 0).all(), what
    return on, r1 - r0


@pytest.mark.parametrize("name", R.SPECIAL)
def test_each_shape_on_its_own(E, name):
    l = E["at"][name]
    what = "locus %s (%d isoforms, %d bins, %d hits)" % (name, E["niso"][l], int(np.diff(E["h"]["bins"].row_off)[l]), E["hits_of"][l])
    only = np.zeros(E["nl"], bool)
    only[l] = True
    same_assignment_on(E, E["a"], E["h"]["assignment"], only, what)
    same_table_on(E, E["t"], E["h"]["context"], only, what)
    against_by_hand(E, E["a"], only, what)
    table_against_by_hand(E, E["t"], only, what)
    on, n_rows = invariants(E, E["a"], E["t"], l, E["mass"], what)
    nb = int(np.diff(E["h"]["bins"].row_off)[l])
    if name in ("EMPTY", "NOBIN"):
        assert not on.any() and n_rows == 0 and int(E["a"].unassigned[l]) == E["hits_of"][l]
        return
    assert on.any() and 0 < n_rows <= nb
    i0, i1 = int(E["annot"].iso_off[l]), int(E["annot"].iso_off[l + 1])
    erased = E["r"]["keep"][i0:i1] == 0
    assert (E["a"].post_mass[i0:i1] > 0.0).sum() > 1                                  # the sums went to several addresses
    if name in R.EXACT_BINS:
        assert nb == R.EXACT_BINS[name]
    for first in (32, 256):                                                           # ... beyond the first compat word, beyond the column loop's first stride
        if E["niso"][l] > first:
            assert (E["a"].post_mass[i0 + first:i1] > 0.0).any() or erased[first:].all()


def test_the_later_passes_of_the_persistent_loops(E):
    """A workgroup's second, third, ... locus (asg_column_kernel, ctx_order_kernel, ctx_gather_kernel: locus l is taken in pass
    l // grid) and its second, third, ... work item (asg_hit_kernel, ctx_count_kernel: item i in pass i // grid), each pass compared
    as a group of its own, so that the first pass being right cannot average a failure away."""
    grid, nl = E["grid"], E["nl"]
    by_locus = np.arange(nl) // grid
    # every work item's locus (a split locus has several, behind each other; a locus without hits has none) and the item's pass
    item_locus = np.repeat(np.arange(nl), -(-E["hits_of"] // R.ITEM_HITS))
    item_pass = np.arange(item_locus.size) // grid
    assert by_locus.max() >= 2 and item_pass.max() >= 2
    for how, last in (("loci", int(by_locus.max())), ("work items", int(item_pass.max()))):
        for p in range(1, last + 1):
            if how == "loci":
                group = by_locus == p
            else:       # the loci with an item in this pass
                group = np.zeros(nl, bool)
                group[item_locus[item_pass == p]] = True
            what = "pass %d of the grid over the %s" % (p + 1, how)
            assert group.sum() > (grid // 2 if p < last else 0), what
            same_assignment_on(E, E["a"], E["h"]["assignment"], group, what)
            same_table_on(E, E["t"], E["h"]["context"], group, what)
            against_by_hand(E, E["a"], group, what)
            table_against_by_hand(E, E["t"], group, what)
    # a workgroup's next locus differs in width from the one before
    small = np.ones(E["nl"], bool)
    small[list(E["at"].values())] = False
    l = np.nonzero(small[:-grid] & small[grid:])[0]
    assert (E["niso"][l] != E["niso"][l + grid]).all()


def test_the_later_rounds_of_the_row_scan(E):
    """ctx_scan_kernel scans 4096 loci per round and carries the rows so far into the next one."""
    want = np.asarray(E["table_want"][0], np.int64)
    got = np.asarray(E["t"].locus_row_off, np.int64)
    rounds = np.arange(E["nl"] + 1) // R.SCAN_ROUND
    assert rounds.max() >= 2
    for k in range(1, int(rounds.max()) + 1):
        np.testing.assert_array_equal(got[rounds == k], want[rounds == k], err_msg="locus_row_off in round %d of the scan" % (k + 1))
        assert (np.diff(want[rounds == k]) > 0).any()
    assert E["t"].n_rows == want[-1] > 2 * R.SCAN_ROUND


def test_the_same_call_twice_and_table_and_assignment_in_turns(E):
    a1, t1, a2, t2 = E["turns"]
    for what, t in (("the table behind an assignment", t1), ("the table behind two assignments", t2), ("the same call again", E["again"]["context"])):
        assert_same_table(t, E["t"], what)
    for what, a in (("the assignment again", a1), ("the assignment behind a table", a2), ("the same call again", E["again"]["assignment"])):
        assert_same_assignment(a, E["a"], E["annot"].iso_off, E["hits_of"], what)       # exact arrays; post_mass within the device-to-device bound
    for k in ("theta", "fpkm", "frac", "tpm", "keep", "status", "iters"):
        np.testing.assert_array_equal(bits(E["again"][k]), bits(E["r"][k]), err_msg=k)


def test_front_quantifier_fragment_assignment(ctx):
    """FrontQuantifier.fragment_assignment(): the unique hits of step() -- and the stream of stream_step() -- live on behind the pass
    for their masses.  Records -> assignment, the table in between, the same records through the chunked stream."""
    import stream_util as SU
    from strawberry_amd import front
    kw = dict(n_loci=200, n_frags=1e5, seed=23, resident=True, empirical=True, min_isoform_frac=0.002)
    plain = front.FrontQuantifier(ctx, **kw)
    try:
        plain.step()
        with pytest.raises(_lib.SbgpuError, match="no pass has run with keep_context=True"):
            plain._assignment_hits()
        with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
            plain.fragment_assignment()
    finally:
        plain.close()
    q = front.FrontQuantifier(ctx, keep_context=True, **kw)
    try:
        q.step()
        iso_off, hits_of = np.asarray(q.annot.iso_off), np.diff(q.front_hit_off)
        keep, theta = q.keep[:q.n_iso].copy(), q.theta[:q.n_iso].copy()
        a1 = q.fragment_assignment()
        t = q.context_table()
        a2 = q.fragment_assignment()
        assert a1.n_hits == int(q.front_hit_off[-1]) == q._front_hits[3] and t.n_rows > q.n_loci
        assert_same_assignment(a2, a1, iso_off, hits_of, "behind the table")
        q.to_host(q.n_bytes // 6 + 4096, pinned=False)
        info = q.stream_step()
        assert info["chunks"] > 3 and info["unique_hits"] == a1.n_hits
        np.testing.assert_array_equal(q.front_hit_off, np.concatenate([[0], np.cumsum(hits_of)]))
        np.testing.assert_array_equal(q.theta[:q.n_iso].view(np.uint64), theta.view(np.uint64))
        d_mass, n = q._assignment_hits()
        mass = SU._d2h(d_mass, n, np.float32).astype(np.float64)       # the masses of sbgpu_front_stream_hits
        a3 = q.fragment_assignment()
        assert_same_assignment(a3, a1, iso_off, hits_of, "through the stream")
        t3 = q.context_table()
        assert_same_table(t3, t, "through the stream")
        # the invariants of every locus under those masses
        assert n == a3.n_hits and (mass > 0.0).all()
        on = a3.map_iso >= 0
        loc = np.repeat(np.arange(q.n_loci), hits_of)
        assigned = np.bincount(loc, weights=np.where(on, mass, 0.0), minlength=q.n_loci)
        bound = (hits_of + np.diff(iso_off) + 8) * EPS * assigned
        for k in ("post_mass", "map_mass"):
            assert (np.abs(np.add.reduceat(getattr(a3, k), iso_off[:-1]) - assigned) <= bound).all(), k
        assert (a3.unique_mass <= a3.map_mass).all() and (a3.post_mass[keep == 0] == 0.0).all() and (a3.map_mass[keep == 0] == 0.0).all()
        np.testing.assert_array_equal(a3.unassigned, hits_of - np.bincount(loc, weights=on, minlength=q.n_loci).astype(np.int64))
        assert on.sum() > n // 2 and (a3.n_cand > 1).sum() > n // 20
        # ... and the table's: row_hits sums to locus_hits, the rows come in the order of Python's sorted coordinate tuples
        # (the bins' keys come from the pass' handle: exporting it is the last thing done with it)
        row_locus = np.repeat(np.arange(q.n_loci), np.diff(t3.locus_row_off))
        np.testing.assert_array_equal(np.bincount(row_locus, weights=t3.row_hits[:t3.n_rows], minlength=q.n_loci).astype(np.uint32), t3.locus_hits)
        assert (t3.row_hits[:t3.n_rows] > 0).all() and (t3.locus_hits <= hits_of).all() and int(t3.locus_hits.sum()) > n // 2
        bins = eb.LocusBins.__new__(eb.LocusBins)
        handle, q.context_handle = q.context_handle, None
        bins._export(ctx.L, q.annot, handle, n, q.annot.compat_words, q.annot.key_words, with_hit_bin=False)   # destroys the handle
        for l in range(q.n_loci):
            coords = bins.bin_coords(l)
            r0, r1 = int(t3.locus_row_off[l]), int(t3.locus_row_off[l + 1])
            got = [tuple(coords[b - int(bins.row_off[l])]) for b in t3.row_bin[r0:r1].tolist()]
            assert got == sorted(got) and len(set(got)) == len(got), l
    finally:
        q.close()
    # closed: the kept stream and the handle are gone, and nothing reads them
    assert q._front_hits is None and q.context_handle is None
    with pytest.raises(_lib.SbgpuError, match="keep_context=True"):
        q.fragment_assignment()
    with pytest.raises(_lib.SbgpuError, match="no pass has run with keep_context=True"):
        q._assignment_hits()
