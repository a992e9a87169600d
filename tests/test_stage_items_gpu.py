"""The work-item boundary of the retained-result stages (csrc/stage_host.h: build_hit_items, kStageItemHits): two loci of two
isoforms with exactly 16384 and 16385 hits -- one item that owns its results (plain stores) and one locus split in two (the second
item holds a single hit; atomics) -- through one resident call with retention on, then the `-f` table, the fragment assignment
and the isoform coverage on that one handle, each against its host form: integers exactly, floating sums with the helpers and
bounds tests/test_retained_edges_gpu.py and tests/test_isoform_coverage_gpu.py use for split loci."""
import numpy as np
import pytest

import coverage_util as CU
import retained_util as R
from strawberry_amd import assign, context, coverage
from strawberry_amd import exonbin as eb
from test_context_table_gpu import assert_same_table
from test_fragment_assign_gpu import assert_same_assignment
from test_isoform_coverage_gpu import device_hits, host_forms

pytestmark = pytest.mark.gpu
COUNTS = (R.ITEM_HITS, R.ITEM_HITS + 1)


def boundary_sample():
    """-> (Annotation, Hits): locus l has COUNTS[l] unique hits; built as retained_util.edge_sample() builds its locus A"""
    rng = np.random.default_rng(R.SEED)
    loci, keyed = [], []
    for l, n_want in enumerate(COUNTS):
        base = 10000 + R.STRIDE * l
        ex = [(base + 700 * k, base + 700 * k + 399) for k in range(6)]
        isos = R.exon_subsets(rng, ex, 2)
        own = set()
        for lb, rb in R.sampled_pairs(rng, isos, 30000):
            if len(own) == n_want:
                break
            f = eb.hit_features(list(lb), list(rb))
            if f is not None:
                own.add((l, f[1][0], f[2][-1], tuple(map(tuple, f))))
        assert len(own) == n_want
        loci.append(isos)
        keyed += sorted(own)
    annot = eb.Annotation(loci)
    hits = eb.Hits([k[0] for k in keyed], [k[3] for k in keyed])
    hits.mass = np.ascontiguousarray(R.MASSES[np.random.default_rng(R.SEED + 1).integers(0, R.MASSES.size, hits.n_hits)])
    return annot, hits


def test_one_item_and_one_item_plus_a_hit(oracle):
    import torch
    from strawberry_amd import em
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    ctx = em.default_context(0)
    annot, hits = boundary_sample()
    hits_of = np.bincount(hits.hit_locus, minlength=annot.n_loci)
    assert hits_of.tolist() == list(COUNTS) and np.diff(annot.iso_off).tolist() == [2, 2]
    assert coverage.limits()["item_hits"] == R.ITEM_HITS and R.n_items(hits_of) == 3
    law = InsertSize(*R.LAW)
    dev = torch.device("cuda", ctx.device)
    # (with_context: the call runs with retention on and builds the table once itself)
    r = quantify_resident(annot, hits, law, R.RL, hits.n_hits, keep_handle=True, ctx=ctx, min_isoform_frac=R.MIN_ISOFORM_FRAC, with_context=True)
    with r["handle"] as handle:
        d_hits, own = device_hits(hits, dev)
        d_theta, d_mass = torch.from_numpy(r["theta"].copy()).to(dev), torch.from_numpy(hits.mass.copy()).to(dev)
        t = context.context_table_device(ctx, handle)
        a = assign.fragment_assign_device(ctx, handle, d_theta, hits.n_hits, d_hit_mass=d_mass)
        c = coverage.isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=d_mass)
        del own
    h = quantify_host(annot, hits, law, R.RL, ctx=ctx, assignment_theta=r["theta"], assignment_keep=r["keep"], assignment_status=r["status"],
                      context_keep=r["keep"], context_status=r["status"])
    for k in ("theta", "status", "iters"):
        np.testing.assert_array_equal(h[k], r[k], err_msg=k)
    what = "16384 and 16385 hits"
    # the table: all integers and copies of weights -- exact, rows and hits included
    assert_same_table(t, r["context"], what + ", the table again on the handle")
    assert_same_table(t, h["context"], what)
    assert t.locus_hits.tolist() == h["context"].locus_hits.tolist() and int(t.locus_hits.min()) > R.ITEM_HITS // 2
    # the assignment: map_iso, n_cand, map_prob, unique_mass, map_mass, unassigned exact; post_mass within (hits + 8) 2^-52
    assert_same_assignment(a, h["assignment"], annot.iso_off, hits_of, what)
    assert (a.map_iso >= 0).sum() > R.ITEM_HITS and (a.n_cand > 1).any() and (a.post_mass > 0.0).all()
    assert int(a.unassigned.sum()) == hits.n_hits - int((a.map_iso >= 0).sum())
    # the coverage: within (hits of the locus + 8) 2^-52 of the host form, zeros exactly
    host, = host_forms(oracle, annot, hits, h, r["keep"], r["status"], r["theta"])
    CU.compare(c, host, annot, hits.hit_locus, False, what + ", coverage")
    assert (c.exon_bases > 0.0).any() and (c.iso_bases > 0.0).all()
