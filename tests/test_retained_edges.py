"""tests/retained_util.py::edge_sample() on the CPU: the sample holds what it was built for, and on it the host forms of the `-f`
table (sbgpu_context_table_host) and of the fragment assignment (sbgpu_fragment_assign_host) equal the independent restatements
of tests/test_context_table.py and tests/test_fragment_assign.py -- which so far had seen four candidates per hit at most --
under their own bounds: (niso + hits of the locus + 8) * 2^-52 relative for map_prob and post_mass; everything else exact --
unique_mass and map_mass too, although the masses are fractions: float32 masses between 2^-3 and 1 are multiples of 2^-26, and
their sums stay far below 2^27, so they are exact in double in any order.

No GPU here: words from the oracle's exon-bin restatement, weights from its bin-weight model, theta / status from its EM, keep
from its epilogue.  tests/test_retained_edges_gpu.py runs the device forms on the same sample."""
import numpy as np
import pytest

import retained_util as R
from strawberry_amd import assign, context
from strawberry_amd import exonbin as eb
from test_context_table import Handle, arrays_by_hand, check_arrays, oracle_weights
from test_fragment_assign import by_hand, check

N_SMALL = 8200


@pytest.fixture(scope="module")
def S(oracle):
    annot, hits = R.edge_sample(N_SMALL, oracle=oracle)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    F = oracle_weights(oracle, bins, oracle.make_insert(*R.LAW), False)
    theta, status, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    ab = oracle.abundance(bins.iso_off, theta, status, bins.iso_len, hits.n_hits, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    want, posterior = by_hand(bins, hits.hit_locus, compat, F, theta, ab["keep"], status, hits.mass)
    return dict(annot=annot, hits=hits, compat=compat, key=key, bins=bins, F=F, theta=theta, status=status, keep=ab["keep"], want=want,
                posterior=posterior)


def test_the_sample_holds_what_it_was_built_for(S):
    fig = R.sample_conditions(S["annot"], S["hits"], S["bins"], S["F"], S["status"], S["keep"], S["want"]["n_cand"], S["posterior"], N_SMALL)
    print({k: v for k, v in fig.items() if k not in ("hits_of", "hit_off")})
    # on an MI355X (256 CUs: a grid of 2048) the loci and the work items are more than two passes of the grid
    assert R.device_conditions(fig, 256) == 2048
    at = R.edge_layout(N_SMALL)
    passes = {name: l // 2048 for name, l in at.items()}
    assert len({passes["A"], passes["B"]}) == 2 and max(passes.values()) >= 3 and min(passes.values()) == 0, passes   # spread, not all in front
    small = np.ones(S["annot"].n_loci, bool)
    small[list(at.values())] = False
    niso = np.diff(S["annot"].iso_off)
    l = np.nonzero(small[:-2048] & small[2048:])[0]
    assert (niso[l] != niso[l + 2048]).all()        # a workgroup's next locus differs in width


def test_host_assignment_equals_the_restatement(S):
    with Handle(S["annot"], S["hits"], S["compat"], S["key"]) as H:
        t = assign.fragment_assign_host(H.h, S["compat"], S["theta"], F=S["F"], keep=S["keep"], status=S["status"], hit_mass=S["hits"].mass)
    m = S["hits"].mass
    assert m.min() >= 2.0 ** -3 and m.max() <= 1.0 and m.astype(np.float64).sum() < 2.0 ** 27
    check(t, S["want"], S["bins"], S["hits"].hit_locus, True, keep=S["keep"], mass=m)       # (True: unique_mass and map_mass exactly)


def test_host_table_equals_the_restatement(S):
    with Handle(S["annot"], S["hits"], S["compat"], S["key"]) as H:
        t = context.context_table_host(H.h, S["compat"], F=S["F"], keep=S["keep"], status=S["status"])
    check_arrays(t, S["bins"], arrays_by_hand(S["bins"], S["compat"], S["F"], S["keep"], S["status"]))
    assert t.n_rows > 2 * R.SCAN_ROUND
