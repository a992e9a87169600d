"""The bin-table merge (include/sbgpu.h: sbgpu_bins_merge_*) restated in plain Python -- a dict from key tuple to
row, list appends, numpy fancy indexing; no call into the library -- and the key sets the tests merge: distinct random keys
per locus, a second sample made of a kept part, fresh rows and a permutation, and the adversarial sets (keys equal in all but
one word, swapped pairs, keys that all land in one slot of the deep form's table)."""
import numpy as np

MAX_BINS = 5632


class Sample:
    """iso_off, row_off [n_loci + 1]; key [n_bins, key_words] uint32; count [n_bins] int32; F [n_elem]; X [n_elem of the other] or None"""

    def __init__(self, iso_off, row_off, key, count, F, X=None):
        self.iso_off, self.row_off = np.asarray(iso_off, np.int64), np.asarray(row_off, np.int64)
        self.key = np.ascontiguousarray(key, np.uint32)
        assert self.key.ndim == 2 and len(self.key) == int(self.row_off[-1])
        self.key_words = self.key.shape[1]
        self.count, self.F = np.ascontiguousarray(count, np.int32), np.ascontiguousarray(F, np.float64)
        self.X = None if X is None else np.ascontiguousarray(X, np.float64)
        self.n_loci = len(self.iso_off) - 1
        niso, nb = np.diff(self.iso_off), np.diff(self.row_off)
        self.f_off = np.concatenate([[0], np.cumsum(nb * niso)]).astype(np.int64)
        assert len(self.count) == int(self.row_off[-1]) and len(self.F) == int(self.f_off[-1])

    def without_X(self):
        return Sample(self.iso_off, self.row_off, self.key, self.count, self.F)


def by_hand(a, b):
    """-> dict: row_off, f_off, row_a, row_b, count_a, count_b, F_a, F_b of the merge of Samples a and b"""
    assert a.n_loci == b.n_loci and (a.iso_off == b.iso_off).all() and a.key_words == b.key_words
    row_off, f_off, row_a, row_b, F_a, F_b = [0], [0], [], [], [], []
    Xa, Xb = (b.F if a.X is None else a.X), (a.F if b.X is None else b.X)
    assert len(Xa) == len(b.F) and len(Xb) == len(a.F)
    for l in range(a.n_loci):
        a0, a1, b0, b1 = int(a.row_off[l]), int(a.row_off[l + 1]), int(b.row_off[l]), int(b.row_off[l + 1])
        K = int(a.iso_off[l + 1] - a.iso_off[l])
        where_b = {tuple(b.key[i]): i for i in range(b0, b1)}
        assert len(where_b) == b1 - b0, "a duplicate key in B"
        ra, rb, seen = [], [], set()
        for i in range(a0, a1):
            k = tuple(a.key[i])
            assert k not in seen, "a duplicate key in A"
            seen.add(k)
            ra.append(i - a0), rb.append(where_b.get(k, b0 - 1) - b0)
        for i in range(b0, b1):
            if tuple(b.key[i]) not in seen:
                ra.append(-1), rb.append(i - b0)
        ra, rb = np.array(ra, np.int64), np.array(rb, np.int64)
        nu = len(ra)
        Fa, Fb = a.F[a.f_off[l]:a.f_off[l + 1]].reshape(a1 - a0, K), b.F[b.f_off[l]:b.f_off[l + 1]].reshape(b1 - b0, K)
        Xal, Xbl = Xa[b.f_off[l]:b.f_off[l + 1]].reshape(b1 - b0, K), Xb[a.f_off[l]:a.f_off[l + 1]].reshape(a1 - a0, K)
        oa, ob = np.zeros((nu, K)), np.zeros((nu, K))
        oa[ra >= 0], oa[ra < 0] = Fa[ra[ra >= 0]], Xal[rb[ra < 0]]
        ob[rb >= 0], ob[rb < 0] = Fb[rb[rb >= 0]], Xbl[ra[rb < 0]]
        F_a.append(oa.reshape(-1)), F_b.append(ob.reshape(-1))
        row_a.append(np.where(ra >= 0, ra + a0, -1)), row_b.append(np.where(rb >= 0, rb + b0, -1))
        row_off.append(row_off[-1] + nu), f_off.append(f_off[-1] + nu * K)
    cat = lambda v, dt: np.concatenate(v + [np.zeros(0, dt)]).astype(dt)  # noqa: E731
    row_a, row_b = cat(row_a, np.int32), cat(row_b, np.int32)
    count_a = np.where(row_a >= 0, np.concatenate([a.count, [0]])[row_a], 0).astype(np.int32)
    count_b = np.where(row_b >= 0, np.concatenate([b.count, [0]])[row_b], 0).astype(np.int32)
    return dict(row_off=np.array(row_off, np.int64), f_off=np.array(f_off, np.int64), row_a=row_a, row_b=row_b, count_a=count_a, count_b=count_b,
                F_a=cat(F_a, np.float64), F_b=cat(F_b, np.float64))


def assert_same(t, want, label=""):
    """a merge.MergedBins against by_hand's dict: integers and doubles bit for bit"""
    for k in ("row_off", "f_off", "row_a", "row_b", "count_a", "count_b"):
        np.testing.assert_array_equal(getattr(t, k), want[k], err_msg="%s %s" % (label, k))
    for k in ("F_a", "F_b"):
        np.testing.assert_array_equal(getattr(t, k).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (label, k))


# ---- key sets

def distinct_keys(rng, n, key_words):
    """n distinct keys of key_words words; the words are small, so that single words repeat across keys"""
    seen, out = set(), []
    top = 1 << 30 if key_words == 1 else max(40, 4 * int(np.ceil(n ** (1.0 / key_words))))
    while len(out) < n:
        k = tuple(int(x) for x in rng.integers(0, top, key_words))
        if k not in seen:
            seen.add(k), out.append(k)
    return np.array(out, np.uint32).reshape(n, key_words)


def sample_of_batch(batch, key_words, seed):
    """A golden batch as sample A: distinct random keys per locus"""
    rng = np.random.default_rng(seed)
    keys = [distinct_keys(rng, int(n), key_words) for n in np.diff(batch.row_off)]
    return Sample(batch.iso_off, batch.row_off, np.concatenate(keys + [np.zeros((0, key_words), np.uint32)]), batch.count, batch.F)


def second_sample(a, seed, keep=0.6, fresh=0.5):
    """(A with X, B with X): B keeps a random part of A's rows (shared) under another law (F * 1.3), drops the rest (A-only), adds
    fresh-keyed rows (B-only) and permutes its order.  The X arrays are random: a mix-up of F and X shows."""
    rng = np.random.default_rng(seed)
    row_off, keys, count, F = [0], [], [], []
    for l in range(a.n_loci):
        a0, a1, K = int(a.row_off[l]), int(a.row_off[l + 1]), int(a.iso_off[l + 1] - a.iso_off[l])
        Fa = a.F[a.f_off[l]:a.f_off[l + 1]].reshape(a1 - a0, K)
        shared = np.flatnonzero(rng.random(a1 - a0) < keep)
        n_new = min(int(rng.binomial(max(a1 - a0, 2), fresh)), MAX_BINS - (a1 - a0))
        have = set(tuple(k) for k in a.key[a0:a1])
        new = []
        while len(new) < n_new:
            k = tuple(int(x) for x in rng.integers(1 << 20, 1 << 30, a.key_words))
            if k not in have:
                have.add(k), new.append(k)
        kl = np.concatenate([a.key[a0:a1][shared], np.array(new, np.uint32).reshape(n_new, a.key_words)])
        Fl = np.concatenate([Fa[shared] * 1.3, rng.random((n_new, K)) * (rng.random((n_new, K)) < 0.7)])
        order = rng.permutation(len(kl))
        keys.append(kl[order]), F.append(Fl[order].reshape(-1)), count.append(rng.integers(0, 50, len(kl)))
        row_off.append(row_off[-1] + len(kl))
    b = Sample(a.iso_off, row_off, np.concatenate(keys + [np.zeros((0, a.key_words), np.uint32)]), np.concatenate(count + [np.zeros(0, np.int64)]),
               np.concatenate(F + [np.zeros(0)]))
    return (Sample(a.iso_off, a.row_off, a.key, a.count, a.F, rng.random(len(b.F)) + 2.0), Sample(b.iso_off, b.row_off, b.key, b.count, b.F, rng.random(len(a.F)) + 4.0))


def key_hash(key):
    """rule 6's hash of every key [n, key_words], restated"""
    k = np.asarray(key, np.uint64)
    h = np.full(len(k), 0x811C9DC5, np.uint64)
    for w in range(k.shape[1]):
        h = ((h ^ k[:, w]) * np.uint64(0x01000193)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(15))


def adversarial_keys(kind, n, key_words, rng, table_slots=None):
    """n distinct keys [n, key_words] of one kind: `last` equal in all but the last word, `first` equal in all but the first,
    `swapped` (key_words 2): the pairs (u, v) and (v, u), `collide`: all in one slot of a table of table_slots slots"""
    if kind in ("last", "first"):
        k = np.full((n, key_words), 0xABCD1234, np.uint32)
        k[:, -1 if kind == "last" else 0] = rng.permutation(4 * n)[:n] + 1
        return k
    if kind == "swapped":
        assert key_words == 2 and n % 2 == 0
        u = rng.permutation(8 * n)[:n].reshape(n // 2, 2) + 1
        return np.concatenate([u, u[:, ::-1]]).astype(np.uint32)[rng.permutation(n)]
    assert kind == "collide" and table_slots
    out = np.zeros((0, key_words), np.uint32)
    while len(out) < n:
        k = rng.integers(0, 1 << 32, (n * table_slots // 2, key_words), dtype=np.uint64).astype(np.uint32)
        k = k[(key_hash(k) & np.uint64(table_slots - 1)) == 5]
        out = np.unique(np.concatenate([out, k]), axis=0)
    return out[rng.permutation(len(out))[:n]]


def one_locus_pair(keys_a, keys_b, K, rng, with_X=True):
    """two single-locus Samples of K isoforms with the given keys"""
    na, nb = len(keys_a), len(keys_b)
    a = Sample([0, K], [0, na], keys_a, rng.integers(0, 90, na), rng.random(na * K) + 1.0, rng.random(nb * K) + 2.0 if with_X else None)
    b = Sample([0, K], [0, nb], keys_b, rng.integers(0, 90, nb), rng.random(nb * K) + 3.0, rng.random(na * K) + 4.0 if with_X else None)
    return a, b


def split_keys(keys, n_shared, n_a_only, rng):
    """a key set cut into A's keys (shared + A-only) and B's (shared + the rest), each in an order of its own"""
    shared, only_a, only_b = keys[:n_shared], keys[n_shared:n_shared + n_a_only], keys[n_shared + n_a_only:]
    ka, kb = np.concatenate([shared, only_a]), np.concatenate([shared, only_b])
    return ka[rng.permutation(len(ka))], kb[rng.permutation(len(kb))]


def concat(pairs):
    """[(a, b), ...] single- or multi-locus Sample pairs of one key width -> one pair over all their loci"""
    out = []
    for s in (0, 1):
        xs = [p[s] for p in pairs]
        others = [p[1 - s] for p in pairs]
        cat_off = lambda offs: np.concatenate([[0]] + [np.diff(o) for o in offs]).cumsum()  # noqa: E731
        X = None if any(x.X is None for x in xs) else np.concatenate([x.X for x in xs])
        assert X is None or len(X) == sum(len(o.F) for o in others)
        out.append(Sample(cat_off([x.iso_off for x in xs]), cat_off([x.row_off for x in xs]), np.concatenate([x.key for x in xs]),
                          np.concatenate([x.count for x in xs]), np.concatenate([x.F for x in xs]), X))
    return tuple(out)
