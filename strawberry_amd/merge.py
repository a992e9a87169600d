"""Two samples on ONE bin table: the union of their bins by key, zero counts where a sample saw nothing, and -- where a sample
lacks a bin -- the other sample's bin weighed under this sample's insert-size law (include/sbgpu.h states the rule under
sbgpu_bins_merge_*).  The merged tables are inputs of the unchanged differential-usage rule (diff.py).

Sample         one sample's arrays: iso_off, row_off (host), key [n_bins * key_words] uint32, count int32, F float64, X or None
merge_host     the two host calls (shapes, fill)
merge_device   sbgpu_bins_merge_device: key, count, F, X in HBM (torch tensors or device addresses)
limits         the kernels' thresholds by name

Both return a MergedBins.  ChainQuantifier / FrontQuantifier(keep_bootstrap=True).differential_usage(other, shared_bins=True)
merges two retained samples and tests them (diff.model_diff_merged_device).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, check_lengths, check_tensors, ptr

NAMES = _lib.sbgpu_bins_merged_t._NAMES
DTYPES = dict(row_a=np.int32, row_b=np.int32, count_a=np.int32, count_b=np.int32, F_a=np.float64, F_b=np.float64)
PER_ELEM = ("F_a", "F_b")
LIMIT_NAMES = ("group_max_bins", "table_slots", "max_bins", "tile_vals", "tile_rows", "threads", "grid_per_cu", "reg_words")


def limits():
    """The thresholds (csrc/merge_rules.h, csrc/merge_device.h) by name: see sbgpu_bins_merge_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_bins_merge_limits(out), "sbgpu_bins_merge_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


class Sample:
    """One sample of a merge.  key_words: None takes it from key's second dimension."""

    def __init__(self, iso_off, row_off, key, count, F, X=None, key_words=None):
        self.iso_off, self.row_off, self.key, self.count, self.F, self.X = iso_off, row_off, key, count, F, X
        self.key_words = int(key_words if key_words is not None else np.shape(key)[1])


class MergedBins(Results):
    """row_off, f_off (int64) [n_loci + 1]: the union's offsets; row_a, row_b (int32) [n_bins]: each union row's global bin in A
    and in B, or -1; count_a, count_b (int32) [n_bins]; F_a, F_b (float64) [n_elem].
    want: the names to bring to the host (None: all) -- the device form copies nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device form; valid until its next quantify / merge call)."""
    STRUCT = _lib.sbgpu_bins_merged_t

    def __init__(self, iso_off, want=None):
        unknown = set(want or ()) - set(NAMES)
        if unknown:
            raise ValueError("MergedBins: unknown arrays %s" % sorted(unknown))
        self.iso_off = np.ascontiguousarray(iso_off, np.int64)
        self.n_loci = len(self.iso_off) - 1
        self.want = tuple(NAMES) if want is None else tuple(want)
        self.row_off, self.f_off = np.zeros(self.n_loci + 1, np.int64), np.zeros(self.n_loci + 1, np.int64)
        self.n_bins = self.n_elem = 0
        self.device = {}
        for k in NAMES:
            setattr(self, k, None)

    def _struct(self):
        s = self.STRUCT()
        s.row_off, s.f_off = self.row_off.ctypes.data, self.f_off.ctypes.data
        return s

    def _sized(self, n_bins, n_elem):
        """the sizes are known: the wanted arrays (one spare entry, so that an empty one still has an address)"""
        self.n_bins, self.n_elem = int(n_bins), int(n_elem)
        for k in self.want:
            setattr(self, k, np.zeros((self.n_elem if k in PER_ELEM else self.n_bins) + 1, DTYPES[k]))
        return [None if getattr(self, k) is None else getattr(self, k).ctypes.data for k in NAMES]

    def _finish(self, s=None):
        for k in self.want:
            setattr(self, k, getattr(self, k)[:self.n_elem if k in PER_ELEM else self.n_bins])
        if s is not None:
            self.device = {k: int(getattr(s, "d_" + k)) for k in NAMES if getattr(s, "d_" + k)}
        return self

    def fetch(self, ctx, s, stream=None):
        """sizes first, then fill: the wanted arrays of the device result `s` come to the host"""
        ptrs = self._sized(s.n_bins, s.n_elem)
        _lib.check(ctx.L.sbgpu_bins_merge_fetch(ctx.h, C.byref(s), *ptrs, stream), "sbgpu_bins_merge_fetch")
        return self._finish(s)

    def batches(self):
        """-> (A, B): the merged tables as two synth.LocusBatch (row_off, iso_off, f_off, count, F) of the differential rule"""
        from .synth import LocusBatch
        length = np.full(int(self.iso_off[-1]), 1000, np.int32)
        return tuple(LocusBatch(self.row_off, self.iso_off, self.f_off, getattr(self, "count_" + x), getattr(self, "F_" + x), length, "merged_" + x)
                     for x in "ab")


def _struct_of(sample, who, device):
    """-> (sbgpu_merge_sample_t, what it points into)"""
    iso_off, row_off = np.ascontiguousarray(sample.iso_off, np.int64), np.ascontiguousarray(sample.row_off, np.int64)
    if iso_off.size < 1 or row_off.size != iso_off.size:
        raise ValueError("%s: row_off and iso_off hold n_loci + 1 entries" % who)
    if device:
        check_tensors(who, key=(sample.key, "torch.int32"), count=(sample.count, "torch.int32"), F=(sample.F, "torch.float64"), X=(sample.X, "torch.float64"))
        hold = (iso_off, row_off, sample.key, sample.count, sample.F, sample.X)
        p = [addr(x) for x in hold[2:]]
    else:
        key, count = as_array(sample.key, np.uint32), as_array(sample.count, np.int32)
        F, X = as_array(sample.F, np.float64), as_array(sample.X, np.float64)
        n_bins = int(row_off[-1])
        n_elem = int(((row_off[1:] - row_off[:-1]) * (iso_off[1:] - iso_off[:-1])).sum())
        check_lengths(who, ("key", key, n_bins * max(sample.key_words, 0)), ("count", count, n_bins), ("F", F, n_elem))
        hold = (iso_off, row_off, key, count, F, X)
        p = [ptr(x) for x in hold[2:]]
    return _lib.sbgpu_merge_sample_t(iso_off.size - 1, iso_off.ctypes.data, row_off.ctypes.data, sample.key_words, 0, *p), hold


def merge_host(sample_a, sample_b, want=None):
    """The merge of two Samples on the host -> MergedBins"""
    L = _lib.load()
    (a, hold_a), (b, hold_b) = _struct_of(sample_a, "merge_host", False), _struct_of(sample_b, "merge_host", False)
    if hold_a[4] is not None and hold_b[5] is not None:
        check_lengths("merge_host", ("X of sample B", hold_b[5], hold_a[4].size))
    if hold_b[4] is not None and hold_a[5] is not None:
        check_lengths("merge_host", ("X of sample A", hold_a[5], hold_b[4].size))
    t = MergedBins(hold_a[0], want)
    sizes = (C.c_int64 * 2)()
    _lib.check(L.sbgpu_bins_merge_shapes_host(C.byref(a), C.byref(b), sizes, *([None] * 4)), "sbgpu_bins_merge_shapes_host")
    p = dict(zip(NAMES, t._sized(sizes[0], sizes[1])))
    _lib.check(L.sbgpu_bins_merge_shapes_host(C.byref(a), C.byref(b), sizes, t.row_off.ctypes.data, t.f_off.ctypes.data, p["row_a"], p["row_b"]),
               "sbgpu_bins_merge_shapes_host")
    if any(p[k] for k in ("count_a", "count_b", "F_a", "F_b")):
        _lib.check(L.sbgpu_bins_merge_fill_host(C.byref(a), C.byref(b), p["count_a"], p["count_b"], p["F_a"], p["F_b"]), "sbgpu_bins_merge_fill_host")
    del hold_a, hold_b
    return t._finish()


def merge_device(ctx, sample_a, sample_b, stream=None, want=None):
    """sbgpu_bins_merge_device for two Samples whose key (int32 tensor holding the uint32 words), count, F and X are torch tensors
    on the context's device, or device addresses; iso_off and row_off are host arrays -> MergedBins"""
    (a, hold_a), (b, hold_b) = _struct_of(sample_a, "merge_device", True), _struct_of(sample_b, "merge_device", True)
    t = MergedBins(hold_a[0], want)
    s = t._struct()
    _lib.check(ctx.L.sbgpu_bins_merge_device(ctx.h, C.byref(a), C.byref(b), stream, C.byref(s)), "sbgpu_bins_merge_device")
    del hold_a, hold_b
    return t.fetch(ctx, s, stream)
