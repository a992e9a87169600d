"""Fragment assignment: which isoform every hit came from, and how sure that is (include/sbgpu.h states the rule).

fragment_assign_host    sbgpu_fragment_assign_host: the plain CPU statement, on a handle that holds hit -> bin
fragment_assign_device  sbgpu_fragment_assign_device: built in HBM from what a resident call kept
                        (sbgpu_context_table_keep; quantify_resident(with_assignment=True), ChainQuantifier / FrontQuantifier(keep_context=True))

Both forms return a FragmentAssignment.  map_iso is the index inside the hit's locus (-1: unassigned); the per-isoform sums are
laid out as theta is.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

PER_HIT = (("map_iso", np.int32), ("map_prob", np.float64), ("n_cand", np.int32))
PER_ISO = (("unique_mass", np.float64), ("map_mass", np.float64), ("post_mass", np.float64))


class FragmentAssignment(Results):
    """map_iso / map_prob / n_cand [n_hits]; unique_mass / map_mass / post_mass [n_iso]; unassigned [n_loci] (int64).
    want: the names to bring to the host (None: all) -- the device form copies nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device form; valid until its next quantify / assignment call)."""
    STRUCT = _lib.sbgpu_fragment_assign_t

    def __init__(self, n_hits, n_iso, n_loci, want=None):
        sizes = {k: (n_hits, dt) for k, dt in PER_HIT}
        sizes.update({k: (n_iso, dt) for k, dt in PER_ISO})
        sizes["unassigned"] = (n_loci, np.int64)
        self._arrays(sizes, want)
        self.n_hits = 0

    def _struct(self):
        s = super()._struct()
        s.n_hits = self._sizes["map_iso"][0]     # (the library refuses another count before it writes)
        return s

    def _finish(self, s):
        self.n_hits = int(s.n_hits)
        return super()._finish(s)


def fragment_assign_host(handle, compat, theta, F=None, keep=None, status=None, hit_mass=None, want=None):
    """handle: an sbgpu_bins_t that holds hit -> bin (sbgpu_bins_create, sbgpu_quantify_host); compat [n_hits, cw]: the hits'
    compat words; theta [n_iso]: the abundances the posterior is taken under; F: the bin weights (None: the handle's own);
    keep [n_iso] / status [n_loci] (None: all kept / all started); hit_mass [n_hits] float32 (None: 1.0 each)."""
    L = _lib.load()
    handle = getattr(handle, "h", handle)
    n_loci, n_iso = bins_info(L, handle)[:2]
    compat = np.ascontiguousarray(compat, np.uint32)
    cw = compat.shape[1] if compat.ndim == 2 else 1
    n_hits = compat.shape[0] if compat.ndim == 2 else compat.size
    theta, F, keep, status = as_array(theta, np.float64), as_array(F, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    hit_mass = as_array(hit_mass, np.float32)
    check_lengths("fragment_assign_host", ("theta", theta, n_iso), ("keep", keep, n_iso), ("status", status, n_loci), ("hit_mass", hit_mass, n_hits))
    t = FragmentAssignment(n_hits, n_iso, n_loci, want)
    s = t._struct()
    _lib.check(L.sbgpu_fragment_assign_host(handle, ptr(compat), cw, ptr(F), ptr(theta), ptr(keep), ptr(status), ptr(hit_mass), C.byref(s)),
               "sbgpu_fragment_assign_host")
    return t._finish(s)


def fragment_assign_device(ctx, handle, d_theta, n_hits, d_hit_mass=None, stream=None, want=None):
    """Right after a resident call made with retention on (sbgpu_context_table_keep), on its handle, before the context's next
    quantify call.  d_theta: a float64 torch tensor on the context's device, or a device address ([n_iso]; normally the call's
    own d_theta); n_hits: the call's hit count (it sizes the host arrays); d_hit_mass: float32 tensor / address of the masses the
    call was given, or None for unit masses."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    n_loci, n_iso = bins_info(L, handle)[:2]
    check_tensors("fragment_assign_device", d_theta=(d_theta, "torch.float64"), d_hit_mass=(d_hit_mass, "torch.float32"))
    t = FragmentAssignment(int(n_hits), n_iso, n_loci, want)
    s = t._struct()
    _lib.check(L.sbgpu_fragment_assign_device(ctx.h, handle, addr(d_theta), addr(d_hit_mass), stream, C.byref(s)), "sbgpu_fragment_assign_device")
    return t._finish(s)
