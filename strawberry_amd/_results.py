"""What the wrappers of the retained-result stages share (context.py, assign.py, coverage.py, fit.py, bootstrap.py):
the holder of a stage's results, the device-address and tensor checks of the device forms' arguments, and the coercion and
length check of the host forms' arrays."""
import ctypes as C

import numpy as np

from . import _lib


class Results:
    """Named host arrays beside a ctypes struct that has a pointer `name` and a device pointer `d_name` for each.
    A subclass sets STRUCT and calls _arrays({name: (entries, dtype)}, want) -- want: the names to bring to the host (None:
    all); the others are None and nothing is copied for them.  .device: name -> device address of the context's copy."""
    STRUCT = None

    def _arrays(self, sizes, want):
        unknown = set(want or ()) - set(sizes)
        if unknown:
            raise ValueError("%s: unknown arrays %s" % (type(self).__name__, sorted(unknown)))
        self._sizes = sizes
        for k, (n, dt) in sizes.items():
            setattr(self, k, np.zeros(max(n, 1), dt) if want is None or k in want else None)
        self.device = {}

    def _struct(self):
        s = self.STRUCT()
        for k in self._sizes:
            a = getattr(self, k)
            setattr(s, k, None if a is None else a.ctypes.data)
        return s

    def _finish(self, s):
        for k, (n, _) in self._sizes.items():
            a = getattr(self, k)
            if a is not None:
                setattr(self, k, a[:n])
            p = getattr(s, "d_" + k)
            if p:
                self.device[k] = int(p)
        return self


def bins_info(L, handle):
    """sbgpu_bins_info's eight numbers: n_loci, n_iso, n_bins, n_elem, ..."""
    info = (C.c_int64 * 8)()
    _lib.check(L.sbgpu_bins_info(handle, info), "sbgpu_bins_info")
    return [int(x) for x in info]


def addr(x):
    """a torch tensor's, or a plain device address; None stays None"""
    return None if x is None else (int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


def check_tensors(who, **tensors):
    """name=(x, "torch.<dtype>"): x where it is a tensor (not None, not an address) is contiguous, of that dtype, on a device"""
    for name, (x, dt) in tensors.items():
        if hasattr(x, "data_ptr") and (str(x.dtype) != dt or not x.is_cuda or not x.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous %s tensor on the context's device" % (who, name, dt))


def as_array(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


def ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def check_lengths(who, *named):
    """(name, array or None, entries needed), ..."""
    for name, a, n in named:
        if a is not None and a.size < n:
            raise ValueError("%s: %s holds %d entries, %d are needed" % (who, name, a.size, n))
