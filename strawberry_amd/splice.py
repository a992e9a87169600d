"""Splicing events: for every annotated exon and intron the share of the transcripts across it that include it (PSI), its
bootstrap interval and its read support (include/sbgpu.h states the rule).

SpliceEvents           the event table of an annotation (sbgpu_splice_events_build_host): built once per annotation, on the host;
                       .to_device(ctx) uploads it once, for every sample quantified against that annotation
splice_psi_host        sbgpu_splice_psi_host: PSI of every event for one or many abundance rows, plain CPU
splice_psi_device      sbgpu_splice_psi_device: the same bits from spl_psi_kernel, on device arrays as they stand
splice_support_host    sbgpu_splice_support_host: the events' support from the coverage's exon_bases / junction_mass
splice_support_device  sbgpu_splice_support_device: the same from spl_support_kernel
splice_psi             the composition behind quantify_resident(with_splicing=True) and ChainQuantifier.splice_psi(): PSI of a
                       resident call's FPKM / keep, the intervals from a bootstrap's replicates, the support from a coverage
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, check_tensors, ptr

FLAG_NAMES = ("FIRST", "LAST", "INTERNAL", "SKIPPED", "RETAINED")      # bit 0 .. 4 (include/sbgpu.h: SBGPU_SPLICE_*)
FIRST, LAST, INTERNAL, SKIPPED, RETAINED = 1, 2, 4, 8, 16
KIND_NAMES = ("exon", "intron")
LIMIT_NAMES = ("mask_iso", "threads")
_DTYPES = dict(event_off=np.int64, event_locus=np.int32, event_kind=np.uint8, event_left=np.uint32, event_right=np.uint32, event_flags=np.uint8,
               n_span=np.int32, incl_off=np.int64, incl_iso=np.int32, incl_exon=np.int64, iso_off=np.int64, iso_left=np.uint32, iso_right=np.uint32)


def limits():
    """spl_psi_kernel's threshold and workgroup (csrc/splice_device.h) by name: see sbgpu_splice_limits."""
    out = (C.c_int64 * 2)()
    _lib.check(_lib.load().sbgpu_splice_limits(out), "sbgpu_splice_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def flag_words(flags):
    """the flag bits of one event as words: 9 -> "FIRST|SKIPPED"; 0 -> "-" """
    return "|".join(n for b, n in enumerate(FLAG_NAMES) if int(flags) >> b & 1) or "-"


class SpliceEvents:
    """The event table: the arrays of sbgpu_splice_events_t by name (host arrays), n_loci / n_iso / n_exons / n_events / n_incl."""
    NAMES = _lib.sbgpu_splice_events_t._NAMES

    @classmethod
    def build(cls, annot):
        """annot: an exonbin.Annotation (or anything with its _struct())"""
        L = _lib.load()
        a = annot if isinstance(annot, _lib.sbgpu_annotation_t) else annot._struct()
        shape = (C.c_int64 * 2)()
        _lib.check(L.sbgpu_splice_events_shapes_host(C.byref(a), shape), "sbgpu_splice_events_shapes_host")
        t = cls()
        t.n_loci = int(a.n_loci)
        iso_off = np.ctypeslib.as_array(C.cast(a.iso_off, C.POINTER(C.c_int64)), shape=(t.n_loci + 1,))
        t.n_iso, t.n_events, t.n_incl = int(iso_off[-1]), int(shape[0]), int(shape[1])
        sizes = dict(event_off=t.n_loci + 1, incl_off=t.n_events + 1, incl_iso=t.n_incl, incl_exon=t.n_incl, iso_off=t.n_loci + 1, iso_left=t.n_iso,
                     iso_right=t.n_iso)
        for k in cls.NAMES:
            setattr(t, k, np.zeros(sizes.get(k, t.n_events), _DTYPES[k]))
        s = t._struct()
        _lib.check(L.sbgpu_splice_events_build_host(C.byref(a), C.byref(s)), "sbgpu_splice_events_build_host")
        t.n_exons = int(s.n_exons)
        return t

    def _struct(self):
        s = _lib.sbgpu_splice_events_t()
        for k in s._COUNTS:
            setattr(s, k, int(getattr(self, k, 0)))
        for k in self.NAMES:
            a = getattr(self, k)
            setattr(s, k, a.ctypes.data if a.size else None)
        return s

    @property
    def n_incl_of(self):
        """entries of every event's inclusion list [n_events]"""
        return np.diff(self.incl_off).astype(np.int32)

    def alternative(self):
        """the events that are not constitutive within their span: n_incl != n_span"""
        return self.n_incl_of != self.n_span

    def census(self):
        f = self.event_flags
        return {"events": self.n_events, "exon_events": int((self.event_kind == 0).sum()), "intron_events": int((self.event_kind == 1).sum()),
                "alternative": int(self.alternative().sum()), "skipped": int((f & SKIPPED != 0).sum()), "retained": int((f & RETAINED != 0).sum())}

    def to_device(self, ctx):
        """Upload once, reuse across samples -> DeviceSpliceEvents (torch owns the copies)."""
        return DeviceSpliceEvents(ctx, self)

    def rows(self, names=None):
        """-> (locus, kind, left, right, flags as words, n_incl, n_span) per event, for a TSV; names: the loci's names"""
        n_incl = self.n_incl_of
        for u in range(self.n_events):
            l = int(self.event_locus[u])
            yield (names[l] if names else l, KIND_NAMES[int(self.event_kind[u])], int(self.event_left[u]), int(self.event_right[u]),
                   flag_words(self.event_flags[u]), int(n_incl[u]), int(self.n_span[u]))


class DeviceSpliceEvents:
    """The table in HBM: .d name -> tensor, .struct the sbgpu_splice_events_t of their addresses, .host the SpliceEvents."""

    def __init__(self, ctx, events):
        import torch
        self.ctx, self.host = ctx, events
        self.dev = torch.device("cuda", ctx.device)
        view = {np.dtype(np.uint32): np.int32}      # (uint32 travels as its bit pattern)
        self.d = {k: torch.from_numpy(np.ascontiguousarray(getattr(events, k)).view(view.get(getattr(events, k).dtype, getattr(events, k).dtype))).to(self.dev)
                  for k in events.NAMES}
        self.struct = s = _lib.sbgpu_splice_events_t()
        for k in s._COUNTS:
            setattr(s, k, int(getattr(events, k)))
        for k, t in self.d.items():
            setattr(s, k, t.data_ptr() if t.numel() else None)
        for k in s._COUNTS:
            setattr(self, k, int(getattr(events, k)))


class SplicePsi(Results):
    """psi [n_events] (float64; NaN where no kept spanning isoform has abundance).  With a bootstrap also mean / var / lo / hi
    [n_events], defined_count [n_events] (int32: replicates in which the event was defined) and -- asked for -- rep [n_rep, n_events];
    with a coverage also support [n_events].  What was not computed is None.  .events: the SpliceEvents."""
    OPTIONAL = ("mean", "var", "lo", "hi", "defined_count", "rep", "support")

    def __init__(self, events, psi, **more):
        self.events = events
        self._arrays({"psi": (events.n_events, np.float64)}, None)
        self.psi = np.asarray(psi, np.float64).reshape(-1)[:events.n_events]
        unknown = set(more) - set(self.OPTIONAL) - {"rank_lo", "rank_hi", "n_rep"}
        if unknown:
            raise ValueError("SplicePsi: unknown arrays %s" % sorted(unknown))
        for k in self.OPTIONAL + ("rank_lo", "rank_hi", "n_rep"):
            setattr(self, k, more.get(k))

    def alternative(self):
        return self.events.alternative()

    def rows(self, names=None):
        """-> the table's (locus, kind, left, right, flags, n_incl, n_span), then psi, then -- where computed -- mean, var, lo, hi,
        defined_count, and support, per event, for a TSV"""
        extra = [k for k in ("mean", "var", "lo", "hi", "defined_count", "support") if getattr(self, k) is not None]
        for u, row in enumerate(self.events.rows(names)):
            yield row + (float(self.psi[u]),) + tuple(int(getattr(self, k)[u]) if k == "defined_count" else float(getattr(self, k)[u]) for k in extra)

    def header(self):
        return ("locus", "kind", "left", "right", "flags", "n_incl", "n_span", "psi") + tuple(
            k for k in ("mean", "var", "lo", "hi", "defined_count", "support") if getattr(self, k) is not None)


def _host_table(events):
    return events.host if isinstance(events, DeviceSpliceEvents) else events


def splice_psi_host(events, x, keep=None):
    """x: [n_iso] or [n_rows, n_iso] (float64); keep: the same shape (int32; None: every isoform enters)
    -> (psi [n_rows, n_events] float64, defined_count [n_events] int32)"""
    L = _lib.load()
    x = np.ascontiguousarray(x, np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    keep = as_array(keep, np.int32)
    if x.ndim != 2 or x.shape[1] != events.n_iso or (keep is not None and keep.size != x.size):
        raise ValueError("splice_psi_host: x must be [n_rows, n_iso] and keep of the same shape")
    n_rows = x.shape[0]
    psi = np.zeros((n_rows, events.n_events), np.float64)
    defined = np.zeros(events.n_events, np.int32)
    s = events._struct()
    _lib.check(L.sbgpu_splice_psi_host(C.byref(s), n_rows, ptr(x), ptr(keep), ptr(psi), ptr(defined)), "sbgpu_splice_psi_host")
    return psi, defined


def splice_support_host(events, exon_bases=None, junction_mass=None):
    """exon_bases / junction_mass: [n_exons] (float64), either may be None -> support [n_events]"""
    L = _lib.load()
    xb, jm = as_array(exon_bases, np.float64), as_array(junction_mass, np.float64)
    for name, a in (("exon_bases", xb), ("junction_mass", jm)):
        if a is not None and a.size < events.n_exons:
            raise ValueError("splice_support_host: %s holds %d entries, %d are needed" % (name, a.size, events.n_exons))
    out = np.zeros(events.n_events, np.float64)
    s = events._struct()
    _lib.check(L.sbgpu_splice_support_host(C.byref(s), None if xb is None else xb.ctypes.data, None if jm is None else jm.ctypes.data, ptr(out)),
               "sbgpu_splice_support_host")
    return out


def _stream(ctx, stream):
    import torch
    return torch.cuda.current_stream(torch.device("cuda", ctx.device)).cuda_stream if stream is None else stream


def splice_psi_device(ctx, d_events, x, keep=None, n_rows=None, stream=None):
    """d_events: a DeviceSpliceEvents; x (float64) / keep (int32; None: every isoform enters): torch tensors [n_iso] or
    [n_rows, n_iso] on the context's device, or plain device addresses with n_rows given (the d_fpkm / d_keep of a resident
    call, the d_fpkm_rep / d_keep_rep of a bootstrap).  -> (psi [n_rows, n_events], defined_count [n_events]): device tensors,
    queued on `stream` (default: torch's current one), not synchronised."""
    import torch
    check_tensors("splice_psi_device", x=(x, "torch.float64"), keep=(keep, "torch.int32"))
    if hasattr(x, "data_ptr"):
        rows = 1 if x.dim() == 1 else int(x.shape[0])
        if x.numel() != rows * d_events.n_iso or (hasattr(keep, "data_ptr") and keep.numel() != x.numel()):
            raise ValueError("splice_psi_device: x must be [n_rows, n_iso] and keep of the same shape")
        n_rows = rows
    elif n_rows is None:
        raise ValueError("splice_psi_device: n_rows is needed with a device address")
    n_rows = int(n_rows)
    nu = d_events.n_events
    psi = torch.empty((n_rows, nu), dtype=torch.float64, device=d_events.dev)
    defined = torch.zeros(nu, dtype=torch.int32, device=d_events.dev)
    _lib.check(ctx.L.sbgpu_splice_psi_device(ctx.h, C.byref(d_events.struct), n_rows, addr(x) if n_rows and d_events.n_iso else None, addr(keep),
                                             psi.data_ptr() if psi.numel() else None, defined.data_ptr() if nu else None, _stream(ctx, stream)),
               "sbgpu_splice_psi_device")
    return psi, defined


def splice_support_device(ctx, d_events, d_exon_bases=None, d_junction_mass=None, stream=None):
    """d_exon_bases / d_junction_mass: float64 tensors or device addresses [n_exons] (a coverage's .device entries), either may
    be None -> support [n_events], a device tensor queued on `stream`, not synchronised."""
    import torch
    check_tensors("splice_support_device", d_exon_bases=(d_exon_bases, "torch.float64"), d_junction_mass=(d_junction_mass, "torch.float64"))
    out = torch.zeros(d_events.n_events, dtype=torch.float64, device=d_events.dev)
    _lib.check(ctx.L.sbgpu_splice_support_device(ctx.h, C.byref(d_events.struct), addr(d_exon_bases), addr(d_junction_mass),
                                                 out.data_ptr() if out.numel() else None, _stream(ctx, stream)), "sbgpu_splice_support_device")
    return out


def as_device_events(ctx, events, annot=None):
    """events: a DeviceSpliceEvents, a SpliceEvents (uploaded here), or None / True (built from annot and uploaded here)"""
    if isinstance(events, DeviceSpliceEvents):
        return events
    if events is None or events is True:
        events = SpliceEvents.build(annot)
    if not isinstance(events, SpliceEvents):
        raise ValueError("splicing events: a SpliceEvents, a DeviceSpliceEvents, True or None is needed")
    return events.to_device(ctx)


def splice_psi(ctx, d_events, d_fpkm, d_keep, bootstrap=None, coverage=None, replicates=False):
    """PSI of one resident call: d_fpkm / d_keep are its device arrays (addresses or tensors, [n_iso]).
    bootstrap: the dict of bootstrap.abundance_bootstrap_device run on that call's handle (its "device" entry names d_fpkm_rep /
    d_keep_rep, valid until the context's next bootstrap or quantify call): PSI per replicate, then sbgpu_replicate_stats_device
    at the bootstrap's ranks -> mean, var, lo, hi, defined_count (and rep with replicates=True).
    coverage: a coverage.IsoformCoverage of the device form (its .device names exon_bases / junction_mass) -> support.
    -> a SplicePsi of host arrays; synchronises torch's current stream."""
    import torch
    dev = d_events.dev
    nu = d_events.n_events
    if d_events.n_iso and not addr(d_fpkm):
        raise _lib.SbgpuError("splice_psi: no resident call's FPKM on the device")
    psi, _ = splice_psi_device(ctx, d_events, d_fpkm, d_keep, n_rows=1)
    more = {}
    if bootstrap is not None:
        where = bootstrap.get("device")
        if not where or not where.get("fpkm_rep") or not where.get("keep_rep"):
            raise _lib.SbgpuError("splice_psi: the bootstrap's replicates are not on the device")
        B = int(bootstrap["n_rep"])
        rep, defined = splice_psi_device(ctx, d_events, where["fpkm_rep"], where["keep_rep"], n_rows=B)
        stats = {k: torch.zeros(max(nu, 1), dtype=torch.float64, device=dev) for k in ("mean", "var", "lo", "hi")}
        if nu:
            _lib.check(ctx.L.sbgpu_replicate_stats_device(ctx.h, B, nu, rep.data_ptr(), int(bootstrap["rank_lo"]), int(bootstrap["rank_hi"]),
                                                          *(stats[k].data_ptr() for k in ("mean", "var", "lo", "hi")), _stream(ctx, None)),
                       "sbgpu_replicate_stats_device")
        more.update({k: v[:nu].cpu().numpy() for k, v in stats.items()})
        more.update(defined_count=defined.cpu().numpy(), rank_lo=int(bootstrap["rank_lo"]), rank_hi=int(bootstrap["rank_hi"]), n_rep=B)
        if replicates:
            more["rep"] = rep.cpu().numpy()
    if coverage is not None:
        where = getattr(coverage, "device", None) or {}
        if not where.get("exon_bases") or not where.get("junction_mass"):
            raise _lib.SbgpuError("splice_psi: the coverage's arrays are not on the device (give isoform_coverage_device's result)")
        more["support"] = splice_support_device(ctx, d_events, where["exon_bases"], where["junction_mass"]).cpu().numpy()
    return SplicePsi(d_events.host, psi.cpu().numpy(), **more)
