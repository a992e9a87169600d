"""Fragments -> abundances for a batch of loci: the device-resident chain behind
LocusContext's constructor + estimate_abundances (/root/reference/include/estimate.hpp:60-103,
src/estimate.cpp:279-355) as Sample::quantifyCluster drives them (src/alignments.cpp:1505-1546).

    hits --exonbin kernel--> compat/key words --host bookkeeping--> bins, counts, (bin, isoform) pairs
         --bin-weight kernel--> F (written straight into the EM batch) --EM kernels--> theta
         --epilogue kernels--> FPKM / Frac / TPM

torch holds the device buffers; every number is produced by libsbgpu.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from .binweight import InsertSize  # noqa: F401  (re-exported: the caller builds one)
from .em import EmBatchSolver, _torch, default_context
from .exonbin import LocusBins
from .synth import LocusBatch


class _LazyHitBin:
    """hit -> bin of the device grouping: stays in HBM until somebody asks for it as an array."""

    def __init__(self, d):
        self._d, self._h = d, None

    def __array__(self, dtype=None, copy=None):
        if self._h is None:
            self._h = self._d.cpu().numpy()
        return self._h if dtype is None else self._h.astype(dtype)

    def __getitem__(self, k):
        return np.asarray(self)[k]


class LocusQuantifier:
    def __init__(self, annot, hits, insert, read_len, long_read=False, ctx=None, device=0, device_bins=True):
        """device_bins: group the hits into bins on the GPU when the input allows it (sorted hits, whole-number
        masses; sbgpu_bins_create_device), else -- or when False -- on the host."""
        self.torch = torch = _torch()
        self.ctx = ctx or default_context(device)
        self.dev = torch.device("cuda", self.ctx.device)
        self.annot, self.hits = annot, hits
        self.insert, self.read_len, self.long_read = insert, int(read_len), bool(long_read)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
        # device copies of the kernel inputs (uint32 travels as int32 bit patterns)
        self._d = {k: up(getattr(annot, k).view(np.int32) if getattr(annot, k).dtype == np.uint32 else getattr(annot, k))
                   for k in ("iso_off", "exon_off", "exon_left", "exon_right", "seg_off", "seg_left", "seg_right")}
        self._d.update({k: up(getattr(hits, k).view(np.int32) if getattr(hits, k).dtype == np.uint32 else getattr(hits, k))
                        for k in ("hit_locus", "feat_off", "feat_code", "feat_left", "feat_right")})
        self._d["mass"] = up(hits.mass)
        self.device_bins = bool(device_bins)
        self.bins_on_device = False
        self.bins = None
        self.solver = None

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _p(self, name):
        t = self._d[name]
        return t.data_ptr() if t.numel() else None

    def assign_bins(self):
        """A5: kernel for the interval tests, then the host bookkeeping.  -> LocusBins"""
        torch, a, h = self.torch, self.annot, self.hits
        cw, kw = a.compat_words, a.key_words
        self.d_compat = torch.zeros((max(h.n_hits, 1), cw), dtype=torch.int32, device=self.dev)
        self.d_key = torch.zeros((max(h.n_hits, 1), kw), dtype=torch.int32, device=self.dev)
        an = _lib.sbgpu_annotation_t(a.n_loci, self._p("iso_off"), self._p("exon_off"), self._p("exon_left"),
                                     self._p("exon_right"), self._p("seg_off"), self._p("seg_left"), self._p("seg_right"))
        ht = _lib.sbgpu_hits_t(h.n_hits, self._p("hit_locus"), self._p("feat_off"), self._p("feat_code"),
                               self._p("feat_left"), self._p("feat_right"))
        _lib.check(self.ctx.L.sbgpu_exonbin_device(self.ctx.h, C.byref(an), C.byref(ht), cw, kw, self.d_compat.data_ptr(),
                                                   self.d_key.data_ptr(), self._stream()), "sbgpu_exonbin_device")
        self.bins = None
        if self.device_bins and h.n_hits:
            self.d_hit_bin = torch.zeros(h.n_hits, dtype=torch.int64, device=self.dev)
            self.bins = LocusBins.on_device(self.ctx, a, h, ht, self._p("mass"), cw, kw, self.d_compat.data_ptr(),
                                            self.d_key.data_ptr(), self.d_hit_bin.data_ptr(), self._stream())
            if self.bins is not None:
                self.bins.hit_bin = _LazyHitBin(self.d_hit_bin)
        self.bins_on_device = self.bins is not None
        if self.bins is None:   # host form: bring the words back
            compat = self.d_compat[:h.n_hits].cpu().numpy().view(np.uint32)
            key = self.d_key[:h.n_hits].cpu().numpy().view(np.uint32)
            self.bins = LocusBins(a, h, compat, key)
        return self.bins

    def bin_weights(self):
        """A4: one weight per (bin, isoform) pair, scattered into the EM batch's F on the device."""
        torch, b = self.torch, self.bins
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)  # noqa: E731
        self.d_F = torch.zeros(max(b.n_elem, 1), dtype=torch.float64, device=self.dev)
        if b.n_pairs == 0:
            return self.d_F
        if self.long_read:      # F = 1/L_j: neither the segments nor the pdf are looked at
            pdf = np.zeros(2, np.float64)
        else:
            span = np.diff(np.concatenate([[0], np.cumsum(b.pair_seg_lens.astype(np.int64))])[b.pair_seg_off])
            pdf = self.insert.pdf_table(int(span.max()) + 1, self.read_len)
        d_off, d_seg = up(b.pair_seg_off), up(b.pair_seg_lens.view(np.int32))
        d_mask, d_len = up(b.pair_implicit_mask.view(np.int32)), up(b.pair_iso_len)
        d_idx, d_pdf = up(b.pair_out_index), up(pdf)
        lmin_base = self.insert.start_offset if self.insert.use_emp else self.read_len
        _lib.check(self.ctx.L.sbgpu_binweight_device(
            self.ctx.h, b.n_pairs, d_off.data_ptr(), d_seg.data_ptr(), d_mask.data_ptr(), d_len.data_ptr(),
            d_idx.data_ptr(), d_pdf.data_ptr(), len(pdf), self.read_len, lmin_base, int(self.long_read),
            self.d_F.data_ptr(), self._stream()), "sbgpu_binweight_device")
        self.torch.cuda.current_stream(self.dev).synchronize()  # the inputs above go out of scope
        return self.d_F

    def solve(self, total_mapped_reads, **abundance_kw):
        """A1-A3, A7: EM + abundance epilogue + TPM over all loci.  -> results dict (host arrays)."""
        b = self.bins
        batch = LocusBatch(b.row_off, b.iso_off, b.f_off, b.count, None, b.iso_len, "hits")
        self.solver = s = EmBatchSolver(batch, self.ctx, d_F=self.d_F)
        s.run_em()
        s.run_abundance(total_mapped_reads, **abundance_kw)
        s.run_tpm()
        return s.results()

    def bootstrap(self, n_rep, seed, rep_first=0, locus_id=None, keep_replicates=False):
        """The EM bootstrap on the bins' counts and the weights the chain holds on the device (after assign_bins and
        bin_weights): EmBatchSolver.run_bootstrap on solve()'s batch -> its dict of device tensors.  locus_id: the loci's
        global ids where this annotation is a part of a sample."""
        if self.bins is None or getattr(self, "d_F", None) is None:
            raise _lib.SbgpuError("bootstrap: assign_bins() and bin_weights() come first")
        if self.solver is None or self.solver.d_F is not self.d_F:   # (solve() leaves one; new weights make it stale)
            b = self.bins
            self.solver = EmBatchSolver(LocusBatch(b.row_off, b.iso_off, b.f_off, b.count, None, b.iso_len, "hits"), self.ctx, d_F=self.d_F)
        return self.solver.run_bootstrap(n_rep, seed, rep_first=rep_first, locus_id=locus_id, keep_replicates=keep_replicates)

    def run(self, total_mapped_reads, **abundance_kw):
        self.assign_bins()
        self.bin_weights()
        return self.solve(total_mapped_reads, **abundance_kw)


def quantify_host(annot, hits, insert, read_len, long_read=False, ctx=None, device=0, context_keep=None, context_status=None,
                  assignment_theta=None, assignment_keep=None, assignment_status=None):
    """sbgpu_quantify_host: the whole chain as one C-ABI call on host arrays (what a C / C++ driver uses).
    insert=None: build the empirical insert-size distribution from the hits.
    context_keep (per isoform, from the caller's epilogue; context_status: the EM's per locus, default this call's): also the
    `-f` table's arrays from the handle, through the host form (context.context_table_host) -> "context".
    assignment_theta (per isoform; True: this call's theta), with assignment_keep / assignment_status (default: all kept / this
    call's status): also every hit's isoform posterior through the host form (assign.fragment_assign_host, under the hits' own
    masses) -> "assignment".
    -> dict(theta, status, iters, compat, bins (LocusBins incl. hit_bin), F, insert (mean, sd, use_emp, ...))"""
    from .exonbin import LocusBins
    ctx = ctx or default_context(device)
    L = ctx.L
    a, h = annot._struct(), hits._struct()
    n_iso = int(annot.iso_off[-1])
    theta = np.zeros(n_iso + 1, np.float64)
    status = np.zeros(annot.n_loci + 1, np.int32)
    iters = np.zeros(annot.n_loci + 1, np.int32)
    cw, kw = annot.compat_words, annot.key_words
    compat = np.zeros((max(hits.n_hits, 1), cw), np.uint32)
    used = _lib.sbgpu_insert_t()
    ins = insert._struct(read_len, long_read) if insert is not None else None
    handle = C.c_void_p()
    _lib.check(L.sbgpu_quantify_host(ctx.h, C.byref(a), C.byref(h), hits.mass.ctypes.data if hits.n_hits else None,
                                     C.byref(ins) if ins is not None else None, int(read_len), int(long_read),
                                     theta.ctypes.data, status.ctypes.data, iters.ctypes.data, compat.ctypes.data,
                                     C.byref(used), C.byref(handle)), "sbgpu_quantify_host")
    info = (C.c_int64 * 8)()
    _lib.check(L.sbgpu_bins_info(handle, info), "sbgpu_bins_info")
    F = np.zeros(max(int(info[3]), 1), np.float64)
    _lib.check(L.sbgpu_bins_export_weights(handle, F.ctypes.data), "sbgpu_bins_export_weights")
    emp = None
    if used.use_emp:
        n = used.end_offset - used.start_offset + 1
        emp = np.ctypeslib.as_array(used.emp_hist, shape=(n,)).copy()
    table = None
    if context_keep is not None:
        from . import context
        try:
            table = context.context_table_host(handle, compat[:hits.n_hits], keep=context_keep,
                                               status=status[:annot.n_loci] if context_status is None else context_status)
        except Exception:
            L.sbgpu_bins_destroy(handle)
            raise
    assignment = None
    if assignment_theta is not None:
        from . import assign
        try:
            assignment = assign.fragment_assign_host(
                handle, compat[:hits.n_hits], theta[:n_iso] if assignment_theta is True else assignment_theta, keep=assignment_keep,
                status=status[:annot.n_loci] if assignment_status is None else assignment_status, hit_mass=hits.mass)
        except Exception:
            L.sbgpu_bins_destroy(handle)
            raise
    bins = LocusBins.__new__(LocusBins)
    bins._export(L, annot, handle, hits.n_hits, cw, kw, with_hit_bin=True)   # destroys the handle
    return {"theta": theta[:n_iso], "status": status[:annot.n_loci], "iters": iters[:annot.n_loci],
            "compat": compat[:hits.n_hits], "bins": bins, "F": F[:int(info[3])], "context": table, "assignment": assignment,
            "insert": {"mean": used.mean, "sd": used.sd, "use_emp": bool(used.use_emp), "start_offset": used.start_offset,
                       "end_offset": used.end_offset, "total_reads": used.total_reads, "emp_hist": emp}}


class BinsHandle:
    """Owner of an sbgpu_bins_t a call handed out: `h` is the raw handle (what bootstrap.abundance_bootstrap_device and
    context.context_table_device take; they accept this object too).  close() -- also on __exit__ and when the object is
    collected -- destroys it, once."""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def close(self):
        if self.h is not None and self.h.value:
            self.L.sbgpu_bins_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: the library may be gone already
            pass


def quantify_resident(annot, hits, insert, read_len, mapped_reads, long_read=False, ctx=None, device=0, comm=None,
                      min_isoform_frac=0.0, filter_by_expression=True, effective_len_norm=False, with_context=False, bootstrap=None,
                      keep_bootstrap=False, keep_handle=False, with_assignment=False, with_coverage=False, with_fit=False, with_info=False,
                      with_support=False, with_body_profile=False, iso_strand=None, n_pos=20, with_splicing=False, with_variational=False):
    """sbgpu_quantify_resident on host hits brought to the device first (torch owns the copies): pass 1 (insert=None: the
    empirical insert-size law, built on the device), bins, weights, EM, FPKM / Frac / keep, the FPKM all-reduce over `comm`
    (dist.AbiComm / dist.HostComm; None: a world of one), TPM.  The hits must come grouped by locus.
    with_context: the call keeps what the `-f` table needs (sbgpu_context_table_keep) and the table is built on the device
    (context.context_table_device) -> "context"; "bins": the handle's LocusBins (the rows index its bins).
    with_assignment: the same retention, and every hit's isoform posterior under the call's theta and the hits' masses, built on
    the device (assign.fragment_assign_device) -> "assignment"; "bins" as with_context.
    with_coverage: the same retention, and the isoform-resolved coverage under the call's theta and the hits' masses, built on the
    device from the hits the call was given (coverage.isoform_coverage_device) -> "coverage"; "bins" as with_context.
    with_body_profile: the same retention, and the transcript-body coverage profile under the call's theta and the hits' masses at
    n_pos positional bins, oriented by iso_strand (one of 0, 1, 2 per isoform; None: all 0), built on the device
    (body.body_profile_device) -> "body_profile": a body.BodyProfile; "bins" as with_context.
    bootstrap = dict(n_rep=, seed=, level=0.95, locus_id=None, ...): the call keeps what the bootstrap needs (sbgpu_bootstrap_keep)
    and bootstrap.abundance_bootstrap_device runs on its handle with these arguments (and `comm`) -> "bootstrap": its dict; "bins" as above.
    With locus=True among them the bootstrap is sbgpu_locus_bootstrap_device: "bootstrap" also holds "frac" and "locus" (DESIGN 3.19).
    with_fit: the bootstrap's retention, and the model fit under the call's theta, keep and status, built on the device
    (fit.model_fit_device) -> "fit": a fit.ModelFit; "bins" as with_context.
    with_info: the bootstrap's retention, and the isoform information under the call's theta, keep and status, built on the device
    (info.model_info_device) -> "isoform_info": an info.IsoformInfo ("info" is the handle's sizes); "bins" as with_context.
    with_support: the bootstrap's retention, and the drop-one isoform support under the call's keep, built on the device
    (support.model_loo_device) -> "isoform_support": a support.IsoformSupport; "bins" as with_context.
    with_variational (True, or a dict of alpha / change_limit / max_iter): the bootstrap's retention, and the variational Bayes solve of
    the call's bins, on the device (vb.model_vb_device) -> "variational": a vb.VariationalFit, and "variational_abundance": its
    abundance() under the call's epilogue parameters; "bins" as with_context.  The call's own results do not change.
    with_splicing (True, or a splice.SpliceEvents / splice.DeviceSpliceEvents built before: the table is annotation-only): the PSI
    of every annotated exon and intron from the call's d_fpkm / d_keep, built on the device (splice.splice_psi) -> "splicing": a
    splice.SplicePsi; with bootstrap=dict(...) also its mean, variance and interval over the bootstrap's replicates at the bootstrap's
    ranks, defined_count and (unless the bootstrap has replicates=False) the PSI matrix rep [n_rep, n_events], with with_coverage=True
    also its support.  Nothing more is retained, and no other result changes.
    keep_bootstrap: retention for the bootstrap on, without running it (for a caller that runs it several times).
    keep_handle: the handle is not exported but returned as "handle", a BinsHandle that owns it -- it is destroyed by its close(),
    as a context manager, or when the object is collected; the caller runs bootstrap.abundance_bootstrap_device /
    context.context_table_device on it before the context's next quantify call.
    -> dict(theta, fpkm, frac, tpm, keep, status, iters, insert, total_fpkm, total_mapped_reads, n_frag_lens, info)"""
    import torch
    ctx = ctx or default_context(device)
    L = ctx.L
    dev = torch.device("cuda", ctx.device)
    if hits.n_hits > 1 and (np.diff(hits.hit_locus) < 0).any():
        raise ValueError("quantify_resident: hits must be grouped by locus")
    off = np.concatenate([[0], np.cumsum(np.bincount(hits.hit_locus, minlength=annot.n_loci))]).astype(np.int64)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)  # noqa: E731
    d = {"hit_locus": up(hits.hit_locus, np.int32), "feat_off": up(hits.feat_off, np.int64), "feat_code": up(hits.feat_code, np.uint8),
         "feat_left": up(hits.feat_left, np.int32), "feat_right": up(hits.feat_right, np.int32)}
    d_mass = up(hits.mass, np.float32)
    hs = _lib.sbgpu_hits_t()
    hs.n_hits = hits.n_hits
    for k, v in d.items():
        setattr(hs, k, v.data_ptr())
    a = annot._struct()
    n_iso, nl = int(annot.iso_off[-1]), annot.n_loci
    res = {k: np.zeros(n_iso + 1, np.float64) for k in ("theta", "fpkm", "frac", "tpm")}
    res["keep"] = np.zeros(n_iso + 1, np.int32)
    res["status"], res["iters"] = np.zeros(nl + 1, np.int32), np.zeros(nl + 1, np.int32)
    out = _lib.sbgpu_abundances_t()
    for k, v in res.items():
        setattr(out, k, v.ctypes.data)
    par = _lib.sbgpu_abundance_params_t(0, int(effective_len_norm), int(filter_by_expression), 0, 0.0, float(min_isoform_frac))
    used = _lib.sbgpu_insert_t()
    ins = insert._struct(read_len, long_read) if insert is not None else None
    handle = C.c_void_p()
    torch.cuda.synchronize(dev)
    retain = bool(with_context) or bool(with_assignment) or bool(with_coverage) or bool(with_body_profile)
    if retain:
        _lib.check(L.sbgpu_context_table_keep(ctx.h, 1), "sbgpu_context_table_keep")
    keep_bootstrap = bool(keep_bootstrap) or bootstrap is not None or bool(with_fit) or bool(with_info) or bool(with_support) or bool(with_variational)
    if keep_bootstrap:
        _lib.check(L.sbgpu_bootstrap_keep(ctx.h, 1), "sbgpu_bootstrap_keep")
    try:
        _lib.check(L.sbgpu_quantify_resident(ctx.h, C.byref(a), C.byref(hs), d_mass.data_ptr(), off.ctypes.data,
                                             C.byref(ins) if ins is not None else None, int(read_len), int(long_read), int(mapped_reads),
                                             C.byref(par), comm.h if comm is not None else None, C.byref(used), C.byref(out),
                                             C.byref(handle)), "sbgpu_quantify_resident")
    finally:
        if retain:
            L.sbgpu_context_table_keep(ctx.h, 0)    # (what the call kept stays until the context's next quantify call)
        if keep_bootstrap:
            L.sbgpu_bootstrap_keep(ctx.h, 0)
    emp = None
    if used.use_emp:
        emp = np.ctypeslib.as_array(used.emp_hist, shape=(used.end_offset - used.start_offset + 1,)).copy()
    owner = BinsHandle(L, handle) if keep_handle else None     # (from here on an exception frees the handle with the object)
    info = (C.c_int64 * 8)()
    _lib.check(L.sbgpu_bins_info(handle, info), "sbgpu_bins_info")
    table = bins = boot = assignment = cov = model_fit = iso_info = iso_support = profile = variational = variational_abundance = None
    if retain or bootstrap is not None or with_fit or with_info or with_support or with_variational:
        from . import assign, body, context, coverage, fit, support, vb
        from . import info as isoform_info
        from .bootstrap import abundance_bootstrap_device
        from .exonbin import LocusBins
        try:
            if bootstrap is not None:
                boot = abundance_bootstrap_device(ctx, handle, comm=comm, **bootstrap)
            if with_context:
                table = context.context_table_device(ctx, handle)
            if with_assignment:
                assignment = assign.fragment_assign_device(ctx, handle, int(out.d_theta), hits.n_hits, d_hit_mass=d_mass)
            if with_coverage:
                cov = coverage.isoform_coverage_device(ctx, handle, annot, hs, int(out.d_theta), d_hit_mass=d_mass)
            if with_body_profile:
                profile = body.body_profile_device(ctx, handle, annot, hs, int(out.d_theta), d_hit_mass=d_mass, iso_strand=iso_strand, n_pos=n_pos)
            if with_fit:
                model_fit = fit.model_fit_device(ctx, handle, int(out.d_theta), int(out.d_keep), int(out.d_status))
            if with_info:
                iso_info = isoform_info.model_info_device(ctx, handle, int(out.d_theta), int(out.d_keep), int(out.d_status))
            if with_support:
                iso_support = support.model_loo_device(ctx, handle, int(out.d_keep), keep=res["keep"][:n_iso])
            if with_variational:
                vpar = _lib.sbgpu_abundance_params_t(int(out.total_mapped_reads), par.effective_len_norm, par.filter_by_expression, 0,
                                                     float(used.mean), par.min_isoform_frac)
                variational = vb.model_vb_device(ctx, handle, abundance=vpar, **(with_variational if isinstance(with_variational, dict) else {}))
                variational_abundance = variational.abundance()
        except Exception:
            if owner is None:
                L.sbgpu_bins_destroy(handle)
            raise
        if not keep_handle:
            bins = LocusBins.__new__(LocusBins)
            bins._export(L, annot, handle, hits.n_hits, annot.compat_words, annot.key_words, with_hit_bin=False)   # destroys the handle
    elif not keep_handle:
        L.sbgpu_bins_destroy(handle)
    splicing = None
    if with_splicing is not False and with_splicing is not None:
        # (the call's d_fpkm / d_keep, the bootstrap's replicates and the coverage's arrays all live until the context's next call)
        from . import splice
        splicing = splice.splice_psi(ctx, splice.as_device_events(ctx, with_splicing, annot), int(out.d_fpkm or 0), int(out.d_keep or 0),
                                     bootstrap=boot, coverage=cov, replicates=bool(bootstrap is not None and bootstrap.get("replicates", True)))
    r = {k: (v[:n_iso] if k not in ("status", "iters") else v[:nl]) for k, v in res.items()}
    r.update({"insert": {"mean": used.mean, "sd": used.sd, "use_emp": bool(used.use_emp), "start_offset": used.start_offset,
                         "end_offset": used.end_offset, "total_reads": used.total_reads, "emp_hist": emp},
              "total_fpkm": float(out.total_fpkm), "total_mapped_reads": int(out.total_mapped_reads), "n_frag_lens": int(out.n_frag_lens),
              "info": {"n_bins": int(info[2]), "n_elem": int(info[3]), "n_pairs": int(info[4])}})
    if with_context:
        r.update(context=table, bins=bins)
    if with_assignment:
        r.update(assignment=assignment, bins=bins)
    if with_coverage:
        r.update(coverage=cov, bins=bins)
    if with_body_profile:
        r.update(body_profile=profile, bins=bins)
    if bootstrap is not None:
        r.update(bootstrap=boot, bins=bins)
    if with_fit:
        r.update(fit=model_fit, bins=bins)
    if with_info:
        r.update(isoform_info=iso_info, bins=bins)
    if with_support:
        r.update(isoform_support=iso_support, bins=bins)
    if with_variational:
        r.update(variational=variational, variational_abundance=variational_abundance, bins=bins)
    if splicing is not None:
        r["splicing"] = splicing
    if keep_handle:
        r["handle"] = owner
    return r
