"""Differential isoform usage between two GROUPS of replicate samples: does the usage of a locus differ between two conditions by
more than it differs among the replicates of each?  Every sample is solved, every group under one shared theta, all samples under
one shared theta (pooled problems whose columns are scaled so that the shared theta is the joint maximum-likelihood one), and the
likelihoods are compared on two levels (include/sbgpu.h states the rule).

em_gdiff_host       the three host calls around a solver the caller brings (the library has no CPU EM)
em_gdiff_device     sbgpu_em_gdiff_device: built in HBM for S batches of one annotation
model_gdiff_device  sbgpu_model_gdiff_device: from what S resident calls kept for the bootstrap on S contexts of one device
                    (ChainQuantifier / FrontQuantifier(keep_bootstrap=True).differential_usage_groups(group_a, group_b))

All return a GroupDifferentialUsage.  Samples are numbered group A's first; a per-sample array is [S, n_iso] or [S, n_loci].
With one sample in each group the result is diff.py's two-sample test (lr_between is its lr_stat) bit for bit.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr
from .diff import chi2_sf

NAMES = _lib.sbgpu_em_gdiff_t._NAMES
PER_ISO = ("theta_sample", "theta_group", "theta_all", "usage_sample", "usage_group", "usage_all", "delta_usage")
PER_SAMPLE = ("theta_sample", "usage_sample", "loglik_own", "loglik_group", "loglik_all", "n_frag", "status_sample", "iters_sample")
PER_GROUP = ("theta_group", "usage_group", "status_group", "iters_group")
FLOAT64 = PER_ISO + ("lr_between", "lr_within", "loglik_own", "loglik_group", "loglik_all")
INT64 = ("n_frag", "lost_shift")
DTYPES = {k: np.float64 if k in FLOAT64 else np.int64 if k in INT64 else np.int32 for k in NAMES}
LIMIT_NAMES = ("max_kept", "max_pooled_bins", "tile_vals", "tile_rows", "group_max_kept", "threads", "grid_per_cu", "default_bytes", "max_samples")
OK, EMPTY, SOLE, TOO_WIDE, TOO_DEEP, _ONE_SAMPLE, UNSOLVED, ONE_GROUP, THIN = range(9)
STATUS_NAMES = ("OK", "EMPTY", "SOLE", "TOO_WIDE", "TOO_DEEP", "ONE_SAMPLE", "UNSOLVED", "ONE_GROUP", "THIN")
KIND_OWN, KIND_GROUP_A, KIND_GROUP_B, KIND_ALL = range(4)
MAX_SAMPLES = 16


def limits():
    """The thresholds (csrc/gdiff_rules.h, csrc/gdiff_device.h) by name: see sbgpu_em_gdiff_limits."""
    out = (C.c_int64 * 9)()
    _lib.check(_lib.load().sbgpu_em_gdiff_limits(out), "sbgpu_em_gdiff_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def params(max_bytes=0):
    """max_bytes: the device scratch one chunk of sub-problems may take (0: 1 GiB)"""
    return _lib.sbgpu_gdiff_params_t(int(max_bytes), 0)


def _beta_cf(a, b, x):
    """The continued fraction of the incomplete beta function (modified Lentz; to 1e-16 relative or 2000 terms)"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = tiny if abs(d) < tiny else d
    d = 1.0 / d
    h = d
    for m in range(1, 2000):
        m2 = 2 * m
        for num in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + num * d
            d = tiny if abs(d) < tiny else d
            c = 1.0 + num / c
            c = tiny if abs(c) < tiny else c
            d = 1.0 / d
            step = d * c
            h *= step
        if abs(step - 1.0) < 1e-16:
            break
    return h


def _beta_reg(a, b, x, y):
    """The regularised incomplete beta function I_x(a, b), a, b > 0, with y = 1 - x given by the caller (no cancellation): the
    continued fraction on the side where it converges fast, the symmetry I_x(a, b) = 1 - I_y(b, a) on the other."""
    if x <= 0.0:
        return 0.0
    if y <= 0.0:
        return 1.0
    lead = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(y))
    if x < (a + 1.0) / (a + b + 2.0):
        return min(1.0, max(0.0, lead * _beta_cf(a, b, x) / a))
    return min(1.0, max(0.0, 1.0 - lead * _beta_cf(b, a, y) / b))


def f_sf(x, d1, d2):
    """The survival function of F with (d1, d2) >= 1 degrees of freedom at x: I_{d2 / (d2 + d1 x)}(d2 / 2, d1 / 2); 1.0 at
    x <= 0, 0.0 at infinity."""
    x = float(x)
    if not x > 0.0:
        return 1.0
    if math.isinf(x):
        return 0.0
    den = d2 + d1 * x
    return _beta_reg(0.5 * d2, 0.5 * d1, d2 / den, d1 * x / den)


class GroupDifferentialUsage(Results):
    """theta_sample, usage_sample [S, n_iso]; theta_group, usage_group [2, n_iso]; theta_all, usage_all, delta_usage [n_iso]
    (float64); lr_between, lr_within [n_loci], loglik_own, loglik_group, loglik_all [S, n_loci] (float64); n_frag [S, n_loci],
    lost_shift (int64); dof_between, dof_within, p_a, p_b, gdiff_status, top_iso, status_all, iters_all [n_loci], status_sample,
    iters_sample [S, n_loci], status_group, iters_group [2, n_loci] (int32).
    want: the names to bring to the host (None: all) -- the device forms copy nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / gdiff call)."""
    STRUCT = _lib.sbgpu_em_gdiff_t

    def __init__(self, iso_off, n_a, n_b, want=None):
        self.iso_off = np.ascontiguousarray(iso_off, np.int64)
        self.n_loci, self.n_iso = len(self.iso_off) - 1, int(self.iso_off[-1])
        self.n_a, self.n_b, self.n_samples = int(n_a), int(n_b), int(n_a) + int(n_b)
        lead = lambda k: self.n_samples if k in PER_SAMPLE else 2 if k in PER_GROUP else 1  # noqa: E731
        self._lead = {k: lead(k) for k in NAMES}
        self._arrays({k: (lead(k) * (self.n_iso if k in PER_ISO else self.n_loci), DTYPES[k]) for k in NAMES}, want)

    def _finish(self, s):
        Results._finish(self, s)
        for k in PER_SAMPLE + PER_GROUP:
            a = getattr(self, k)
            if a is not None:
                setattr(self, k, a.reshape(self._lead[k], -1))
        return self

    def _compared(self, l):
        return int(self.gdiff_status[l]) == OK and int(self.lost_shift[l]) == 0 and int(self.dof_between[l]) >= 1

    def dispersion(self):
        """Per locus: phi = max(1, lr_within / dof_within), the replicates' excess over multinomial sampling; NaN where there is
        no within-group degree of freedom or the locus is not compared (status not OK, or lost_shift != 0)."""
        phi = np.full(self.n_loci, np.nan)
        for l in range(self.n_loci):
            if self._compared(l) and int(self.dof_within[l]) >= 1:
                phi[l] = max(1.0, float(self.lr_within[l]) / int(self.dof_within[l]))
        return phi

    def p_value(self, method="chi2"):
        """Per locus.  chi2: the chi-squared survival function with dof_between degrees of freedom at max(lr_between, 0) -- the
        two-sample test's, blind to variation among replicates.  quasi: F = (lr_between / dof_between) / dispersion() on
        (dof_between, dof_within) degrees of freedom; chi2 where dof_within is 0.  NaN where lost_shift != 0 or the status is
        neither OK nor SOLE; 1.0 for SOLE."""
        if method not in ("chi2", "quasi"):
            raise ValueError("p_value: method is 'chi2' or 'quasi'")
        p = np.full(self.n_loci, np.nan)
        for l in range(self.n_loci):
            if int(self.gdiff_status[l]) == SOLE:
                p[l] = 1.0
            elif self._compared(l):
                d1, d2 = int(self.dof_between[l]), int(self.dof_within[l])
                if method == "chi2" or d2 < 1:
                    p[l] = chi2_sf(self.lr_between[l], d1)
                else:
                    phi = max(1.0, float(self.lr_within[l]) / d2)
                    p[l] = f_sf(float(self.lr_between[l]) / d1 / phi, d1, d2)
        return p

    def significant(self, alpha=0.05, method="quasi"):
        """The loci whose p-value is below alpha, ascending (a NaN is never significant)."""
        p = self.p_value(method)
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(p < alpha)

    def rows(self, names=None):
        """-> (locus, status, p_a, p_b, lr_between, dof_between, lr_within, dof_within, dispersion, p_chi2, p_quasi, lost_shift,
        top_iso, top delta_usage) per locus, for a TSV: the locus as its index, or -- names = locus names -- by name."""
        pc, pq, phi = self.p_value("chi2"), self.p_value("quasi"), self.dispersion()
        for l in range(self.n_loci):
            top = int(self.top_iso[l])
            yield (names[l] if names else l, STATUS_NAMES[int(self.gdiff_status[l])], int(self.p_a[l]), int(self.p_b[l]), float(self.lr_between[l]),
                   int(self.dof_between[l]), float(self.lr_within[l]), int(self.dof_within[l]), float(phi[l]), float(pc[l]), float(pq[l]),
                   int(self.lost_shift[l]), top, float(self.delta_usage[int(self.iso_off[l]) + top]) if top >= 0 else 0.0)


def _groups(n_a, n_b, who):
    if n_a < 1 or n_b < 1 or n_a + n_b > MAX_SAMPLES:
        raise _lib.SbgpuError("%s: each group holds at least one sample, both together at most %d" % (who, MAX_SAMPLES))


def _pointers(values):
    """a C array of pointers (None: NULL) -> (array, what it points into)"""
    return (C.c_void_p * len(values))(*values)


def _keeps(keeps, S, n_iso, who):
    """keeps: None, or S entries each None or [n_iso] -> (list of arrays / None, C array of pointers or None)"""
    if keeps is None:
        return [None] * S, None
    if len(keeps) != S:
        raise ValueError("%s: keeps holds one entry per sample" % who)
    arrays = [as_array(k, np.int32) for k in keeps]
    check_lengths(who, *(("keep[%d]" % i, a, n_iso) for i, a in enumerate(arrays)))
    return arrays, _pointers([None if a is None else a.ctypes.data for a in arrays])


def _offsets(batches, who):
    rows = [np.ascontiguousarray(b.row_off, np.int64) for b in batches]
    isos = [np.ascontiguousarray(b.iso_off, np.int64) for b in batches]
    if isos[0].size < 1 or any(r.size != i.size for r, i in zip(rows, isos)):
        raise ValueError("%s: row_off and iso_off hold n_loci + 1 entries" % who)
    if any(i.size != isos[0].size or (i != isos[0]).any() for i in isos):
        raise _lib.SbgpuError("%s: the batches differ in n_loci or iso_off: they are not over one annotation" % who)
    return rows, isos[0]


def shapes_host(row_offs_a, row_offs_b, iso_off, keeps=None):
    """Rules 1 and 2 -> dict: gdiff_status [n_loci] (before the solves); sub_locus, sub_kind, sub_sample [n_sub]; row_off,
    iso_off, f_off [n_sub + 1] of the sub-batch.  row_offs_a, row_offs_b: one row_off per sample of each group."""
    L = _lib.load()
    n_a, n_b = len(row_offs_a), len(row_offs_b)
    _groups(n_a, n_b, "shapes_host")
    rows = [np.ascontiguousarray(r, np.int64) for r in list(row_offs_a) + list(row_offs_b)]
    iso_off = np.ascontiguousarray(iso_off, np.int64)
    if iso_off.size < 1 or any(r.size != iso_off.size for r in rows):
        raise ValueError("shapes_host: every row_off and iso_off hold n_loci + 1 entries")
    n_loci = iso_off.size - 1
    keep_arrays, keep_p = _keeps(keeps, n_a + n_b, int(iso_off[-1]), "shapes_host")
    sizes = (C.c_int64 * 4)()
    args = (n_loci, n_a, n_b, _pointers([r.ctypes.data for r in rows]), iso_off.ctypes.data, keep_p, sizes)
    _lib.check(L.sbgpu_em_gdiff_shapes_host(*args, *([None] * 7)), "sbgpu_em_gdiff_shapes_host")
    n_sub = int(sizes[0])
    out = dict(gdiff_status=np.zeros(max(n_loci, 1), np.int32), sub_locus=np.zeros(max(n_sub, 1), np.int32), sub_kind=np.zeros(max(n_sub, 1), np.int32),
               sub_sample=np.zeros(max(n_sub, 1), np.int32), row_off=np.zeros(n_sub + 1, np.int64), iso_off=np.zeros(n_sub + 1, np.int64),
               f_off=np.zeros(n_sub + 1, np.int64))
    order = ("gdiff_status", "sub_locus", "sub_kind", "sub_sample", "row_off", "iso_off", "f_off")
    _lib.check(L.sbgpu_em_gdiff_shapes_host(*args, *(out[k].ctypes.data for k in order)), "sbgpu_em_gdiff_shapes_host")
    del keep_arrays
    out["gdiff_status"] = out["gdiff_status"][:n_loci]
    for k in ("sub_locus", "sub_kind", "sub_sample"):
        out[k] = out[k][:n_sub]
    return out


def _batch_structs(batches, who, weights=True):
    """-> (C array of pointers to sbgpu_batch_t, what they point into)"""
    hold, structs = [], []
    for b in batches:
        row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (b.row_off, b.iso_off, b.f_off))
        count = np.ascontiguousarray(b.count, np.int32)
        F = np.ascontiguousarray(b.F, np.float64) if weights else None
        check_lengths(who, ("count", count, int(row_off[-1])), ("F", F, int(f_off[-1])))
        structs.append(_lib.sbgpu_batch_t(len(row_off) - 1, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F)))
        hold.append((row_off, iso_off, f_off, count, F))
    return _pointers([C.addressof(s) for s in structs]), (hold, structs)


def expand_host(batches_a, batches_b, keeps=None, shapes=None):
    """The sub-batch's (count, F) for two groups of batches (row_off, iso_off, f_off, count, F each) and their keeps; shapes:
    shapes_host's, or None."""
    L = _lib.load()
    batches = list(batches_a) + list(batches_b)
    n_a, n_b = len(batches_a), len(batches_b)
    _groups(n_a, n_b, "expand_host")
    rows, iso_off = _offsets(batches, "expand_host")
    keep_arrays, keep_p = _keeps(keeps, n_a + n_b, int(iso_off[-1]), "expand_host")
    sh = shapes or shapes_host(rows[:n_a], rows[n_a:], iso_off, keep_arrays if keeps is not None else None)
    sub_count, sub_F = np.zeros(max(int(sh["row_off"][-1]), 1), np.int32), np.zeros(max(int(sh["f_off"][-1]), 1), np.float64)
    bp, hold = _batch_structs(batches, "expand_host")
    _lib.check(L.sbgpu_em_gdiff_expand_host(n_a, n_b, bp, keep_p, sub_count.ctypes.data, sub_F.ctypes.data), "sbgpu_em_gdiff_expand_host")
    del hold, keep_arrays
    return sub_count[:int(sh["row_off"][-1])], sub_F[:int(sh["f_off"][-1])]


def cross_inputs(sh, theta, status, level):
    """The cross fit's (theta, status) for a sub-batch: level 0 -- every OWN sub-problem gets its group's (its own where the group
    has one present sample); level 1 -- ALL's.  Group and ALL sub-problems keep their own."""
    sub_iso_off = np.asarray(sh["iso_off"], np.int64)
    x_theta, x_status = np.array(theta, np.float64), np.array(status, np.int32)
    kinds, loci = sh["sub_kind"], sh["sub_locus"]
    for q in range(len(kinds)):
        if kinds[q] != KIND_OWN:
            continue
        group_kind = KIND_GROUP_A if sh["sub_sample"][q] < sh["n_a"] else KIND_GROUP_B
        want = KIND_ALL if level else group_kind
        src, r = None, q + 1
        while r < len(kinds) and loci[r] == loci[q]:     # (a locus' sub-problems are consecutive)
            if kinds[r] == want:
                src = r
            r += 1
        if src is None:
            continue
        x_theta[int(sub_iso_off[q]):int(sub_iso_off[q + 1])] = theta[int(sub_iso_off[src]):int(sub_iso_off[src + 1])]
        x_status[q] = status[src]
    return x_theta, x_status


def em_gdiff_host(batches_a, batches_b, keeps, solve, want=None):
    """batches_a, batches_b: the two groups' batches (row_off, iso_off, f_off, count, F: synth.LocusBatch) over one annotation;
    keeps: None or one entry per sample ([n_iso] or None); solve: a callable (row_off, iso_off, f_off, count, F) -> (theta,
    status, iters) that solves a batch as sbgpu_em_run_device does.  The sub-batch is made (shapes, expansion), solved by `solve`,
    fitted three times by sbgpu_em_fit_host with nothing erased (own; at the groups' theta; at ALL's), and reduced."""
    from . import fit as _fit
    L = _lib.load()
    batches = list(batches_a) + list(batches_b)
    n_a, n_b = len(batches_a), len(batches_b)
    _groups(n_a, n_b, "em_gdiff_host")
    rows, iso_off = _offsets(batches, "em_gdiff_host")
    keep_arrays, keep_p = _keeps(keeps, n_a + n_b, int(iso_off[-1]), "em_gdiff_host")
    sh = shapes_host(rows[:n_a], rows[n_a:], iso_off, keep_arrays if keeps is not None else None)
    sh["n_a"] = n_a
    sub_count, sub_F = expand_host(batches_a, batches_b, keeps, sh)
    n_sub = len(sh["sub_locus"])
    theta, status, iters = solve(sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F)
    theta, status, iters = np.ascontiguousarray(theta, np.float64), np.ascontiguousarray(status, np.int32), np.ascontiguousarray(iters, np.int32)
    check_lengths("em_gdiff_host", ("theta", theta, int(sh["iso_off"][-1])), ("status", status, n_sub), ("iters", iters, n_sub))

    class _Sub:
        row_off, iso_off, f_off, count, F = sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F
    levels = ((theta, status), cross_inputs(sh, theta, status, 0), cross_inputs(sh, theta, status, 1))
    own, grp, all_ = [_fit.em_fit_host(_Sub, t if t.size else np.zeros(1), None, s if n_sub else None, want=("loglik", "n_live", "n_dropped", "n_impossible"))
                      for t, s in levels]
    t = GroupDifferentialUsage(iso_off, n_a, n_b, want)
    s = t._struct()
    bp, hold = _batch_structs(batches, "em_gdiff_host", False)
    _lib.check(L.sbgpu_em_gdiff_stat_host(n_a, n_b, bp, keep_p, ptr(theta), ptr(status), ptr(iters), ptr(own.loglik), ptr(own.n_live), ptr(own.n_dropped),
                                          ptr(own.n_impossible), ptr(grp.loglik), ptr(grp.n_dropped), ptr(grp.n_impossible), ptr(all_.loglik),
                                          ptr(all_.n_dropped), ptr(all_.n_impossible), C.byref(s)), "sbgpu_em_gdiff_stat_host")
    del hold, keep_arrays
    t.sub = dict(sh, count=sub_count, F=sub_F, theta=theta, status=status, iters=iters, fit=own, cross_group=grp, cross_all=all_)
    return t._finish(s)


def _keeps_host(keeps, d_keeps, S):
    """the keeps on the host, for the shapes of with_sub_batch: given, or read back from tensors"""
    if keeps is not None or d_keeps is None:
        return keeps
    out = []
    for k in d_keeps:
        if k is not None and not hasattr(k, "cpu"):
            raise ValueError("gdiff: a d_keep is a device address: give keeps (the same values on the host) too")
        out.append(None if k is None else k.cpu().numpy())
    return out


def _device_keeps(d_keeps, S, who):
    if d_keeps is None:
        return None
    if len(d_keeps) != S:
        raise ValueError("%s: d_keeps holds one entry per sample" % who)
    check_tensors(who, **{"d_keeps[%d]" % i: (k, "torch.int32") for i, k in enumerate(d_keeps)})
    return _pointers([addr(k) for k in d_keeps])


def em_gdiff_device(ctx, samples_a, samples_b, d_keeps=None, keeps=None, max_bytes=0, stream=None, want=None, with_sub_batch=False):
    """samples_a, samples_b: the two groups, each a list of (plan, d_count, d_F) -- em.Plan, int32 and float64 torch tensors on
    the context's device (or device addresses); d_keeps: None or one int32 tensor / address / None per sample; max_bytes: the
    scratch budget of one chunk (0: 1 GiB); with_sub_batch: the expanded sub-batch comes back too, as .sub = dict(shapes_host's
    arrays, count, F) -- for a caller that checks the expansion (keeps: the keeps on the host, where d_keeps are addresses)."""
    samples = list(samples_a) + list(samples_b)
    n_a, n_b = len(samples_a), len(samples_b)
    _groups(n_a, n_b, "em_gdiff_device")
    for i, (_, d_count, d_F) in enumerate(samples):
        check_tensors("em_gdiff_device", **{"d_count[%d]" % i: (d_count, "torch.int32"), "d_F[%d]" % i: (d_F, "torch.float64")})
    keep_p = _device_keeps(d_keeps, n_a + n_b, "em_gdiff_device")
    plans = [x[0] for x in samples]
    t = GroupDifferentialUsage(plans[0].iso_off, n_a, n_b, want)
    s, p = t._struct(), params(max_bytes)
    if with_sub_batch:
        rows, iso_off = _offsets(plans, "em_gdiff_device")
        sh = shapes_host(rows[:n_a], rows[n_a:], iso_off, _keeps_host(keeps, d_keeps, n_a + n_b))
        sub_count, sub_F = np.zeros(int(sh["row_off"][-1]) + 1, np.int32), np.zeros(int(sh["f_off"][-1]) + 1)
        s.sub_count, s.sub_F = sub_count.ctypes.data, sub_F.ctypes.data
        t.sub = dict(sh, n_a=n_a, count=sub_count[:-1], F=sub_F[:-1])
    _lib.check(ctx.L.sbgpu_em_gdiff_device(ctx.h, n_a, n_b, _pointers([pl.h for pl in plans]), _pointers([addr(x[1]) for x in samples]),
                                           _pointers([addr(x[2]) for x in samples]), keep_p, C.byref(p), stream, C.byref(s)), "sbgpu_em_gdiff_device")
    return t._finish(s)


def model_gdiff_device(group_a, group_b, d_keeps=None, keeps=None, max_bytes=0, stream=None, want=None, with_sub_batch=False):
    """Right after S resident calls made with bootstrap_keep on, before any of their contexts' next quantify call.  group_a,
    group_b: lists of (ctx, handle), contexts of one device.  d_keeps: None or each call's keep (int32 tensor, device address or
    None) per sample.  The work and the results' device copies are the first context's.  with_sub_batch: as em_gdiff_device's."""
    pairs = list(group_a) + list(group_b)
    n_a, n_b = len(group_a), len(group_b)
    _groups(n_a, n_b, "model_gdiff_device")
    handles = [getattr(h, "h", h) for _, h in pairs]
    if any(h is None for h in handles) or any(c is None for c, _ in pairs):
        raise _lib.SbgpuError("model_gdiff_device: null argument (a context or a handle is None)")
    L = pairs[0][0].L
    keep_p = _device_keeps(d_keeps, n_a + n_b, "model_gdiff_device")

    def offsets(h):
        n = bins_info(L, h)[0]
        row_off, iso_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        _lib.check(L.sbgpu_bins_export(h, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
        return row_off, iso_off
    t = GroupDifferentialUsage(offsets(handles[0])[1], n_a, n_b, want)
    s, p = t._struct(), params(max_bytes)
    if with_sub_batch:
        offs = [offsets(h) for h in handles]
        sh = shapes_host([o[0] for o in offs[:n_a]], [o[0] for o in offs[n_a:]], offs[0][1], _keeps_host(keeps, d_keeps, n_a + n_b))
        sub_count, sub_F = np.zeros(int(sh["row_off"][-1]) + 1, np.int32), np.zeros(int(sh["f_off"][-1]) + 1)
        s.sub_count, s.sub_F = sub_count.ctypes.data, sub_F.ctypes.data
        t.sub = dict(sh, n_a=n_a, count=sub_count[:-1], F=sub_F[:-1])
    _lib.check(L.sbgpu_model_gdiff_device(n_a, n_b, _pointers([c.h for c, _ in pairs]), _pointers(handles), keep_p, C.byref(p), stream, C.byref(s)),
               "sbgpu_model_gdiff_device")
    return t._finish(s)
