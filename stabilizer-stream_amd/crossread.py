"""Bank read-out on the device for the pair and matrix objects (include/psdcascade_crossread.h, psdcxr_*): the stitched rows of every
selected pair of a CsdCascadeBank (or a CsdCascade) with, when asked, their frequencies, coherence, the H1 transfer function and
the sums of up to 8 frequency bands a pair, or the m * m rows of every selected group of a CsmCascadeBank (or a CsmCascade), in one
call: one drain, one kernel launch for all units, at most one more for the bands.  (The host forms make two C calls: the layout
first, to size their arrays, then the read-out, whose drain finds the pipeline idle.  The device forms and layout are one call each.)

    from stabilizer_stream_amd import crossread
    r = crossread.bank_csd(bank, coherence=True, transfer=True, bands=[(1e-4, 1e-3)])      # host arrays
    crossread.bank_csd_device(bank, stride, coherence=t.data_ptr())                        # into a torch tensor [P][stride] f64

Every f32 value and frequency equals what bank.csd(unit) and Break.frequencies return, byte for byte; coherence and H1 are formed
in f64 from the f64 accumulators.  The functions take the object; they add nothing to it."""
import ctypes as C

import numpy as np

from .bankread import _BREAK, _CAP, MAX_BANDS, _bands, _Breaks, _CInfo, _pkg  # noqa: F401  (one record layout, one lazy Break list)

_set = False


def _lib():
    """the package's library with the prototypes of include/psdcascade_crossread.h set"""
    global _set
    L = _pkg().lib()
    if not _set:
        u32, i, vp, sz = C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
        head = [vp, vp, u32, i, u32, i]  # handle, units, n_sel, keep_overlap, min_count, keep_transition_band
        tail = [vp, vp, vp, sz, C.POINTER(_CInfo)]  # lens, n_breaks, breaks, breaks_cap, info
        pair = [vp] * 6 + [sz, vp, u32, vp]  # sxx, syy, sxy, freq, coherence, transfer, stride, bands, n_bands, band_sums
        for name, args in (("cross_layout", head + tail), ("cross_csd_device", head + pair + [vp] + tail), ("cross_csd", head + pair + tail),
                           ("cross_release", [vp]), ("csm_layout", head + tail), ("csm_rows_device", head + [vp, vp, sz, vp] + tail),
                           ("csm_rows", head + [vp, vp, sz] + tail), ("csm_release", [vp])):
            fn = getattr(L, "psdcxr_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        _set = True
    return L


def _bank(obj, kinds):
    """(the bank behind `obj`, its C family): kinds = "cross", "csm" or both"""
    pkg = _pkg()
    b = obj._b if isinstance(obj, (pkg.CsdCascade, pkg.CsmCascade)) else obj
    # (the exact classes: the zoom, IQ and AM/PM pair banks are other objects behind other handle types)
    kind = {pkg.CsdCascadeBank: "cross", pkg.CsmCascadeBank: "csm"}.get(type(b))
    if kind not in kinds:
        names = " or ".join({"cross": "a CsdCascadeBank or a CsdCascade", "csm": "a CsmCascadeBank or a CsmCascade"}[k] for k in kinds)
        raise pkg.PsdError(pkg.ERR_ARG, "this read-out takes " + names)
    return b, kind


class _Call:
    """the arguments every psdcxr_ call shares, and what it returns through them"""

    def __init__(self, obj, units, opts, kinds):
        pkg = _pkg()
        self.b, self.kind = _bank(obj, kinds)
        opts = pkg.MergeOpts() if opts is None else opts
        if units is None:
            self.sel, self.rows = None, self.b.n_pairs if self.kind == "cross" else self.b.n_groups
        else:
            u = [int(v) for v in units]
            if any(not 0 <= v <= pkg.U32_MAX for v in u):
                raise pkg.PsdError(pkg.ERR_ARG, "unit indices must be in [0, 2^32)")
            self.sel, self.rows = np.zeros(max(1, len(u)), np.uint32), len(u)  # (never NULL: that selects every unit)
            self.sel[:len(u)] = u
        if not 0 <= int(opts.min_count) <= pkg.U32_MAX:
            raise pkg.PsdError(pkg.ERR_ARG, "min_count must be in [0, 2^32)")
        self.head = (self.b._h, self.sel.ctypes.data if self.sel is not None else None, self.rows, int(opts.keep_overlap),
                     int(opts.min_count), int(opts.keep_transition_band))
        self.lens = np.zeros(max(1, self.rows), np.uintp)
        self.nb = np.zeros(max(1, self.rows), np.uintp)
        self.br = np.zeros(max(1, self.rows * _CAP), _BREAK)
        self.info = _CInfo()
        self.tail = (self.lens.ctypes.data, self.nb.ctypes.data, self.br.ctypes.data, _CAP, C.byref(self.info))

    def fn(self, name):
        return getattr(_lib(), "psdcxr_" + self.kind + "_" + name)

    def layout(self):
        self.b._ck(self.fn("layout")(*self.head, *self.tail))
        return int(self.info.max_len)

    def result(self):
        return {"lens": self.lens[:self.rows].tolist(), "breaks": _Breaks(self.br, self.nb[:self.rows].tolist())}


def _ptr(p):
    return C.c_void_p(p) if p else None


def layout(bank, units=None, opts=None):
    """dict(lens, breaks, max_len) of the selected pairs of a CsdCascadeBank / CsdCascade or groups of a CsmCascadeBank / CsmCascade
    (None: all, in order; else indices in any order, duplicates allowed): per unit the stitched length and the list of Break that
    csd(unit, opts) returns (`breaks` reads like a list of lists; the Break objects are made when it is first indexed).  Drains the
    bank; launches nothing."""
    c = _Call(bank, units, opts, ("cross", "csm"))
    width = c.layout()
    return {**c.result(), "max_len": width}


def bank_csd(bank, pairs=None, opts=None, frequencies=False, coherence=False, transfer=False, bands=None):
    """dict(sxx, syy, sxy, lens, breaks, launches) of the selected pairs: sxx and syy are float32 [P][max_len], sxy complex64, row i
    holding lens[i] values and NaN behind them; breaks one list of Break a row.  frequencies=True adds `frequencies` (float32),
    coherence=True `coherence` (float64: |Sxy|^2 / (Sxx Syy), NaN where the denominator is zero), transfer=True `transfer`
    (complex128: H1 = Sxy / Sxx, NaN where Sxx is zero), all of the same shape and NaN behind each row's length; bands=[(lo, hi), ...]
    (at most 8, in cycles per sample) adds `band_sums` float64 [P][n_bands][4]: the trapezoidal integrals of sxx, syy, re sxy and
    im sxy over the bins whose frequency lies in [lo, hi] (band_coherence and band_transfer take them)."""
    c = _Call(bank, pairs, opts, ("cross",))
    width = c.layout()
    shape = (c.rows, width)
    out = {"sxx": np.full(shape, np.nan, np.float32), "syy": np.full(shape, np.nan, np.float32), "sxy": np.full(shape, np.nan, np.complex64)}
    if frequencies:
        out["frequencies"] = np.full(shape, np.nan, np.float32)
    if coherence:
        out["coherence"] = np.full(shape, np.nan, np.float64)
    if transfer:
        out["transfer"] = np.full(shape, np.nan, np.complex128)
    ba, nb = _bands(bands)
    if ba is not None:
        out["band_sums"] = np.zeros((c.rows, nb, 4), np.float64)
    if width:  # (else no selected pair has an included stage: nothing to launch, the band sums are 0.0)
        ptrs = [out[k].ctypes.data if k in out else None for k in ("sxx", "syy", "sxy", "frequencies", "coherence", "transfer")]
        c.b._ck(c.fn("csd")(*c.head, *ptrs, width, ba.ctypes.data if nb else None, nb, out["band_sums"].ctypes.data if nb else None, *c.tail))
    return {**out, **c.result(), "launches": int(c.info.launches)}


def bank_csd_device(bank, stride, sxx=None, syy=None, sxy=None, freq=None, coherence=None, transfer=None, pairs=None, opts=None, bands=None,
                    band_ptr=None, done_event=None):
    """bank_csd() written into device memory.  sxx, syy, freq (float32), coherence (float64), sxy (float32 pairs) and transfer
    (float64 pairs) are device addresses (tensor.data_ptr()) of rows of `stride` bins, any may be None; row i receives lens[i]
    bins, the rest of the row is left as it is.  band_ptr is a device address of float64 [P][n_bands][4] (with bands).
    done_event: None -- the call returns when the kernels have completed -- or a hipEvent_t handle, as the after= arguments of
    the feeds take it: it is recorded behind the kernels on the bank's stream and the call returns without waiting.  Returns
    dict(lens, breaks, launches)."""
    c = _Call(bank, pairs, opts, ("cross",))
    ba, nb = _bands(bands)
    c.b._ck(c.fn("csd_device")(*c.head, *[_ptr(p) for p in (sxx, syy, sxy, freq, coherence, transfer)], int(stride),
                               ba.ctypes.data if nb else None, nb, _ptr(band_ptr), _ptr(done_event), *c.tail))
    return {**c.result(), "launches": int(c.info.launches)}


def bank_rows(bank, groups=None, opts=None, frequencies=False):
    """dict(rows, lens, breaks, launches) of the selected groups of a CsmCascadeBank / CsmCascade: rows is float32
    [G][m * m][max_len] in the row order csm_matrix reads, NaN behind each group's length; frequencies=True adds `frequencies`
    float32 [G][max_len]."""
    c = _Call(bank, groups, opts, ("csm",))
    width = c.layout()
    out = {"rows": np.full((c.rows, c.b.m * c.b.m, width), np.nan, np.float32)}
    if frequencies:
        out["frequencies"] = np.full((c.rows, width), np.nan, np.float32)
    if width:
        c.b._ck(c.fn("rows")(*c.head, out["rows"].ctypes.data, out["frequencies"].ctypes.data if frequencies else None, width, *c.tail))
    return {**out, **c.result(), "launches": int(c.info.launches)}


def bank_rows_device(bank, stride, rows=None, freq=None, groups=None, opts=None, done_event=None):
    """bank_rows() written into device memory: rows a device address of float32 [G][m * m][stride], freq of float32 [G][stride],
    either may be None; the rest as bank_csd_device."""
    c = _Call(bank, groups, opts, ("csm",))
    c.b._ck(c.fn("rows_device")(*c.head, _ptr(rows), _ptr(freq), int(stride), _ptr(done_event), *c.tail))
    return {**c.result(), "launches": int(c.info.launches)}


def band_coherence(band_sums):
    """(re^2 + im^2) / (xx yy) of band sums [..., 4] = (xx, yy, re xy, im xy), NaN where the denominator is zero"""
    s = np.asarray(band_sums, np.float64)
    den = s[..., 0] * s[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, (s[..., 2] * s[..., 2] + s[..., 3] * s[..., 3]) / np.where(den != 0, den, 1.0), np.nan)


def band_transfer(band_sums):
    """H1 = (re + i im) / xx of band sums [..., 4], NaN where xx is zero"""
    s = np.asarray(band_sums, np.float64)
    xx = s[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(xx != 0, (s[..., 2] + 1j * s[..., 3]) / np.where(xx != 0, xx, 1.0), np.nan + 0j)


def release(bank):
    """free the buffers the read-outs keep with the bank (they go with the bank anyway; the next read-out makes them again)"""
    b, kind = _bank(bank, ("cross", "csm"))
    b._ck(getattr(_lib(), "psdcxr_" + kind + "_release")(b._h))
