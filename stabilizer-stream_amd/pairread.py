"""Bank read-out on the device for the pair carrier objects (include/ext/psdcascade_pairread.h, psdcpr_*): the stitched auto and cross
spectra of both sides of every selected pair of a ZoomCsdCascadeBank, IqCsdCascadeBank, ZoomAmPmCsdCascadeBank or
IqAmPmCsdCascadeBank (or of their single objects) with, when asked, their frequencies, coherence, H1 and the sums of up to 8
frequency bands; for the AM/PM cross banks the carriers, cab, cba, the four AM/PM cross spectra and their band integrals, in one
call: one drain, one kernel launch for all pairs, at most one more for the bands.  (The host forms make two C calls: the layout
first, to size their arrays, then the read-out, whose drain finds the pipeline idle.  The device forms and layout are one call each.)

    from stabilizer_stream_amd import pairread
    r = pairread.bank_am_pm_cross(bank, bands=[(1e-4, 1e-2)])   # host arrays; r["band_sums"][p, 0, 1]: integrated cross phase noise
    pairread.bank_csd_device(bank, stride, coh_up=t.data_ptr())  # into a torch tensor [P][stride] f64

For the 8-row banks the f32 rows and the frequencies equal what bank.csd(p) and Break.frequencies return, byte for byte; cab and cba
equal bank.sidebands(p).  The functions take the object; they add nothing to it."""
import ctypes as C

import numpy as np

from .bankread import _BREAK, _CAP, MAX_BANDS, _bands, _Breaks, _CInfo, _pkg  # noqa: F401  (one record layout, one lazy Break list)

_set = False
_CSD, _AMPM = "csd", "ampm"
_ALL = (_CSD, _AMPM)
_CSD_OUTS = ("saa_up", "saa_lo", "sbb_up", "sbb_lo", "sab_up", "sab_lo", "freq", "coh_up", "coh_lo", "h1_up", "h1_lo")
_AMPM_OUTS = ("freq", "cab", "cba", "s_am", "s_pm", "s_am_pm", "s_pm_am", "carrier")


def _lib():
    """the package's library with the prototypes of include/ext/psdcascade_pairread.h set"""
    global _set
    L = _pkg().lib()
    if not _set:
        u32, i, vp, sz = C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
        head = [vp, vp, u32, i, u32, i]  # handle, pairs, n_sel, keep_overlap, min_count, keep_transition_band
        tail = [vp, vp, vp, sz, C.POINTER(_CInfo)]  # lens, n_breaks, breaks, breaks_cap, info
        band = [sz, vp, u32, vp]  # stride, bands, n_bands, band_sums
        for name, args in (("layout", head + tail), ("csd_device", head + [vp] * 11 + band + [vp] + tail), ("csd", head + [vp] * 11 + band + tail),
                           ("ampm_device", head + [vp] * 9 + band + [vp] + tail), ("ampm", head + [vp] * 9 + band + tail), ("release", [vp])):
            fn = getattr(L, "psdcpr_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        _set = True
    return L


def _bank(obj, kinds):
    """(the bank behind `obj`, its family): kinds = the families the call takes"""
    pkg = _pkg()
    singles = (pkg.ZoomCsdCascade, pkg.IqCsdCascade, pkg.ZoomAmPmCsdCascade, pkg.IqAmPmCsdCascade)
    b = obj._b if type(obj) in singles else obj
    # (the exact classes: a subclass may be another object)
    kind = {pkg.ZoomCsdCascadeBank: _CSD, pkg.IqCsdCascadeBank: _CSD, pkg.ZoomAmPmCsdCascadeBank: _AMPM,
            pkg.IqAmPmCsdCascadeBank: _AMPM}.get(type(b))
    if kind not in kinds:
        names = {_CSD: "a ZoomCsdCascade[Bank] or IqCsdCascade[Bank]", _AMPM: "a ZoomAmPmCsdCascade[Bank] or IqAmPmCsdCascade[Bank]"}
        raise pkg.PsdError(pkg.ERR_ARG, "this read-out takes " + ", ".join(names[k] for k in kinds))
    return b, kind


class _Call:
    """the arguments every psdcpr_ call shares, and what it returns through them"""

    def __init__(self, obj, pairs, opts, kinds):
        pkg = _pkg()
        self.b, self.kind = _bank(obj, kinds)
        opts = pkg.MergeOpts() if opts is None else opts
        if pairs is None:
            self.sel, self.rows = None, self.b.n_pairs
        else:
            ps = [int(p) for p in pairs]
            if any(not 0 <= p <= pkg.U32_MAX for p in ps):
                raise pkg.PsdError(pkg.ERR_ARG, "pair indices must be in [0, 2^32)")
            self.sel, self.rows = np.zeros(max(1, len(ps)), np.uint32), len(ps)  # (never NULL: that selects every pair)
            self.sel[:len(ps)] = ps
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
        return getattr(_lib(), "psdcpr_" + name)

    def layout(self):
        self.b._ck(self.fn("layout")(*self.head, *self.tail))
        return int(self.info.max_len)

    def carriers(self, carriers):
        """the [P][5] f64 array of the given (p_ab, w, q) (None: the carriers come from bin 0 of stage 0)"""
        if carriers is None:
            return None
        rows = [(float(c[0]), complex(c[1]), complex(c[2])) for c in carriers]
        if len(rows) != self.rows:
            raise _pkg().PsdError(_pkg().ERR_ARG, "carriers: one (p_ab, w, q) a selected pair")
        return np.ascontiguousarray(np.array([(p, w.real, w.imag, q.real, q.imag) for p, w, q in rows], np.float64).reshape(-1, 5))

    def result(self):
        return {"lens": self.lens[:self.rows].tolist(), "breaks": _Breaks(self.br, self.nb[:self.rows].tolist()),
                "launches": int(self.info.launches)}


def _ptr(p):
    return C.c_void_p(p) if p else None


def _host(a):
    return a.ctypes.data if a is not None else None


def layout(bank, pairs=None, opts=None):
    """dict(lens, breaks, max_len) of the selected pairs of any of the four banks or single objects (None: all, in order; else
    indices in any order, duplicates allowed): per pair the stitched length and the list of Break that csd(pair, opts) returns
    (`breaks` reads like a list of lists; the Break objects are made when it is first indexed).  Drains the bank; launches nothing."""
    c = _Call(bank, pairs, opts, _ALL)
    width = c.layout()
    r = c.result()
    return {"lens": r["lens"], "breaks": r["breaks"], "max_len": width}


def bank_csd(bank, pairs=None, opts=None, frequencies=False, coherence=False, transfer=False, bands=None):
    """dict(saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, lens, breaks, launches) of the selected pairs of any of the four banks:
    float32 [P][max_len] (sab complex64), row i holding lens[i] values and NaN behind them.  frequencies=True adds `frequencies`;
    coherence=True adds `coherence_up`, `coherence_lo` (float64, from the f64 accumulators); transfer=True adds `transfer_up`,
    `transfer_lo` (complex128, H1 = S_ab / S_aa a side); bands=[(lo, hi), ...] (at most 8, in cycles per sample from the carrier) adds
    `band_sums` float64 [P][n_bands][8]: the trapezoidal integrals of the eight stitched f32 rows (S_aa up, lo; S_bb up, lo; Re S_ab
    up, lo; Im S_ab up, lo) over the bins whose frequency lies in [lo, hi]."""
    c = _Call(bank, pairs, opts, _ALL)
    width = c.layout()
    shape = (c.rows, width)
    out = {k: np.full(shape, np.nan, np.float32) for k in _CSD_OUTS[:4]}
    out["sab_up"], out["sab_lo"] = (np.full(shape, np.nan, np.complex64) for _ in range(2))
    if frequencies:
        out["frequencies"] = np.full(shape, np.nan, np.float32)
    if coherence:
        out["coherence_up"], out["coherence_lo"] = np.full(shape, np.nan), np.full(shape, np.nan)
    if transfer:
        out["transfer_up"], out["transfer_lo"] = (np.full(shape, np.nan, np.complex128) for _ in range(2))
    ba, nb = _bands(bands)
    if ba is not None:
        out["band_sums"] = np.zeros((c.rows, nb, 8), np.float64)
    if width:  # (else no selected pair has an included stage: nothing to launch, the band sums are 0.0)
        keys = _CSD_OUTS[:6] + ("frequencies", "coherence_up", "coherence_lo", "transfer_up", "transfer_lo")
        c.b._ck(c.fn("csd")(*c.head, *(_host(out.get(k)) for k in keys), width, _host(ba) if nb else None, nb,
                            out["band_sums"].ctypes.data if nb else None, *c.tail))
    return {**out, **c.result()}


def bank_csd_device(bank, stride, saa_up=None, saa_lo=None, sbb_up=None, sbb_lo=None, sab_up=None, sab_lo=None, freq=None, coh_up=None,
                    coh_lo=None, h1_up=None, h1_lo=None, pairs=None, opts=None, bands=None, band_ptr=None, done_event=None):
    """bank_csd() written into device memory: the outputs are device addresses (tensor.data_ptr()) of rows of `stride` bins -- saa_*,
    sbb_*, freq float32; sab_* float32 (re, im) pairs; coh_* float64; h1_* float64 pairs -- any may be None; row i receives lens[i]
    bins, the rest of the row is left as it is.  band_ptr is a device address of float64 [P][n_bands][8] (with bands).  done_event:
    None -- the call returns when the kernels have completed -- or a hipEvent_t handle: it is recorded behind the kernels on the
    bank's stream and the call returns without waiting.  Returns dict(lens, breaks, launches)."""
    c = _Call(bank, pairs, opts, _ALL)
    ba, nb = _bands(bands)
    outs = (saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, freq, coh_up, coh_lo, h1_up, h1_lo)
    c.b._ck(c.fn("csd_device")(*c.head, *(_ptr(p) for p in outs), int(stride), _host(ba) if nb else None, nb, _ptr(band_ptr),
                               _ptr(done_event), *c.tail))
    return c.result()


def bank_am_pm_cross(bank, pairs=None, carriers=None, opts=None, frequencies=False, bands=None):
    """dict(cab, cba, s_am, s_pm, s_am_pm, s_pm_am, carrier, lens, breaks, launches) of the selected pairs of a
    ZoomAmPmCsdCascadeBank / IqAmPmCsdCascadeBank: complex128 [P][max_len], cab and cba what sidebands(p) returns, the four AM/PM
    cross spectra what am_pm_cross(p) returns, NaN behind each row's length; carrier float64 [P][7] = (p_ab, re w, im w, re q, im q,
    lock_w, lock_q) as carriers(p) returns them.  carriers: None -- each pair's carriers are read on the device from bin 0 of stage 0
    (Detrend.NONE only) -- or one (p_ab, w, q) a selected pair, what am_pm_cross(p, carriers=...) takes (the locks are then NaN).  A
    pair without carriers (never fed, all zeros) has the carrier (0, NaN x 6) and NaN in its AM/PM rows.  bands adds `band_sums`
    complex128 [P][n_bands][4] = the integrals of s_am, s_pm, s_am_pm, s_pm_am; [..., 1] is the integrated cross-correlated phase
    noise in rad^2."""
    c = _Call(bank, pairs, opts, (_AMPM,))
    ca = c.carriers(carriers)
    width = c.layout()
    shape = (c.rows, width)
    out = {k: np.full(shape, np.nan, np.complex128) for k in _AMPM_OUTS[1:7]}
    if frequencies:
        out["frequencies"] = np.full(shape, np.nan, np.float32)
    out["carrier"] = np.full((c.rows, 7), np.nan)
    ba, nb = _bands(bands)
    sums = np.zeros((c.rows, nb, 4), np.complex128) if ba is not None else None
    keys = ("frequencies",) + _AMPM_OUTS[1:]
    c.b._ck(c.fn("ampm")(*c.head, _host(ca), *(_host(out.get(k)) for k in keys), width, _host(ba) if nb else None, nb,
                         sums.ctypes.data if nb else None, *c.tail))
    if sums is not None:
        out["band_sums"] = sums
    return {**out, **c.result()}


def bank_am_pm_cross_device(bank, stride, freq=None, cab=None, cba=None, s_am=None, s_pm=None, s_am_pm=None, s_pm_am=None, carrier=None,
                            pairs=None, carriers=None, opts=None, bands=None, band_ptr=None, done_event=None):
    """bank_am_pm_cross() written into device memory: cab, cba and the four AM/PM rows are device addresses of float64 (re, im) rows
    of `stride` bins, freq of float32 rows, carrier of float64 [P][7], band_ptr of float64 [P][n_bands][8]; `carriers` stays a host
    sequence; the rest as bank_csd_device"""
    c = _Call(bank, pairs, opts, (_AMPM,))
    ca = c.carriers(carriers)
    ba, nb = _bands(bands)
    outs = (freq, cab, cba, s_am, s_pm, s_am_pm, s_pm_am, carrier)
    c.b._ck(c.fn("ampm_device")(*c.head, _host(ca), *(_ptr(p) for p in outs), int(stride), _host(ba) if nb else None, nb, _ptr(band_ptr),
                                _ptr(done_event), *c.tail))
    return c.result()


def band_coherence(band_sums):
    """(coherence upper, coherence lower) of band sums [..., 8] of bank_csd: (re^2 + im^2) / (aa bb) a side, NaN where the
    denominator is zero"""
    s = np.asarray(band_sums, np.float64)
    out = []
    for side in (0, 1):
        den = s[..., side] * s[..., 2 + side]
        with np.errstate(divide="ignore", invalid="ignore"):
            num = s[..., 4 + side] * s[..., 4 + side] + s[..., 6 + side] * s[..., 6 + side]
            out.append(np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan))
    return tuple(out)


def release(bank):
    """free the buffers the read-outs keep with the bank (they go with the bank anyway; the next read-out makes them again)"""
    b, _ = _bank(bank, _ALL)
    b._ck(_lib().psdcpr_release(b._h))
