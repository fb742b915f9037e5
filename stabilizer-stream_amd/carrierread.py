"""Bank read-out on the device for the carrier objects (include/psdcascade_carrierread.h, psdczr_*): the stitched sidebands of every
selected channel of a ZoomCascadeBank, IqCascadeBank, ZoomSkCascadeBank, IqSkCascadeBank, ZoomAmPmCascadeBank or IqAmPmCascadeBank
(or of their single-channel objects) with, when asked, their frequencies and the sums of up to 8 frequency bands; for the SK banks
the spectral kurtosis of both sides; for the AM/PM banks the carrier, s_am, s_pm, s_ampm and the band integrals of s_am and s_pm
(integrated amplitude and phase noise), in one call: one drain, one kernel launch for all channels, at most one more for the
bands.  (The host forms make two C calls: the layout first, to size their arrays, then the read-out, whose drain finds the pipeline
idle.  The device forms and layout are one call each.)

    from stabilizer_stream_amd import carrierread
    r = carrierread.bank_am_pm(bank, bands=[(1e-4, 1e-2)])          # host arrays; r["band_sums"][c, 0, 3]: integrated phase noise
    carrierread.bank_sk_device(bank, stride, sk_upper=t.data_ptr()) # into a torch tensor [C][stride] f64

upper, lower and the frequencies equal what bank.psd(c) and Break.frequencies return, byte for byte; sk_upper / sk_lower equal
bank.sk(c).  The functions take the object; they add nothing to it."""
import ctypes as C

import numpy as np

from .bankread import _BREAK, _CAP, MAX_BANDS, _bands, _Breaks, _CInfo, _pkg  # noqa: F401  (one record layout, one lazy Break list)

_set = False
_SIDES, _SK, _AMPM = "sides", "sk", "ampm"


def _lib():
    """the package's library with the prototypes of include/psdcascade_carrierread.h set"""
    global _set
    L = _pkg().lib()
    if not _set:
        u32, i, vp, sz = C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
        head = [vp, vp, u32, i, u32, i]  # handle, channels, n_sel, keep_overlap, min_count, keep_transition_band
        tail = [vp, vp, vp, sz, C.POINTER(_CInfo)]  # lens, n_breaks, breaks, breaks_cap, info
        band = [sz, vp, u32, vp]  # stride, bands, n_bands, band_sums
        for name, args in (("layout", head + tail), ("sides_device", head + [vp] * 3 + band + [vp] + tail), ("sides", head + [vp] * 3 + band + tail),
                           ("sk_device", head + [vp] * 5 + [sz, vp] + tail), ("sk", head + [vp] * 5 + [sz] + tail),
                           ("ampm_device", head + [vp] * 8 + band + [vp] + tail), ("ampm", head + [vp] * 8 + band + tail), ("release", [vp])):
            fn = getattr(L, "psdczr_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        _set = True
    return L


def _bank(obj, kinds):
    """(the bank behind `obj`, its family): kinds = the families the call takes"""
    pkg = _pkg()
    singles = (pkg.ZoomCascade, pkg.IqCascade, pkg.ZoomSkCascade, pkg.IqSkCascade, pkg.ZoomAmPmCascade, pkg.IqAmPmCascade)
    b = obj._b if type(obj) in singles else obj
    # (the exact classes: the waterfall and pair banks are other objects, and a subclass may be one of them)
    kind = {pkg.ZoomCascadeBank: _SIDES, pkg.IqCascadeBank: _SIDES, pkg.ZoomSkCascadeBank: _SK, pkg.IqSkCascadeBank: _SK,
            pkg.ZoomAmPmCascadeBank: _AMPM, pkg.IqAmPmCascadeBank: _AMPM}.get(type(b))
    if kind not in kinds:
        names = {_SIDES: "a ZoomCascade[Bank] or IqCascade[Bank]", _SK: "a ZoomSkCascade[Bank] or IqSkCascade[Bank]",
                 _AMPM: "a ZoomAmPmCascade[Bank] or IqAmPmCascade[Bank]"}
        raise pkg.PsdError(pkg.ERR_ARG, "this read-out takes " + ", ".join(names[k] for k in kinds))
    return b, kind


_ALL = (_SIDES, _SK, _AMPM)


class _Call:
    """the arguments every psdczr_ call shares, and what it returns through them"""

    def __init__(self, obj, channels, opts, kinds):
        pkg = _pkg()
        self.b, self.kind = _bank(obj, kinds)
        opts = pkg.MergeOpts() if opts is None else opts
        if channels is None:
            self.sel, self.rows = None, self.b.n_channels
        else:
            ch = [int(c) for c in channels]
            if any(not 0 <= c <= pkg.U32_MAX for c in ch):
                raise pkg.PsdError(pkg.ERR_ARG, "channel indices must be in [0, 2^32)")
            self.sel, self.rows = np.zeros(max(1, len(ch)), np.uint32), len(ch)  # (never NULL: that selects every channel)
            self.sel[:len(ch)] = ch
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
        return getattr(_lib(), "psdczr_" + name)

    def layout(self):
        self.b._ck(self.fn("layout")(*self.head, *self.tail))
        return int(self.info.max_len)

    def carriers(self, carriers):
        """the [S][2] f64 array of the given complex amplitudes (None: the carriers come from bin 0 of stage 0)"""
        if carriers is None:
            return None
        a = np.atleast_1d(np.asarray(carriers, np.complex128))
        if a.shape != (self.rows,):
            raise _pkg().PsdError(_pkg().ERR_ARG, "carriers: one complex amplitude a selected channel")
        return np.ascontiguousarray(np.stack([a.real, a.imag], axis=1))

    def result(self):
        return {"lens": self.lens[:self.rows].tolist(), "breaks": _Breaks(self.br, self.nb[:self.rows].tolist()),
                "launches": int(self.info.launches)}


def _ptr(p):
    return C.c_void_p(p) if p else None


def _host(a):
    return a.ctypes.data if a is not None else None


def layout(bank, channels=None, opts=None):
    """dict(lens, breaks, max_len) of the selected channels of any of the six banks or single objects (None: all, in order; else
    indices in any order, duplicates allowed): per channel the stitched length and the list of Break that psd(channel, opts)
    returns (`breaks` reads like a list of lists; the Break objects are made when it is first indexed).  Drains the bank; launches
    nothing."""
    c = _Call(bank, channels, opts, _ALL)
    width = c.layout()
    r = c.result()
    return {"lens": r["lens"], "breaks": r["breaks"], "max_len": width}


def _sides(c, width, frequencies):
    shape = (c.rows, width)
    out = {"upper": np.full(shape, np.nan, np.float32), "lower": np.full(shape, np.nan, np.float32)}
    if frequencies:
        out["frequencies"] = np.full(shape, np.nan, np.float32)
    return out


def bank_sides(bank, channels=None, opts=None, frequencies=False, bands=None):
    """dict(upper, lower, lens, breaks, launches) of the selected channels of any of the six banks: float32 [C][max_len], row i
    holding lens[i] values and NaN behind them; frequencies=True adds `frequencies`; bands=[(lo, hi), ...] (at most 8, in cycles per
    sample from the carrier) adds `band_sums` float64 [C][n_bands][2]: the trapezoidal integrals of upper and lower over the bins
    whose frequency lies in [lo, hi]."""
    c = _Call(bank, channels, opts, _ALL)
    width = c.layout()
    out = _sides(c, width, frequencies)
    ba, nb = _bands(bands)
    if ba is not None:
        out["band_sums"] = np.zeros((c.rows, nb, 2), np.float64)
    if width:  # (else no selected channel has an included stage: nothing to launch, the band sums are 0.0)
        c.b._ck(c.fn("sides")(*c.head, out["upper"].ctypes.data, out["lower"].ctypes.data, _host(out.get("frequencies")), width,
                              _host(ba) if nb else None, nb, out["band_sums"].ctypes.data if nb else None, *c.tail))
    return {**out, **c.result()}


def bank_sides_device(bank, stride, upper=None, lower=None, freq=None, channels=None, opts=None, bands=None, band_ptr=None, done_event=None):
    """bank_sides() written into device memory: upper, lower, freq are device addresses (tensor.data_ptr()) of float32 rows of
    `stride` bins, any may be None; row i receives lens[i] bins, the rest of the row is left as it is.  band_ptr is a device address
    of float64 [C][n_bands][2] (with bands).  done_event: None -- the call returns when the kernels have completed -- or a
    hipEvent_t handle: it is recorded behind the kernels on the bank's stream and the call returns without waiting.  Returns
    dict(lens, breaks, launches)."""
    c = _Call(bank, channels, opts, _ALL)
    ba, nb = _bands(bands)
    c.b._ck(c.fn("sides_device")(*c.head, _ptr(upper), _ptr(lower), _ptr(freq), int(stride), _host(ba) if nb else None, nb, _ptr(band_ptr),
                                 _ptr(done_event), *c.tail))
    return c.result()


def bank_sk(bank, channels=None, opts=None, frequencies=False):
    """bank_sides() of a ZoomSkCascadeBank / IqSkCascadeBank (without bands) and `sk_upper`, `sk_lower`: float64 [C][max_len], the
    spectral kurtosis sk(c) returns, NaN where a stage has fewer than two averages or no power, and behind each row's length"""
    c = _Call(bank, channels, opts, (_SK,))
    width = c.layout()
    out = _sides(c, width, frequencies)
    out["sk_upper"], out["sk_lower"] = np.full((c.rows, width), np.nan), np.full((c.rows, width), np.nan)
    if width:
        c.b._ck(c.fn("sk")(*c.head, out["upper"].ctypes.data, out["lower"].ctypes.data, _host(out.get("frequencies")), out["sk_upper"].ctypes.data,
                           out["sk_lower"].ctypes.data, width, *c.tail))
    return {**out, **c.result()}


def bank_sk_device(bank, stride, upper=None, lower=None, freq=None, sk_upper=None, sk_lower=None, channels=None, opts=None, done_event=None):
    """bank_sk() written into device memory: sk_upper and sk_lower are device addresses of float64 rows of `stride` bins; the rest
    as bank_sides_device"""
    c = _Call(bank, channels, opts, (_SK,))
    c.b._ck(c.fn("sk_device")(*c.head, _ptr(upper), _ptr(lower), _ptr(freq), _ptr(sk_upper), _ptr(sk_lower), int(stride), _ptr(done_event),
                              *c.tail))
    return c.result()


def bank_am_pm(bank, channels=None, carriers=None, opts=None, frequencies=False, bands=None):
    """dict(upper, lower, s_am, s_pm, s_ampm, carrier, lens, breaks, launches) of the selected channels of a ZoomAmPmCascadeBank /
    IqAmPmCascadeBank: s_am and s_pm float64 [C][max_len], s_ampm complex128, what am_pm(c) returns, NaN behind each row's length;
    carrier float64 [C][4] = (power, re u, im u, lock) as carrier(c) returns them.  carriers: None -- each channel's carrier is
    read on the device from bin 0 of stage 0 (Detrend.NONE only) -- or one complex amplitude A a selected channel, what
    am_pm(c, carrier=A) takes (lock is then NaN).  A channel without a carrier (never fed, all zeros) has the carrier
    (0, NaN, NaN, NaN) and NaN in its AM/PM rows.  bands adds `band_sums` float64 [C][n_bands][4] = the integrals of upper, lower,
    s_am and s_pm; [..., 3] is the integrated phase noise in rad^2."""
    c = _Call(bank, channels, opts, (_AMPM,))
    ca = c.carriers(carriers)
    width = c.layout()
    out = _sides(c, width, frequencies)
    out["s_am"], out["s_pm"] = np.full((c.rows, width), np.nan), np.full((c.rows, width), np.nan)
    out["s_ampm"] = np.full((c.rows, width), np.nan, np.complex128)
    out["carrier"] = np.full((c.rows, 4), np.nan)
    ba, nb = _bands(bands)
    if ba is not None:
        out["band_sums"] = np.zeros((c.rows, nb, 4), np.float64)
    c.b._ck(c.fn("ampm")(*c.head, _host(ca), out["upper"].ctypes.data, out["lower"].ctypes.data, _host(out.get("frequencies")),
                         out["s_am"].ctypes.data, out["s_pm"].ctypes.data, out["s_ampm"].ctypes.data, out["carrier"].ctypes.data, width,
                         _host(ba) if nb else None, nb, out["band_sums"].ctypes.data if nb else None, *c.tail))
    return {**out, **c.result()}


def bank_am_pm_device(bank, stride, upper=None, lower=None, freq=None, s_am=None, s_pm=None, s_ampm=None, carrier=None, channels=None,
                      carriers=None, opts=None, bands=None, band_ptr=None, done_event=None):
    """bank_am_pm() written into device memory: s_am, s_pm (float64), s_ampm (float64 pairs) are device addresses of rows of
    `stride` bins, carrier of float64 [C][4], band_ptr of float64 [C][n_bands][4]; `carriers` stays a host array; the rest as
    bank_sides_device"""
    c = _Call(bank, channels, opts, (_AMPM,))
    ca = c.carriers(carriers)
    ba, nb = _bands(bands)
    c.b._ck(c.fn("ampm_device")(*c.head, _host(ca), _ptr(upper), _ptr(lower), _ptr(freq), _ptr(s_am), _ptr(s_pm), _ptr(s_ampm), _ptr(carrier),
                                int(stride), _host(ba) if nb else None, nb, _ptr(band_ptr), _ptr(done_event), *c.tail))
    return c.result()


def release(bank):
    """free the buffers the read-outs keep with the bank (they go with the bank anyway; the next read-out makes them again)"""
    b, _ = _bank(bank, _ALL)
    b._ck(_lib().psdczr_release(b._h))
