"""Bank read-out on the device (include/psdcascade_readout.h, psdcr_*): the stitched PSD of every selected channel of a
PsdCascadeBank (or a PsdCascade), its frequencies and the integrated power of up to 8 frequency bands a channel, in one call: one
drain, one kernel launch for all rows, at most one more for the bands.  (bank_psd makes two C calls: the layout first, to size its
arrays, then the read-out, whose drain finds the pipeline idle.  bank_psd_device and layout are one call each.)

    from stabilizer_stream_amd import bankread
    r = bankread.bank_psd(bank, frequencies=True, bands=[(1e-4, 1e-3)])      # host arrays
    bankread.bank_psd_device(bank, t.data_ptr(), t.shape[1])                 # into a torch tensor [C][stride] f32

Every PSD value and frequency equals what bank.psd(c) and Break.frequencies return, byte for byte.  The functions take the object;
they add nothing to it."""
import collections.abc
import ctypes as C
import sys

import numpy as np

MAX_BANDS = 8  # PSDCR_MAX_BANDS
_CAP = 16  # MAX_STAGES: no channel has more breaks
# psdc_break as a numpy record (the fields of the package's _CBreak)
_BREAK = np.dtype([("start", "<u8"), ("include", "<u4"), ("count", "<u4"), ("avg", "<u4"), ("_pad", "<u4"), ("bins_start", "<u8"),
                   ("bins_end", "<u8"), ("fft_size", "<u8"), ("decimation", "<u8"), ("pending", "<u8"), ("processed", "<u8")])


class _CInfo(C.Structure):
    _fields_ = [("launches", C.c_uint32), ("jobs", C.c_uint32), ("max_len", C.c_uint64)]


def _pkg():
    return sys.modules[__name__.rpartition(".")[0]]


_set = False


def _lib():
    """the package's library with the prototypes of include/psdcascade_readout.h set"""
    global _set
    L = _pkg().lib()
    if not _set:
        u32, i, vp, sz = C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
        head = [vp, vp, u32, i, u32, i]  # handle, channels, n_sel, keep_overlap, min_count, keep_transition_band
        tail = [vp, vp, vp, sz, C.POINTER(_CInfo)]  # lens, n_breaks, breaks, breaks_cap, info
        L.psdcr_bank_layout.restype = C.c_int
        L.psdcr_bank_layout.argtypes = head + tail
        L.psdcr_bank_psd_device.restype = C.c_int
        L.psdcr_bank_psd_device.argtypes = head + [vp, vp, sz, vp, u32, vp, vp] + tail
        L.psdcr_bank_psd.restype = C.c_int
        L.psdcr_bank_psd.argtypes = head + [vp, vp, sz, vp, u32, vp] + tail
        L.psdcr_release.restype = C.c_int
        L.psdcr_release.argtypes = [vp]
        _set = True
    return L


def _bank(obj):
    pkg = _pkg()
    b = obj._b if isinstance(obj, pkg.PsdCascade) else obj
    if not isinstance(b, pkg.PsdCascadeBank):
        raise pkg.PsdError(pkg.ERR_ARG, "bank read-outs take a PsdCascadeBank or a PsdCascade")
    return b


class _Breaks(collections.abc.Sequence):
    """One list of Break a selected row, read like a list of lists.  The Break objects are made from the C records when a row is
    first asked for: a consumer that wants only the rows on the device does not pay for a few hundred Python objects a call."""

    def __init__(self, records, counts):
        self._rec, self._nb, self._rows = records, counts, None

    def _all(self):
        if self._rows is None:
            Break = _pkg().Break
            self._rows = [[Break(t[0], bool(t[1]), t[2], t[3], range(t[5], t[6]), t[7], t[8], t[9], t[10])
                           for t in self._rec[i * _CAP:i * _CAP + n].tolist()] for i, n in enumerate(self._nb)]
        return self._rows

    def __len__(self):
        return len(self._nb)

    def __getitem__(self, i):
        return self._all()[i]

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(self._all())


class _Call:
    """the arguments every psdcr_ call shares, and what it returns through them"""

    def __init__(self, obj, channels, opts):
        pkg = _pkg()
        self.b = _bank(obj)
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

    def result(self):
        return {"lens": self.lens[:self.rows].tolist(), "breaks": _Breaks(self.br, self.nb[:self.rows].tolist())}


def _bands(bands):
    """(float32 [n_bands][2] or None, n_bands)"""
    if bands is None:
        return None, 0
    a = np.ascontiguousarray(np.asarray(bands, np.float32).reshape(-1, 2))
    return a, a.shape[0]


def layout(bank, channels=None, opts=None):
    """dict(lens, breaks, max_len) of the selected channels (None: all, in order; else indices in any order, duplicates allowed):
    per row the stitched length and the list of Break that psd(channel, opts) returns (`breaks` reads like a list of lists; the
    Break objects are made when it is first indexed).  Drains the bank; launches nothing."""
    c = _Call(bank, channels, opts)
    c.b._ck(_lib().psdcr_bank_layout(*c.head, *c.tail))
    return {**c.result(), "max_len": int(c.info.max_len)}


def bank_psd(bank, channels=None, opts=None, frequencies=False, bands=None):
    """dict(psd, lens, breaks, launches) of the selected channels: psd is float32 [C][max_len] with row i holding lens[i] values and
    NaN behind them, breaks one list of Break a row.  frequencies=True adds `frequencies` (the same shape, NaN behind each row's
    length); bands=[(lo, hi), ...] (at most 8, in cycles per sample) adds `band_power` float64 [C][n_bands]: the trapezoidal
    integral of the row over the bins whose frequency lies in [lo, hi].  (The row width comes from a layout call first: the second
    drain finds the pipeline idle.)"""
    c = _Call(bank, channels, opts)
    L = _lib()
    c.b._ck(L.psdcr_bank_layout(*c.head, *c.tail))
    width = int(c.info.max_len)
    shape = (c.rows, width)
    psd = np.full(shape, np.nan, np.float32)
    freq = np.full(shape, np.nan, np.float32) if frequencies else None
    ba, nb = _bands(bands)
    bp = np.zeros((c.rows, nb), np.float64) if ba is not None else None
    if width:  # (else no selected channel has an included stage: nothing to launch, the band powers are 0.0)
        c.b._ck(L.psdcr_bank_psd(*c.head, psd.ctypes.data, freq.ctypes.data if frequencies else None, width,
                                 ba.ctypes.data if nb else None, nb, bp.ctypes.data if nb else None, *c.tail))
    out = {"psd": psd, **c.result(), "launches": int(c.info.launches)}
    if frequencies:
        out["frequencies"] = freq
    if ba is not None:
        out["band_power"] = bp
    return out


def bank_psd_device(bank, psd_ptr, stride, channels=None, opts=None, freq_ptr=None, bands=None, band_ptr=None, done_event=None):
    """bank_psd() written into device memory.  psd_ptr and freq_ptr are device addresses (tensor.data_ptr()) of float32 rows of
    `stride` elements, either may be None; row i receives lens[i] values, the rest of the row is left as it is.  band_ptr is a
    device address of float64 [C][n_bands] (with bands).  done_event: None -- the call returns when the kernels have completed --
    or a hipEvent_t handle, as the after= arguments of the feeds take it: it is recorded behind the kernels on the bank's stream
    and the call returns without waiting.  Returns dict(lens, breaks, launches)."""
    c = _Call(bank, channels, opts)
    ba, nb = _bands(bands)
    c.b._ck(_lib().psdcr_bank_psd_device(*c.head, C.c_void_p(psd_ptr) if psd_ptr else None, C.c_void_p(freq_ptr) if freq_ptr else None,
                                         int(stride), ba.ctypes.data if nb else None, nb, C.c_void_p(band_ptr) if band_ptr else None,
                                         C.c_void_p(done_event) if done_event else None, *c.tail))
    return {**c.result(), "launches": int(c.info.launches)}


def release(bank):
    """free the buffers the read-outs keep with the bank (they go with the bank anyway; the next read-out makes them again)"""
    b = _bank(bank)
    b._ck(_lib().psdcr_release(b._h))
