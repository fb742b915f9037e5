"""Var read-out on the device (include/psdcascade_var.h, psdcv_*): the Allan, modified Allan and main-lobe variance curves of every
selected channel of a PsdCascadeBank (or a PsdCascade) for up to 4096 taus and up to 4 descriptors, in one call: one drain, one
kernel launch that reads the accumulators; no stitched row is written or copied.

    from stabilizer_stream_amd import bankvar
    r = bankvar.bank_var(bank, taus)                                       # AVAR: r["var"] float64 [C][T]
    r = bankvar.bank_var(bank, taus, [bankvar.Var.avar(), bankvar.Var.mvar(), bankvar.Var.fvar()])   # [C][3][T]
    bankvar.bank_var_device(bank, t.data_ptr(), taus)                      # into a torch tensor [C][1][T] f64
    bankvar.rows_var_device(bank, psd.data_ptr(), freq.data_ptr(), stride, lens, taus, t.data_ptr())  # rows already on the device

The rows are phase PSDs with frequencies in cycles per sample, taus are in samples.  With a sample rate fs, Var on (f fs, tau / fs)
and a density per Hz is fs^2 times the result here.  Everything is computed in f64 on the f32 rows (the header states the
definition and how it differs from the reference's f32 fold, which var_eval keeps).  The functions take the object; they add
nothing to it."""
import ctypes as C
import dataclasses
import sys

import numpy as np

from . import bankread

MAX_VARS = 4  # PSDCV_MAX_VARS
MAX_TAUS = 4096  # PSDCV_MAX_TAUS
MAX_EXP = 16  # PSDCV_MAX_EXP
FLT_MAX = float(np.finfo(np.float32).max)
_VAR = np.dtype([("x_exp", "<i4"), ("sinx_exp", "<i4"), ("clip", "<f4"), ("dc_cut", "<u4")])  # psdcv_var


@dataclasses.dataclass(frozen=True)
class Var:
    """the reference's Var: sum over the bins from dc_cut on, while f <= clip / tau, of the trapezoids of
    p f^2 sin(pi f tau)^sinx_exp (pi f tau)^x_exp.  The default is the Allan variance."""
    x_exp: int = -2
    sinx_exp: int = 4
    clip: float = FLT_MAX
    dc_cut: int = 2

    @classmethod
    def avar(cls, dc_cut=2):
        return cls(dc_cut=dc_cut)

    @classmethod
    def mvar(cls, dc_cut=2):
        return cls(x_exp=-4, sinx_exp=6, dc_cut=dc_cut)

    @classmethod
    def fvar(cls, dc_cut=2):
        """the Allan variance of the main lobe alone: f <= 1 / tau"""
        return cls(clip=1.0, dc_cut=dc_cut)


def _pkg():
    return sys.modules[__name__.rpartition(".")[0]]


_set = False


def _lib():
    """the package's library with the prototypes of include/psdcascade_var.h set"""
    global _set
    L = bankread._lib()
    if not _set:
        u32, i, vp, sz = C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
        head = [vp, vp, u32, i, u32, i]  # handle, channels, n_sel, keep_overlap, min_count, keep_transition_band
        what = [vp, u32, vp, u32]  # vars, n_vars, taus, n_taus
        tail = [vp, vp, vp, sz, C.POINTER(bankread._CInfo)]  # lens, n_breaks, breaks, breaks_cap, info
        L.psdcv_bank_var_device.restype = C.c_int
        L.psdcv_bank_var_device.argtypes = head + what + [vp, vp] + tail
        L.psdcv_bank_var.restype = C.c_int
        L.psdcv_bank_var.argtypes = head + what + [vp] + tail
        L.psdcv_rows_var_device.restype = C.c_int
        L.psdcv_rows_var_device.argtypes = [vp, vp, vp, sz, vp, u32] + what + [vp, vp, C.POINTER(bankread._CInfo)]
        _set = True
    return L


def _what(var, taus):
    """(psdcv_var records, float32 taus, whether `var` was one Var)"""
    pkg = _pkg()
    single = var is None or isinstance(var, Var)
    vs = [Var() if var is None else var] if single else list(var)
    rec = np.zeros(max(1, len(vs)), _VAR)
    for k, v in enumerate(vs):
        if not isinstance(v, Var):
            raise pkg.PsdError(pkg.ERR_ARG, "var must be a bankvar.Var or a sequence of them")
        if not (-2 ** 31 <= int(v.x_exp) < 2 ** 31 and -2 ** 31 <= int(v.sinx_exp) < 2 ** 31 and 0 <= int(v.dc_cut) <= pkg.U32_MAX):
            raise pkg.PsdError(pkg.ERR_ARG, "a Var field out of range")
        rec[k] = (int(v.x_exp), int(v.sinx_exp), np.float32(v.clip), int(v.dc_cut))
    t = np.ascontiguousarray(np.asarray(taus, np.float32).reshape(-1))
    return rec, len(vs), t if len(t) else np.zeros(1, np.float32), len(t), single


def bank_var(bank, taus, var=None, channels=None, opts=None):
    """dict(var, lens, breaks, launches) of the selected channels (None: all, in order; else indices in any order, duplicates
    allowed): var is float64 [C][T] for one Var (None: the Allan variance) or [C][V][T] for a sequence of up to 4 (they share one
    sine a term), T = len(taus) <= 4096, taus in samples; lens and breaks describe the stitched rows the variances belong to, as
    bankread.layout returns them.  A channel without an included stage gives 0.0."""
    c = bankread._Call(bank, channels, opts)
    rec, nv, t, nt, single = _what(var, taus)
    buf = np.zeros(max(1, c.rows * nv * nt), np.float64)  # (never NULL: no row or no tau is the library's to judge)
    out = buf[:c.rows * nv * nt].reshape(c.rows, nv, nt)
    c.b._ck(_lib().psdcv_bank_var(*c.head, rec.ctypes.data, nv, t.ctypes.data, nt, buf.ctypes.data, *c.tail))
    return {"var": out[:, 0, :] if single else out, **c.result(), "launches": int(c.info.launches)}


def bank_var_device(bank, out_ptr, taus, var=None, channels=None, opts=None, done_event=None):
    """bank_var() written into device memory: out_ptr is a device address (tensor.data_ptr()) of float64 [C][V][T] (V = 1 for one
    Var); nothing else is written.  done_event: None -- the call returns when the kernel has completed -- or a hipEvent_t handle:
    it is recorded behind the kernel on the bank's stream and the call returns without waiting.  Returns dict(lens, breaks, launches)."""
    c = bankread._Call(bank, channels, opts)
    rec, nv, t, nt, _ = _what(var, taus)
    c.b._ck(_lib().psdcv_bank_var_device(*c.head, rec.ctypes.data, nv, t.ctypes.data, nt, C.c_void_p(out_ptr) if out_ptr else None,
                                         C.c_void_p(done_event) if done_event else None, *c.tail))
    return {**c.result(), "launches": int(c.info.launches)}


def rows_var_device(obj, psd_ptr, freq_ptr, stride, lens, taus, out_ptr, var=None, done_event=None):
    """The same curves from rows that lie on the device already: row i is float32 psd_ptr[i * stride ...) with its frequencies at
    freq_ptr[i * stride ...), lens[i] <= stride elements (what bankread.bank_psd_device, crossread.bank_csd_device or an uploaded
    am_pm() row left there); out_ptr is float64 [len(lens)][V][T].  `obj` (a PsdCascadeBank or PsdCascade) lends its stream and
    tables: the call does not drain it and orders behind a done_event read-out of the same object without a host synchronisation.
    On the output of bank_psd_device it gives bank_var_device's bits.  Returns dict(launches)."""
    pkg = _pkg()
    b = bankread._bank(obj)
    ln = [int(v) for v in lens]
    if any(not 0 <= v <= pkg.U32_MAX for v in ln):
        raise pkg.PsdError(pkg.ERR_ARG, "row lengths must be in [0, 2^32)")
    la = np.zeros(max(1, len(ln)), np.uint32)
    la[:len(ln)] = ln
    rec, nv, t, nt, _ = _what(var, taus)
    info = bankread._CInfo()
    b._ck(_lib().psdcv_rows_var_device(b._h, C.c_void_p(psd_ptr) if psd_ptr else None, C.c_void_p(freq_ptr) if freq_ptr else None, int(stride),
                                       la.ctypes.data, len(ln), rec.ctypes.data, nv, t.ctypes.data, nt, C.c_void_p(out_ptr) if out_ptr else None,
                                       C.c_void_p(done_event) if done_event else None, C.byref(info)))
    return {"launches": int(info.launches)}
