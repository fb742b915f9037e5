"""Robust read-outs of the waterfall cascades (include/psdcascade_robust.h, psdcx_*): per bin the median, the minimum, the maximum
and the spectral-kurtosis-excised mean over a stage's newest complete blocks, computed on the device from the ring in one launch.

    from stabilizer_stream_amd import robust
    r = robust.stage_robust(wf, stage=0, sk_limits=robust.sk_limits(wf.block))
    psd, breaks = robust.robust_psd(wf, kind="median")

`wf` is a WaterfallCascade, ZoomWaterfallCascade or one of their banks.  The functions take the object; they add nothing to it."""
import ctypes as C
import sys

import numpy as np

MAX_ROWS = 4096  # PSDCX_ROBUST_MAX_ROWS
KINDS = ("median", "min", "max", "excised")
_OUTPUTS = KINDS + ("kept",)


class _CRobustInfo(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("block", C.c_uint32), ("first_block", C.c_uint64), ("last_block", C.c_uint64)]


def _pkg():
    return sys.modules[__name__.rpartition(".")[0]]


_set = False


def _lib():
    """the package's library with the four prototypes of include/psdcascade_robust.h set"""
    global _set
    L = _pkg().lib()
    if not _set:
        u32, dbl, vp = C.c_uint32, C.c_double, C.c_void_p
        for name in ("psdcx_wf_robust", "psdcx_wf_robust_device", "psdcx_zwf_robust", "psdcx_zwf_robust_device"):
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = [vp, u32, u32, u32, dbl, dbl, vp, vp, vp, vp, vp, C.POINTER(_CRobustInfo)]
        _set = True
    return L


def _bank(wf):
    """(the bank behind a cascade or the bank itself, whether it is a zoom object)"""
    pkg = _pkg()
    b = wf._b if isinstance(wf, pkg.WaterfallCascade) else wf
    if not isinstance(b, pkg.WaterfallCascadeBank):
        raise pkg.PsdError(pkg.ERR_ARG, "robust read-outs take a WaterfallCascade, a ZoomWaterfallCascade or one of their banks")
    return b, isinstance(b, pkg.ZoomWaterfallCascadeBank)


def _shape(b, zoom):
    return (2, b.n // 2 + 1) if zoom else (b.n // 2 + 1,)


def _call(wf, stage, channel, max_rows, limits, ptrs, device):
    pkg = _pkg()
    b, zoom = _bank(wf)
    cap = MAX_ROWS if max_rows is None else int(max_rows)
    if not 0 <= cap <= pkg.U32_MAX or not 0 <= int(stage) <= pkg.U32_MAX or not 0 <= int(channel) <= pkg.U32_MAX:
        raise pkg.PsdError(pkg.ERR_ARG, "max_rows, stage and channel must be in [0, 2^32)")
    lo, hi = (float("nan"), float("nan")) if limits is None else (float(limits[0]), float(limits[1]))
    fn = getattr(_lib(), ("psdcx_zwf_robust" if zoom else "psdcx_wf_robust") + ("_device" if device else ""))
    info = _CRobustInfo()
    b._ck(fn(b._h, int(channel), int(stage), cap, lo, hi, *(C.c_void_p(ptrs[k]) if ptrs.get(k) else None for k in _OUTPUTS),
             C.byref(info)))
    return {"rows": int(info.rows), "first_block": int(info.first_block), "last_block": int(info.last_block)}


def stage_robust(wf, stage, channel=0, max_rows=None, sk_limits=None):
    """dict(median, min, max, rows, first_block, last_block) over the newest min(max_rows, complete blocks, 4096) complete blocks
    of `stage`, and with sk_limits=(lo, hi) also excised and kept: the mean of the rows whose spectral kurtosis lies in [lo, hi]
    and their number.  Arrays are float32 [n/2 + 1], or [2][n/2 + 1] (upper, lower) of a zoom object, scaled as image() scales a
    complete block; kept is uint32.  With rows == 0 (no complete block yet) the arrays are NaN and kept is 0."""
    b, zoom = _bank(wf)
    names = _OUTPUTS if sk_limits is not None else KINDS[:3]
    out = {k: (np.zeros(_shape(b, zoom), np.uint32) if k == "kept" else np.full(_shape(b, zoom), np.nan, np.float32)) for k in names}
    out.update(_call(wf, stage, channel, max_rows, sk_limits, {k: out[k].ctypes.data for k in names}, False))
    return out


def stage_robust_device(wf, stage, ptrs, channel=0, max_rows=None, sk_limits=None):
    """stage_robust() written into device memory: ptrs maps any of "median", "min", "max", "excised", "kept" to a device address
    (a torch tensor's data_ptr()) of the output's shape, float32 (kept: uint32 / int32).  Outputs left out or None are not
    computed.  Returns dict(rows, first_block, last_block) when the kernel has completed; with rows == 0 nothing is written."""
    unknown = [k for k in ptrs if k not in _OUTPUTS]
    if unknown:
        raise _pkg().PsdError(_pkg().ERR_ARG, f"unknown output {unknown[0]!r} (one of {', '.join(_OUTPUTS)})")
    return _call(wf, stage, channel, max_rows, sk_limits, ptrs, True)


def sk_limits(block, nsigma=3.0):
    """(1 - nsigma sk_sigma(block), 1 + nsigma sk_sigma(block)): the band around the Gaussian value 1 in which a block of `block`
    segments counts as clean.  The real-valued bins 0 and n/2 read 2 for Gaussian noise and fall outside a narrow band."""
    s = _pkg().sk_sigma(block)
    return (1.0 - nsigma * s, 1.0 + nsigma * s)


def median_to_mean(block):
    """The factor that takes the median of a gamma variate of shape `block` to its mean, in the Wilson-Hilferty form
    1 / (1 - 1 / (9 block))^3: multiply a median row by it to read it as a mean of Gaussian noise.  It assumes `block`
    INDEPENDENT segments a row, so it is an approximation for overlapped Hann segments (their equivalent number is smaller)."""
    return 1.0 / (1.0 - 1.0 / (9.0 * float(block))) ** 3


def _gsc(pkg, b, stage):
    """the f32 factor the stitch applies to a stage of count B and this decimation: read from stitch() of a row of ones"""
    ones = np.ones((1, b.n // 2 + 1), np.float32)
    out, _ = pkg.stitch(b.n, [b.block], [pkg.U32_MAX], [0], ones, pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True),
                        window=b._table())
    return np.float32(out[0]) * np.float32(8.0 ** -stage)


def robust_psd(wf, kind="median", channel=0, blocks=None, sk_limits=None, opts=None):
    """(psd, breaks), or (upper, lower, breaks) of a zoom object: the stitched log-resolution spectrum made of every stage's robust
    row `kind` ("median", "min", "max" or "excised", the last with sk_limits) over its newest `blocks` complete blocks (None: all
    the ring holds, 4096 at most).  A stage enters the stitch with the count of one block where it has a complete block and
    with 0 where it has none."""
    pkg = _pkg()
    if kind not in KINDS:
        raise pkg.PsdError(pkg.ERR_ARG, f"kind {kind!r}: one of {', '.join(KINDS)}")
    if kind == "excised" and sk_limits is None:
        raise pkg.PsdError(pkg.ERR_ARG, 'kind "excised" needs sk_limits')
    opts = pkg.MergeOpts() if opts is None else opts
    b, zoom = _bank(wf)
    nsides = 2 if zoom else 1
    ns = b.num_stages(channel)
    counts, avgs, pend = [], [], []
    rows = np.zeros((nsides, max(ns, 1), b.n // 2 + 1), np.float32)
    for k in range(ns):
        r = stage_robust(wf, k, channel, blocks, sk_limits)
        counts.append(b.block if r["rows"] else 0)
        avgs.append(pkg.U32_MAX >> (3 * k) if 3 * k < 32 else 0)
        pend.append(b.stage_blocks(channel, k)["pending"])
        if r["rows"]:
            rows[:, k] = r[kind].reshape(nsides, -1) / _gsc(pkg, b, k)
    out = [pkg.stitch(b.n, counts, avgs, pend, rows[s, :ns], opts, window=b._table()) for s in range(nsides)]
    return (*(o[0] for o in out), out[0][1])
