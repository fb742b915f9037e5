"""numpy restatement of the arithmetic of include/psdcascade_carrierread.h, in the header's operation order: every product and sum
is one numpy f64 operation (numpy does not fuse), so an implementation that rounds each on its own gives these bytes."""
import numpy as np

NAN = float("nan")


def job_gsc(n, count64, nenbw, power, decimation):
    """the f32 scale of a stage: 1 / (gain * decimation), gain = (float)((n / 2) * count) * nenbw * power, all in f32"""
    gain = np.float32((n // 2) * int(count64)) * np.float32(nenbw) * np.float32(power)
    with np.errstate(divide="ignore"):
        return np.float32(1.0) / (gain * np.float32(decimation))


def placed(acc, breaks, n, counts64, nenbw, power):
    """the f64 accumulators [ns][rows][bins] laid along the stitched row by the Breaks (deepest stage first): ([rows][L], the
    f32 scale of each element as f64 [L], the Break count of each element [L])"""
    parts, g, m = [], [], []
    for i, b in enumerate(breaks):
        if b.include and len(b.bins):
            s = len(breaks) - 1 - i
            parts.append(acc[s][:, b.bins.start:b.bins.stop])
            g.append(np.full(len(b.bins), np.float64(job_gsc(n, counts64[s], nenbw, power, b.decimation))))
            m.append(np.full(len(b.bins), b.count, np.int64))
    if not parts:
        return np.zeros((acc.shape[1] if acc.ndim == 3 else 0, 0)), np.zeros(0), np.zeros(0, np.int64)
    return np.concatenate(parts, axis=1), np.concatenate(g), np.concatenate(m)


def sk(count, s1, s2):
    """M < 2 or s1 == 0: NaN; else (M + 1) / (M - 1) * (M * s2 / (s1 * s1) - 1)"""
    m = np.asarray(count, np.float64)
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0)
    return np.where((np.asarray(count) < 2) | (s1 == 0.0), np.nan, v)


def carrier_from_bin0(n, power_f32, count0, U0, L0, cr0, ci0):
    """(P, ur, ui, lock) from the raw accumulators of bin 0 of stage 0; (0, NaN, NaN, NaN) without an average or with comp[0] == 0"""
    if count0 is None or count0 < 1:
        return 0.0, NAN, NAN, NAN
    cr0, ci0 = np.float64(cr0), np.float64(ci0)
    mag = np.sqrt(cr0 * cr0 + ci0 * ci0)
    if not mag > 0.0:
        return 0.0, NAN, NAN, NAN
    n2p = np.float64(n) * np.float64(n) * np.float64(np.float32(power_f32))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(mag / (np.float64(count0) * n2p)), float(cr0 / mag), float(ci0 / mag), float(mag / np.sqrt(np.float64(U0) * np.float64(L0)))


def carrier_given(A):
    """(P, ur, ui, NaN) of a given complex amplitude: P = re^2 + im^2, u = (A A) / P"""
    re_, im = np.float64(complex(A).real), np.float64(complex(A).imag)
    P = re_ * re_ + im * im
    return float(P), float((re_ * re_ - im * im) / P), float((2.0 * (re_ * im)) / P), NAN


def split(U, L, CR, CI, g, P, ur, ui):
    """(s_am, s_pm, s_ampm complex) of bins with the f64 accumulators U, L, CR, CI and the scale g (the f32 factor as f64)"""
    if not ur == ur:
        P = NAN
    P, ur, ui = np.float64(P), np.float64(ur), np.float64(ui)
    with np.errstate(divide="ignore", invalid="ignore"):
        Us, Ls, cr, ci = U * g, L * g, CR * g, CI * g
        Dr, Di, mean = cr * ur + ci * ui, ci * ur - cr * ui, 0.5 * (Us + Ls)
        x = np.empty(np.shape(mean), np.complex128)  # (filled part by part: a product with 1j would turn an infinity into NaN)
        x.real, x.imag = Di / (2.0 * P), (Ls - Us) / (4.0 * P)
        return (mean + Dr) / (2.0 * P), (mean - Dr) / (2.0 * P), x
