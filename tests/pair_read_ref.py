"""numpy restatement of the arithmetic of include/ext/psdcascade_pairread.h, in the header's operation order: every product and sum is
one numpy REAL f64 operation (one ufunc each; numpy's complex multiplication and division are never used: their vector loops may
fuse a multiply with an add), so an implementation that rounds each on its own gives these bytes."""
import numpy as np

from carrier_read_ref import job_gsc, placed  # noqa: F401  (the same jobs and f32 scale)

NAN = float("nan")
NO_CARRIER = (0.0, NAN, NAN, NAN, NAN, NAN, NAN)


def scaled(acc, g):
    """(float)acc * gsc: the f32 cast, then one f32 multiply (g: the f32 scale of each element, held as f64)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(acc, np.float64).astype(np.float32) * np.asarray(g, np.float64).astype(np.float32)


def frequencies(breaks):
    """(float)k * rbw, rbw = 1 / (float)(fft_size * decimation)"""
    parts = [np.arange(b.bins.start, b.bins.stop, dtype=np.float32) * (np.float32(1.0) / np.float32(b.fft_size * b.decimation))
             for b in breaks if b.include and len(b.bins)]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def coherence(aa, bb, re_, im):
    """(re^2 + im^2) / (aa bb), NaN where aa bb == 0"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = aa * bb
        return np.where(den != 0, (re_ * re_ + im * im) / den, np.nan)


def transfer(aa, re_, im):
    """[L][2] = (re / aa, im / aa), NaN where aa == 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.where(aa != 0, re_ / aa, np.nan), np.where(aa != 0, im / aa, np.nan)], axis=-1)


def csd_sides(rows, g):
    """dict of what psdcpr_csd writes for stitched accumulator rows [>= 8][L] with the scale g [L]"""
    f = [scaled(rows[r], g) for r in range(8)]
    pair = lambda re_, im: np.stack([re_, im], axis=-1)  # noqa: E731
    return {"saa_up": f[0], "saa_lo": f[1], "sbb_up": f[2], "sbb_lo": f[3], "sab_up": pair(f[4], f[6]), "sab_lo": pair(f[5], f[7]),
            "coh_up": coherence(rows[0], rows[2], rows[4], rows[6]), "coh_lo": coherence(rows[1], rows[3], rows[5], rows[7]),
            "h1_up": transfer(rows[0], rows[4], rows[6]), "h1_lo": transfer(rows[1], rows[5], rows[7]), "f32": f}


def carriers_from_bin0(n, power_f32, count0, a0):
    """(P, wr, wi, qr, qi, lock_w, lock_q) from a0[r] = the raw accumulator of row r at bin 0 of stage 0; NO_CARRIER without an
    average, or with |u| == 0 or |c| == 0"""
    if count0 is None or count0 < 1:
        return NO_CARRIER
    a0 = np.asarray(a0, np.float64)
    ur, ui, cr, ci = a0[4], a0[6], a0[8], a0[9]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu, mc = np.sqrt(ur * ur + ui * ui), np.sqrt(cr * cr + ci * ci)
        if not mu > 0.0 or not mc > 0.0:
            return NO_CARRIER
        n2p = np.float64(n) * np.float64(n) * np.float64(np.float32(power_f32))
        return tuple(float(v) for v in (mu / (np.float64(count0) * n2p), ur / mu, ui / mu, cr / mc, ci / mc,
                                        mu / np.sqrt(a0[0] * a0[2]), mc / np.sqrt(a0[0] * a0[3])))


def carriers_given(p_ab, w, q):
    """(P, w / |w|, q / |q|, NaN, NaN): the magnitudes by hypot, each component divided on its own"""
    w, q = complex(w), complex(q)
    mw, mq = np.hypot(np.float64(w.real), np.float64(w.imag)), np.hypot(np.float64(q.real), np.float64(q.imag))
    return (float(p_ab), float(np.float64(w.real) / mw), float(np.float64(w.imag) / mw), float(np.float64(q.real) / mq),
            float(np.float64(q.imag) / mq), NAN, NAN)


def split(rows, g, car):
    """[L][8] = (re, im) of s_am, s_pm, s_am_pm, s_pm_am from stitched accumulator rows [12][L], the scale g [L] and the carriers
    (the first five values of a record; a record without carriers gives NaN everywhere)"""
    P, wr, wi, qr, qi = (np.float64(v) for v in car[:5])
    if not wr == wr:
        P = np.float64(NAN)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Ur, Lr, Ui, Li = rows[4] * g, rows[5] * g, rows[6] * g, rows[7] * g
        Cr, Ci, Br, Bi = rows[8] * g, rows[9] * g, rows[10] * g, rows[11] * g
        t1r, t1i = Ur * wr + Ui * wi, Ui * wr - Ur * wi
        t2r, t2i = Cr * qr + Ci * qi, Cr * qi - Ci * qr
        t3r, t3i = Br * qr + Bi * qi, Bi * qr - Br * qi
        t4r, t4i = Lr * wr + Li * wi, Lr * wi - Li * wr
        d = np.float64(4.0) * P
        xr, xi = ((t1r - t2r) + t3r) - t4r, ((t1i - t2i) + t3i) - t4i
        yr, yi = ((t1r + t2r) - t3r) - t4r, ((t1i + t2i) - t3i) - t4i
        return np.stack([(((t1r + t2r) + t3r) + t4r) / d, (((t1i + t2i) + t3i) + t4i) / d,
                         (((t1r - t2r) - t3r) + t4r) / d, (((t1i - t2i) - t3i) + t4i) / d,
                         xi / d, np.negative(xr) / d, np.negative(yi) / d, yr / d], axis=-1)


def cross_rows(rows, g):
    """cab, cba [L][2] each: acc * (double)gsc"""
    return np.stack([rows[8] * g, rows[9] * g], axis=-1), np.stack([rows[10] * g, rows[11] * g], axis=-1)


def band_sums(values, freq, bands, threads=256, wave=64):
    """The band sums of csrc/bank_readout.h in its order: values [R][L] f64 (an f32 row cast to f64 is exact), freq [L] f32, bands
    [(lo, hi)] compared in f32.  Thread t adds the trapezoids of the elements t, t + threads, ... in sequence; within a wavefront the
    tree v[l] += v[l + off], off = 32 ... 1; then the wavefronts in order.  Returns [n_bands][R]."""
    values = np.atleast_2d(np.asarray(values, np.float64))
    R, L = values.shape
    f = np.asarray(freq, np.float32)
    f64 = f.astype(np.float64)
    out = np.zeros((len(bands), R))
    if L == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        prev = np.concatenate([np.zeros((R, 1)), values[:, :-1]], axis=1)
        fprev = np.concatenate([[0.0], f64[:-1]])
        tk = (0.5 * (values + prev)) * (f64 - fprev)
        for b, (lo, hi) in enumerate(np.asarray(bands, np.float32).reshape(-1, 2)):
            held = (lo <= f) & (f <= hi)
            acc = np.zeros((R, threads))
            for e0 in range(0, L, threads):  # one step of every thread at a time, in the order each thread adds
                idx = np.arange(e0, min(L, e0 + threads))
                m = held[idx]
                acc[:, idx[m] - e0] = acc[:, idx[m] - e0] + tk[:, idx[m]]
            v = acc.reshape(R, threads // wave, wave).copy()
            off = wave // 2
            while off:
                v[:, :, :off] = v[:, :, :off] + v[:, :, off:2 * off]
                off //= 2
            s = v[:, 0, 0]
            for w in range(1, threads // wave):
                s = s + v[:, w, 0]
            out[b] = s
    return out
