"""The definition of include/psdcascade_var.h restated in numpy f64: the reference value of every Var read-out test.  Vectorised, a
plain np.sum, the exact fold with np.fmod.  No library, no device."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
AVAR = dict(x_exp=-2, sinx_exp=4, clip=FLT_MAX, dc_cut=2)
MVAR = dict(x_exp=-4, sinx_exp=6, clip=FLT_MAX, dc_cut=2)
FVAR = dict(x_exp=-2, sinx_exp=4, clip=1.0, dc_cut=2)
# the reference's test vector (src/var.rs): its f32 fold gives REF_F32, the definition REF_F64 (the f32 rounding of pi f tau = 76.3)
REF_P, REF_F, REF_TAU = [1000.0, 100.0, 1.2, 3.4, 5.6], [0.0, 1.0, 3.0, 6.0, 9.0], 2.7
REF_F32, REF_F64 = 0.13478442, 0.134782674


def powi(x, e):
    """square and multiply, 1 / r for a negative exponent"""
    u, r, b = abs(int(e)), np.ones_like(x), x.copy()
    while u:
        if u & 1:
            r = r * b
        b = b * b
        u >>= 1
    return 1.0 / r if e < 0 else r


def limit(f, tau, clip, dc_cut):
    """E: the first e >= dc_cut with !(f[e] <= clip / tau) in f32, or len(f)"""
    f = np.asarray(f, np.float32)
    with np.errstate(over="ignore"):
        lim = np.float32(clip) / np.float32(tau)
    bad = ~(f <= lim)
    bad[:dc_cut] = False
    hit = np.flatnonzero(bad)
    return int(hit[0]) if len(hit) else len(f)


def var_ref(p, f, tau, x_exp=-2, sinx_exp=4, clip=FLT_MAX, dc_cut=2):
    """(var, sum |t|, E) of one row for one tau"""
    p32, f32 = np.asarray(p, np.float32), np.asarray(f, np.float32)
    E = limit(f32, tau, clip, dc_cut)
    if dc_cut >= E:
        return 0.0, 0.0, E
    pe, fe = p32[dc_cut:E].astype(np.float64), f32[dc_cut:E].astype(np.float64)
    with np.errstate(all="ignore"):
        x = fe * np.float64(np.float32(tau))
        w = np.pi * x
        r = np.fmod(x, 2.0)
        neg = r > 1.0
        r = np.where(neg, r - 1.0, r)
        r = np.where(r > 0.5, 1.0 - r, r)
        s = np.sin(np.pi * r)
        s = np.where(neg, -s, s)
        a = ((pe * fe) * fe) * (powi(s, sinx_exp) * powi(w, x_exp))
        t = (a + np.concatenate(([0.0], a[:-1]))) * (fe - np.concatenate(([0.0], fe[:-1])))
        return float(np.sum(t)), float(np.sum(np.abs(t))), E


def tolerance(L, sum_abs):
    """(L + 64) 2^-52 sum |t|: L 2^-53 a side for two differently ordered f64 sums; 64 ulp for two sines of a few ulp each on
    [0, pi/2] raised to at most the 16th power, plus the dozen roundings of a term"""
    return (L + 64) * 2.0 ** -52 * sum_abs


def check(got, p, f, tau, var, what=None):
    """assert one result against the restatement: NaN exactly where it gives NaN, else within the tolerance; returns |error| / tolerance"""
    want, sum_abs, E = var_ref(p, f, tau, **var)
    if np.isnan(want) or np.isnan(got):
        assert np.isnan(want) and np.isnan(got), (what, got, want)
        return 0.0
    tol = tolerance(len(p), sum_abs)
    assert abs(got - want) <= tol, (what, got, want, tol, E)
    return abs(got - want) / tol if tol else 0.0
