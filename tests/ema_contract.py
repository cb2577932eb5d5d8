"""The recipe of efgh_ema_update (include/efgh_hip.h) restated in numpy, and the one-step bound its tests hold the kernel to.

    t    Adam's step count (state->applied, or the host's `step`)
    d    (float) min((double) decay_f32, warmup ? (1 + t) / (10 + t) : 1)      float64, rounded once
    omd  1.f - d                                                               one fp32 subtraction
    e    fmaf(omd, w - e, e)                                                   one fp32 subtraction, one fused multiply-add

No tests in this file."""
import numpy as np


def decay_at(decay, warmup, t):
    """the fp32 decay used at step count t"""
    ramp = (1.0 + float(t)) / (10.0 + float(t)) if warmup else 1.0
    return np.float32(min(float(np.float32(decay)), ramp))


def omd_of(d):
    """the fp32 complement the kernel multiplies by (exact for d >= 0.5)"""
    return np.float32(1.0) - np.float32(d)


def update(e, w, d):
    """one update in float64 from fp32 inputs: e + omd * (w - e) with omd the kernel's fp32 complement of d"""
    e64, w64 = np.asarray(e, np.float64), np.asarray(w, np.float64)
    return e64 + float(omd_of(d)) * (w64 - e64)


def bound(e, w, d):
    """|e_gpu - e64| <= 2^-24 (omd |w - e| + |e64|) (1 + 2^-20) + 2^-149: one rounding of w - e (relative 2^-24, scaled by omd in
    the product) and one rounding of the fused multiply-add (relative 2^-24 of the result); the factor covers the second-order
    terms and the last term a denormal result"""
    e64, w64 = np.asarray(e, np.float64), np.asarray(w, np.float64)
    omd = float(omd_of(d))
    return 2.0 ** -24 * (omd * np.abs(w64 - e64) + np.abs(update(e, w, d))) * (1.0 + 2.0 ** -20) + 2.0 ** -149


def inputs(n, seed):
    """(e, w) as fp32: magnitudes 10^U(-20, 18), relative steps 10^U(-8, 1), with +-0 and denormals scattered in"""
    rs = np.random.RandomState(seed)
    with np.errstate(over='ignore'):
        e = (rs.standard_normal(n) * 10.0 ** rs.uniform(-20, 18, n)).astype(np.float32)
        w = (e.astype(np.float64) * (1.0 + rs.standard_normal(n) * 10.0 ** rs.uniform(-8, 1, n))).astype(np.float32)
    w[~np.isfinite(w)] = 0.0
    for arr, off in ((e, 0), (w, 3)):
        k = np.arange(n)
        arr[(k + off) % 11 == 0] = 0.0
        arr[(k + off) % 13 == 0] = -0.0
        arr[(k + off) % 17 == 0] = np.float32(1e-41) * np.where(k[(k + off) % 17 == 0] % 2, 1, -1).astype(np.float32)
    return e, w
