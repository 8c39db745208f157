"""numpy restatement of gi_ema_update (csrc/elementwise.hip: ema_kernel) and the bound its tests use.

The kernel, per element, with om = 1.0f - decay formed in fp32:
    diff = p - ema              rounded to fp32
    ema  = fmaf(om, diff, ema)  one rounding
Here the fused multiply-add is formed in float64 and rounded once to float32. om * diff is a product of two 24-bit
significands, exact in float64; adding ema then rounds to 53 bits before the rounding to 24, so the restatement can differ from
the fused instruction by one float32 ulp in rare double-rounding cases. The bound below leaves room for that.

The bound, against the float64 value E = ema + om * (p - ema):
    |out - E| <= 2^-23 * (|E| + om * |p - ema|) + 2^-149
one rounding of diff (relative 2^-24) scaled by om, plus one rounding of the result (relative 2^-24 of |E|), with a factor 2 of
margin, plus the smallest subnormal for results that leave the normal range."""
import numpy as np


def om_of(decay):
    """1 - decay as the host forms it: in float32."""
    return np.float32(1.0) - np.float32(decay)


def ema_update(ema, p, decay):
    ema = np.asarray(ema, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    om = om_of(decay)
    diff = (p - ema).astype(np.float32)
    return (np.float64(om) * diff.astype(np.float64) + ema.astype(np.float64)).astype(np.float32)


def exact(ema, p, decay):
    """E in float64, from the float32 inputs and the float32 om."""
    ema = np.asarray(ema, dtype=np.float32).astype(np.float64)
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    return ema + np.float64(om_of(decay)) * (p - ema)


def bound(ema, p, decay):
    ema64 = np.asarray(ema, dtype=np.float32).astype(np.float64)
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64)
    om = np.float64(om_of(decay))
    return 2.0 ** -23 * (np.abs(exact(ema, p, decay)) + om * np.abs(p64 - ema64)) + 2.0 ** -149


def worst_ratio(out, ema, p, decay):
    """max over the elements of |out - E| / bound: at most 1 when `out` is within the bound."""
    err = np.abs(np.asarray(out, dtype=np.float32).astype(np.float64) - exact(ema, p, decay))
    return float((err / bound(ema, p, decay)).max())
