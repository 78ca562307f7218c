"""NumPy twin of csrc/acq_log.h: LogEI, the logarithm of the textbook expected improvement, and its partials --
the same two branches, the same continued-fraction depth, the same operation order.  Arrays in, arrays out."""
import numpy as np
from scipy.special import erfc

LOGEI_SWITCH = -4.0
LOGEI_CF_DEPTH = 40
INV_SQRT_2PI = 0.3989422804014327
SQRT2 = 1.4142135623730951
HALF_LOG_2PI = 0.9189385332046728

# Tolerances.  WORST: this twin's worst error over tests/golden/logei_table.npz against the 80-digit reference,
# |d| / |ref| for the partials and |d| / max(|ref|, 1) for the value (which crosses 0 where EI = 1), rounded up to two digits.  All
# three maxima sit in the direct branch next to the switch, z in (-4, -3.5], where h = phi + z Phi cancels ~20-fold and the rounding
# of z^2 inside exp alone contributes ~1e-14; the continued-fraction branch stays within 1.1e-15 (value) and 3.9e-16 (partials).
# The host test bounds the twin by 2 x WORST, the device test bounds the kernels by 8 x WORST (OCML's erfc / exp / log differ
# from libm by a few ulp, amplified the same ~20-fold).
WORST = {"value": 2.4e-14, "dmu": 3.5e-14, "ds2": 3.3e-14}
SLACK_PRUNE = 2.0 ** -38   # k_prune_bound: ub = f + SLACK_PRUNE (1 + |f|)


def tolerance(name, ref, factor):
    """|d| <= rtol |ref| + atol with rtol = factor x WORST; atol = rtol for the value where |ref| < 1, else 0."""
    rtol = factor * WORST[name]
    ref = np.asarray(ref, dtype=np.float64)
    atol = np.where(np.abs(ref) < 1.0, rtol, 0.0) if name == "value" else 0.0
    with np.errstate(invalid="ignore"):
        return rtol * np.abs(ref) + atol


def assert_close(name, got, ref, factor, what=""):
    """Rows whose reference is not finite (-inf value, an overflowing partial) must match exactly; the rest within tolerance()."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), (what, name, "non-finite rows differ")
    err = np.abs(got[fin] - ref[fin])
    tol = tolerance(name, ref[fin], factor)
    bad = ~(err <= tol)
    assert not bad.any(), (what, name, int(bad.sum()), float(np.nanmax(err / np.maximum(tol, 1e-300))), got[fin][bad][:3], ref[fin][bad][:3])
    return float(np.max(err / np.maximum(np.abs(ref[fin]), 1.0 if name == "value" else 1e-300))) if err.size else 0.0


def logei_parts(z):
    """(log h, Phi / h, phi / h) of h(z) = phi(z) + z Phi(z)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    logh, Phi_h, phi_h = np.empty_like(z), np.empty_like(z), np.empty_like(z)
    with np.errstate(all="ignore"):
        hi = z > LOGEI_SWITCH
        zz = z[hi]
        phi = INV_SQRT_2PI * np.exp(-0.5 * (zz * zz))
        Phi = 0.5 * erfc(-zz / SQRT2)
        h = phi + zz * Phi
        logh[hi], Phi_h[hi], phi_h[hi] = np.log(h), Phi / h, phi / h
        lo = ~hi
        zz = z[lo]
        t = -zz
        r = np.zeros_like(t)
        for k in range(LOGEI_CF_DEPTH, 1, -1):
            r = float(k) / (t + r)
        tr = t + r
        c1 = 1.0 / tr
        tc = t + c1
        logh[lo] = -0.5 * (zz * zz) - HALF_LOG_2PI + np.log(c1 / tc)
        Phi_h[lo] = tr
        phi_h[lo] = tc * tr
    return logh, Phi_h, phi_h


def logei(mu, s2, tau):
    """value, d/dmu, d/ds2 at (mu, s2) for the incumbent tau (scalar or array)."""
    mu, s2, tau = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64),
                                      np.asarray(tau, dtype=np.float64))
    shape = mu.shape
    mu, s2, tau = mu.ravel(), s2.ravel(), tau.ravel()
    val, dmu, ds2 = np.empty_like(mu), np.empty_like(mu), np.empty_like(mu)
    with np.errstate(all="ignore"):
        zero = s2 == 0.0
        above = mu > tau
        D = np.where(zero & above, mu - tau, 1.0)
        val[zero] = np.where(above, np.log(D), -np.inf)[zero]
        dmu[zero] = np.where(above, 1.0 / D, 0.0)[zero]
        ds2[zero] = 0.0
        nz = ~zero
        s = np.sqrt(s2[nz])
        logh, a, b = logei_parts((mu[nz] - tau[nz]) / s)
        val[nz] = np.log(s) + logh
        dmu[nz] = a / s
        ds2[nz] = b / (2.0 * s2[nz])
    return val.reshape(shape), dmu.reshape(shape), ds2.reshape(shape)
