"""NumPy references of max-value entropy search over a candidate set (include/bohip_mes.h).  No device.

The float64 twin follows the header operation for operation (the device differs from it in exp, erfc, log, log1p -- libm's here --
and in the order in which S(y) adds its R terms):
  terms(mu, s2, m)            u and its two partials, broadcast
  values(mu, var, maxvals)    MES_j and the partials: ascending k from +0.0, one division by K
  record(values)              the arg-max record of bohip_gp_score
  logcdf(g), S(y, mu, var)    the stable log Phi and the sum the quantile search brackets
  quantiles(mu, var)          lo, hi, 14 passes of 16-section -> (y25, y50, y75)
  uniforms(seed, K)           the first uniform of bohip_thompson_normal(seed, k, 0)
  maxvals(mu, var, K, seed, floor)
  quantile_bounds / maxval_bounds   the derived error bounds the tests assert
The extended-precision evaluator (mpmath): mp_u, mp_dudg, mp_root (plain bisection at 50 digits).
"""
import math

import numpy as np
from scipy.special import erfc

C_HALF_LOG_2PI, SQRT2, RSQRT2PI = 0.9189385332046728, 1.4142135623730951, 0.3989422804014327
SWITCH, CF_DEPTH = -4.0, 40
PASSES, PROBES = 14, 15
LOGP = (-1.3862943611198906, -0.6931471805599453, -0.2876820724517809)        # log 0.25, log 0.5, log 0.75
P = (0.25, 0.5, 0.75)
GUMBEL_DEN, LOGLOG2 = 1.5725335836855193, -0.36651292058166435                # log(log 4) - log(log(4/3)), log(log 2)
KMAX, RMAX = 1024, 524288
EPS = np.finfo(np.float64).eps


def _cf(t):
    r = np.zeros_like(t)
    for k in range(CF_DEPTH, 1, -1):
        r = float(k) / (t + r)
    return r, 1.0 / (t + r)


def u_of_gamma(g):
    """(u, du/dgamma, lambda) for an array of finite gamma, in the header's three forms."""
    g = np.asarray(g, dtype=np.float64)
    u, d, lam = np.empty_like(g), np.empty_like(g), np.empty_like(g)
    with np.errstate(all="ignore"):
        pos, mid, deep = g > 0.0, (g <= 0.0) & (g > SWITCH), g <= SWITCH
        x = g[pos]
        phi = RSQRT2PI * np.exp(-0.5 * (x * x))
        Phic = 0.5 * erfc(x / SQRT2)
        l = phi / (1.0 - Phic)
        u[pos] = (x * l) / 2.0 - np.log1p(-Phic)
        d[pos] = -((l / 2.0) * ((1.0 + x * x) + x * l))
        lam[pos] = l
        x = g[mid]
        phi = RSQRT2PI * np.exp(-0.5 * (x * x))
        Phi = 0.5 * erfc(-x / SQRT2)
        l = phi / Phi
        u[mid] = (x * l) / 2.0 - np.log(Phi)
        d[mid] = -((l / 2.0) * ((1.0 + x * x) + x * l))
        lam[mid] = l
        t = -g[deep]
        r, c1 = _cf(t)
        l = t + c1
        u[deep] = (C_HALF_LOG_2PI + np.log(l)) - (0.5 * t) * c1
        d[deep] = -((l / 2.0) * (r * c1))
        lam[deep] = l
    return u, d, lam


def terms(mu, s2, m):
    """u(mu, s2, m), du/dmu, du/ds2, broadcast over the three arguments."""
    mu, s2, m = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (mu, s2, m)))
    u = np.full(mu.shape, np.nan)
    dmu, ds2 = u.copy(), u.copy()
    with np.errstate(all="ignore"):
        ok = np.isfinite(mu) & np.isfinite(s2) & np.isfinite(m) & (s2 >= 0.0)
        zero = ok & (s2 == 0.0)
        u[zero], dmu[zero], ds2[zero] = 0.0, 0.0, 0.0
        live = ok & ~zero
        sd = np.sqrt(s2[live])
        g = (m[live] - mu[live]) / sd
        uu, d, _ = u_of_gamma(g)
        u[live] = uu
        dmu[live] = (-d) / sd
        ds2[live] = ((-d) * g) / (2.0 * s2[live])
    return u, dmu, ds2


def values(mu, var, maxvals):
    """MES_j and its partials in mu_j and s2_j."""
    mu, var = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
    mv = np.asarray(maxvals, dtype=np.float64).ravel()
    su, sa, sb = np.zeros(mu.size), np.zeros(mu.size), np.zeros(mu.size)
    for m in mv:
        u, a, b = terms(mu, var, m)
        su, sa, sb = su + u, sa + a, sb + b
    K = float(mv.size)
    return su / K, sa / K, sb / K


def record(vals):
    """bohip_gp_score's arg-max: first maximum under strict '>' from -Inf, NaN never wins, (-Inf, -1) if nothing can win."""
    v = np.asarray(vals, dtype=np.float64)
    ok = v > -np.inf                                                          # False for NaN
    if not ok.any():
        return -math.inf, -1
    best = np.max(v[ok])
    return float(best), int(np.flatnonzero(ok & (v == best))[0])


def logcdf(g):
    g = np.asarray(g, dtype=np.float64)
    out = np.empty_like(g)
    with np.errstate(all="ignore"):
        pos, mid, deep = g > 0.0, (g <= 0.0) & (g > SWITCH), g <= SWITCH
        out[pos] = np.log1p(-(0.5 * erfc(g[pos] / SQRT2)))
        out[mid] = np.log(0.5 * erfc(-g[mid] / SQRT2))
        t = -g[deep]
        _, c1 = _cf(t)
        out[deep] = (-0.5 * (g[deep] * g[deep]) - C_HALF_LOG_2PI) - np.log(t + c1)
    return out


def _split(mu, var):
    mu, var = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        ok = np.isfinite(mu) & np.isfinite(var) & (var >= 0.0)
    mu, var = mu[ok], var[ok]
    flat = var == 0.0
    return mu[~flat], np.sqrt(var[~flat]), mu[flat]


def S(y, mu, var):
    """sum_j log Phi((y - mu_j) / sigma_j) over the finite candidates; s2 == 0 adds 0 when y >= mu_j and -Inf otherwise."""
    m, sd, point = _split(mu, var)
    if point.size and not np.all(y >= point):
        return -math.inf
    return float(np.sum(logcdf((y - m) / sd))) if m.size else 0.0


def bracket(mu, var):
    """lo = max_j (mu_j - 5 sigma_j), hi = max_j (mu_j + 5 sigma_j) over the finite candidates ((-Inf, -Inf) if there is none)."""
    m, sd, point = _split(mu, var)
    m, s5 = np.concatenate([m, point]), np.concatenate([5.0 * sd, np.zeros(point.size)])
    if m.size == 0:
        return -math.inf, -math.inf
    return float(np.max(m - s5)), float(np.max(m + s5))


def quantiles(mu, var):
    """(y25, y50, y75) by the header's search, and the first bracket (lo, hi)."""
    lo0, hi0 = bracket(mu, var)
    if hi0 == lo0:
        return np.array([lo0, lo0, lo0]), (lo0, hi0)
    m, sd, point = _split(mu, var)
    pmax = float(np.max(point)) if point.size else -math.inf
    out = []
    for logp in LOGP:
        lo, hi = lo0, hi0
        for _ in range(PASSES):
            ys = np.array([lo + (hi - lo) * float(i) / 16.0 for i in range(PROBES + 2)])      # [0] = lo ... [16]: unused
            s = np.array([(-math.inf if ys[i] < pmax else float(np.sum(logcdf((ys[i] - m) / sd)))) for i in range(1, PROBES + 1)])
            hit = np.flatnonzero(s >= logp)
            first = int(hit[0]) if hit.size else PROBES                       # s[i] belongs to probe i + 1
            new_hi = ys[first + 1] if first < PROBES else hi
            new_lo = lo if first == 0 else ys[first]
            lo, hi = float(new_lo), float(new_hi)
        out.append(lo + 0.5 * (hi - lo))
    return np.array(out), (lo0, hi0)


_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def uniforms(seed, K):
    """u_k, the first uniform of bohip_thompson_normal(seed, k, 0)."""
    out = np.empty(K)
    for k in range(K):
        h = _splitmix64((seed & _M64) ^ _splitmix64((k * 0xD1B54A32D192ED03) & _M64))
        out[k] = (float(h >> 11) + 1.0) * (1.0 / 9007199254740993.0)
    return out


def maxvals(mu, var, K, seed, floor=-math.inf):
    """(quantiles, maxvals) of mode BOHIP_MES_GUMBEL."""
    q, (lo0, hi0) = quantiles(mu, var)
    if hi0 == lo0:
        m = np.full(K, lo0)
    else:
        b = (q[2] - q[0]) / GUMBEL_DEN
        a = q[1] + b * LOGLOG2
        m = a - b * np.log(-np.log(uniforms(seed, K)))
    return q, np.where(m > floor, m, floor)


def S_prime(y, mu, var):
    """dS/dy = sum_j lambda_j / sigma_j at y."""
    m, sd, _ = _split(mu, var)
    _, _, lam = u_of_gamma((y - m) / sd)
    return float(np.sum(lam / sd))


def quantile_bounds(mu, var, roots):
    """Per quantile: 2 (hi - lo) 16^-14 (the final bracket, and one probe's worth of a misjudged comparison) + 4 eps |root| (the
    probes' own rounding) + (R + 16) eps (-log p) / S'(root) (the rounding of the sum: every term is <= 0, so sum |terms| = -log p
    at the root, moved to y through the slope)."""
    lo0, hi0 = bracket(mu, var)
    R = np.asarray(mu).size
    return np.array([2.0 * (hi0 - lo0) * 16.0 ** -PASSES + 4.0 * EPS * abs(r) + (R + 16) * EPS * (-lp) / S_prime(r, mu, var)
                     for r, lp in zip(roots, LOGP)])


def maxval_bounds(qb, seed, K, m):
    """The quantile bounds carried through a = y50 + b log log 2, b = (y75 - y25) / 1.5725 and m = a - b log(-log u)."""
    g = np.abs(np.log(-np.log(uniforms(seed, K))))
    return qb[1] + (qb[0] + qb[2]) / 1.5725 * (0.3665 + g) + 8.0 * EPS * np.abs(m)


# ---- extended precision ---------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath

    return mpmath


def mp_logcdf(x):
    """log Phi(x); for x > 0 as log1p(-Phi(-x)): log(ncdf(x)) returns 0 beyond x ~ 15 even at 60 digits."""
    mp = _mp()
    return mp.log1p(-mp.ncdf(-x)) if x > 0 else mp.log(mp.ncdf(x))


def _mp_u(g):
    mp = _mp()
    Phi = 1 - mp.ncdf(-g) if g > 0 else mp.ncdf(g)
    return g * (mp.npdf(g) / Phi) / 2 - mp_logcdf(g)


def mp_u(g, dps=60):
    """u(gamma) = gamma lambda / 2 - log Phi(gamma), lambda = phi / Phi, as written, at `dps` digits."""
    mp = _mp()
    with mp.workdps(dps):
        return _mp_u(mp.mpf(g))


def mp_dudg(g, dps=60):
    """du/dgamma by mpmath's numerical differentiation of mp_u (the step and the working precision are its own)."""
    mp = _mp()
    with mp.workdps(dps):
        return mp.diff(_mp_u, mp.mpf(g))


def mp_root(mu, var, p, lo, hi, dps=50):
    """The root of S(y) = log p in [lo, hi] by plain bisection at `dps` digits (candidates with s2 > 0 only)."""
    mp = _mp()
    m, sd, point = _split(mu, var)
    assert point.size == 0
    with mp.workdps(dps):
        mm, ss = [mp.mpf(float(v)) for v in m], [mp.mpf(float(v)) for v in sd]
        target = mp.log(mp.mpf(p))
        f = lambda y: mp.fsum(mp_logcdf((y - a) / b) for a, b in zip(mm, ss)) - target   # noqa: E731
        lo, hi = mp.mpf(lo), mp.mpf(hi)
        assert f(lo) < 0 < f(hi)
        while hi - lo > mp.mpf(10) ** (-(dps - 12)) * max(1, abs(hi)):
            mid = (lo + hi) / 2
            if f(mid) < 0:
                lo = mid
            else:
                hi = mid
        return (lo + hi) / 2
