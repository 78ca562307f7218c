"""The NumPy twin of the gradient of noisy expected improvement (include/bohip_nei_grad.h) -- TEST INFRASTRUCTURE ONLY.
No device.  One function, the header's formula from nei_reference.Twin's pieces at the twin's precision (float64 or np.longdouble from
the same statements); the functor partials are float64 closed forms (acq_partials' for EI and PI, logei_reference's for LogEI).

WORST_GRAD: the largest |float64 twin - extended twin| gradient component over every input of tests/test_nei_grad_gpu.py at
jitter_rel = 1e-6 (test_nei_grad_host.py test_tolerance_source recomputes it and asserts the stored constants are within 2 x), rounded
up to two digits.  Scale-free: EI in units of s_f max_k e^(-ll_k), PI in units of max_k e^(-ll_k), LogEI relative to
max(1, |ref|_inf) of the candidate.  The device is held to nei_reference.DEVICE_FACTOR = 16 x these.
"""
import math

import numpy as np
from scipy.special import erf

import nei_reference as nr
from logei_reference import logei

WORST_GRAD = {"EI": 1.1e-10, "PI": 1.2e-10, "LogEI": 2.1e-07}   # measured: 1.04e-10, 1.18e-10, 2.04e-07

# The inputs of tests/test_nei_grad_gpu.py.  N = 63 and 65 join nei_reference.NS (k_nei_mix's 64-column tile), R = 129 its RS (the
# 128-candidate tile), S = 15, 16, 17, 65 at N = 129 the contraction's 16-deep step and its padding.
NS, RS, SS = (1, 17, 63, 65, 129, 300), (1, 40, 129, 700), (0, 1, 5, 64)
S_EDGES = (15, 16, 17, 65)
D20 = dict(kern="SEArd", d=20, ll=math.log(2.0), lsig=math.log(3.0), lnoise=-2.0, beta=13.0, N=129, R=40, S=5)   # (synth's y at d = 20 is 13 +- 3)
# EI and PI are EXACTLY 0 where z = (m_s - tau_s) / s is below -38 (PI: -8.3, where 1 + erf cancels), which is where synth's candidates
# lie on these dense designs (the noise-free s^2 reaches 2e-7): up to 100 % of them (se3 N >= 129), whatever the seed or S -- neither
# changes s^2.  There the gradient comparison would say nothing, so EI and PI get candidates of their own, chosen per model so that
# every candidate is live AND the twin's gradient is many device bounds large (test_nei_grad_host.py asserts both); LogEI, finite
# everywhere, keeps synth's own candidates.
#   se3, the weighted handle, d = 20: synth's candidates moved FAR_SHIFT length-scales out of the data's box along the first
#       coordinate, where s^2 is of the order of s_f^2 (near a site of these designs s is 1e-3 and the live zone a few s wide).
#   m32: y = 6 +- 2 under beta = 0, so out of the box z is about -8 and the gradients fall below the bound's resolution (1e-7 bounds at
#       N = 300).  Its candidates lie INSIDE the design instead, on a shell of RING length-scales around the site with the largest
#       posterior mean (the plug-in incumbent), where s is 0.05 - 0.3 and z is O(1): directions by synth's candidates' own offsets.
FAR_SHIFT = 2.5
RING = (0.02, 0.2)


def d20_spec():
    """The widest dimension bucket: nei_reference.data's recipe at d = 20."""
    X, y, Xs = nr.synth(D20["N"], 20, nr.R_MAX, 1000 * 20 + D20["N"])
    return dict(kern="SEArd", X=X, y=y, ll=np.full(20, D20["ll"]), lsig=D20["lsig"], nu=math.exp(2.0 * D20["lnoise"]) + nr.EPS,
                beta=D20["beta"], Xs=Xs[:D20["R"]])


_XS = {}


def spec(tag, acq="LogEI"):
    """The twin's arguments for an input; Xs: the candidates `acq` is compared at (see FAR_SHIFT and RING)."""
    a = dict(d20_spec() if tag == "d20" else nr.spec(tag))
    key = (tag, acq != "LogEI")
    if acq != "LogEI" and key not in _XS:
        Xs, ell = a["Xs"], math.exp(float(np.max(a["ll"])))
        if a["kern"] == "Mat32Iso":
            F0 = nr.twin(tag).fantasies(*nr.normals(nr.SEED, 0, len(a["y"])))[0][0]
            u = Xs - 0.5                                                     # synth's candidates are uniform in the unit box
            r = RING[0] + (RING[1] - RING[0]) * (np.arange(len(Xs)) * 0.6180339887 % 1.0)
            _XS[key] = a["X"][int(np.argmax(F0))] + (r * ell / np.linalg.norm(u, axis=1))[:, None] * u
        else:
            _XS[key] = Xs + (1.0 + FAR_SHIFT * ell) * np.eye(Xs.shape[1])[0]
    if acq != "LogEI":
        a["Xs"] = _XS[key]
    return a


def partials(acq, m, s2, tau):
    """(d/dmu, d/ds2) of the functor, float64, elementwise: acq_partials' closed forms (kernels_score.hip)."""
    m, s2, tau = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (m, s2, tau)))
    if acq == "LogEI":
        return logei(m, s2, tau)[1:]
    with np.errstate(all="ignore"):
        zero = s2 == 0.0
        s = np.sqrt(np.where(zero, 1.0, s2))
        D = m - tau
        z = D / s
        phi = 0.3989422804014327 * np.exp(-0.5 * z * z)
        if acq == "EI":
            Phi = 0.5 * (1.0 + erf(z / math.sqrt(2.0)))
            dmu = np.where(zero, np.where(m > tau, 1.0, 0.0), Phi + D * phi / s - z * phi / s)
            ds2 = np.where(zero, 0.0, (D * phi - z * phi) * (-z / (2.0 * s2)))
        else:
            dmu = np.where(zero, 0.0, phi / s)
            ds2 = np.where(zero, 0.0, phi * (-z / (2.0 * s2)))
    return dmu, ds2


def gradient(t, Xs, alpha, tau, acq):
    """(grad (R, d), score (R,)) of NEI at the rows of Xs for the twin t (its precision), alpha (N, S1), tau (S1)."""
    dt = t.dt
    Xs = np.asarray(Xs, dtype=dt)
    S1 = len(tau)
    m, s2 = t.moments(Xs, alpha)                                             # m (R, S1), s^2 (R)
    Ks = nr.cov(t.kern, t.X, Xs, t.ll, t.lsig, dt)                           # (N, R)
    U = nr.solve_lower_t(t.Ld, nr.solve_lower(t.Ld, Ks))                     # u = W_d'W_d k*
    m64, s64, tau64 = np.asarray(m, dtype=np.float64), np.asarray(s2, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    score, each = nr.score(acq, m64, s64, tau64)
    dmu, ds2 = partials(acq, m64, s64[:, None], tau64[None, :])           # (R, S1)
    with np.errstate(all="ignore"):
        if acq == "LogEI":
            v = each.T                                                       # (R, S1)
            vmax = v.max(axis=1, keepdims=True)
            e = np.where(v == vmax, 1.0, np.exp(v - vmax))
            tot = np.zeros(len(v))
            for s in range(S1):
                tot = tot + e[:, s]
            p = np.where(vmax == -np.inf, 0.0, e / tot[:, None])
        else:
            p = np.full(dmu.shape, 1.0 / S1)
        omega = np.where(p == 0.0, 0.0, p * dmu)
        c = np.zeros(len(omega))
        for s in range(S1):
            c = c + np.where(p[:, s] == 0.0, 0.0, p[:, s] * ds2[:, s])
    c = np.where(s64 > 0.0, c, 0.0)
    E = np.asarray(omega, dtype=dt) @ alpha.T - dt(2.0) * np.asarray(c, dtype=dt)[:, None] * U.T   # (R, N)
    il = np.exp(-np.asarray(t.ll, dtype=dt)) * np.ones(Xs.shape[1], dtype=dt)
    T = Xs[:, None, :] - t.X[None, :, :]                                     # (R, N, d)
    r2 = ((T * il) ** 2).sum(axis=2)
    if t.kern == "SEArd":
        fac = -(t.s2f * np.exp(-r2 / dt(2.0)))
    else:
        fac = -dt(3.0) * t.s2f * np.exp(-np.sqrt(dt(3.0) * r2))
    grad = np.einsum("rn,rnk->rk", fac * E, T) * (il * il)
    return grad, score


_GRADS = {}


def reference(tag, S, acq, dt=np.float64):
    """dict(grad (R, d), score, m, s2, tau, s2f, asum, scale) of one input at all its candidates, computed once and shared."""
    key = (tag, S, acq, dt)
    if key not in _GRADS:
        a = spec(tag, acq)
        if tag == "d20":
            t = nr.Twin(a["kern"], a["X"], a["y"], a["ll"], a["lsig"], a["nu"], a["beta"], nr.JREL, dt)
        else:
            t = nr.twin(tag, nr.JREL, dt)
        mkey = (tag, S, dt)
        if mkey not in _GRADS:
            F, tau, alpha = t.fantasies(*nr.normals(nr.SEED, S, len(t.y)))
            _GRADS[mkey] = (F, tau, alpha)
        F, tau, alpha = _GRADS[mkey]
        grad, score = gradient(t, a["Xs"], alpha, tau, acq)
        m, s2 = t.moments(a["Xs"], alpha)
        _GRADS[key] = dict(grad=grad, score=score, m=m, s2=s2, F=F, tau=tau, s2f=float(t.s2f),
                           asum=float(np.abs(alpha).sum(axis=0).max()), scale=float(np.exp(-np.min(np.asarray(a["ll"], dtype=np.float64)))))
    return _GRADS[key]


def distance(acq, got, ref):
    """max |got - ref| over the components of every candidate (rows), in WORST_GRAD's units; ref: reference()'s dict."""
    g = np.asarray(ref["grad"], dtype=np.float64)
    d = np.abs(np.asarray(got, dtype=np.float64) - g)
    if acq == "LogEI":
        return d.max(axis=1) / np.maximum(1.0, np.abs(g).max(axis=1))
    unit = ref["scale"] * (math.sqrt(ref["s2f"]) if acq == "EI" else 1.0)
    return d.max(axis=1) / unit


def all_inputs():
    """Every (tag, R, S) tests/test_nei_grad_gpu.py compares: the source of WORST_GRAD."""
    out = [((model, N), max(RS), S) for model in nr.MODELS for N in NS for S in SS]
    out += [(("se3", 129), 40, S) for S in S_EDGES]
    out += [("d20", D20["R"], D20["S"]), (("se3", nr.BIG_N, max(nr.BIG_RS)), 300, nr.BIG_S), ("weighted", nr.R_MAX, 5)]
    return out
