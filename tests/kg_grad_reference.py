"""The NumPy twin of the knowledge gradient at free points and its gradient (include/bohip_kg_grad.h) -- TEST
INFRASTRUCTURE ONLY.  No device.  The header's definition from the posterior's pieces at the twin's precision (float64 or np.longdouble
from the same statements); the value is kg_reference.kg_march's on the float64 lines.

WORST_GRAD: the largest distance (nei_grad_reference.distance's measure: max component error of a point in units of
s_f max_k e^(-ll_k)) between the float64 twin and the extended twin over every input of tests/test_kg_grad_gpu.py, rounded up to two
digits (test_kg_grad_host.py test_tolerance_source recomputes it and asserts the stored constant is within 2 x).  The device is held to
nei_reference.DEVICE_FACTOR = 16 x it.  The point x = a_j is not part of it: there the own line and line j coincide for EVERY z, KG has a
kink in x (the two lines' slopes have different gradients: grad_x Sigma(a_j, x) = grad sigma^2 / 2 at x = a_j), and which of the two
one-sided gradients comes out hangs on the last bit of the lines.  At that point the device is compared with the twin's formula on
the device's OWN lines (ElasticGPE.kg_last_lines), at the same bound.
"""
import math

import numpy as np
from scipy.special import erfc

import kg_reference as kr
import nei_reference as nr

WORST_GRAD = 3.2e-13   # measured: 3.13e-13 (the N = 1536 cases; 1.23e-13 without them)

# (kern, N, d, R, E, lnoise): every N, R, E, d and kernel of the issue appears; R + 1 odd and even, R past kg_cross's 128-line tile,
# E past its 64-point tile, N inside one row tile, one past it, several; then the point with a large nu, E past the 256 points at which
# the finish takes its tiled form (d <= 16), and N = 1536, where the row-wise finish splits the observations over two workgroups (both
# instantiations; kernels and d at which KG and its gradient are of a size there: under SEArd this dense a design leaves KG = 0)
CASES = [("SEArd", 40, 3, 37, 5, -2.0), ("SEArd", 129, 1, 1, 1, -2.0), ("SEArd", 300, 20, 257, 130, -2.0),
         ("Mat52Ard", 129, 3, 257, 5, -2.0), ("Mat52Ard", 40, 1, 37, 130, -2.0), ("Mat52Ard", 300, 20, 1, 5, -2.0),
         ("Mat12Ard", 300, 3, 37, 130, -2.0), ("Mat12Ard", 40, 20, 257, 1, -2.0), ("Mat12Ard", 129, 1, 37, 5, -2.0),
         ("SEArd", 129, 3, 37, 5, 1.5), ("Mat52Ard", 40, 3, 37, 300, -2.0),
         ("Mat12Ard", 1536, 3, 37, 5, -2.0), ("Mat52Ard", 1536, 20, 37, 5, -2.0)]
LL, LSIG, BETA = math.log(0.5), 0.0, 0.0


def case_data(case):
    """dict(X (N, d), y, A (R, d), Xe (E, d), dup: the index of the point that equals a_0, or -1).  The points: uniform in the box,
    then (E >= 5) the site of the largest observation moved a little, an observed site, and a_0 itself."""
    kern, N, d, R, E, lnoise = case
    rng = np.random.default_rng(1000 * N + 10 * R + d)
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(axis=1) / math.sqrt(d)) + 0.1 * rng.standard_normal(N)
    A, Xe = rng.random((R, d)), rng.random((E, d))
    dup = -1
    if E >= 5:
        Xe[1] = np.clip(X[int(np.argmax(y))] + 0.01, 0.0, 1.0)
        Xe[2] = X[N // 2]
        Xe[3] = A[0]
        dup = 3
    return dict(kern=kern, X=X, y=y, A=A, Xe=Xe, dup=dup, ll=np.full(d, LL + 0.5 * math.log(d)), lsig=LSIG,
                nu=math.exp(2.0 * lnoise) + nr.EPS, lnoise=lnoise, beta=BETA)


def k_fx(kern, T, il, s2f, dt):
    """(k, fx) for the differences T (..., d): k(x, y), and fx with dk/dx = fx T il^2."""
    r2 = ((T * il) ** 2).sum(axis=-1)
    with np.errstate(all="ignore"):
        if kern == "SEArd":
            k = s2f * np.exp(-r2 / dt(2.0))
            return k, -k
        if kern == "Mat52Ard":
            s = np.sqrt(dt(5.0) * r2)
            return s2f * (dt(1.0) + s + dt(5.0) / dt(3.0) * r2) * np.exp(-s), -(dt(5.0) / dt(3.0)) * s2f * (dt(1.0) + s) * np.exp(-s)
        r = np.sqrt(r2)                                                      # Mat12Ard; fx = 0 at r = 0
        k = s2f * np.exp(-r)
        return k, np.where(r > 0, -k / np.where(r > 0, r, dt(1.0)), dt(0.0))


class Twin:
    def __init__(self, c, dt=np.float64):
        self.c, self.dt = c, dt
        self.X, self.A = np.asarray(c["X"], dtype=dt), np.asarray(c["A"], dtype=dt)
        self.il = np.exp(-np.asarray(c["ll"], dtype=dt))
        self.s2f, self.nu = np.exp(dt(2.0) * dt(c["lsig"])), dt(c["nu"])
        K = k_fx(c["kern"], self.X[:, None, :] - self.X[None, :, :], self.il, self.s2f, dt)[0]
        self.L = nr.chol(K + self.nu * np.eye(len(K), dtype=dt))
        self.alpha = nr.solve_lower_t(self.L, nr.solve_lower(self.L, np.asarray(c["y"], dtype=dt) - dt(c["beta"])))
        KA = k_fx(c["kern"], self.X[:, None, :] - self.A[None, :, :], self.il, self.s2f, dt)[0]   # (N, R)
        self.VA = nr.solve_lower(self.L, KA)
        self.muA = dt(c["beta"]) + KA.T @ self.alpha

    def point(self, x, lines=None):
        """(kg, nseg, grad (d,), mu, s2, Sig (R,), envelope, kg at the twin's precision) at one point; lines = (Sig, s2, mu, mu_A): the
        envelope and its weights from these instead of the twin's own."""
        dt, c = self.dt, self.c
        x = np.asarray(x, dtype=dt)
        TX, TA = x[None, :] - self.X, x[None, :] - self.A
        kx, fx = k_fx(c["kern"], TX, self.il, self.s2f, dt)
        ka, fa = k_fx(c["kern"], TA, self.il, self.s2f, dt)
        v = nr.solve_lower(self.L, kx[:, None])[:, 0]
        mu, s2, Sig = dt(c["beta"]) + kx @ self.alpha, max(self.s2f - v @ v, dt(0.0)), ka - self.VA.T @ v
        muA = self.muA
        if lines is not None:
            Sig, s2, mu, muA = (np.asarray(a, dtype=dt) for a in lines)
        R, dd = len(Sig), s2 + self.nu
        if not (dd > 0 and np.isfinite(dd)):
            return 0.0, 0, np.zeros(len(x)), mu, s2, Sig, [], dt(0.0)
        s = np.sqrt(dd)
        a, b = np.append(muA, mu), np.append(Sig, s2) / s
        kg, nseg = kr.kg_march(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        env, zs = envelope(a, b)
        zs = [-math.inf] + zs + [math.inf]
        phi = lambda z: dt(0.3989422804014327) * np.exp(-dt(0.5) * (dt(z) * dt(z))) if math.isfinite(z) else dt(0.0)   # noqa: E731
        Phi = lambda z: dt(0.5) * dt(erfc(-float(z) / math.sqrt(2.0))) if dt is np.float64 else _Phi_ext(z)          # noqa: E731
        own_top = R == 0 or mu > muA.max()
        csig, cmu, t, direct = dt(0.0), dt(-1.0 if own_top else 0.0), np.zeros(len(v), dtype=dt), np.zeros(len(x), dtype=dt)
        q_own, kgx = None, dt(0.0)
        for i, cl in enumerate(env):
            q = phi(zs[i]) - phi(zs[i + 1])
            if i > 0:                                                        # the term of the step onto this line: db h(-|z|)
                az = abs(zs[i])
                kgx = kgx + (b[cl] - b[env[i - 1]]) * (phi(az) - az * Phi(-az))
            if cl == R:
                q_own, lo, hi = q, zs[i], zs[i + 1]
                if own_top:
                    cmu = -(Phi(lo) + Phi(-hi))
                else:
                    cmu = Phi(-lo) - Phi(-hi) if lo >= 0 else Phi(hi) - Phi(lo)
            else:
                csig = csig - q * Sig[cl] / (dt(2.0) * (dd * s))
                t = t + (q / s) * self.VA[:, cl]
                direct = direct + (q / s) * fa[cl] * TA[cl] * self.il * self.il
        if q_own is not None:
            csig = csig + q_own * (s2 + dt(2.0) * self.nu) / (dt(2.0) * (dd * s))
        if not s2 > 0:
            csig = dt(0.0)
        e = cmu * self.alpha + nr.solve_lower_t(self.L, (-(dt(2.0) * csig) * v - t)[:, None])[:, 0]
        grad = ((fx * e)[:, None] * TX).sum(axis=0) * self.il * self.il + direct
        return kg, nseg, grad, mu, s2, Sig, env, kgx

    def all_points(self):
        return [self.point(x) for x in self.c["Xe"]]


def _Phi_ext(z):
    """Phi of an extended argument: float64's erfc at the rounded argument plus the first-order term of the rest (erfc's own 1e-16 is
    far below the error of the twin's solves, which is what WORST_GRAD measures)."""
    if not math.isfinite(z):
        return np.longdouble(0.0 if z < 0 else 1.0)
    z = np.longdouble(z)
    z0 = np.longdouble(float(z))
    return np.longdouble(0.5) * np.longdouble(erfc(-float(z0) / math.sqrt(2.0))) + (z - z0) * np.longdouble(0.3989422804014327) * np.exp(-z0 * z0 / 2)


def envelope(a, b):
    """The march of include/bohip_kg.h on the lines (a, b) at their precision: (lines c_0 .. c_n, break points z_1 .. z_n)."""
    live = np.flatnonzero(np.isfinite(a) & np.isfinite(b))
    if live.size == 0:
        return [], []
    c = int(live[np.lexsort((live, -a[live], b[live]))[0]])
    env, zs = [c], []
    while True:
        U = live[b[live] > b[c]]
        if U.size == 0:
            return env, zs
        z = (a[c] - a[U]) / (b[U] - b[c])
        k = int(np.lexsort((U, -a[U], -b[U], z))[0])
        c = int(U[k])
        env.append(c)
        zs.append(float(z[k]) if a.dtype == np.float64 else z[k])


def unit(c):
    """nei_grad_reference.distance's unit for EI-like scores: s_f max_k e^(-ll_k)."""
    return math.exp(c["lsig"]) * float(np.exp(-np.min(c["ll"])))


_REFS = {}


def reference(case, dt=np.float64):
    """The twin and its results at every point of a case, computed once and shared."""
    key = (case, dt)
    if key not in _REFS:
        t = Twin(case_data(case), dt)
        _REFS[key] = (t, t.all_points())
    return _REFS[key]
