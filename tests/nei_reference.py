"""The NumPy twin of noisy expected improvement (include/bohip_nei.h) -- TEST INFRASTRUCTURE ONLY.  No device.

ONE set of statements, the header's definition line by line, run at two precisions: ``Twin(..., dt=np.float64)`` and
``Twin(..., dt=np.longdouble)``.  Nothing here calls LAPACK: the factorisation and the substitutions are written out so that both
precisions run the same code.  The standard normals are the library's own, ``bohip_thompson_normal(seed, 2 s, i)`` and
``(seed, 2 s + 1, i)`` through ctypes (host code: no GPU needed).  The acquisition functors are pend_reference's (float64: the
moments of the extended twin are rounded to float64 first, so a score difference between the twins is what the moments' error does
to the score, not the functor's own rounding).

The inputs of tests/test_nei_gpu.py are made here (``spec``, ``all_inputs``), so that tests/test_nei_host.py can measure the float64
twin against the extended one on exactly those inputs.  The worst figures of that comparison are the constants WORST below; the
device is held to 16 x them (what tests/test_limits_gpu.py grants over a CPU-measured twin error).  All figures are scale-free: F,
m_s and EI in units of s_f, s^2 in units of s_f^2, PI as it is, LogEI relative to max(1, |value|) (its values reach -1e6 in the
far tail, where one ulp of the mean moves them by more than any absolute figure could grant).
"""
import math

import numpy as np

import pend_reference as pr
from conftest import synth

EPS = np.finfo(np.float64).eps
BS = 64

# The worst |float64 twin - extended twin| over every input of tests/test_nei_gpu.py at jitter_rel = 1e-6 (test_nei_host.py
# test_tolerance_source recomputes them and asserts the float64 twin stays within 2 x), rounded up to two digits.  Keys: fantasies F
# (and tau), the means m_s, the variance s^2, the scores per acquisition.
WORST = {"F": 6.3e-11, "m": 5.7e-11, "s2": 2.5e-13, "EI": 4.8e-10, "PI": 5.1e-10, "LogEI": 4.0e-08}
DEVICE_FACTOR = 16.0


# ---- the model pieces, at the precision of their arguments -------------------------------------------------------------------------
def cov(kern, A, B, ll, lsig, dt):
    """k(A, B) for SEArd and Mat32Iso (the two families of the device tests), rows = points."""
    A, B = np.asarray(A, dtype=dt), np.asarray(B, dtype=dt)
    il = np.exp(-np.asarray(ll, dtype=dt)) * np.ones(A.shape[1], dtype=dt)
    D = (A * il)[:, None, :] - (B * il)[None, :, :]
    r2 = (D * D).sum(axis=2)
    s2f = np.exp(dt(2.0) * dt(lsig))
    if kern == "SEArd":
        return s2f * np.exp(-r2 / dt(2.0))
    if kern == "Mat32Iso":
        s = np.sqrt(dt(3.0) * r2)
        return s2f * (dt(1.0) + s) * np.exp(-s)
    raise ValueError(kern)


def chol(A):
    """Lower Cholesky factor, blocked left-looking; raises on a non-positive pivot."""
    A = np.array(A)
    n = len(A)
    L = np.zeros_like(A)
    for j0 in range(0, n, BS):
        j1 = min(n, j0 + BS)
        P = A[j0:, j0:j1] - L[j0:, :j0] @ L[j0:j1, :j0].T
        for j in range(j0, j1):
            c = j - j0
            v = P[c:, c] - L[j:, j0:j] @ L[j, j0:j]
            if not v[0] > 0:
                raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
            L[j, j] = np.sqrt(v[0])
            L[j + 1:, j] = v[1:] / L[j, j]
    return L


def solve_lower(L, B):
    """X with L X = B."""
    X = np.array(B, dtype=L.dtype)
    n = len(L)
    for j0 in range(0, n, BS):
        j1 = min(n, j0 + BS)
        for j in range(j0, j1):
            X[j] = (X[j] - L[j, j0:j] @ X[j0:j]) / L[j, j]
        if j1 < n:
            X[j1:] = X[j1:] - L[j1:, j0:j1] @ X[j0:j1]
    return X


def solve_lower_t(L, B):
    """X with L' X = B."""
    X = np.array(B, dtype=L.dtype)
    n = len(L)
    for j1 in range(n, 0, -BS):
        j0 = max(0, j1 - BS)
        for j in range(j1 - 1, j0 - 1, -1):
            X[j] = (X[j] - L[j + 1:j1, j] @ X[j + 1:j1]) / L[j, j]
        if j0 > 0:
            X[:j0] = X[:j0] - L[j0:j1, :j0].T @ X[j0:j1]
    return X


_NORMALS = {}


def normals(seed, S, N):
    """(Z, E), S1 x N each, S1 = max(S, 1): the library's draws; S = 0: zeros (the plug-in form).  The draws of fantasy s do not
    depend on S, so the table of the largest S asked for so far serves every smaller one."""
    if S == 0:
        return np.zeros((1, N)), np.zeros((1, N))
    have = _NORMALS.get((seed, N))
    if have is None or have[0].shape[0] < S:
        from bohip import _lib

        fn = _lib.load().bohip_thompson_normal
        Z = np.array([[fn(seed, 2 * s, i) for i in range(N)] for s in range(S)])
        E = np.array([[fn(seed, 2 * s + 1, i) for i in range(N)] for s in range(S)])
        have = _NORMALS[(seed, N)] = (Z, E)
    return have[0][:S], have[1][:S]


class Twin:
    """The definition for one resident model.  X (N, d), y (N), nu (N): the noise term cK's diagonal carries for every row."""

    def __init__(self, kern, X, y, ll, lsig, nu, beta, jitter_rel, dt=np.float64, steps=0, nu_d=None):
        self.kern, self.ll, self.lsig, self.dt = kern, ll, lsig, dt
        self.X, self.y, self.beta = np.asarray(X, dtype=dt), np.asarray(y, dtype=dt), dt(beta)
        N = len(self.y)
        self.nu = np.asarray(nu, dtype=dt) * np.ones(N, dtype=dt)
        self.s2f = np.exp(dt(2.0) * dt(lsig))
        self.delta = dt(jitter_rel) * self.s2f * dt(10.0) ** steps          # delta = jitter_rel k(x, x)
        K = cov(kern, self.X, self.X, ll, lsig, dt)
        self.K = K
        self.LA = chol(K + np.diag(self.nu))                                   # A = K + D = L L'
        if nu_d is not None:                                                   # (a WRONG twin on purpose: D without a part of what A carries)
            self.nu = np.asarray(nu_d, dtype=dt) * np.ones(N, dtype=dt)
        self.Ld = chol(K + self.delta * np.eye(N, dtype=dt))                   # K_d = K + delta I = L_d L_d'

    def cond_kd(self):
        w = np.linalg.eigvalsh(np.asarray(self.K, dtype=np.float64) + float(self.delta) * np.eye(len(self.y)))
        return float(w[-1] / w[0])

    def a_inv(self, B):
        return solve_lower_t(self.LA, solve_lower(self.LA, B))

    def fantasies(self, Z, E):
        """F (S1, N), tau (S1), alpha (N, S1) for the draws Z, E (S1, N)."""
        dt = self.dt
        Z, E = np.asarray(Z, dtype=dt).T, np.asarray(E, dtype=dt).T           # columns = fantasies
        G = self.Ld @ Z                                                        # g_s = L_d z_s
        R = (self.y - self.beta)[:, None] - G - np.sqrt(self.nu)[:, None] * E  # r_s = (y - beta) - g_s - sqrt(nu_i) e_s,i
        F = self.beta + G + R - self.nu[:, None] * self.a_inv(R)               # f_s = beta + g_s + r_s - D A^-1 r_s
        tau = F.max(axis=0)                                                    # tau_s = max_i f_s,i
        alpha = solve_lower_t(self.Ld, solve_lower(self.Ld, F - self.beta))    # alpha_s = K_d^-1 (f_s - beta)
        return F.T, tau, alpha

    def moments(self, Xs, alpha):
        """m (R, S1) and s^2 (R) at the candidates Xs (R, d)."""
        Ks = cov(self.kern, self.X, np.asarray(Xs, dtype=self.dt), self.ll, self.lsig, self.dt)   # (N, R)
        m = self.beta + Ks.T @ alpha                                           # m_s(x) = beta + k*' alpha_s
        V = solve_lower(self.Ld, Ks)
        s2 = np.maximum(self.s2f - (V * V).sum(axis=0), self.dt(0.0))          # s^2(x) = max(k(x, x) - |W_d k*|^2, 0)
        return m, s2


def score(acq, m, s2, tau):
    """NEI (R,) from m (R, S1), s^2 (R), tau (S1): the functor per fantasy, then the mean in the order s = 0, 1, ... (LogEI: the
    max-shifted log-mean-exp).  float64, whatever the precision of the moments."""
    m, s2, tau = (np.asarray(a, dtype=np.float64) for a in (m, s2, tau))
    each = np.array([pr.acq(acq, [float(tau[s])], m[:, s], s2) for s in range(len(tau))])
    return pr.average(acq, each), each


def top_two(sc):
    """(index of the first arg-max, score gap to the runner-up); NaN / -Inf never win."""
    s = np.where(np.isnan(sc), -np.inf, sc)
    i = int(np.argmax(s))
    if not s[i] > -np.inf:
        return -1, math.inf
    rest = np.delete(s, i)
    second = rest.max() if rest.size else -np.inf
    return i, float(s[i] - second) if second > -np.inf else math.inf


# ---- the inputs of the device tests ---------------------------------------------------------------------------------------------------
# Length-scales: cond(K_d) at jitter_rel = 1e-6 stays below 1e9 for every N used (test_nei_host.py asserts it).
MODELS = {"se3": dict(kern="SEArd", d=3, ll=math.log(0.5), lsig=0.0, lnoise=-2.0, beta=0.0),
          "m32": dict(kern="Mat32Iso", d=9, ll=math.log(1.5), lsig=0.0, lnoise=-2.0, beta=0.0)}
NS, RS, SS = (1, 17, 129, 300), (1, 40, 700), (0, 1, 5, 64)
R_MAX = 700
JREL, JREL_DEFAULT = 1e-6, 1e-8
ACQS = ("EI", "PI", "LogEI")
SEED = 20190606
S_EDGES = (3, 4, 5, 63, 65)                 # k_nei_means' tile edges in S, at N = 129 (the 128-row boundary in N), R = 40
BIG_N, BIG_RS, BIG_S = 1100, (200, 300), 5  # nine row tiles: R = 300 takes the companion's split-K pass (R = 200 is below the small limit there)
CHUNK_N, CHUNK_R, CHUNK_S = 17, 65537, 5    # one candidate past the chunk cap at N = 17: more than one K*' chunk


def model_nu(model):
    return math.exp(2.0 * MODELS[model]["lnoise"]) + EPS


def model_ll(model):
    p = MODELS[model]
    return np.full(p["d"], p["ll"]) if p["kern"].endswith("Ard") else np.array([p["ll"]])


def data(model, N, R=R_MAX, seed=None):
    """(X, y, Xs) of the device tests: the BASELINE recipe, one seed per (model, N).  X and y do not depend on R, and a smaller R is
    a prefix of the candidates."""
    d = MODELS[model]["d"]
    X, y, Xs = synth(N, d, max(R, R_MAX), (1000 * d + N) if seed is None else seed)
    return X, y, Xs[:R]


def weighted_data():
    """40 sites of 1 .. 5 evaluations each (SEArd, d = 3): (x_raw (d, n_evals), y_raw, X sites (N, d), ybar, reps, Xs)."""
    rng = np.random.default_rng(4040)
    X = rng.random((40, 3))
    reps = 1 + np.arange(40) % 5
    f = np.sin(3 * X).sum(1)
    cols = np.repeat(np.arange(40), reps)
    y_raw = f[cols] + 0.3 * rng.standard_normal(len(cols))
    ybar = np.array([y_raw[cols == i].mean() for i in range(40)])
    return np.asfortranarray(X[cols].T), y_raw, X, ybar, reps, rng.random((R_MAX, 3))


JIT_LL, JIT_LSIG, JIT_LNOISE, JIT_REL = np.zeros(2), 5.0, -25.0, 1e-3


def jitter_data():
    """tests/test_hardening_gpu.py's singular model: 60 positions observed five times each, sigma_f^2 = e^10, noise e^-50.  Under
    set_jitter(1e-3, 3) the first try adds J = 1e-3 (sigma_f^2 + noise) to the diagonal and succeeds: D carries it."""
    rng = np.random.default_rng(11)
    pos = rng.random((60, 2)) * 10 - 5
    X = np.repeat(pos, 5, axis=0)
    y = -(((X - 1) ** 2).sum(1) + rng.standard_normal(len(X)))
    J = JIT_REL * (math.exp(2 * JIT_LSIG) + math.exp(2 * JIT_LNOISE))
    return X, y, rng.random((40, 2)) * 10 - 5, J


def spec(tag):
    """The twin's arguments for an input of the device tests: dict(kern, X, y, ll, lsig, nu, beta, Xs, N).  Tags: (model, N) and
    (model, N, R) of the grid, "weighted", "weighted-ignored" (every nu_i = nu), "jitter", "jitter-ignored" (A as the device factors it, D without J: without J in A the model is singular)."""
    if tag in ("weighted", "weighted-ignored"):
        _, _, X, ybar, reps, Xs = weighted_data()
        p = MODELS["se3"]
        nu = model_nu("se3") / (reps if tag == "weighted" else 1.0)
        return dict(kern=p["kern"], X=X, y=ybar, ll=model_ll("se3"), lsig=p["lsig"], nu=nu, beta=p["beta"], Xs=Xs)
    if tag in ("jitter", "jitter-ignored"):
        X, y, Xs, J = jitter_data()
        nu = math.exp(2 * JIT_LNOISE) + EPS
        return dict(kern="SEArd", X=X, y=y, ll=JIT_LL, lsig=JIT_LSIG, nu=nu + J, beta=0.0, Xs=Xs, nu_d=None if tag == "jitter" else nu)
    model, N = tag[0], tag[1]
    p = MODELS[model]
    X, y, Xs = data(model, N, tag[2] if len(tag) > 2 else R_MAX)
    return dict(kern=p["kern"], X=X, y=y, ll=model_ll(model), lsig=p["lsig"], nu=model_nu(model), beta=p["beta"], Xs=Xs)


_TWINS, _RESULTS = {}, {}


def twin(tag, jitter_rel=JREL, dt=np.float64):
    key = (tag[:2] if isinstance(tag, tuple) else tag, jitter_rel, dt)
    if key not in _TWINS:
        a = spec(tag)
        _TWINS[key] = Twin(a["kern"], a["X"], a["y"], a["ll"], a["lsig"], a["nu"], a["beta"], jitter_rel, dt, nu_d=a.get("nu_d"))
    return _TWINS[key]


def reference(tag, S, jitter_rel=JREL, dt=np.float64):
    """dict(F, tau, m, s2, s2f, asum) of one input at all its candidates, computed once and shared: a case with fewer candidates
    reads the first rows.  asum: the largest sum_i |alpha_s,i| (pend_reference.value_bound's floor)."""
    key = (tag, S, jitter_rel, dt)
    if key not in _RESULTS:
        t = twin(tag, jitter_rel, dt)
        Z, E = normals(SEED, S, len(t.y))
        F, tau, alpha = t.fantasies(Z, E)
        m, s2 = t.moments(spec(tag)["Xs"], alpha)
        _RESULTS[key] = dict(F=F, tau=tau, m=m, s2=s2, s2f=float(t.s2f), asum=float(np.abs(alpha).sum(axis=0).max()))
    return _RESULTS[key]


def all_inputs():
    """Every (tag, S) the device tests compare at jitter_rel = 1e-6: the source of WORST."""
    out = [((model, N), S) for model in MODELS for N in NS for S in SS]
    out += [(("se3", 129), S) for S in S_EDGES if S not in SS]
    out += [(("se3", BIG_N, max(BIG_RS)), BIG_S), (("se3", CHUNK_N, CHUNK_R), CHUNK_S), ("weighted", 5), ("jitter", 5)]
    return out


def figures(a, b):
    """The scale-free distances between two references (dicts of F, tau, m, s2) and their scores: the keys of WORST.  F, m, EI in
    units of s_f, s^2 in units of s_f^2, PI as it is, LogEI relative to max(1, |value|)."""
    s2f = a["s2f"]
    sf = math.sqrt(s2f)
    out = {"F": max(float(np.max(np.abs(a["F"] - b["F"]))), float(np.max(np.abs(a["tau"] - b["tau"])))) / sf,
           "m": float(np.max(np.abs(a["m"] - b["m"]))) / sf, "s2": float(np.max(np.abs(a["s2"] - b["s2"]))) / s2f}
    for acq in ACQS:
        sa, sb = score(acq, a["m"], a["s2"], a["tau"])[0], score(acq, b["m"], b["s2"], b["tau"])[0]
        out[acq] = float(np.max(score_distance(acq, sa, sb, s2f), initial=0.0))
    return out


def score_distance(acq, got, ref, s2f):
    """|got - ref| in the units of WORST[acq], where both are finite (elsewhere they must agree exactly: the caller checks)."""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(got) & np.isfinite(ref)
        d = np.abs(got - ref)[fin]
    if acq == "EI":
        return d / math.sqrt(s2f)
    if acq == "LogEI":
        return d / np.maximum(1.0, np.abs(ref[fin]))
    return d


def bounds(ref, N):
    """The device's bounds around a float64 reference: 16 x WORST of the matching quantity, in the reference's scale; for the
    mu-like and sigma^2-like quantities test_pend_gpu's bound where that is larger.  The scores' bounds are in score_distance's units."""
    s2f = ref["s2f"]
    sf = math.sqrt(s2f)
    return {"F": DEVICE_FACTOR * WORST["F"] * sf,
            "m": np.maximum(DEVICE_FACTOR * WORST["m"] * sf, pr.value_bound(ref["m"], s2f, ref["asum"])),
            "s2": np.maximum(DEVICE_FACTOR * WORST["s2"] * s2f, 1e-6 * np.abs(ref["s2"]) + 64 * N * EPS * s2f),
            "EI": DEVICE_FACTOR * WORST["EI"], "PI": DEVICE_FACTOR * WORST["PI"], "LogEI": DEVICE_FACTOR * WORST["LogEI"]}


def near_tie(acq, sc, s2f):
    """Whether the two best scores differ by less than twice the device's score bound."""
    i, gap = top_two(sc)
    if i < 0 or gap == math.inf:
        return False
    unit = math.sqrt(s2f) if acq == "EI" else (max(1.0, abs(sc[i])) if acq == "LogEI" else 1.0)
    return gap < 2.0 * DEVICE_FACTOR * WORST[acq] * unit
