"""Who owns device memory (csrc/devbuf.h): the scratch of every feature grows, is kept, and goes with its handle.

  1  grow, fall back, grow again: on ONE handle every feature is called at a small size, at a size that makes it reallocate its
     block, and at the small size again.  bohip_debug_live_bytes says the middle call raised the device bytes and the third left
     them alone; every call returns what the same call returns on a fresh handle.
  2  the model's own regrowth (alloc_model) under features that keep ld-sized chunk buffers.
  3  nothing is left behind: the bytes after test 1's whole sequence and the destroys are the bytes before, also around a
     bohip_gp_create that fails late (an out-of-memory answer to its factor matrices, after the streams and events exist).

A fresh handle here has the very history of the lived-in one as far as the numbers go (one append_, one factorisation); what differs
is the scratch.  Integers (arg-max indices, picks, evaluation counts) and the q-EI draws and picks -- what tests/test_lifecycle_gpu.py
holds bit for bit on a lived-in handle -- must be equal; every other output is held to that file's form of bound, |a - b| <= 1e-6 |b| +
64 N eps scale with scale = max(1, max |b|) of the array, and the test prints whether it was equal bit for bit anyway."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N, D = 200, 3
KERNELS = ["SEArd", "Mat52Ard"]
LL, LSIG, LNOISE, BETA = np.full(D, np.log(0.5)), 0.0, -2.0, 0.0
TAU = 1.5
LB, UB = np.zeros(D), np.ones(D)
FRONT, REF = np.array([[0.5, 1.0], [1.0, 0.5]]), np.array([-3.0, -3.0])
THETA = np.array([[LNOISE + 0.1 * h, 0.05 * h, *(LL + 0.07 * h), LSIG - 0.03 * h] for h in range(6)])


def xs_of(R, seed=100):
    return np.asfortranarray(synth(1, D, R, seed=seed + R)[2].T)


def model(bohip, kern, seed, capacity=N, n=N):
    X, y, _ = synth(n, D, 1, seed=seed)
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(LL, LSIG), logNoise=LNOISE, capacity=capacity)
    m.append_(X.T, y)
    return m


class World:
    """A handle and, made on demand, what the features over several objects need: three constraint models, a second objective, a
    paths object."""

    def __init__(self, bohip, kern, m=None):
        self.b, self.kern, self.m = bohip, kern, m if m is not None else model(bohip, kern, 0)
        self._cons, self._m1, self._paths = None, None, None

    @property
    def cons(self):
        if self._cons is None:
            self._cons = [model(self.b, self.kern, s) for s in (1, 2, 3)]
        return self._cons

    @property
    def m1(self):
        if self._m1 is None:
            self._m1 = model(self.b, self.kern, 4)
        return self._m1

    @property
    def paths(self):
        if self._paths is None:
            self._paths = self.m.draw_paths(S=4, M=64, seed=5)
        return self._paths

    def make_all(self):
        return self.cons, self.m1, self.paths

    def close(self):
        if self._paths is not None:
            self._paths.close()
        for m in [self.m, self._m1] + (self._cons or []):
            if m is not None:
                m.close()


def score_con(w, C_):
    return w.b.ConstrainedGPE(w.m, w.cons[:C_], [0.0] * C_, [1] * C_).score("EI", [TAU], xs_of(300), want_grad=True)


# name, (small, big), call.  The size that grows is read from the host code: the feature's OWN block where it has one (so the order of
# the features does not matter), the shared scoring scratch for `score`, which runs first.
FEATURES = [
    ("score", (40, 700), lambda w, R: w.m.score("EI", [TAU], xs_of(R))),                    # row-wise -> chunked; dXs, dmu ... dscore
    ("score_grad", (40, 700), lambda w, R: w.m.score_grad("EI", [TAU], xs_of(R))),          # dgrad
    ("predict_cov", (40, 300), lambda w, R: w.m.predict_cov(xs_of(R))),                     # dVV, dcov: Rp = 128 -> 384 (before the joint forms)
    ("predict_grad", (40, 300), lambda w, R: w.m.predict_grad(xs_of(R))),                   # ensure_con's block, C = 0 with Jacobians
    ("ascend", (4, 40), lambda w, R: w.m.ascend("EI", [TAU], LB, UB, xs_of(R), maxeval=40)),   # the ascent block starts at 32
    ("qei_batch", ((16, 8, 2), (64, 64, 4)),
     lambda w, a: w.m.qei_batch(xs_of(a[0]), a[2], S=a[1], seed=7, tau=TAU, want_samples=True)),
    ("kg", (8, 64), lambda w, R: w.m.kg(xs_of(R))),
    ("mes", (40, 700), lambda w, R: w.m.mes(xs_of(R), samples=8, seed=3)),
    ("score_con", (1, 3), score_con),                                                        # (C + 1) R moments: 59 600 bytes > 52 400
    ("score_mo", (40, 2000), lambda w, R: w.b.score_mo(w.m, w.m1, FRONT, REF, xs_of(R))),
    ("score_ens", (2, 6), lambda w, H: w.m.score_ensemble("EI", [TAU], xs_of(100), THETA[:H], want_each=True, want_moments=True)),
    ("score_ens_grad", (2, 6), lambda w, H: w.m.score_ensemble_grad("EI", [TAU], xs_of(100), THETA[:H], want_each=True)),   # ens_alpha
    ("mll_grad_batch", (1, 5), lambda w, H: w.m.mll_grad_batch(THETA[:H])),                 # fit_io
    ("select_batch", (40, 700), lambda w, R: w.m.select_batch("EI", [TAU], xs_of(R), 3)),   # dBV, dbatch
    ("sample_joint", (40, 700), lambda w, R: w.m.sample_joint(xs_of(R), S=4, seed=9)),      # the sampler's factor workspace
    ("thompson", (4, 100), lambda w, S: w.m.thompson(xs_of(100), S, seed=11)),              # S records (q-EI's 64 draws left 64)
    ("paths_eval", (100, 5000), lambda w, R: w.paths.eval(xs_of(R))),
    ("paths_eval_grad", (100, 5000), lambda w, R: w.paths.eval_grad(xs_of(R), path_of=np.arange(R) % 4)),
]
EXACT = {"qei_batch"}


def live_bytes(bohip):
    from bohip import _lib

    fn = _lib.load().bohip_debug_live_bytes
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_int64)]
    out = []
    for kind in (0, 1):
        v = C.c_int64(-1)
        assert fn(kind, C.byref(v)) == 0
        out.append(int(v.value))
    return tuple(out)


def flat(res):
    """The arrays and numbers of a result, in order (strings and None dropped)."""
    if res is None or isinstance(res, str):
        return []
    if isinstance(res, np.ndarray):
        return [res]
    if np.isscalar(res):
        return [np.asarray(res)]
    return [a for part in res for a in flat(part)]


def compare(name, got, want, exact):
    got, want = flat(got), flat(want)
    assert len(got) == len(want) and len(got) > 0, name
    bitwise = True
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, i)
        same = a.tobytes() == b.tobytes()
        bitwise &= same
        if exact or a.dtype.kind in "iub":
            assert same, (name, i, "not equal bit for bit")
        elif not same:
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], b[~fin], equal_nan=True), (name, i)
            scale = max(1.0, float(np.max(np.abs(b[fin])))) if fin.any() else 1.0
            err, tol = np.abs(a[fin] - b[fin]), 1e-6 * np.abs(b[fin]) + 64 * N * EPS * scale
            assert np.all(err <= tol), (name, i, float(np.max(err / tol)))
    return bitwise


@pytest.fixture(scope="module")
def fresh(bohip):
    """(kernel, feature, size index) -> what the call returns on a fresh handle; computed once, read-only."""
    cache = {}

    def get(kern, k, which):
        if (kern, k, which) not in cache:
            name, sizes, call = FEATURES[k]
            w = World(bohip, kern)
            try:
                cache[kern, k, which] = call(w, sizes[which])
            finally:
                w.close()
            for a in flat(cache[kern, k, which]):
                a.setflags(write=False)
        return cache[kern, k, which]

    return get


def run_sequence(bohip, kern, w, check=None):
    """Every feature at small, big, small on the world `w`; with `check` the live bytes around the calls are asserted and
    check(k, which, result) sees every result."""
    for k, (name, sizes, call) in enumerate(FEATURES):
        w.make_all()                                                         # (before the readings: the companions hold memory too)
        before = live_bytes(bohip)
        r0 = call(w, sizes[0])
        after_small = live_bytes(bohip)
        r1 = call(w, sizes[1])
        after_big = live_bytes(bohip)
        r2 = call(w, sizes[0])
        after_again = live_bytes(bohip)
        if check:
            assert after_small[0] >= before[0], name
            assert after_big[0] > after_small[0], (name, "the middle call did not reallocate", after_small, after_big)
            assert after_again == after_big, (name, "the third call changed the live bytes", after_big, after_again)
            for which, r in ((0, r0), (1, r1), (0, r2)):
                check(k, which, r)


@pytest.mark.parametrize("kern", KERNELS)
def test_grow_fall_back_grow_again(bohip, fresh, kern):
    w = World(bohip, kern)
    report = []

    def check(k, which, r):
        name = FEATURES[k][0]
        report.append((name, compare(f"{kern} {name} at {FEATURES[k][1][which]}", r, fresh(kern, k, which), name in EXACT)))

    try:
        run_sequence(bohip, kern, w, check)
    finally:
        w.close()
    not_bitwise = sorted({n for n, same in report if not same})
    print(f"  {kern}: {len(report)} calls compared with fresh handles; not equal bit for bit (within the bound): {not_bitwise or 'none'}")


@pytest.mark.parametrize("kern", KERNELS)
def test_regrowth_of_the_model(bohip, kern):
    """An append past the capacity re-makes the model's buffers and drops the ld-sized chunk buffers (dKsT, dVT, dUT, dq, dBV) that
    the three calls made at the old ld; the same calls then give what a fresh handle of the new capacity gives."""
    from bohip import _lib

    X, y, _ = synth(N, D, 1, seed=0)
    calls = [lambda m: m.score("EI", [TAU], xs_of(700)), lambda m: m.score_grad("EI", [TAU], xs_of(700)),
             lambda m: m.select_batch("EI", [TAU], xs_of(700), 3)]
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(LL, LSIG), logNoise=LNOISE, capacity=120)
    f = None
    try:
        m.append_(X[:100].T, y[:100])
        for c in calls:
            c(m)
        cap0, refits0 = m.info(_lib.INFO_CAPACITY), m.info(_lib.INFO_REFITS)
        m.append_(X[100:].T, y[100:])
        assert m.info(_lib.INFO_CAPACITY) > cap0 == 120 and m.nobs == N
        f = bohip.ElasticGPE(D, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(LL, LSIG), logNoise=LNOISE,
                             capacity=m.info(_lib.INFO_CAPACITY))
        f.append_(X.T, y)
        same = [compare(f"{kern} call {i} after the regrowth", c(m), c(f), False) for i, c in enumerate(calls)]
        assert m.info(_lib.INFO_REFITS) > refits0
        print(f"  {kern}: capacity {cap0} -> {m.info(_lib.INFO_CAPACITY)}; equal bit for bit to the fresh handle: {same}")
    finally:
        m.close()
        if f is not None:
            f.close()


def test_nothing_is_left_behind(bohip):
    from bohip import _lib

    lib = _lib.load()
    model(bohip, "SEArd", 0).close()                                          # process-wide one-time state exists from here on
    before = live_bytes(bohip)
    w = World(bohip, "SEArd")
    try:
        run_sequence(bohip, "SEArd", w)
        held = live_bytes(bohip)
    finally:
        w.close()
    assert held[0] > before[0] and held[1] > before[1]                        # (the sequence did hold device and pinned memory)
    assert live_bytes(bohip) == before
    # a create that fails after its streams, events, pinned block and first device buffers exist: 2^20 observations ask for four
    # factor matrices of 8.8 TB each, which the allocator declines
    h = C.c_void_p()
    rc = lib.bohip_gp_create(D, 1 << 20, 0, 0, C.byref(h))
    assert rc != 0 and not h.value, rc
    assert live_bytes(bohip) == before
    m = model(bohip, "SEArd", 0)                                              # and the next handle works
    try:
        sc, bv, bi = m.score("EI", [TAU], xs_of(40))
        assert np.all(np.isfinite(sc)) and bv == sc[bi]
    finally:
        m.close()
    assert live_bytes(bohip) == before
