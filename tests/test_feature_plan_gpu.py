"""The launch structure of the calls over several settings or several models (csrc/bohip.hip: ens_drive, fill_fit_args,
moments_to_values, multi_posterior, the two stages), pinned.  A sibling of test_pass_plan_gpu.py with the same two rules:

  1  the launches of a call: the exact ordered stage labels of m.timing() on EVERY handle that takes part;
  2  the numbers: every output equals, bit for bit, what the same call gives as the FIRST call on fresh handles built from the same
     data -- the handles under test have had other calls before it (a throw-away call, or the case's own history).

The table was fixed on the library as it was BEFORE the host code of these calls was given one owner each, and has to hold on every
library after it.  Three things it pins that are not obvious:
  - bohip_gp_mll_grad_batch records no stage, so its row is empty (what it pins is rule 2 over several launch groups);
  - a foreign handle that serves two constraints is collected once per appearance, and the second collection finds nothing: its
    labels read empty after the call;
  - under "Feasibility" the objective's handle runs the combine only.

Shapes.  Ensemble and fit: d = 3, N = 40, so M = 48 (one 16-panel short of a power of two), a slab of (2 M + 1)(M + 8) = 5432 doubles
and, under BOHIP_FIT_WS_MAX_MB=1, Hc = 2^20 / (8 x 5432) = 24 settings a launch: H = Hc + 1 is two groups.  R = 20, and 16384 + 77
for two candidate chunks.  Several models: the e2e members of test_con_gpu.py (N = 65, 17, 130; d = 4), R = 33."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth
from test_fit_gpu import model_of, settings

pytestmark = pytest.mark.gpu

KERN, D, N = "Mat52Ard", 3, 40
M = -(-N // 16) * 16
SLAB = (2 * M + 1) * (M + 8)
HC = (1 << 20) // (8 * SLAB)                 # fit_plan under BOHIP_FIT_WS_MAX_MB=1
R2 = 16384 + 77
TAU = 0.4
FRONT = np.array([[0.1, 0.5, 0.9], [0.8, 0.4, 0.2]])
REF = np.array([-1.0, -1.0])
D_E2E, R_E2E = 4, 33


# ---- the handles of a case -----------------------------------------------------------------------------------------------------------
def make_ens(bohip):
    X, y, _ = synth(N, D, 1, seed=N)
    return [model_of(bohip, KERN, X, y)]


def make_anchor(bohip):
    return [bohip.ElasticGPE(2)]               # no observations: the device and the stream only


def make_members(bohip):
    from test_con_gpu import member_data

    return [model_of(bohip, kern, X, y) for kern, X, y, _ in member_data()]


def xs_of(R, d=D):
    return np.asfortranarray(synth(1, d, R, seed=1000 + R)[2].T)


def theta_of(H):
    return settings(KERN, D, H, seed=7 + H)


# ---- the calls: f(bohip, handles) -> arrays ----------------------------------------------------------------------------------------
def ens(H, R):
    return lambda b, ms: tuple(ms[0].score_ensemble("EI", [TAU], xs_of(R), theta_of(H), want_each=True, want_moments=True))


def ens_grad(H, R):
    def call(b, ms):
        res, grad, eg = ms[0].score_ensemble_grad("EI", [TAU], xs_of(R), theta_of(H), want_each=True)
        return tuple(res) + (grad, eg)
    return call


def fit(H):
    return lambda b, ms: ms[0].mll_grad_batch(theta_of(H))


def crafted(rows, R):
    rng = np.random.default_rng(50 + rows + R)
    return rng.uniform(-1.0, 1.0, (rows, R)), rng.uniform(0.01, 1.0, (rows, R))


def con_values(C_, R, partials, record):
    """bohip_con_values itself: the Python wrapper always asks for the record."""
    def call(b, ms):
        from bohip import _lib
        from bohip.model import _con_args, _ip, _ptr

        m = ms[0]
        aid, p, t, s = _con_args("EI", [0.3], np.linspace(-0.3, 0.3, C_), [1, -1, 1, -1][:C_])
        mu, var = crafted(C_ + 1, R)
        value, logfeas = np.empty(R), np.empty(R)
        dmu, dvar = (np.empty((C_ + 1, R)), np.empty((C_ + 1, R))) if partials else (None, None)
        best = _lib.Best()
        _lib.check(m._lib.bohip_con_values(m._h, aid, _ptr(p), C_, _ptr(t), s.ctypes.data_as(_ip), _ptr(mu), _ptr(var), R, _ptr(value),
                                           _ptr(logfeas), _ptr(dmu) if partials else None, _ptr(dvar) if partials else None,
                                           C.byref(best) if record else None))
        return [value, logfeas] + ([dmu, dvar] if partials else []) + ([np.array([best.val, best.idx])] if record else [])
    return call


def ehvi_values(R, partials, record):
    def call(b, ms):
        from bohip import _lib
        from bohip.model import _ptr

        m = ms[0]
        mu, var = crafted(2, R)
        value = np.empty(R)
        dmu, dvar = (np.empty((2, R)), np.empty((2, R))) if partials else (None, None)
        best = _lib.Best()
        _lib.check(m._lib.bohip_mo_ehvi_values(m._h, _ptr(FRONT), FRONT.shape[1], _ptr(REF), _ptr(mu), _ptr(var), R, _ptr(value),
                                               _ptr(dmu) if partials else None, _ptr(dvar) if partials else None,
                                               C.byref(best) if record else None))
        return [value] + ([dmu, dvar] if partials else []) + ([np.array([best.val, best.idx])] if record else [])
    return call


def score_con(acq, which, grad):
    """which: the handle of every constraint (0 is the objective's own)."""
    def call(b, ms):
        thr, senses = [-0.3, 0.25, 0.4][:len(which)], [1, -1, -1][:len(which)]
        res = b.ConstrainedGPE(ms[0], [ms[w] for w in which], thr, senses).score(acq, [] if acq == "Feasibility" else [TAU],
                                                                                   xs_of(R_E2E, D_E2E), want_grad=grad)
        return [a for a in res if a is not None]
    return call


def score_mo(second, grad):
    def call(b, ms):
        res = b.score_mo(ms[0], ms[second], FRONT, REF, xs_of(R_E2E, D_E2E), want_grad=grad)
        return [a for a in res if a is not None]
    return call


def throw_away(b, ms):
    for m in ms:
        if m.nobs:
            m.predict_f(xs_of(1, m.dim))
        else:
            con_values(0, 3, False, True)(b, [m])


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
FACTOR, FACTOR_G, REDUCE = ["ens_factor"], ["ens_factor", "ens_alpha"], ["ens_reduce"]
ENS = FACTOR + ["ens_score"] + REDUCE * 2
ENS_G = FACTOR_G + ["ens_grad"] + REDUCE * 2
POST = ["kstar", "trigemm_sq", "con_post"]
POST_G = ["kstar", "trigemm_sq+V", "gemm_U", "con_post"]

# name: (handles, history or None for the throw-away call, the call, capped workspace, the labels of every handle)
TABLE = {
    "ens-fresh": (make_ens, None, ens(3, 20), False, [ENS]),
    "ens_grad-fresh": (make_ens, None, ens_grad(3, 20), False, [ENS_G]),
    "ens_grad-again": (make_ens, [ens_grad(3, 20)], ens_grad(3, 20), False, [["ens_grad"] + REDUCE * 2]),
    "ens_grad-after-ens": (make_ens, [ens(3, 20)], ens_grad(3, 20), False, [ENS_G]),
    "ens-not-resident": (make_ens, None, ens(HC + 1, 20), True, [(FACTOR + ["ens_score"]) * 2 + REDUCE * 2]),
    "ens_grad-not-resident": (make_ens, None, ens_grad(HC + 1, 20), True, [(FACTOR_G + ["ens_grad"]) * 2 + REDUCE * 2]),
    "ens_grad-not-resident-again": (make_ens, [ens_grad(HC + 1, 20)], ens_grad(HC + 1, 20), True,
                                    [(FACTOR_G + ["ens_grad"]) * 2 + REDUCE * 2]),
    "ens-two-chunks": (make_ens, None, ens(3, R2), False, [FACTOR + ["ens_score"] + REDUCE + ["ens_score"] + REDUCE * 2]),
    "ens_grad-two-chunks": (make_ens, None, ens_grad(3, R2), False, [FACTOR_G + ["ens_grad"] + REDUCE + ["ens_grad"] + REDUCE * 2]),
    "mll_grad_batch-two-groups": (make_ens, None, fit(HC + 1), True, [[]]),
    "con_values": (make_anchor, None, con_values(2, 300, False, False), False, [["con_combine"]]),
    "con_values-record": (make_anchor, None, con_values(2, 300, False, True), False, [["con_combine"]]),
    "con_values-partials": (make_anchor, None, con_values(2, 300, True, False), False, [["con_combine"]]),
    "con_values-partials-record": (make_anchor, None, con_values(2, 300, True, True), False, [["con_combine"]]),
    "ehvi_values": (make_anchor, None, ehvi_values(300, False, False), False, [["mo_ehvi"]]),
    "ehvi_values-record": (make_anchor, None, ehvi_values(300, False, True), False, [["mo_ehvi"]]),
    "ehvi_values-partials": (make_anchor, None, ehvi_values(300, True, False), False, [["mo_ehvi"]]),
    "ehvi_values-partials-record": (make_anchor, None, ehvi_values(300, True, True), False, [["mo_ehvi"]]),
    "score_con-C0": (make_members, None, score_con("EI", [], True), False, [POST_G + ["con_combine"], [], []]),
    "score_con-C2": (make_members, None, score_con("EI", [1, 2], True), False, [POST_G + ["con_combine"], POST_G, POST_G]),
    "score_con-C2-value": (make_members, None, score_con("LogEI", [1, 2], False), False, [POST + ["con_combine"], POST, POST]),
    "score_con-C3-repeats": (make_members, None, score_con("EI", [1, 0, 1], True), False, [POST_G * 2 + ["con_combine"], [], []]),
    "score_con-feasibility": (make_members, None, score_con("Feasibility", [1], True), False, [["con_combine"], POST_G, []]),
    "score_mo-two": (make_members, None, score_mo(1, True), False, [POST_G + ["mo_ehvi"], POST_G, []]),
    "score_mo-two-value": (make_members, None, score_mo(2, False), False, [POST + ["mo_ehvi"], [], POST]),
    "score_mo-one-twice": (make_members, None, score_mo(0, True), False, [POST_G * 2 + ["mo_ehvi"], [], []]),
}


def flat(res):
    if isinstance(res, np.ndarray):
        return [res]
    if res is None:
        return []
    if np.isscalar(res):
        return [np.asarray(res)]
    return [a for part in res for a in flat(part)]


def same_bits(got, want):
    got, want = flat(got), flat(want)
    return len(got) == len(want) > 0 and all(a.shape == b.shape and a.dtype == b.dtype and
                                             np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
                                             for a, b in zip(got, want))


def run_case(bohip, name, lived):
    """-> (what the call returns, the labels of every handle or None): on handles that have lived, or as their first call."""
    make, history, call, _, _ = TABLE[name]
    ms = make(bohip)
    try:
        if lived:
            for prior in [throw_away] if history is None else history:
                prior(bohip, ms)
            for m in ms:
                m.enable_timing(True)
        out = call(bohip, ms)
        return out, ([[label for label, _ in m.timing(cap=4096)] for m in ms] if lived else None)
    finally:
        for m in ms:
            m.close()


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


@pytest.mark.parametrize("name", list(TABLE))
def test_labels_and_bits(bohip, name, monkeypatch):
    if TABLE[name][3]:
        monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")                  # read at every call
    want, _ = run_case(bohip, name, lived=False)
    got, seen = run_case(bohip, name, lived=True)
    print(f"  {name}: {seen}")
    assert seen == TABLE[name][4]
    assert same_bits(got, want), "not equal bit for bit to the first call on fresh handles"
