"""The batched leave-one-out objective without a GPU (include/bohip_loo_batch.h): the ABI in every table that binds
it, the fit's dispatch, and the NumPy restatement of the kernel's algebra (tests/loo_batch_reference.py) against the twin of the
resident path (tests/loo_reference.py).

Bounds.  Both twins are float64 evaluations of the same quantities from the same cK, condition <= 3e3 at the BASELINE setting used
here, by different routes (an explicit inverse factor against a library solve): they differ by ~ eps x condition ~ 1e-12 relative;
1e-10 of the largest magnitude is asked, as tests/test_loo_host.py asks of the fast formula against brute force."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_batch_reference as lb   # noqa: E402
import loo_reference as lr   # noqa: E402
from conftest import ROOT, synth   # noqa: E402
from matern_reference import KERNELS   # noqa: E402

WANT = {"bohip_gp_loo_grad_batch"}
BOUND = 1e-10


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_loo_batch_header_exports_ctypes_and_julia_agree():
    """include/bohip_loo_batch.h <-> exports <-> _lib.LOO_BATCH_SIGNATURES <-> julia/BOHipLOOBatch.jl: the one symbol, the same
    types argument by argument, and in no other header or table."""
    from bohip import _lib

    def protos_of(name):
        raw = open(os.path.join(ROOT, "include", name)).read()
        hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
        return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr)}

    c_types = {"int": "int", "int64_t": "i64", "double*": "ptr(double)", "int64_t*": "ptr(i64)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for name, (res, arglist) in protos_of("bohip_loo_batch.h").items():
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in arglist.split(",")]
        protos[name] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [res] + args]
    assert set(protos) == WANT == set(_lib.LOO_BATCH_SIGNATURES)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "bohip_loo_batch.h":
            assert not WANT & set(protos_of(other)), other
    tables = [k for k in vars(_lib) if k.endswith("SIGNATURES") and k != "LOO_BATCH_SIGNATURES"]
    assert {"SIGNATURES", "FIT_SIGNATURES", "LOO_SIGNATURES"} <= set(tables)
    for k in tables:
        assert not WANT & set(getattr(_lib, k)), k
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "i64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int64): "ptr(i64)"}
    jl_types = {"Cint": "int", "Int64": "i64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(i64)"}
    src = open(os.path.join(ROOT, "julia", "BOHipLOOBatch.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.LOO_BATCH_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
        assert getattr(_lib.load(), name).argtypes == args               # bound by the load loop
    assert protos["bohip_gp_loo_grad_batch"] == ["int", "ptr(void)", "i64"] + ["ptr(double)"] * 4 + ["ptr(i64)"]
    for f in os.listdir(os.path.join(ROOT, "julia")):
        if f.endswith(".jl") and f != "BOHipLOOBatch.jl":
            assert ":bohip_gp_loo_grad_batch" not in open(os.path.join(ROOT, "julia", f)).read(), f
    assert 'include("BOHipLOOBatch.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert re.search(r"^function loo_grad_batch\(", src, flags=re.M)
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_arguments_are_argument_errors():
    from bohip import _lib

    full = _lib.load()
    out = np.zeros(8)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    fake = C.c_void_p(8)                                           # never dereferenced: theta / total are looked at first
    assert full.bohip_gp_loo_grad_batch(None, 1, p, p, p, p, None) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()
    assert full.bohip_gp_loo_grad_batch(fake, 1, None, p, p, p, None) == _lib.E_ARG
    assert full.bohip_gp_loo_grad_batch(fake, 1, p, None, p, p, None) == _lib.E_ARG
    assert np.all(out == 0.0)


# ---- the fit's dispatch ---------------------------------------------------------------------------------------------------------
class FakeBatchModel:
    """Has loo_grad_batch, whose answer names its slots; every other objective call is a failure of the test."""

    def __init__(self, mean_const):
        from bohip.model import MeanConst, MeanZero, SEArd

        self.kernel, self.mean, self.logNoise, self.nobs = SEArd([0.1, 0.2], 0.3), MeanConst(0.5) if mean_const else MeanZero(), -1.0, 9
        self.calls = []

    def mll_batch_dims(self):
        return 5, 512

    def loo_grad_batch(self, Theta, want_grad=True, want_logp=False):
        assert not want_logp
        self.calls.append((np.array(Theta), want_grad))
        H = Theta.shape[0]
        G = np.tile(np.array([10.0, 20.0, 30.0, 31.0, 40.0]), (H, 1)) + np.arange(H)[:, None] * 0.5 if want_grad else None
        piv = np.zeros(H, dtype=np.int64)
        piv[3] = 7                                                  # a failed row: whatever its total says, the fit sees -inf
        return 100.0 + np.arange(H), G, piv

    def refuse(self, *a, **kw):
        raise AssertionError("another objective call was made")

    loo_grad = loo = mll = mll_grad = mll_grad_batch = set_params_ = refuse


@pytest.mark.parametrize("mean_const", [True, False])
def test_fit_objective_loo_takes_one_batched_call_and_maps_the_slots(mean_const):
    from bohip.bopt import _FIT_BATCH_MIN_H, _LOO_BATCH_MIN_H, _fit_objective

    assert _FIT_BATCH_MIN_H == ((64, 2), (128, 2), (256, 2), (512, 8))
    assert all(len(r) == 2 for r in _LOO_BATCH_MIN_H) and [r[0] for r in _LOO_BATCH_MIN_H] == [64, 128, 256, 512]
    m = FakeBatchModel(mean_const)
    opt = dict(domean=True, noise=False, kern=True, objective="loo")
    p = 4 if mean_const else 3
    fg = _fit_objective(m, opt, 3, m.refuse, p, 8)
    X = np.arange(p * 8, dtype=float).reshape(p, 8)
    f, G = fg(X)
    assert len(m.calls) == 1 and m.calls[0][1] is True
    Theta = m.calls[0][0]
    assert Theta.shape == (8, 5)
    idx = [1, 2, 3, 4] if mean_const else [2, 3, 4]               # of [noise, mean, ll0, ll1, lsigma]
    np.testing.assert_array_equal(Theta[:, idx], X.T)
    np.testing.assert_array_equal(Theta[:, 0], np.full(8, -1.0))   # the fixed noise rides along as a constant
    if not mean_const:
        np.testing.assert_array_equal(Theta[:, 1], np.zeros(8))
    want_f = 100.0 + np.arange(8)
    want_f[3] = -np.inf
    np.testing.assert_array_equal(f, want_f)
    want = np.array([20.0, 30.0, 31.0, 40.0] if mean_const else [30.0, 31.0, 40.0])
    np.testing.assert_array_equal(G, want[:, None] + np.arange(8)[None, :] * 0.5)
    # value only: one more call, no gradient asked for or returned
    f2, G2 = _fit_objective(m, opt, 3, m.refuse, p, 8, want_grad=False)(X)
    assert len(m.calls) == 2 and m.calls[1][1] is False and G2 is None
    np.testing.assert_array_equal(f2, want_f)
    # one column is below the table's entry: the loop (which this fake refuses)
    with pytest.raises(AssertionError, match="another objective"):
        _fit_objective(m, opt, 3, m.refuse, p, 1)(X[:, :1])


# ---- the kernel's algebra, restated ---------------------------------------------------------------------------------------------
def setting(kern, d, beta):
    nl = 1 if KERNELS[kern][1] else d
    return np.concatenate([[-2.0, beta], np.full(nl, math.log(0.5)) + 0.05 * np.arange(nl), [0.0]])


def errors(kern, N, beta, mask=True):
    X, y, _ = synth(N, 3, 1, seed=60 + N)
    t = setting(kern, 3, beta)
    tot, g, logp = lb.twin(kern, X, y, t, mask=mask)
    tot_ref, g_ref = lr.grad_vec(kern, X, y, t)
    fast = lr.loo_fast(kern, X, y, t[2:-1], t[-1], t[0], t[1])
    return (abs(tot - tot_ref) / abs(tot_ref), np.abs(g - g_ref).max() / np.abs(g_ref).max(),
            np.abs(logp - fast[2]).max() / np.abs(fast[2]).max(), abs(tot - fast[3]) / abs(fast[3]))


@pytest.mark.parametrize("beta", [0.0, 0.3], ids=["MeanZero", "MeanConst"])
@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("N", [1, 2, 16, 17, 33])
def test_restated_algebra_is_the_reference(kern, N, beta):
    e = errors(kern, N, beta)
    print(f"{kern} N={N} beta={beta}: total {e[0]:.2e} grad {e[1]:.2e} logp {e[2]:.2e} total/fast {e[3]:.2e}")
    assert max(e) <= BOUND


def test_the_shapes_can_see_a_missing_padding_mask():
    """N = 17 has fifteen identity rows.  Without the mask each of them adds -1/2 log 2 pi to the total."""
    e = errors("Mat52Ard", 17, 0.3, mask=False)
    print("unmasked:", e)
    assert max(e) > 100 * BOUND
    assert max(errors("Mat52Ard", 16, 0.3, mask=False)) <= BOUND   # (no padding at 16: nothing to mask)
