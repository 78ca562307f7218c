"""The gradient of noisy expected improvement without a GPU (include/bohip_nei_grad.h): the analytic gradient of the
extended-precision twin against central differences of its score, the source of the device's bound (nei_grad_reference.WORST_GRAD),
the two conditions the device inputs must meet, and the ABI in every table that binds it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nei_grad_reference as ng   # noqa: E402
import nei_reference as nr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_score_nei_grad"}


@pytest.mark.parametrize("model", list(nr.MODELS))
@pytest.mark.parametrize("S", (0, 5))
@pytest.mark.parametrize("acq", nr.ACQS)
def test_gradient_is_the_derivative_of_the_score(model, S, acq):
    """Central differences of the extended twin's score (nei_reference.score), h = 1e-4 length-scales: truncation O(h^2) ~ 1e-8,
    rounding of the float64 functor ~ eps / h ~ 2e-12, against the bound 1e-6 of the largest |component| over the candidates."""
    N, R = 17, 36
    tag = (model, N)
    t = nr.twin(tag, nr.JREL, np.longdouble)
    Xs = np.asarray(nr.spec(tag)["Xs"][:R], dtype=np.longdouble)
    _, tau, alpha = t.fantasies(*nr.normals(nr.SEED, S, N))
    grad, _ = ng.gradient(t, Xs, alpha, tau, acq)
    d = Xs.shape[1]
    h = np.longdouble(1e-4) * np.exp(np.longdouble(nr.MODELS[model]["ll"]))
    steps = np.concatenate([sgn * h * np.eye(d, dtype=np.longdouble) for sgn in (1, -1)])      # (2 d, d)
    P = (Xs[:, None, :] + steps[None, :, :]).reshape(-1, d)
    m, s2 = t.moments(P, alpha)
    sc = nr.score(acq, m, s2, tau)[0].reshape(R, 2, d)
    fd = (sc[:, 0, :] - sc[:, 1, :]) / float(2 * h)
    fin = np.isfinite(fd).all(axis=1)
    big = float(np.max(np.abs(grad[fin])))
    err = float(np.max(np.abs(np.asarray(grad, dtype=np.float64) - fd)[fin]))
    print(f"{model} S={S} {acq}: largest component {big:.3g}, worst |analytic - central difference| {err:.3g} = {err / big:.3g} of it")
    assert fin.sum() >= R - 1 and big > 0 and err <= 1e-6 * big


def test_tolerance_source():
    """The float64 twin against the extended twin on every input of the device test: the constants nei_grad_reference.WORST_GRAD."""
    worst = {k: 0.0 for k in ng.WORST_GRAD}
    for tag, R, S in ng.all_inputs():
        for acq in nr.ACQS:
            ref = ng.reference(tag, S, acq, dt=np.longdouble)
            got = ng.reference(tag, S, acq)["grad"]
            worst[acq] = max(worst[acq], float(np.max(ng.distance(acq, got[:R], dict(ref, grad=ref["grad"][:R])))))
    print("float64 twin against the extended twin, worst gradient figures:", {k: f"{v:.3g}" for k, v in worst.items()})
    print("nei_grad_reference.WORST_GRAD:", ng.WORST_GRAD)
    for k in worst:
        assert worst[k] <= 2 * ng.WORST_GRAD[k], (k, worst[k])
        assert ng.WORST_GRAD[k] <= 2 * worst[k], (k, "the stored constant is not the measured one")


def test_device_inputs_are_well_conditioned():
    """cond(K_d) at jitter_rel = 1e-6 stays below 1e9 for every (model, N) of the device test."""
    for model in nr.MODELS:
        for N in ng.NS:
            c = nr.twin((model, N)).cond_kd()
            print(f"{model} N = {N}: cond(K_d) = {c:.3g}")
            assert c < 1e9
    assert nr.Twin(**{k: v for k, v in ng.d20_spec().items() if k != "Xs"}, jitter_rel=nr.JREL).cond_kd() < 1e9


def test_device_inputs_are_not_vacuous():
    """For every input and acquisition of the device test: fewer than 1 % of the candidates have a twin score of exactly 0 or -Inf,
    and the twin's gradient is large against what the device is granted -- the median over the candidates of the largest component is
    at least 100 device bounds (16 x WORST_GRAD, in nei_grad_reference.distance's units), so a zero or wrong-signed device gradient
    cannot pass.  At synth's own candidates EI and PI miss the first on 63 of the 165 (input, acquisition) pairs, up to 100 % dead from
    se3 N = 129 on: nei_grad_reference.FAR_SHIFT / RING say where they are compared instead."""
    for tag, R, S in ng.all_inputs():
        for acq in nr.ACQS:
            ref = ng.reference(tag, S, acq)
            sc = ref["score"][:R]
            dead = float(np.mean((sc == 0.0) | (sc == -np.inf)))
            size = float(np.median(ng.distance(acq, np.zeros_like(ref["grad"][:R]), dict(ref, grad=ref["grad"][:R]))))
            bounds = size / (nr.DEVICE_FACTOR * ng.WORST_GRAD[acq])
            print(f"{tag} S={S} {acq}: dead {dead:.3f}, median gradient {bounds:.3g} device bounds")
            assert dead < 0.01 and bounds >= 100, (tag, S, acq, dead, bounds)


def test_header_exports_ctypes_and_julia_agree():
    """include/bohip_nei_grad.h <-> exports <-> _lib.NEI_GRAD_SIGNATURES <-> julia/BOHipNEIGrad.jl: the same symbol, the same types
    argument by argument, not in the model's header or table nor in bohip_nei.h's."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_nei_grad.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double": "double", "double*": "ptr(double)", "bohip_gp*": "ptr(void)", "int64_t": "int64", "uint64_t": "uint64",
               "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.NEI_GRAD_SIGNATURES)
    assert not WANT & (set(_lib.SIGNATURES) | set(_lib.NEI_SIGNATURES)) and len(_lib.NEI_SIGNATURES) == 6
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_double: "double", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Float64": "double", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipNEIGrad.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in WANT:
        assert hasattr(lib, name), name
        res, args = _lib.NEI_GRAD_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipNEIGrad.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert re.search(r"^function nei_grad\(", src, flags=re.M)
