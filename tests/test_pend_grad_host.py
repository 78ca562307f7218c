"""The gradient under pending evaluations without a GPU (include/bohip_pend_grad.h): the analytic gradient of the
extended-precision twin against central differences of its score, the source of the device's bound
(pend_grad_reference.WORST_GRAD) with the condition that makes the device comparison say something, and the ABI in every table
that binds it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pend_grad_reference as pg   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_score_pending_grad"}


@pytest.mark.parametrize("case", ("n17-p1-S1", "n17-p1-S0-R1", "n17-p32-S257"))
@pytest.mark.parametrize("raise_tau", (False, True))
@pytest.mark.parametrize("acq", pg.ACQS)
def test_gradient_is_the_derivative_of_the_score(case, raise_tau, acq):
    """Central differences of the extended twin's SCORE, h = 1e-5 length-scales, against the bound 1e-6 of the largest |component|
    over the candidates: the truncation is (h / r)^2 relative for Matern 1/2, r the distance to the nearest site in length-scales
    (>= 0.02 here: 3e-7; h^2 = 1e-10 for the smooth families), the float64 functor's rounding eps / h ~ 2e-11.  S = 0: the believer."""
    kern, X, y, Xs, Xp, S, seed, params = pg.inputs(case, acq)
    t = pg.Twin(kern, X, y, Xp, np.longdouble)
    Xs, Z = np.asarray(Xs[:24], dtype=np.longdouble), pg.normals(case)
    R, d = Xs.shape
    grad, _ = t.gradient(Xs, acq, params, Z, raise_tau)
    h = np.longdouble(1e-5) * np.exp(np.longdouble(pg.tp.LL))
    steps = np.concatenate([sgn * h * np.eye(d, dtype=np.longdouble) for sgn in (1, -1)])
    sc = t.score((Xs[:, None, :] + steps[None, :, :]).reshape(-1, d), acq, params, Z, raise_tau)[0].reshape(R, 2, d)
    fd = (sc[:, 0, :] - sc[:, 1, :]) / float(2 * h)
    big = float(np.max(np.abs(grad)))
    err = float(np.max(np.abs(np.asarray(grad, dtype=np.float64) - fd)))
    print(f"{case} {acq} raise={raise_tau}: largest component {big:.3g}, worst |analytic - central difference| {err:.3g}")
    assert np.isfinite(fd).all() and big > 0 and err <= 1e-6 * big


def test_tolerance_source_and_inputs_are_not_vacuous():
    """The float64 twin against the extended twin on every input of the device test: the constants WORST_GRAD.  And for every input
    and acquisition: every compared candidate has a finite gradient, and the median over the candidates of the twin's largest
    component is at least 100 device bounds, so a zero or wrong-signed device gradient cannot pass."""
    worst = {k: 0.0 for k in pg.ACQS}
    for case in pg.CASES:
        for acq in pg.ACQS:
            ref = pg.reference(case, acq, pg.RAISE[acq], np.longdouble)["grad"]
            got = pg.reference(case, acq, pg.RAISE[acq])["grad"]
            worst[acq] = max(worst[acq], float(np.max(pg.distance(acq, got, ref))))
            size = float(np.median(pg.distance(acq, np.zeros_like(got), got))) / (pg.DEVICE_FACTOR * pg.WORST_GRAD[acq])
            print(f"{case} {acq}: median gradient {size:.3g} device bounds")
            assert np.isfinite(got).all() and size >= 100, (case, acq, size)
    print("float64 twin against the extended twin, worst gradient figures:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in worst:
        assert worst[k] <= 2 * pg.WORST_GRAD[k], (k, worst[k])
        assert pg.WORST_GRAD[k] <= 2 * worst[k], (k, worst[k], "the stored constant is not the measured one")


def test_header_exports_ctypes_and_julia_agree():
    """include/bohip_pend_grad.h <-> exports <-> _lib.PEND_GRAD_SIGNATURES <-> julia/BOHipPendGrad.jl: the same symbol, the same
    types argument by argument, not in the model's table nor in bohip_pend.h's."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_pend_grad.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double*": "ptr(double)", "bohip_gp*": "ptr(void)", "int64_t": "int64", "uint64_t": "uint64",
               "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.PEND_GRAD_SIGNATURES)
    assert not WANT & (set(_lib.SIGNATURES) | set(_lib.PEND_SIGNATURES)) and len(_lib.PEND_SIGNATURES) == 4
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipPendGrad.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in WANT:
        assert hasattr(lib, name), name
        res, args = _lib.PEND_GRAD_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipPendGrad.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
