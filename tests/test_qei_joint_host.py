"""The joint q-EI of a batch without a GPU (include/bohip_qei_joint.h): the twin's gradient against central differences
of its own value, the condition that makes the arg-max of every case unambiguous, the source of the device's bound
(qei_joint_reference.WORST_VALUE / WORST_GRAD), the ABI in every table that binds it, and acquire_batch's option plumbing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qei_joint_reference as qj   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_qei_joint"}


@pytest.mark.parametrize("case", ("se-n129-q2-B1-S70", "m52-n129-q5-B1-S1024", "m12-n129-q2-B1-S1", "m52-n129-q16-B1-S70"))
def test_gradient_is_the_derivative_of_the_value(case):
    """Central differences of the float64 twin's VALUE, h = 1e-5 length-scales, against 1e-5 of the largest |component|: the
    truncation is h^2 = 1e-10 relative for the smooth families and (h / r)^2 for Matern 1/2 (r >= 0.02 length-scales to the nearest
    site: 3e-7); the value's rounding (1e-13 s_f, WORST_VALUE) over h is 4e-8 s_f / l at q = 16 with its condition number, 1e-9
    elsewhere.  The margin (asserted in the next test) keeps every sample's arg-max and sign fixed over steps of this size."""
    ref = qj.reference(case)
    t = qj._REF[ref["kern"], ref["X"].shape, np.float64]
    Xs, q, Z = ref["Xs"][:ref["q"]], ref["q"], qj.normals(ref["seed"], ref["S"])
    d = Xs.shape[1]
    h = 1e-5 * np.exp(qj.tp.LL)
    fd = np.empty((q, d))
    for j in range(q):
        for k in range(d):
            e = np.zeros((q, d))
            e[j, k] = h
            fd[j, k] = (t.qei(Xs + e, q, Z, ref["tau"], want_grad=False)[0][0] - t.qei(Xs - e, q, Z, ref["tau"], want_grad=False)[0][0]) / (2 * h)
    grad = ref["grad"][:q]
    big, err = float(np.max(np.abs(grad))), float(np.max(np.abs(grad - fd)))
    print(f"{case}: largest component {big:.3g}, worst |analytic - central difference| {err:.3g}")
    assert big > 0 and err <= 1e-5 * big


def test_tolerance_source_and_the_arg_max_is_unambiguous():
    """The float64 twin against the extended twin on every case: the constants WORST_VALUE / WORST_GRAD.  In the extended twin every
    sample's best entry stays MARGIN above the second and away from tau, no group is flagged, and every case has a value above zero
    and a gradient of at least 100 device bounds, so that a zero or wrong-signed device gradient cannot pass."""
    wv = wg = 0.0
    for case in qj.CASES:
        ext, ref = qj.reference(case, np.longdouble), qj.reference(case)
        dv, dg = qj.distances(ref["value"], ref["grad"], ext)
        size = qj.distances(ref["value"], np.zeros_like(ref["grad"]), ref)[1] / (qj.DEVICE_FACTOR * qj.WORST_GRAD)
        print(f"{case}: margin {ext['margin']:.3g}, value {dv:.3g}, gradient {dg:.3g}, largest gradient {size:.3g} device bounds")
        assert ext["margin"] > qj.MARGIN and not ext["pivot"].any() and not ref["pivot"].any(), case
        assert float(np.min(ref["value"])) >= 0 and float(np.max(ref["value"])) > 0 and size >= 100, case
        wv, wg = max(wv, dv), max(wg, dg)
    print(f"float64 twin against the extended twin, worst figures: value {wv:.3g}, gradient {wg:.3g}")
    for got, pinned in ((wv, qj.WORST_VALUE), (wg, qj.WORST_GRAD)):
        assert got <= 2 * pinned and pinned <= 2 * got, (got, pinned, "the stored constant is not the measured one")


def test_header_exports_ctypes_and_julia_agree():
    """include/bohip_qei_joint.h <-> exports <-> _lib.QEI_JOINT_SIGNATURES <-> julia/BOHipQEIJoint.jl: the same symbol, the same types
    argument by argument, not in the model's table nor in bohip_qei.h's; the limits' names."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_qei_joint.h")).read()
    assert (f"#define BOHIP_QEIJ_QMAX {_lib.QEIJ_QMAX}\n" in raw) and (f"#define BOHIP_QEIJ_SMAX {_lib.QEIJ_SMAX}\n" in raw)
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double": "double", "double*": "ptr(double)", "bohip_gp*": "ptr(void)", "int64_t": "int64",
               "uint64_t": "uint64", "int64_t*": "ptr(int64)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.QEI_JOINT_SIGNATURES)
    assert not WANT & (set(_lib.SIGNATURES) | set(_lib.QEI_SIGNATURES)) and len(_lib.QEI_SIGNATURES) == 2
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_double: "double", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int64): "ptr(int64)"}
    jl_types = {"Cint": "int", "Float64": "double", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)"}
    src = open(os.path.join(ROOT, "julia", "BOHipQEIJoint.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in WANT:
        assert hasattr(lib, name), name
        res, args = _lib.QEI_JOINT_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipQEIJoint.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()


class _Model:
    """What acquire_batch reads of a model on the "qei" route, recording the calls."""
    nobs, y = 3, np.zeros(3)

    def __init__(self):
        self.calls = []

    def qei_batch(self, xs, q, draws, seed, tau=None):
        self.calls.append("qei_batch")
        return type("R", (), dict(idx=np.arange(q), gain=np.ones(q)))

    def qei_joint(self, X, q, draws, seed, tau=None):
        self.calls.append("qei_joint")
        return -np.sum((X - 0.5) ** 2, axis=0).reshape(-1, q).sum(axis=1), -2 * (X - 0.5), np.zeros(X.shape[1] // q, dtype=np.int64)


def test_option_plumbing():
    """ "refine" without "method": "qei" raises like the other misplaced batch options; refine = 0 makes the calls and draws of a call
    without the key (the generators end in the same state); refine = 3 climbs model.qei_joint and returns one batch in the box."""
    import bohip

    a, lb, ub = bohip.ExpectedImprovement(0.0), np.zeros(2), np.ones(2)
    with pytest.raises(ValueError, match="needs 'method': 'qei'"):
        bohip.acquire_batch(a, _Model(), lb, ub, 2, {"refine": 2}, setparams=False)
    out = []
    for opts in ({"method": "qei", "candidates": 16}, {"method": "qei", "candidates": 16, "refine": 0}):
        m, rng = _Model(), np.random.default_rng(5)
        v, X = bohip.acquire_batch(a, m, lb, ub, 2, opts, rng=rng, setparams=False)
        out.append((v.tobytes(), X.tobytes(), m.calls, rng.bit_generator.state))
    assert out[0] == out[1] and out[0][2] == ["qei_batch"]
    m = _Model()
    v, X = bohip.acquire_batch(a, m, lb, ub, 2, {"method": "qei", "candidates": 16, "refine": 3}, rng=np.random.default_rng(5), setparams=False)
    assert v.shape == (1,) and X.shape == (2, 2) and "qei_joint" in m.calls and np.all((X >= lb[:, None]) & (X <= ub[:, None]))
    assert np.allclose(X, 0.5, atol=1e-6)
