"""The knowledge gradient at free points without a GPU (include/bohip_kg_grad.h): the ABI in every table that binds it,
the twin's analytic gradient against central differences of its own value at extended precision, the source of the device's bound
(kg_grad_reference.WORST_GRAD) with the cases the device inputs must contain."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_grad_reference as kgr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_kg_set_points", "bohip_gp_kg_points_info", "bohip_gp_kg_grad"}


def test_header_exports_ctypes_and_julia_agree():
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_kg_grad.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double*": "ptr(double)", "bohip_gp*": "ptr(void)", "int64_t": "int64", "int32_t*": "ptr(int32)",
               "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.KG_GRAD_SIGNATURES)
    assert not WANT & (set(_lib.SIGNATURES) | set(_lib.KG_SIGNATURES)) and len(_lib.SIGNATURES) == 62 and len(_lib.KG_SIGNATURES) == 2
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int32): "ptr(int32)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)", "Ptr{Int32}": "ptr(int32)",
                "Ptr{Best}": "ptr(best)"}
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", open(os.path.join(ROOT, "julia", "BOHipKGGrad.jl")).read()):
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in WANT:
        assert hasattr(lib, name), name
        res, args = _lib.KG_GRAD_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipKGGrad.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    for k in ("R", "REBUILDS", "BYTES", "LINES", "LINE_ROWS"):
        assert f"#define BOHIP_KG_POINTS_{k} {getattr(_lib, 'KG_POINTS_' + k)}\n" in raw


@pytest.mark.parametrize("case", [c for c in kgr.CASES if c[1] == 40 or c[5] > 0], ids=str)
def test_gradient_is_the_derivative_of_the_value(case):
    """Central differences of the extended twin's own value, h = 1e-5 length-scales: truncation O(h^2) ~ 1e-10, the float64 erfc inside
    ~ 1e-16 / h ~ 1e-11, against 1e-6 of the largest |component| over the points.  Not at x = a_0, where KG has a kink
    (kg_grad_reference's docstring), and not at Matern 1/2's observed site, a kink of the kernel itself."""
    t = kgr.Twin(kgr.case_data(case), np.longdouble)
    c, d = t.c, t.c["Xe"].shape[1]
    h = np.longdouble(1e-5) * np.exp(np.longdouble(c["ll"][0]))
    big = err = 0.0
    for e, x in enumerate(c["Xe"][:8]):
        if e == c["dup"] or (e == 2 and c["kern"] == "Mat12Ard"):
            continue
        g = t.point(x)[2]
        x = np.asarray(x, dtype=np.longdouble)
        fd = np.array([float((t.point(x + h * u)[7] - t.point(x - h * u)[7]) / (2 * h)) for u in np.eye(d, dtype=np.longdouble)])
        big, err = max(big, float(np.max(np.abs(g)))), max(err, float(np.max(np.abs(np.asarray(g, dtype=np.float64) - fd))))
    print(f"{case}: largest component {big:.3g}, worst |analytic - central difference| {err:.3g}")
    assert big > 0 and err <= 1e-6 * big


def test_tolerance_source():
    """The float64 twin against the extended twin on every input of the device test: kg_grad_reference.WORST_GRAD.  And the cases the
    inputs must contain: the own line inside the envelope, as the strict arg-max of the intercepts, absent from the envelope."""
    worst, seen = 0.0, {"inside": 0, "top": 0, "absent": 0, "dup": 0}
    for case in kgr.CASES:
        (t, lo), (_, hi) = kgr.reference(case), kgr.reference(case, np.longdouble)
        R = case[3]
        for e, (a, b) in enumerate(zip(lo, hi)):
            env = a[6]
            seen["absent"] += R not in env
            seen["inside"] += R in env[1:-1]
            seen["top"] += bool(R == 0 or a[3] > t.muA.max())
            if e == t.c["dup"]:
                seen["dup"] += 1
                continue
            # (the two twins may walk envelopes that differ in segments of no width -- near-collinear lines -- whose q is of no size)
            worst = max(worst, float(np.max(np.abs(a[2] - np.asarray(b[2], dtype=np.float64)))) / kgr.unit(t.c))
    print(f"float64 twin against the extended twin, worst gradient distance {worst:.3g}; stored {kgr.WORST_GRAD:.3g}; cases {seen}")
    assert all(v > 0 for v in seen.values()), seen
    assert worst <= 2 * kgr.WORST_GRAD and kgr.WORST_GRAD <= 2 * worst
