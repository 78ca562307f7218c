"""Greedy q-EHVI without a GPU: the ABI of include/bohip_qehvi.h in every table that binds it, the argument errors that are reported
before any device work, and the option plumbing of acquire_batch's "qehvi" method and of BOpt on duck-typed members."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT   # noqa: E402
from test_mo_host import Duck   # noqa: E402

WANT = {"bohip_mo_qehvi_select", "bohip_gp_qehvi_batch"}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int64)


def test_qehvi_header_exports_ctypes_and_julia_agree():
    """Header <-> exports <-> _lib.QEHVI_SIGNATURES <-> julia/BOHipQEHVI.jl: the same symbols and types, in no other table."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_qehvi.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "uint64_t": "uint64", "double": "double", "double*": "ptr(double)",
               "int64_t*": "ptr(int64)", "int*": "ptr(int)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.QEHVI_SIGNATURES)
    assert not any(WANT & set(getattr(_lib, k)) for k in vars(_lib) if k.endswith("SIGNATURES") and k != "QEHVI_SIGNATURES")
    assert len(_lib.SIGNATURES) == 62 and "0x9E3779B97F4A7C15" in raw and _lib.QEHVI_SEED_XOR == 0x9E3779B97F4A7C15
    assert re.search(r"#define BOHIP_QEHVI_QMAX (\d+)", raw).group(1) == str(_lib.QEHVI_QMAX)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_double: "double", C.c_void_p: "ptr(void)", DP: "ptr(double)",
          IP: "ptr(int64)", C.POINTER(C.c_int): "ptr(int)"}
    jl_types = {"Cint": "int", "Int64": "int64", "UInt64": "uint64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)", "Ptr{Cint}": "ptr(int)"}
    src = open(os.path.join(ROOT, "julia", "BOHipQEHVI.jl")).read()
    jl = {m.group(1): [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
          for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src)}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in sorted(WANT):
        res, args = _lib.QEHVI_SIGNATURES[name]
        assert hasattr(lib, name) and [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert set(jl) == WANT and 'include("BOHipQEHVI.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()


BAD = [  # (what is wrong, changes to the good arguments of bohip_mo_qehvi_select, code, a word of the message)
    ("null handle", dict(gp=None), "E_ARG", b"null"),
    ("front not descending in f2", dict(front=[1.0, 2.0, 1.0, 1.0]), "E_ARG", b"descend"),
    ("front beyond the limit", dict(n_front=1025), "E_UNSUPPORTED", b"1024"),
    ("q > R", dict(q=3), "E_ARG", b"exceeds"),
    ("q beyond the limit", dict(q=17, R=32, S=1), "E_UNSUPPORTED", b"QMAX"),
    ("workspace above 8 GiB", dict(S=1 << 20, R=1 << 12), "E_UNSUPPORTED", b"8 GiB"),
]


@pytest.mark.parametrize("what,change,code,word", BAD, ids=[b[0] for b in BAD])
def test_argument_errors_come_before_any_device_work(what, change, code, word):
    from bohip import _lib

    lib = _lib.load()
    a = {**dict(gp=C.c_void_p(8), front=[1.0, 2.0, 2.0, 1.0], n_front=2, ref=[0.0, 0.0], S=2, R=2, q=1), **change}
    F, front, ref = np.zeros(1024), np.zeros(2 * 1025), np.asarray(a["ref"], dtype=np.float64)
    front[:4] = a["front"]
    idx, gain = np.zeros(32, dtype=np.int64), np.zeros(32)
    rc = lib.bohip_mo_qehvi_select(a["gp"], F.ctypes.data_as(DP), F.ctypes.data_as(DP), a["S"], a["R"], front.ctypes.data_as(DP), a["n_front"],
                                   ref.ctypes.data_as(DP), a["q"], idx.ctypes.data_as(IP), gain.ctypes.data_as(DP))
    assert rc == getattr(_lib, code) and word in lib.bohip_last_error(), (rc, lib.bohip_last_error())
    if a["gp"] is None:
        assert lib.bohip_gp_qehvi_batch(None, None, front.ctypes.data_as(DP), 2, ref.ctypes.data_as(DP), F.ctypes.data_as(DP), 2, 2, 0, 1e-12, 40,
                                        1, idx.ctypes.data_as(IP), gain.ctypes.data_as(DP), None, None, None) == _lib.E_ARG


def duck_model(many=False):   # duck-typed members; records qehvi_batch and answers with the first q candidates
    from bohip.model import ManyObjectiveGPE, MultiObjectiveGPE, QEIBatch

    class Rec(ManyObjectiveGPE if many else MultiObjectiveGPE):
        def qehvi_batch(self, xs, q, S=256, seed=0, jitter=1e-12, max_tries=40, want_samples=False):
            self.calls.append((xs.shape, q, S, seed))
            return QEIBatch(np.arange(q, dtype=np.int64), np.linspace(1.0, 0.5, q), np.zeros(2), np.zeros(2, dtype=np.int32), None)

    m = Rec((Duck(2), Duck(2)), ref=[-1.0, -1.0])
    m.calls = []
    return m.update_(np.random.default_rng(0).random((2, 3)), np.random.default_rng(1).random((2, 3)))


LB, UB = np.zeros(2), np.ones(2)


def test_acquire_batch_reaches_qehvi_batch_and_refuses_what_it_cannot_mean():
    import bohip

    a, m = bohip.ExpectedHypervolumeImprovement(), duck_model()
    seed = int(np.random.default_rng(9).integers(0, 2 ** 63 - 1))
    xs = np.asfortranarray(np.random.default_rng(2).random((2, 12)))
    val, X = bohip.acquire_batch(a, m, LB, UB, 3, {"method": "qehvi", "xs": xs, "draws": 32}, np.random.default_rng(9))
    assert m.calls == [((2, 12), 3, 32, seed)] and val.tolist() == [1.0, 0.75, 0.5]
    np.testing.assert_array_equal(X, xs[:, :3])                           # the marginal gains and X as d x q
    for k in ("fantasy", "raise_tau", "pathwise", "features", "refine"):
        with pytest.raises(ValueError, match="does not go with method 'qehvi'"):
            bohip.acquire_batch(a, m, LB, UB, 2, {"method": "qehvi", k: 1})
    with pytest.raises(ValueError, match="ExpectedHypervolumeImprovement"):
        bohip.acquire_batch(bohip.ExpectedImprovement(), m, LB, UB, 2, {"method": "qehvi"})
    with pytest.raises(ValueError, match="MultiObjectiveGPE"):
        bohip.acquire_batch(a, Duck(2), LB, UB, 2, {"method": "qehvi"})
    with pytest.raises(ValueError, match="two objectives only"):
        bohip.acquire_batch(a, duck_model(many=True), LB, UB, 2, {"method": "qehvi"})
    with pytest.raises(ValueError, match="two objectives only"):
        bohip.model.ManyObjectiveGPE((Duck(2), Duck(2)), ref=[0.0, 0.0]).qehvi_select(np.zeros((1, 1)), np.zeros((1, 1)), 1)
    assert len(m.calls) == 1


def test_bopt_runs_one_selection_and_one_update_per_iteration():
    import bohip

    m = duck_model()
    kw = dict(verbosity=bohip.Silent, maxiterations=2, initializer_iterations=0, rng=np.random.default_rng(0), batchsize=3)
    a, opt, two = bohip.ExpectedHypervolumeImprovement(), bohip.NoModelOptimizer(), lambda x: (x[0], 1.0 - x[0])
    with pytest.raises(ValueError, match="one point per iteration"):
        bohip.BOpt(two, m, a, opt, LB, UB, batchoptions={"method": "fantasy"}, **kw)
    with pytest.raises(ValueError, match="two objectives only"):
        bohip.BOpt(two, duck_model(many=True), a, opt, LB, UB, batchoptions={"method": "qehvi"}, **kw)
    out = bohip.boptimize_(bohip.BOpt(two, m, a, opt, LB, UB, batchoptions={"method": "qehvi", "candidates": 9}, **kw))
    assert [c[:3] for c in m.calls] == [((2, 9), 3, 256)] * 2 and m.nobs == 3 + 2 * 3 and out["observed_front"]["y"].shape[0] == 2
