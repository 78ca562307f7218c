"""GPU tests of the knowledge gradient at free points and its gradient (include/bohip_kg_grad.h): bohip_gp_kg_set_points,
bohip_gp_kg_grad, ElasticGPE.kg_set_points / kg_grad, KnowledgeGradient under acquire_max's "refine".

The reference is the header's definition in NumPy (tests/kg_grad_reference.py, float64 twin).  The gradient's bound is
nei_reference.DEVICE_FACTOR x kg_grad_reference.WORST_GRAD -- the float64 twin's own distance from its extended-precision twin on these
very inputs (tests/test_kg_grad_host.py test_tolerance_source) -- in nei_grad_reference.distance's measure; the values are held to
test_kg_gpu's bounds: bit for bit against bohip_kg_lines on the device's own lines, ORACLE_ABS against the extended twin's value.  Every comparison
prints the share of the bound it uses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_grad_reference as kgr   # noqa: E402
import nei_reference as nr   # noqa: E402
from test_kg_gpu import ORACLE_ABS   # noqa: E402
from test_nei_gpu import bohip, model_of   # noqa: E402, F401

pytestmark = pytest.mark.gpu
BOUND = nr.DEVICE_FACTOR * kgr.WORST_GRAD


@pytest.mark.parametrize("case", kgr.CASES, ids=str)
def test_value_and_gradient(bohip, case):
    t, ref = kgr.reference(case)
    ext = kgr.reference(case, np.longdouble)[1]                         # the values' reference: the float64 twin's own value error
    # reaches 4.2e-14 of max(1, max|mu|) at N = 1536 (Mat52Ard, d = 20), more than ORACLE_ABS itself
    c, R = t.c, case[3]
    m = model_of(bohip, c, lnoise=c["lnoise"])
    m.enable_timing(True)
    muA = m.kg(c["A"].T).mu                                             # (the pass kg_set_points' state is built by)
    m.kg_set_points(c["A"].T)
    res, g = m.kg_grad(c["Xe"].T)
    assert all(k in [n for n, _ in m.timing()] for k in ("kg_cross", "kg_march_w", "kg_mix", "kg_grad_finish"))
    again, g2 = m.kg_grad(c["Xe"].T)                                    # identical bytes, nothing rebuilt
    assert (again.values.tobytes(), again.nseg.tobytes(), g2.tobytes()) == (res.values.tobytes(), res.nseg.tobytes(), g.tobytes())
    assert m.kg_points_info()["rebuilds"] == 1 and m.kg_points_info()["R"] == R
    lines = m.kg_last_lines()
    assert lines.shape == (len(c["Xe"]), R + 1) and lines[:, R].tobytes() == res.var.tobytes()
    nu = np.float64(c["nu"])
    worst_v = worst_g = 0.0
    for e, x in enumerate(c["Xe"]):
        s = np.sqrt(lines[e, R] + nu)                                   # bohip_kg_lines on the device's own lines: the same bits
        kv, ks = m.kg_lines(np.append(muA, res.mu[e]), (lines[e] / s)[None, :])
        assert (kv[0], ks[0]) == (res.values[e], res.nseg[e]), (case, e, kv, ks, res.values[e], res.nseg[e])
        worst_v = max(worst_v, abs(res.values[e] - float(ext[e][7])) / max(1.0, float(np.abs(t.muA).max())))
        want = ref[e][2] if e != c["dup"] else t.point(x, lines=(lines[e, :R], lines[e, R], res.mu[e], muA))[2]
        worst_g = max(worst_g, float(np.max(np.abs(g[:, e] - want))) / kgr.unit(c))
    print(f"{case}: value uses {worst_v / ORACLE_ABS:.3g} of its bound, gradient {worst_g / BOUND:.3g}; segments {res.nseg.min()} .. {res.nseg.max()}")
    assert res.best_idx == int(np.argmax(res.values)) and res.best_val == res.values[res.best_idx]
    assert worst_v <= ORACLE_ABS and worst_g <= BOUND, (case, worst_v / ORACLE_ABS, worst_g / BOUND)
    m.close()


def test_laziness_invalidation_and_errors(bohip):
    from bohip import _lib

    c = kgr.case_data(kgr.CASES[0])
    m = model_of(bohip, c, lnoise=c["lnoise"], n=30, capacity=64)
    m.kg_set_points(c["A"].T)
    m.kg_grad(c["Xe"].T)
    m.append_(c["X"][30:].T, c["y"][30:])                               # the state is rebuilt from the kept points ...
    res, g = m.kg_grad(c["Xe"].T)
    assert m.kg_points_info()["rebuilds"] == 2
    fr, fg = m.kg_set_points(c["A"].T).kg_grad(c["Xe"].T)               # ... to the bytes that setting them anew computes
    assert (fr.values.tobytes(), fr.nseg.tobytes(), fg.tobytes()) == (res.values.tobytes(), res.nseg.tobytes(), g.tobytes())
    # (a fresh handle's one-shot factor differs from the appended one in its last bits, so its gradient does too: held to the bound)
    f = model_of(bohip, c, lnoise=c["lnoise"], capacity=64)
    fg = f.kg_set_points(c["A"].T).kg_grad(c["Xe"].T)[1]
    keep = np.arange(len(c["Xe"])) != c["dup"]
    assert float(np.max(np.abs(fg - g)[:, keep])) / kgr.unit(c) <= BOUND
    f.close()
    m.set_params_(ll=c["ll"] + 0.1)                                     # (a refit from scratch: a fresh handle walks the same steps)
    res, g = m.kg_grad(c["Xe"].T)
    assert m.kg_points_info()["rebuilds"] == 4
    f = model_of(bohip, dict(c, ll=c["ll"] + 0.1), lnoise=c["lnoise"], capacity=64)
    fr, fg = f.kg_set_points(c["A"].T).kg_grad(c["Xe"].T)
    assert (fr.values.tobytes(), fr.nseg.tobytes(), fg.tobytes()) == (res.values.tobytes(), res.nseg.tobytes(), g.tobytes())
    f.close()
    m.kg_set_points(None)
    with pytest.raises(_lib.BohipError) as e:
        m.kg_grad(c["Xe"].T)
    assert e.value.code == _lib.E_STATE
    with pytest.raises(_lib.BohipError, match=r"BOHIP_KG_RMAX \(8192\)") as e:
        m.kg_set_points(np.zeros((3, _lib.KG_RMAX), order="F"))
    assert e.value.code == _lib.E_UNSUPPORTED
    m.close()


def test_acquire_max_refine(bohip):
    """refine = 4 is no worse than refine = 0 under the same seed and stays in the box; refine = 0 is the call without the key."""
    c = kgr.case_data(("SEArd", 40, 2, 1, 1, -2.0))
    m = model_of(bohip, c, lnoise=c["lnoise"])
    lb, ub, a = np.zeros(2), np.ones(2), bohip.KnowledgeGradient()
    out = [bohip.acquire_max(a, m, lb, ub, dict(restarts=2, maxeval=64, **kw), rng=np.random.default_rng(3))
           for kw in ({}, {"refine": 0}, {"refine": 4})]
    assert out[0][0] == out[1][0] and out[0][1].tobytes() == out[1][1].tobytes()
    f, x = out[2]
    print(f"grid maximum {out[0][0]:.6g}, refined {f:.6g}")
    assert f >= out[0][0] and np.all((x >= lb) & (x <= ub))
    m.close()
