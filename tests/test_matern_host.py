"""Matérn 1/2, 3/2 and the iso Matérn kernels (ids 3-7 of include/bohip.h): what can be checked without a GPU.

The ids must be accepted at the C ABI, agree between the header, the Python mirror and the Julia binding, and the NumPy model
of tests/matern_reference.py (the yardstick of the GPU tests) is anchored to scikit-learn and to its own finite differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from matern_reference import KERNELS, NEW_KERNELS, MaternGP, cov, mll_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_kernel_classes_import():
    import bohip

    for name in NEW_KERNELS:
        k = getattr(bohip, name)(np.zeros(1), 0.0)
        assert k.kern == name and name in bohip.__all__
        assert k.iso == name.endswith("Iso")
    assert bohip.SEIso.iso and not bohip.SEArd.iso and not bohip.Mat52Ard.iso


def test_create_accepts_ids_3_to_7():
    from bohip import _lib

    lib = _lib.load()
    ndev = lib.bohip_device_count()
    for kid in range(3, 8):
        h = C.c_void_p()
        rc = lib.bohip_gp_create(2, 10, kid, 0, C.byref(h))
        assert rc == (_lib.OK if ndev > 0 else _lib.E_NODEVICE), (kid, rc, lib.bohip_last_error())
        if rc == _lib.OK:
            lib.bohip_gp_destroy(h)
    for kid in (8, 9, -1):
        h = C.c_void_p()
        assert lib.bohip_gp_create(2, 10, kid, 0, C.byref(h)) == _lib.E_ARG


def test_kernel_ids_agree_everywhere():
    from bohip import _lib

    hdr = open(os.path.join(ROOT, "include", "bohip.h")).read()
    h_ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BOHIP_KERN_(\w+) (\d+)", hdr)}
    jl = open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    body = re.search(r"const KERN = Dict\((.*?)\)\n", jl, re.S).group(1)
    jl_ids = {m.group(1): int(m.group(2)) for m in re.finditer(r":(\w+) => (\d+)", body)}
    assert set(_lib.KERN) == set(KERNELS) == set(jl_ids)
    assert jl_ids == _lib.KERN
    assert {k.upper(): v for k, v in _lib.KERN.items()} == h_ids
    iso = re.search(r"_isokernel\(k::Symbol\) = k in \(([^)]*)\)", jl).group(1)
    assert sorted(s.strip().lstrip(":") for s in iso.split(",")) == sorted(k for k in KERNELS if k.endswith("Iso"))


@pytest.mark.parametrize("nu,kern", [(0.5, "Mat12Ard"), (1.5, "Mat32Ard"), (2.5, "Mat52Ard")])
def test_cov_matches_sklearn(nu, kern):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern

    rng = np.random.default_rng(1)
    X, Y = rng.random((40, 3)), rng.random((30, 3))
    ll, ls = np.log([0.3, 0.7, 1.4]), 0.4
    ref = (ConstantKernel(np.exp(2 * ls)) * Matern(length_scale=np.exp(ll), nu=nu))(X, Y)
    got = cov(kern, X, Y, ll, ls)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)
    iso = cov(kern.replace("Ard", "Iso"), X, Y, [ll[1]], ls)
    ref_iso = (ConstantKernel(np.exp(2 * ls)) * Matern(length_scale=np.exp(ll[1]), nu=nu))(X, Y)
    np.testing.assert_allclose(iso, ref_iso, rtol=1e-13, atol=0)


def test_mat52_equals_oracle():
    from oracle.oracle import np_cov

    rng = np.random.default_rng(2)
    X, Y = rng.random((25, 4)), rng.random((20, 4))
    ll = np.log([0.3, 0.5, 0.9, 1.1])
    np.testing.assert_array_equal(cov("Mat52Ard", X, Y, ll, 0.2), np_cov("Mat52Ard", X, Y, ll, 0.2))
    np.testing.assert_array_equal(cov("SEArd", X, Y, ll, 0.2), np_cov("SEArd", X, Y, ll, 0.2))


def _problem(kern, N=30, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    ll = np.log(np.linspace(0.3, 0.6, d)) if not kern.endswith("Iso") else np.array([np.log(0.4)])
    return X, y, ll, 0.3, -2.0, 0.1


@pytest.mark.parametrize("kern", sorted(KERNELS))
def test_mll_grad_matches_central_differences(kern):
    X, y, ll, ls, ln, b = _problem(kern)
    m, dn, dm, dk = MaternGP(kern, X, y, ll, ls, ln, b).mll_grad()
    theta = np.concatenate([[ln, b], ll, [ls]])

    def f(t):
        return mll_of(kern, X, y, t[2:-1], t[-1], t[0], t[1])

    h = 1e-6
    fd = np.array([(f(theta + h * e) - f(theta - h * e)) / (2 * h) for e in np.eye(theta.size)])
    g = np.concatenate([[dn, dm], dk])
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-7 * np.abs(fd).max())


@pytest.mark.parametrize("kern", sorted(KERNELS))
@pytest.mark.parametrize("acq,params", [("EI", [1.0]), ("PI", [1.0]), ("UCB", [1.5]), ("MI", [1.2, 0.3]), ("MaxMean", [0.0])])
def test_score_grad_matches_central_differences(kern, acq, params):
    X, y, ll, ls, ln, b = _problem(kern)
    gp = MaternGP(kern, X, y, ll, ls, ln, b)
    Xs = np.random.default_rng(5).random((4, X.shape[1]))
    _, g = gp.score_grad(acq, params, Xs)
    h = 1e-6
    for i, x in enumerate(Xs):
        fd = np.array([(gp.score(acq, params, x + h * e)[0] - gp.score(acq, params, x - h * e)[0]) / (2 * h)
                       for e in np.eye(x.size)])
        np.testing.assert_allclose(g[i], fd, rtol=1e-5, atol=1e-7 * max(np.abs(fd).max(), 1e-12))


@pytest.mark.parametrize("kern", ["Mat12Ard", "Mat12Iso"])
def test_mat12_gradient_at_an_observation_follows_the_rule(kern):
    """On an observation the coincident term's k is symmetric in the step, so central differences see exactly the
    minimum-norm subgradient (that term contributes 0); they agree with the rule to O(h), removed by one Richardson step."""
    X, y, ll, ls, ln, b = _problem(kern)
    gp = MaternGP(kern, X, y, ll, ls, ln, b)
    x = X[7].copy()
    mu, s2, dmu, ds2 = gp.posterior_grad(x)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(ds2))
    diff = x[None, :] - X
    r = (diff * diff) @ gp.il2
    assert r[7] == 0.0
    _, g = gp.score_grad("UCB", [1.5], x[None, :])
    assert np.all(np.isfinite(g))

    def cd(h):   # central differences of (mu, sigma^2)
        out = []
        for e in np.eye(x.size):
            (mp, vp), (mm, vm) = gp.predict(x + h * e), gp.predict(x - h * e)
            out.append([(mp[0] - mm[0]) / (2 * h), (vp[0] - vm[0]) / (2 * h)])
        return np.array(out).T

    fd = 2 * cd(5e-6) - cd(1e-5)
    np.testing.assert_allclose(dmu, fd[0], rtol=1e-5, atol=1e-6 * np.abs(fd[0]).max())
    np.testing.assert_allclose(ds2, fd[1], rtol=1e-4, atol=1e-4 * np.abs(fd[1]).max())
    # the dmll diagonal (r = 0 on every i == j) stays finite
    assert np.all(np.isfinite(gp.mll_grad()[3]))
