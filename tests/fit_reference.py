"""What tests/test_fit_host.py and tests/test_fit_gpu.py share: the multimodal marginal likelihood of the multi-start MAP fit, its
objective on the NumPy twin (tests/matern_reference.py) and SciPy's L-BFGS-B from the same starts, computed once per process."""
import functools

import numpy as np
from scipy.optimize import minimize

from matern_reference import MaternGP

KERN = "SEIso"
LO = np.array([-4.0, -2.0, -4.0, -3.0])          # [logNoise, mean, ll, lsigma]
HI = np.array([2.0, 2.0, 3.0, 3.0])
X0 = np.array([0.0, 0.0, 1.5, 0.0])
RESTARTS, SEED = 8, 11


@functools.lru_cache(maxsize=None)
def problem():
    """12 noisy samples of sin(14 x): a "long length-scale, all noise" basin beside a "short length-scale, little noise" one."""
    rng = np.random.default_rng(7)
    X = rng.uniform(0, 1, (12, 1))
    y = np.sin(14 * X[:, 0]) + 0.5 * rng.standard_normal(12)
    return X, y


def twin_mll_grad(theta, kern=KERN, data=None):
    """(mll, gradient) of one row [logNoise, mean, ll..., lsigma] on the twin; (-inf, 0) where the factorisation fails."""
    X, y = data if data is not None else problem()
    theta = np.asarray(theta, float)
    try:
        m, dn, dm, dk = MaternGP(kern, X, y, theta[2:-1], theta[-1], theta[0], theta[1]).mll_grad()
    except np.linalg.LinAlgError:
        return -np.inf, np.zeros(theta.size)
    return m, np.concatenate([[dn, dm], np.ravel(dk)])


def twin_fg_batch(Xc):
    """fg_batch of bopt._multistart_map on the twin: columns are settings."""
    out = [twin_mll_grad(Xc[:, r]) for r in range(Xc.shape[1])]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out], axis=1)


def starts():
    from bohip.utils import latin_hypercube_sampling

    return np.concatenate([X0.reshape(-1, 1), latin_hypercube_sampling(LO, HI, RESTARTS - 1, np.random.default_rng(SEED))], axis=1)


@functools.lru_cache(maxsize=None)
def scipy_best():
    """The end values of SciPy's L-BFGS-B on the twin from the same 8 starts (the reference's optimiser, run per start)."""
    ends = []
    for s in starts().T:
        def neg(x):
            m, g = twin_mll_grad(x)
            return (-m, -g) if np.isfinite(m) else (1e300, np.zeros_like(x))
        ends.append(-minimize(neg, s, jac=True, method="L-BFGS-B", bounds=list(zip(LO, HI)), options=dict(maxfun=500)).fun)
    return np.array(ends)
