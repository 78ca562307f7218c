"""NumPy twin of bohip_gp_score_ens_grad (include/bohip_ens_grad.h): the gradient of one acquisition averaged over H
hyper-parameter settings.

A helper of the ensemble-gradient tests, not a test module.  Per finite row of Theta it is MaternGP.score_grad of
tests/matern_reference.py (LogEI: the partials of tests/logei_reference.py on that model's posterior_grad, with the library's rule
for a clamped variance); a failed row has NaN rows.  The average is ens_reference.average's rule applied to each gradient component."""
import numpy as np

import ens_reference as er
from logei_reference import logei
from matern_reference import first_argmax


def row_score_grad(ref, acq, params, Xs):
    """(scores[R], grad[R, d]) of one setting's model."""
    Xs = np.atleast_2d(Xs)
    if acq != "LogEI":
        return ref.score_grad(acq, list(params), Xs)
    sc, g = np.empty(len(Xs)), np.empty(Xs.shape)
    for i, x in enumerate(Xs):
        mu, s2, dmu, ds2 = ref.posterior_grad(x)
        v, a, b = logei(np.array([mu]), np.array([s2]), params[0])
        sc[i] = v[0]
        g[i] = a[0] * dmu + (b[0] * ds2 if s2 > 0 else 0.0)
    return sc, g


def score_ens_grad(kern, X, y, Theta, acq, params, Xs, weights=None):
    """-> dict(scores[R], grad[R, d], each[H, R], each_grad[H, R, d], pivot, best_val, best_idx, models)."""
    Theta = np.atleast_2d(np.asarray(Theta, dtype=np.float64))
    Xs = np.atleast_2d(Xs)
    H, (R, d) = Theta.shape[0], Xs.shape
    each, eg = np.full((H, R), np.nan), np.full((H, R, d), np.nan)
    pivot = np.zeros(H, dtype=np.int64)
    models = [None] * H
    for h, t in enumerate(Theta):
        if not np.all(np.isfinite(t)):
            pivot[h] = 1
            continue
        try:
            models[h] = er.row_model(kern, X, y, t)
            each[h], eg[h] = row_score_grad(models[h], acq, params, Xs)
        except np.linalg.LinAlgError:
            pivot[h], models[h] = 1, None
    scores = er.average(each, weights, pivot)
    grad = er.average(eg.reshape(H, R * d), weights, pivot).reshape(R, d)
    bv, bi = first_argmax(scores)
    return dict(scores=scores, grad=grad, each=each, each_grad=eg, pivot=pivot, best_val=bv, best_idx=bi, models=models)
