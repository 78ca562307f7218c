"""NumPy twin of bohip_gp_score_ens (include/bohip_ens.h): one acquisition averaged over H hyper-parameter settings.

A helper of the ensemble tests, not a test module.  Per row of Theta = [logNoise, mean, ll..., lsigma] it is
MaternGP(kern, X, y, ll, lsig, lnoise, beta).predict / .score of tests/matern_reference.py (LogEI: tests/logei_reference.py on that
model's moments); a row with a non-finite entry, or whose Cholesky factorisation fails, is failed (pivot > 0, NaN rows).  The
weights are renormalised over the surviving rows and the weighted sum runs in ascending h from 0.0, a row of weight 0 left out; the
arg-max is first_argmax."""
import numpy as np

from logei_reference import logei
from matern_reference import MaternGP, acq_value, first_argmax


def row_model(kern, X, y, t):
    return MaternGP(kern, X, y, t[2:-1], t[-1], t[0], t[1])


def from_moments(acq, params, mu, var):
    """The acquisition of one setting from its moments (MaternGP.score's functors; LogEI: logei_reference)."""
    return np.asarray(logei(mu, var, params[0])[0] if acq == "LogEI" else acq_value(acq, params, mu, var), dtype=np.float64)


def row_values(kern, X, y, t, acq, params, Xs):
    """(mu, var, scores, model) of one setting."""
    ref = row_model(kern, X, y, t)
    mu, var = ref.predict(Xs)
    return mu, var, from_moments(acq, params, mu, var), ref


def average(each, weights, pivot):
    H, R = each.shape
    w = np.ones(H) if weights is None else np.asarray(weights, dtype=np.float64)
    total = 0.0
    for h in range(H):
        if pivot[h] == 0:
            total += w[h]
    scores = np.zeros(R)
    for h in range(H):
        wt = w[h] / total if pivot[h] == 0 else 0.0
        if wt != 0.0:
            scores = scores + wt * each[h]
    return scores


def score_ens(kern, X, y, Theta, acq, params, Xs, weights=None):
    """-> dict(scores, best_val, best_idx, pivot, each, mu, var, models): models[h] is the row's MaternGP, None for a failed row."""
    Theta = np.atleast_2d(np.asarray(Theta, dtype=np.float64))
    Xs = np.atleast_2d(Xs)
    H, R = Theta.shape[0], Xs.shape[0]
    each, mu, var = (np.full((H, R), np.nan) for _ in range(3))
    pivot = np.zeros(H, dtype=np.int64)
    models = [None] * H
    for h, t in enumerate(Theta):
        if not np.all(np.isfinite(t)):
            pivot[h] = 1
            continue
        try:
            mu[h], var[h], each[h], models[h] = row_values(kern, X, y, t, acq, params, Xs)
        except np.linalg.LinAlgError:
            pivot[h] = 1          # (LAPACK does not name the pivot the way the device does: tests with such rows compare pivot > 0)
    scores = average(each, weights, pivot)
    bv, bi = first_argmax(scores)
    return dict(scores=scores, best_val=bv, best_idx=bi, pivot=pivot, each=each, mu=mu, var=var, models=models)
