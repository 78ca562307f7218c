"""Writes tests/golden/logei_table.npz: LogEI and its partials at 80 digits (mpmath), rounded to double.
    python tests/golden/make_logei_golden.py
Columns mu, s2, tau, value, dmu, ds2 (and z, sigma: the grid point a row was made from, for the tests' grid lines).  The
reference is evaluated AT THE STORED DOUBLES mu, s2, tau -- not at the nominal z -- so a row is exact for its own inputs.
A result beyond the range of a double is stored as +-inf (d/ds2 ~ z^2 / (2 s2) overflows for z <= -1e147 at sigma = 1e-8).
z grid: 241 points on [-6, 6]; the branch switch -4 and its two neighbouring doubles; -10^k, k = 1..150; +10^k, k = -3..6;
each crossed with sigma in {1e-8, 1, 1e4}, tau = 0.  Then s2 = 0 rows with mu above and below tau."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 80


def to_double(v):
    if v == mp.inf or v > mp.mpf(2) ** 1024:
        return np.inf
    if v == -mp.inf or v < -(mp.mpf(2) ** 1024):
        return -np.inf
    return float(v)


def reference(mu, s2, tau):
    mu, s2, tau = mp.mpf(float(mu)), mp.mpf(float(s2)), mp.mpf(float(tau))
    if s2 == 0:
        if mu > tau:
            return mp.log(mu - tau), 1 / (mu - tau), mp.mpf(0)
        return -mp.inf, mp.mpf(0), mp.mpf(0)
    s = mp.sqrt(s2)
    z = (mu - tau) / s
    # the lower tail relative to phi, so that nothing underflows: Mills' ratio m = Phi / phi and den = h / phi = 1 + z m
    if z < -3:
        t = -z
        if t <= 100:                           # den ~ 1/t^2 cancels at most 1e4-fold here: 80 digits leave 76
            mills = mp.erfc(t / mp.sqrt(2)) / 2 * mp.exp(t * t / 2) * mp.sqrt(2 * mp.pi)
            den = 1 + z * mills
        else:                                  # the asymptotic series, whose smallest term is ~ exp(-t^2 / 2) < 1e-2000:
            mills, term = mp.mpf(0), 1 / t     # m = (1/t)(1 - 1/t^2 + 3/t^4 - 15/t^6 ...), den = 1/t^2 - 3/t^4 + 15/t^6 ...
            for k in range(200):
                mills += term
                term *= -(2 * k + 1) / (t * t)
                if abs(term) < mp.mpf(10) ** -90 * abs(mills):
                    break
            den, term = mp.mpf(0), 1 / (t * t)
            for k in range(1, 200):
                den += term
                term *= -(2 * k + 1) / (t * t)
                if abs(term) < mp.mpf(10) ** -90 * abs(den):
                    break
        logh = -z * z / 2 - mp.log(2 * mp.pi) / 2 + mp.log(den)
        Phi_h, phi_h = mills / den, 1 / den
    else:
        phi = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
        Phi = mp.erfc(-z / mp.sqrt(2)) / 2
        h = phi + z * Phi
        logh, Phi_h, phi_h = mp.log(h), Phi / h, phi / h
    return mp.log(s) + logh, Phi_h / s, phi_h / (2 * s2)


def main():
    zs = list(np.linspace(-6.0, 6.0, 241))
    zs += [np.nextafter(-4.0, -np.inf), -4.0, np.nextafter(-4.0, np.inf)]
    zs += [-(10.0 ** k) for k in range(1, 151)]
    zs += [10.0 ** k for k in range(-3, 7)]
    rows = []
    for sigma in (1e-8, 1.0, 1e4):
        for z in zs:
            rows.append((z * sigma, sigma * sigma, 0.0, z, sigma))
    for mu, tau in ((1.5, 0.25), (0.25, 1.5), (0.25, 0.25), (-3.0, -7.0), (1e-300, 0.0), (1e300, -1e300)):
        rows.append((mu, 0.0, tau, np.nan, 0.0))
    out = np.empty((len(rows), 8))
    for i, (mu, s2, tau, z, sigma) in enumerate(rows):
        v, a, b = reference(mu, s2, tau)
        out[i] = (mu, s2, tau, to_double(v), to_double(a), to_double(b), z, sigma)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "logei_table.npz")
    np.savez_compressed(path, mu=out[:, 0], s2=out[:, 1], tau=out[:, 2], value=out[:, 3], dmu=out[:, 4], ds2=out[:, 5],
                        z=out[:, 6], sigma=out[:, 7])
    print(path, out.shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
