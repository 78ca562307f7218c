"""Every feature at the documented limit where its host code switches plan: the sizes the NOTES.md sections listed as "NOT run on a
device".  One family per section; the helpers, references and bounds are those of the families' own test files, used unchanged at the
new shapes (DESIGN.md 6h, 6l, 6m, 6n, 6o, 6p each name the limit tested here).

  A  knowledge gradient      the LDS plan across 64 KiB (R = 4080 ... 8192), bohip_gp_kg at R = 4100, a jittered model
  B  max-value entropy       three and nine slices of the sum S, the second turn of the bracket's stride, R = BOHIP_MES_RMAX, the
                             last block of the final reduction, joint mode after a jitter retry
  C  constrained scores      C = 6, 15, 16 against 50 digits; 16 distinct handles; the objective's handle as a constraint; several
                             K*' chunks inside score_con
  D  marginalised            H = 1024: chunk widths 2720 (value) and 1360 (gradient), four chunks each
  E  sample paths            eval_grad over three chunks of 4096 points

Every test prints its worst share of its bound (profiles/limits_tests.txt holds the output of a run on an MI355X).  A reference is
computed once per case on the CPU and never written to."""
import functools
import math

import numpy as np
import pytest

import con_reference as cr
import ens_grad_reference as eg
import ens_reference as er
import mes_reference as mr
import test_con_gpu as tc
import test_ens_grad_gpu as tg
import test_kg_gpu as tk
import test_mes_gpu as tm
import test_path_gpu as tp
from conftest import synth
from matern_reference import KERNELS, first_argmax
from test_ens_gpu import check_rows, close
from test_fit_gpu import model_of, settings
from test_parity_gpu import bohip  # noqa: F401  (fixture)
from test_qei_gpu import empty_model

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


# ==== A. knowledge gradient ==========================================================================================================
def kg_lds_bytes(R):
    """csrc/kernels_kg.hip: a and the point's b as pairs, R rounded up to even, and 256 bytes of reduction scratch."""
    return 16 * (R + (R & 1)) + 256


def tail_lines(a, B):
    """The lines permuted so that row 0's steepest line sits at index R - 1 and its start line (the smallest slope) at R - 2."""
    R = a.size
    b = B[0]
    top, start = int(np.argmax(b)), int(np.argmin(b))
    order = [j for j in range(R) if j not in (top, start)] + [start, top]
    a, B = a[order].copy(), np.ascontiguousarray(B[:, order])
    assert int(np.argmax(B[0])) == R - 1 and int(np.argmin(B[0])) == R - 2
    return a, B


@functools.lru_cache(maxsize=None)
def parabola_twin(R):
    a, B = tk.lines_of("parabola", R, 3, 0)
    return tk.twin_of(a, B)


@pytest.mark.parametrize("R", [4080, 4081, 4097, 8191, 8192])
def test_kg_lines_at_the_edges_of_the_lds_plan(bohip, R):
    """kg_lds_bytes(4080) = 65536 is the last size an unconfigured kernel may ask for; from 4081 on the launch depends on the opt-in of
    one_time_kernel_setup.  An odd R leaves rows 1, 3, ... of B on an 8-byte boundary only (the other load branch of k_kg)."""
    assert kg_lds_bytes(4080) == 65536 < kg_lds_bytes(4081) and kg_lds_bytes(8192) == 131328
    m = empty_model(bohip)
    worst = 0.0
    for E in (1, 3):
        for kind in ("normal", "quarter") + (("parabola",) if R >= 8191 else ()):
            a, B = tk.lines_of(kind, R, E, 100 * R + E)
            if kind == "normal":
                a, B = tail_lines(a, B)                                     # the tail of LDS decides row 0's result
            kg, nseg = m.kg_lines(a, B)
            if kind == "parabola":
                tkg, tseg = (v[:E] for v in parabola_twin(R))               # (row e of E = 1 is row e of E = 3)
                assert np.all(nseg == R - 1)
            else:
                tkg, tseg = tk.twin_of(a, B)
            worst = max(worst, tk.check_against_twin(kg, nseg, tkg, tseg, f"{kind} R = {R} E = {E}"))
            if kind == "normal":
                assert nseg[0] >= 1 and tkg[0] > 0.0
    print(f"  kg_lines R = {R} ({kg_lds_bytes(R)} bytes of LDS): worst share of TWIN_REL {worst / tk.TWIN_REL:.3f}")
    m.close()


def test_gp_kg_above_64_kib(bohip):
    """bohip_gp_kg at R = 4100 (65 856 bytes of LDS), E = 4: the twin on the device's own posterior, and the first four values of an
    E = 64 call, bit for bit."""
    from test_qei_gpu import LL, LSIG, LNOISE, BETA

    R, E = 4100, 4
    X, y, _ = synth(300, 4, 1, seed=31)                                     # test_kg_gpu's model
    xs = np.asfortranarray(synth(1, 4, R, seed=4100)[2].T)
    m = bohip.ElasticGPE(4, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(LL, LSIG), logNoise=LNOISE, capacity=len(y))
    m.append_(X.T, y)
    mu, cov = m.predict_cov(xs)
    res = m.kg(xs, E)
    assert res.values.shape == (E,) and res.mu.tobytes() == mu.tobytes()
    B = np.stack([cov[e] / math.sqrt(cov[e, e] + tk.NU) for e in range(E)])
    tkg, tseg = tk.twin_of(mu, B)
    rel = tk.check_against_twin(res.values, res.nseg, tkg, tseg, f"SEArd R = {R} E = {E}")
    assert np.all(tkg > 0.0) and np.all(tseg >= 1)
    assert res.best_idx == int(np.argmax(tkg)) and res.best_val == res.values[res.best_idx]
    more = m.kg(xs, 64)
    assert more.values[:E].tobytes() == res.values.tobytes() and more.nseg[:E].tolist() == res.nseg.tolist()
    print(f"  gp_kg R = {R}: worst share of TWIN_REL {rel / tk.TWIN_REL:.3f}; segments {res.nseg.tolist()}")
    m.close()


KG_JITTER_SEED = 3                                                          # the candidates' seed (see the test)


def test_kg_on_a_jittered_model(bohip, orc):
    """nu = e^(2 logNoise) + eps + J: the jitter the refit added is on the diagonal of cK, so it is part of the noise of the fantasy
    observation.  test_hardening_gpu's singular model; J from the oracle's twin of the escalation."""
    from bohip import _lib
    from oracle.oracle import fit_with_jitter

    rng = np.random.default_rng(11)
    pos = rng.random((60, 2)) * 10 - 5
    X = np.repeat(pos, 5, axis=0)
    y = -(((X - 1) ** 2).sum(1) + rng.standard_normal(len(X)))
    ll, lsig, lnoise = np.zeros(2), 5.0, -25.0
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(ll, lsig), logNoise=lnoise, capacity=len(y) + 8)
    with pytest.raises(bohip.BohipError):
        m.append_(X.T, y)
    m.set_jitter(1e-8, 10)
    m.fit_()
    _, _, tries, J = fit_with_jitter(orc, X, y, ll, lsig, lnoise, 0.0, 1e-8, 10)
    assert m.info(_lib.INFO_JITTER_STEPS) == tries >= 1 and J > 0.0
    R = 200
    xs = np.asfortranarray(np.random.default_rng(KG_JITTER_SEED).random((2, R)) * 10 - 5)
    mu, cov = m.predict_cov(xs)
    res = m.kg(xs)
    assert res.mu.tobytes() == mu.tobytes()
    nu0 = math.exp(2.0 * lnoise) + EPS
    nu = nu0 + J
    dd = np.diag(cov) + nu
    dead = ~(dd > 0.0)                                                      # Sigma_ee + nu <= 0 (or NaN): the point reports (0.0, 0)
    assert res.values[dead].tolist() == [0.0] * int(dead.sum()) and res.nseg[dead].tolist() == [0] * int(dead.sum())
    print(f"  jittered model: J = {J:.3e} after {tries} tries; {int(dead.sum())} of {R} points have Sigma_ee + nu <= 0")
    assert 4 * int(dead.sum()) <= R, "choose another KG_JITTER_SEED"
    live = np.flatnonzero(~dead)
    with np.errstate(all="ignore"):
        tkg, tseg = tk.twin_of(mu, np.stack([cov[e] / math.sqrt(cov[e, e] + nu) for e in live]))
        okj = np.flatnonzero(np.diag(cov)[live] + nu0 > 0.0)
        without, _ = tk.twin_of(mu, np.stack([cov[e] / math.sqrt(cov[e, e] + nu0) for e in live[okj]]))
    # non-vacuity: without J the twin moves by more than 100 x the tolerance somewhere, so a nu that lacks J cannot pass
    pos_ = tkg[okj] > 0
    moved = float(np.max(np.abs(without[pos_] - tkg[okj][pos_]) / tkg[okj][pos_]))
    print(f"  jittered model: the twin without J differs by {moved:.3e} relative (100 x TWIN_REL = {100 * tk.TWIN_REL:.3e})")
    assert moved > 100 * tk.TWIN_REL
    rel = tk.check_against_twin(res.values[live], res.nseg[live], tkg, tseg, f"jittered SEArd R = E = {R}")
    print(f"  jittered model: worst share of TWIN_REL {rel / tk.TWIN_REL:.3f}")
    m.close()


# ==== B. max-value entropy search ====================================================================================================
MES_SLICE = 8192


def mes_slices(R):
    return 1 if R <= MES_SLICE else -(-R // MES_SLICE)


def gumbel_case(kind, R):
    """test_mes_gpu.candidates, and at R = 65537 two crafted last candidates: index 65536 is past the first turn of the bracket's
    stride (256 workgroups of 256 threads)."""
    mu, var = tm.candidates(kind, R, 40 * R + len(kind))
    if R == 65537 and kind == "random":                                     # the candidate that sets hi0 = max mu + 5 sigma
        hi = float(np.max(mu + 5.0 * np.sqrt(var)))
        mu[-1], var[-1] = hi - 4.0, 1.0                                     # mu + 5 sigma = hi + 1
        assert int(np.argmax(mu + 5.0 * np.sqrt(var))) == R - 1
    if R == 65537 and kind == "some_flat":                                  # the largest mu, with sigma^2 = 0: no root lies below it
        mu[-1], var[-1] = float(np.max(mu)) + 2.25, 0.0                     # (above y25 of the others: it pins the lowest quantile)
        assert int(np.argmax(mu)) == R - 1
    return mu, var


@pytest.mark.parametrize("kind", ["random", "some_flat", "offset"])
@pytest.mark.parametrize("R", [16385, 65537])
def test_gumbel_over_many_slices(bohip, R, kind):
    """R = 16385: three slices of per = 5462 candidates, the last one ragged.  R = 65537: nine slices, and the bracket's 256
    workgroups take a second turn of their stride for the last candidate."""
    assert mes_slices(16385) == 3 and -(-16385 // 3) == 5462 and mes_slices(65537) == 9 and (65537 + 255) // 256 > 256
    m = empty_model(bohip)
    K = 16
    mu, var = gumbel_case(kind, R)
    q, mv = m.mes_gumbel(mu, var, samples=K, seed=11)
    tm.check_gumbel(q, mv, mu, var, K, 11, -math.inf, f"{kind} R = {R}")
    q2, mv2 = m.mes_gumbel(mu, var, samples=K, seed=11)                      # two calls, identical bits
    assert q2.tobytes() == q.tobytes() and mv2.tobytes() == mv.tobytes()
    if R == 65537 and kind == "some_flat":
        lo0, hi0 = mr.bracket(mu, var)                                      # S(y) = -Inf below the flat candidate at the last index:
        width = 2.0 * (hi0 - lo0) * 16.0 ** -mr.PASSES                       # y25 is that candidate's mu, up to the final bracket
        assert abs(q[0] - mu[-1]) <= width and q[1] >= mu[-1] - width
        fmu = mu.copy()                                                     # every sigma^2 = 0 and the maximum at the last index: exact, so
        fmu[-1] = float(np.max(mu)) + 1.0                                   # a bracket that misses index 65536 cannot pass
        q, mv = m.mes_gumbel(fmu, np.zeros(R), samples=K, seed=11)
        assert q.tolist() == [fmu[-1]] * 3 and mv.tolist() == [fmu[-1]] * K
    m.close()


def sparse_rmax():
    """R = BOHIP_MES_RMAX with 4096 live candidates, one per 128 indices at a varying offset: each of the 64 slices holds exactly 64 of
    them, the last one at index R - 1.  The others are not finite: NaN mu, +Inf sigma^2, negative sigma^2 in turn."""
    R = mr.RMAX
    rng = np.random.default_rng(524288)
    mu, var = np.zeros(R), np.ones(R)
    j = np.arange(R)
    mu[j % 3 == 0] = math.nan
    var[j % 3 == 1] = math.inf
    var[j % 3 == 2] = -1.0
    off = rng.integers(0, 128, 4096)
    off[-1] = 127
    live = np.arange(4096) * 128 + off
    mu[live], var[live] = rng.standard_normal(4096), rng.uniform(0.01, 2.0, 4096)
    return mu, var, live


def test_gumbel_at_rmax(bohip):
    R = mr.RMAX
    assert R == 524288 and mes_slices(R) == 64
    mu, var, live = sparse_rmax()
    per = -(-R // mes_slices(R))
    counts = np.bincount(live // per, minlength=64)
    assert counts.tolist() == [64] * 64 and live[-1] == R - 1               # non-vacuity: live candidates in every slice
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(mu) & np.isfinite(var) & (var >= 0.0)
    assert np.array_equal(np.flatnonzero(fin), live)
    m = empty_model(bohip)
    K = 16
    q, mv = m.mes_gumbel(mu, var, samples=K, seed=7)
    tm.check_gumbel(q, mv, mu[live], var[live], K, 7, -math.inf, f"4096 live of R = {R}")
    q2, mv2 = m.mes_gumbel(mu[live], var[live], samples=K, seed=7)
    qb = mr.quantile_bounds(mu[live], var[live], q2)
    print(f"  4096 live of R = {R}: |whole - live alone| / (2 x bound) = {np.max(np.abs(q - q2) / (2.0 * qb)):.3f}")
    assert np.all(np.abs(q - q2) <= 2.0 * qb)                               # (both within the bound of the root)
    # flat: every sigma^2 = 0 and the maximum of mu at the last index -- exact
    fmu = np.random.default_rng(1).standard_normal(R)
    fmu[-1] = float(fmu.max()) + 0.25
    q, mv = m.mes_gumbel(fmu, np.zeros(R), samples=K, seed=7)
    assert tm.check_gumbel(q, mv, fmu, np.zeros(R), K, 7, -math.inf, f"flat R = {R}") == (0.0, 0.0)
    assert q.tolist() == [fmu[-1]] * 3 and mv.tolist() == [fmu[-1]] * K
    m.close()


def test_values_at_rmax(bohip):
    """bohip_mes_values at R = 524288: 2048 blocks, and their records into k_argmax_final."""
    R, K = mr.RMAX, 2
    mu, s2, mv = tm.sweep(R, K)
    m = empty_model(bohip)
    val, bv, bi = m.mes_values(mu, s2, mv)
    h = R // 2
    a, b = m.mes_values(mu[:h], s2[:h], mv)[0], m.mes_values(mu[h:], s2[h:], mv)[0]
    assert np.concatenate([a, b]).tobytes() == val.tobytes()                # a value depends on its candidate alone
    assert (bv, bi) == mr.record(val)
    sub = np.r_[0:300, h - 150:h + 150, R - 300:R]
    err = tm.rel_err(val[sub], mr.values(mu[sub], s2[sub], mv)[0])
    print(f"  mes_values R = {R}: worst relative error against the twin on 900 candidates {err:.3e}")
    assert err <= tm.REL
    late = mu.copy()
    for keep in (300, 256):                                                 # the last 300 candidates lie in blocks 2046 and 2047 of the
        late = mu.copy()                                                    # final reduction, the last 256 are block 2047
        late[:R - keep] = math.nan
        val2, bv2, bi2 = m.mes_values(late, s2, mv)
        assert np.isnan(val2[:R - keep]).all() and val2[R - keep:].tobytes() == val[R - keep:].tobytes()
        assert (bv2, bi2) == mr.record(val2) and bi2 >= R - keep
    assert bi2 // 256 == 2047
    m.close()


def test_joint_mode_after_a_jitter_retry(bohip, orc):
    """Duplicated candidate columns make Sigma exactly singular (test_joint_gpu's recipe): the first factorisation fails, the retry
    adds a jitter, and the max values are the row maxima of the draws made after it."""
    m, xs, *_ = tm.model_and_posterior(bohip, orc, "SEArd", 300, 8)
    xs = np.asfortranarray(np.concatenate([xs[:, :200], xs[:, :100]], axis=1))    # 100 exactly dependent columns of Sigma
    K = 8
    js = m.sample_joint(xs, S=K, seed=17, jitter=1e-12, max_tries=40)
    res = m.mes(xs, samples=K, mode="joint", seed=17, jitter_rel=1e-12, max_tries=40)
    print(f"  joint mode: {res.tries} failed factorisations, jitter {res.jitter:.3e}")
    assert res.tries >= 1 and res.jitter > 0.0 and (res.jitter, res.tries) == (js.jitter, js.tries)
    assert res.maxvals.tobytes() == js.samples.max(axis=1).tobytes()
    assert res.mu.tobytes() == js.mu.tobytes() and np.isnan(res.quantiles).all()
    tw = mr.values(res.mu, res.var, res.maxvals)[0]
    err = tm.rel_err(res.values, tw)
    print(f"  joint mode: worst |device - twin| / twin of the values {err:.3e}")
    assert err <= tm.REL and (res.best_val, res.best_idx) == mr.record(res.values)


# ==== E. sample paths ================================================================================================================
PATHS_GRAD_CHUNK = 4096


@pytest.mark.parametrize("S", [3, 64])                                      # row form, MFMA form
def test_path_gradients_over_three_chunks(bohip, S):
    """eval_grad stages PATHS_GRAD_CHUNK points at a time through one buffer.  R = 4096, 4097 and 2 x 4096 + 5, with a path_of that
    changes across every boundary: the bytes of the calls on [0, 4096), [4096, 8192) and the tail; 40 points straddling each
    boundary against the twin with test_path_gpu's bounds; and f against eval at those points on those paths."""
    kern, N, d, M, seed = "Mat52Ard", 129, 4, 256, 99
    ll = np.full(d, -0.4)
    X, y, _ = synth(N, d, 1, seed=17)
    m = tp.build(bohip, kern, X, y, ll)
    R = 2 * PATHS_GRAD_CHUNK + 5
    xs = np.random.default_rng(8).random((R, d))
    po = (np.arange(R) + np.arange(R) // PATHS_GRAD_CHUNK) % S              # every chunk has a pattern of its own
    assert po[4095] != po[4096] and po[8191] != po[8192] and not np.array_equal(po[:4096], po[4096:8192])
    worst = {}
    with m.draw_paths(S, M, seed) as p:
        f, g = p.eval_grad(xs.T, po)
        for lo, hi in ((0, 4096), (4096, 8192), (8192, R)):
            f1, g1 = p.eval_grad(xs[lo:hi].T, po[lo:hi])
            assert f1.tobytes() == f[lo:hi].tobytes(), (lo, hi)
            assert np.ascontiguousarray(g1).tobytes() == np.ascontiguousarray(g[:, lo:hi]).tobytes(), (lo, hi)
        for Rs in (4096, 4097):                                             # exactly one chunk; one chunk and a tail of one point
            f2, g2 = p.eval_grad(xs[:Rs].T, po[:Rs])
            assert f2.tobytes() == f[:Rs].tobytes() and np.ascontiguousarray(g2).tobytes() == np.ascontiguousarray(g[:, :Rs]).tobytes()
        sub = np.r_[4076:4116, 8172:R]                                      # 40 points across the first boundary, 25 across the second
        vals = p.eval(xs[sub].T)[0]
        tw = tp.device_twin(kern, X, y, ll, M, seed, p.coef(0)[0])
        for s in sorted(set(po[sub].tolist())):
            _, w, u = p.coef(s)
            k = sub[po[sub] == s]
            vb = tw.value_bound(xs[k], u, w)
            worst["values"] = max(worst.get("values", 0.0), float(np.max(np.abs(f[k] - tw.value(xs[k], u, w)) / vb)))
            worst["gradients"] = max(worst.get("gradients", 0.0),
                                     float(np.max(np.abs(g[:, k].T - tw.grad(xs[k], u, w)) / tw.grad_bound(xs[k], u, w))))
            ev = vals[s][po[sub] == s]                                      # eval's value of the same point on the same path: both are
            worst["f against eval"] = max(worst.get("f against eval", 0.0), float(np.max(np.abs(f[k] - ev) / (2.0 * vb))))   # within vb
    print(f"  eval_grad R = {R} S = {S}: worst fraction of each bound: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    m.close()


# ==== D. marginalised acquisition ====================================================================================================
ENS_H, ENS_KERN, ENS_N, ENS_D = 1024, "Mat12Ard", 17, 3
ENS_ROWS = (0, 511, 1023)


def ens_chunk(H, per_candidate):
    """csrc/bohip.hip: candidates per chunk, the H x Rc planes within 64 MiB, a multiple of the 16-candidate tile, at most 16384."""
    return max(16, min(16384, ((64 << 20) // (per_candidate * H)) // 16 * 16))


def count(m, label):
    return sum(1 for name, _ in m.timing(cap=4096) if name == label)


@functools.lru_cache(maxsize=None)
def ens_case(R, Rc, side):
    """(X, y, Xs, Theta, row models, sub): `sub` the `side` candidates on either side of every chunk boundary and the last 5."""
    X, y, Xs = synth(ENS_N, ENS_D, R, seed=4000 + R)
    Theta = settings(ENS_KERN, ENS_D, ENS_H, seed=1024)
    refs = [er.row_model(ENS_KERN, X, y, t) for t in Theta]
    sub = np.unique(np.concatenate([np.arange(max(b - side, 0), min(b + side, R)) for b in range(Rc, R, Rc)] + [np.arange(R - 5, R)]))
    for a in (X, y, Xs, Theta, sub):
        a.setflags(write=False)
    return X, y, Xs, Theta, refs, sub


class Rows:
    def __init__(self, res, cols):
        self.mu, self.var, self.each = res.mu[:, cols], res.var[:, cols], res.each[:, cols]


def test_ensemble_scores_with_1024_settings(bohip, monkeypatch):
    """H = 1024: Rc = 2720, a multiple of 16 and not of 256, so k_ens_reduce's blocks of 256 candidates start at offsets no smaller H
    produces; R = 3 x 2720 + 5 is four chunks."""
    H, N = ENS_H, ENS_N
    Rc = ens_chunk(H, 24)
    R = 3 * Rc + 5
    assert Rc == 2720 and Rc % 256 != 0
    X, y, Xs, Theta, refs, sub = ens_case(R, Rc, 24)
    p = [float(np.median(y))]
    m = model_of(bohip, ENS_KERN, X, y)
    m.enable_timing(True)
    full = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    assert full.route == "device" and np.all(full.pivot == 0)
    assert (count(m, "ens_factor"), count(m, "ens_score"), count(m, "ens_reduce")) == (1, 4, 5)
    # the twin: all 1024 row models on the candidates around the three boundaries and the last five
    mv = [r.predict(Xs[sub]) for r in refs]
    mu_r, var_r = np.array([a for a, _ in mv]), np.array([b for _, b in mv])
    each_r = np.array([er.from_moments("EI", p, mu_r[h], var_r[h]) for h in range(H)])
    tol = check_rows(Rows(full, sub), refs, mu_r, var_r, each_r, N, "H = 1024", rows=ENS_ROWS)
    piv0 = np.zeros(H, dtype=np.int64)
    close(full.scores[sub], er.average(each_r, None, piv0), tol.sum(axis=0) / H, "H = 1024 scores")
    assert (full.best_val, full.best_idx) == first_argmax(full.scores)
    for lo in range(0, R, Rc):                                              # a call on a chunk's slice alone gives the slice's bytes
        hi = min(lo + Rc, R)
        part = m.score_ensemble("EI", p, Xs[lo:hi].T, Theta, want_each=True, want_moments=True)
        for name in ("each", "mu", "var"):
            np.testing.assert_array_equal(getattr(part, name), getattr(full, name)[:, lo:hi], err_msg=f"{name} [{lo}, {hi})")
        np.testing.assert_array_equal(part.scores, full.scores[lo:hi], err_msg=f"scores [{lo}, {hi})")
    # the winner in the last chunk: every earlier candidate is a copy of the poorest point
    late = Xs.copy()
    late[:3 * Rc] = Xs[int(np.argmin(full.scores))]
    res = m.score_ensemble("EI", p, late.T, Theta)
    assert (res.best_val, res.best_idx) == first_argmax(res.scores) and res.best_idx >= 3 * Rc
    np.testing.assert_array_equal(res.scores[3 * Rc:], full.scores[3 * Rc:])
    # a failed row and unequal weights, two of them 0: k_ens_weights and the skip of a zero weight with H > 256
    bad = Theta.copy()
    bad[700, 0] = np.nan
    w = np.random.default_rng(5).uniform(0.1, 2.0, H)
    w[[5, 900]] = 0.0
    res = m.score_ensemble("EI", p, Xs.T, bad, weights=w)
    piv = np.zeros(H, dtype=np.int64)
    piv[700] = 1
    assert np.array_equal(res.pivot > 0, piv > 0)
    wt = np.where(piv == 0, w, 0.0)
    wt = wt / wt.sum()
    close(res.scores[sub], er.average(each_r, w, piv), (wt[:, None] * tol).sum(axis=0), "H = 1024, a failed row, unequal weights")
    assert (res.best_val, res.best_idx) == first_argmax(res.scores)
    # the workspace capped: the settings are factored and scored 50 at a time inside every chunk -- the same bytes
    M = -(-N // 16) * 16
    Hc = (1 << 20) // ((2 * M + 1) * (M + 8) * 8)
    assert Hc == 50
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")
    capped = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    assert (count(m, "ens_factor"), count(m, "ens_score")) == (4 * -(-H // Hc), 4 * -(-H // Hc))
    for name in ("scores", "each", "mu", "var", "pivot"):
        np.testing.assert_array_equal(getattr(capped, name), getattr(full, name), err_msg=name)
    assert (capped.best_val, capped.best_idx) == (full.best_val, full.best_idx)
    m.close()


def test_ensemble_gradient_with_1024_settings(bohip):
    """The gradient call's chunk: Rc = 1360 at H = 1024 and d = 3; R = 3 x 1360 + 5 is four chunks."""
    H, N, d = ENS_H, ENS_N, ENS_D
    Rc = ens_chunk(H, 8 * (3 + d))
    R = 3 * Rc + 5
    assert Rc == 1360 and Rc % 256 != 0
    X, y, Xs, Theta, refs, sub = ens_case(R, Rc, 24)
    p = [float(np.median(y))]
    m = model_of(bohip, ENS_KERN, X, y)
    m.enable_timing(True)
    cold = tg.raw_grad(bohip, m, "EI", p, Xs, Theta)
    assert cold["rc"] == 0 and np.all(cold["pivot"] == 0)
    assert (count(m, "ens_factor"), count(m, "ens_alpha"), count(m, "ens_grad")) == (1, 1, 4)
    warm = tg.raw_grad(bohip, m, "EI", p, Xs, Theta)                          # the factors of the call before are reused
    assert warm["rc"] == 0 and (count(m, "ens_factor"), count(m, "ens_alpha"), count(m, "ens_grad")) == (0, 0, 4)
    for name in ("scores", "grad", "each", "each_grad", "mu", "var", "pivot"):
        np.testing.assert_array_equal(warm[name], cold[name], err_msg=name)
    assert warm["best"] == cold["best"] == first_argmax(cold["scores"])
    val = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)   # the values are score_ensemble's, bit for bit
    for name in ("scores", "each", "mu", "var", "pivot"):
        np.testing.assert_array_equal(cold[name], getattr(val, name), err_msg=name)
    assert cold["best"] == (val.best_val, val.best_idx)
    for lo in range(0, R, Rc):
        hi = min(lo + Rc, R)
        part = tg.raw_grad(bohip, m, "EI", p, Xs[lo:hi], Theta)
        assert part["rc"] == 0
        np.testing.assert_array_equal(part["grad"], cold["grad"][lo:hi], err_msg=f"grad [{lo}, {hi})")
        np.testing.assert_array_equal(part["each_grad"], cold["each_grad"][:, lo:hi], err_msg=f"each_grad [{lo}, {hi})")
        np.testing.assert_array_equal(part["scores"], cold["scores"][lo:hi], err_msg=f"scores [{lo}, {hi})")
    # three settings on the 48 candidates around every boundary; the average of all 1024 on the 2 on either side and the last five
    for h in ENS_ROWS:
        _, g_r = eg.row_score_grad(refs[h], "EI", p, Xs[sub])
        close(cold["each_grad"][h][sub], g_r, tg.grad_tols(g_r[None])[0], f"H = 1024 each_grad[{h}]")
    near = np.array([j for j in sub if j >= R - 5 or (min(j % Rc, Rc - j % Rc) <= 2 and j >= Rc - 2)])
    assert all(b - 1 in near and b in near for b in range(Rc, R, Rc))
    g_all = np.array([eg.row_score_grad(r, "EI", p, Xs[near])[1] for r in refs])
    tol = tg.grad_tols(g_all)
    close(cold["grad"][near], tg.avg(g_all, None), tol.sum(axis=0) / H, f"H = 1024 grad on {near.size} candidates")
    close(cold["each_grad"][:, near], g_all, tol, "H = 1024 each_grad, every setting")
    m.close()


# ==== C. constrained scores ==========================================================================================================
@pytest.fixture(scope="module")
def anchor(bohip):
    m = bohip.ElasticGPE(2)                                                 # no observations: the device and the stream only
    yield m
    m.close()


@pytest.mark.parametrize("C_", [6, 15, 16])
@pytest.mark.parametrize("acq", cr.FORMS)
def test_con_values_with_many_constraints(bohip, anchor, acq, C_):
    """ConParams carries thr[16] and sense[16] by value, indexed at run time: C = 6, 15 and 16 against the 50-digit evaluator on
    con_reference.crafted_near's moments (every threshold its own, neighbouring senses opposite, the hard entries in every row).
    Bound: 16 x WORST_MANY, the twin's own error measured on this grid (tests/test_con_host.py)."""
    from test_con_host import live_share, many_ref

    R = 257
    thr, s, mu, var, fr, Lr, pmr, pvr = many_ref(acq, C_)
    if acq in cr.PRODUCT:                                                   # non-vacuity: not 0 against 0
        assert live_share(fr) >= 0.5
    f, L, pm, pv, bv, bi = anchor.con_values(acq, [0.3], thr, s, mu, var, want_grad=True)
    f2, L2, none_m, none_v, bv2, bi2 = anchor.con_values(acq, [0.3], thr, s, mu, var)
    assert none_m is None and none_v is None and f2.tobytes() == f.tobytes() and L2.tobytes() == L.tobytes() and (bv2, bi2) == (bv, bi)
    W = cr.WORST_MANY
    shares = {"value": cr.worst_share(f, fr, 16 * W["value"]), "dmu": cr.worst_share(pm, pmr, 16 * W["dmu"]),
              "dvar": cr.worst_share(pv, pvr, 16 * W["dvar"])}
    ok = np.isfinite(Lr)
    shares["logfeas"] = cr.worst_share(L[ok], Lr[ok], 16 * W["value"])
    print(f"{acq} C={C_} R={R}: worst share of 16 x WORST_MANY {shares}; {live_share(fr):.2f} of the scores are finite and not 0")
    assert max(shares.values()) <= 1.0, shares
    assert not np.any(np.isnan(pm[:, np.isfinite(f)])) and not np.any(np.isnan(pv[:, np.isfinite(f)]))
    assert (bv, bi) == cr.record(f)
    if bi >= 0:
        assert f[bi] == bv and not np.isnan(bv)
    tv, ti = cr.record(fr)
    assert ti == bi or abs(f[ti] - f[bi]) <= 32 * W["value"] * max(1.0, abs(tv))


def check_score_con(bohip, members, twins, acq, tau, thr, senses, Xs, tw, ts, tgb, what, halves=True):
    """The assertions of test_con_gpu.test_score_con_against_the_twin on one ConstrainedGPE call: members[0] / twins[0] the objective,
    the others the constraints in order (a handle may appear more than once, the objective's among them)."""
    R, d = Xs.shape
    cm = bohip.ConstrainedGPE(members[0], members[1:], thr, senses)
    val = cm.score(acq, [tau], Xs.T)
    grd = cm.score(acq, [tau], Xs.T, want_grad=True)
    for a, b in ((val.scores, grd.scores), (val.logfeas, grd.logfeas), (val.mu, grd.mu), (val.var, grd.var)):
        assert a.tobytes() == b.tobytes(), what                             # value call == gradient call, bit for bit
    assert (val.best_val, val.best_idx) == (grd.best_val, grd.best_idx) and val.grad is None and grd.grad.shape == (d, R)
    s_share = np.max(np.abs(val.scores - tw["scores"]) / ts)
    smooth = np.ones(R, dtype=bool)
    for m_, t_ in zip(range(len(twins)), [tau] + list(thr)):
        if m_ == 0 and acq == "Feasibility":
            continue
        with np.errstate(all="ignore"):
            smooth &= (tw["var"][m_] > 0) & (np.abs(tw["mu"][m_] - t_) / np.sqrt(tw["var"][m_]) < 6.0)
    g_share = np.max(np.abs(grd.grad.T - tw["grad"])[smooth] / tgb[smooth]) if smooth.any() else 0.0
    print(f"{what}: worst share of the bound: score {s_share:.3g}, gradient {g_share:.3g} on {int(smooth.sum())} smooth candidates")
    assert s_share <= 1.0 and g_share <= 1.0, what
    assert np.all(np.isfinite(grd.grad[:, np.isfinite(grd.scores)]))
    rows = slice(1, None) if acq == "Feasibility" else slice(None)
    for m_ in range(len(twins))[rows]:
        bm, bv = cr.moment_bounds(twins[m_], tw["mu"][m_], tw["var"][m_])
        assert np.all(np.abs(val.mu[m_] - tw["mu"][m_]) <= bm) and np.all(np.abs(val.var[m_] - tw["var"][m_]) <= bv), (what, m_)
    if acq == "Feasibility":
        assert np.all(np.isnan(val.mu[0])) and np.all(np.isnan(val.var[0]))
    assert tc.lead_ok(tw, ts), ("choose another trial for", what)          # the arg-max is the twin's, with no exemption
    assert val.best_idx == tw["best_idx"] and val.best_val == val.scores[val.best_idx]
    if halves:                                                              # two halves scored separately give the bytes of the whole
        h = R // 2
        a, b = cm.score(acq, [tau], Xs[:h].T, want_grad=True), cm.score(acq, [tau], Xs[h:].T, want_grad=True)
        assert np.concatenate([a.scores, b.scores]).tobytes() == grd.scores.tobytes()
        assert np.concatenate([a.grad, b.grad], axis=1).tobytes(order="F") == grd.grad.tobytes(order="F")
    return val, grd


def live_scores(tw):
    return float(np.mean(np.isfinite(tw["scores"]) & (tw["scores"] != 0.0)))


def tau_of(acq, y):
    """test_con_gpu.e2e_twin's rule: the median observation, and the maximum under PI (which saturates at the median)."""
    return float(np.max(y)) if acq == "PI" else float(np.median(y))


# -- 16 distinct handles ---------------------------------------------------------------------------------------------------------------
MANY_C = 16
MANY_THR = tuple((-1.0) ** c * (0.02 + 0.01 * c) for c in range(MANY_C))   # near every member's median (its y is centred there);
MANY_SENSES = tuple(1 if c % 2 == 0 else -1 for c in range(MANY_C))         # neighbours differ in threshold and in sense
# trials of the candidates' seed, chosen on the CPU from the twin alone so that its winner leads by > 4 x the two tolerances (lead_ok)
MANY_TRIAL = {}


@functools.lru_cache(maxsize=None)
def many_members():
    """The objective of test_con_gpu and 16 constraint members of their own: N = 5 ... 20, d = 4, the kernels in turn."""
    out = [tc.member_data()[0]]
    for c in range(MANY_C):
        kern = list(KERNELS)[c % len(KERNELS)]
        X, y, _ = synth(5 + c, tc.D_E2E, 1, seed=500 + c)
        y = y - float(np.median(y))
        out.append((kern, X, y, tc.twin_of(kern, X, y)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def many_twin(acq, R):
    data = many_members()
    t = MANY_TRIAL.get((acq, R), 0)
    Xs = np.random.default_rng(1600 + R + 10007 * t).random((R, tc.D_E2E))
    twins = [m[3] for m in data]
    tau = tau_of(acq, data[0][2])
    tw = cr.score_con(twins, acq, [tau], MANY_THR, MANY_SENSES, Xs)
    ts, tgb = cr.propagate(twins, acq, tw)
    for a in (Xs, ts, tgb):
        a.setflags(write=False)
    return Xs, twins, tau, tw, ts, tgb


@pytest.fixture(scope="module")
def many_models(bohip):
    ms = [model_of(bohip, kern, X, y) for kern, X, y, _ in many_members()]
    yield ms
    for m in ms:
        m.close()


@pytest.mark.parametrize("R", [17, 300])
@pytest.mark.parametrize("acq", cr.FORMS)
def test_score_con_over_sixteen_handles(bohip, many_models, acq, R):
    """C = 16 over 16 distinct handles: 17 streams joined by events, and thr[c], sense[c] of every c up to 15."""
    Xs, twins, tau, tw, ts, tgb = many_twin(acq, R)
    assert len({id(m) for m in many_models}) == MANY_C + 1
    if acq in cr.PRODUCT:
        assert live_scores(tw) >= 0.5                                       # non-vacuity: not 0 against 0
    check_score_con(bohip, many_models, twins, acq, tau, MANY_THR, MANY_SENSES, Xs, tw, ts, tgb, f"{acq} C=16 R={R}")


# -- the objective's handle among the constraints ----------------------------------------------------------------------------------------
OWN_TRIAL = {}


@functools.lru_cache(maxsize=None)
def own_twin(acq, where):
    """where = "first": the objective's handle is constraint 0 of 1; "third": constraint 2 of 3, after the two models of test_con_gpu."""
    data = tc.member_data()
    med = float(np.median(data[0][2]))
    which, thr, senses = ((0,), (med - 0.2,), (1,)) if where == "first" else ((1, 2, 0), (-0.3, 0.25, med + 0.3), (1, -1, -1))
    t = OWN_TRIAL.get((acq, where), 0)
    Xs = np.random.default_rng(1700 + len(which) + 10007 * t).random((300, tc.D_E2E))
    twins = [data[0][3]] + [data[w][3] for w in which]
    tau = tau_of(acq, data[0][2])
    tw = cr.score_con(twins, acq, [tau], thr, senses, Xs)
    ts, tgb = cr.propagate(twins, acq, tw)
    for a in (Xs, ts, tgb):
        a.setflags(write=False)
    return which, thr, senses, Xs, twins, tau, tw, ts, tgb


@pytest.fixture(scope="module")
def e2e_models(bohip):
    ms = [model_of(bohip, kern, X, y) for kern, X, y, _ in tc.member_data()]
    yield ms
    for m in ms:
        m.close()


@pytest.mark.parametrize("where", ["first", "third"])
@pytest.mark.parametrize("acq", cr.FORMS)
def test_score_con_with_the_objective_as_a_constraint(bohip, e2e_models, acq, where):
    """t_lo <= f: the objective's own handle serves a constraint, so bohip_gp_score_con computes its posterior a second time on its
    own stream, with no event to wait for."""
    which, thr, senses, Xs, twins, tau, tw, ts, tgb = own_twin(acq, where)
    if acq in cr.PRODUCT:
        assert live_scores(tw) >= 0.5
    members = [e2e_models[0]] + [e2e_models[w] for w in which]
    assert members[1 + which.index(0)] is members[0]
    val, _ = check_score_con(bohip, members, twins, acq, tau, thr, senses, Xs, tw, ts, tgb, f"{acq}, objective as the {where} constraint")
    if acq != "Feasibility":                                                # the same model, the same candidates: the same moments
        c = 1 + which.index(0)
        assert val.mu[c].tobytes() == val.mu[0].tobytes() and val.var[c].tobytes() == val.var[0].tobytes()


# -- several K*' chunks inside score_con -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_members():
    X, y, Xs = synth(200, 3, 70001, seed=17)                                # test_predict_grad_over_two_candidate_chunks' shape
    Xc, yc, _ = synth(900, 3, 1, seed=18)                                   # another N: another leading dimension, another chunk
    yc = yc - float(np.median(yc))
    for a in (X, y, Xs, Xc, yc):
        a.setflags(write=False)
    return X, y, Xs, Xc, yc, tc.twin_of("Mat52Ard", X, y), tc.twin_of("SEArd", Xc, yc)


@pytest.mark.parametrize("acq", ["EI", "LogEI"])
def test_score_con_over_several_candidate_chunks(bohip, acq):
    """R = 70001: two K*' chunks in the objective (N = 200) and three in the constraint (N = 900), inside ONE score_con call.  400
    candidates across each member's own first boundary and the last 300 against the twin; a call on a slice alone gives its bytes."""
    from bohip import _lib

    X, y, Xs, Xc, yc, tw_o, tw_c = chunk_members()
    R = len(Xs)
    obj, con = model_of(bohip, "Mat52Ard", X, y), model_of(bohip, "SEArd", Xc, yc)
    cm = bohip.ConstrainedGPE(obj, [con], [0.05], [1])
    tau = float(np.median(y))
    full = cm.score(acq, [tau], Xs.T, want_grad=True)
    ch_o, ch_c = obj.info(_lib.INFO_SCORE_CHUNK), con.info(_lib.INFO_SCORE_CHUNK)
    print(f"  {acq}: K*' chunks of {ch_o} (objective) and {ch_c} (constraint) candidates")
    assert 0 < ch_o < R and 0 < ch_c < R and ch_o != ch_c
    assert (full.best_val, full.best_idx) == cr.record(full.scores)
    twins = [tw_o, tw_c]
    for lo, hi, what in ((ch_o - 192, ch_o + 208, "the objective's boundary"), (ch_c - 192, ch_c + 208, "the constraint's boundary"),
                         (R - 300, R, "the tail")):
        tw = cr.score_con(twins, acq, [tau], [0.05], [1], Xs[lo:hi])
        ts, tgb = cr.propagate(twins, acq, tw)
        if acq in cr.PRODUCT:
            assert live_scores(tw) >= 0.5
        s_share = np.max(np.abs(full.scores[lo:hi] - tw["scores"]) / ts)
        with np.errstate(all="ignore"):
            smooth = np.all([(tw["var"][m_] > 0) & (np.abs(tw["mu"][m_] - t_) / np.sqrt(tw["var"][m_]) < 6.0)
                             for m_, t_ in ((0, tau), (1, 0.05))], axis=0)
        g_share = np.max(np.abs(full.grad[:, lo:hi].T - tw["grad"])[smooth] / tgb[smooth])
        print(f"  {acq}, {what}: worst share of the bound: score {s_share:.3g}, gradient {g_share:.3g} on {int(smooth.sum())} candidates")
        assert s_share <= 1.0 and g_share <= 1.0 and smooth.sum() >= 100, what
        for m_ in (0, 1):
            bm, bv = cr.moment_bounds(twins[m_], tw["mu"][m_], tw["var"][m_])
            assert np.all(np.abs(full.mu[m_, lo:hi] - tw["mu"][m_]) <= bm) and np.all(np.abs(full.var[m_, lo:hi] - tw["var"][m_]) <= bv)
        for m_ in (obj, con):                                               # a shard takes the summation schedule of the whole set only when
            m_.set_batch_hint(R)                                            # told its size: alone, 400 candidates at N = 900 go split-K
        alone = cm.score(acq, [tau], Xs[lo:hi].T, want_grad=True)
        for m_ in (obj, con):
            m_.set_batch_hint(0)
        for name in ("scores", "logfeas"):
            assert getattr(alone, name).tobytes() == getattr(full, name)[lo:hi].tobytes(), (what, name)
        for name in ("mu", "var"):
            assert getattr(alone, name).tobytes() == np.ascontiguousarray(getattr(full, name)[:, lo:hi]).tobytes(), (what, name)
        assert np.asfortranarray(alone.grad).tobytes(order="F") == np.asfortranarray(full.grad[:, lo:hi]).tobytes(order="F"), what
    cm.close()
