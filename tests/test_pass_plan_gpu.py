"""The launch structure of the posterior pass (csrc/bohip.hip: PassPlan, choose_route, chunk_pass), pinned.

Every feature sits on one pipeline -- K*' chunk, k_trigemm_sq (optionally storing V'), optionally U' = V'W, a per-chunk finish -- and
the host code holds that loop once.  What must never move when the host layer is rearranged:

  1  the route and the launches of a call: the exact ordered stage labels of m.timing() for every route (small pass, split-K, whole-K
     in one chunk, whole-K in two chunks) and every caller of the loop;
  2  the numbers: every output equals, bit for bit, what the same call gives as the FIRST call of a fresh handle built from the same
     data -- the handle under test has had another call before it;
  3  no call relies on what the previous one left on the handle: one handle runs calls of every route back to back and each still
     gives the fresh handle's bits, under each of the three ascent drivers (BOHIP_ASC_LOCKSTEP unset, 1, 2; one child process each).

Shapes (d = 2): N = 130 at capacity 130 has two row tiles (no split-K, small pass up to 256 candidates) and ld = 272, so the chunk cap
is 65536 candidates and R = 66561 (R512 = 67072) runs as two chunks of round_up(33536, 512) = 33792.  N = 900 has eight row tiles, so
R = 300 (5 candidate tiles x 8 < 512 jobs) takes the split-K route.  The interleaving case needs all routes on ONE handle, hence one
N per handle: the N = 900 handle has split-K and runs R = 66561 as three chunks of 22528 (ld = 1040, cap 32256); the N = 130 handle has
the two-chunk pass and the one-launch ascent (N <= 256)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, synth

pytestmark = pytest.mark.gpu

D = 2
TAU = 1.5
R2 = 66561          # two chunks at N = 130
CHUNK2 = 33792
SMALL = ["small_V"]
SMALL_G = ["small_V+U"]
WHOLE = ["kstar", "trigemm_sq"]
WHOLE_G = ["kstar", "trigemm_sq+V", "gemm_U", "score+grad"]
POST_G = ["kstar", "trigemm_sq+V", "gemm_U", "con_post"]
COV = ["kstar", "trigemm_sq+V", "gemm_VV", "post_cov"]
BATCH = ["kstar", "trigemm_sq+V", "batch_rounds"]

CALLS = {
    "predict_f": lambda m, xs: m.predict_f(xs),
    "score": lambda m, xs: m.score("EI", [TAU], xs),
    "score_grad": lambda m, xs: m.score_grad("EI", [TAU], xs),
    "predict_grad": lambda m, xs: m.predict_grad(xs),
    "predict_cov": lambda m, xs: m.predict_cov(xs),
    "select_batch3": lambda m, xs: m.select_batch("EI", [TAU], xs, 3),
    "select_batch2": lambda m, xs: m.select_batch("EI", [TAU], xs, 2),
    "ascend": lambda m, xs: m.ascend("EI", [TAU], np.zeros(D), np.ones(D), xs, maxeval=200),
}

# (N, call, R, labels, score_launches or None, score_chunk or None)
TABLE = [
    (130, "predict_f", 8, SMALL, None, None),
    (130, "score", 8, SMALL, None, None),
    (130, "score_grad", 8, SMALL_G, None, None),
    (130, "score", 300, WHOLE, None, None),
    (130, "score_grad", 300, WHOLE_G, None, None),
    (130, "predict_grad", 8, POST_G, None, None),
    (130, "predict_grad", 300, POST_G, None, None),
    (130, "predict_cov", 40, COV, None, None),
    (130, "select_batch3", 300, BATCH, None, None),
    (900, "score", 300, ["kstar", "split_V", "score"], None, None),
    (900, "score_grad", 300, ["kstar", "split_V", "split_U", "score+grad"], None, None),
    (900, "predict_grad", 300, ["kstar", "split_V", "split_U", "con_post"], None, None),
    (130, "score", R2, WHOLE * 2, 2, CHUNK2),
    (130, "score_grad", R2, WHOLE_G * 2, None, CHUNK2),
    (130, "select_batch2", R2, ["kstar", "trigemm_sq+V"] * 2 + ["batch_rounds"], 2, CHUNK2),
]


def xs_of(R):
    return np.asfortranarray(synth(1, D, R, seed=1000 + R)[2].T)


def make(bohip, N):
    X, y, _ = synth(N, D, 1, seed=N)
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X.T, y)
    m.fit_()
    return m


def flat(res):
    if isinstance(res, np.ndarray):
        return [res]
    if np.isscalar(res):
        return [np.asarray(res)]
    return [a for part in res for a in flat(part)]


def same_bits(got, want):
    got, want = flat(got), flat(want)
    return len(got) == len(want) > 0 and all(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
                                             and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


@pytest.fixture(scope="module")
def fresh(bohip):
    """(N, call, R) -> what the call returns as the first call of a fresh handle; computed once, read-only."""
    cache = {}

    def get(N, call, R):
        if (N, call, R) not in cache:
            m = make(bohip, N)
            try:
                cache[N, call, R] = CALLS[call](m, xs_of(R))
            finally:
                m.close()
            for a in flat(cache[N, call, R]):
                a.setflags(write=False)
        return cache[N, call, R]

    return get


@pytest.mark.parametrize("N,call,R,labels,launches,chunk", TABLE, ids=[f"N{t[0]}-{t[1]}-R{t[2]}" for t in TABLE])
def test_labels_and_bits(bohip, fresh, N, call, R, labels, launches, chunk):
    from bohip import _lib

    want = fresh(N, call, R)
    m = make(bohip, N)
    try:
        m.predict_f(xs_of(1))                       # the throw-away call: whatever a first call adds has run
        m.enable_timing(True)
        got = CALLS[call](m, xs_of(R))
        seen = [name for name, _ in m.timing(cap=4096)]
        print(f"  N = {N} {call} R = {R}: {seen}")
        assert seen == labels
        assert same_bits(got, want), "not equal bit for bit to the first call of a fresh handle"
        if launches is not None:
            assert m.info(_lib.INFO_SCORE_LAUNCHES) == launches
        if chunk is not None:
            assert m.info(_lib.INFO_SCORE_CHUNK) == chunk
    finally:
        m.close()


# the interleaving order: multi-chunk, small, split (N = 900; one whole-K chunk at N = 130), predict_cov, score_grad chunked,
# acquire_max with 4 starts, predict_f
SEQUENCE = [("score", R2), ("score", 8), ("score_grad", 8), ("score", 300), ("score_grad", 300), ("predict_grad", 300),
            ("predict_cov", 40), ("score_grad", R2), ("ascend", 4), ("predict_f", 8)]


def interleave_child():
    """Runs in a child process: both handles through SEQUENCE, each result against a fresh handle's first call."""
    import bohip as b

    out = {}
    for N in (130, 900):
        lived = make(b, N)
        try:
            for call, R in SEQUENCE:
                got = CALLS[call](lived, xs_of(R))
                f = make(b, N)
                try:
                    want = CALLS[call](f, xs_of(R))
                finally:
                    f.close()
                rec = {"same": bool(same_bits(got, want))}
                if call == "ascend":
                    rec["evals"] = [int(got[5]), int(want[5])]
                    rec["best"] = [float(got[2]), int(got[3])]
                out[f"{N}-{call}-{R}"] = rec
        finally:
            lived.close()
    print("RESULT" + json.dumps(out))


@pytest.mark.parametrize("lockstep", [None, "1", "2"], ids=["free", "lockstep", "own_launch"])
def test_interleaved_calls_give_the_fresh_bits(lockstep):
    env = dict(os.environ)
    env.pop("BOHIP_ASC_LOCKSTEP", None)
    if lockstep is not None:
        env["BOHIP_ASC_LOCKSTEP"] = lockstep
    code = "import sys; sys.path[:0] = [%r, %r]; import test_pass_plan_gpu as t; t.interleave_child()" % (ROOT, os.path.join(ROOT, "tests"))
    o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert o.returncode == 0, o.stderr[-2000:]
    res = json.loads([l for l in o.stdout.splitlines() if l.startswith("RESULT")][-1][6:])
    assert len(res) == 2 * len(SEQUENCE)
    for key, rec in res.items():
        print(f"  {key}: {rec}")
        assert rec["same"], (key, "differs from the fresh handle's first call")      # (ascend: f, X, the record, best_x and evals)
        if "evals" in rec:
            assert rec["evals"][0] == rec["evals"][1] >= 1, key
