"""Raw outputs of every scoring route of the library on seeded inputs, for byte comparisons between two builds.
Usage: dump_scoring_routes.py OUT.npz            (BOHIP_LIB selects the build; run each build in a fresh process)
       dump_scoring_routes.py --compare A.npz B.npz   (exit 1 when an array differs in a byte)
Every case records the arrays a call returns and the timing() stage names of the call, which say which route it took; a case that
did not take the route it is here for is an error.  SE kernel unless said otherwise."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = 0
    for k in sorted(set(a.files) | set(b.files)):
        if k not in a.files or k not in b.files:
            print(f"{k:44s} only in {'A' if k in a.files else 'B'}")
            bad += 1
            continue
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        bad += not same
        print(f"{k:44s} {str(a[k].shape):14s} {'identical' if same else 'DIFFERS'}")
    print(f"{len(a.files)} arrays, {bad} differ")
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    import bohip
    from bohip import _lib

    lib = _lib.load()
    out, routes = {}, []

    def model(N, d, kernel=None, seed=0):
        rng = np.random.default_rng(seed + N)
        X = rng.random((N, d))
        y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
        k = (kernel or bohip.SEArd)(np.full(d, np.log(0.5)), 0.0)
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=k, logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        m.enable_timing(True)
        return m, y

    def cand(N, d, R):
        return np.random.default_rng(7 * N + R + d).random((R, d))

    def stages(m):
        return [n for n, _ in m.timing()]

    def put(case, want, m, **arrays):   # want: stage names the route must show
        st = stages(m)
        assert all(w in st for w in want), (case, want, st)
        routes.append(f"{case}: {' '.join(st)}")
        for k, v in arrays.items():
            out[f"{case}/{k}"] = np.asarray(v)

    def prune_stat(m):
        f = lib.bohip_debug_prune_stat
        f.restype, f.argtypes = C.c_int64, [C.c_void_p]
        return f(m._h)

    def set_form(m, form):
        f = lib.bohip_debug_prune_round2_form
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
        assert f(m._h, form) == 0

    def value_and_grad(case, m, y, Xs, want_v, want_g):
        sc, bv, bi = m.score("EI", [y.max()], Xs.T)
        put(f"{case}/score", want_v, m, scores=sc, best_val=bv, best_idx=bi)
        mu, var = m.predict_f(Xs.T)
        put(f"{case}/predict", want_v, m, mu=mu, var=var)
        sg, g = m.score_grad("EI", [y.max()], Xs.T)
        put(f"{case}/score_grad", want_g, m, scores=sg, grad=g)

    # the small pass: one pass of 16, three passes (no step folded in)
    m, y = model(1100, 3)
    for R in (16, 40):
        value_and_grad(f"small_N1100_d3_R{R}", m, y, cand(1100, 3, R), ["small_V"], ["small_V+U"])
    # split-K, k_grad_finish at two observation splits; d = 20: k_grad_finish<32>
    m, y = model(1600, 3)
    value_and_grad("split_N1600_d3_R300", m, y, cand(1600, 3, 300), ["split_V", "score"], ["split_V", "split_U", "score+grad"])
    m, y = model(1600, 20)
    sg, g = m.score_grad("EI", [y.max()], cand(1600, 20, 300).T)
    put("split_N1600_d20_R300/score_grad", ["split_V", "split_U", "score+grad"], m, scores=sg, grad=g)
    # value-only calls that prune, round 2 in its steady (0) and its long (1) form; N = 1060: the last row tile is a solo upper half
    for N in (1100, 1060):
        for form in (0, 1):
            m, y = model(N, 3)
            set_form(m, form)
            assert prune_stat(m) == -1
            _, bv, bi = m.score("EI", [y.max()], cand(N, 3, 4096).T, want_scores=False)
            stat = prune_stat(m)
            assert stat >= 0, (N, form, stat)   # (-1: the call did not prune)
            put(f"pruned_N{N}_d3_R4096_form{form}", ["kstar", "trigemm_sq"], m, best_val=bv, best_idx=bi, round2_list=stat)
    # the same shape with every output: the fused whole-K pass; with the gradient: the chunked route, k_grad_finish_tiled
    m, y = model(1100, 3)
    value_and_grad("whole_N1100_d3_R4096", m, y, cand(1100, 3, 4096), ["kstar", "trigemm_sq"], ["trigemm_sq+V", "gemm_U", "score+grad"])
    assert prune_stat(m) == -1
    # Matern 3/2: the LOW instantiations of the small pass and of split-K
    m, y = model(1100, 3, kernel=bohip.Mat32Ard)
    value_and_grad("mat32_N1100_d3_R16", m, y, cand(1100, 3, 16), ["small_V"], ["small_V+U"])
    value_and_grad("mat32_N1100_d3_R300", m, y, cand(1100, 3, 300), ["split_V", "score"], ["split_V", "split_U", "score+grad"])
    # acquire_max: the step inside k_small_u (10 starts: one pass), k_asc_step (40 starts: three passes), one workgroup per start (N = 200)
    for N, S, want in ((1100, 10, ["small_V+U"]), (1100, 40, ["small_V+U"]), (200, 10, ["ascent_wg"])):
        m, y = model(N, 3)
        starts = np.random.default_rng(N + S).random((S, 3))
        f, X, bv, bi, bx, ev = m.ascend("UCB", [2.0], np.zeros(3), np.ones(3), starts.T)
        put(f"ascent_N{N}_d3_S{S}", want, m, f=f, x=X, best_val=bv, best_idx=bi, best_x=bx, evaluations=ev)
    out["routes"] = np.array(routes)
    np.savez(sys.argv[1], **out)
    print("\n".join(routes))
    print(f"{len(out) - 1} arrays -> {sys.argv[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
