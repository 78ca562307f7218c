#!/usr/bin/env python
"""Median wall time of posterior sample paths against the joint draw over a candidate set.

    --mode joint    model.sample_joint(X, S): the yardstick, N = 3000, d = 8, R = 4096, S = 1 and 64 (works with an older library
                    build too: BOHIP_LIB selects it, symbols it lacks are not bound)
    --mode paths    this build's model.draw_paths(S, 2048) + eval on the same candidates, S = 1 and 64, with the stage split
    --mode eval     eval alone at R = 4096 and 65536 for S = 1, 8, 64, 256, 1024 (winners only): wall time, the `path_eval` stage and,
                    for the MFMA form, its rate 2 R (N + M) S / t
    --mode forms    the `path_eval` stage at R = 4096 over S = 1 .. 128 with either kernel forced (BOHIP_PATH_MFMA_MIN is read at
                    every draw, so one process measures both): where the two cross is where the library switches
    --mode grad     eval_grad of 10 and 80 points at N = 3000
    --mode draw10k  the draw at N = 10^4, S = 64, M = 2048, with its stage split

    python tools/time_path_draw.py --mode paths [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402
from time_joint_draw import model, problem, stage_medians, timed  # noqa: E402

M = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("joint", "paths", "eval", "forms", "grad", "draw10k"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    if a.mode == "joint":   # an older build lacks the bohip_paths symbols: bind what it exports
        import ctypes
        from bohip import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES):
            for sym in [k for k in table if not hasattr(have, k)]:
                del table[sym]
    N, d, R = (10000, 8, 4096) if a.mode == "draw10k" else (3000, 8, 4096)
    X, y, Xs = problem(N, d, R)
    m = model(X, y)
    if a.mode == "joint":
        for S in (1, 64):
            best = timed(lambda: m.sample_joint(Xs, S, 5, want_samples=False), a.reps)
            full = timed(lambda: m.sample_joint(Xs, S, 5), a.reps)
            print(f"{lib:22s} joint  N={N} R={R} S={S:4d}  winners only: median {np.median(best):8.3f} ms  min {best.min():8.3f} ms;  "
                  f"with samples: median {np.median(full):8.3f} ms", flush=True)
    elif a.mode == "paths":
        for S in (1, 64):
            def both(values):
                with m.draw_paths(S, M, 5) as p:
                    return p.eval(Xs, want_values=values)

            best = timed(lambda: both(False), a.reps)
            full = timed(lambda: both(True), a.reps)
            m.enable_timing(True)                                            # (timing() holds the last call's stages: read it twice)
            rows = []
            for _ in range(a.reps + 1):
                with m.draw_paths(S, M, 5) as p:
                    t_draw = m.timing()
                    p.eval(Xs, want_values=False)
                    rows.append(t_draw + m.timing())
            m.enable_timing(False)
            st = [(n, float(np.median([ms for r in rows[1:] for k, ms in r if k == n]))) for n, _ in rows[0]]
            print(f"{lib:22s} paths N={N} R={R} S={S:4d} M={M}  winners only: median {np.median(best):8.3f} ms  min {best.min():8.3f} ms;  "
                  f"with values: median {np.median(full):8.3f} ms", flush=True)
            print("    " + "  ".join(f"{n} {ms:.3f}" for n, ms in st), flush=True)
    elif a.mode == "eval":
        for Rr in (4096, 65536):
            xs = np.asfortranarray(np.random.default_rng(4).random((Rr, d)).T)
            for S in (1, 8, 64, 256, 1024):
                with m.draw_paths(S, M, 5) as p:
                    ts = timed(lambda: p.eval(xs, want_values=False), a.reps)
                    st = dict(stage_medians(m, lambda: p.eval(xs, want_values=False), a.reps))["path_eval"]
                form = "mfma" if S >= int(os.environ.get("BOHIP_PATH_MFMA_MIN", "24")) else "rows"
                rate = f"  {2.0 * Rr * (N + M) * S / st / 1e9:7.2f} TF/s" if form == "mfma" else ""
                print(f"{lib:22s} eval   N={N} R={Rr:5d} S={S:4d} {form}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  "
                      f"path_eval {st:8.3f} ms{rate}", flush=True)
    elif a.mode == "forms":
        for S in (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 128):
            out = []
            for knob in ("1000000", "1"):                                    # every S on the row form, every S on the MFMA form
                os.environ["BOHIP_PATH_MFMA_MIN"] = knob
                with m.draw_paths(S, M, 5) as p:
                    out.append(dict(stage_medians(m, lambda: p.eval(Xs, want_values=False), a.reps))["path_eval"])
            print(f"{lib:22s} forms  N={N} R={R} S={S:4d}  path_eval: k_path_rows {out[0]:8.3f} ms   k_path_mfma {out[1]:8.3f} ms", flush=True)
        del os.environ["BOHIP_PATH_MFMA_MIN"]
    elif a.mode == "grad":
        with m.draw_paths(64, M, 5) as p:
            for n in (10, 80):
                pts = Xs[:, :n]
                ts = timed(lambda: p.eval_grad(pts, np.arange(n) % 64), a.reps)
                st = dict(stage_medians(m, lambda: p.eval_grad(pts, np.arange(n) % 64), a.reps))["path_grad"]
                print(f"{lib:22s} grad   N={N} points={n:3d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  path_grad {st:8.3f} ms",
                      flush=True)
    else:
        ts = timed(lambda: m.draw_paths(64, M, 5).close(), a.reps)
        st = stage_medians(m, lambda: m.draw_paths(64, M, 5).close(), a.reps)
        print(f"{lib:22s} draw   N={N} S=  64 M={M}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms", flush=True)
        print("    " + "  ".join(f"{n} {ms:.3f}" for n, ms in st), flush=True)
    m.close()


if __name__ == "__main__":
    main()
