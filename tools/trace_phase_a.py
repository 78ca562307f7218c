"""Per-workgroup timeline of the phase-A launch of the pruned arg-max at the bench shape (N = 3000, d = 8, R = 4096): span of the
launch, workgroups per CU, duration and cycles per chunk of every job of the table, the loop's phases of a computing wave.
Run with BOHIP_LIB = csrc/abl/libbohip_trace.so (make -C bayesianoptimization.jl_amd/csrc abl/libbohip_trace.so).
PA_TABLE: the job table in launch order, "rt:h,rt:h,..." (h = -1: a whole tile, the form before k_trigemm_sq_pa); default
phase_a_jobs's table for m = 3."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bohip
from bohip import _lib
from bench import synth, lhs, N_OBS, DIM
lib = _lib.load()
X, y = synth(0)
R = 4096
Xs = lhs(R, 1)
m = bohip.ElasticGPE(DIM, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(DIM, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N_OBS)
m.append_(X.T, y)
for _ in range(8):
    m.score("EI", [float(y.max())], Xs.T, want_scores=False)
f = lib.bohip_debug_prune_stat
f.restype, f.argtypes = C.c_int64, [C.c_void_p]
print("prune stat (>= 0: the call pruned):", f(m._h))
tab = [tuple(int(x) for x in e.split(":")) for e in os.environ.get("PA_TABLE", "1:1,1:0,2:1,2:0,0:1,0:0").split(",")]
CT = (R + 63) // 64
n_local = (CT + 7) // 8
nb = 8 * n_local * len(tab)
buf = (C.c_ulonglong * (6 * nb))()
lib.bohip_debug_trace_read.restype = C.c_int
assert lib.bohip_debug_trace_read(buf, C.c_int64(6 * nb)) == 0
t = np.frombuffer(buf, dtype=np.uint64).reshape(nb, 6).astype(np.int64)
t0, t1, hw, xcc_reg = t[:, 0].copy(), t[:, 1].copy(), t[:, 2], t[:, 3]
dw, dc = (t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 5] - t[:, 4]).astype(np.float64)
ok = t1 > 0
mhz = dc[ok] / dw[ok] * 100.0
print(f"core clock over {ok.sum()} workgroups: mean {mhz.mean():.0f} MHz, min {mhz.min():.0f}, max {mhz.max():.0f}")
base = t0[ok].min()
t0 -= base; t1 -= base
span = t1[ok].max()
xcc = xcc_reg & 0xF
cu = (hw >> 8) & 0xF; sh = (hw >> 12) & 1; se = (hw >> 13) & 7
key = ((xcc * 8 + se) * 2 + sh) * 16 + cu
ncu = len(set(key[ok]))
print(f"blocks {nb} (with work {ok.sum()}), span {span} ticks of 10 ns = {span / 100:.2f} us, distinct CUs used {ncu} of 256")
slot = np.arange(nb) >> 3
job = slot // n_local
rt = np.array([tab[j][0] for j in job]); hh = np.array([tab[j][1] for j in job])
pb = (C.c_ulonglong * (nb * 8 * 4))()
lib.bohip_debug_phase_read.restype = C.c_int
assert lib.bohip_debug_phase_read(pb, C.c_int64(nb * 8 * 4)) == 0
ph = np.frombuffer(pb, dtype=np.uint64).reshape(nb, 8, 4).astype(np.float64)
for j, (r_, h_) in enumerate(tab):
    sel = ok & (job == j)
    d = (t1 - t0)[sel]
    cyc = (t[:, 5] - t[:, 4])[sel].astype(np.float64)
    p = ph[sel][:, 0, :]   # wave 0 (a computing wave in every form)
    n = p[:, 3].mean()
    print(f"  job {j}: rt={r_} h={h_:2d}  wgs {sel.sum():3d}  dur mean {d.mean():7.1f} max {d.max():6d} ticks  start mean {t0[sel].mean():7.1f}  end mean {t1[sel].mean():7.1f} max {t1[sel].max():6d}"
          f"  chunks {n:4.0f}  cycles/chunk whole job {cyc.mean() / n:6.0f}  loop: issue+mfma {p[:, 0].sum() / p[:, 3].sum():6.0f} vmcnt {p[:, 1].sum() / p[:, 3].sum():5.0f} barrier {p[:, 2].sum() / p[:, 3].sum():5.0f}")
busy = {}
ev = {}
for k_, a, b in zip(key[ok], t0[ok], t1[ok]):
    busy[k_] = busy.get(k_, 0) + (b - a)
    ev.setdefault(k_, []).append((a, 1)); ev[k_].append((b, -1))
bz = np.array(list(busy.values()))
print(f"workgroups per CU over the launch (sum of WG durations / span), over the {ncu} CUs used: mean {bz.mean() / span:.3f}; over all 256 CUs: {bz.sum() / span / 256:.3f}")
cnt = np.array([len(v) // 2 for v in ev.values()])
print(f"workgroups placed per used CU: min {cnt.min()} mean {cnt.mean():.2f} max {cnt.max()}")
e = np.array([max(b for b, d in v if d < 0) for v in ev.values()])
print(f"per-CU last end: min {e.min()} mean {e.mean():.0f} max {e.max()} (span {span})")
