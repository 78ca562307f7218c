"""Multi-GPU model: the candidate set of the multi-restart search (reference src/acquisition.jl:54-68) sharded over a
device list inside ONE process, through the ``bohip_mgp_*`` entry points of libbohip (in-library RCCL: ncclCommInitAll,
one ncclAllGather of the 16-byte arg-max records, device-side reduce).  Same surface as ``ElasticGPE`` where it applies.

The one-process-per-GPU form (``torch.distributed.run``) uses ``ElasticGPE.comm_init`` / ``score_sharded_dev`` instead;
``dist.py`` keeps the torch.distributed fallback used by the CPU (gloo) tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Best, check
from .model import MeanZero, SEArd, _cols, _ptr


def _params(params):
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
    if p.size < 2:
        p = np.concatenate([p, np.zeros(2 - p.size)])
    return p


class MultiGPE:
    """``MultiGPE(d, devices=[0, 1, ...], shards_per_device=1; mean, kernel, logNoise, capacity)``: one replica of the
    GP per device (x, y and the hyper-parameters are broadcast; every device factors redundantly), candidates sharded
    contiguously, winners exchanged over RCCL.  ``score`` returns the GLOBAL (value, index), bit-identical to
    ``ElasticGPE.score`` on the whole set."""

    def __init__(self, d, devices=(0,), shards_per_device=1, mean=None, kernel=None, logNoise=-2.0, capacity=1024, collapse=False):
        if collapse:
            raise ValueError("MultiGPE does not support replicated sites (collapse=True): the device list keeps its replicas in step "
                             "by plain appends; use ElasticGPE(collapse=True) on one device")
        self.dim = int(d)
        self.mean = mean if mean is not None else MeanZero()
        self.kernel = kernel if kernel is not None else SEArd(np.zeros(d), 0.0)
        self.logNoise = float(logNoise)
        self.devices = [int(v) for v in devices]
        self.shards_per_device = int(shards_per_device)
        self._lib = _lib.load()
        h = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        check(self._lib.bohip_mgp_create(self.dim, int(capacity), _lib.KERN[self.kernel.kern], devs, len(self.devices),
                                         self.shards_per_device, C.byref(h)))
        self._h = h
        _lib.register(self)
        self._x = np.zeros((self.dim, 0), order="F")
        self._y = np.zeros(0)
        self._push_hyper()

    def close(self):
        """Release every replica, the communicators and the worker threads now (idempotent; run at interpreter exit too)."""
        h, self._h = getattr(self, "_h", None), None
        for p in list(getattr(self, "_paths", ())):               # paths objects borrow a replica's stream: they go first
            p.close()
        if h:
            self._lib.bohip_mgp_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _push_hyper(self):
        ll = self.kernel.ll
        ll = np.ascontiguousarray(np.broadcast_to(ll, (self.dim,)) if ll.size == 1 else ll)
        check(self._lib.bohip_mgp_set_hyper(self._h, _ptr(ll), self.kernel.lsigma, self.logNoise, self.mean.beta))

    x = property(lambda self: self._x)
    y = property(lambda self: self._y)
    nobs = property(lambda self: self._y.size)

    @property
    def n_shards(self):
        return self.info(_lib.MGP_INFO_SHARDS)

    def info(self, what):
        v = C.c_int64()
        check(self._lib.bohip_mgp_info(self._h, what, C.byref(v)))
        return v.value

    def append_(self, x, y):
        x = _cols(x, self.dim)
        y = np.ascontiguousarray(np.atleast_1d(np.asarray(y, dtype=np.float64)))
        if x.shape[1] != y.size:
            raise ValueError("x and y disagree on the number of observations")
        rc = self._lib.bohip_mgp_append(self._h, _ptr(x), _ptr(y), y.size)
        if rc in (_lib.OK, _lib.E_NOTPD):
            self._x = np.asfortranarray(np.concatenate([self._x, x], axis=1))
            self._y = np.concatenate([self._y, y])
        check(rc)
        return self

    def append_sites_(self, x, ybar, reps, ss, ymax=None):
        raise ValueError("MultiGPE does not support replicated sites (append_sites_): the device list keeps its replicas in step by "
                         "plain appends; use ElasticGPE(collapse=True) on one device")

    def fit_(self):
        check(self._lib.bohip_mgp_refit(self._h))
        return self

    def score(self, acq, params, xs, want_scores=True):
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        p = _params(params)
        sc = np.empty(R) if want_scores else None
        best = Best()
        check(self._lib.bohip_mgp_score(self._h, _lib.ACQ[acq], _ptr(p), _ptr(xs), R, _ptr(sc) if want_scores else None,
                                        C.byref(best)))
        return sc, best.val, best.idx

    def select_batch(self, acq, params, xs, q, fantasy="believer", raise_tau=False):
        """Not implemented for a device list: every shard of V' would need the picked candidate's row v_s broadcast per round
        (DESIGN.md 10).  Use ElasticGPE.select_batch on one device."""
        raise NotImplementedError("MultiGPE.select_batch: batch selection runs on one device (ElasticGPE.select_batch)")

    def set_pending(self, xp):
        """Not implemented for a device list: the pending set and the state derived from it live on ONE handle.  Use
        ElasticGPE.set_pending on one device."""
        raise NotImplementedError("MultiGPE.set_pending: pending evaluations run on one device (ElasticGPE.set_pending)")

    def set_candidates(self, xs):
        xs = _cols(xs, self.dim)
        check(self._lib.bohip_mgp_set_candidates(self._h, _ptr(xs), xs.shape[1]))

    def score_resident(self, acq, params):
        p = _params(params)
        best = Best()
        check(self._lib.bohip_mgp_score_resident(self._h, _lib.ACQ[acq], _ptr(p), C.byref(best)))
        return best.val, best.idx

    def thompson(self, xs, S, seed=0):
        xs = _cols(xs, self.dim)
        out = (Best * S)()
        check(self._lib.bohip_mgp_thompson(self._h, _ptr(xs), xs.shape[1], S, seed, out))
        return np.array([b.val for b in out]), np.array([b.idx for b in out], dtype=np.int64)

    def set_maxtime(self, seconds):
        """NLopt's maxtime for the device ascent, on every replica (0 = unlimited)."""
        check(self._lib.bohip_mgp_set_maxtime(self._h, float(seconds)))

    def set_ascent_stop(self, ftol_abs=0.0, xtol_rel=0.0, stopval=float("inf")):
        """NLopt's ftol_abs / xtol_rel / stopval for the device ascent, on every replica"""
        check(self._lib.bohip_mgp_set_ascent_stop(self._h, float(ftol_abs), float(xtol_rel), float(stopval)))

    def set_jitter(self, rel, max_tries=10):
        """see ElasticGPE.set_jitter; applied to every replica"""
        check(self._lib.bohip_mgp_set_jitter(self._h, float(rel), int(max_tries)))

    def ascend(self, acq, params, lowerbounds, upperbounds, starts, maxeval=2000, ftol_rel=1e-10, xtol_abs=1e-10):
        starts = _cols(starts, self.dim)
        R = starts.shape[1]
        p = _params(params)
        lb = np.ascontiguousarray(lowerbounds, dtype=np.float64)
        ub = np.ascontiguousarray(upperbounds, dtype=np.float64)
        f = np.empty(R)
        X = np.empty((self.dim, R), order="F")
        best = Best()
        bx = np.empty(self.dim)
        ev = C.c_int64(0)
        check(self._lib.bohip_mgp_acquire_max(self._h, _lib.ACQ[acq], _ptr(p), _ptr(lb), _ptr(ub), _ptr(starts), R, int(maxeval),
                                              float(ftol_rel), float(xtol_abs), _ptr(X), _ptr(f), C.byref(best), _ptr(bx),
                                              C.byref(ev)))
        return f, X, best.val, best.idx, bx, ev.value

    def direct_max(self, acq, params, lowerbounds, upperbounds, maxeval=2000, stopval=float("inf"), maxtime=0.0, seed=0):
        """:GN_DIRECT_L in one library call (ElasticGPE.direct_max, bohip_gp_direct_max) on the FIRST replica: an iteration of the search is a
        handful of points that depend on the iteration before, so there is nothing to shard -- every device holds the whole model."""
        lb = np.ascontiguousarray(lowerbounds, dtype=np.float64)
        ub = np.ascontiguousarray(upperbounds, dtype=np.float64)
        if lb.size != self.dim or ub.size != self.dim:
            raise ValueError("bounds must have one entry per input dimension")
        p = np.zeros(2)
        if params is not None:
            q = np.atleast_1d(np.asarray(params, dtype=np.float64))
            p[:q.size] = q[:2]
        g = self._lib.bohip_mgp_handle(self._h, 0)
        bf = C.c_double(); bx = np.empty(self.dim); ev = C.c_int64(); dc = C.c_int64()
        check(self._lib.bohip_gp_direct_max(g, _lib.ACQ[acq], _ptr(p), _ptr(lb), _ptr(ub), int(maxeval), float(stopval),
                                            float(maxtime or 0.0), int(seed), C.byref(bf), _ptr(bx), C.byref(ev), C.byref(dc)))
        return float(bf.value), bx, int(ev.value), int(dc.value)

    def sample_joint(self, xs, S=1, seed=0, jitter=1e-12, max_tries=40, want_samples=True, want_factor=False):
        """Joint posterior draws (ElasticGPE.sample_joint, bohip_gp_sample_joint) on the FIRST replica: Sigma couples all candidates,
        so there is nothing to shard -- every device holds the whole model."""
        from .model import _sample_joint

        g = self._lib.bohip_mgp_handle(self._h, 0)
        return _sample_joint(self._lib, g, _cols(xs, self.dim), S, seed, jitter, max_tries, want_samples, want_factor)

    def nei(self, X, S=32, seed=0, acq="ei", jitter_rel=1e-8, want_scores=True):
        """ElasticGPE.nei (bohip_gp_score_nei) on the FIRST replica, as sample_joint: the noise-free companion and the fantasies live
        on ONE handle."""
        from .model import _nei

        return _nei(self._lib, self._lib.bohip_mgp_handle(self._h, 0), _cols(X, self.dim), S, seed, acq, jitter_rel, want_scores)

    def nei_fantasies(self, S=32, seed=0, jitter_rel=1e-8):
        """ElasticGPE.nei_fantasies (bohip_gp_nei_fantasies) on the FIRST replica."""
        from .model import _nei_fantasies

        return _nei_fantasies(self._lib, self._lib.bohip_mgp_handle(self._h, 0), self._y.size, S, seed, jitter_rel)

    def qei_batch(self, xs, q, S=256, seed=0, tau=None, jitter=1e-12, max_tries=40, want_samples=False):
        """ElasticGPE.qei_batch (bohip_gp_qei_batch) on the FIRST replica, as sample_joint."""
        from .model import _qei_batch, maxy

        g = self._lib.bohip_mgp_handle(self._h, 0)
        return _qei_batch(self._lib, g, _cols(xs, self.dim), q, S, seed, maxy(self) if tau is None else tau, jitter, max_tries,
                          want_samples)

    def qei_select(self, samples, tau, q):
        """ElasticGPE.qei_select (bohip_gp_qei_select) on the FIRST replica."""
        from .model import _qei_select

        return _qei_select(self._lib, self._lib.bohip_mgp_handle(self._h, 0), samples, tau, q)

    def kg(self, xs, n_eval=None):
        """ElasticGPE.kg (bohip_gp_kg) on the FIRST replica, as sample_joint: Sigma couples all candidates."""
        from .model import _kg

        return _kg(self._lib, self._lib.bohip_mgp_handle(self._h, 0), _cols(xs, self.dim), n_eval)

    def kg_lines(self, a, B):
        """ElasticGPE.kg_lines (bohip_kg_lines) on the FIRST replica."""
        from .model import _kg_lines

        return _kg_lines(self._lib, self._lib.bohip_mgp_handle(self._h, 0), a, B)

    def mes(self, xs, samples=16, mode="gumbel", seed=0, floor=None, jitter_rel=1e-12, max_tries=40):
        """ElasticGPE.mes (bohip_gp_mes) on the FIRST replica, as kg: the max values are those of the whole candidate set."""
        from .model import _mes

        return _mes(self._lib, self._lib.bohip_mgp_handle(self._h, 0), _cols(xs, self.dim), samples, mode, seed, floor, jitter_rel,
                    max_tries)

    def mes_values(self, mu, var, maxvals, want_grad=False):
        """ElasticGPE.mes_values (bohip_mes_values) on the FIRST replica."""
        from .model import _mes_values

        return _mes_values(self._lib, self._lib.bohip_mgp_handle(self._h, 0), mu, var, maxvals, want_grad)

    def mes_gumbel(self, mu, var, samples=16, seed=0, floor=None):
        """ElasticGPE.mes_gumbel (bohip_mes_gumbel) on the FIRST replica."""
        from .model import _mes_gumbel

        return _mes_gumbel(self._lib, self._lib.bohip_mgp_handle(self._h, 0), mu, var, samples, seed, floor)

    def mll_batch_dims(self):
        P, nmax = C.c_int64(), C.c_int64()
        check(self._lib.bohip_gp_mll_batch_dims(self._lib.bohip_mgp_handle(self._h, 0), C.byref(P), C.byref(nmax)))
        return int(P.value), int(nmax.value)

    def mll_grad_batch(self, Theta, want_grad=True):
        """ElasticGPE.mll_grad_batch on the FIRST replica, as draw_paths: every device holds the whole model."""
        from .model import _mll_grad_batch

        return _mll_grad_batch(self._lib, self._lib.bohip_mgp_handle(self._h, 0), Theta, want_grad)

    def loo(self):
        """ElasticGPE.loo (bohip_gp_loo) on the FIRST replica, as mll_grad_batch: every device holds the whole model."""
        from .model import _loo

        return _loo(self._lib, self._lib.bohip_mgp_handle(self._h, 0), self._y)

    def loo_grad(self):
        """ElasticGPE.loo_grad (bohip_gp_loo_grad) on the FIRST replica."""
        from .model import _loo_grad

        return _loo_grad(self._lib, self._lib.bohip_mgp_handle(self._h, 0), (1 if self.kernel.iso else self.dim) + 1)

    def loo_grad_batch(self, Theta, want_grad=True, want_logp=False):
        """ElasticGPE.loo_grad_batch (bohip_gp_loo_grad_batch) on the FIRST replica."""
        from .model import _loo_grad_batch

        return _loo_grad_batch(self._lib, self._lib.bohip_mgp_handle(self._h, 0), self.nobs, Theta, want_grad, want_logp)

    def draw_paths(self, S=1, M=2048, seed=0):
        """Posterior sample paths (ElasticGPE.draw_paths, bohip_gp_paths_draw) on the FIRST replica, as sample_joint: the object is
        self-contained and lives on that device.  Close it before the model."""
        import weakref

        from .model import PosteriorPaths

        p = PosteriorPaths(self._lib, self._lib.bohip_mgp_handle(self._h, 0), self.dim, S, M, seed)
        if not hasattr(self, "_paths"):
            self._paths = weakref.WeakSet()
        self._paths.add(p)
        return p

    def replica_factor(self, i):
        """Cholesky factor held by the i-th device (tests: every replica is the same model)."""
        g = self._lib.bohip_mgp_handle(self._h, i)
        L = np.zeros((self.nobs, self.nobs))
        check(self._lib.bohip_gp_get_factor(g, _ptr(L)))
        return L


def comm_unique_id():
    """The bytes rank 0 ships to the other ranks (ncclUniqueId) before ``ElasticGPE.comm_init``."""
    buf = (C.c_char * _lib.UNIQUE_ID_BYTES)()
    check(_lib.load().bohip_comm_unique_id(buf, _lib.UNIQUE_ID_BYTES))
    return bytes(buf)
