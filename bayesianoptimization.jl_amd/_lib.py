"""ctypes binding of libbohip.so (include/bohip.h, include/bohip_paths.h, include/bohip_fit.h, include/bohip_qei.h, include/bohip_acq.h, include/bohip_kg.h, include/bohip_ens.h, include/bohip_ens_grad.h, include/bohip_mes.h, include/bohip_con.h, include/bohip_mo.h, include/bohip_mom.h, include/bohip_loo.h, include/bohip_loo_batch.h, include/bohip_rep.h, include/bohip_pend.h, include/bohip_nei.h).  No CPU fallback: importing works without a
GPU (so the ABI can be inspected), but every compute entry point raises when the library or the
device is missing."""
from __future__ import annotations

import atexit
import ctypes as C
import importlib.util
import os
import sys
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOHIP_LIB") or os.path.join(_HERE, "csrc", "libbohip.so")   # BOHIP_LIB: measurement builds (csrc/abl)

OK, E_ARG, E_NOTPD, E_HIP, E_NODEVICE, E_STATE, E_UNSUPPORTED, E_COMM = 0, -1, -2, -3, -4, -5, -6, -7
KERN = {"SEArd": 0, "SEIso": 1, "Mat52Ard": 2, "Mat32Ard": 3, "Mat12Ard": 4, "Mat52Iso": 5, "Mat32Iso": 6, "Mat12Iso": 7}
ACQ = {"EI": 0, "PI": 1, "UCB": 2, "MI": 3, "MaxMean": 4, "ThompsonDraw": 5, "LogEI": 6}   # (5: bohip_gp_direct_max only; 6: bohip_acq.h)
INFO_PIVOT, INFO_CAPACITY, INFO_REFITS, INFO_APPENDS = 0, 1, 2, 3
INFO_CHOL_FORM, INFO_CHOL_FALLBACKS, INFO_CHOL_ABORT_TILES, INFO_JITTER_STEPS = 4, 5, 6, 7
INFO_SCORE_LAUNCHES, INFO_SCORE_CHUNK, INFO_KERNEL_CLOCK_MHZ = 8, 9, 10
INFO_COMM_NRANKS, INFO_COMM_EXCHANGES, INFO_COMM_RCCL_VERSION, INFO_CHOL_LOCK_SKIPS = 11, 12, 13, 14
MGP_INFO_DEVICES, MGP_INFO_SHARDS, MGP_INFO_EXCHANGES, MGP_INFO_RCCL_VERSION, MGP_INFO_COMM_NRANKS = 0, 1, 2, 3, 4
UNIQUE_ID_BYTES = 128
FANTASY_BELIEVER, FANTASY_CONST, BATCH_RAISE_TAU = 0, 1, 1   # bohip_gp_select_batch
PATHS_S_MAX, PATHS_M_MAX = 4096, 16384                       # bohip_gp_paths_draw
FIT_NMAX = 512                                               # bohip_gp_mll_grad_batch
KG_RMAX = 8192                                               # bohip_gp_kg / bohip_kg_lines (BOHIP_KG_RMAX)
MES_KMAX, MES_RMAX, MES_GUMBEL, MES_JOINT = 1024, 524288, 0, 1  # bohip_gp_mes / bohip_mes_values / bohip_mes_gumbel


class Best(C.Structure):
    _fields_ = [("val", C.c_double), ("idx", C.c_int64)]


class BohipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbohip error {code}: {msg}")
        self.code = code


class NotPositiveDefinite(BohipError):
    pass


_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_gp = C.c_void_p
_mgp = C.c_void_p
_ip = C.POINTER(C.c_int)

# every symbol include/bohip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "bohip_gp_create": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(_gp)]),
    "bohip_gp_destroy": (None, [_gp]),
    "bohip_gp_set_hyper": (C.c_int, [_gp, _dp, C.c_double, C.c_double, C.c_double]),
    "bohip_gp_append": (C.c_int, [_gp, _dp, _dp, C.c_int64]),
    "bohip_gp_refit": (C.c_int, [_gp]),
    "bohip_gp_dims": (C.c_int, [_gp, _i64p, _i64p]),
    "bohip_gp_maxy": (C.c_int, [_gp, _dp]),
    "bohip_gp_get_xy": (C.c_int, [_gp, _dp, _dp]),
    "bohip_gp_mll": (C.c_int, [_gp, _dp]),
    "bohip_gp_mll_grad": (C.c_int, [_gp, _dp, _dp, _dp, _dp]),
    "bohip_gp_set_batch_hint": (C.c_int, [_gp, C.c_int64]),
    "bohip_gp_predict_cov": (C.c_int, [_gp, _dp, C.c_int64, _dp, _dp]),
    "bohip_gp_acquire_max": (C.c_int, [_gp, C.c_int, _dp, _dp, _dp, _dp, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                      _dp, _dp, C.POINTER(Best), _dp, _i64p]),
    "bohip_gp_set_maxtime": (C.c_int, [_gp, C.c_double]),
    "bohip_gp_set_ascent_stop": (C.c_int, [_gp, C.c_double, C.c_double, C.c_double]),
    "bohip_gp_set_jitter": (C.c_int, [_gp, C.c_double, C.c_int]),
    "bohip_gp_predict": (C.c_int, [_gp, _dp, C.c_int64, _dp, _dp]),
    "bohip_gp_score": (C.c_int, [_gp, C.c_int, _dp, _dp, C.c_int64, _dp, C.POINTER(Best)]),
    "bohip_gp_select_batch": (C.c_int, [_gp, C.c_int, _dp, _dp, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_int, _i64p, _dp, _dp,
                                       _dp]),
    "bohip_gp_score_grad": (C.c_int, [_gp, C.c_int, _dp, _dp, C.c_int64, _dp, _dp]),
    "bohip_gp_thompson": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.POINTER(Best)]),
    "bohip_thompson_normal": (C.c_double, [C.c_uint64, C.c_int64, C.c_int64]),
    "bohip_gp_sample_joint": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_double, C.c_int, _dp, _dp, _dp,
                                       C.POINTER(Best), _dp, _ip]),
    "bohip_direct_create": (C.c_int, [C.c_int64, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "bohip_direct_destroy": (None, [C.c_void_p]),
    "bohip_direct_ask": (C.c_int, [C.c_void_p, _dp, C.c_int64, _i64p]),
    "bohip_direct_tell": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "bohip_direct_best": (C.c_int, [C.c_void_p, _dp, _dp, _i64p, _i64p]),
    "bohip_gp_direct_max": (C.c_int, [_gp, C.c_int, _dp, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.c_uint64, _dp, _dp,
                                     _i64p, _i64p]),
    "bohip_gp_score_dev": (C.c_int, [_gp, C.c_int, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bohip_gp_predict_dev": (C.c_int, [_gp, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bohip_gp_set_stream": (C.c_int, [_gp, C.c_void_p]),
    "bohip_gp_synchronize": (C.c_int, [_gp]),
    "bohip_gp_get_factor": (C.c_int, [_gp, _dp]),
    "bohip_gp_get_alpha": (C.c_int, [_gp, _dp]),
    "bohip_gp_info": (C.c_int, [_gp, C.c_int, _i64p]),
    "bohip_debug_set_chol_inv_g": (C.c_int, [C.c_int]),
    "bohip_gp_enable_timing": (C.c_int, [_gp, C.c_int]),
    "bohip_gp_get_timing": (C.c_int, [_gp, C.POINTER(C.c_char_p), _dp, C.c_int]),
    # multi-GPU: one process, a device list (in-library RCCL)
    "bohip_mgp_create": (C.c_int, [C.c_int64, C.c_int64, C.c_int, _ip, C.c_int, C.c_int, C.POINTER(_mgp)]),
    "bohip_mgp_destroy": (None, [_mgp]),
    "bohip_mgp_set_hyper": (C.c_int, [_mgp, _dp, C.c_double, C.c_double, C.c_double]),
    "bohip_mgp_append": (C.c_int, [_mgp, _dp, _dp, C.c_int64]),
    "bohip_mgp_refit": (C.c_int, [_mgp]),
    "bohip_mgp_score": (C.c_int, [_mgp, C.c_int, _dp, _dp, C.c_int64, _dp, C.POINTER(Best)]),
    "bohip_mgp_set_candidates": (C.c_int, [_mgp, _dp, C.c_int64]),
    "bohip_mgp_score_resident": (C.c_int, [_mgp, C.c_int, _dp, C.POINTER(Best)]),
    "bohip_mgp_thompson": (C.c_int, [_mgp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.POINTER(Best)]),
    "bohip_mgp_acquire_max": (C.c_int, [_mgp, C.c_int, _dp, _dp, _dp, _dp, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                       _dp, _dp, C.POINTER(Best), _dp, _i64p]),
    "bohip_mgp_set_maxtime": (C.c_int, [_mgp, C.c_double]),
    "bohip_mgp_set_ascent_stop": (C.c_int, [_mgp, C.c_double, C.c_double, C.c_double]),
    "bohip_mgp_set_jitter": (C.c_int, [_mgp, C.c_double, C.c_int]),
    "bohip_mgp_handle": (_gp, [_mgp, C.c_int]),
    "bohip_mgp_info": (C.c_int, [_mgp, C.c_int, _i64p]),
    # multi-GPU: one process per device
    "bohip_comm_unique_id": (C.c_int, [C.c_void_p, C.c_int64]),
    "bohip_gp_comm_init": (C.c_int, [_gp, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "bohip_gp_comm_destroy": (C.c_int, [_gp]),
    "bohip_gp_score_sharded_dev": (C.c_int, [_gp, C.c_int, _dp, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_void_p]),
    "bohip_gp_thompson_sharded": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_int64,
                                           C.POINTER(Best)]),
    "bohip_last_error": (C.c_char_p, []),
    "bohip_version": (C.c_char_p, []),
    "bohip_device_count": (C.c_int, []),
}

# every symbol include/bohip_paths.h declares (the posterior sample paths, an object of its own beside the model's ABI)
_paths = C.c_void_p
PATHS_SIGNATURES = {
    "bohip_gp_paths_draw": (C.c_int, [_gp, C.c_int64, C.c_int64, C.c_uint64, C.POINTER(_paths)]),
    "bohip_paths_destroy": (None, [_paths]),
    "bohip_paths_dims": (C.c_int, [_paths, _i64p, _i64p, _i64p, _i64p]),
    "bohip_paths_eval": (C.c_int, [_paths, _dp, C.c_int64, _dp, C.POINTER(Best)]),
    "bohip_paths_eval_grad": (C.c_int, [_paths, _dp, C.c_int64, _i64p, _dp, _dp]),
    "bohip_paths_coef": (C.c_int, [_paths, C.c_int64, _dp, _dp, _dp]),
}

# every symbol include/bohip_fit.h declares (the marginal likelihood and its gradient at H settings in one launch)
FIT_SIGNATURES = {
    "bohip_gp_mll_batch_dims": (C.c_int, [_gp, _i64p, _i64p]),
    "bohip_gp_mll_grad_batch": (C.c_int, [_gp, C.c_int64, _dp, _dp, _dp, _i64p]),
}

# every symbol include/bohip_qei.h declares (greedy Monte-Carlo q-EI over joint draws that stay on the device)
QEI_SIGNATURES = {
    "bohip_gp_qei_batch": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_double, C.c_int, C.c_double, C.c_int64, _i64p, _dp,
                                    _dp, _dp, _ip]),
    "bohip_gp_qei_select": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_double, C.c_int64, _i64p, _dp]),
}

# every symbol include/bohip_acq.h declares (the acquisition functors and their partials on their own; the id of LogEI)
ACQ_SIGNATURES = {
    "bohip_acq_eval": (C.c_int, [C.c_int, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp]),
}

# every symbol include/bohip_kg.h declares (the knowledge gradient over a candidate set, exact, on the device)
_i32p = C.POINTER(C.c_int32)
KG_SIGNATURES = {
    "bohip_gp_kg": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, _dp, _i32p, _dp, C.POINTER(Best)]),
    "bohip_kg_lines": (C.c_int, [_gp, _dp, _dp, C.c_int64, C.c_int64, _dp, _i32p]),
}

# every symbol include/bohip_ens.h declares (one acquisition averaged over H hyper-parameter settings, on the device)
ENS_SIGNATURES = {
    "bohip_gp_score_ens": (C.c_int, [_gp, C.c_int, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp, _i64p, C.POINTER(Best)]),
}

# every symbol include/bohip_ens_grad.h declares (the gradient of that average, on the device)
ENS_GRAD_SIGNATURES = {
    "bohip_gp_score_ens_grad": (C.c_int, [_gp, C.c_int, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _i64p,
                                          C.POINTER(Best)]),
}

# every symbol include/bohip_mes.h declares (max-value entropy search over a candidate set, on the device)
MES_SIGNATURES = {
    "bohip_gp_mes": (C.c_int, [_gp, _dp, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp,
                               _dp, C.POINTER(Best), _dp, _ip]),
    "bohip_mes_values": (C.c_int, [_gp, _dp, _dp, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_mes_gumbel": (C.c_int, [_gp, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_double, _dp, _dp]),
}

# every symbol include/bohip_con.h declares (constrained optimisation: the posterior's Jacobians, the combine stage, the whole call)
CON_FEASIBILITY = -1
CON_CMAX = 16
CON_SIGNATURES = {
    "bohip_gp_predict_grad": (C.c_int, [_gp, _dp, C.c_int64, _dp, _dp, _dp, _dp]),
    "bohip_con_values": (C.c_int, [_gp, C.c_int, _dp, C.c_int64, _dp, _ip, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_gp_score_con": (C.c_int, [_gp, C.c_int, _dp, C.c_int64, C.POINTER(_gp), _dp, _ip, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp,
                                     C.POINTER(Best)]),
}

# every symbol include/bohip_mo.h declares (two objectives: the observed front on the host, the exact EHVI stage, the whole call)
MO_FRONT_MAX = 1024
MO_GROUP = 16
MO_SIGNATURES = {
    "bohip_mo_front": (C.c_int, [_dp, C.c_int64, _dp, _dp, C.c_int64, _i64p, _dp]),
    "bohip_mo_ehvi_values": (C.c_int, [_gp, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_gp_score_mo": (C.c_int, [_gp, _gp, _dp, C.c_int64, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp, C.POINTER(Best)]),
}

# every symbol include/bohip_mom.h declares (two to four objectives: the front and its boxes on the host, the exact EHVI stage over the
# boxes, the whole call)
MOM_OBJ_MAX, MOM_FRONT_MAX, MOM_BOX_MAX, MOM_LANES = 4, 256, 65536, 64
MOM_SIGNATURES = {
    "bohip_mom_front": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, _dp, C.c_int64, _i64p, _dp]),
    "bohip_mom_boxes": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, _dp, _i64p, _i32p, C.c_int64, _i64p]),
    "bohip_mom_ehvi_values": (C.c_int, [_gp, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_gp_score_mom": (C.c_int, [C.POINTER(_gp), C.c_int64, _dp, C.c_int64, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp, C.POINTER(Best)]),
}

# every symbol include/bohip_loo.h declares (leave-one-out predictions at the observations, their log-probability and its gradient)
LOO_SIGNATURES = {
    "bohip_gp_loo": (C.c_int, [_gp, _dp, _dp, _dp, _dp]),
    "bohip_gp_loo_grad": (C.c_int, [_gp, _dp, _dp, _dp, _dp]),
}

# the symbol include/bohip_loo_batch.h declares (the leave-one-out objective and its gradient at H settings in one launch)
LOO_BATCH_SIGNATURES = {
    "bohip_gp_loo_grad_batch": (C.c_int, [_gp, C.c_int64, _dp, _dp, _dp, _dp, _i64p]),
}

# every symbol include/bohip_rep.h declares (replicated sites: r evaluations at one position as one row with noise nu / r)
REP_SIGNATURES = {
    "bohip_gp_append_sites": (C.c_int, [_gp, _dp, _dp, _i64p, _dp, C.c_int64]),
    "bohip_gp_sites_info": (C.c_int, [_gp, _i64p, _i64p, _dp, _dp, _ip]),
    "bohip_gp_get_reps": (C.c_int, [_gp, _i64p]),
}

# every symbol include/bohip_pend.h declares (pending evaluations: the acquisition averaged over fantasies at points out for evaluation)
PEND_PMAX, PEND_SMAX, PEND_RAISE_TAU = 32, 1024, 1
PEND_SIGNATURES = {
    "bohip_gp_pending_set": (C.c_int, [_gp, _dp, C.c_int64]),
    "bohip_gp_pending_info": (C.c_int, [_gp, _i64p, _dp, _dp, _dp]),
    "bohip_gp_score_pending": (C.c_int, [_gp, C.c_int, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_int, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_pend_values": (C.c_int, [_gp, C.c_int, _dp, C.c_int64, C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(Best)]),
}

# every symbol include/bohip_nei.h declares (noisy expected improvement: EI / PI / LogEI averaged over posterior draws of the noise-free
# function values at the observed sites)
NEI_SMAX = 1024
NEI_INFO_REFITS, NEI_INFO_APPENDS, NEI_INFO_REBUILDS, NEI_INFO_JITTER_STEPS, NEI_INFO_BYTES, NEI_INFO_DELTA = 0, 1, 2, 3, 4, 5
NEI_SIGNATURES = {
    "bohip_gp_nei_prepare": (C.c_int, [_gp, C.c_double, C.c_int64, C.c_uint64]),
    "bohip_gp_nei_fantasies": (C.c_int, [_gp, C.c_double, C.c_int64, C.c_uint64, _dp, _dp]),
    "bohip_gp_score_nei": (C.c_int, [_gp, C.c_int, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_double, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_nei_values": (C.c_int, [_gp, C.c_int, C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, C.POINTER(Best)]),
    "bohip_gp_nei_info": (C.c_int, [_gp, C.c_int, _dp]),
    "bohip_gp_nei_release": (C.c_int, [_gp]),
}

_lib = None

# Live device objects are closed at interpreter exit BEFORE the HIP / RCCL runtimes run their own static destructors:
# a handle finalised after that (e.g. one kept alive by a traceback until shutdown) would free into a dead runtime.
_live = weakref.WeakSet()


def register(obj):
    _live.add(obj)


@atexit.register
def _close_all():
    for o in list(_live):
        try:
            o.close()
        except Exception:
            pass


def _one_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
    /opt/rocm's); whichever is dlopen'ed first wins for both users, and torch cannot see the GPU when
    the system copy got there first.  So when PyTorch is installed (it is the plumbing for device
    memory, streams and the process group in bench.py / dist.py) and not yet imported, load its copy
    first.  BOHIP_SYSTEM_HIP=1 skips this.  RCCL needs no such care: libbohip binds it with
    dlopen("librccl.so.1") at the first multi-GPU call, which returns the copy the process already holds
    (preloading torch's librccl here made the process abort in a static destructor at exit)."""
    if "torch" in sys.modules or os.environ.get("BOHIP_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    for name in ("libamdhip64.so",):
        cand = os.path.join(os.path.dirname(spec.origin), "lib", name)
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def load():
    """dlopen libbohip.so and bind every declared symbol (all headers).  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BohipError(E_NODEVICE, f"{LIB_PATH} not built (run __graft_entry__.build()); there is no CPU fallback")
    _one_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(PATHS_SIGNATURES.items()) + list(FIT_SIGNATURES.items())
                              + list(QEI_SIGNATURES.items()) + list(ACQ_SIGNATURES.items()) + list(KG_SIGNATURES.items())
                              + list(ENS_SIGNATURES.items()) + list(ENS_GRAD_SIGNATURES.items()) + list(MES_SIGNATURES.items())
                              + list(CON_SIGNATURES.items()) + list(MO_SIGNATURES.items()) + list(LOO_SIGNATURES.items())
                              + list(LOO_BATCH_SIGNATURES.items()) + list(REP_SIGNATURES.items()) + list(PEND_SIGNATURES.items())
                              + list(NEI_SIGNATURES.items()) + list(MOM_SIGNATURES.items())):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def acq_eval(acq, params, mu, var, partials=True):
    """bohip_acq_eval: the functor `acq` (a key of ACQ) on the (mu, var) pairs, on the device.  -> (value, dmu, dvar), the last two
    None without `partials`."""
    import numpy as np

    lib = load()
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    var = np.ascontiguousarray(var, dtype=np.float64).ravel()
    if mu.size != var.size:
        raise ValueError("mu and var differ in length")
    p = np.ascontiguousarray(list(params) + [0.0, 0.0], dtype=np.float64)
    out = [np.empty(mu.size) for _ in range(3 if partials else 1)]
    ptr = lambda a: a.ctypes.data_as(_dp)   # noqa: E731
    check(lib.bohip_acq_eval(ACQ[acq], ptr(p), mu.size, ptr(mu), ptr(var), ptr(out[0]), ptr(out[1]) if partials else None,
                             ptr(out[2]) if partials else None))
    return (out[0], out[1], out[2]) if partials else (out[0], None, None)


def check(rc):
    if rc == OK:
        return
    msg = load().bohip_last_error().decode()
    if rc == E_NOTPD:
        raise NotPositiveDefinite(rc, msg)
    raise BohipError(rc, msg)
