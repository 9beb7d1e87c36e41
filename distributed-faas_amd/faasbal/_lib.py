"""ctypes binding of libfaasbal.so (C ABI in include/faasbal.h).

There is no CPU fallback: if the HIP library is missing or no GPU is visible,
loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfaasbal.so")

FB_EV_REGISTER, FB_EV_RECONNECT, FB_EV_HEARTBEAT, FB_EV_RESULT, FB_EV_OTHER, FB_EV_LEAVE = 0, 1, 2, 3, 4, 5
FB_EV_DRAIN = 7  # (6 is unassigned); val != 0 drains, val == 0 resumes
# a draining record is marked in its free count (include/faasbal.h): draining iff free < FB_DRAIN_BELOW,
# true free count = free + FB_DRAIN_BIAS
FB_DRAIN_BIAS, FB_DRAIN_BELOW = 1 << 30, -(1 << 29)
FB_EVS_APPLIED, FB_EVS_RECONNECT, FB_EVS_UNKNOWN = 0, 1, 2
FB_OK, FB_EINVAL, FB_ENOMEM, FB_EHIP, FB_ERANGE, FB_ENOSPC, FB_ESTATE, FB_ERERUN = 0, -1, -2, -3, -4, -5, -6, -7
ERRNAMES = {FB_EINVAL: "FB_EINVAL", FB_ENOMEM: "FB_ENOMEM", FB_EHIP: "FB_EHIP", FB_ERANGE: "FB_ERANGE",
            FB_ENOSPC: "FB_ENOSPC", FB_ESTATE: "FB_ESTATE", FB_ERERUN: "FB_ERERUN"}

# Every symbol include/faasbal.h declares (checked by tests/test_abi.py).
EXPORTS = ("fb_create", "fb_destroy", "fb_last_error", "fb_load_state", "fb_read_state", "fb_tick_launch",
           "fb_tick_wait", "fb_tick_commit", "fb_get_assignments", "fb_get_orphans", "fb_get_evicted",
           "fb_get_event_status", "fb_tick", "fb_device_view_get", "fb_timing_enable", "fb_timing_read",
           "fb_selftest", "fb_debug_read", "fb_sync", "fb_set_stream", "fb_get_local_assignments",
           "fb_create_sharded", "fb_load_shard", "fb_read_shard_log", "fb_exchange_bytes", "fb_bind_exchange",
           "fb_tick_continue", "fb_create_deque", "fb_tick_stage", "fb_tick_launch_staged", "fb_host_alloc",
           "fb_host_free", "fb_purge_launch", "fb_apply_events", "fb_purge", "fb_assign", "fb_get_outputs",
           "fb_read_inflight", "fb_set_compact", "fb_get_outputs_compact", "fb_expand_compact",
           "fb_set_window", "fb_window_stats", "fb_set_compact_out", "fb_set_eager_commit", "fb_set_path",
           "fb_set_round_hint", "fb_set_full_assign", "fb_timing_gate", "fb_timing_span",
           "fb_timing_mark", "fb_log_compact", "fb_pool_stats", "fb_pool_stats_shard", "fb_pool_merge",
           "fb_log_compact_shard_bytes", "fb_log_compact_shard_mark", "fb_log_compact_shard_apply",
           "fb_log_compact_shard_cancel", "fb_log_reclaim", "fb_log_reclaim_shard")


class TickResult(C.Structure):
    _fields_ = [("n_assigned", C.c_int64), ("n_orphans", C.c_int64), ("queue_len", C.c_int64),
                ("log_head", C.c_int64), ("n_evicted", C.c_int32), ("fill_level", C.c_int32),
                ("max_free", C.c_int32), ("reruns", C.c_int32), ("n_local", C.c_int64),
                ("n_orphans_local", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


PS_FREE_BINS, PS_MAX_EDGES = 33, 15  # FB_PS_FREE_BINS, FB_PS_MAX_EDGES


class PoolSummary(C.Structure):
    """fb_pool_summary."""
    _fields_ = [(k, C.c_int64) for k in ("n_slots", "n_registered", "n_expired", "n_queued", "n_queued_expired",
                                          "dispatchable", "free_total", "log_head", "inflight",
                                          "inflight_expired", "inflight_max")] + \
               [("oldest_hb", C.c_double), ("newest_hb", C.c_double),
                ("free_hist", C.c_int64 * PS_FREE_BINS), ("age_hist", C.c_int64 * (PS_MAX_EDGES + 1))]


class DeviceView(C.Structure):
    _fields_ = [("free_processes", C.c_void_p), ("last_heartbeat", C.c_void_p), ("registered", C.c_void_p),
                ("queue", C.c_void_p), ("log_slot", C.c_void_p), ("orphans", C.c_void_p),
                ("evicted", C.c_void_p), ("n_workers", C.c_int32), ("queue_len", C.c_int64),
                ("log_head", C.c_int64), ("last_heartbeat_stride", C.c_int32),
                ("free_processes_stride", C.c_int32)]


class FaasbalError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERRNAMES.get(code, code), msg))
        self.code = code


_LIB = None
_P = C.c_void_p


def load(path=None):
    """Load and prototype libfaasbal.so.  Raises if it has not been built.
    FAASBAL_LIB overrides the default path (A/B of two builds of the library)."""
    global _LIB
    if path is None:
        path = os.environ.get("FAASBAL_LIB") or LIB_PATH
    if _LIB is not None and path == _LIB._name:
        return _LIB
    if not os.path.exists(path):
        raise ImportError("libfaasbal.so not found at %s: run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950)" % path)
    # torch bundles its own HIP runtime under the same soname as /opt/rocm's.
    # Whichever loads first serves the whole process; when this library came
    # first, a later `import torch` (faasbal.sharded's exchange buffers) found no
    # GPU on the box.  Processes that use torch import it first (faasbal.sharded,
    # bench.py's ranks, tests/conftest.py) or set FAASBAL_TORCH=1; the one-GPU
    # dispatcher and gateway never pay torch's import and bind /opt/rocm's runtime.
    if "torch" not in sys.modules and os.environ.get("FAASBAL_TORCH") == "1":
        try:
            import torch  # noqa: F401
        except Exception:  # a torch that fails to load must not stop the library
            pass
    lib = C.CDLL(path)
    i32, i64, dbl = C.c_int32, C.c_int64, C.c_double
    proto = {
        "fb_create": (C.c_int, [C.POINTER(_P), i32, i64, i32, C.c_int]),
        "fb_destroy": (C.c_int, [_P]),
        "fb_last_error": (C.c_char_p, [_P]),
        "fb_load_state": (C.c_int, [_P, i32, _P, _P, _P, _P, _P, i64, _P, i64]),
        "fb_read_state": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
        "fb_tick_launch": (C.c_int, [_P, dbl, dbl, i32, _P, _P, _P, _P, _P, i64]),
        "fb_tick_wait": (C.c_int, [_P, C.POINTER(TickResult)]),
        "fb_tick_commit": (C.c_int, [_P]),
        "fb_get_assignments": (C.c_int, [_P, i64, i64, _P]),
        "fb_get_orphans": (C.c_int, [_P, i64, _P]),
        "fb_get_evicted": (C.c_int, [_P, i32, _P]),
        "fb_get_event_status": (C.c_int, [_P, i32, _P]),
        "fb_tick": (C.c_int, [_P, dbl, dbl, i32, _P, _P, _P, _P, _P, i64, C.POINTER(TickResult),
                              _P, _P, _P, _P]),
        "fb_apply_events": (C.c_int, [_P, dbl, i32, _P, _P, _P, _P, _P, C.POINTER(TickResult), _P, _P, _P]),
        "fb_purge": (C.c_int, [_P, dbl, dbl, C.POINTER(TickResult), _P, _P]),
        "fb_get_outputs": (C.c_int, [_P, _P, _P, _P]),
        "fb_assign": (C.c_int, [_P, dbl, dbl, i64, C.POINTER(TickResult), _P, _P, _P]),
        "fb_device_view_get": (C.c_int, [_P, C.POINTER(DeviceView)]),
        "fb_timing_enable": (C.c_int, [_P, C.c_int]),
        "fb_timing_read": (C.c_int, [_P, i32, C.POINTER(C.c_char_p), C.POINTER(dbl), C.POINTER(i64),
                                     C.POINTER(i32)]),
        "fb_timing_gate": (C.c_int, [_P, C.c_int]),
        "fb_timing_mark": (C.c_int, [_P]),
        "fb_timing_span": (C.c_int, [_P, C.POINTER(dbl), C.POINTER(i32)]),
        "fb_debug_read": (C.c_int, [_P, _P, i64, C.POINTER(i64)]),
        "fb_selftest": (C.c_int, [_P, C.POINTER(i32)]),
        "fb_sync": (C.c_int, [_P]),
        "fb_set_stream": (C.c_int, [_P, _P]),
        "fb_get_local_assignments": (C.c_int, [_P, i64, i64, _P, _P]),
        "fb_create_sharded": (C.c_int, [C.POINTER(_P), i32, i32, i64, i32, C.c_int, i32, i32]),
        "fb_load_shard": (C.c_int, [_P, i32, i32, _P, _P, _P, _P, _P, i64, _P, _P, i64, i64]),
        "fb_read_shard_log": (C.c_int, [_P, _P, C.POINTER(i64), C.POINTER(i64)]),
        "fb_exchange_bytes": (C.c_int, [_P, i32, C.POINTER(i64)]),
        "fb_bind_exchange": (C.c_int, [_P, _P, i64]),
        "fb_tick_continue": (C.c_int, [_P]),
        "fb_create_deque": (C.c_int, [C.POINTER(_P), i32, i64, i64, i32, C.c_int]),
        "fb_tick_stage": (C.c_int, [_P, dbl, i32, _P, _P, _P, _P, _P]),
        "fb_tick_launch_staged": (C.c_int, [_P, dbl, i64]),
        "fb_host_alloc": (C.c_int, [_P, i64, C.POINTER(_P)]),
        "fb_host_free": (C.c_int, [_P, _P]),
        "fb_purge_launch": (C.c_int, [_P, dbl, dbl]),
        "fb_read_inflight": (C.c_int, [_P, _P]),
        "fb_log_compact": (C.c_int, [_P, i64, _P, i64, C.POINTER(i64)]),
        "fb_log_compact_shard_bytes": (C.c_int, [_P, C.POINTER(i64)]),
        "fb_log_compact_shard_mark": (C.c_int, [_P, _P, i64, C.POINTER(i64)]),
        "fb_log_compact_shard_apply": (C.c_int, [_P, i64, _P, i64, C.POINTER(i64)]),
        "fb_log_compact_shard_cancel": (C.c_int, [_P]),
        "fb_log_reclaim": (C.c_int, [_P, i64, _P, _P, _P, i64, C.POINTER(i64)]),
        "fb_log_reclaim_shard": (C.c_int, [_P, i64, _P, _P, _P, i64, C.POINTER(i64)]),
        "fb_pool_stats": (C.c_int, [_P, dbl, dbl, _P, C.c_int32, C.POINTER(PoolSummary)]),
        "fb_pool_stats_shard": (C.c_int, [_P, dbl, dbl, _P, C.c_int32, C.POINTER(PoolSummary), C.POINTER(i64)]),
        "fb_pool_merge": (C.c_int, [_P, C.POINTER(PoolSummary), C.POINTER(i64), C.c_int32, C.POINTER(PoolSummary)]),
        "fb_set_compact": (C.c_int, [_P, C.c_int]),
        "fb_set_window": (C.c_int, [_P, C.c_int]),
        "fb_set_eager_commit": (C.c_int, [_P, C.c_int]),
        "fb_set_compact_out": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64]),
        "fb_window_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "fb_get_outputs_compact": (C.c_int, [_P, _P, _P, i64, C.POINTER(i64), _P, _P]),
        "fb_expand_compact": (C.c_int, [_P, _P, _P, i64, _P]),
        "fb_set_path": (C.c_int, [_P, C.c_char_p, C.c_int]),
        "fb_set_round_hint": (C.c_int, [_P, C.c_int32]),
        "fb_set_full_assign": (C.c_int, [_P, C.c_int]),
    }
    for name, (res, args) in proto.items():
        fn = getattr(lib, name, None)
        if fn is None:  # an older build given by FAASBAL_LIB (A/B runs); the ABI test checks the real one
            continue
        fn.restype = res
        fn.argtypes = args
    if _LIB is None:
        _LIB = lib
    return lib
