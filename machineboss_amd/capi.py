"""ctypes binding of the C-ABI in include/mbhip.h (libmbhip.so, built in-tree by machineboss_amd.build).

This is the stub a Python caller of the reference (python/machineboss/boss.py shells out to the ``boss`` CLI) would
use instead.  There is no CPU fallback: every compute entry point raises if the HIP library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MBHIP_LIBRARY") or os.path.join(HERE, "libmbhip.so")      # (MBHIP_LIBRARY: another build of the same library, e.g. the sanitizer build of scripts/asan_planner.sh)

MB_FORWARD, MB_VITERBI, MB_BACKWARD = 0, 1, 2
MB_MATERIALISE, MB_ROLLING = 0, 1
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_SMALL, KERNEL_MEDIUM = 0, 1, 2, 3

EXPORTS = [
    "mb_device_count", "mb_set_device", "mb_synchronize", "mb_last_error", "mb_last_device_ms", "mb_last_kernel_name", "mb_last_launch_count",
    "mb_machine_create", "mb_machine_set_weights", "mb_machine_destroy", "mb_machine_n_states", "mb_machine_n_trans",
    "mb_machine_n_levels", "mb_machine_edge_order",
    "mb_batch_create", "mb_batch_destroy", "mb_batch_cells", "mb_batch_forward", "mb_viterbi_path_bound",
    "mb_batch_viterbi", "mb_batch_counts", "mb_fill", "mb_forward_batch", "mb_viterbi_batch", "mb_counts_batch",
    "mb_set_kernel", "mb_set_memory_budget", "mb_memory_budget", "mb_release_workspace", "mb_debug_jit_source", "mb_debug_persist_plan", "mb_debug_small_source", "mb_debug_wide_retimed", "mb_debug_wide_parts", "mb_debug_wide_jit",
    "mb_jit_stats", "mb_alloc_stats", "mb_machine_sweep_ops", "mb_set_option", "mb_get_option", "mb_log_sum_exp", "mb_log_sum_exp_n", "mb_log_inner_product",
    "mb_batch_set_envelopes", "mb_fill_env",
    "mb_comm_unique_id", "mb_comm_init", "mb_comm_destroy", "mb_allreduce_counts",
    "mb_profiles_create", "mb_profiles_destroy", "mb_profiles_forward", "mb_profile_path_bound", "mb_profiles_viterbi",
    "mb_profiles_counts", "mb_profile_fill", "mb_profiles_create_merged", "mb_profile_fill_merged",
    "mb_profiles_row_posteriors", "mb_profiles_set_rows",
    "mb_profile_pairs_create", "mb_profile_pairs_destroy", "mb_profile_pairs_forward", "mb_profile_pair_path_bound",
    "mb_profile_pairs_viterbi", "mb_profile_pairs_counts", "mb_profile_pair_fill",
    "mb_profile_pairs_create_merged", "mb_profile_pair_fill_merged",
    "mb_profile_pairs_set_envelopes", "mb_profile_pair_fill_env", "mb_profile_pairs_cells",
    "mb_profile_pairs_row_posteriors", "mb_profile_pairs_set_rows", "mb_profile_pairs_sample",
    "mb_profile_pairs_row_posteriors_merged", "mb_profile_pairs_set_rows_merged",
    "mb_profile_pairs_set_envelopes_merged", "mb_profile_pair_fill_merged_env", "mb_profile_pairs_sample_merged",
    "mb_profile_twos_create", "mb_profile_twos_destroy", "mb_profile_twos_forward", "mb_profile_twos_viterbi", "mb_profile_twos_counts",
    "mb_profile_twos_row_posteriors", "mb_profile_twos_set_rows",
    "mb_profile_two_fill",
    "mb_profile_twos_set_envelopes", "mb_profile_two_fill_env", "mb_profile_twos_cells", "mb_profile_twos_sample",
    "mb_profile_twos_set_envelopes_merged", "mb_profile_two_fill_merged_env",
    "mb_profile_twos_create_merged", "mb_profile_two_fill_merged", "mb_profile_twos_row_posteriors_merged",
    "mb_prefix_create", "mb_prefix_destroy", "mb_prefix_root", "mb_prefix_extend", "mb_prefix_release", "mb_prefix_free_nodes",
    "mb_prefix_node_cells", "mb_prefix_create_profiles", "mb_prefix_create_merged",
]

_lib = None


class MbError(RuntimeError):
    """The library's non-zero status, carrying mb_last_error() -- the reference throws runtime_error (src/util.cpp:39-48)."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MbError("libmbhip.so is not built (run `python -m machineboss_amd.build`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    i32p, i64p, u32p, u16p, dp = (C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint16), C.POINTER(C.c_double))
    L.mb_device_count.restype = C.c_int
    L.mb_set_device.argtypes = [C.c_int]
    L.mb_last_error.restype = C.c_char_p
    L.mb_last_device_ms.restype = C.c_double
    L.mb_last_kernel_name.restype = C.c_char_p
    L.mb_last_launch_count.restype = C.c_int64
    L.mb_machine_create.restype = vp
    L.mb_machine_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp]
    L.mb_machine_set_weights.argtypes = [vp, dp]
    L.mb_machine_destroy.argtypes = [vp]
    L.mb_machine_destroy.restype = None
    L.mb_machine_n_states.argtypes = [vp]; L.mb_machine_n_states.restype = C.c_int32
    L.mb_machine_n_trans.argtypes = [vp]; L.mb_machine_n_trans.restype = C.c_int64
    L.mb_machine_n_levels.argtypes = [vp]; L.mb_machine_n_levels.restype = C.c_int32
    L.mb_machine_edge_order.argtypes = [vp, C.c_int, u32p]
    L.mb_batch_create.restype = vp
    L.mb_batch_create.argtypes = [vp, C.c_int64, i32p, i64p, i32p, i64p]
    L.mb_batch_destroy.argtypes = [vp]; L.mb_batch_destroy.restype = None
    L.mb_batch_cells.argtypes = [vp]; L.mb_batch_cells.restype = C.c_int64
    L.mb_batch_forward.argtypes = [vp, C.c_int, dp]
    L.mb_viterbi_path_bound.argtypes = [vp, C.c_int64, C.c_int64]; L.mb_viterbi_path_bound.restype = C.c_int64
    L.mb_batch_viterbi.argtypes = [vp, dp, i64p, u32p, C.c_int64]
    L.mb_batch_counts.argtypes = [vp, dp, dp, dp]
    L.mb_fill.argtypes = [vp, C.c_int, i32p, C.c_int64, i32p, C.c_int64, C.c_int32, dp]
    L.mb_forward_batch.argtypes = [vp, C.c_int64, i32p, i64p, i32p, i64p, C.c_int, dp]
    L.mb_viterbi_batch.argtypes = [vp, C.c_int64, i32p, i64p, i32p, i64p, dp, i64p, u32p, C.c_int64]
    L.mb_counts_batch.argtypes = [vp, C.c_int64, i32p, i64p, i32p, i64p, dp, dp, dp]
    L.mb_set_kernel.argtypes = [C.c_int]
    L.mb_set_memory_budget.argtypes = [C.c_size_t]
    L.mb_memory_budget.restype = C.c_size_t
    L.mb_batch_set_envelopes.argtypes = [vp, i64p, i32p, i32p]
    L.mb_fill_env.argtypes = [vp, C.c_int, i32p, C.c_int64, i32p, C.c_int64, C.c_int32, i32p, i32p, dp]
    L.mb_debug_jit_source.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.mb_debug_small_source.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp,
                                        C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.mb_debug_wide_retimed.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp,
                                        C.c_int, C.c_int, C.c_char_p]
    L.mb_debug_wide_parts.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.mb_debug_wide_jit.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, u32p, u32p, u16p, u16p, dp,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.mb_log_sum_exp.argtypes = [C.c_double, C.c_double]; L.mb_log_sum_exp.restype = C.c_double
    L.mb_log_sum_exp_n.argtypes = [dp, C.c_size_t]; L.mb_log_sum_exp_n.restype = C.c_double
    L.mb_log_inner_product.argtypes = [dp, dp, dp, C.c_size_t]; L.mb_log_inner_product.restype = C.c_double
    L.mb_jit_stats.argtypes = [dp, i64p, i64p]
    L.mb_alloc_stats.argtypes = [i64p, i64p, i64p, C.POINTER(C.c_uint64), dp]
    L.mb_machine_sweep_ops.argtypes = [C.c_void_p, dp, dp, C.POINTER(C.c_char_p)]
    L.mb_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.mb_get_option.argtypes = [C.c_char_p]; L.mb_get_option.restype = C.c_char_p
    L.mb_comm_unique_id.argtypes = [C.c_char_p]
    L.mb_comm_init.argtypes = [C.c_char_p, C.c_int, C.c_int]; L.mb_comm_init.restype = vp
    L.mb_comm_destroy.argtypes = [vp]; L.mb_comm_destroy.restype = None
    L.mb_allreduce_counts.argtypes = [vp, dp, C.c_size_t, dp]
    L.mb_profiles_create.restype = vp
    L.mb_profiles_create.argtypes = [vp, C.c_int64, dp, i64p]
    L.mb_profiles_destroy.argtypes = [vp]; L.mb_profiles_destroy.restype = None
    L.mb_profiles_forward.argtypes = [vp, C.c_int, dp]
    L.mb_profile_path_bound.argtypes = [vp, C.c_int64]; L.mb_profile_path_bound.restype = C.c_int64
    L.mb_profiles_viterbi.argtypes = [vp, dp, i64p, u32p, i32p, C.c_int64]
    L.mb_profiles_counts.argtypes = [vp, dp, dp, dp]
    L.mb_profile_fill.argtypes = [vp, C.c_int, dp, C.c_int64, dp]
    L.mb_profiles_create_merged.restype = vp
    L.mb_profiles_create_merged.argtypes = [vp, C.c_int64, dp, i64p, C.c_int32, i32p]
    L.mb_profile_fill_merged.argtypes = [vp, C.c_int, dp, C.c_int64, C.c_int32, i32p, dp]
    L.mb_profiles_row_posteriors.argtypes = [vp, dp, dp]
    L.mb_profiles_set_rows.argtypes = [vp, dp]
    L.mb_profile_pairs_create.restype = vp
    L.mb_profile_pairs_create.argtypes = [vp, C.c_int64, i32p, i64p, dp, i64p]
    L.mb_profile_pairs_destroy.argtypes = [vp]; L.mb_profile_pairs_destroy.restype = None
    L.mb_profile_pairs_forward.argtypes = [vp, C.c_int, dp]
    L.mb_profile_pair_path_bound.argtypes = [vp, C.c_int64, C.c_int64]; L.mb_profile_pair_path_bound.restype = C.c_int64
    L.mb_profile_pairs_viterbi.argtypes = [vp, dp, i64p, u32p, i32p, C.c_int64]
    L.mb_profile_pairs_counts.argtypes = [vp, dp, dp, dp]
    L.mb_profile_pair_fill.argtypes = [vp, C.c_int, i32p, C.c_int64, dp, C.c_int64, dp]
    L.mb_profile_pairs_create_merged.restype = vp
    L.mb_profile_pairs_create_merged.argtypes = [vp, C.c_int64, i32p, i64p, dp, i64p, C.c_int32, i32p]
    L.mb_profile_pair_fill_merged.argtypes = [vp, C.c_int, i32p, C.c_int64, dp, C.c_int64, C.c_int32, i32p, dp]
    L.mb_profile_pairs_set_envelopes.argtypes = [vp, i64p, i32p, i32p]
    L.mb_profile_pair_fill_env.argtypes = [vp, C.c_int, i32p, C.c_int64, dp, C.c_int64, i32p, i32p, dp]
    L.mb_profile_pairs_cells.argtypes = [vp]; L.mb_profile_pairs_cells.restype = C.c_int64
    L.mb_profile_pairs_row_posteriors.argtypes = [vp, dp, dp]
    L.mb_profile_pairs_set_rows.argtypes = [vp, dp]
    L.mb_profile_pairs_sample.argtypes = [vp, C.c_int64, C.c_uint64, dp, i64p, u32p, i32p, dp, C.c_int64]
    L.mb_profile_pairs_sample_merged.argtypes = [vp, C.c_int64, C.c_uint64, dp, i64p, u32p, i32p, i32p, dp, C.c_int64]
    L.mb_profile_pairs_row_posteriors_merged.argtypes = [vp, dp, dp]
    L.mb_profile_pairs_set_rows_merged.argtypes = [vp, dp]
    L.mb_profile_pairs_set_envelopes_merged.argtypes = [vp, i64p, i32p, i32p]
    L.mb_profile_pair_fill_merged_env.argtypes = [vp, C.c_int, i32p, C.c_int64, dp, C.c_int64, C.c_int32, i32p, i32p, i32p, dp]
    L.mb_profile_twos_create.restype = vp
    L.mb_profile_twos_create.argtypes = [vp, C.c_int64, dp, i64p, dp, i64p]
    L.mb_profile_twos_destroy.argtypes = [vp]; L.mb_profile_twos_destroy.restype = None
    L.mb_profile_twos_forward.argtypes = [vp, C.c_int, dp]
    L.mb_profile_twos_viterbi.argtypes = [vp, dp, i64p, u32p, i32p, i32p, C.c_int64]
    L.mb_profile_twos_sample.argtypes = [vp, C.c_int64, C.c_uint64, dp, i64p, u32p, i32p, i32p, dp, C.c_int64]
    L.mb_profile_twos_counts.argtypes = [vp, dp, dp, dp]
    L.mb_profile_twos_row_posteriors.argtypes = [vp, dp, dp, dp]
    L.mb_profile_twos_row_posteriors_merged.argtypes = [vp, dp, dp, dp]
    L.mb_profile_twos_set_rows.argtypes = [vp, dp, dp]
    L.mb_profile_two_fill.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, dp]
    L.mb_profile_twos_set_envelopes.argtypes = [vp, i64p, i32p, i32p]
    L.mb_profile_two_fill_env.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, i32p, i32p, dp]
    L.mb_profile_twos_set_envelopes_merged.argtypes = [vp, i64p, i32p, i32p]
    L.mb_profile_two_fill_merged_env.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int32, i32p, i32p, i32p, dp]
    L.mb_profile_twos_cells.argtypes = [vp]; L.mb_profile_twos_cells.restype = C.c_int64
    L.mb_profile_twos_create_merged.restype = vp
    L.mb_profile_twos_create_merged.argtypes = [vp, C.c_int64, dp, i64p, dp, i64p, C.c_int32, i32p]
    L.mb_profile_two_fill_merged.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int32, i32p, dp]
    L.mb_prefix_create.restype = vp
    L.mb_prefix_create.argtypes = [vp, C.c_int64, i32p, i64p, dp, C.c_int64]
    L.mb_prefix_create_profiles.restype = vp
    L.mb_prefix_create_profiles.argtypes = [vp, C.c_int64, dp, i64p, dp, C.c_int64]
    L.mb_prefix_create_merged.restype = vp
    L.mb_prefix_create_merged.argtypes = [vp, C.c_int64, dp, i64p, C.c_int32, i32p, dp, C.c_int64]
    L.mb_prefix_destroy.argtypes = [vp]; L.mb_prefix_destroy.restype = None
    L.mb_prefix_root.argtypes = [vp, C.c_int64, i64p, dp, dp]
    L.mb_prefix_extend.argtypes = [vp, C.c_int64, i64p, i64p, i32p, i64p, dp, dp]
    L.mb_prefix_release.argtypes = [vp, C.c_int64, i64p]
    L.mb_prefix_free_nodes.argtypes = [vp]; L.mb_prefix_free_nodes.restype = C.c_int64
    L.mb_prefix_node_cells.argtypes = [vp, C.c_int64, dp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MbError(load().mb_last_error().decode() or "mbhip error")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def device_count() -> int:
    return load().mb_device_count()


def set_device(d: int):
    _check(load().mb_set_device(d))


def set_kernel(which: int):
    _check(load().mb_set_kernel(which))


def set_memory_budget(nbytes: int):
    _check(load().mb_set_memory_budget(nbytes))


def memory_budget() -> int:
    """Bytes the pools of one call may take now (the explicit budget, else a share of the device)."""
    return int(load().mb_memory_budget())


def release_workspace():
    _check(load().mb_release_workspace())


def jit_stats() -> dict:
    """hiprtc work done by this process: compile wall time, number of compiles, code objects served by the disk cache."""
    ms = C.c_double(0.0); n = C.c_int64(0); h = C.c_int64(0)
    _check(load().mb_jit_stats(C.byref(ms), C.byref(n), C.byref(h)))
    return {"compile_ms": round(ms.value, 1), "compiles": n.value, "cache_hits": h.value}


def alloc_stats() -> dict:
    """Device allocations the matrix pools cost this process so far (steady-state calls do none)."""
    a = C.c_int64(0); f = C.c_int64(0); e = C.c_int64(0); b = C.c_uint64(0); ms = C.c_double(0.0)
    _check(load().mb_alloc_stats(C.byref(a), C.byref(f), C.byref(e), C.byref(b), C.byref(ms)))
    return {"pool_allocs": a.value, "pool_frees": f.value, "evictions": e.value, "bytes_allocated": b.value, "ms": round(ms.value, 2)}


def sweep_ops(dm) -> dict:
    """v_exp_f32 / v_log_f32 per lattice cell of the machine's log-sum-exp Forward sweep, and the kernel family that runs it."""
    e = C.c_double(0.0); l = C.c_double(0.0); f = C.c_char_p()
    _check(load().mb_machine_sweep_ops(dm.h, C.byref(e), C.byref(l), C.byref(f)))
    return {"exp_per_cell": e.value, "log_per_cell": l.value, "family": (f.value or b"").decode()}


def set_option(name: str, value=None):
    _check(load().mb_set_option(name.encode(), None if value is None else str(value).encode()))


def options() -> dict:
    """The library's option table (mb_get_option(NULL)): name -> {kind, default, class, note}."""
    rows = (line.split("\t") for line in load().mb_get_option(None).decode().splitlines())
    return {r[0]: {"kind": r[1], "default": r[2], "class": r[3], "note": r[4]} for r in rows}


def last_device_ms() -> float:
    return load().mb_last_device_ms()


def last_launch_count() -> int:
    return load().mb_last_launch_count()


def last_kernel_name() -> str:
    return load().mb_last_kernel_name().decode()


def synchronize():
    """Wait for everything the library queued on its device (the timing bracket of a multi-rank host)."""
    _check(load().mb_synchronize())


class Comm:
    """RCCL communicator of the C-ABI (mb_comm*) on the library's own HIP runtime and stream: what a C++ host uses, and what
    shard.RankGroup opens for the Python hosts (bench.py, boss.py)."""

    def __init__(self, unique_id: bytes, nRanks: int, rank: int):
        self.h = load().mb_comm_init(unique_id, nRanks, rank)
        if not self.h:
            raise MbError(load().mb_last_error().decode())

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load().mb_comm_unique_id(buf))
        return buf.raw

    def allreduce_counts(self, counts: np.ndarray, loglike: float):
        assert counts.dtype == np.float64 and counts.flags.c_contiguous
        ll = C.c_double(loglike)
        _check(load().mb_allreduce_counts(self.h, _p(counts, C.c_double), counts.size, C.byref(ll)))
        return counts, ll.value

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mb_comm_destroy(self.h)
            self.h = None


def debug_jit_source(em, path: str, mode: int = MB_FORWARD, backward: bool = False, closure: int = 1, G: int = 2):
    """Write the HIP source of the run-time specialised tile kernel for this machine (host only, no GPU needed).
    closure: 0 = levelled program, K >= 1 = silent closure in K stages."""
    a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
         np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
         np.ascontiguousarray(em.logWeight, np.float64)]
    _check(load().mb_debug_jit_source(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                      _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double),
                                      mode, int(backward), int(closure), G, path.encode()))


def debug_medium_program(em, path: str, mode: int = MB_FORWARD, backward: bool = False, closure: int = 1, G: int = 2) -> dict:
    """The tiled family's PROGRAM for this machine as the kernels read it (host only, no GPU needed): chunk descriptors `desc`
    [nChunks][8], records `rec` (w, srcOff, dstOff), the usage slots `flat` [(table, first record)] of a flat count program, and
    the scalars S, Spad, LPG, G, nIn, nOut, seedOff, dummyOff, backward, closure, counting, flatCount, fusedEmit, twoTables, the fused emit slots
    `fused` and the loop-time accumulator map `accMap` of a flat count program (mb_api.hip,
    mb_debug_jit_source with mode + 32; the semantics are med_slow_supercell's, mb_medium.hip)."""
    debug_jit_source(em, path, mode=mode | 32, backward=backward, closure=closure, G=G)
    head = np.fromfile(path, np.int32, 16)
    assert head[0] == 0x4D454431
    keys = ("S", "Spad", "LPG", "G", "nChunks", "nIn", "nOut", "seedOff", "dummyOff", "nRec", "nFlat", "backward", "closure", "counting", "flatCount")
    out = {k: int(v) for k, v in zip(keys, head[1:])}
    off = 64
    out["desc"] = np.fromfile(path, np.int32, out["nChunks"] * 8, offset=off).reshape(out["nChunks"], 8); off += out["nChunks"] * 32
    out["rec"] = np.fromfile(path, np.dtype([("w", "<f8"), ("srcOff", "<u4"), ("dstOff", "<u4")]), out["nRec"], offset=off); off += out["nRec"] * 16
    flags = out["flatCount"]
    out["flatCount"], out["fusedEmit"], out["twoTables"] = flags & 1, (flags >> 1) & 1, (flags >> 2) & 1
    out["flat"] = np.fromfile(path, np.int32, out["nFlat"] * 3, offset=off).reshape(out["nFlat"], 3); off += out["nFlat"] * 12      # (table, first record, placement: 2 = VGPRs)
    out["wref"] = np.fromfile(path, np.int32, out["nRec"], offset=off); off += out["nRec"] * 4      # per record: >= 0 its transition, -1 padding, <= -2 a closure pair
    nFused, nLoop = (int(v) for v in np.fromfile(path, np.int32, 2, offset=off)); off += 8
    out["fused"] = np.fromfile(path, np.int32, nFused * 3, offset=off).reshape(nFused, 3); off += nFused * 12                        # emit slots of the fill rounds that also add usage
    out["accMap"] = np.fromfile(path, np.int32, nLoop, offset=off); off += nLoop * 4                                                  # loop-time accumulator entry -> transition
    assert os.path.getsize(path) == off
    return out


def debug_small_source(em, path: str, mode: int = 0, backward: bool = False, materialise: bool = True, envelopes: bool = False):
    """Write the HIP source of the small-machine family's sweep for this machine (host only, no GPU needed).
    mode: 0 sum, 1 max (fp64 cells), 2 max (traceback bytes), 3 Forward fused with posterior counts."""
    a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
         np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
         np.ascontiguousarray(em.logWeight, np.float64)]
    _check(load().mb_debug_small_source(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                        _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double),
                                        mode, int(backward), int(materialise) | (2 if envelopes else 0), path.encode()))


def debug_small_program(em, path: str, backward: bool = False) -> dict:
    """The small-machine family's PROGRAM for this machine (host only, no GPU needed; mb_debug_small_source with mode + 32): the
    evaluation order of the states, per state its candidates (T, src, dup, tab) in the reference's enumeration order (`decOff` [S + 1]
    delimits them), and the weight / edge-id tables `w`, `eid` with their layout (`off`, `nTab` by kind T: 0 match, 1 input-only,
    2 output-only, 3 silent)."""
    debug_small_source(em, path, mode=32, backward=backward)
    head = np.fromfile(path, np.int32, 20)
    assert head[0] == 0x534D5031
    out = {k: int(v) for k, v in zip(("S", "nIn", "nOut", "backward", "seedState", "endState", "nEntries"), head[1:8])}
    out["off"] = [int(v) for v in head[8:12]]; out["nTab"] = [int(v) for v in head[12:16]]
    nc, S, pos = int(head[16]), out["S"], 80
    out["order"] = np.fromfile(path, np.int32, S, offset=pos); pos += 4 * S
    out["decOff"] = np.fromfile(path, np.int32, S + 1, offset=pos); pos += 4 * (S + 1)
    out["cand"] = np.fromfile(path, np.int32, 4 * nc, offset=pos).reshape(nc, 4); pos += 16 * nc
    out["w"] = np.fromfile(path, np.float64, out["nEntries"], offset=pos); pos += 8 * out["nEntries"]
    out["eid"] = np.fromfile(path, np.int32, out["nEntries"], offset=pos); pos += 4 * out["nEntries"]
    assert os.path.getsize(path) == pos and out["decOff"][-1] == nc
    return out


def debug_wide_retimed(em, path: str, mode: int = MB_VITERBI, backward: bool = False, tb_codes: bool = False) -> dict:
    """The retimed program of a one-tape machine as the kernel reads it (host only, no GPU needed): the header fields and
    the record streams, one per rotation of the ring, as a structured array [stream][slot][lane] of (w, src, pad).
    tb_codes (forward max program only): the program that keeps one traceback code per cell, with its decode tables
    `tbOff` [S + 1], `tbEntry` (position in the incoming view << 16 | emitting << 15 | source state; 0xFFFFFFFF: the seed)
    and `inEid` (incoming view position -> global edge id)."""
    a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
         np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
         np.ascontiguousarray(em.logWeight, np.float64)]
    _check(load().mb_debug_wide_retimed(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                        _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double),
                                        mode | (16 if tb_codes else 0), int(backward), path.encode()))
    head = np.fromfile(path, np.int32, 12)
    assert head[0] == 0x52455431
    keys = ("lanes", "slots", "NB", "NVs", "kMax", "rowLen", "nPen", "period", "S", "inL2", "streams")
    out = {k: int(v) for k, v in zip(keys, head[1:])}
    nrec = (out["NB"] * out["slots"] + 8) * out["lanes"]
    rec = np.fromfile(path, np.dtype([("w", "<f8"), ("src", "<u4"), ("pad", "<u4")]), count=nrec, offset=48)
    assert rec.size == nrec
    out["records"] = rec[:out["NB"] * out["slots"] * out["lanes"]].reshape(out["NB"], out["slots"], out["lanes"])
    out["tail"] = rec[out["NB"] * out["slots"] * out["lanes"]:].reshape(8, out["lanes"])
    rest = np.fromfile(path, np.uint32, offset=48 + 16 * nrec)
    if tb_codes:
        pos = 0
        for k in ("tbOff", "tbEntry", "inEid"):
            n = int(rest[pos]); out[k] = rest[pos + 1:pos + 1 + n].copy(); pos += 1 + n
        assert pos == rest.size and out["tbOff"].size == em.nStates + 1 and out["inEid"].size == em.nTransitions
    else:
        assert rest.size == 0
    return out


def debug_wide_parts(em, path: str, k: int, lanes: int = 256, mode: int = MB_VITERBI, backward: bool = False, tb_codes: bool = False) -> dict:
    """The k-part form of the retimed program (k workgroups per sequence; host only): {"nExp": exchange columns, "S": states,
    "parts": [per part the fields of debug_wide_retimed + Sloc, nImp, expBase, expIdx0, nExp, resultEntry, gmap, impIdx]}; tb_codes:
    + the decode tables of the parts' candidate lists, joined over the machine's states (tbOff, tbEntry, inEid)."""
    a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
         np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
         np.ascontiguousarray(em.logWeight, np.float64)]
    _check(load().mb_debug_wide_parts(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                      _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double),
                                      mode | (16 if tb_codes else 0), int(backward), int(k), int(lanes), path.encode()))
    head = np.fromfile(path, np.int32, 4)
    assert head[0] == 0x52455432
    out = {"nExp": int(head[2]), "S": int(head[3]), "parts": []}
    pos = 16
    keys = ("lanes", "slots", "NB", "NVs", "kMax", "rowLen", "nPen", "period", "Sloc", "nImp", "expBase", "expIdx0", "nExp", "resultEntry", "nTab", "w2Offset")
    for _ in range(int(head[1])):
        ph = np.fromfile(path, np.int32, 16, offset=pos); pos += 64
        part = {k_: int(v) for k_, v in zip(keys, ph)}
        tab = np.fromfile(path, np.uint32, part["nTab"], offset=pos); pos += 4 * part["nTab"]
        part["gmap"], part["impIdx"] = tab[:part["Sloc"]].astype(np.int64), tab[part["Sloc"]:].astype(np.int64)
        assert part["impIdx"].size == part["nImp"]
        nrec = (part["NB"] * part["slots"] + 8) * part["lanes"]
        rec16 = np.fromfile(path, np.dtype([("w", "<f8"), ("src", "<u4"), ("pad", "<u4")]), count=nrec, offset=pos); pos += 16 * nrec
        rec = np.zeros(nrec, np.dtype([("w", "<f8"), ("src", "<u4"), ("pad", "<u4"), ("w2", "<f8")]))
        for f in ("w", "src", "pad"): rec[f] = rec16[f]
        if part["w2Offset"]:      # two-transition candidates: the second weights, one per record, behind the records
            assert part["w2Offset"] == 16 * nrec
            rec["w2"] = np.fromfile(path, "<f8", count=nrec, offset=pos); pos += 8 * nrec
        part["records"] = rec[:part["NB"] * part["slots"] * part["lanes"]].reshape(part["NB"], part["slots"], part["lanes"])
        part["inL2"] = 0
        out["parts"].append(part)
    if tb_codes:
        rest = np.fromfile(path, np.uint32, offset=pos); q = 0
        for k_ in ("tbOff", "tbEntry", "inEid"):
            n = int(rest[q]); out[k_] = rest[q + 1:q + 1 + n].copy(); q += 1 + n
        assert q == rest.size and out["tbOff"].size == em.nStates + 1 and out["inEid"].size == em.nTransitions
        pos += 4 * rest.size
    assert os.path.getsize(path) == pos
    return out


def debug_wide_jit(em, path: str, k: int = 1, lanes: int = 0, mode: int = MB_VITERBI, backward: bool = False, tb_codes: bool = False,
                   acc: bool = False, compile: bool = False) -> dict:
    """The one-tape sweep GENERATED for this machine (mb_wide_jit.cpp; host only): the HIP source goes to `path`, and what it unrolls
    comes back as {"nExp", "S", "parts": [{geometry ..., "slots": [(anyPen, anyW2)], "rounds": [{firstSlot, depth, sync, uniform, gAll,
    anyMixed, resultLane}], "fields": [(kind, index, cm, words)], "table": uint32 [words][lanes], "impIdx"}]} -- the per-lane constant
    table exactly as the kernel loads it.  compile: also through hiprtc (raises when the kernel would spill to scratch memory)."""
    a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
         np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
         np.ascontiguousarray(em.logWeight, np.float64)]
    _check(load().mb_debug_wide_jit(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                    _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double),
                                    mode | (16 if tb_codes else 0) | (64 if acc else 0), int(backward), int(k), int(lanes), int(compile), path.encode()))
    prog = path + ".prog"
    head = np.fromfile(prog, np.int32, 4)
    assert head[0] == 0x4A495431
    out = {"nExp": int(head[2]), "S": int(head[3]), "parts": []}
    pos = 16
    keys = ("lanes", "NB", "NVs", "kMax", "rowLen", "nPen", "nImp", "Sloc", "expBase", "nExp", "expIdx0", "resultEntry", "nSlots", "nRounds", "NPT", "U",
            "penBase", "tokBase", "ringBase", "dummyAddr", "ldsBytes", "nFields", "nWords", "pad")
    for _ in range(int(head[1])):
        ph = np.fromfile(prog, np.int32, 24, offset=pos); pos += 96
        part = {k_: int(v) for k_, v in zip(keys, ph)}
        sl = np.fromfile(prog, np.int32, 2 * part["nSlots"], offset=pos).reshape(-1, 2); pos += 8 * part["nSlots"]
        rd = np.fromfile(prog, np.int32, 8 * part["nRounds"], offset=pos).reshape(-1, 8); pos += 32 * part["nRounds"]
        fd = np.fromfile(prog, np.int32, 4 * part["nFields"], offset=pos).reshape(-1, 4); pos += 16 * part["nFields"]
        part["slots"] = [(bool(x[0]), bool(x[1])) for x in sl]
        part["rounds"] = [dict(firstSlot=int(x[0]), depth=int(x[1]), sync=bool(x[2]), uniform=bool(x[3]), gAll=int(x[4]), anyMixed=bool(x[5]), resultLane=int(x[6]), gMask=int(x[7])) for x in rd]
        part["fields"] = [tuple(int(v) for v in x) for x in fd]
        part["table"] = np.fromfile(prog, np.uint32, part["nWords"] * part["lanes"], offset=pos).reshape(part["nWords"], part["lanes"]); pos += 4 * part["nWords"] * part["lanes"]
        part["level"], part["IP"], part["ring"] = part["pad"] & 0xff, (part["pad"] >> 8) & 0xfff, part["pad"] >> 20
        if part["level"] >= 1:      # the packed address words of a streamed program: [rotation][item][lane]
            n = part["NB"] * part["IP"] * part["lanes"]
            part["stream"] = np.fromfile(prog, np.uint32, n, offset=pos).reshape(part["NB"], part["IP"], part["lanes"]); pos += 4 * n
        if len(out["parts"]) > 0 or int(head[1]) > 1:
            part["impIdx"] = np.fromfile(prog, np.uint32, part["nImp"], offset=pos).astype(np.int64); pos += 4 * part["nImp"]
        out["parts"].append(part)
    assert os.path.getsize(prog) == pos
    return out


class DeviceMachine:
    """Device-resident flattened machine (mb_machine*), built from an evalmachine.EvaluatedMachine."""

    def __init__(self, em):
        L = load()
        self.em = em
        a = [np.ascontiguousarray(em.src, np.uint32), np.ascontiguousarray(em.dst, np.uint32),
             np.ascontiguousarray(em.inTok, np.uint16), np.ascontiguousarray(em.outTok, np.uint16),
             np.ascontiguousarray(em.logWeight, np.float64)]
        self.h = L.mb_machine_create(em.nStates, em.nInTok, em.nOutTok, em.nTransitions, _p(a[0], C.c_uint32),
                                     _p(a[1], C.c_uint32), _p(a[2], C.c_uint16), _p(a[3], C.c_uint16), _p(a[4], C.c_double))
        if not self.h:
            raise MbError(L.mb_last_error().decode())
        self.nStates, self.nTrans = em.nStates, em.nTransitions

    def close(self):
        if getattr(self, "h", None) and _lib is not None:   # at interpreter shutdown the module globals may be gone
            try:
                _lib.mb_machine_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def set_weights(self, logWeight):
        lw = np.ascontiguousarray(logWeight, np.float64)
        assert lw.shape == (self.nTrans,)
        _check(load().mb_machine_set_weights(self.h, _p(lw, C.c_double)))

    def n_levels(self) -> int:
        return load().mb_machine_n_levels(self.h)

    def edge_order(self, which: int) -> np.ndarray:
        o = np.empty(self.nTrans, np.uint32)
        _check(load().mb_machine_edge_order(self.h, which, _p(o, C.c_uint32)))
        return o

    def fill(self, mode: int, inp, out, startState: int = 0, envStart=None, envEnd=None) -> np.ndarray:
        """Full matrix [outLen+1][inLen+1][nStates] (DPMatrix cell storage, src/dpmatrix.h:90-96); with an envelope
        (inStart[o], inEnd[o] per output position) the cells outside it are -inf."""
        i = np.ascontiguousarray(inp, np.int32); o = np.ascontiguousarray(out, np.int32)
        cells = np.empty((len(o) + 1, len(i) + 1, self.nStates), np.float64)
        es = None if envStart is None else np.ascontiguousarray(envStart, np.int32)
        ee = None if envEnd is None else np.ascontiguousarray(envEnd, np.int32)
        _check(load().mb_fill_env(self.h, mode, _p(i, C.c_int32), len(i), _p(o, C.c_int32), len(o), startState,
                                  _p(es, C.c_int32), _p(ee, C.c_int32), _p(cells, C.c_double)))
        return cells

    def path_bound(self, inLen: int, outLen: int) -> int:
        return load().mb_viterbi_path_bound(self.h, inLen, outLen)


class DeviceBatch:
    """Device-resident tokenised pair list (mb_batch*)."""

    def __init__(self, dm: DeviceMachine, inTok, inOff, outTok, outOff):
        self.dm = dm
        self.inTok = np.ascontiguousarray(inTok, np.int32); self.outTok = np.ascontiguousarray(outTok, np.int32)
        self.inOff = np.ascontiguousarray(inOff, np.int64); self.outOff = np.ascontiguousarray(outOff, np.int64)
        self.nPairs = len(self.inOff) - 1
        assert len(self.outOff) == self.nPairs + 1
        L = load()
        self.h = L.mb_batch_create(dm.h, self.nPairs, _p(self.inTok, C.c_int32), _p(self.inOff, C.c_int64),
                                   _p(self.outTok, C.c_int32), _p(self.outOff, C.c_int64))
        if not self.h:
            raise MbError(L.mb_last_error().decode())

    @classmethod
    def from_pairs(cls, dm: DeviceMachine, pairs):
        """pairs: iterable of (inputTokens, outputTokens)."""
        pairs = list(pairs)
        inOff = np.zeros(len(pairs) + 1, np.int64); outOff = np.zeros(len(pairs) + 1, np.int64)
        for k, (a, b) in enumerate(pairs):
            inOff[k + 1] = inOff[k] + len(a); outOff[k + 1] = outOff[k] + len(b)
        cat = lambda xs: (np.concatenate([np.asarray(x, np.int32) for x in xs]) if len(xs) else np.zeros(0, np.int32)).astype(np.int32)
        return cls(dm, cat([a for a, _ in pairs]), inOff, cat([b for _, b in pairs]), outOff)

    def set_envelopes(self, envs):
        """envs: per pair either None (full) or (inStart, inEnd) arrays of outLen+1 entries (src/seqpair.h:75-97)."""
        off = np.zeros(self.nPairs + 1, np.int64)
        st, en = [], []
        for k, e in enumerate(envs):
            n = 0
            if e is not None:
                st.append(np.asarray(e[0], np.int32)); en.append(np.asarray(e[1], np.int32)); n = len(st[-1])
            off[k + 1] = off[k] + n
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(1, np.int32), np.int32)
        a, b = cat(st), cat(en)
        _check(load().mb_batch_set_envelopes(self.h, _p(off, C.c_int64), _p(a, C.c_int32), _p(b, C.c_int32)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.mb_batch_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def cells(self) -> int:
        return load().mb_batch_cells(self.h)

    def forward(self, flags: int = MB_MATERIALISE) -> np.ndarray:
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_batch_forward(self.h, flags, _p(ll, C.c_double)))
        return ll

    def viterbi(self, paths: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        ll = np.empty(self.nPairs, np.float64)
        if not paths:
            _check(load().mb_batch_viterbi(self.h, _p(ll, C.c_double), None, None, 0))
            return ll, None, None
        # mb_viterbi_path_bound is linear in the lengths: (inLen + outLen + 1) * levels + 1 per pair
        per = self.dm.path_bound(1, 0) - self.dm.path_bound(0, 0)
        lens = np.diff(self.inOff) + np.diff(self.outOff)
        cap = int((lens + 1).sum() * per + self.nPairs) if self.nPairs else 0
        off = np.zeros(self.nPairs + 1, np.int64); edges = np.empty(max(cap, 1), np.uint32)   # worst case; only the used part is touched
        _check(load().mb_batch_viterbi(self.h, _p(ll, C.c_double), _p(off, C.c_int64), _p(edges, C.c_uint32), cap))
        return ll, off, edges[:off[-1]]

    def counts(self, counts: Optional[np.ndarray] = None):
        """Returns (counts[nTrans], loglikeSum, loglike[nPairs]); accumulates into ``counts`` if given."""
        if counts is None:
            counts = np.zeros(self.dm.nTrans, np.float64)
        assert counts.dtype == np.float64 and counts.shape == (self.dm.nTrans,) and counts.flags.c_contiguous
        s = C.c_double(0.0)
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_batch_counts(self.h, _p(counts, C.c_double), C.byref(s), _p(ll, C.c_double)))
        return counts, s.value, ll


class DeviceProfiles:
    """Device-resident batch of profile tapes (mb_profiles*) for a machine with an empty input tape: per profile a
    [rows, nOutTok + 1] array of log weights, column 0 = the blank (profile.Profile.logRows).  With ``colTok`` the profiles are
    CTC-merged (mb_profiles_create_merged): per profile a [rows, nCols + 1] array, column 0 the blank and column c a CSV column
    whose output token is colTok[c - 1] (profile.Profile.mergeRows); every method works the same."""

    def __init__(self, dm: DeviceMachine, profiles, colTok=None):
        self.dm = dm
        self.colTok = None if colTok is None else np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
        width = dm.em.nOutTok + 1 if colTok is None else len(self.colTok) + 1
        rows = [np.asarray(p, np.float64).reshape(-1, width) for p in profiles]
        self.nProfiles = len(rows)
        self.rowOff = np.zeros(self.nProfiles + 1, np.int64)
        for k, r in enumerate(rows):
            self.rowOff[k + 1] = self.rowOff[k] + len(r)
        self.logP = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((1, width)), np.float64)
        L = load()
        if colTok is None:
            self.h = L.mb_profiles_create(dm.h, self.nProfiles, _p(self.logP, C.c_double), _p(self.rowOff, C.c_int64))
        else:
            self.h = L.mb_profiles_create_merged(dm.h, self.nProfiles, _p(self.logP, C.c_double), _p(self.rowOff, C.c_int64),
                                                 len(self.colTok), _p(self.colTok, C.c_int32))
        if not self.h:
            raise MbError(L.mb_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.mb_profiles_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def forward(self, flags: int = MB_ROLLING) -> np.ndarray:
        ll = np.empty(self.nProfiles, np.float64)
        _check(load().mb_profiles_forward(self.h, flags, _p(ll, C.c_double)))
        return ll

    def viterbi(self, paths: bool = True):
        """Returns (loglike, pathOff, pathEdges, pathRow); the last three are None without paths."""
        ll = np.empty(self.nProfiles, np.float64)
        if not paths:
            _check(load().mb_profiles_viterbi(self.h, _p(ll, C.c_double), None, None, None, 0))
            return ll, None, None, None
        L = load()
        cap = int(sum(L.mb_profile_path_bound(self.dm.h, int(n)) for n in np.diff(self.rowOff)))
        off = np.zeros(self.nProfiles + 1, np.int64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32)
        _check(L.mb_profiles_viterbi(self.h, _p(ll, C.c_double), _p(off, C.c_int64), _p(edges, C.c_uint32), _p(rows, C.c_int32), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy()

    def counts(self, counts: Optional[np.ndarray] = None):
        """Returns (counts[nTrans], loglikeSum, loglike[nProfiles]); accumulates into ``counts`` if given."""
        if counts is None:
            counts = np.zeros(self.dm.nTrans, np.float64)
        assert counts.dtype == np.float64 and counts.shape == (self.dm.nTrans,) and counts.flags.c_contiguous
        s = C.c_double(0.0)
        ll = np.empty(self.nProfiles, np.float64)
        _check(load().mb_profiles_counts(self.h, _p(counts, C.c_double), C.byref(s), _p(ll, C.c_double)))
        return counts, s.value, ll

    def row_posteriors(self):
        """Returns (post[sumRows, width], loglike[nProfiles]), width = nOutTok + 1 or, merged, nCols + 1: post[rowOff[k] + r][x] is
        the posterior probability that row r of profile k was consumed as column x (0: the blank), the gradient of loglike[k] in
        that entry of the profile; zeros for a profile whose likelihood is -inf (docs/profile_tapes.md, "Row posteriors of
        one-tape profiles").  Plain and merged profiles alike."""
        post = np.zeros((int(self.rowOff[-1]), self.logP.shape[1]), np.float64)
        ll = np.empty(self.nProfiles, np.float64)
        _check(load().mb_profiles_row_posteriors(self.h, _p(post, C.c_double), _p(ll, C.c_double)))
        return post, ll

    def set_profiles(self, profiles):
        """New rows for every profile, of the shapes the object was created with.  A refused table (NaN, +inf) leaves the old rows
        in effect."""
        width = self.logP.shape[1]
        rows = [np.asarray(q, np.float64).reshape(-1, width) for q in profiles]
        if len(rows) != self.nProfiles or any(len(r) != n for r, n in zip(rows, np.diff(self.rowOff))):
            raise ValueError("one profile per profile of the object with the rows it was created with, please")
        logP = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((1, width)), np.float64)
        _check(load().mb_profiles_set_rows(self.h, _p(logP, C.c_double)))
        self.logP = logP


def profile_fill(dm: DeviceMachine, mode: int, logP) -> np.ndarray:
    """One profile's lattice [rows + 1, 2, nStates] (layer 0 = arrived at the row, 1 = after the silent moves)."""
    P = np.ascontiguousarray(np.asarray(logP, np.float64).reshape(-1, dm.em.nOutTok + 1))
    cells = np.empty((len(P) + 1, 2, dm.nStates), np.float64)
    _check(load().mb_profile_fill(dm.h, mode, _p(P, C.c_double), len(P), _p(cells, C.c_double)))
    return cells


def profile_fill_merged(dm: DeviceMachine, mode: int, logP, colTok) -> np.ndarray:
    """One merged profile's lattice [rows + 1, 2, nCols + 1, nStates] (layer 0 = arrived at the row, 1 = after the silent moves;
    plane 0 = the last row took the blank, plane c = it took column c)."""
    ct = np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
    P = np.ascontiguousarray(np.asarray(logP, np.float64).reshape(-1, len(ct) + 1))
    cells = np.empty((len(P) + 1, 2, len(ct) + 1, dm.nStates), np.float64)
    _check(load().mb_profile_fill_merged(dm.h, mode, _p(P, C.c_double), len(P), len(ct), _p(ct, C.c_int32), _p(cells, C.c_double)))
    return cells


class DeviceProfilePairs:
    """Device-resident batch of (input sequence, profile) pairs (mb_profile_pairs*) for a machine with an input alphabet: pair k is
    the token sequence ``inputs[k]`` (1..nInTok) against the [rows, nOutTok + 1] log weights ``profiles[k]``, column 0 = the blank
    (profile.Profile.logRows).  The yardstick is profile.PairProfileDP (docs/profile_tapes.md, "Pairs").  With ``colTok`` the
    profiles are CTC-merged (mb_profile_pairs_create_merged): per pair a [rows, nCols + 1] array, column 0 the blank and column c a
    CSV column whose output token is colTok[c - 1] (profile.Profile.mergeRows); every method works the same and the yardstick is
    profile.PairMergedProfileDP."""

    def __init__(self, dm: DeviceMachine, inputs, profiles, colTok=None):
        self.dm = dm
        self.colTok = None if colTok is None else np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
        width = dm.em.nOutTok + 1 if colTok is None else len(self.colTok) + 1
        rows = [np.asarray(p, np.float64).reshape(-1, width) for p in profiles]
        xs = [np.asarray(x, np.int64).reshape(-1) for x in inputs]
        if len(xs) != len(rows):
            raise ValueError("as many input sequences as profiles, please")
        self.nPairs = len(rows)
        self.rowOff = np.zeros(self.nPairs + 1, np.int64); self.inOff = np.zeros(self.nPairs + 1, np.int64)
        for k, (x, r) in enumerate(zip(xs, rows)):
            self.rowOff[k + 1] = self.rowOff[k] + len(r)
            self.inOff[k + 1] = self.inOff[k] + len(x)
        self.logP = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((1, width)), np.float64)
        self.inTok = np.ascontiguousarray(np.concatenate(xs + [np.zeros(1, np.int64)]), np.int32)
        L = load()
        if colTok is None:
            self.h = L.mb_profile_pairs_create(dm.h, self.nPairs, _p(self.inTok, C.c_int32), _p(self.inOff, C.c_int64),
                                               _p(self.logP, C.c_double), _p(self.rowOff, C.c_int64))
        else:
            self.h = L.mb_profile_pairs_create_merged(dm.h, self.nPairs, _p(self.inTok, C.c_int32), _p(self.inOff, C.c_int64),
                                                      _p(self.logP, C.c_double), _p(self.rowOff, C.c_int64), len(self.colTok),
                                                      _p(self.colTok, C.c_int32))
        if not self.h:
            raise MbError(L.mb_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.mb_profile_pairs_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def path_cap(self) -> int:
        L = load()
        return int(sum(L.mb_profile_pair_path_bound(self.dm.h, int(i), int(r)) for i, r in zip(np.diff(self.inOff), np.diff(self.rowOff))))

    def set_envelopes(self, envs):
        """envs: per pair None (full: the pair keeps the sweeps over the whole rectangle), a seqpair.Envelope or an (inStart,
        inEnd) pair of rows + 1 entries each; ``None`` instead of a list clears every envelope (docs/profile_tapes.md, "Pairs
        under an envelope").  Plain profiles; an object created with ``colTok`` takes set_merged_envelopes."""
        _set_envelopes(load().mb_profile_pairs_set_envelopes, self.h, self.nPairs, envs)

    def set_merged_envelopes(self, envs):
        """set_envelopes for an object created with ``colTok``: a cell outside is -inf in every plane, and the sweeps, the counts and
        merged_row_posteriors visit the envelope cells alone (docs/profile_tapes.md, "Pairs against a merged profile under an
        envelope").  The yardstick is profile.PairMergedProfileDP with ``env``."""
        _set_envelopes(load().mb_profile_pairs_set_envelopes_merged, self.h, self.nPairs, envs)

    def cells(self) -> int:
        """Doubles of the materialised lattices of all pairs under the current envelopes."""
        return int(load().mb_profile_pairs_cells(self.h))

    def forward(self, flags: int = MB_ROLLING) -> np.ndarray:
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_pairs_forward(self.h, flags, _p(ll, C.c_double)))
        return ll

    def viterbi(self, paths: bool = True, cap: Optional[int] = None):
        """Returns (loglike, pathOff, pathEdges, pathRow); the last three are None without paths.  ``cap``: the size of the path
        buffers (default: the sum of the pairs' path bounds, which is what the library asks for)."""
        ll = np.empty(self.nPairs, np.float64)
        if not paths:
            _check(load().mb_profile_pairs_viterbi(self.h, _p(ll, C.c_double), None, None, None, 0))
            return ll, None, None, None
        cap = self.path_cap() if cap is None else int(cap)
        off = np.zeros(self.nPairs + 1, np.int64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32)
        _check(load().mb_profile_pairs_viterbi(self.h, _p(ll, C.c_double), _p(off, C.c_int64), _p(edges, C.c_uint32), _p(rows, C.c_int32), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy()

    def sample_paths(self, nSamples: int, seed: int = 0, cap: Optional[int] = None):
        """``nSamples`` alignments per pair drawn from the posterior on the device (mb_profile_pairs_sample; docs/profile_tapes.md,
        "Posterior path samples").  Returns (loglike[nPairs], off[nPairs * nSamples + 1], edges, rows, logq[nPairs * nSamples]):
        path k * nSamples + j is sample j of pair k in the format of viterbi(), logq its log posterior probability.  A sample
        depends on (seed, k, j) alone.  ``cap``: the size of the path buffers (default: nSamples times path_cap()).  Plain profiles
        only.  The yardstick is profile.PairProfileDP.samplePaths with ``pair=k``."""
        nSamples = int(nSamples)
        cap = self.path_cap() * max(nSamples, 0) if cap is None else int(cap)
        n = self.nPairs * max(nSamples, 0)
        ll = np.empty(self.nPairs, np.float64)
        off = np.zeros(n + 1, np.int64); logq = np.empty(n, np.float64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32)
        _check(load().mb_profile_pairs_sample(self.h, nSamples, int(seed) & 0xffffffffffffffff, _p(ll, C.c_double), _p(off, C.c_int64),
                                              _p(edges, C.c_uint32), _p(rows, C.c_int32), _p(logq, C.c_double), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy(), logq

    def merged_sample_paths(self, nSamples: int, seed: int = 0, cap: Optional[int] = None):
        """sample_paths() for an object created with ``colTok`` (mb_profile_pairs_sample_merged; docs/profile_tapes.md, "Posterior
        path samples of pairs against a merged profile").  Returns (loglike[nPairs], off[nPairs * nSamples + 1], edges, rows,
        rowCol[nSamples * sumRows], logq[nPairs * nSamples]): rowCol[rowOff[k] * nSamples + j * L_k + r] is the column row r of
        sample j of pair k took (0: the blank; c: column c, fresh or repeated; -1 in every row of a -inf pair), which with the edges
        determines the lattice path whose log posterior probability logq is.  The yardstick is
        profile.PairMergedProfileDP.samplePaths with ``pair=k``."""
        nSamples = int(nSamples)
        cap = self.path_cap() * max(nSamples, 0) if cap is None else int(cap)
        n = self.nPairs * max(nSamples, 0)
        ll = np.empty(self.nPairs, np.float64)
        off = np.zeros(n + 1, np.int64); logq = np.empty(n, np.float64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32)
        rowCol = np.full(max(int(self.rowOff[-1]) * max(nSamples, 0), 1), -1, np.int32)
        _check(load().mb_profile_pairs_sample_merged(self.h, nSamples, int(seed) & 0xffffffffffffffff, _p(ll, C.c_double), _p(off, C.c_int64),
                                                     _p(edges, C.c_uint32), _p(rows, C.c_int32), _p(rowCol, C.c_int32), _p(logq, C.c_double), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy(), rowCol[:int(self.rowOff[-1]) * nSamples], logq

    def counts(self, counts: Optional[np.ndarray] = None):
        """Returns (counts[nTrans], loglikeSum, loglike[nPairs]); accumulates into ``counts`` if given."""
        if counts is None:
            counts = np.zeros(self.dm.nTrans, np.float64)
        assert counts.dtype == np.float64 and counts.shape == (self.dm.nTrans,) and counts.flags.c_contiguous
        s = C.c_double(0.0)
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_pairs_counts(self.h, _p(counts, C.c_double), C.byref(s), _p(ll, C.c_double)))
        return counts, s.value, ll

    def row_posteriors(self):
        """Returns (post[sumRows, nOutTok + 1], loglike[nPairs]): post[rowOff[k] + r][o] is the posterior probability that row r of
        pair k was consumed as output token o (column 0: as the blank), the gradient of loglike[k] in that entry of the profile;
        zeros for a pair whose likelihood is -inf (docs/profile_tapes.md, "Row posteriors").  Plain profiles only."""
        post = np.zeros((int(self.rowOff[-1]), self.logP.shape[1]), np.float64)
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_pairs_row_posteriors(self.h, _p(post, C.c_double), _p(ll, C.c_double)))
        return post, ll

    def _set_rows(self, call, profiles):
        width = self.logP.shape[1]
        rows = [np.asarray(q, np.float64).reshape(-1, width) for q in profiles]
        if len(rows) != self.nPairs or any(len(r) != n for r, n in zip(rows, np.diff(self.rowOff))):
            raise ValueError("one profile per pair with the rows it was created with, please")
        logP = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((1, width)), np.float64)
        _check(call(self.h, _p(logP, C.c_double)))
        self.logP = logP

    def set_profiles(self, profiles):
        """New rows for every pair, of the shapes the object was created with; the inputs and the envelopes stay.  A refused
        table (NaN, +inf) leaves the old rows in effect."""
        self._set_rows(load().mb_profile_pairs_set_rows, profiles)

    def merged_row_posteriors(self):
        """Returns (post[sumRows, nCols + 1], loglike[nPairs]) of an object created with ``colTok``: post[rowOff[k] + r][c] is the
        posterior probability that row r of pair k was consumed as column c (column 0: as the blank) -- the blank out of every
        plane, the repeat of column c, and the emissions of colTok[c - 1] out of every other plane -- the gradient of loglike[k]
        in that entry of the merged profile; zeros for a pair whose likelihood is -inf (docs/profile_tapes.md, "Row posteriors
        of pairs against a merged profile").  The yardstick is profile.PairMergedProfileDP.rowPosteriors."""
        post = np.zeros((int(self.rowOff[-1]), self.logP.shape[1]), np.float64)
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_pairs_row_posteriors_merged(self.h, _p(post, C.c_double), _p(ll, C.c_double)))
        return post, ll

    def set_merged_profiles(self, profiles):
        """set_profiles for an object created with ``colTok``: new [rows, nCols + 1] rows for every pair."""
        self._set_rows(load().mb_profile_pairs_set_rows_merged, profiles)


def _env_rows(env):
    """(inStart, inEnd) as int32 arrays from a seqpair.Envelope or a pair of sequences."""
    a, b = (env.inStart, env.inEnd) if hasattr(env, "inStart") else env
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), np.int32); b = np.ascontiguousarray(np.asarray(b).reshape(-1), np.int32)
    if len(a) != len(b):
        raise ValueError("inStart and inEnd of an envelope have one entry per row each")
    return a, b


def _set_envelopes(call, h, nPairs, envs):
    """The envelopes of a pairs object through its set_envelopes entry ``call``: one None, Envelope or (inStart, inEnd) per pair,
    packed; ``None`` instead of a list clears."""
    if envs is None:
        _check(call(h, None, None, None))
        return
    envs = list(envs)
    if len(envs) != nPairs:
        raise ValueError("one envelope (or None) per pair, please")
    off = np.zeros(nPairs + 1, np.int64)
    st, en = [], []
    for k, e in enumerate(envs):
        n = 0
        if e is not None:
            a, b = _env_rows(e)
            st.append(a); en.append(b); n = len(a)
        off[k + 1] = off[k] + n
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(1, np.int32), np.int32)
    a, b = cat(st), cat(en)
    _check(call(h, _p(off, C.c_int64), _p(a, C.c_int32), _p(b, C.c_int32)))


def profile_pair_fill(dm: DeviceMachine, mode: int, x, logP, env=None) -> np.ndarray:
    """One pair's lattice [len(x) + 1, rows + 1, 2, nStates] (layer 0 = arrived at (i, row), 1 = after the output-less moves).
    ``env``: a seqpair.Envelope or (inStart, inEnd); the cells outside it are -inf in both layers."""
    P = np.ascontiguousarray(np.asarray(logP, np.float64).reshape(-1, dm.em.nOutTok + 1))
    xs = np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1), np.int32)
    cells = np.empty((len(xs) + 1, len(P) + 1, 2, dm.nStates), np.float64)
    if env is None:
        _check(load().mb_profile_pair_fill(dm.h, mode, _p(xs, C.c_int32), len(xs), _p(P, C.c_double), len(P), _p(cells, C.c_double)))
        return cells
    a, b = _env_rows(env)
    if len(a) != len(P) + 1:
        raise MbError("Envelope/sequence mismatch")
    _check(load().mb_profile_pair_fill_env(dm.h, mode, _p(xs, C.c_int32), len(xs), _p(P, C.c_double), len(P), _p(a, C.c_int32),
                                           _p(b, C.c_int32), _p(cells, C.c_double)))
    return cells


def profile_pair_fill_merged(dm: DeviceMachine, mode: int, x, logP, colTok, env=None) -> np.ndarray:
    """One pair's lattice against a merged profile, [len(x) + 1, rows + 1, 2, nCols + 1, nStates] (layer 0 = arrived at (i, row),
    1 = after the output-less moves; plane 0 = the last row took the blank, plane c = it took column c).  ``env``: a
    seqpair.Envelope or (inStart, inEnd); the cells outside it are -inf in both layers and all planes."""
    ct = np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
    P = np.ascontiguousarray(np.asarray(logP, np.float64).reshape(-1, len(ct) + 1))
    xs = np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1), np.int32)
    cells = np.empty((len(xs) + 1, len(P) + 1, 2, len(ct) + 1, dm.nStates), np.float64)
    if env is None:
        _check(load().mb_profile_pair_fill_merged(dm.h, mode, _p(xs, C.c_int32), len(xs), _p(P, C.c_double), len(P), len(ct),
                                                  _p(ct, C.c_int32), _p(cells, C.c_double)))
        return cells
    a, b = _env_rows(env)
    if len(a) != len(P) + 1:
        raise MbError("Envelope/sequence mismatch")
    _check(load().mb_profile_pair_fill_merged_env(dm.h, mode, _p(xs, C.c_int32), len(xs), _p(P, C.c_double), len(P), len(ct),
                                                  _p(ct, C.c_int32), _p(a, C.c_int32), _p(b, C.c_int32), _p(cells, C.c_double)))
    return cells


class DeviceProfileTwos:
    """Device-resident batch of (input profile, output profile) pairs (mb_profile_twos*) for a machine with an input alphabet: pair k
    is the [rows, nInTok + 1] log weights ``inProfiles[k]`` (profile.Profile.logRowsIn) against the [rows, nOutTok + 1] log weights
    ``outProfiles[k]`` (profile.Profile.logRows), column 0 of either the blank.  The yardstick is profile.TwoProfileDP
    (docs/profile_tapes.md, "Pairs of profiles").  ``envs``: what envelopes() takes (docs/profile_tapes.md, "Pairs of profiles
    under an envelope"); the yardstick is then TwoProfileDP(env=...).  With ``colTok`` the output profiles are CTC-merged
    (mb_profile_twos_create_merged): per pair a [rows, nCols + 1] array, column 0 the blank and column c a CSV column whose output
    token is colTok[c - 1] (profile.Profile.mergeRows); forward, viterbi, counts, cells and set_profiles work the same and the
    yardstick is profile.TwoMergedProfileDP (docs/profile_tapes.md, "Pairs of profiles against a merged profile").  ``envs``,
    envelopes() and row_posteriors take plain profiles; the envelopes of a merged object are ``mergedEnvs`` / merged_envelopes()
    (docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope"; the yardstick is then
    TwoMergedProfileDP with ``env``), its row posteriors merged_row_posteriors."""

    def __init__(self, dm: DeviceMachine, inProfiles, outProfiles, envs=None, colTok=None, mergedEnvs=None):
        self.dm = dm
        self.colTok = None if colTok is None else np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
        if self.colTok is not None and envs is not None:
            raise MbError("envelopes take plain profiles")
        wa, wb = dm.em.nInTok + 1, dm.em.nOutTok + 1 if colTok is None else len(self.colTok) + 1
        As = [np.asarray(p, np.float64).reshape(-1, wa) for p in inProfiles]
        Bs = [np.asarray(p, np.float64).reshape(-1, wb) for p in outProfiles]
        if len(As) != len(Bs):
            raise ValueError("as many input profiles as output profiles, please")
        self.nPairs = len(As)
        self.rowOff = np.zeros(self.nPairs + 1, np.int64); self.inOff = np.zeros(self.nPairs + 1, np.int64)
        for k, (a, b) in enumerate(zip(As, Bs)):
            self.inOff[k + 1] = self.inOff[k] + len(a)
            self.rowOff[k + 1] = self.rowOff[k] + len(b)
        self.logA = np.ascontiguousarray(np.concatenate(As + [np.zeros((1, wa))]), np.float64)
        self.logB = np.ascontiguousarray(np.concatenate(Bs + [np.zeros((1, wb))]), np.float64)
        L = load()
        if self.colTok is None:
            self.h = L.mb_profile_twos_create(dm.h, self.nPairs, _p(self.logA, C.c_double), _p(self.inOff, C.c_int64),
                                              _p(self.logB, C.c_double), _p(self.rowOff, C.c_int64))
        else:
            self.h = L.mb_profile_twos_create_merged(dm.h, self.nPairs, _p(self.logA, C.c_double), _p(self.inOff, C.c_int64),
                                                     _p(self.logB, C.c_double), _p(self.rowOff, C.c_int64), len(self.colTok),
                                                     _p(self.colTok, C.c_int32))
        if not self.h:
            raise MbError(L.mb_last_error().decode())
        if envs is not None:
            self.envelopes(envs)
        if mergedEnvs is not None:
            self.merged_envelopes(mergedEnvs)

    def envelopes(self, envs):
        """Replaces the envelopes.  envs: per pair None, a seqpair.Envelope or an (inStart, inEnd) pair of rows + 1 entries each --
        output row r holds the input-row positions inStart[r] <= i < inEnd[r]; ``None`` instead of a list clears every envelope.
        If any pair has one, every pair runs the envelope kernels, a pair given None under the full envelope (the same bits as
        without).  A refused list (MbError) leaves the object without envelopes."""
        _set_envelopes(load().mb_profile_twos_set_envelopes, self.h, self.nPairs, envs)

    def merged_envelopes(self, envs):
        """envelopes() for an object created with ``colTok``: a cell outside is -inf in every plane of every layer, and the sweeps,
        the counts and merged_row_posteriors visit the envelope cells alone (docs/profile_tapes.md, "Pairs of profiles against a
        merged profile under an envelope").  As there, no call mixes geometries: a pair given None runs under the full envelope,
        with the bits it has without.  A refused list (MbError) leaves the object without envelopes."""
        _set_envelopes(load().mb_profile_twos_set_envelopes_merged, self.h, self.nPairs, envs)

    def cells(self) -> int:
        """Doubles of the materialised lattices of all pairs under the current envelopes."""
        return int(load().mb_profile_twos_cells(self.h))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.mb_profile_twos_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def path_cap(self) -> int:
        L = load()
        return int(sum(L.mb_profile_pair_path_bound(self.dm.h, int(i), int(r)) for i, r in zip(np.diff(self.inOff), np.diff(self.rowOff))))

    def forward(self, flags: int = MB_ROLLING) -> np.ndarray:
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_twos_forward(self.h, flags, _p(ll, C.c_double)))
        return ll

    def viterbi(self, paths: bool = True, cap: Optional[int] = None):
        """Returns (loglike, pathOff, pathEdges, pathRow, pathInRow); the last four are None without paths.  ``cap``: the size of
        the path buffers (default: the sum of the pairs' path bounds, which is what the library asks for)."""
        ll = np.empty(self.nPairs, np.float64)
        if not paths:
            _check(load().mb_profile_twos_viterbi(self.h, _p(ll, C.c_double), None, None, None, None, 0))
            return ll, None, None, None, None
        cap = self.path_cap() if cap is None else int(cap)
        off = np.zeros(self.nPairs + 1, np.int64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32); ins = np.empty(max(cap, 1), np.int32)
        _check(load().mb_profile_twos_viterbi(self.h, _p(ll, C.c_double), _p(off, C.c_int64), _p(edges, C.c_uint32), _p(rows, C.c_int32),
                                              _p(ins, C.c_int32), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy(), ins[:off[-1]].copy()

    def sample_paths(self, nSamples: int, seed: int = 0, cap: Optional[int] = None):
        """``nSamples`` alignments per pair drawn from the posterior on the device (mb_profile_twos_sample; docs/profile_tapes.md,
        "Posterior path samples of pairs of profiles").  Returns (loglike[nPairs], off[nPairs * nSamples + 1], edges, rows, inRows,
        logq[nPairs * nSamples]): path k * nSamples + j is sample j of pair k in the format of viterbi(), logq its log posterior
        probability.  A sample depends on (seed, k, j) alone.  ``cap``: the size of the path buffers (default: nSamples times
        path_cap()).  Plain profiles only, with or without envelopes.  The yardstick is profile.TwoProfileDP.samplePaths with
        ``pair=k``."""
        nSamples = int(nSamples)
        cap = self.path_cap() * max(nSamples, 0) if cap is None else int(cap)
        n = self.nPairs * max(nSamples, 0)
        ll = np.empty(self.nPairs, np.float64)
        off = np.zeros(n + 1, np.int64); logq = np.empty(n, np.float64)
        edges = np.empty(max(cap, 1), np.uint32); rows = np.empty(max(cap, 1), np.int32); ins = np.empty(max(cap, 1), np.int32)
        _check(load().mb_profile_twos_sample(self.h, nSamples, int(seed) & 0xffffffffffffffff, _p(ll, C.c_double), _p(off, C.c_int64),
                                             _p(edges, C.c_uint32), _p(rows, C.c_int32), _p(ins, C.c_int32), _p(logq, C.c_double), cap))
        return ll, off, edges[:off[-1]].copy(), rows[:off[-1]].copy(), ins[:off[-1]].copy(), logq

    def counts(self, counts: Optional[np.ndarray] = None):
        """Returns (counts[nTrans], loglikeSum, loglike[nPairs]); accumulates into ``counts`` if given."""
        if counts is None:
            counts = np.zeros(self.dm.nTrans, np.float64)
        assert counts.dtype == np.float64 and counts.shape == (self.dm.nTrans,) and counts.flags.c_contiguous
        s = C.c_double(0.0)
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_twos_counts(self.h, _p(counts, C.c_double), C.byref(s), _p(ll, C.c_double)))
        return counts, s.value, ll

    def row_posteriors(self, inputs: bool = True, outputs: bool = True):
        """Returns (postA[sumK, nInTok + 1], postB[sumRows, nOutTok + 1], loglike[nPairs]): postB[rowOff[k] + r][o] is the posterior
        probability that output row r of pair k was consumed as output token o, postA[inOff[k] + i][a] that input row i was
        consumed as input token a (column 0 of either: as its blank) -- the gradients of loglike[k] in those entries of the two
        profiles; zeros for a pair whose likelihood is -inf (docs/profile_tapes.md, "Row posteriors of pairs of profiles").
        ``inputs=False`` / ``outputs=False``: that table is None and its kernel is not launched."""
        postA = np.zeros((int(self.inOff[-1]), self.logA.shape[1]), np.float64) if inputs else None
        postB = np.zeros((int(self.rowOff[-1]), self.logB.shape[1]), np.float64) if outputs else None
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_twos_row_posteriors(self.h, _p(postA, C.c_double), _p(postB, C.c_double), _p(ll, C.c_double)))
        return postA, postB, ll

    def merged_row_posteriors(self, inputs: bool = True, outputs: bool = True):
        """Of a merged object: returns (postA[sumK, nInTok + 1], postB[sumRows, nCols + 1], loglike[nPairs]).  postB[rowOff[k] + r][c]
        is the posterior probability that output row r of pair k was consumed as column c (0: the blank; a column holds its repeats
        and its fresh emissions), postA[inOff[k] + i][a] that input row i was consumed as input token a (0: the input blank) -- the
        gradients of loglike[k] in those entries of the two profiles; zeros for a pair whose likelihood is -inf
        (docs/profile_tapes.md, "Row posteriors of pairs of profiles against a merged profile").  ``inputs=False`` /
        ``outputs=False``: that table is None and its kernel is not launched."""
        postA = np.zeros((int(self.inOff[-1]), self.logA.shape[1]), np.float64) if inputs else None
        postB = np.zeros((int(self.rowOff[-1]), self.logB.shape[1]), np.float64) if outputs else None
        ll = np.empty(self.nPairs, np.float64)
        _check(load().mb_profile_twos_row_posteriors_merged(self.h, _p(postA, C.c_double), _p(postB, C.c_double), _p(ll, C.c_double)))
        return postA, postB, ll

    def set_profiles(self, inProfiles=None, outProfiles=None):
        """New rows for every pair on the input tape, the output tape or both (None: keep), of the shapes the object was created
        with.  A refused table (NaN, +inf) leaves both old tables in effect."""
        def table(profiles, old, off):
            if profiles is None:
                return None
            rows = [np.asarray(q, np.float64).reshape(-1, old.shape[1]) for q in profiles]
            if len(rows) != self.nPairs or any(len(r) != n for r, n in zip(rows, np.diff(off))):
                raise ValueError("one profile per pair with the rows it was created with, please")
            return np.ascontiguousarray(np.concatenate(rows + [np.zeros((1, old.shape[1]))]), np.float64)
        logA, logB = table(inProfiles, self.logA, self.inOff), table(outProfiles, self.logB, self.rowOff)
        _check(load().mb_profile_twos_set_rows(self.h, _p(logA, C.c_double), _p(logB, C.c_double)))
        if logA is not None:
            self.logA = logA
        if logB is not None:
            self.logB = logB


def profile_two_fill(dm: DeviceMachine, mode: int, logA, logB, env=None) -> np.ndarray:
    """One pair's lattice [rows of A + 1, rows of B + 1, 3, nStates] (layer 0 = arrived at (i, row), 1 = after the output-less
    moves, 2 = committed to wait for the next input row).  ``env``: a seqpair.Envelope or (inStart, inEnd); the cells outside it
    are -inf in all three layers."""
    A = np.ascontiguousarray(np.asarray(logA, np.float64).reshape(-1, dm.em.nInTok + 1))
    B = np.ascontiguousarray(np.asarray(logB, np.float64).reshape(-1, dm.em.nOutTok + 1))
    cells = np.empty((len(A) + 1, len(B) + 1, 3, dm.nStates), np.float64)
    if env is None:
        _check(load().mb_profile_two_fill(dm.h, mode, _p(A, C.c_double), len(A), _p(B, C.c_double), len(B), _p(cells, C.c_double)))
        return cells
    a, b = _env_rows(env)
    if len(a) != len(B) + 1:
        raise MbError("Envelope/sequence mismatch")
    _check(load().mb_profile_two_fill_env(dm.h, mode, _p(A, C.c_double), len(A), _p(B, C.c_double), len(B), _p(a, C.c_int32),
                                          _p(b, C.c_int32), _p(cells, C.c_double)))
    return cells


def profile_two_fill_merged(dm: DeviceMachine, mode: int, logA, logB, colTok, env=None) -> np.ndarray:
    """One pair's lattice against a merged output profile, [rows of A + 1, rows of B + 1, 3, nCols + 1, nStates] (layers as
    profile_two_fill; plane 0 = the last row took the blank, plane c = it took column c).  ``env``: a seqpair.Envelope or
    (inStart, inEnd); the cells outside it are -inf in all layers and planes."""
    ct = np.ascontiguousarray(np.asarray(colTok).reshape(-1), np.int32)
    A = np.ascontiguousarray(np.asarray(logA, np.float64).reshape(-1, dm.em.nInTok + 1))
    B = np.ascontiguousarray(np.asarray(logB, np.float64).reshape(-1, len(ct) + 1))
    cells = np.empty((len(A) + 1, len(B) + 1, 3, len(ct) + 1, dm.nStates), np.float64)
    if env is None:
        _check(load().mb_profile_two_fill_merged(dm.h, mode, _p(A, C.c_double), len(A), _p(B, C.c_double), len(B), len(ct),
                                                 _p(ct, C.c_int32), _p(cells, C.c_double)))
        return cells
    a, b = _env_rows(env)
    if len(a) != len(B) + 1:
        raise MbError("Envelope/sequence mismatch")
    _check(load().mb_profile_two_fill_merged_env(dm.h, mode, _p(A, C.c_double), len(A), _p(B, C.c_double), len(B), len(ct),
                                                 _p(ct, C.c_int32), _p(a, C.c_int32), _p(b, C.c_int32), _p(cells, C.c_double)))
    return cells


class DevicePrefix:
    """Device-resident node lattices of prefix searches (mb_prefix*): ``outputs`` is one token sequence per search, ``logR`` the
    machine's log((I - N)^-1) (prefixtree.logSumInTrans), ``maxNodes`` the fixed size of the node pool.  The tree is the caller's:
    nodes are slot numbers (prefixtree.PrefixTree, docs/decoding.md).  With ``profiles`` -- per search a [rows, nOutTok + 1] array
    of log weights, column 0 the blank (profile.Profile.logRows) -- the searches decode soft outputs and ``outputs`` is not read.
    With ``colTok`` as well the profiles are CTC-merged ([rows, nCols + 1] tables and the column map of profile.Profile.mergeRows,
    k_prefix_fill_merged) and a node's lattice has nCols + 1 planes."""

    def __init__(self, dm: DeviceMachine, outputs, logR, maxNodes: int, profiles=None, colTok=None):
        self.dm = dm
        self.colTok = None if colTok is None else np.ascontiguousarray(colTok, np.int32).reshape(-1)
        if self.colTok is not None and profiles is None:
            raise MbError("a column map needs profiles")
        width = dm.em.nOutTok + 1 if self.colTok is None else len(self.colTok) + 1
        if profiles is not None:
            outs = [np.asarray(p, np.float64).reshape(-1, width) for p in profiles]
        else:
            outs = [np.asarray(o, np.int32).reshape(-1) for o in outputs]
        self.nSeq = len(outs)
        self.outOff = np.zeros(self.nSeq + 1, np.int64)          # tokens, or rows
        for k, o in enumerate(outs):
            self.outOff[k + 1] = self.outOff[k] + len(o)
        R = np.ascontiguousarray(logR, np.float64)
        assert R.shape == (dm.nStates, dm.nStates)
        L = load()
        if profiles is not None:
            self.logP = np.ascontiguousarray(np.concatenate(outs + [np.zeros((1, width))]), np.float64)
        if self.colTok is not None:
            self.h = L.mb_prefix_create_merged(dm.h, self.nSeq, _p(self.logP, C.c_double), _p(self.outOff, C.c_int64), len(self.colTok),
                                               _p(self.colTok, C.c_int32), _p(R, C.c_double), int(maxNodes))
        elif profiles is not None:
            self.h = L.mb_prefix_create_profiles(dm.h, self.nSeq, _p(self.logP, C.c_double), _p(self.outOff, C.c_int64), _p(R, C.c_double), int(maxNodes))
        else:
            self.outTok = np.ascontiguousarray(np.concatenate(outs + [np.zeros(1, np.int32)]), np.int32)
            self.h = L.mb_prefix_create(dm.h, self.nSeq, _p(self.outTok, C.c_int32), _p(self.outOff, C.c_int64), _p(R, C.c_double), int(maxNodes))
        if not self.h:
            raise MbError(L.mb_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.mb_prefix_destroy(self.h)
            except Exception:
                pass
            self.h = None

    __del__ = close

    def root(self, seq: int = 0) -> Tuple[int, float, float]:
        """(node, logSeqProb, logPrefixProb) of the root of search ``seq``."""
        n = C.c_int64(-1); a = C.c_double(); b = C.c_double()
        _check(load().mb_prefix_root(self.h, int(seq), C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def extend(self, seq, parent, inTok) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """One launch: child i of node parent[i] (search seq[i]) by input token inTok[i]; (nodes, logSeqProb, logPrefixProb)."""
        sq = np.ascontiguousarray(seq, np.int64); pa = np.ascontiguousarray(parent, np.int64); tk = np.ascontiguousarray(inTok, np.int32)
        n = len(sq)
        assert len(pa) == n and len(tk) == n
        ch = np.empty(n, np.int64); a = np.empty(n, np.float64); b = np.empty(n, np.float64)
        _check(load().mb_prefix_extend(self.h, n, _p(sq, C.c_int64), _p(pa, C.c_int64), _p(tk, C.c_int32), _p(ch, C.c_int64),
                                       _p(a, C.c_double), _p(b, C.c_double)))
        return ch, a, b

    def release(self, nodes) -> None:
        nd = np.ascontiguousarray(nodes, np.int64)
        if len(nd):
            _check(load().mb_prefix_release(self.h, len(nd), _p(nd, C.c_int64)))

    def free_nodes(self) -> int:
        return load().mb_prefix_free_nodes(self.h)

    def node_cells(self, node: int, seq: int) -> np.ndarray:
        """The node's lattice [outLen + 1, 2, nStates] (layer 0 = seq, 1 = prefix), against merged profiles [rows + 1, 2, nCols + 1,
        nStates]; ``seq`` is the node's search (for the shape)."""
        L = int(self.outOff[seq + 1] - self.outOff[seq])
        cells = np.empty((L + 1, 2, self.dm.nStates) if self.colTok is None else (L + 1, 2, len(self.colTok) + 1, self.dm.nStates), np.float64)
        _check(load().mb_prefix_node_cells(self.h, int(node), _p(cells, C.c_double)))
        return cells
