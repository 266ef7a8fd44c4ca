"""kvsep -- Python binding (ctypes) of libkvsep_crc32c.so for tests and bench.

The product is the C ABI in include/kvsep_crc32c.h (C++ host code + gfx950 HIP kernels); this module
only marshals arguments.  It mirrors the reference's util/crc32c.h interface (extend / value / mask /
unmask, util/crc32c.h:17-38) and adds the batched device/host entry points.

There is no CPU fallback here: if the shared library is missing, importing the GPU entry points
raises; if no gfx950 device is present, Context() raises.  The oracle under oracle/ is never used.
"""
from __future__ import annotations

import ctypes
import os
import re
import sys

try:  # torch first: its libamdhip64.so.7 then serves our library too (same soname, one HIP runtime)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host-only entry points
    torch = None

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkvsep_crc32c.so")
HEADER_PATH = os.path.join(_HERE, "..", "..", "include", "kvsep_crc32c.h")

KVSEP_OK = 0
MASK_DELTA = 0xA282EAD8  # util/crc32c.h:22
OFFSET_SKIP = 2**64 - 1  # KVSEP_OFFSET_SKIP: dst_off of a block the offsets pass did not lay out

_lib = None


class KvsepError(RuntimeError):
    pass


def _u32p():
    return ctypes.POINTER(ctypes.c_uint32)


def _u64p():
    return ctypes.POINTER(ctypes.c_uint64)


_SIGS = {
    "kvsep_crc32c_extend": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "kvsep_crc32c_value": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_size_t]),
    "kvsep_crc32c_mask": (ctypes.c_uint32, [ctypes.c_uint32]),
    "kvsep_crc32c_unmask": (ctypes.c_uint32, [ctypes.c_uint32]),
    "kvsep_accelerated_crc32c": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "kvsep_set_offload_threshold": (None, [ctypes.c_uint64]),
    "kvsep_set_offload_wait": (None, [ctypes.c_int]),
    "kvsep_offload_stats": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_crc32c_kernel_name": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_crc32c_extend_host": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "kvsep_crc32c_host_path": (ctypes.c_char_p, []),
    "kvsep_crc32c_ctx_set_host_node": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_ctx_host_placement": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_ctx_inject_failure": (ctypes.c_int, [ctypes.c_void_p]),
    "kvsep_crc32c_plan_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_int)]),
    "kvsep_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "kvsep_pci_numa_node": (ctypes.c_int, [ctypes.c_char_p]),
    "kvsep_device_numa_node": (ctypes.c_int, [ctypes.c_int]),
    "kvsep_numa_node_cpus": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "kvsep_bind_process_numa": (ctypes.c_int, [ctypes.c_int]),
    "kvsep_host_page_node": (ctypes.c_int, [ctypes.c_void_p]),
    "kvsep_crc32c_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "kvsep_crc32c_ctx_destroy": (None, [ctypes.c_void_p]),
    "kvsep_crc32c_ctx_set_piece_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_crc32c_ctx_set_schedule": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_ctx_set_kernel": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_crc32c_reserve_captures": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_release_captures": (ctypes.c_int, [ctypes.c_void_p]),
    "kvsep_crc32c_capture_sets": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "kvsep_crc32c_ctx_set_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_ctx_get_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_uint64)]),
    "kvsep_crc32c_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_crc32c_verify_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_uint64]),
    "kvsep_crc32c_verify_list_device": (ctypes.c_int, [ctypes.c_void_p] * 11 + [ctypes.c_uint64, ctypes.c_void_p,
                                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_sst_verify_list_device": (ctypes.c_int, [ctypes.c_void_p] * 9 + [ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_sst_verify_list_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] +
                                   [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_log_verify_device": (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint64]),
    "kvsep_crc32c_group_verify_list_device": (ctypes.c_int, [ctypes.c_void_p] * 14 + [ctypes.c_uint64]),
    "kvsep_crc32c_combine": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "kvsep_crc32c_concat_device": (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_crc32c_gather_device": (ctypes.c_int, [ctypes.c_void_p] * 9 + [ctypes.c_uint64] * 4),
    "kvsep_crc32c_gather_host": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_crc32c_pack_device": (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_vlog_frame_offsets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "kvsep_vlog_frame_device": (ctypes.c_int, [ctypes.c_void_p] * 9 + [ctypes.c_uint64, ctypes.c_void_p] +
                                [ctypes.c_uint64] * 4),
    "kvsep_sst_frame_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p] +
                               [ctypes.c_uint64] * 3),
    "kvsep_crc32c_offsets_device": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64] * 3 +
                                    [ctypes.c_void_p] * 3 + [ctypes.c_uint64] * 2),
    "kvsep_crc32c_salvage_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
                                    [ctypes.c_uint64]),
    "kvsep_sst_salvage_device": (ctypes.c_int, [ctypes.c_void_p] * 10 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
                                 [ctypes.c_uint64] * 3),
    "kvsep_vlog_frame_auto_device": (ctypes.c_int, [ctypes.c_void_p] * 9 + [ctypes.c_uint64] * 2 +
                                     [ctypes.c_void_p] * 2 + [ctypes.c_uint64] * 4),
    "kvsep_log_walk_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 4 +
                              [ctypes.c_uint64, ctypes.c_void_p]),
    "kvsep_log_accept_gaps_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 5 +
                                     [ctypes.c_uint64] + [ctypes.c_void_p] * 4),
    "kvsep_log_read_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 7 +
                              [ctypes.c_uint64] + [ctypes.c_void_p] * 3),
    "kvsep_vlog_walk_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
                               [ctypes.c_uint64] + [ctypes.c_void_p] * 2),
    "kvsep_vlog_read_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 5 +
                               [ctypes.c_uint64] * 2 + [ctypes.c_void_p] * 7),
    "kvsep_log_chains": (ctypes.c_uint64, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3),
    "kvsep_log_chains_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64] + [ctypes.c_void_p] * 6),
    "kvsep_log_records_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 7 +
                                 [ctypes.c_uint64] + [ctypes.c_void_p] * 9 + [ctypes.c_uint64] +
                                 [ctypes.c_void_p] * 4),
    "kvsep_log_frame_layout": (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_uint64] * 2 + [ctypes.c_void_p] * 4),
    "kvsep_log_frame_device": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64] * 2 + [ctypes.c_void_p] +
                               [ctypes.c_uint64] + [ctypes.c_void_p] * 7 + [ctypes.c_uint64] +
                               [ctypes.c_void_p] * 2 + [ctypes.c_uint64]),
    "kvsep_crc32c_group_extend_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                                      ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]),
    "kvsep_crc32c_batch_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_crc32c_batch_host_span": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_uint64]),
    "kvsep_fill_splitmix64_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_uint64]),
    "kvsep_stream_read_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p]),
    "kvsep_vlog_walk": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "kvsep_vlog_verify_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_vlog_frame_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "kvsep_log_walk": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_log_verify_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p]),
    "kvsep_log_frame_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "kvsep_log_accept": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                           ctypes.c_void_p]),
    "kvsep_log_accept_gaps": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_sst_trailers_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_sst_verify_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "kvsep_sst_footer": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_sst_index_walk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_sst_index_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
                               [ctypes.c_uint64] + [ctypes.c_void_p] * 2),
    "kvsep_sst_table_verify_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 6 +
                                      [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64] +
                                      [ctypes.c_void_p] * 3),
    "kvsep_sst_index_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4 +
                             [ctypes.c_uint64] + [ctypes.c_void_p] * 2),
    "kvsep_sst_index_keys_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 5 +
                                    [ctypes.c_uint64] + [ctypes.c_void_p] * 2),
    "kvsep_sst_index_build": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                                      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_sst_footer_build": (ctypes.c_int, [ctypes.c_uint64] * 4 + [ctypes.c_void_p]),
    "kvsep_sst_index_build_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                             ctypes.c_uint64] + [ctypes.c_void_p] * 3),
    "kvsep_sst_table_finish_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                              ctypes.c_uint64] + [ctypes.c_void_p] * 4),
    "kvsep_sst_table_rewrite_device": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                               ctypes.c_uint64] + [ctypes.c_void_p] * 7 +
                                       [ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 7),
    "kvsep_sst_trailers_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_sst_verify_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint64]),
    "kvsep_crc32c_partition": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]),
    "kvsep_crc32c_group_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "kvsep_crc32c_group_destroy": (None, [ctypes.c_void_p]),
    "kvsep_crc32c_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "kvsep_crc32c_group_ctx": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "kvsep_crc32c_group_batch_host_span": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_crc32c_group_verify_host_span": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_uint64]),
    "kvsep_vlog_verify_host_group": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kvsep_crc32c_group_batch_device": (ctypes.c_int, [ctypes.c_void_p] * 9),
    "kvsep_crc32c_group_verify_device": (ctypes.c_int, [ctypes.c_void_p] * 13),
    "kvsep_host_alloc_pinned": (ctypes.c_void_p, [ctypes.c_uint64]),
    "kvsep_host_free_pinned": (None, [ctypes.c_void_p]),
    "kvsep_last_error": (ctypes.c_char_p, []),
    "kvsep_build_info": (ctypes.c_char_p, []),
    "kvsep_abi_version": (ctypes.c_int, []),
    "kvsep_device_count": (ctypes.c_int, []),
}


def lib():
    """Load libkvsep_crc32c.so (raises loudly if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KvsepError(f"{LIB_PATH} missing: run `make -C kv-separate_amd` (or __graft_entry__.build())")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def header_functions(path: str = HEADER_PATH):
    """Names of every function declared in include/kvsep_crc32c.h."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kvsep_[a-z0-9_]+)\s*\(", src)))


def _check(rc: int, what: str):
    if rc != KVSEP_OK:
        raise KvsepError(f"{what} failed ({rc}): {lib().kvsep_last_error().decode(errors='replace')}")


def _buf(data):
    """(ctypes pointer, keepalive) for bytes / bytearray / numpy arrays."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data)
        return a.ctypes.data_as(ctypes.c_void_p), a
    if isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(data, dtype=np.uint8)
        return a.ctypes.data_as(ctypes.c_void_p), a
    raise TypeError(type(data))


def _checked_len(keep, n):
    """n defaults to the whole buffer; a larger n would read past it."""
    if n is None:
        return keep.nbytes
    if n < 0 or n > keep.nbytes:
        raise ValueError(f"n = {n} outside the {keep.nbytes}-byte buffer")
    return n


# ------------------------------------------------------------------ scalar mirror of util/crc32c.h
def extend(init_crc: int, data, n: int | None = None) -> int:
    """leveldb::crc32c::Extend (util/crc32c.h:17)."""
    p, keep = _buf(data)
    n = _checked_len(keep, n)
    return lib().kvsep_crc32c_extend(init_crc & 0xFFFFFFFF, p, n)


def value(data, n: int | None = None) -> int:
    """leveldb::crc32c::Value (util/crc32c.h:20)."""
    return extend(0, data, n)


def mask(crc: int) -> int:
    """leveldb::crc32c::Mask (util/crc32c.h:29)."""
    return lib().kvsep_crc32c_mask(crc & 0xFFFFFFFF)


def unmask(masked: int) -> int:
    """leveldb::crc32c::Unmask (util/crc32c.h:35)."""
    return lib().kvsep_crc32c_unmask(masked & 0xFFFFFFFF)


def extend_host(init_crc: int, data, n: int | None = None) -> int:
    p, keep = _buf(data)
    n = _checked_len(keep, n)
    return lib().kvsep_crc32c_extend_host(init_crc & 0xFFFFFFFF, p, n)


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """Extend(crc_a, B) from crc_b = Value(B) and len_b = |B| (kvsep_crc32c_combine): the CRC of A||B from the CRCs of
    its parts.  Host only, exact for every len_b < 2**64."""
    return lib().kvsep_crc32c_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b)


def host_path() -> str:
    """The host leg this process runs ("fold", "sse42" or "portable"; kvsep_crc32c_host_path)."""
    return lib().kvsep_crc32c_host_path().decode()


# ------------------------------------------------------------------ device context
def _stream_handle(stream):
    if stream is None:
        if torch is not None and torch.cuda.is_available():
            return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return ctypes.c_void_p(0)
    if hasattr(stream, "cuda_stream"):
        return ctypes.c_void_p(stream.cuda_stream)
    return ctypes.c_void_p(int(stream))


def _dptr(t):
    if t is None:
        return ctypes.c_void_p(0)
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


DEFAULT_PIECE_BYTES = 128 * 1024  # the library default (kvsep_crc32c_ctx, crc32c_device.hip)


class Context:
    """One per device: uploads the Z_d tables once, owns scratch and staging."""

    def __init__(self, device: int = 0, piece_bytes: int | None = None, dynamic: bool | None = None):
        h = ctypes.c_void_p()
        _check(lib().kvsep_crc32c_ctx_create(device, ctypes.byref(h)), "kvsep_crc32c_ctx_create")
        self._h = h
        self.device = device
        if piece_bytes is not None:
            self.set_piece_bytes(piece_bytes)
        if dynamic is not None:
            self.set_schedule(dynamic)

    def close(self):
        if getattr(self, "_h", None):
            lib().kvsep_crc32c_ctx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_piece_bytes(self, n: int):
        _check(lib().kvsep_crc32c_ctx_set_piece_bytes(self._h, n), "set_piece_bytes")

    def set_schedule(self, dynamic):
        """True = guided dynamic, False = static contiguous runs, "rr" = static round-robin items, None = auto
        (guided only when long blocks are split)."""
        v = -1 if dynamic is None else 2 if dynamic == "rr" else (1 if dynamic else 0)
        _check(lib().kvsep_crc32c_ctx_set_schedule(self._h, v), "set_schedule")

    KERNELS = {"auto": 0, "wide": 1, "narrow": 2, "narrow16": 3, "narrow8": 4, "sorted": 5, "claim": 6, "claim16": 7,
               "coop": 8}

    def set_kernel(self, kernel: str):
        """Kernel choice for unsplit batches (kvsep_crc32c_ctx_set_kernel): "auto" (default), "wide", or the narrow
        kernel whenever the max_len hint is <= 64 KiB ("narrow"; "narrow16" / "narrow8" pin its workgroup size,
        "sorted" its sorted-window form for ragged batches, "claim" / "claim16" its workgroup-run form with LDS claims,
        8 / 16 lanes per block, "coop" the form whose 8 waves share each 8-block group).  Never changes a result."""
        _check(lib().kvsep_crc32c_ctx_set_kernel(self._h, self.KERNELS[kernel]), "set_kernel")

    def set_host_node(self, node: int):
        """NUMA node for this context's pinned staging and copier threads (-1: no placement; default: the device's)."""
        _check(lib().kvsep_crc32c_ctx_set_host_node(self._h, node), "set_host_node")

    def host_placement(self):
        """-> {"device_node", "staging_node", "copier_cpus"} (kvsep_crc32c_ctx_host_placement)."""
        dn, sn = ctypes.c_int(), ctypes.c_int()
        cpus = (ctypes.c_int * 4096)()
        n = lib().kvsep_crc32c_ctx_host_placement(self._h, ctypes.byref(dn), ctypes.byref(sn), cpus, 4096)
        if n < 0:
            _check(n, "host_placement")
        return {"device_node": dn.value, "staging_node": sn.value, "copier_cpus": list(cpus[:min(n, 4096)])}

    def inject_failure(self):
        """Fault injection (tests; csrc/kvsep_testing.h): the next batched call fails right after enqueuing its CRC
        kernel.  The library honours it only under KVSEP_TEST_HOOKS=1 (tests/conftest.py sets it)."""
        _check(lib().kvsep_crc32c_ctx_inject_failure(self._h), "inject_failure")

    def reserve(self, count: int, total_bytes: int):
        _check(lib().kvsep_crc32c_reserve(self._h, count, total_bytes), "reserve")

    def reserve_captures(self, nsets: int):
        """At least `nsets` capture sets (one per graph capture that may be held at once)."""
        _check(lib().kvsep_crc32c_reserve_captures(self._h, nsets), "reserve_captures")

    def release_captures(self):
        """Every capture set free again: only once the graphs captured so far are destroyed."""
        _check(lib().kvsep_crc32c_release_captures(self._h), "release_captures")

    def capture_sets(self):
        """(number of capture sets, how many a graph holds)."""
        held = ctypes.c_int(0)
        n = lib().kvsep_crc32c_capture_sets(self._h, ctypes.byref(held))
        _check(n if n < 0 else 0, "capture_sets")
        return n, held.value

    def kernel_name(self, count: int, max_len: int, total_bytes: int = 0) -> str:
        """The main kernel a batch of `count` blocks with these max_len / total_bytes hints runs on."""
        return lib().kvsep_crc32c_kernel_name(self._h, count, total_bytes, max_len).decode()

    def plan_query(self, count: int, max_len: int, total_bytes: int = 0):
        """(piece_bytes, pieces_needed, guided) of a batch with these hints (tests; csrc/kvsep_testing.h): the piece
        size it is cut at, the plan entries it needs (0: unsplit, no plan) and whether it runs the guided schedule."""
        pb, pn, gd = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        _check(lib().kvsep_crc32c_plan_query(self._h, count, total_bytes, max_len, ctypes.byref(pb), ctypes.byref(pn),
                                             ctypes.byref(gd)), "plan_query")
        return pb.value, pn.value, bool(gd.value)

    def set_timing(self, on: bool):
        _check(lib().kvsep_crc32c_ctx_set_timing(self._h, 1 if on else 0), "set_timing")

    def get_timing(self):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        _check(lib().kvsep_crc32c_ctx_get_timing(self._h, ctypes.byref(ms), ctypes.byref(n)), "get_timing")
        return ms.value, n.value

    # -- device form (torch tensors or raw device addresses)
    def batch_device(self, base, off, length, out, init=None, count=None, total_bytes=None, max_len=0, stream=None):
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_crc32c_batch_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off),
                                               _dptr(length), _dptr(init), _dptr(out), count, total_bytes,
                                               max_len), "kvsep_crc32c_batch_device")
        return out

    def verify_device(self, base, off, length, expected_masked, out, first_bad, nbad, init=None, count=None,
                      total_bytes=None, max_len=0, stream=None):
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_crc32c_verify_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off),
                                                _dptr(length), _dptr(init), _dptr(expected_masked), _dptr(out),
                                                _dptr(first_bad), _dptr(nbad), count, total_bytes, max_len),
               "kvsep_crc32c_verify_device")
        return out

    def verify_list_device(self, base, off, length, expected_masked, out, first_bad, nbad, bad_idx=None, bad_cap=None,
                           ok=None, init=None, count=None, total_bytes=None, max_len=0, stream=None):
        """verify_device, then the list pass (kvsep_crc32c_verify_list_device): bad_idx (int64 / uint64 device tensor,
        bad_cap defaults to its length) receives the mismatching block indices, ascending, at most bad_cap of them; ok
        (uint8 device tensor of `count`, optional) 1 / 0 per block."""
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        if bad_cap is None:
            bad_cap = 0 if bad_idx is None else int(bad_idx.numel())
        _check(lib().kvsep_crc32c_verify_list_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off),
                                                     _dptr(length), _dptr(init), _dptr(expected_masked), _dptr(out),
                                                     _dptr(first_bad), _dptr(nbad), _dptr(bad_idx), bad_cap, _dptr(ok),
                                                     count, total_bytes, max_len),
               "kvsep_crc32c_verify_list_device")
        return out

    def log_verify_device(self, base, off, length, stored, ok, count=None, total_bytes=None, max_len=0, stream=None):
        """db/log_reader.cc:246-259 for a device-resident log image: off / length / stored as log_walk gives them, on
        the device; ok (uint8 device tensor) = 1 where the record's checksum matches (kvsep_log_verify_device)."""
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_log_verify_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off), _dptr(length),
                                             _dptr(stored), _dptr(ok), count, total_bytes, max_len),
               "kvsep_log_verify_device")
        return ok

    def log_walk_device(self, base, n, nrec, off=None, length=None, stored=None, type=None, cap=None, stream=None):
        """kvsep_log_walk_device: the walk of log_walk over the n bytes of the device image at base.  nrec (one-element
        int64 device tensor) receives the number of physical records; off / length (int64), stored (int32) and type
        (uint8), each optional, are written for exactly cap elements: the records first, zeros after them."""
        if cap is None:
            cap = min(int(t.numel()) for t in (off, length, stored, type) if t is not None and not isinstance(t, int))
        _check(lib().kvsep_log_walk_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off), _dptr(length),
                                           _dptr(stored), _dptr(type), cap, _dptr(nrec)), "kvsep_log_walk_device")
        return nrec

    def sst_index_device(self, file_base, n, handle, off, length, nblocks, status, cap=None, stream=None):
        """kvsep_sst_index_device: the walk of sst_index_walk over the index block handle (int64 device tensor:
        index_off, index_len) names in the n-byte device image at file_base.  off / length (int64) are written for
        exactly cap elements: the data blocks' handles first, zeros after them; nblocks (one-element int64) receives the
        full count, status (one-element int32) a SST_* code."""
        if cap is None:
            cap = min(int(off.numel()), int(length.numel()))
        _check(lib().kvsep_sst_index_device(self._h, _stream_handle(stream), _dptr(file_base), n, _dptr(handle),
                                            _dptr(off), _dptr(length), cap, _dptr(nblocks), _dptr(status)),
               "kvsep_sst_index_device")
        return nblocks

    def sst_table_verify_device(self, file_base, n, off, length, crc, ok, nblocks, handles, status, first_bad=None,
                                nbad=None, bad_idx=None, bad_cap=None, cap=None, max_len_hint=0, stream=None):
        """kvsep_sst_table_verify_device: footer, index walk and the read check of every block of the n-byte device
        table image at file_base, on one stream.  off / length (int64), crc (int32) and ok (uint8, optional) have cap
        slots: the data blocks in index order, the metaindex block, the index block, padding.  handles (4 int64), nblocks
        (one int64) and status (one int32, a SST_* code) are device tensors; first_bad / nbad / bad_idx as in
        sst_verify_list_device."""
        if cap is None:
            cap = min(int(off.numel()), int(length.numel()), int(crc.numel()))
        if bad_cap is None:
            bad_cap = int(bad_idx.numel()) if bad_idx is not None else 0
        _check(lib().kvsep_sst_table_verify_device(self._h, _stream_handle(stream), _dptr(file_base), n, _dptr(off),
                                                   _dptr(length), _dptr(crc), _dptr(first_bad), _dptr(nbad),
                                                   _dptr(bad_idx), bad_cap, _dptr(ok), cap, max_len_hint,
                                                   _dptr(nblocks), _dptr(handles), _dptr(status)),
               "kvsep_sst_table_verify_device")
        return status

    def sst_index_keys_device(self, file_base, n, handle, off, length, key_off, key_len, nblocks, status, cap=None,
                              stream=None):
        """kvsep_sst_index_keys_device: sst_index_device, and key_off / key_len (int64, cap elements): where each emitted
        entry's key bytes lie in the image and how long they are.  An entry that shares key bytes with the one before
        it stops the walk with SST_SHARED_KEY."""
        if cap is None:
            cap = min(int(off.numel()), int(length.numel()), int(key_off.numel()), int(key_len.numel()))
        _check(lib().kvsep_sst_index_keys_device(self._h, _stream_handle(stream), _dptr(file_base), n, _dptr(handle),
                                                 _dptr(off), _dptr(length), _dptr(key_off), _dptr(key_len), cap,
                                                 _dptr(nblocks), _dptr(status)), "kvsep_sst_index_keys_device")
        return nblocks

    def sst_index_build_device(self, key_base, key_off, key_len, blk_off, blk_len, dst, dst_bytes, at, out_len, status,
                               keep=None, count=None, stream=None):
        """kvsep_sst_index_build_device: the index block BlockBuilder writes at restart interval 1 for the kept entries
        (keep[i] != 0 and blk_off[i] != OFFSET_SKIP), with its trailer, at dst + at[0].  key_off / key_len / blk_off /
        blk_len / at / out_len are int64 device tensors, keep uint8, status (one int32) a SSTW_* code."""
        if count is None:
            count = int(key_off.numel())
        _check(lib().kvsep_sst_index_build_device(self._h, _stream_handle(stream), _dptr(key_base), _dptr(key_off),
                                                  _dptr(key_len), _dptr(blk_off), _dptr(blk_len), _dptr(keep), count,
                                                  _dptr(dst), dst_bytes, _dptr(at), _dptr(out_len), _dptr(status)),
               "kvsep_sst_index_build_device")
        return status

    def sst_table_finish_device(self, key_base, key_off, key_len, blk_off, blk_len, dst, dst_bytes, data_end, index_len,
                                table_bytes, status, keep=None, count=None, stream=None):
        """kvsep_sst_table_finish_device: the empty metaindex block at dst + data_end[0], the index block of
        sst_index_build_device after it, the footer after its trailer; table_bytes (one int64) the table's size."""
        if count is None:
            count = int(key_off.numel())
        _check(lib().kvsep_sst_table_finish_device(self._h, _stream_handle(stream), _dptr(key_base), _dptr(key_off),
                                                   _dptr(key_len), _dptr(blk_off), _dptr(blk_len), _dptr(keep), count,
                                                   _dptr(dst), dst_bytes, _dptr(data_end), _dptr(index_len),
                                                   _dptr(table_bytes), _dptr(status)), "kvsep_sst_table_finish_device")
        return status

    def sst_table_rewrite_device(self, file_base, n, dst, dst_bytes, off, length, key_off, key_len, crc, ok, dst_off,
                                 nblocks, handles, status, index_len, table_bytes, wstatus, nkept=None, cap=None,
                                 max_len_hint=0, stream=None):
        """kvsep_sst_table_rewrite_device: the n-byte device table image at file_base without its bad blocks, as a
        table, in dst: sst_table_verify_device with the keys walk, the salvage copy of the data blocks that passed, then
        sst_table_finish_device with the new handles.  off / length / key_off / key_len / dst_off (int64), crc (int32)
        and ok (uint8) have cap slots; status is the source's SST_* code, wstatus a SSTW_* code."""
        if cap is None:
            cap = min(int(t.numel()) for t in (off, length, key_off, key_len, crc, ok, dst_off))
        _check(lib().kvsep_sst_table_rewrite_device(self._h, _stream_handle(stream), _dptr(file_base), n, _dptr(dst),
                                                    dst_bytes, _dptr(off), _dptr(length), _dptr(key_off),
                                                    _dptr(key_len), _dptr(crc), _dptr(ok), _dptr(dst_off), cap,
                                                    max_len_hint, _dptr(nblocks), _dptr(nkept), _dptr(handles),
                                                    _dptr(status), _dptr(index_len), _dptr(table_bytes),
                                                    _dptr(wstatus)), "kvsep_sst_table_rewrite_device")
        return wstatus

    def log_accept_gaps_device(self, base, n, off, length, type, ok, nrec, accept, gap=None, dropped=None,
                               bad_length=None, cap=None, stream=None):
        """kvsep_log_accept_gaps_device: log_accept_gaps over the device image and the arrays log_walk_device wrote,
        with the verdicts ok (uint8, cap bytes).  accept / gap (uint8) are written for cap elements; dropped /
        bad_length are one-element int64 device tensors."""
        cap = int(ok.numel()) if cap is None else cap
        _check(lib().kvsep_log_accept_gaps_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off),
                                                  _dptr(length), _dptr(type), _dptr(ok), _dptr(nrec), cap,
                                                  _dptr(accept), _dptr(gap), _dptr(dropped), _dptr(bad_length)),
               "kvsep_log_accept_gaps_device")
        return accept

    def log_read_device(self, base, n, off, length, stored, type, ok, accept, nrec, gap=None, dropped=None,
                        bad_length=None, cap=None, stream=None):
        """kvsep_log_read_device: log_walk_device, log_verify_device over all cap elements and log_accept_gaps_device,
        chained on one stream with no host step."""
        cap = int(ok.numel()) if cap is None else cap
        _check(lib().kvsep_log_read_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off), _dptr(length),
                                           _dptr(stored), _dptr(type), _dptr(ok), _dptr(accept), _dptr(gap), cap,
                                           _dptr(nrec), _dptr(dropped), _dptr(bad_length)), "kvsep_log_read_device")
        return accept

    def vlog_walk_device(self, base, n, nrec, off=None, length=None, stored=None, consumed=None, cap=None,
                         stream=None):
        """kvsep_vlog_walk_device: the walk of vlog_walk over the n bytes of the device image at base.  nrec and
        consumed (one-element int64 device tensors, consumed optional) receive the record count and the end of the last
        complete record; off / length (int64) and stored (int32), each optional, are written for exactly cap elements:
        the records first, then padding (off = length = 0, stored = mask(0)).  With no array cap is 0: the counting
        call."""
        if cap is None:
            cap = min([int(t.numel()) for t in (off, length, stored) if t is not None and not isinstance(t, int)],
                      default=0)
        _check(lib().kvsep_vlog_walk_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off), _dptr(length),
                                            _dptr(stored), cap, _dptr(nrec), _dptr(consumed)), "kvsep_vlog_walk_device")
        return nrec

    def vlog_read_device(self, base, n, off, length, stored, crc, nrec, ok=None, consumed=None, first_bad=None,
                         nbad=None, ngood=None, good_bytes=None, drop_bytes=None, cap=None, max_len_hint=0,
                         stream=None):
        """kvsep_vlog_read_device: vlog_walk_device, verify_device over all cap elements (the ok[] pass of the list form
        when ok, uint8, is given) and the totals of vlog_verify_host, chained on one stream with no host step.  crc is
        an int32 device tensor of cap elements; the result words are one-element int64 device tensors."""
        if cap is None:
            cap = min(int(t.numel()) for t in (off, length, stored, crc))
        _check(lib().kvsep_vlog_read_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off), _dptr(length),
                                            _dptr(stored), _dptr(crc), _dptr(ok), cap, max_len_hint, _dptr(nrec),
                                            _dptr(consumed), _dptr(first_bad), _dptr(nbad), _dptr(ngood),
                                            _dptr(good_bytes), _dptr(drop_bytes)), "kvsep_vlog_read_device")
        return nrec

    def log_chains_device(self, type, accept, nrec, first, whole, nchain, gap=None, off=None, length=None,
                          frag_off=None, frag_len=None, nwhole=None, cap=None, stream=None):
        """kvsep_log_chains_device: log_chains over the arrays the device reader wrote, count = min(nrec, cap).  first
        (int64, cap + 1 elements) and whole (uint8, cap) are written in full; off / length / frag_off / frag_len
        (int64, cap) go together: frag_* receive the records' payload descriptors.  nrec, nchain and nwhole are
        one-element int64 device tensors."""
        cap = int(whole.numel()) if cap is None else cap
        _check(lib().kvsep_log_chains_device(self._h, _stream_handle(stream), _dptr(type), _dptr(accept), _dptr(gap),
                                             _dptr(off), _dptr(length), _dptr(nrec), cap, _dptr(first), _dptr(whole),
                                             _dptr(frag_off), _dptr(frag_len), _dptr(nchain), _dptr(nwhole)),
               "kvsep_log_chains_device")
        return first, whole

    def log_records_device(self, base, n, off, length, stored, type, ok, accept, gap, nrec, frag_off, frag_len, first,
                           whole, nchain, dst, dst_bytes, rec_off, end, rec_len=None, nwhole=None, dropped=None,
                           bad_length=None, cap=None, stream=None):
        """kvsep_log_records_device: log_read_device, log_chains_device, the offsets pass over the chains (keep = whole)
        and the gather-copy, chained on one stream with no host step: dst receives the records log::Reader returns, back
        to back from offset 0; rec_off / rec_len (int64, cap) say where each chain's record went and how long it is."""
        cap = int(ok.numel()) if cap is None else cap
        _check(lib().kvsep_log_records_device(self._h, _stream_handle(stream), _dptr(base), n, _dptr(off),
                                              _dptr(length), _dptr(stored), _dptr(type), _dptr(ok), _dptr(accept),
                                              _dptr(gap), cap, _dptr(nrec), _dptr(dropped), _dptr(bad_length),
                                              _dptr(frag_off), _dptr(frag_len), _dptr(first), _dptr(whole),
                                              _dptr(nchain), _dptr(dst), dst_bytes, _dptr(rec_off), _dptr(rec_len),
                                              _dptr(end), _dptr(nwhole)), "kvsep_log_records_device")
        return dst

    def log_frame_device(self, base, off, length, dest_length, dst, dst_bytes, rec_at, frag_first, frag_off, frag_len,
                         frag_at, frag_type, frag_crc, nfrag, written, keep=None, count=None, frag_cap=None,
                         total_bytes=0, stream=None):
        """kvsep_log_frame_device: the records [base + off[i], + length[i]) with keep[i] != 0 (keep optional), appended
        to a log of dest_length bytes the way log::Writer::AddRecord does, into dst from offset 0, with no host step.
        rec_at (int64, count) and frag_first (int64, count + 1) are log_frame_layout's; frag_off / frag_len / frag_at
        (int64), frag_type (uint8) and frag_crc (int32) describe the physical records and are written for exactly
        frag_cap elements; nfrag and written are one-element int64 device tensors.  rec_off / rec_len / whole of
        log_records_device go in as off / length / keep."""
        count = int(length.numel()) if count is None else count
        frag_cap = int(frag_type.numel()) if frag_cap is None else frag_cap
        _check(lib().kvsep_log_frame_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off), _dptr(length),
                                            _dptr(keep), count, dest_length, _dptr(dst), dst_bytes, _dptr(rec_at),
                                            _dptr(frag_first), _dptr(frag_off), _dptr(frag_len), _dptr(frag_at),
                                            _dptr(frag_type), _dptr(frag_crc), frag_cap, _dptr(nfrag), _dptr(written),
                                            total_bytes), "kvsep_log_frame_device")
        return dst

    def concat_device(self, seg_crc, seg_len, first, out, init=None, count=None, nseg=None, stream=None):
        """kvsep_crc32c_concat_device: out[i] = the fold of combine over segments [first[i], first[i + 1]) of seg_crc /
        seg_len, starting at init[i] (0 without init).  Device tensors (or addresses, then count and nseg are needed);
        first has count + 1 entries."""
        count = int(first.numel()) - 1 if count is None else count
        nseg = int(seg_len.numel()) if nseg is None else nseg
        _check(lib().kvsep_crc32c_concat_device(self._h, _stream_handle(stream), _dptr(seg_crc), _dptr(seg_len),
                                                _dptr(first), _dptr(init), _dptr(out), count, nseg),
               "kvsep_crc32c_concat_device")
        return out

    def gather_device(self, base, seg_off, seg_len, first, seg_crc, out, init=None, count=None, nseg=None,
                      total_bytes=None, max_len=0, stream=None):
        """kvsep_crc32c_gather_device: out[i] = Extend(init[i], the segments [first[i], first[i + 1]) of base back to
        back); seg_crc (nseg words) receives every segment's Value.  total_bytes / max_len: the hints of batch_device
        over the segments."""
        count = int(first.numel()) - 1 if count is None else count
        nseg = int(seg_len.numel()) if nseg is None else nseg
        if total_bytes is None:
            total_bytes = int(seg_len.sum().item()) if nseg else 0
        _check(lib().kvsep_crc32c_gather_device(self._h, _stream_handle(stream), _dptr(base), _dptr(seg_off),
                                                _dptr(seg_len), _dptr(first), _dptr(init), _dptr(seg_crc), _dptr(out),
                                                count, nseg, total_bytes, max_len), "kvsep_crc32c_gather_device")
        return out

    def pack_device(self, base, seg_off, seg_len, first, dst, dst_bytes, dst_off, count=None, nseg=None, stream=None):
        """kvsep_crc32c_pack_device: the bytes of segments [first[i], first[i + 1]) of base go back to back to dst +
        dst_off[i], byte-exact; a block that does not lie inside [0, dst_bytes) is not written.  Device tensors (or
        addresses, then count and nseg are needed); first has count + 1 entries."""
        count = int(first.numel()) - 1 if count is None else count
        nseg = int(seg_len.numel()) if nseg is None else nseg
        _check(lib().kvsep_crc32c_pack_device(self._h, _stream_handle(stream), _dptr(base), _dptr(seg_off),
                                              _dptr(seg_len), _dptr(first), _dptr(dst), dst_bytes, _dptr(dst_off),
                                              count, nseg), "kvsep_crc32c_pack_device")
        return dst

    def vlog_frame_device(self, base, seg_off, seg_len, first, seg_crc, crc_out, dst, dst_bytes, rec_off, count=None,
                          nseg=None, total_bytes=None, max_len=0, stream=None):
        """kvsep_vlog_frame_device: gather_device without init (seg_crc, crc_out = Value of every segment / payload),
        then dst + rec_off[i] = [Mask(crc_out[i])][len_i][payload i] (db/value_log_writer.cc:46-76); rec_off from
        vlog_frame_offsets.  total_bytes / max_len: the hints of batch_device over the segments."""
        count = int(first.numel()) - 1 if count is None else count
        nseg = int(seg_len.numel()) if nseg is None else nseg
        if total_bytes is None:
            total_bytes = int(seg_len.sum().item()) if nseg else 0
        _check(lib().kvsep_vlog_frame_device(self._h, _stream_handle(stream), _dptr(base), _dptr(seg_off),
                                             _dptr(seg_len), _dptr(first), _dptr(seg_crc), _dptr(crc_out), _dptr(dst),
                                             dst_bytes, _dptr(rec_off), count, nseg, total_bytes, max_len),
               "kvsep_vlog_frame_device")
        return dst

    def sst_frame_device(self, base, off, length, types, masked_out, dst, dst_bytes, blk_off, count=None,
                         total_bytes=None, max_len=0, stream=None):
        """kvsep_sst_frame_device: sst_trailers_device (masked_out), then dst + blk_off[i] = [block i][types[i]]
        [masked_out[i] LE32] (table/table_builder.cc:209-232)."""
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_sst_frame_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off), _dptr(length),
                                            _dptr(types), _dptr(masked_out), _dptr(dst), dst_bytes, _dptr(blk_off),
                                            count, total_bytes, max_len), "kvsep_sst_frame_device")
        return dst

    def offsets_device(self, seg_len, dst_off, end, first=None, keep=None, keep_before=None, head=0, tail=0, start=0,
                       nkept=None, count=None, nseg=None, stream=None):
        """kvsep_crc32c_offsets_device: dst_off[i] = start + the (head + size + tail) of the kept blocks before i, or
        OFFSET_SKIP for a dropped block; end / nkept (one-element uint64 / int64 device tensors) the layout's end and
        the number of kept blocks.  keep: uint8 device tensor (keep[i] != 0); keep_before: one-element device tensor
        (i < its value); at most one of them.  Without first, block i is segment i."""
        nseg = int(seg_len.numel()) if nseg is None else nseg
        if count is None:
            count = int(first.numel()) - 1 if first is not None else nseg
        _check(lib().kvsep_crc32c_offsets_device(self._h, _stream_handle(stream), _dptr(seg_len), _dptr(first),
                                                 _dptr(keep), _dptr(keep_before), head, tail, start, _dptr(dst_off),
                                                 _dptr(end), _dptr(nkept), count, nseg),
               "kvsep_crc32c_offsets_device")
        return dst_off

    def salvage_device(self, base, off, length, dst, dst_bytes, dst_off, end, keep=None, keep_before=None, nkept=None,
                       count=None, stream=None):
        """kvsep_crc32c_salvage_device: the kept blocks of base go back to back to dst from offset 0 (offsets_device,
        then pack_device with the dst_off it wrote)."""
        count = int(off.numel()) if count is None else count
        _check(lib().kvsep_crc32c_salvage_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off),
                                                 _dptr(length), _dptr(keep), _dptr(keep_before), _dptr(dst), dst_bytes,
                                                 _dptr(dst_off), _dptr(end), _dptr(nkept), count),
               "kvsep_crc32c_salvage_device")
        return dst

    def sst_salvage_device(self, file_base, off, length, out, ok, dst, dst_bytes, dst_off, end, first_bad=None,
                           nbad=None, nkept=None, count=None, total_bytes=None, max_len=0, stream=None):
        """kvsep_sst_salvage_device: the SST read check with ok[], then the passed blocks with their 5-byte trailers
        contiguous in dst; dst_off[i] where block i went (OFFSET_SKIP: it failed)."""
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_sst_salvage_device(self._h, _stream_handle(stream), _dptr(file_base), _dptr(off),
                                              _dptr(length), _dptr(out), _dptr(first_bad), _dptr(nbad), _dptr(ok),
                                              _dptr(dst), dst_bytes, _dptr(dst_off), _dptr(end), _dptr(nkept), count,
                                              total_bytes, max_len), "kvsep_sst_salvage_device")
        return dst

    def vlog_frame_auto_device(self, base, seg_off, seg_len, first, seg_crc, crc_out, dst, dst_bytes, rec_off, end,
                               start=0, count=None, nseg=None, total_bytes=None, max_len=0, stream=None):
        """kvsep_vlog_frame_auto_device: vlog_frame_device with rec_off (an output here) and end computed on the
        device, records back to back from `start`."""
        count = int(first.numel()) - 1 if count is None else count
        nseg = int(seg_len.numel()) if nseg is None else nseg
        if total_bytes is None:
            total_bytes = int(seg_len.sum().item()) if nseg else 0
        _check(lib().kvsep_vlog_frame_auto_device(self._h, _stream_handle(stream), _dptr(base), _dptr(seg_off),
                                                  _dptr(seg_len), _dptr(first), _dptr(seg_crc), _dptr(crc_out),
                                                  _dptr(dst), dst_bytes, start, _dptr(rec_off), _dptr(end), count, nseg,
                                                  total_bytes, max_len), "kvsep_vlog_frame_auto_device")
        return dst

    def stream_read(self, src, nbytes: int, sink, stream=None):
        _check(lib().kvsep_stream_read_device(self._h, _stream_handle(stream), _dptr(src), nbytes, _dptr(sink)),
               "kvsep_stream_read_device")

    # -- host forms (numpy / bytes)
    def batch_host_span(self, buf, off, length, init=None):
        p, keep = _buf(buf)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        out = np.zeros(off.size, dtype=np.uint32)
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.uint32)
            ip = init.ctypes.data_as(ctypes.c_void_p)
        _check(lib().kvsep_crc32c_batch_host_span(self._h, p, keep.nbytes, off.ctypes.data_as(ctypes.c_void_p),
                                                  length.ctypes.data_as(ctypes.c_void_p), ip,
                                                  out.ctypes.data_as(ctypes.c_void_p), off.size),
               "kvsep_crc32c_batch_host_span")
        return out

    def batch_host(self, blocks, init=None):
        """blocks: list of bytes-like objects (gathered through pinned staging)."""
        keep = [_buf(b) for b in blocks]
        n = len(blocks)
        ptrs = (ctypes.c_void_p * n)(*[k[0].value for k in keep])
        lens = np.array([k[1].nbytes for k in keep], dtype=np.uint64)
        out = np.zeros(n, dtype=np.uint32)
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.uint32)
            ip = init.ctypes.data_as(ctypes.c_void_p)
        _check(lib().kvsep_crc32c_batch_host(self._h, ip, ptrs, lens.ctypes.data_as(ctypes.c_void_p),
                                             out.ctypes.data_as(ctypes.c_void_p), n), "kvsep_crc32c_batch_host")
        return out

    def gather_host(self, segments, first, init=None):
        """kvsep_crc32c_gather_host: segments = list of bytes-like objects; block i is segments [first[i],
        first[i + 1]) back to back -> uint32 array of len(first) - 1 CRCs."""
        keep = [_buf(b) for b in segments]
        n = len(segments)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k[0].value for k in keep])
        lens = np.array([k[1].nbytes for k in keep], dtype=np.uint64)
        first = np.ascontiguousarray(first, dtype=np.uint64)
        count = first.size - 1
        out = np.zeros(max(count, 1), dtype=np.uint32)
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.uint32)
            ip = init.ctypes.data_as(ctypes.c_void_p)
        vp = ctypes.c_void_p
        _check(lib().kvsep_crc32c_gather_host(self._h, ip, ptrs, lens.ctypes.data_as(vp), first.ctypes.data_as(vp),
                                              out.ctypes.data_as(vp), count, n), "kvsep_crc32c_gather_host")
        return out[:count]

    # -- framings (vlog / log / SST call sites)
    def vlog_verify(self, image, with_drop=False):
        """db/value_log_reader.cc:86-138 over a whole vlog image -> (records, good, good_bytes), plus the byte count
        reported with "checksum mismatch" (0 if none) when with_drop."""
        p, keep = _buf(image)
        n, g, gb, dr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().kvsep_vlog_verify_host(self._h, p, keep.nbytes, ctypes.byref(n), ctypes.byref(g),
                                            ctypes.byref(gb), ctypes.byref(dr)), "kvsep_vlog_verify_host")
        return (n.value, g.value, gb.value, dr.value) if with_drop else (n.value, g.value, gb.value)

    def vlog_frame(self, payloads, out=None):
        """db/value_log_writer.cc:46-76 for a batch of payloads -> bytes of the framed records; with `out` (a
        writable uint8 numpy array of >= sum(8 + len) bytes) the records are framed into it and the byte count
        is returned instead."""
        keep = [_buf(b) for b in payloads]
        k = len(payloads)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[x[0].value for x in keep])
        lens = np.array([x[1].nbytes for x in keep], dtype=np.uint64)
        need = int(lens.sum()) + 8 * k
        dst = np.zeros(max(need, 1), dtype=np.uint8) if out is None else out
        w = ctypes.c_uint64()
        _check(lib().kvsep_vlog_frame_host(self._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p), k,
                                           dst.ctypes.data_as(ctypes.c_void_p), dst.nbytes, ctypes.byref(w)),
               "kvsep_vlog_frame_host")
        return dst[:w.value].tobytes() if out is None else w.value

    def log_frame(self, records, dest_length: int = 0, out=None):
        """db/log_writer.cc:35-115: AddRecord of each record onto a log of length dest_length -> appended bytes;
        with `out` (a writable uint8 numpy array, large enough) they are written into it and the count returned."""
        keep = [_buf(b) for b in records]
        k = len(records)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[x[0].value for x in keep])
        lens = np.array([x[1].nbytes for x in keep], dtype=np.uint64)
        w = ctypes.c_uint64()
        if out is None:
            lib().kvsep_log_frame_host(self._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p), k, dest_length, None, 0,
                                       ctypes.byref(w))  # sizing call: *written even when dst is short
        dst = np.zeros(max(w.value, 1), dtype=np.uint8) if out is None else out
        _check(lib().kvsep_log_frame_host(self._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p), k, dest_length,
                                          dst.ctypes.data_as(ctypes.c_void_p), dst.nbytes, ctypes.byref(w)),
               "kvsep_log_frame_host")
        return dst[:w.value].tobytes() if out is None else w.value

    def frame_raw(self, kind: str, addrs, lens, out, dest_length: int = 0) -> int:
        """The framing writers on prebuilt arrays: addrs = uint64 host addresses of the payloads, lens = their
        uint64 lengths, out = a writable uint8 numpy array (kind "vlog" or "log").  No per-record Python work,
        so a caller framing thousands of records pays only the C-ABI call.  Returns the bytes written."""
        addrs = np.ascontiguousarray(addrs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        w = ctypes.c_uint64()
        vp = ctypes.c_void_p
        if kind == "vlog":
            rc = lib().kvsep_vlog_frame_host(self._h, addrs.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size,
                                             out.ctypes.data_as(vp), out.nbytes, ctypes.byref(w))
        else:
            rc = lib().kvsep_log_frame_host(self._h, addrs.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size,
                                            dest_length, out.ctypes.data_as(vp), out.nbytes, ctypes.byref(w))
        _check(rc, f"kvsep_{kind}_frame_host")
        return w.value

    def log_verify(self, image):
        """db/log_reader.cc:246-259 per physical record of a log/MANIFEST image -> array of 0/1."""
        p, keep = _buf(image)
        cnt = log_walk(image)[0].size
        ok = np.zeros(max(cnt, 1), dtype=np.uint8)
        n = ctypes.c_uint64()
        _check(lib().kvsep_log_verify_host(self._h, p, keep.nbytes, ok.ctypes.data_as(ctypes.c_void_p), ok.size,
                                           ctypes.byref(n)), "kvsep_log_verify_host")
        return ok[:n.value]

    def sst_trailers_device(self, base, off, length, types, masked_out, count=None, total_bytes=None, max_len=0,
                            stream=None):
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_sst_trailers_device(self._h, _stream_handle(stream), _dptr(base), _dptr(off),
                                               _dptr(length), _dptr(types), _dptr(masked_out), count, total_bytes,
                                               max_len), "kvsep_sst_trailers_device")

    def sst_verify_device(self, file_base, off, length, out, first_bad, nbad, count=None, total_bytes=None,
                          max_len=0, stream=None):
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        _check(lib().kvsep_sst_verify_device(self._h, _stream_handle(stream), _dptr(file_base), _dptr(off),
                                             _dptr(length), _dptr(out), _dptr(first_bad), _dptr(nbad), count,
                                             total_bytes, max_len), "kvsep_sst_verify_device")

    def sst_verify_list_device(self, file_base, off, length, out, first_bad, nbad, bad_idx=None, bad_cap=None, ok=None,
                               count=None, total_bytes=None, max_len=0, stream=None):
        """sst_verify_device, then the list pass (kvsep_sst_verify_list_device): the call for RepairDB::ScanTable and
        paranoid reads.  bad_idx / bad_cap / ok as in verify_list_device."""
        count = int(off.numel()) if count is None else count
        if total_bytes is None:
            total_bytes = int(length.sum().item()) if count else 0
        if bad_cap is None:
            bad_cap = 0 if bad_idx is None else int(bad_idx.numel())
        _check(lib().kvsep_sst_verify_list_device(self._h, _stream_handle(stream), _dptr(file_base), _dptr(off),
                                                  _dptr(length), _dptr(out), _dptr(first_bad), _dptr(nbad),
                                                  _dptr(bad_idx), bad_cap, _dptr(ok), count, total_bytes, max_len),
               "kvsep_sst_verify_list_device")

    def sst_verify_list(self, image, off, length, bad_cap=None):
        """sst_verify plus the bad blocks' indices (kvsep_sst_verify_list_host) -> (out, first_bad, nbad, bad): bad =
        the first min(nbad, bad_cap) mismatching handles, ascending (bad_cap defaults to every handle)."""
        p, keep = _buf(image)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        if off.size != length.size:
            raise ValueError("off and length must have the same length")
        k = off.size
        bad_cap = k if bad_cap is None else int(bad_cap)
        out = np.zeros(max(k, 1), dtype=np.uint32)
        bad = np.zeros(max(bad_cap, 1), dtype=np.uint64)
        fb, nb = ctypes.c_uint64(), ctypes.c_uint64()
        vp = ctypes.c_void_p
        _check(lib().kvsep_sst_verify_list_host(self._h, p, keep.nbytes, off.ctypes.data_as(vp),
                                                length.ctypes.data_as(vp), out.ctypes.data_as(vp), ctypes.byref(fb),
                                                ctypes.byref(nb), bad.ctypes.data_as(vp) if bad_cap else None, bad_cap,
                                                k), "kvsep_sst_verify_list_host")
        first = -1 if fb.value == 0xFFFFFFFFFFFFFFFF else fb.value
        return out[:k], first, nb.value, bad[:min(nb.value, bad_cap)]

    def sst_trailers(self, blocks, types):
        """table/table_builder.cc:209-232 for host-resident blocks -> uint32 trailer words
        Mask(Extend(Value(block), &type, 1)) (kvsep_sst_trailers_host)."""
        keep = [_buf(b) for b in blocks]
        k = len(blocks)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[x[0].value for x in keep])
        lens = np.array([x[1].nbytes for x in keep], dtype=np.uint64)
        t = np.ascontiguousarray(types, dtype=np.uint8)
        if t.size != k:
            raise ValueError("blocks and types must have the same length")
        out = np.zeros(max(k, 1), dtype=np.uint32)
        _check(lib().kvsep_sst_trailers_host(self._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p),
                                             t.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), k),
               "kvsep_sst_trailers_host")
        return out[:k]

    def sst_trailers_raw(self, addrs, lens, types, out):
        """kvsep_sst_trailers_host on prebuilt arrays: addrs = uint64 host addresses of the blocks, lens their uint64
        lengths, types uint8, out a uint32 array filled with the trailer words.  No per-block Python work."""
        addrs = np.ascontiguousarray(addrs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        t = np.ascontiguousarray(types, dtype=np.uint8)
        if addrs.size != lens.size or t.size != lens.size:
            raise ValueError("addrs, lens and types must have the same length")
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous
                and out.size >= lens.size):
            raise ValueError("out must be a contiguous uint32 array with room for every block")
        vp = ctypes.c_void_p
        _check(lib().kvsep_sst_trailers_host(self._h, addrs.ctypes.data_as(vp), lens.ctypes.data_as(vp),
                                             t.ctypes.data_as(vp), out.ctypes.data_as(vp), lens.size),
               "kvsep_sst_trailers_host")
        return out

    def sst_verify(self, image, off, length):
        """table/format.cc:73-108 for every block handle (off, length) of a host SST file image -> (out, first_bad,
        nbad): out[i] = Value(block, len + 1); first_bad = -1 when every block matches its stored trailer word."""
        p, keep = _buf(image)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        if off.size != length.size:
            raise ValueError("off and length must have the same length")
        k = off.size
        out = np.zeros(max(k, 1), dtype=np.uint32)
        fb, nb = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().kvsep_sst_verify_host(self._h, p, keep.nbytes, off.ctypes.data_as(ctypes.c_void_p),
                                           length.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(fb), ctypes.byref(nb), k), "kvsep_sst_verify_host")
        first = -1 if fb.value == 0xFFFFFFFFFFFFFFFF else fb.value
        return out[:k], first, nb.value


def vlog_walk(image):
    """Header walk of a vlog image (db/value_log_reader.cc:86-108) -> (off, len, stored, consumed)."""
    p, keep = _buf(image)
    cnt = lib().kvsep_vlog_walk(p, keep.nbytes, None, None, None, 0, None)
    off = np.zeros(cnt, np.uint64)
    ln = np.zeros(cnt, np.uint64)
    st = np.zeros(cnt, np.uint32)
    used = ctypes.c_uint64()
    lib().kvsep_vlog_walk(p, keep.nbytes, off.ctypes.data_as(ctypes.c_void_p), ln.ctypes.data_as(ctypes.c_void_p),
                          st.ctypes.data_as(ctypes.c_void_p), cnt, ctypes.byref(used))
    return off, ln, st, used.value


def vlog_frame_offsets(lens, start: int = 0):
    """kvsep_vlog_frame_offsets: (rec_off, end) of vlog records of these payload lengths laid back to back from
    `start`: rec_off[i] = start + sum(8 + lens[:i]), end = start + sum(8 + lens).  Host only; raises for a length over
    2**32 - 1 or offsets that leave 64 bits."""
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    rec_off = np.zeros(lens.size, np.uint64)
    end = ctypes.c_uint64()
    vp = ctypes.c_void_p
    _check(lib().kvsep_vlog_frame_offsets(lens.ctypes.data_as(vp), lens.size, start, rec_off.ctypes.data_as(vp),
                                          ctypes.byref(end)), "kvsep_vlog_frame_offsets")
    return rec_off, end.value


def log_walk(image):
    """Physical-record walk of a log/MANIFEST image (db/log_reader.cc:189-272) -> (off, len, stored, type)."""
    p, keep = _buf(image)
    cnt = lib().kvsep_log_walk(p, keep.nbytes, None, None, None, None, 0)
    off = np.zeros(cnt, np.uint64)
    ln = np.zeros(cnt, np.uint64)
    st = np.zeros(cnt, np.uint32)
    ty = np.zeros(cnt, np.uint8)
    lib().kvsep_log_walk(p, keep.nbytes, off.ctypes.data_as(ctypes.c_void_p), ln.ctypes.data_as(ctypes.c_void_p),
                         st.ctypes.data_as(ctypes.c_void_p), ty.ctypes.data_as(ctypes.c_void_p), cnt)
    return off, ln, st, ty


SST_OK, SST_BAD_FOOTER, SST_INDEX_CHECKSUM, SST_INDEX_COMPRESSED = 0, 1, 2, 3
SST_BAD_RESTARTS, SST_BAD_ENTRY, SST_BAD_HANDLE, SST_CAP = 4, 5, 6, 7
SST_SHARED_KEY = 8
SSTW_OK, SSTW_TOO_LARGE, SSTW_NO_ROOM, SSTW_SOURCE = 0, 1, 2, 3
OFFSET_SKIP = 0xFFFFFFFFFFFFFFFF


def sst_footer(image):
    """Footer of an SST image (table/format.cc:37-60) -> ((meta_off, meta_len, index_off, index_len), status)."""
    p, keep = _buf(image)
    h = np.zeros(4, np.uint64)
    st = ctypes.c_uint32()
    _check(lib().kvsep_sst_footer(p, keep.nbytes, h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st)),
           "kvsep_sst_footer")
    return tuple(int(x) for x in h), st.value


def sst_index_walk(block, cap=None):
    """Walk of one index block's contents (table/block.cc) -> (off, len, nblocks, status).  With cap the arrays have cap
    elements (zeros after the handles) and nblocks is still the full count; without it they hold every handle."""
    p, keep = _buf(block)
    vp = ctypes.c_void_p
    nb, st = ctypes.c_uint64(), ctypes.c_uint32()
    if cap is None:
        _check(lib().kvsep_sst_index_walk(p, keep.nbytes, None, None, 0, ctypes.byref(nb), ctypes.byref(st)),
               "kvsep_sst_index_walk")
        cap = nb.value
    off = np.zeros(max(cap, 1), np.uint64)
    ln = np.zeros(max(cap, 1), np.uint64)
    _check(lib().kvsep_sst_index_walk(p, keep.nbytes, off.ctypes.data_as(vp), ln.ctypes.data_as(vp), cap,
                                      ctypes.byref(nb), ctypes.byref(st)), "kvsep_sst_index_walk")
    return off[:cap], ln[:cap], nb.value, st.value


def sst_index_keys(block, cap=None):
    """sst_index_walk with keys (kvsep_sst_index_keys) -> (off, len, key_off, key_len, nblocks, status): key_off[i] /
    key_len[i] say where entry i's key bytes lie in the block.  SST_SHARED_KEY at an entry that shares key bytes."""
    p, keep = _buf(block)
    vp = ctypes.c_void_p
    nb, st = ctypes.c_uint64(), ctypes.c_uint32()
    if cap is None:
        _check(lib().kvsep_sst_index_keys(p, keep.nbytes, None, None, None, None, 0, ctypes.byref(nb),
                                          ctypes.byref(st)), "kvsep_sst_index_keys")
        cap = nb.value
    a = [np.zeros(max(cap, 1), np.uint64) for _ in range(4)]
    _check(lib().kvsep_sst_index_keys(p, keep.nbytes, *[x.ctypes.data_as(vp) for x in a], cap, ctypes.byref(nb),
                                      ctypes.byref(st)), "kvsep_sst_index_keys")
    return a[0][:cap], a[1][:cap], a[2][:cap], a[3][:cap], nb.value, st.value


def sst_index_build(key_base, key_off, key_len, blk_off, blk_len, keep=None, dst=None, at: int = 0):
    """The index block of the kept entries with its trailer (kvsep_sst_index_build) -> (bytes, out_len, status).
    Without dst the block is sized first and returned on its own (block + 5 bytes; empty after a refusal); with dst (a
    uint8 array) it is written at dst[at:] and dst is returned."""
    p, hold = _buf(key_base)
    vp = ctypes.c_void_p
    arrs = [np.ascontiguousarray(x, np.uint64) for x in (key_off, key_len, blk_off, blk_len)]
    count = len(arrs[0])
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    ol, st = ctypes.c_uint64(), ctypes.c_uint32()

    def call(d, nbytes, where):
        _check(lib().kvsep_sst_index_build(p, *[x.ctypes.data_as(vp) for x in arrs],
                                           None if k is None else k.ctypes.data_as(vp), count, d.ctypes.data_as(vp),
                                           nbytes, where, ctypes.byref(ol), ctypes.byref(st)), "kvsep_sst_index_build")

    if dst is not None:
        call(dst, dst.nbytes, at)
        return dst, ol.value, st.value
    probe = np.zeros(1, np.uint8)
    call(probe, 0, 0)  # no room: *out_len is the needed length
    if st.value != SSTW_NO_ROOM:
        return b"", ol.value, st.value
    out = np.zeros(ol.value + 5, np.uint8)
    call(out, out.nbytes, 0)
    return out.tobytes(), ol.value, st.value


def sst_footer_build(meta, index) -> bytes:
    """Footer::EncodeTo (kvsep_sst_footer_build): meta / index = (off, len) -> the 48 bytes."""
    out = np.zeros(48, np.uint8)
    _check(lib().kvsep_sst_footer_build(meta[0], meta[1], index[0], index[1], out.ctypes.data_as(ctypes.c_void_p)),
           "kvsep_sst_footer_build")
    return out.tobytes()


def log_accept(off, ok, n: int):
    """log::Reader acceptance (db/log_reader.cc:250-258) from the walk and per-record checksum verdicts ->
    (accept 0/1 array, bytes reported dropped with "checksum mismatch")."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    acc = np.zeros(max(off.size, 1), np.uint8)
    dropped = lib().kvsep_log_accept(off.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p),
                                     off.size, n, acc.ctypes.data_as(ctypes.c_void_p))
    return acc[:off.size], int(dropped)


def log_accept_gaps(image, ok):
    """kvsep_log_accept_gaps over the host image log_walk walked and its records' checksum verdicts -> (accept, gap,
    bytes reported with "checksum mismatch", bytes reported with "bad record length"); gap[i] = 1 where the reader
    met a bad record length or a zero header between record i-1 and record i (reset the assembly there)."""
    p, keep = _buf(image)
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    acc = np.zeros(max(ok.size, 1), np.uint8)
    gap = np.zeros(max(ok.size, 1), np.uint8)
    bad_len = ctypes.c_uint64()
    dropped = lib().kvsep_log_accept_gaps(p, keep.nbytes, ok.ctypes.data_as(ctypes.c_void_p), ok.size,
                                          acc.ctypes.data_as(ctypes.c_void_p), gap.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.byref(bad_len))
    return acc[:ok.size], gap[:ok.size], int(dropped), int(bad_len.value)


def log_chains(type, accept, gap=None):
    """kvsep_log_chains: the chains of the physical records (type from log_walk, accept / gap from log_accept_gaps) ->
    (first, whole, nchain, nwhole).  first has count + 1 entries: chain j is the records [first[j], first[j + 1]), and
    first[nchain:] = count; whole[j] = 1 where chain j is a record log::Reader returns."""
    type = np.ascontiguousarray(type, dtype=np.uint8)
    accept = np.ascontiguousarray(accept, dtype=np.uint8)
    count = type.size
    if accept.size != count or (gap is not None and np.size(gap) != count):
        raise ValueError("type, accept and gap must have one element per record")
    vp = ctypes.c_void_p
    g = None if gap is None else np.ascontiguousarray(gap, dtype=np.uint8)
    first = np.zeros(count + 1, np.uint64)
    whole = np.zeros(max(count, 1), np.uint8)
    nwhole = ctypes.c_uint64()
    nchain = lib().kvsep_log_chains(type.ctypes.data_as(vp), accept.ctypes.data_as(vp),
                                    None if g is None else g.ctypes.data_as(vp), count, first.ctypes.data_as(vp),
                                    whole.ctypes.data_as(vp), ctypes.byref(nwhole))
    return first, whole[:count], int(nchain), int(nwhole.value)


def log_frame_layout(length, keep=None, dest_length=0):
    """kvsep_log_frame_layout: where log::Writer::AddRecord puts records of these lengths appended to a log of
    dest_length bytes -> (rec_at, frag_first, nfrag, written).  rec_at[i] = the offset of record i's first header from
    the first appended byte (OFFSET_SKIP where keep[i] == 0); frag_first has count + 1 entries: record i is the physical
    records [frag_first[i], frag_first[i + 1]); written = the appended bytes."""
    length = np.ascontiguousarray(length, dtype=np.uint64)
    count = length.size
    if keep is not None and np.size(keep) != count:
        raise ValueError("keep must have one element per record")
    vp = ctypes.c_void_p
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    rec_at = np.zeros(max(count, 1), np.uint64)
    frag_first = np.zeros(count + 1, np.uint64)
    nfrag, written = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().kvsep_log_frame_layout(length.ctypes.data_as(vp), None if k is None else k.ctypes.data_as(vp), count,
                                        dest_length, rec_at.ctypes.data_as(vp), frag_first.ctypes.data_as(vp),
                                        ctypes.byref(nfrag), ctypes.byref(written)), "kvsep_log_frame_layout")
    return rec_at[:count], frag_first, int(nfrag.value), int(written.value)


def partition(length, parts: int) -> np.ndarray:
    """kvsep_crc32c_partition: block-range bounds (parts + 1 entries) balanced by bytes."""
    length = np.ascontiguousarray(length, dtype=np.uint64)
    b = np.zeros(parts + 1, dtype=np.uint64)
    _check(lib().kvsep_crc32c_partition(length.ctypes.data_as(ctypes.c_void_p), length.size, parts,
                                        b.ctypes.data_as(ctypes.c_void_p)), "kvsep_crc32c_partition")
    return b


class Group:
    """Several devices in one process (kvsep_crc32c_group_*): one context and stream per listed device."""

    def __init__(self, devices):
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(lib().kvsep_crc32c_group_create(arr, len(devices), ctypes.byref(h)), "kvsep_crc32c_group_create")
        self._h = h
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_h", None):
            lib().kvsep_crc32c_group_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return lib().kvsep_crc32c_group_size(self._h)

    def batch_host_span(self, buf, off, length, init=None, expected_masked=None):
        """-> out, or (out, first_bad, nbad) with expected_masked."""
        p, keep = _buf(buf)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        out = np.zeros(off.size, dtype=np.uint32)
        vp = ctypes.c_void_p
        ip = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
        ipp = None if ip is None else ip.ctypes.data_as(vp)
        if expected_masked is None:
            _check(lib().kvsep_crc32c_group_batch_host_span(self._h, p, keep.nbytes, off.ctypes.data_as(vp),
                                                            length.ctypes.data_as(vp), ipp, out.ctypes.data_as(vp),
                                                            off.size), "kvsep_crc32c_group_batch_host_span")
            return out
        ex = np.ascontiguousarray(expected_masked, dtype=np.uint32)
        fb, nb = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().kvsep_crc32c_group_verify_host_span(self._h, p, keep.nbytes, off.ctypes.data_as(vp),
                                                         length.ctypes.data_as(vp), ipp, ex.ctypes.data_as(vp),
                                                         out.ctypes.data_as(vp), ctypes.byref(fb), ctypes.byref(nb),
                                                         off.size), "kvsep_crc32c_group_verify_host_span")
        return out, fb.value, nb.value

    def extend_host(self, init_crc: int, data, n: int | None = None) -> int:
        """Extend(init_crc, data[:n]) of ONE buffer, each member checksumming 1 / size() of it
        (kvsep_crc32c_group_extend_host)."""
        p, keep = _buf(data)
        n = _checked_len(keep, n)
        out = ctypes.c_uint32()
        _check(lib().kvsep_crc32c_group_extend_host(self._h, init_crc & 0xFFFFFFFF, p, n, ctypes.byref(out)),
               "kvsep_crc32c_group_extend_host")
        return out.value

    def vlog_verify(self, image):
        """kvsep_vlog_verify_host_group -> (records, good, good_bytes, drop_bytes)."""
        p, keep = _buf(image)
        v = [ctypes.c_uint64() for _ in range(4)]
        _check(lib().kvsep_vlog_verify_host_group(self._h, p, keep.nbytes, *[ctypes.byref(x) for x in v]),
               "kvsep_vlog_verify_host_group")
        return tuple(x.value for x in v)

    def batch_device(self, shards, expected_masked=None, index_base=None):
        """shards: per member a dict(base=, off=, len=, out=, [init=], total_bytes=, max_len=) of device tensors /
        addresses on that member's device.  -> None, or (first_bad, nbad) over all shards with expected_masked
        (per-member device arrays) and index_base (global index of each shard's first block)."""
        n = len(shards)
        P = ctypes.c_void_p * n
        U = ctypes.c_uint64 * n
        base = P(*[_dptr(s["base"]).value for s in shards])
        off = P(*[_dptr(s["off"]).value for s in shards])
        ln = P(*[_dptr(s["len"]).value for s in shards])
        out = P(*[_dptr(s["out"]).value for s in shards])
        init = P(*[_dptr(s.get("init")).value for s in shards])
        cnt = U(*[int(s["off"].numel()) for s in shards])
        tot = U(*[int(s["total_bytes"]) for s in shards])
        ml = U(*[int(s.get("max_len", 0)) for s in shards])
        if expected_masked is None:
            _check(lib().kvsep_crc32c_group_batch_device(self._h, base, off, ln, init, out, cnt, tot, ml),
                   "kvsep_crc32c_group_batch_device")
            return None
        ex = P(*[_dptr(e).value for e in expected_masked])
        ib = U(*[int(x) for x in index_base])
        fb, nb = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().kvsep_crc32c_group_verify_device(self._h, base, off, ln, init, ex, out, ib, cnt, tot, ml,
                                                      ctypes.byref(fb), ctypes.byref(nb)),
               "kvsep_crc32c_group_verify_device")
        return fb.value, nb.value

    def verify_list_device(self, shards, expected_masked, index_base, bad_cap):
        """batch_device's verify form plus the merged list (kvsep_crc32c_group_verify_list_device) -> (first_bad, nbad,
        bad): bad = the first min(nbad, bad_cap) mismatching global indices index_base[i] + k, ascending."""
        n = len(shards)
        P = ctypes.c_void_p * n
        U = ctypes.c_uint64 * n
        base = P(*[_dptr(s["base"]).value for s in shards])
        off = P(*[_dptr(s["off"]).value for s in shards])
        ln = P(*[_dptr(s["len"]).value for s in shards])
        out = P(*[_dptr(s["out"]).value for s in shards])
        init = P(*[_dptr(s.get("init")).value for s in shards])
        cnt = U(*[int(s["off"].numel()) for s in shards])
        tot = U(*[int(s["total_bytes"]) for s in shards])
        ml = U(*[int(s.get("max_len", 0)) for s in shards])
        ex = P(*[_dptr(e).value for e in expected_masked])
        ib = U(*[int(x) for x in index_base])
        bad = np.zeros(max(int(bad_cap), 1), dtype=np.uint64)
        fb, nb = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().kvsep_crc32c_group_verify_list_device(
            self._h, base, off, ln, init, ex, out, ib, cnt, tot, ml, ctypes.byref(fb), ctypes.byref(nb),
            bad.ctypes.data_as(ctypes.c_void_p) if bad_cap else None, int(bad_cap)),
            "kvsep_crc32c_group_verify_list_device")
        return fb.value, nb.value, bad[:min(nb.value, int(bad_cap))]


def fill_splitmix64(dst, nbytes: int, seed: int, stream_offset: int = 0, stream=None):
    """Device synthetic data (same stream as oracle_fill_splitmix64 / splitmix64_bytes below)."""
    _check(lib().kvsep_fill_splitmix64_device(_stream_handle(stream), _dptr(dst), nbytes, seed & (2**64 - 1),
                                              stream_offset), "kvsep_fill_splitmix64_device")


def splitmix64_bytes(nbytes: int, seed: int, stream_offset: int = 0) -> np.ndarray:
    """Host (numpy) version of the synthetic byte stream, for small test cases."""
    w0 = stream_offset >> 3
    w1 = (stream_offset + nbytes + 7) >> 3
    j = np.arange(w0, w1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (j + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    b = z.astype("<u8").view(np.uint8)
    s = stream_offset - (w0 << 3)
    return b[s:s + nbytes].copy()


def device_count() -> int:
    return lib().kvsep_device_count()


# ------------------------------------------------------------------ topology and host placement
def pci_bus_id(device: int) -> str:
    """PCI bus ID of a device, as sysfs spells it ("0000:75:00.0"; kvsep_device_pci_bus_id)."""
    buf = ctypes.create_string_buffer(64)
    _check(lib().kvsep_device_pci_bus_id(device, buf, 64), "kvsep_device_pci_bus_id")
    return buf.value.decode()


def pci_numa_node(bus_id: str) -> int:
    """NUMA node of a PCI function from sysfs (-1 unknown); no device needed."""
    return lib().kvsep_pci_numa_node(bus_id.encode())


def device_numa_node(device: int) -> int:
    return lib().kvsep_device_numa_node(device)


def numa_node_cpus(node: int) -> list:
    n = lib().kvsep_numa_node_cpus(node, None, 0)
    cpus = (ctypes.c_int * max(n, 1))()
    lib().kvsep_numa_node_cpus(node, cpus, n)
    return list(cpus[:n])


def bind_process_numa(node: int) -> int:
    """Every thread of this process onto the CPUs of `node` it may use, `node` the calling thread's preferred memory
    node (kvsep_bind_process_numa) -> number of CPUs bound to (0: nothing changed)."""
    return lib().kvsep_bind_process_numa(node)


def host_page_node(addr: int) -> int:
    """NUMA node of the page at host address `addr` (-1 unknown)."""
    return lib().kvsep_host_page_node(ctypes.c_void_p(addr))


def format_cpulist(cpus) -> str:
    """[0, 1, 2, 3, 8] -> "0-3,8" (the sysfs cpulist spelling)."""
    cpus = sorted(set(int(c) for c in cpus))
    out, i = [], 0
    while i < len(cpus):
        j = i
        while j + 1 < len(cpus) and cpus[j + 1] == cpus[j] + 1:
            j += 1
        out.append(str(cpus[i]) if j == i else f"{cpus[i]}-{cpus[j]}")
        i = j + 1
    return ",".join(out)


def build_info() -> str:
    return lib().kvsep_build_info().decode()
