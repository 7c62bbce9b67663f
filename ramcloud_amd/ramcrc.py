"""Python binding of libramcrc (include/ramcrc.h) -- the product path.

The CRC work happens in the HIP kernels of libramcrc.so; this module only
passes pointers.  There is no CPU fallback for the device entry points: if the
library is missing or a call fails, an exception is raised.

Device memory and streams come from PyTorch (plumbing only): tensors are
passed by data_ptr(), streams by torch.cuda.current_stream().cuda_stream.
"""
import ctypes
import os

import numpy as np

from . import build as _build

_c = ctypes
_lib = None

FINALIZE = 1

_ERRORS = {0: "ok", -1: "invalid argument", -2: "out of memory", -3: "HIP error",
           -4: "no usable device", -5: "RCCL error", -6: "launch refused (scratch too small, or a placement list refused)",
           -7: "launch refused (inconsistent bin layout)",
           -8: "another shard rank failed"}

EINVAL = -1
ENOMEM = -2
EREFUSED = -6
EINTERNAL = -7
EPEER = -8

# ramcrc_ctx_set_option options (include/ramcrc.h)
OPT_SERIAL_WALK = 1
OPT_WALK_PART_SHIFT = 2
OPT_TEST_FAIL_AFTER_COUNT = 3
OPT_TEST_DIRTY_BINS = 4
OPT_TEST_BIN_STRAGGLER = 5
OPT_BIN_ONE = 6
OPT_VERIFY_IN_WALK = 7


class RamcrcError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def lib_path():
    # RAMCRC_LIB selects a tuning variant built by `python -m ramcloud_amd.build --variants`
    return os.environ.get("RAMCRC_LIB") or _build.LIB


def lib():
    """Load libramcrc.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RamcrcError(f"libramcrc.so not built ({path}); run python -m ramcloud_amd.build")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7,
    # with the same soname as /opt/rocm's, and whichever is loaded first
    # serves both.  Loading this library first left torch on /opt/rocm's
    # runtime, which then reported no GPU; importing torch first keeps every
    # caller on torch's runtime.
    import torch  # noqa: F401
    L = _c.CDLL(path)
    if path != _build.LIB:
        _check_variant(L, path)
    vp, u32, u64, i32 = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int
    sig = {
        "ramcrc_update_hw": (u32, [u32, vp, u64]),
        "ramcrc_update_sw": (u32, [u32, vp, u64]),
        "ramcrc_update": (u32, [u32, vp, u64]),
        "ramcrc_cpu_has_hw": (i32, []),
        "ramcrc_shift": (u32, [u32, u64]),
        "ramcrc_combine": (u32, [u32, u32, u64]),
        "ramcrc_ctx_create": (i32, [i32, _c.POINTER(vp)]),
        "ramcrc_ctx_destroy": (i32, [vp]),
        "ramcrc_ctx_reserve": (i32, [vp, u64, u64]),
        "ramcrc_debug_scratch_allocations": (i32, [_c.POINTER(u64)]),
        "ramcrc_segments_device": (i32, [vp, vp, u64, u64, vp, vp, u32, vp]),
        "ramcrc_batch_device": (i32, [vp, vp, vp, vp, vp, vp, u64, u32, vp]),
        "ramcrc_entries_device": (i32, [vp, vp, vp, vp, vp, vp, u64, u32, vp]),
        "ramcrc_batch_host": (i32, [vp, vp, vp, vp, vp, u64, u32]),
        "ramcrc_stream_host": (i32, [vp, vp, u64, u64, vp, u32, i32, i32]),
        "ramcrc_segment_walk_device": (i32, [vp, vp, u64, u32, u64, vp, vp, vp, u64, vp, vp]),
        "ramcrc_verify_objects_device": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "ramcrc_replay_verify_device": (i32, [vp, vp, u64, u32, u64, vp, vp, vp, u64, vp, vp, vp]),
        "ramcrc_segments_certify_device": (i32, [vp, vp, u64, u32, u64, vp, vp, vp, vp]),
        "ramcrc_recovery_append_device": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp, u64, vp, u32,
                                                vp, u64, u32, vp, vp, vp]),
        "ramcrc_recovery_append_host": (i32, [vp, u64, u64, vp, vp, u64, vp, u64, u32, vp, u64, u32,
                                              vp, vp]),
        "ramcrc_replay_sidelog_device": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp, u64, vp, u32,
                                               vp, u64, u32, vp, vp, vp, vp, vp]),
        "ramcrc_replay_sidelog_host": (i32, [vp, u64, u64, vp, vp, u64, vp, u64, u32, vp, u64, u32,
                                             vp, vp, vp, vp]),
        "ramcrc_recovery_partition_device": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp, u32, u32,
                                                   vp, u64, vp, vp, vp, vp]),
        "ramcrc_recovery_partition_host": (i32, [vp, u64, u64, vp, vp, u64, vp, u32, u32, vp, u64,
                                                 _c.POINTER(u64), vp, vp]),
        "ramcrc_replay_resolve_device": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp, vp, vp, u64,
                                               vp, vp, vp]),
        "ramcrc_replay_resolve_host": (i32, [vp, u64, u64, vp, vp, u64, vp, vp, vp, u64,
                                             _c.POINTER(u64), vp]),
        "ramcrc_replay_table_create": (i32, [vp, u64, u32, _c.POINTER(vp)]),
        "ramcrc_replay_table_destroy": (i32, [vp]),
        "ramcrc_replay_table_reset": (i32, [vp, vp]),
        "ramcrc_replay_table_add_device": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp, vp,
                                                 _c.POINTER(u32), vp]),
        "ramcrc_replay_table_live_device": (i32, [vp, u32, vp, vp, u64, vp, vp, vp]),
        "ramcrc_replay_table_stats_device": (i32, [vp, vp, vp]),
        "ramcrc_replay_table_create_host": (i32, [u64, u32, _c.POINTER(vp)]),
        "ramcrc_replay_table_destroy_host": (i32, [vp]),
        "ramcrc_replay_table_reset_host": (i32, [vp]),
        "ramcrc_replay_table_add_host": (i32, [vp, vp, u64, u64, vp, vp, u64, vp, vp,
                                               _c.POINTER(u32)]),
        "ramcrc_replay_table_live_host": (i32, [vp, u32, vp, vp, u64, _c.POINTER(u64), vp]),
        "ramcrc_replay_table_stats_host": (i32, [vp, vp]),
        "ramcrc_replay_table_lookup_device": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "ramcrc_replay_table_lookup_host": (i32, [vp, vp, u64, vp, u64, vp, vp, vp]),
        "ramcrc_replay_table_read_device": (i32, [vp, vp, u64, vp, u64, vp, vp, u32, vp, u64, vp, vp,
                                                  vp, vp]),
        "ramcrc_replay_table_read_host": (i32, [vp, vp, u64, vp, u64, vp, vp, u32, vp, u64, vp, vp,
                                                vp]),
        "ramcrc_replay_table_read_hashes_device": (i32, [vp, u64, vp, u64, u32, vp, u64, u64, vp, vp, vp]),
        "ramcrc_replay_table_read_hashes_host": (i32, [vp, u64, vp, u64, u32, vp, u64, u64, vp, vp]),
        "ramcrc_replay_table_enumerate_device": (i32, [vp, u64, u64, u64, u64, u64, u64, vp, u32, u32, vp, u64,
                                                       u64, vp, vp]),
        "ramcrc_replay_table_enumerate_host": (i32, [vp, u64, u64, u64, u64, u64, u64, vp, u32, u32, vp, u64,
                                                     u64, vp]),
        "ramcrc_replay_table_index_build_device": (i32, [vp, u64, u32, vp, u64, vp, vp, u64, vp, vp]),
        "ramcrc_replay_table_index_build_host": (i32, [vp, u64, u32, vp, u64, vp, vp, u64, vp]),
        "ramcrc_index_lookup_device": (i32, [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, vp, vp]),
        "ramcrc_index_lookup_host": (i32, [vp, vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, vp]),
        "ramcrc_replay_table_write_device": (i32, [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, u32,
                                                   vp, vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_write_host": (i32, [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, u32,
                                                 vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_remove_device": (i32, [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, u32,
                                                    vp, vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_remove_host": (i32, [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, u32,
                                                  vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_increment_device": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, u64, u32, vp, vp,
                                                       u32, vp, vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_increment_host": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, u64, u32, vp, vp,
                                                     u32, vp, vp, vp, vp, vp]),
        "ramcrc_replay_table_clean_size_device": (i32, [vp, vp, u32, vp, vp, vp]),
        "ramcrc_replay_table_clean_device": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, u64, vp, vp, vp,
                                                   vp, vp, _c.POINTER(u32), vp]),
        "ramcrc_replay_table_clean_size_host": (i32, [vp, vp, u32, vp, vp]),
        "ramcrc_replay_table_clean_host": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, u64, vp, vp, vp,
                                                 vp, vp, _c.POINTER(u32)]),
        "ramcrc_replay_table_migrate_device": (i32, [vp, vp, u32, u64, u64, u64, u32, u32, u32, vp, u32, u64,
                                                     u32, vp, vp, vp, u64, vp, vp, vp]),
        "ramcrc_replay_table_migrate_host": (i32, [vp, vp, u32, u64, u64, u64, u32, u32, u32, vp, u32, u64,
                                                   u32, vp, vp, vp, u64, vp, vp]),
        "ramcrc_segment_fill_objects": (i32, [vp, u32, u32, u64, _c.POINTER(u32), vp]),
        "ramcrc_assemble_objects_device": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "ramcrc_assemble_objects_host": (i32, [vp, vp, vp, u64]),
        "ramcrc_ctx_set_timing": (i32, [vp, i32]),
        "ramcrc_ctx_scan_time": (i32, [vp, _c.POINTER(_c.c_double), _c.POINTER(u64)]),
        "ramcrc_ctx_status": (i32, [vp, _c.POINTER(u32)]),
        "ramcrc_ctx_check": (i32, [vp, vp]),
        "ramcrc_ctx_set_option": (i32, [vp, i32, _c.c_int64]),
        "ramcrc_segment_fill_objects_device": (i32, [vp, vp, u64, u32, u64, u32, u64, vp, vp,
                                                     _c.POINTER(u32)]),
        "ramcrc_shard_unique_id": (i32, [vp]),
        "ramcrc_shard_create_all": (i32, [vp, i32, _c.POINTER(vp)]),
        "ramcrc_shard_create_rank": (i32, [vp, i32, i32, i32, _c.POINTER(vp)]),
        "ramcrc_shard_destroy": (i32, [vp]),
        "ramcrc_shard_range": (i32, [u64, i32, i32, _c.POINTER(u64), _c.POINTER(u64)]),
        "ramcrc_shard_local_count": (i32, [vp]),
        "ramcrc_shard_info": (i32, [vp, i32, _c.POINTER(i32), _c.POINTER(i32), _c.POINTER(vp),
                                    _c.POINTER(vp)]),
        "ramcrc_shard_segments": (i32, [vp, vp, u64, u64, vp, u32]),
        "ramcrc_shard_sync": (i32, [vp]),
        "ramcrc_shard_results": (i32, [vp, i32, vp, u64]),
        "ramcrc_stream_create_cu_mask": (i32, [i32, vp, u32, _c.POINTER(vp)]),
        "ramcrc_stream_destroy": (i32, [vp]),
        "ramcrc_ctx_set_cus": (i32, [vp, i32]),
        "ramcrc_strerror": (_c.c_char_p, [i32]),
        "ramcrc_last_hip_error": (i32, []),
        "ramcrc_device_count": (i32, []),
        "ramcrc_build_info": (_c.c_char_p, []),
        "ramcrc_ctx_debug_bins": (i32, [vp, vp, u64, _c.POINTER(u32)]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if path == _build.LIB:
                raise   # the product library must export the whole header
            continue    # an older A/B variant (RAMCRC_LIB)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def build_defines(info):
    """The -D knobs a library was built with, from its ramcrc_build_info()."""
    if " defines=" not in info:
        return []
    d = info.split(" defines=", 1)[1].split()
    return d[0].split(",") if d and d[0] != "none" else []


def _check_variant(L, path):
    """RAMCRC_LIB: only A/B variants of this tree's table that compute exact
    results (build.UNSAFE_DEFINES) may replace the product library."""
    f = L.ramcrc_build_info
    f.restype = _c.c_char_p
    info = f().decode("ascii", "replace")
    if "src_sha=" not in info:
        raise RamcrcError(f"RAMCRC_LIB={path} is not a libramcrc build")
    bad = _build.unsafe_defines(build_defines(info))
    if bad:
        raise RamcrcError(f"RAMCRC_LIB={path} is a probe build ({bad}); refusing to load it")


def exported_symbols():
    return [n for n in dir(lib()) if n.startswith("ramcrc_")]


def _check(rc, what):
    if rc != 0:
        msg = lib().ramcrc_strerror(rc).decode()
        raise RamcrcError(f"{what} failed: {_ERRORS.get(rc, rc)} ({msg})", rc)


def _buf(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    else:
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return a, _c.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------ host
def update(state, data):
    """Crc32C::update on the host hardware path; returns the raw state."""
    a, p = _buf(data)
    return int(lib().ramcrc_update(state & 0xFFFFFFFF, p, a.size))


def update_sw(state, data):
    a, p = _buf(data)
    return int(lib().ramcrc_update_sw(state & 0xFFFFFFFF, p, a.size))


def update_hw(state, data):
    a, p = _buf(data)
    return int(lib().ramcrc_update_hw(state & 0xFFFFFFFF, p, a.size))


def crc32c(data):
    """Crc32C().update(data).getResult() on the host."""
    return (~update(0xFFFFFFFF, data)) & 0xFFFFFFFF


def shift(state, nbytes):
    return int(lib().ramcrc_shift(state & 0xFFFFFFFF, nbytes))


def combine(raw_a, raw_b, len_b):
    return int(lib().ramcrc_combine(raw_a & 0xFFFFFFFF, raw_b & 0xFFFFFFFF, len_b))


def cpu_has_hw():
    return bool(lib().ramcrc_cpu_has_hw())


def device_count():
    return int(lib().ramcrc_device_count())


def scratch_allocations():
    """How often this process has allocated or grown device scratch
    (ramcrc_debug_scratch_allocations): unchanged across a call that does not
    allocate."""
    n = _c.c_uint64(0)
    _check(lib().ramcrc_debug_scratch_allocations(_c.byref(n)), "ramcrc_debug_scratch_allocations")
    return n.value


def segment_fill_objects(seg, value_len, first_key=0):
    """Host append path: fill an empty segment (numpy uint8, pre-filled value
    bytes) with RecoverSegmentBenchmark-shaped objects.  Returns
    (n_objects, segment_length, checksum)."""
    if not (isinstance(seg, np.ndarray) and seg.dtype == np.uint8 and seg.flags.c_contiguous):
        raise RamcrcError("segment must be a contiguous numpy uint8 array")
    n = _c.c_uint32(0)
    cert = np.zeros(2, dtype=np.uint32)
    rc = lib().ramcrc_segment_fill_objects(_c.c_void_p(seg.ctypes.data), seg.size, value_len,
                                           first_key, _c.byref(n), _c.c_void_p(cert.ctypes.data))
    _check(rc, "ramcrc_segment_fill_objects")
    return n.value, int(cert[0]), int(cert[1])


def recovery_append_host(segments, seg_stride, n_seg, status, entries, place, n_part, out,
                         out_stride, out_capacity):
    """RecoverySegmentBuilder::build's append loop on the host
    (ramcrc_recovery_append_host).  All arguments are C-contiguous numpy
    arrays: segments uint8; status uint32 [n_seg, 4]; entries uint32 [n, 4]
    (segment, offset, length, header); place uint32 [m, 2] (record,
    partition) or segments.PLACEMENT_DTYPE [m]; out uint8, written in place.
    Returns (certs uint32 [n_seg * n_part, 2], status uint32 [n_seg * n_part,
    2]); raises RamcrcError (code EINVAL) where the device form refuses."""
    def arr(a, dtype):
        a = np.asarray(a)
        if a.dtype.fields is not None:
            a = a.view(np.uint32)
        if a.dtype != dtype or not a.flags.c_contiguous:
            raise RamcrcError(f"expected a contiguous {np.dtype(dtype).name} array")
        return a
    segments, out = arr(segments, np.uint8), arr(out, np.uint8)
    status, entries, place = arr(status, np.uint32), arr(entries, np.uint32), arr(place, np.uint32)
    n_out = int(n_seg) * int(n_part)
    if (segments.size < n_seg * seg_stride or out.size < n_out * out_stride
            or status.size < 4 * n_seg or not out.flags.writeable):
        raise RamcrcError("recovery_append_host: an array is smaller than its geometry")
    certs = np.zeros((n_out, 2), np.uint32)
    ostat = np.zeros((n_out, 2), np.uint32)
    p = lambda a: _c.c_void_p(a.ctypes.data)
    rc = lib().ramcrc_recovery_append_host(p(segments), seg_stride, n_seg, p(status), p(entries),
                                           entries.size // 4, p(place), place.size // 2, n_part,
                                           p(out), out_stride, out_capacity, p(certs), p(ostat))
    _check(rc, "ramcrc_recovery_append_host")
    return certs, ostat


def replay_sidelog_host(segments, seg_stride, n_seg, status, entries, live, timestamp, out,
                        out_stride, out_capacity, want_refs=True):
    """ObjectManager::replaySegment's side log on the host
    (ramcrc_replay_sidelog_host): the append at one partition with kept
    tombstones rewritten (segmentId 0, `timestamp`, a recomputed checksum).
    Arrays as recovery_append_host takes them; live uint32 [m, 2] (record, 0).
    Returns (certs uint32 [n_seg, 2], status uint32 [n_seg, 2], refs uint32
    [m, 2] (output, offset; LOG_REF_NONE twice where not appended) or None,
    counts: a segments.SIDELOG_COUNTS_DTYPE scalar); raises RamcrcError (code
    EINVAL) where the device form refuses."""
    from . import segments as _seg

    def arr(a, dtype):
        a = np.asarray(a)
        if a.dtype.fields is not None:
            a = a.view(np.uint32)
        if a.dtype != dtype or not a.flags.c_contiguous:
            raise RamcrcError(f"expected a contiguous {np.dtype(dtype).name} array")
        return a
    segments, out = arr(segments, np.uint8), arr(out, np.uint8)
    status, entries, live = arr(status, np.uint32), arr(entries, np.uint32), arr(live, np.uint32)
    if (segments.size < n_seg * seg_stride or out.size < n_seg * out_stride
            or status.size < 4 * n_seg or not out.flags.writeable):
        raise RamcrcError("replay_sidelog_host: an array is smaller than its geometry")
    m = live.size // 2
    certs = np.zeros((n_seg, 2), np.uint32)
    ostat = np.zeros((n_seg, 2), np.uint32)
    refs = np.zeros((m, 2), np.uint32) if want_refs else None
    counts = np.zeros(1, _seg.SIDELOG_COUNTS_DTYPE)
    p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None else None
    rc = lib().ramcrc_replay_sidelog_host(p(segments), seg_stride, n_seg, p(status), p(entries),
                                          entries.size // 4, p(live), m, int(timestamp), p(out),
                                          out_stride, out_capacity, p(certs), p(ostat), p(refs),
                                          p(counts))
    _check(rc, "ramcrc_replay_sidelog_host")
    return certs, ostat, refs, counts[0]


def recovery_partition_host(segments, seg_stride, n_seg, status, entries, tablets, n_part,
                            place_cap=None):
    """RecoverySegmentBuilder::build's placement decision on the host
    (ramcrc_recovery_partition_host).  segments uint8; status uint32 [n_seg, 4];
    entries uint32 [n, 4]; tablets segments.TABLET_DTYPE [t].  place_cap: the
    list's capacity (None: sized to the need).  Returns (place uint32 [m, 2]
    with m = min(needed, place_cap), needed, key_hash uint64 [n], part_status
    uint32 [n_seg, 4]: flags, placed, unplaced, dead); raises RamcrcError (code
    EINVAL) where the device form refuses."""
    from . import segments as _seg
    segments = np.ascontiguousarray(segments, np.uint8)
    status = np.ascontiguousarray(np.asarray(status).view(np.uint32)).reshape(-1, 4)
    entries = np.ascontiguousarray(np.asarray(entries).view(np.uint32)).reshape(-1, 4)
    tablets = np.ascontiguousarray(tablets, _seg.TABLET_DTYPE).reshape(-1)
    n = entries.shape[0]
    if segments.size < n_seg * seg_stride or status.shape[0] < n_seg:
        raise RamcrcError("recovery_partition_host: an array is smaller than its geometry")
    key_hash = np.zeros(n, np.uint64)
    pstat = np.zeros((n_seg, 4), np.uint32)
    p = lambda a: _c.c_void_p(a.ctypes.data) if a.size else None
    need = _c.c_uint64(0)

    def call(cap):
        place = np.zeros((cap, 2), np.uint32)
        rc = lib().ramcrc_recovery_partition_host(p(segments), seg_stride, n_seg, p(status),
                                                  p(entries), n, p(tablets), tablets.size, n_part,
                                                  p(place), cap, _c.byref(need), p(key_hash),
                                                  p(pstat))
        _check(rc, "ramcrc_recovery_partition_host")
        return place

    if place_cap is None:
        call(0)
        place_cap = need.value
    place = call(place_cap)
    return place[:min(need.value, place_cap)], need.value, key_hash, pstat


def replay_resolve_host(segments, seg_stride, n_seg, status, entries, key_hash=None,
                        live_cap=None):
    """ObjectManager::replaySegment's newest-wins decision on the host
    (ramcrc_replay_resolve_host).  segments uint8; status uint32 [n_seg, 4];
    entries uint32 [n, 4]; key_hash uint64 [n] or None (computed).  live_cap:
    the list's capacity (None: one slot per record).  Returns (winner uint32
    [n], live uint32 [m, 2] with m = min(needed, live_cap), needed, counts: a
    segments.RESOLVE_COUNTS_DTYPE scalar); raises RamcrcError (code EINVAL)
    where the device form refuses."""
    from . import segments as _seg
    segments = np.ascontiguousarray(segments, np.uint8)
    status = np.ascontiguousarray(np.asarray(status).view(np.uint32)).reshape(-1, 4)
    entries = np.ascontiguousarray(np.asarray(entries).view(np.uint32)).reshape(-1, 4)
    n = entries.shape[0]
    if segments.size < n_seg * seg_stride or status.shape[0] < n_seg:
        raise RamcrcError("replay_resolve_host: an array is smaller than its geometry")
    if key_hash is not None:
        key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
        if key_hash.size < n:
            raise RamcrcError("replay_resolve_host: fewer hashes than records")
    cap = n if live_cap is None else int(live_cap)
    winner = np.zeros(n, np.uint32)
    live = np.zeros((cap, 2), np.uint32)
    counts = np.zeros(1, _seg.RESOLVE_COUNTS_DTYPE)
    need = _c.c_uint64(0)
    p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
    rc = lib().ramcrc_replay_resolve_host(p(segments), seg_stride, n_seg, p(status), p(entries), n,
                                          p(key_hash), p(winner), p(live), cap, _c.byref(need),
                                          p(counts))
    _check(rc, "ramcrc_replay_resolve_host")
    return winner, live[:min(need.value, cap)], need.value, counts[0]


class Index:
    """A built secondary index (ramcrc_replay_table_index_build_device / _host):
    the sorted entries (segments.INDEX_ENTRY_DTYPE, 32 bytes each), the dense
    copy of their hashes, the index's own copy of its keys and the build's
    summary (segments.INDEX_BUILD_SUMMARY_DTYPE).  CUDA tensors for a device
    index, numpy arrays for a host index.  An index is self-contained: it
    outlives the table's later adds and cleans, merely going stale."""

    def __init__(self, entries, hashes, index_keys, summary):
        self.entries, self.hashes, self.index_keys, self.summary = entries, hashes, index_keys, summary


def index_lookup_host(index, qkeys, queries, out_capacity=None):
    """A batch of lookupIndexKeys over a host index (ramcrc_index_lookup_host).
    qkeys: uint8 [qkeys_bytes]; queries: segments.INDEX_QUERY_DTYPE [n]
    (segments.index_queries packs both); out_capacity: the reply's room in
    hashes, default: room for every query's max_hashes, at most the index's
    entries each.  Returns (out_hashes: uint64 [hashes], results:
    segments.INDEX_RESULT_DTYPE [n], summary: a
    segments.INDEX_LOOKUP_SUMMARY_DTYPE scalar);
    segments.index_lookup_hashes splits the reply."""
    from . import segments as _seg
    qkeys = np.ascontiguousarray(qkeys, np.uint8).reshape(-1)
    queries = np.ascontiguousarray(queries, _seg.INDEX_QUERY_DTYPE).reshape(-1)
    n = queries.shape[0]
    ne = int(index.summary["n_entries"])
    if out_capacity is None:
        out_capacity = int(np.minimum(queries["max_hashes"].astype(np.uint64), ne).sum())
    out = np.zeros(int(out_capacity), np.uint64)
    results = np.zeros(n, _seg.INDEX_RESULT_DTYPE)
    summary = np.zeros(1, _seg.INDEX_LOOKUP_SUMMARY_DTYPE)
    bs = np.array([index.summary], _seg.INDEX_BUILD_SUMMARY_DTYPE)
    p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
    rc = lib().ramcrc_index_lookup_host(p(index.entries), p(index.hashes), p(index.index_keys), p(bs),
                                        p(qkeys), qkeys.size, p(queries), n, p(out), out.size,
                                        p(results), p(summary))
    _check(rc, "ramcrc_index_lookup_host")
    return out[:int(summary[0]["hashes"])], results, summary[0]


class ReplayTableHost:
    """The persistent replay table on the host (ramcrc_replay_table_*_host):
    replay_resolve_host's decision fed batch by batch.  The table keeps the
    arrays of every added batch alive until reset() or close()."""

    def __init__(self, key_cap, max_batches):
        h = _c.c_void_p()
        _check(lib().ramcrc_replay_table_create_host(int(key_cap), int(max_batches), _c.byref(h)),
               "ramcrc_replay_table_create_host")
        self._h = h
        self._keep = []

    def close(self):
        if self._h:
            lib().ramcrc_replay_table_destroy_host(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(lib().ramcrc_replay_table_reset_host(self._h), "ramcrc_replay_table_reset_host")
        self._keep = []

    def add(self, segments, seg_stride, n_seg, status, entries, key_hash=None):
        """Resolve one walk's records into the table; arrays as
        replay_resolve_host takes them.  Returns the batch number; raises
        RamcrcError (code EINVAL) where the device form spoils the table, on a
        spoiled table, and past max_batches."""
        segments = np.ascontiguousarray(segments, np.uint8)
        status = np.ascontiguousarray(np.asarray(status).view(np.uint32)).reshape(-1, 4)
        entries = np.ascontiguousarray(np.asarray(entries).view(np.uint32)).reshape(-1, 4)
        n = entries.shape[0]
        if segments.size < n_seg * seg_stride or status.shape[0] < n_seg:
            raise RamcrcError("ReplayTableHost.add: an array is smaller than its geometry")
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.add: fewer hashes than records")
        work = np.zeros(max(n, 1), np.uint64)
        none = 0xFFFFFFFF
        batch = _c.c_uint32(none)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_add_host(self._h, p(segments), seg_stride, n_seg, p(status),
                                                p(entries), n, p(key_hash), p(work),
                                                _c.byref(batch))
        if batch.value != none:   # the batch has a number: the table reads its arrays from now on
            self._keep.append((segments, status, entries, key_hash, work))
        _check(rc, "ramcrc_replay_table_add_host")
        return batch.value

    def live(self, batch, live_cap=None):
        """The verdict on one batch as the table stands.  Returns (winner:
        segments.REPLAY_REF_DTYPE [n], live uint32 [m, 2] with m = min(needed,
        live_cap), needed, counts: a segments.RESOLVE_COUNTS_DTYPE scalar)."""
        from . import segments as _seg
        if not 0 <= int(batch) < len(self._keep) or self._keep[int(batch)] is None:
            raise RamcrcError("ReplayTableHost.live: no such batch, or a cleaned one", EINVAL)
        n = self._keep[int(batch)][2].shape[0]
        cap = n if live_cap is None else int(live_cap)
        winner = np.zeros(n, _seg.REPLAY_REF_DTYPE)
        live = np.zeros((cap, 2), np.uint32)
        counts = np.zeros(1, _seg.RESOLVE_COUNTS_DTYPE)
        need = _c.c_uint64(0)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a.size else None
        rc = lib().ramcrc_replay_table_live_host(self._h, int(batch), p(winner), p(live), cap,
                                                 _c.byref(need), p(counts))
        _check(rc, "ramcrc_replay_table_live_host")
        return winner, live[:min(need.value, cap)], need.value, counts[0]

    def stats(self):
        """A segments.REPLAY_TABLE_STATS_DTYPE scalar."""
        from . import segments as _seg
        st = np.zeros(1, _seg.REPLAY_TABLE_STATS_DTYPE)
        _check(lib().ramcrc_replay_table_stats_host(self._h, _c.c_void_p(st.ctypes.data)),
               "ramcrc_replay_table_stats_host")
        return st[0]

    def lookup(self, keys, queries, key_hash=None):
        """What the table holds for each key.  keys: uint8 [keys_bytes], the
        key buffer; queries: segments.LOOKUP_KEY_DTYPE [n]
        (segments.lookup_queries packs both); key_hash: uint64 [n] or None
        (computed).  Returns (results: segments.LOOKUP_RESULT_DTYPE [n], counts:
        a segments.LOOKUP_COUNTS_DTYPE scalar); on a spoiled table the results
        are the wrapper's zeros and counts["spoiled"] is 1."""
        from . import segments as _seg
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
        queries = np.ascontiguousarray(queries, _seg.LOOKUP_KEY_DTYPE).reshape(-1)
        n = queries.shape[0]
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.lookup: fewer hashes than queries")
        results = np.zeros(n, _seg.LOOKUP_RESULT_DTYPE)
        counts = np.zeros(1, _seg.LOOKUP_COUNTS_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_lookup_host(self._h, p(keys), keys.size, p(queries), n,
                                                   p(key_hash), p(results), p(counts))
        _check(rc, "ramcrc_replay_table_lookup_host")
        return results, counts[0]

    def read(self, keys, queries, reply_cap, rules=None, value_only=False, key_hash=None,
             want_results=False):
        """A multi-read's reply (ramcrc_replay_table_read_host).  keys, queries,
        key_hash as lookup takes them; rules: segments.REJECT_RULES_DTYPE [n]
        (segments.read_rules packs them) or None: no rules; reply_cap: the
        reply's limit in bytes.  Returns (reply: uint8 [reply_bytes], part_off:
        uint64 [n], READ_NONE where a query was not returned, summary: a
        segments.READ_SUMMARY_DTYPE scalar, results:
        segments.LOOKUP_RESULT_DTYPE [n] or None); segments.multi_read_parts
        splits the reply.  On a spoiled table the reply is empty, part_off and
        results are the wrapper's zeros and summary["spoiled"] is 1."""
        from . import segments as _seg
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
        queries = np.ascontiguousarray(queries, _seg.LOOKUP_KEY_DTYPE).reshape(-1)
        n = queries.shape[0]
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.read: fewer hashes than queries")
        if rules is not None:
            rules = np.ascontiguousarray(rules, _seg.REJECT_RULES_DTYPE).reshape(-1)
            if rules.size < n:
                raise RamcrcError("ReplayTableHost.read: fewer rules than queries")
        reply_cap = int(reply_cap)
        # no reply is longer than its parts: 16 bytes and at most the longest
        # payload each, so a cap beyond that changes nothing
        # (a cleaned batch keeps its number and holds nothing)
        longest = max([int(k[2][:, 2].max()) for k in self._keep if k is not None and k[2].shape[0]],
                      default=0)
        room = min(reply_cap, n * (16 + longest))
        reply = np.zeros(room, np.uint8)
        part_off = np.zeros(n, np.uint64)
        results = np.zeros(n, _seg.LOOKUP_RESULT_DTYPE) if want_results else None
        summary = np.zeros(1, _seg.READ_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_read_host(
            self._h, p(keys), keys.size, p(queries), n, p(key_hash), p(rules),
            _seg.READ_VALUE_ONLY if value_only else 0, p(reply), room, p(part_off), p(results),
            p(summary))
        _check(rc, "ramcrc_replay_table_read_host")
        return reply[:int(summary[0]["reply_bytes"])], part_off, summary[0], results

    def read_hashes(self, table_id, hashes, max_length, reply_capacity=None):
        """An indexed read's reply (ramcrc_replay_table_read_hashes_host): for
        every asked primary-key hash the objects of table_id whose record hash
        equals it.  hashes: uint64 [n]; max_length: the reference's maxLength;
        reply_capacity: the reply buffer's size, default: room for max_length
        and one hash's overshoot.  Returns (reply: uint8 [reply_bytes], parts:
        segments.HASH_PART_DTYPE [n], summary: a
        segments.READ_HASHES_SUMMARY_DTYPE scalar);
        segments.read_hashes_objects splits the reply.  On a spoiled table the
        reply is empty, parts are the wrapper's zeros and summary["spoiled"]
        is 1."""
        from . import segments as _seg
        hashes = np.ascontiguousarray(hashes, np.uint64).reshape(-1)
        n = hashes.shape[0]
        # no reply is longer than every held object sent for every hash, 12
        # bytes and at most the payload each
        held = sum(int(k[2][:, 2].sum()) + 12 * k[2].shape[0] for k in self._keep if k is not None)
        if reply_capacity is None:
            reply_capacity = min(int(max_length), n * held) + held
        room = min(int(reply_capacity), n * held)
        reply = np.zeros(room, np.uint8)
        parts = np.zeros(n, _seg.HASH_PART_DTYPE)
        summary = np.zeros(1, _seg.READ_HASHES_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_read_hashes_host(
            self._h, int(table_id), p(hashes), n, 0, p(reply), room, int(max_length), p(parts),
            p(summary))
        _check(rc, "ramcrc_replay_table_read_hashes_host")
        return reply[:int(summary[0]["reply_bytes"])], parts, summary[0]

    def enumerate(self, table_id, max_bytes, first_hash=0, last_hash=0xFFFFFFFFFFFFFFFF, bucket_index=0,
                  bucket_next_hash=0, bucket_limit=0, stale=None, keys_only=False, payload_capacity=None):
        """One reply of a table enumeration (ramcrc_replay_table_enumerate_host):
        the objects of table_id with first_hash <= hash <= last_hash, bucket by
        bucket from the cursor (bucket_index, bucket_next_hash) up to
        bucket_limit (0: every bucket), as {u32 length, log entry} entries
        that end within max_bytes.  stale: the iterator's stale frames
        (segments.enum_frames or its rows); keys_only: entries end before the
        value; payload_capacity: the payload buffer's size, default: room for
        max_bytes.  Returns (payload: uint8 [payload_bytes], summary: a
        segments.ENUMERATE_SUMMARY_DTYPE scalar, whose next_bucket and
        next_hash are the cursor to go on with);
        segments.enumerate_objects splits the payload.  On a spoiled table
        the payload is empty and summary["spoiled"] is 1."""
        from . import segments as _seg
        if stale is None:
            stale = []
        if not (isinstance(stale, np.ndarray) and stale.dtype == _seg.ENUM_FRAME_DTYPE):
            stale = _seg.enum_frames(stale)
        stale = np.ascontiguousarray(stale)
        # no payload is longer than every held object sent once, 4 bytes and
        # at most the log entry each
        held = sum(int(k[2][:, 2].sum()) + 4 * k[2].shape[0] for k in self._keep if k is not None)
        if payload_capacity is None:
            payload_capacity = min(int(max_bytes), held)
        room = min(int(payload_capacity), held)
        payload = np.zeros(room, np.uint8)
        summary = np.zeros(1, _seg.ENUMERATE_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_enumerate_host(
            self._h, int(table_id), int(first_hash), int(last_hash), int(bucket_index),
            int(bucket_next_hash), int(bucket_limit), p(stale), stale.shape[0],
            _seg.ENUM_KEYS_ONLY if keys_only else 0, p(payload), room, int(max_bytes), p(summary))
        _check(rc, "ramcrc_replay_table_enumerate_host")
        return payload[:int(summary[0]["payload_bytes"])], summary[0]

    def index_build(self, table_id, index_id, entry_capacity=None, keys_capacity=None):
        """The sorted secondary index of table_id's key index_id (>= 1) over the
        table's object winners (ramcrc_replay_table_index_build_host).
        entry_capacity, keys_capacity: the arrays' room, default: what the
        sizing call reports.  Returns an Index of numpy arrays, cut to what
        was written, whose summary is a segments.INDEX_BUILD_SUMMARY_DTYPE
        scalar; on overflow or a spoiled table the arrays are empty."""
        from . import segments as _seg
        summary = np.zeros(1, _seg.INDEX_BUILD_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        if entry_capacity is None or keys_capacity is None:
            rc = lib().ramcrc_replay_table_index_build_host(self._h, int(table_id), int(index_id), None, 0,
                                                            None, None, 0, p(summary))
            _check(rc, "ramcrc_replay_table_index_build_host")
            if entry_capacity is None:
                entry_capacity = int(summary[0]["entries_needed"])
            if keys_capacity is None:
                keys_capacity = int(summary[0]["key_bytes_needed"])
        entries = np.zeros(int(entry_capacity), _seg.INDEX_ENTRY_DTYPE)
        hashes = np.zeros(int(entry_capacity), np.uint64)
        keys = np.zeros(int(keys_capacity), np.uint8)
        rc = lib().ramcrc_replay_table_index_build_host(
            self._h, int(table_id), int(index_id), p(entries), entries.size, p(hashes), p(keys), keys.size,
            p(summary))
        _check(rc, "ramcrc_replay_table_index_build_host")
        n, kb = int(summary[0]["n_entries"]), int(summary[0]["key_bytes"])
        return Index(entries[:n], hashes[:n], keys[:kb], summary[0])

    def write(self, data, reqs, out_capacity, next_version, timestamp=0, rules=None,
              key_hash=None, batch_segment_id=None, want_refs=True, want_old=False):
        """A multi-write (ramcrc_replay_table_write_host): the table is not
        changed; the call returns the log segment to walk and add as the next
        batch.  data: uint8 [data_bytes], the keysAndValue images; reqs:
        segments.WRITE_REQ_DTYPE [n] (segments.write_requests packs both);
        rules and key_hash as read takes them; batch_segment_id: uint64 [batches]
        or None.  Returns (out: uint8 [out_capacity], its bytes from the head on
        untouched zeros; cert: a segments.CERT_DTYPE scalar; parts:
        segments.WRITE_PART_DTYPE [n]; refs: segments.WRITE_REF_DTYPE [n] or
        None; old: segments.LOOKUP_RESULT_DTYPE [n] or None; summary: a
        segments.WRITE_SUMMARY_DTYPE scalar).  On a spoiled table everything but
        the summary is the wrapper's zeros and summary["spoiled"] is 1."""
        from . import segments as _seg
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        reqs = np.ascontiguousarray(reqs, _seg.WRITE_REQ_DTYPE).reshape(-1)
        n = reqs.shape[0]
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.write: fewer hashes than requests")
        if rules is not None:
            rules = np.ascontiguousarray(rules, _seg.REJECT_RULES_DTYPE).reshape(-1)
            if rules.size < n:
                raise RamcrcError("ReplayTableHost.write: fewer rules than requests")
        if batch_segment_id is not None:
            batch_segment_id = np.ascontiguousarray(batch_segment_id, np.uint64).reshape(-1)
            if batch_segment_id.size < len(self._keep):
                raise RamcrcError("ReplayTableHost.write: fewer segment ids than batches")
        out = np.zeros(int(out_capacity), np.uint8)
        cert = np.zeros(1, _seg.CERT_DTYPE)
        parts = np.zeros(n, _seg.WRITE_PART_DTYPE)
        refs = np.zeros(n, _seg.WRITE_REF_DTYPE) if want_refs else None
        old = np.zeros(n, _seg.LOOKUP_RESULT_DTYPE) if want_old else None
        summary = np.zeros(1, _seg.WRITE_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_write_host(
            self._h, p(data), data.size, p(reqs), n, p(key_hash), p(rules), int(next_version),
            int(timestamp), p(batch_segment_id), p(out), out.size,
            _c.c_void_p(cert.ctypes.data), p(parts), p(refs), p(old),
            _c.c_void_p(summary.ctypes.data))
        _check(rc, "ramcrc_replay_table_write_host")
        return out, cert[0], parts, refs, old, summary[0]

    def remove(self, keys, reqs, out_capacity, next_version, timestamp=0, rules=None,
               key_hash=None, batch_segment_id=None, want_refs=True, want_old=False):
        """A multi-remove (ramcrc_replay_table_remove_host): the table is not
        changed; the call returns the log segment of tombstones to walk and add
        as the next batch.  keys: uint8 [keys_bytes]; reqs:
        segments.LOOKUP_KEY_DTYPE [n] (segments.lookup_queries packs both);
        rules and key_hash as read takes them; batch_segment_id: uint64 [batches]
        or None.  Returns (out: uint8 [out_capacity], its bytes from the head on
        untouched zeros; cert: a segments.CERT_DTYPE scalar; parts:
        segments.REMOVE_PART_DTYPE [n]; refs: uint32 [n] or None; old:
        segments.LOOKUP_RESULT_DTYPE [n] or None; summary: a
        segments.REMOVE_SUMMARY_DTYPE scalar).  On a spoiled table everything but
        the summary is the wrapper's zeros and summary["spoiled"] is 1."""
        from . import segments as _seg
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
        reqs = np.ascontiguousarray(reqs, _seg.LOOKUP_KEY_DTYPE).reshape(-1)
        n = reqs.shape[0]
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.remove: fewer hashes than requests")
        if rules is not None:
            rules = np.ascontiguousarray(rules, _seg.REJECT_RULES_DTYPE).reshape(-1)
            if rules.size < n:
                raise RamcrcError("ReplayTableHost.remove: fewer rules than requests")
        if batch_segment_id is not None:
            batch_segment_id = np.ascontiguousarray(batch_segment_id, np.uint64).reshape(-1)
            if batch_segment_id.size < len(self._keep):
                raise RamcrcError("ReplayTableHost.remove: fewer segment ids than batches")
        out = np.zeros(int(out_capacity), np.uint8)
        cert = np.zeros(1, _seg.CERT_DTYPE)
        parts = np.zeros(n, _seg.REMOVE_PART_DTYPE)
        refs = np.zeros(n, np.uint32) if want_refs else None
        old = np.zeros(n, _seg.LOOKUP_RESULT_DTYPE) if want_old else None
        summary = np.zeros(1, _seg.REMOVE_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_remove_host(
            self._h, p(keys), keys.size, p(reqs), n, p(key_hash), p(rules), int(next_version),
            int(timestamp), p(batch_segment_id), p(out), out.size,
            _c.c_void_p(cert.ctypes.data), p(parts), p(refs), p(old),
            _c.c_void_p(summary.ctypes.data))
        _check(rc, "ramcrc_replay_table_remove_host")
        return out, cert[0], parts, refs, old, summary[0]

    def increment(self, keys, reqs, args, out_capacity, next_version, timestamp=0, rules=None,
                  key_hash=None, batch_segment_id=None, want_refs=True, want_old=False):
        """A multi-increment (ramcrc_replay_table_increment_host): the table is
        not changed; the call returns the log segment of new objects and
        tombstones to walk and add as the next batch.  keys: uint8 [keys_bytes];
        reqs: segments.LOOKUP_KEY_DTYPE [n] (segments.lookup_queries packs both);
        args: segments.INCREMENT_ARG_DTYPE [n] (segments.increment_args); rules
        and key_hash as read takes them; batch_segment_id: uint64 [batches] or
        None.  Returns (out: uint8 [out_capacity], its bytes from the head on
        untouched zeros; cert: a segments.CERT_DTYPE scalar; parts:
        segments.INCREMENT_PART_DTYPE [n]; refs: segments.WRITE_REF_DTYPE [n] or
        None; old: segments.LOOKUP_RESULT_DTYPE [n] or None; summary: a
        segments.INCREMENT_SUMMARY_DTYPE scalar).  On a spoiled table everything
        but the summary is the wrapper's zeros and summary["spoiled"] is 1."""
        from . import segments as _seg
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
        reqs = np.ascontiguousarray(reqs, _seg.LOOKUP_KEY_DTYPE).reshape(-1)
        args = np.ascontiguousarray(args, _seg.INCREMENT_ARG_DTYPE).reshape(-1)
        n = reqs.shape[0]
        if args.size < n:
            raise RamcrcError("ReplayTableHost.increment: fewer args than requests")
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, np.uint64).reshape(-1)
            if key_hash.size < n:
                raise RamcrcError("ReplayTableHost.increment: fewer hashes than requests")
        if rules is not None:
            rules = np.ascontiguousarray(rules, _seg.REJECT_RULES_DTYPE).reshape(-1)
            if rules.size < n:
                raise RamcrcError("ReplayTableHost.increment: fewer rules than requests")
        if batch_segment_id is not None:
            batch_segment_id = np.ascontiguousarray(batch_segment_id, np.uint64).reshape(-1)
            if batch_segment_id.size < len(self._keep):
                raise RamcrcError("ReplayTableHost.increment: fewer segment ids than batches")
        out = np.zeros(int(out_capacity), np.uint8)
        cert = np.zeros(1, _seg.CERT_DTYPE)
        parts = np.zeros(n, _seg.INCREMENT_PART_DTYPE)
        refs = np.zeros(n, _seg.WRITE_REF_DTYPE) if want_refs else None
        old = np.zeros(n, _seg.LOOKUP_RESULT_DTYPE) if want_old else None
        summary = np.zeros(1, _seg.INCREMENT_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_increment_host(
            self._h, p(keys), keys.size, p(reqs), n, p(args), p(key_hash), p(rules), int(next_version),
            int(timestamp), p(batch_segment_id), p(out), out.size,
            _c.c_void_p(cert.ctypes.data), p(parts), p(refs), p(old),
            _c.c_void_p(summary.ctypes.data))
        _check(rc, "ramcrc_replay_table_increment_host")
        return out, cert[0], parts, refs, old, summary[0]

    def clean_size(self, victims):
        """What clean(victims) would need and move now
        (ramcrc_replay_table_clean_size_host); changes nothing.  Returns (usage:
        segments.CLEAN_USAGE_DTYPE [n_victims], summary: a
        segments.CLEAN_SUMMARY_DTYPE scalar)."""
        from . import segments as _seg
        victims = np.ascontiguousarray(victims, np.uint32).reshape(-1)
        usage = np.zeros(victims.size, _seg.CLEAN_USAGE_DTYPE)
        summary = np.zeros(1, _seg.CLEAN_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a.size else None
        rc = lib().ramcrc_replay_table_clean_size_host(self._h, p(victims), victims.size, p(usage),
                                                       _c.c_void_p(summary.ctypes.data))
        _check(rc, "ramcrc_replay_table_clean_size_host")
        return usage, summary[0]

    def clean(self, victims, out_capacity, out_entries_cap, want_moved=True, fill=0):
        """Clean batches out of the table (ramcrc_replay_table_clean_host): the
        victims' live records move to one survivor segment, which becomes the
        next batch; the victims' arrays are released.  Returns a dict: out
        (uint8 [out_capacity]), cert (a segments.CERT_DTYPE scalar), status
        (uint32 [1, 4]), entries (uint32 [out_entries_cap, 4]), n_entries, work
        (uint64 [out_entries_cap]), moved (segments.REPLAY_REF_DTYPE
        [out_entries_cap] or None), usage, summary, batch.  Every output array
        starts as bytes of `fill`.  Raises RamcrcError (code EINVAL) for bad
        arguments and where the survivors do not fit; in the latter case the
        table is spoiled and the exception carries the dict as `.outputs`."""
        from . import segments as _seg
        victims = np.ascontiguousarray(victims, np.uint32).reshape(-1)
        ecap = int(out_entries_cap)

        def mk(shape, dt):
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            return np.full(nbytes, fill, np.uint8).view(dt).reshape(shape)

        out = mk((int(out_capacity),), np.uint8)
        cert = mk((1,), _seg.CERT_DTYPE)
        status = mk((1, 4), np.uint32)
        entries = mk((ecap, 4), np.uint32)
        n_entries = mk((1,), np.uint64)
        work = mk((ecap,), np.uint64)
        moved = mk((ecap,), _seg.REPLAY_REF_DTYPE) if want_moved else None
        usage = mk((victims.size,), _seg.CLEAN_USAGE_DTYPE)
        summary = mk((1,), _seg.CLEAN_SUMMARY_DTYPE)
        none = 0xFFFFFFFF
        batch = _c.c_uint32(none)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_clean_host(
            self._h, p(victims), victims.size, p(out), out.size, _c.c_void_p(cert.ctypes.data),
            _c.c_void_p(status.ctypes.data), p(entries), ecap, _c.c_void_p(n_entries.ctypes.data),
            p(work), p(moved), p(usage), _c.c_void_p(summary.ctypes.data), _c.byref(batch))
        res = dict(out=out, cert=cert[0], status=status, entries=entries, n_entries=n_entries,
                   work=work, moved=moved, usage=usage, summary=summary[0], batch=batch.value)
        if batch.value != none:   # the number is taken: the victims are retired
            for b in victims:
                self._keep[int(b)] = None
            # the rows the table reads: those past the count hold the fill
            n = 0 if int(summary[0]["spoiled"]) else int(n_entries[0])
            self._keep.append((out, status, entries[:n], None, work[:n]))
        try:
            _check(rc, "ramcrc_replay_table_clean_host")
        except RamcrcError as e:
            if batch.value != none:   # (not an argument error: the call ran and refused)
                e.outputs = res
            raise
        return res

    def migrate(self, batches, table_id, out_capacity, max_segments, first_hash=0,
                last_hash=0xFFFFFFFFFFFFFFFF, live_only=False, start=(0, 0), out_stride=None,
                want_sent=True, sent_cap=None, fill=0, flags=None):
        """Migrate a tablet out of the table (ramcrc_replay_table_migrate_host):
        the objects and tombstones of table_id with a record hash in
        [first_hash, last_hash], from the listed batches in order from the
        cursor `start` = (list index, record), packed into at most max_segments
        transfer segments of out_capacity bytes.  Returns a dict: out (uint8
        [max_segments, out_stride]), certs (segments.CERT_DTYPE [max_segments]),
        counts (segments.MIGRATE_COUNT_DTYPE [max_segments]), sent
        (segments.REPLAY_REF_DTYPE [sent_cap] or None), seg_first (uint64
        [max_segments]), summary (a segments.MIGRATE_SUMMARY_DTYPE scalar).
        Every output array starts as bytes of `fill`; the table does not
        change."""
        from . import segments as _seg
        batches = np.ascontiguousarray(batches, np.uint32).reshape(-1)
        stride = int(out_capacity if out_stride is None else out_stride)
        nseg = int(max_segments)
        if flags is None:
            flags = MIGRATE_LIVE_ONLY if live_only else 0

        def mk(shape, dt):
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            return np.full(nbytes, fill, np.uint8).view(dt).reshape(shape)

        if want_sent and sent_cap is None:
            sent_cap = sum(self._keep[int(b)][2].shape[0] for b in batches
                           if int(b) < len(self._keep) and self._keep[int(b)] is not None)
        out = mk((nseg, stride), np.uint8)
        certs = mk((nseg,), _seg.CERT_DTYPE)
        counts = mk((nseg,), _seg.MIGRATE_COUNT_DTYPE)
        sent = mk((int(sent_cap),), _seg.REPLAY_REF_DTYPE) if want_sent else None
        seg_first = mk((nseg,), np.uint64)
        summary = mk((1,), _seg.MIGRATE_SUMMARY_DTYPE)
        p = lambda a: _c.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rc = lib().ramcrc_replay_table_migrate_host(
            self._h, p(batches), batches.size, int(table_id), int(first_hash), int(last_hash), int(flags),
            int(start[0]), int(start[1]), p(out), int(out_capacity), stride, nseg, p(certs), p(counts),
            _c.c_void_p(sent.ctypes.data) if sent is not None else None,
            int(sent_cap) if want_sent else 0, p(seg_first), _c.c_void_p(summary.ctypes.data))
        _check(rc, "ramcrc_replay_table_migrate_host")
        return dict(out=out, certs=certs, counts=counts, sent=sent, seg_first=seg_first,
                    summary=summary[0])


MIGRATE_LIVE_ONLY = 1


# ---------------------------------------------------------------- device
def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return _c.c_void_p(t)
    return _c.c_void_p(t.data_ptr())


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    if isinstance(stream, CuMaskStream):
        return _c.c_void_p(stream.handle)
    if isinstance(stream, int):
        return _c.c_void_p(stream)
    return _c.c_void_p(stream.cuda_stream)


class CuMaskStream:
    """A HIP stream whose kernels run only on the given CUs
    (ramcrc_stream_create_cu_mask).  Pass it as stream= (it converts to the
    raw stream handle); destroy() after the work on it has finished."""

    def __init__(self, device, cus):
        import numpy as np
        mask = np.zeros(8, np.uint32)
        for cu in cus:
            mask[cu // 32] |= np.uint32(1 << (cu % 32))
        words = int(max(cu for cu in cus) // 32 + 1)
        h = _c.c_void_p()
        _check(lib().ramcrc_stream_create_cu_mask(int(device), _c.c_void_p(mask.ctypes.data), words,
                                                  _c.byref(h)), "ramcrc_stream_create_cu_mask")
        self.handle = h.value
        self.ncu = len(set(cus))

    def __int__(self):
        return self.handle

    def destroy(self):
        if self.handle:
            lib().ramcrc_stream_destroy(_c.c_void_p(self.handle))
            self.handle = None


class Context:
    """A libramcrc context on one GPU (scratch + staging).  One per stream/thread."""

    def __init__(self, device=0):
        h = _c.c_void_p()
        _check(lib().ramcrc_ctx_create(int(device), _c.byref(h)), "ramcrc_ctx_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if self._h:
            lib().ramcrc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_timing(self, enable=True):
        _check(lib().ramcrc_ctx_set_timing(self._h, 1 if enable else 0), "ramcrc_ctx_set_timing")

    def scan_time(self):
        """(summed scan-kernel milliseconds, launches) since the last call."""
        ms = _c.c_double(0)
        n = _c.c_uint64(0)
        _check(lib().ramcrc_ctx_scan_time(self._h, _c.byref(ms), _c.byref(n)), "ramcrc_ctx_scan_time")
        return ms.value, n.value

    def status(self):
        s = _c.c_uint32(0)
        _check(lib().ramcrc_ctx_status(self._h, _c.byref(s)), "ramcrc_ctx_status")
        return s.value

    def check(self, stream=None):
        """Wait for `stream`; raise if any launch of this context was refused
        since the last check (ramcrc_ctx_check)."""
        _check(lib().ramcrc_ctx_check(self._h, _stream(stream)), "ramcrc_ctx_check")

    def set_serial_walk(self, enable=True):
        """Walk segments with one wavefront each (the serial chase) instead of
        the parallel walk (RAMCRC_OPT_SERIAL_WALK)."""
        _check(lib().ramcrc_ctx_set_option(self._h, 1, 1 if enable else 0), "ramcrc_ctx_set_option")

    def set_walk_part_shift(self, shift):
        """log2 of the parallel walk's part size, 13..20, forced for every
        batch; 0 = the default, chosen per batch from the entry density
        (RAMCRC_OPT_WALK_PART_SHIFT)."""
        _check(lib().ramcrc_ctx_set_option(self._h, 2, int(shift)), "ramcrc_ctx_set_option")

    def debug_bins(self):
        """Diagnostics: (count[161], cursor[2][161], hist[2][161], next parity)."""
        buf = np.zeros(5 * 161, np.uint64)
        par = _c.c_uint32(0)
        _check(lib().ramcrc_ctx_debug_bins(self._h, _c.c_void_p(buf.ctypes.data), buf.size,
                                           _c.byref(par)), "ramcrc_ctx_debug_bins")
        return buf[:161], buf[161:483].reshape(2, 161), buf[483:].reshape(2, 161), par.value

    def bin_rescues(self):
        """One-launch binnings of this context that aborted (part of the grid
        not dispatched in time) and completed through the two-launch path."""
        buf = np.zeros(5 * 161 + 1, np.uint64)
        par = _c.c_uint32(0)
        _check(lib().ramcrc_ctx_debug_bins(self._h, _c.c_void_p(buf.ctypes.data), buf.size,
                                           _c.byref(par)), "ramcrc_ctx_debug_bins")
        return int(buf[-1])

    def set_option(self, option, value):
        """ramcrc_ctx_set_option (OPT_* above)."""
        _check(lib().ramcrc_ctx_set_option(self._h, int(option), int(value)), "ramcrc_ctx_set_option")

    def set_cus(self, ncu):
        """Size this context's persistent grids for ncu CUs (0 = all): for
        launches on a CU-masked stream (see cu_mask_stream)."""
        _check(lib().ramcrc_ctx_set_cus(self._h, int(ncu)), "ramcrc_ctx_set_cus")

    def reserve(self, max_chunks, max_entries):
        _check(lib().ramcrc_ctx_reserve(self._h, max_chunks, max_entries), "ramcrc_ctx_reserve")

    def index_lookup(self, index, qkeys, queries, out_hashes, results, summary, qkeys_bytes=None,
                     n_queries=None, out_capacity=None, stream=None):
        """A batch of lookupIndexKeys over a built index, on the device
        (ramcrc_index_lookup_device).  index: an Index of CUDA tensors, as
        ReplayTable.index_build returns it; the number of entries is read from
        its summary on the device, so a build and a lookup chain on one stream.
        qkeys: uint8 CUDA, the queries' keys (qkeys_bytes default:
        qkeys.numel()); queries: CUDA holding n segments.INDEX_QUERY_DTYPE
        records (40 bytes each, 8-byte aligned; n_queries default: its bytes /
        40); out_hashes: int64 CUDA out (out_capacity in hashes, default
        out_hashes.numel()); results: CUDA out, 48 bytes a query
        (segments.INDEX_RESULT_DTYPE); summary: int64 CUDA [6] out
        (segments.INDEX_LOOKUP_SUMMARY_DTYPE).  out_hashes goes to
        ReplayTable.read_hashes unchanged.  Asynchronous;
        segments.index_lookup_hashes splits the reply on the host."""
        nbytes = lambda x: 0 if x is None else x.numel() * x.element_size()
        if qkeys_bytes is None:
            qkeys_bytes = nbytes(qkeys)
        if n_queries is None:
            n_queries = nbytes(queries) // 40
        if out_capacity is None:
            out_capacity = nbytes(out_hashes) // 8
        if nbytes(queries) < 40 * n_queries or nbytes(results) < 48 * n_queries:
            raise RamcrcError("Context.index_lookup: queries or results are smaller than n_queries")
        if nbytes(out_hashes) < 8 * out_capacity:
            raise RamcrcError("Context.index_lookup: out_hashes is smaller than out_capacity")
        if nbytes(summary) < 48 or nbytes(index.summary) < 56:
            raise RamcrcError("Context.index_lookup: a summary is too small")
        rc = lib().ramcrc_index_lookup_device(
            self._h, _ptr(index.entries), _ptr(index.hashes), _ptr(index.index_keys), _ptr(index.summary),
            _ptr(qkeys) if qkeys_bytes else None, int(qkeys_bytes), _ptr(queries) if n_queries else None,
            int(n_queries), _ptr(out_hashes) if out_capacity else None, int(out_capacity),
            _ptr(results) if n_queries else None, _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_index_lookup_device")
        return out_hashes

    # All tensors below are CUDA tensors; outputs are int32 tensors holding the
    # uint32 CRC bit patterns.
    def segments(self, data, seg_bytes, nseg, out, init=None, finalize=True, stream=None):
        rc = lib().ramcrc_segments_device(self._h, _ptr(data), seg_bytes, nseg, _ptr(init),
                                          _ptr(out), FINALIZE if finalize else 0, _stream(stream))
        _check(rc, "ramcrc_segments_device")
        return out

    def batch(self, data, off, length, out, init=None, finalize=True, stream=None):
        n = off.numel()
        fl = FINALIZE if finalize else 0
        rc = lib().ramcrc_batch_device(self._h, _ptr(data), _ptr(off), _ptr(length), _ptr(init),
                                       _ptr(out), n, fl, _stream(stream))
        _check(rc, "ramcrc_batch_device")
        return out

    def entries(self, data, off, length, out, init=None, finalize=True, stream=None):
        n = off.numel()
        fl = FINALIZE if finalize else 0
        rc = lib().ramcrc_entries_device(self._h, _ptr(data), _ptr(off), _ptr(length), _ptr(init),
                                         _ptr(out), n, fl, _stream(stream))
        _check(rc, "ramcrc_entries_device")
        return out

    def segment_walk(self, data, seg_stride, seg_capacity, nseg, certs, status, entries,
                     n_entries, stream=None):
        """Segment::checkMetadataIntegrity on the device.  certs: int32 [nseg, 2]
        (segment_length, checksum); status: int32 [nseg, 4]; entries: int32
        [cap, 4]; n_entries: int64 [1]."""
        cap = 0 if entries is None else entries.shape[0]
        rc = lib().ramcrc_segment_walk_device(self._h, _ptr(data), seg_stride, seg_capacity, nseg,
                                              _ptr(certs), _ptr(status), _ptr(entries), cap,
                                              _ptr(n_entries), _stream(stream))
        _check(rc, "ramcrc_segment_walk_device")
        return status

    def certify(self, data, seg_stride, seg_capacity, nseg, heads, certs, flags=None, stream=None):
        """Segment::getAppendedLength's certificate for nseg rebuilt segments
        (ramcrc_segments_certify_device).  heads: int32 CUDA [nseg]; certs:
        int32 CUDA [nseg, 2] out; flags: int32 CUDA [nseg] out or None."""
        rc = lib().ramcrc_segments_certify_device(self._h, _ptr(data), seg_stride, seg_capacity, nseg,
                                                  _ptr(heads), _ptr(certs), _ptr(flags),
                                                  _stream(stream))
        _check(rc, "ramcrc_segments_certify_device")
        return certs

    def recovery_append(self, data, seg_stride, nseg, status, entries, n_entries, place, n_place,
                        n_part, out, out_stride, out_capacity, out_certs, out_status, stream=None):
        """Append walked records into per-partition recovery segments and seal
        them (ramcrc_recovery_append_device).  status, entries, n_entries: a
        walk's tables; place: int32 CUDA [cap, 2] (record, partition), not
        decreasing in record; n_place: int64 CUDA [1]; out: uint8 CUDA holding
        nseg * n_part outputs at out_stride; out_certs, out_status: int32 CUDA
        [nseg * n_part, 2].  Asynchronous; a refused list shows in check()."""
        ecap = 0 if entries is None else entries.shape[0]
        pcap = 0 if place is None else place.shape[0]
        rc = lib().ramcrc_recovery_append_device(
            self._h, _ptr(data), seg_stride, nseg, _ptr(status), _ptr(entries), ecap,
            _ptr(n_entries), _ptr(place), pcap, _ptr(n_place), n_part, _ptr(out), out_stride,
            out_capacity, _ptr(out_certs), _ptr(out_status), _stream(stream))
        _check(rc, "ramcrc_recovery_append_device")
        return out_certs

    def replay_sidelog(self, data, seg_stride, nseg, status, entries, n_entries, live, n_live,
                       timestamp, out, out_stride, out_capacity, out_certs, out_status, counts,
                       refs=None, stream=None):
        """The side log of a replay (ramcrc_replay_sidelog_device): the append
        at one partition over a live list (replay_resolve's or
        ReplayTable.live's), kept tombstones rewritten with segmentId 0,
        `timestamp` and a recomputed checksum.  Tensors as recovery_append
        takes them; counts: int64 CUDA [7] out (segments.SIDELOG_COUNTS_DTYPE);
        refs: int32 CUDA [cap, 2] out (output, offset) or None.  timestamp is
        passed by value: a captured graph replays the captured one.
        Asynchronous; a refused list shows in check()."""
        ecap = 0 if entries is None else entries.shape[0]
        lcap = 0 if live is None else live.shape[0]
        if refs is not None and refs.shape[0] < lcap:
            raise RamcrcError("replay_sidelog: fewer refs than the live list holds")
        rc = lib().ramcrc_replay_sidelog_device(
            self._h, _ptr(data), seg_stride, nseg, _ptr(status), _ptr(entries), ecap,
            _ptr(n_entries), _ptr(live), lcap, _ptr(n_live), int(timestamp), _ptr(out), out_stride,
            out_capacity, _ptr(out_certs), _ptr(out_status), _ptr(refs), _ptr(counts),
            _stream(stream))
        _check(rc, "ramcrc_replay_sidelog_device")
        return out_certs

    def recovery_partition(self, data, seg_stride, nseg, status, entries, n_entries, tablets,
                           n_part, place, n_place, part_status, key_hash=None, n_tablets=None,
                           stream=None):
        """RecoverySegmentBuilder::build's placement decision for a walk's
        records (ramcrc_recovery_partition_device): key hash, tablet lookup,
        liveness.  status, entries, n_entries: a walk's tables; tablets: uint8
        CUDA holding segments.TABLET_DTYPE records (segments.tablets_tensor);
        place: int32 CUDA [cap, 2] out and n_place: int64 CUDA [1] out, as
        recovery_append takes them; part_status: int32 CUDA [nseg, 4] out
        (flags, placed, unplaced, dead); key_hash: int64 CUDA [entries] out or
        None.  Asynchronous; a refusal shows in check()."""
        ecap = 0 if entries is None else entries.shape[0]
        pcap = 0 if place is None else place.shape[0]
        if n_tablets is None:
            n_tablets = 0 if tablets is None else tablets.numel() * tablets.element_size() // 40
        rc = lib().ramcrc_recovery_partition_device(
            self._h, _ptr(data), seg_stride, nseg, _ptr(status), _ptr(entries), ecap,
            _ptr(n_entries), _ptr(tablets), n_tablets, n_part, _ptr(place), pcap, _ptr(n_place),
            _ptr(key_hash), _ptr(part_status), _stream(stream))
        _check(rc, "ramcrc_recovery_partition_device")
        return place

    def replay_resolve(self, data, seg_stride, nseg, status, entries, n_entries, live, n_live,
                       counts, key_hash=None, winner=None, stream=None):
        """Which replayed objects and tombstones a recovery master keeps
        (ramcrc_replay_resolve_device): per key the highest version, a
        tombstone before an object of the same version.  status, entries,
        n_entries: a walk's tables; key_hash: int64 CUDA [entries] (the
        partition call's output) or None (computed); winner: int32 CUDA
        [entries] out or None; live: int32 CUDA [cap, 2] out and n_live: int64
        CUDA [1] out, as recovery_append takes them with n_part = 1; counts:
        int64 CUDA [6] out (segments.RESOLVE_COUNTS_DTYPE).  Asynchronous; a
        refusal shows in check()."""
        ecap = 0 if entries is None else entries.shape[0]
        lcap = 0 if live is None else live.shape[0]
        rc = lib().ramcrc_replay_resolve_device(
            self._h, _ptr(data), seg_stride, nseg, _ptr(status), _ptr(entries), ecap,
            _ptr(n_entries), _ptr(key_hash), _ptr(winner), _ptr(live), lcap, _ptr(n_live),
            _ptr(counts), _stream(stream))
        _check(rc, "ramcrc_replay_resolve_device")
        return live

    def verify_objects(self, data, seg_stride, entries, n_entries, obj_crc, status, stream=None):
        """Object::computeChecksum + comparison for every object record of a walk."""
        rc = lib().ramcrc_verify_objects_device(self._h, _ptr(data), seg_stride, _ptr(entries),
                                                entries.shape[0], _ptr(n_entries), _ptr(obj_crc),
                                                _ptr(status), _stream(stream))
        _check(rc, "ramcrc_verify_objects_device")
        return status

    def replay_verify(self, data, seg_stride, seg_capacity, nseg, certs, status, entries, n_entries,
                      obj_crc, stream=None):
        """segment_walk + verify_objects in one call (ramcrc_replay_verify_device):
        same results; skips the binning pass when every record is a one-window
        object."""
        cap = 0 if entries is None else entries.shape[0]
        rc = lib().ramcrc_replay_verify_device(self._h, _ptr(data), seg_stride, seg_capacity, nseg,
                                               _ptr(certs), _ptr(status), _ptr(entries), cap,
                                               _ptr(n_entries), _ptr(obj_crc), _stream(stream))
        _check(rc, "ramcrc_replay_verify_device")
        return status

    def fill_objects(self, data, seg_stride, capacity, nseg, value_len, first_key=0, certs=None):
        """RecoverSegmentBenchmark-shaped object segments built in place on the
        device (ramcrc_segment_fill_objects_device): returns (objects per
        segment, segment_length, checksum); certs (int32 CUDA [nseg, 2]) gets
        every segment's certificate when given.  Synchronous."""
        cert = np.zeros(2, dtype=np.uint32)
        per = _c.c_uint32(0)
        rc = lib().ramcrc_segment_fill_objects_device(
            self._h, _ptr(data), seg_stride, capacity, nseg, value_len, first_key, _ptr(certs),
            _c.c_void_p(cert.ctypes.data), _c.byref(per))
        _check(rc, "ramcrc_segment_fill_objects_device")
        return per.value, int(cert[0]), int(cert[1])

    def assemble_objects(self, data, off, length, out=None, stream=None):
        """Object::assembleForLog's checksum for serialized objects in `data`
        (uint8 CUDA tensor, modified in place): header.checksum of object i
        (bytes [off[i], off[i]+4)) = Crc32C over bytes [4, length[i])."""
        n = off.numel()
        rc = lib().ramcrc_assemble_objects_device(self._h, _ptr(data), _ptr(off), _ptr(length),
                                                  _ptr(out), n, _stream(stream))
        _check(rc, "ramcrc_assemble_objects_device")
        return out

    def assemble_objects_host(self, objects):
        """Same for host objects (writable contiguous numpy uint8 arrays),
        stamped in place."""
        for o in objects:
            if not (isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.flags.c_contiguous
                    and o.flags.writeable):
                raise RamcrcError("objects must be writable contiguous numpy uint8 arrays")
        n = len(objects)
        ptrs = (_c.c_void_p * max(n, 1))(*[o.ctypes.data for o in objects])
        lens = np.array([o.size for o in objects], dtype=np.uint64)
        rc = lib().ramcrc_assemble_objects_host(self._h, ptrs, _c.c_void_p(lens.ctypes.data), n)
        _check(rc, "ramcrc_assemble_objects_host")

    def batch_host(self, buffers, init=None, finalize=True):
        """CRC a list of host buffers (bytes / numpy) on the GPU; returns np.uint32."""
        arrs = [_buf(b)[0] for b in buffers]
        n = len(arrs)
        ptrs = (_c.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.uint64)
        out = np.zeros(n, dtype=np.uint32)
        init_a = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
        rc = lib().ramcrc_batch_host(self._h, ptrs, _c.c_void_p(lens.ctypes.data),
                                     None if init_a is None else _c.c_void_p(init_a.ctypes.data),
                                     _c.c_void_p(out.ctypes.data), n,
                                     FINALIZE if finalize else 0)
        _check(rc, "ramcrc_batch_host")
        return out

    def stream_host(self, host_segments, seg_bytes, nseg, finalize=True, batch=8, depth=3):
        """Host-to-host streaming CRC (config 5).  host_segments: numpy uint8 or a
        pinned torch CPU tensor; returns np.uint32[nseg]."""
        out = np.zeros(nseg, dtype=np.uint32)
        if hasattr(host_segments, "data_ptr"):
            base = _c.c_void_p(host_segments.data_ptr())
        else:
            base = _c.c_void_p(np.ascontiguousarray(host_segments).ctypes.data)
        rc = lib().ramcrc_stream_host(self._h, base, seg_bytes, nseg, _c.c_void_p(out.ctypes.data),
                                      FINALIZE if finalize else 0, batch, depth)
        _check(rc, "ramcrc_stream_host")
        return out


class ReplayTable:
    """A replay table on the GPU that outlives a call (ramcrc_replay_table_*):
    Context.replay_resolve's decision fed batch by batch.  Every tensor given
    to add() must stay allocated and unchanged until reset() or close(); the
    table holds references to them for that long.  Close it before ctx."""

    def __init__(self, ctx, key_cap, max_batches):
        h = _c.c_void_p()
        _check(lib().ramcrc_replay_table_create(ctx._h, int(key_cap), int(max_batches),
                                                _c.byref(h)), "ramcrc_replay_table_create")
        self._h = h
        self._ctx = ctx
        self._keep = []

    def close(self):
        if self._h:
            lib().ramcrc_replay_table_destroy(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=None):
        """Empty the table and forget its batches; stream-ordered."""
        _check(lib().ramcrc_replay_table_reset(self._h, _stream(stream)),
               "ramcrc_replay_table_reset")
        self._keep = []

    def add(self, data, seg_stride, nseg, status, entries, n_entries, work, key_hash=None,
            stream=None):
        """Resolve one walk's records into the table.  status, entries,
        n_entries: the walk's tables; work: int64 CUDA [entries], written here
        and read by live(); key_hash: int64 CUDA [entries] (the partition
        call's output) or None (computed).  Returns the batch number.
        Asynchronous; a spoiled table shows in Context.check() and stats()."""
        ecap = 0 if entries is None else entries.shape[0]
        if ecap and (work is None or work.numel() < ecap):
            raise RamcrcError("ReplayTable.add: work is smaller than the record table")
        batch = _c.c_uint32(0)
        rc = lib().ramcrc_replay_table_add_device(
            self._h, _ptr(data), seg_stride, nseg, _ptr(status), _ptr(entries), ecap,
            _ptr(n_entries), _ptr(key_hash), _ptr(work), _c.byref(batch), _stream(stream))
        _check(rc, "ramcrc_replay_table_add_device")
        self._keep.append((data, status, entries, n_entries, key_hash, work))
        return batch.value

    def live(self, batch, live, n_live, counts, winner=None, stream=None):
        """The verdict on one batch as the table stands now.  live: int32 CUDA
        [cap, 2] out and n_live: int64 CUDA [1] out, as recovery_append takes
        them with n_part = 1 over that batch's segments; counts: int64 CUDA
        [6] out (segments.RESOLVE_COUNTS_DTYPE); winner: int32 CUDA [entries,
        2] out (segments.REPLAY_REF_DTYPE) or None.  Asynchronous."""
        lcap = 0 if live is None else live.shape[0]
        rc = lib().ramcrc_replay_table_live_device(
            self._h, int(batch), _ptr(winner), _ptr(live), lcap, _ptr(n_live), _ptr(counts),
            _stream(stream))
        _check(rc, "ramcrc_replay_table_live_device")
        return live

    def stats(self, stats, stream=None):
        """The whole table into stats: int64 CUDA [6] out
        (segments.REPLAY_TABLE_STATS_DTYPE).  Asynchronous."""
        _check(lib().ramcrc_replay_table_stats_device(self._h, _ptr(stats), _stream(stream)),
               "ramcrc_replay_table_stats_device")
        return stats

    def lookup(self, keys, queries, results, counts=None, key_hash=None, keys_bytes=None,
               n_queries=None, stream=None):
        """What the table holds for each key, as it stands now.  keys: uint8
        CUDA, the key buffer (keys_bytes: its length, default keys.numel());
        queries: CUDA holding n segments.LOOKUP_KEY_DTYPE records (24 bytes
        each, 8-byte aligned; n_queries default: its bytes / 24); results: CUDA
        out, 32 bytes a query (segments.LOOKUP_RESULT_DTYPE), 16-byte aligned;
        counts: int64 CUDA [5] out (segments.LOOKUP_COUNTS_DTYPE) or None;
        key_hash: int64 CUDA [n] or None (computed).  Read-only on the table.
        Asynchronous."""
        if keys_bytes is None:
            keys_bytes = 0 if keys is None else keys.numel() * keys.element_size()
        if n_queries is None:
            n_queries = 0 if queries is None else queries.numel() * queries.element_size() // 24
        if n_queries and (results is None or results.numel() * results.element_size() < 32 * n_queries):
            raise RamcrcError("ReplayTable.lookup: results is smaller than the queries")
        if key_hash is not None and key_hash.numel() < n_queries:
            raise RamcrcError("ReplayTable.lookup: fewer hashes than queries")
        rc = lib().ramcrc_replay_table_lookup_device(
            self._h, _ptr(keys) if keys_bytes else None, int(keys_bytes), _ptr(queries),
            int(n_queries), _ptr(key_hash), _ptr(results), _ptr(counts), _stream(stream))
        _check(rc, "ramcrc_replay_table_lookup_device")
        return results

    def read(self, keys, queries, reply, summary, rules=None, value_only=False, part_off=None,
             results=None, key_hash=None, keys_bytes=None, n_queries=None, reply_cap=None,
             stream=None):
        """A multi-read's reply, packed on the device
        (ramcrc_replay_table_read_device).  keys, queries, key_hash, keys_bytes,
        n_queries as lookup takes them; reply: uint8 CUDA out, any alignment
        (reply_cap: its limit in bytes, default reply.numel()); summary: int64
        CUDA [10] out (segments.READ_SUMMARY_DTYPE); rules: CUDA holding n
        segments.REJECT_RULES_DTYPE records (16 bytes each, 8-byte aligned) or
        None: no rules; part_off: int64 CUDA [n] out or None; results: CUDA
        out as lookup's or None.  The reply must not overlap an added batch.
        Asynchronous; segments.multi_read_parts splits the reply on the host."""
        if keys_bytes is None:
            keys_bytes = 0 if keys is None else keys.numel() * keys.element_size()
        if n_queries is None:
            n_queries = 0 if queries is None else queries.numel() * queries.element_size() // 24
        if reply_cap is None:
            reply_cap = 0 if reply is None else reply.numel() * reply.element_size()
        nbytes = lambda x: x.numel() * x.element_size()
        if reply_cap and (reply is None or nbytes(reply) < reply_cap):
            raise RamcrcError("ReplayTable.read: reply is smaller than reply_cap")
        if results is not None and nbytes(results) < 32 * n_queries:
            raise RamcrcError("ReplayTable.read: results is smaller than the queries")
        if part_off is not None and nbytes(part_off) < 8 * n_queries:
            raise RamcrcError("ReplayTable.read: part_off is smaller than the queries")
        if rules is not None and nbytes(rules) < 16 * n_queries:
            raise RamcrcError("ReplayTable.read: fewer rules than queries")
        if key_hash is not None and key_hash.numel() < n_queries:
            raise RamcrcError("ReplayTable.read: fewer hashes than queries")
        rc = lib().ramcrc_replay_table_read_device(
            self._h, _ptr(keys) if keys_bytes else None, int(keys_bytes), _ptr(queries),
            int(n_queries), _ptr(key_hash), _ptr(rules),
            1 if value_only else 0, _ptr(reply) if reply_cap else None, int(reply_cap),
            _ptr(part_off), _ptr(results), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_read_device")
        return reply

    def read_hashes(self, table_id, hashes, reply, summary, max_length, parts=None, n_hashes=None,
                    reply_capacity=None, stream=None):
        """An indexed read's reply, packed on the device
        (ramcrc_replay_table_read_hashes_device): for every asked primary-key
        hash the objects of table_id whose record hash equals it.  hashes:
        int64 CUDA [n] (n_hashes default: hashes.numel()); reply: uint8 CUDA
        out, any alignment (reply_capacity: its size in bytes, default
        reply.numel()); max_length: the reference's maxLength, which the reply
        may pass by one hash's parts; summary: int64 CUDA [9] out
        (segments.READ_HASHES_SUMMARY_DTYPE); parts: CUDA out, 16 bytes a hash
        (segments.HASH_PART_DTYPE), 8-byte aligned, or None.  The reply must
        not overlap an added batch.  Read-only on the table.  Asynchronous;
        segments.read_hashes_objects splits the reply on the host."""
        if n_hashes is None:
            n_hashes = 0 if hashes is None else hashes.numel()
        if reply_capacity is None:
            reply_capacity = 0 if reply is None else reply.numel() * reply.element_size()
        nbytes = lambda x: x.numel() * x.element_size()
        if reply_capacity and (reply is None or nbytes(reply) < reply_capacity):
            raise RamcrcError("ReplayTable.read_hashes: reply is smaller than reply_capacity")
        if n_hashes and (hashes is None or nbytes(hashes) < 8 * n_hashes):
            raise RamcrcError("ReplayTable.read_hashes: fewer hashes than n_hashes")
        if parts is not None and nbytes(parts) < 16 * n_hashes:
            raise RamcrcError("ReplayTable.read_hashes: parts is smaller than the hashes")
        if summary is None or nbytes(summary) < 72:
            raise RamcrcError("ReplayTable.read_hashes: summary is smaller than 72 bytes")
        rc = lib().ramcrc_replay_table_read_hashes_device(
            self._h, int(table_id), _ptr(hashes) if n_hashes else None, int(n_hashes), 0,
            _ptr(reply) if reply_capacity else None, int(reply_capacity), int(max_length),
            _ptr(parts), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_read_hashes_device")
        return reply

    def enumerate(self, table_id, payload, summary, max_bytes, first_hash=0,
                  last_hash=0xFFFFFFFFFFFFFFFF, bucket_index=0, bucket_next_hash=0, bucket_limit=0,
                  stale=None, keys_only=False, payload_capacity=None, stream=None):
        """One reply of a table enumeration, packed on the device
        (ramcrc_replay_table_enumerate_device): the objects of table_id with
        first_hash <= hash <= last_hash, bucket by bucket from the cursor
        (bucket_index, bucket_next_hash) up to bucket_limit (0: every bucket),
        as {u32 length, log entry} entries that end within max_bytes.
        payload: uint8 CUDA out, any alignment (payload_capacity: its size in
        bytes, default payload.numel()); summary: int64 CUDA [11] out
        (segments.ENUMERATE_SUMMARY_DTYPE), whose next_bucket and next_hash are
        the cursor to go on with; stale: the iterator's stale frames, host
        memory (segments.enum_frames or its rows), read before the call
        returns; keys_only: entries end before the value.  The payload must
        not overlap an added batch.  Read-only on the table.  Asynchronous;
        segments.enumerate_objects splits the payload on the host."""
        from . import segments as _seg
        if stale is None:
            stale = []
        if not (isinstance(stale, np.ndarray) and stale.dtype == _seg.ENUM_FRAME_DTYPE):
            stale = _seg.enum_frames(stale)
        stale = np.ascontiguousarray(stale)
        if payload_capacity is None:
            payload_capacity = 0 if payload is None else payload.numel() * payload.element_size()
        nbytes = lambda x: x.numel() * x.element_size()
        if payload_capacity and (payload is None or nbytes(payload) < payload_capacity):
            raise RamcrcError("ReplayTable.enumerate: payload is smaller than payload_capacity")
        if summary is None or nbytes(summary) < 88:
            raise RamcrcError("ReplayTable.enumerate: summary is smaller than 88 bytes")
        rc = lib().ramcrc_replay_table_enumerate_device(
            self._h, int(table_id), int(first_hash), int(last_hash), int(bucket_index),
            int(bucket_next_hash), int(bucket_limit),
            _c.c_void_p(stale.ctypes.data) if stale.shape[0] else None, stale.shape[0],
            _seg.ENUM_KEYS_ONLY if keys_only else 0,
            _ptr(payload) if payload_capacity else None, int(payload_capacity), int(max_bytes),
            _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_enumerate_device")
        return payload

    def index_build(self, table_id, index_id, entries, hashes, index_keys, summary, entry_capacity=None,
                    keys_capacity=None, stream=None):
        """The sorted secondary index of table_id's key index_id (>= 1) over the
        table's object winners, built on the device
        (ramcrc_replay_table_index_build_device).  entries: CUDA out, 32 bytes
        an entry (segments.INDEX_ENTRY_DTYPE), 16-byte aligned (entry_capacity
        default: its bytes / 32); hashes: int64 CUDA [entry_capacity] out, the
        dense copy of the entries' hashes; index_keys: uint8 CUDA out, the
        index's own copy of its keys (keys_capacity default:
        index_keys.numel()); summary: int64 CUDA [7] out
        (segments.INDEX_BUILD_SUMMARY_DTYPE).  With the three arrays None and
        both capacities 0 the call only sizes.  Read-only on the table.
        Asynchronous.  Returns an Index holding the four tensors, for
        Context.index_lookup."""
        nbytes = lambda x: 0 if x is None else x.numel() * x.element_size()
        if entry_capacity is None:
            entry_capacity = min(nbytes(entries) // 32, nbytes(hashes) // 8)
        if keys_capacity is None:
            keys_capacity = nbytes(index_keys)
        if nbytes(entries) < 32 * entry_capacity or nbytes(hashes) < 8 * entry_capacity:
            raise RamcrcError("ReplayTable.index_build: entries or hashes are smaller than entry_capacity")
        if nbytes(index_keys) < keys_capacity:
            raise RamcrcError("ReplayTable.index_build: index_keys is smaller than keys_capacity")
        if nbytes(summary) < 56:
            raise RamcrcError("ReplayTable.index_build: summary is smaller than 56 bytes")
        rc = lib().ramcrc_replay_table_index_build_device(
            self._h, int(table_id), int(index_id), _ptr(entries) if entry_capacity else None,
            int(entry_capacity), _ptr(hashes) if entry_capacity else None,
            _ptr(index_keys) if keys_capacity else None, int(keys_capacity), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_index_build_device")
        return Index(entries, hashes, index_keys, summary)

    def write(self, data, reqs, out, out_cert, parts, summary, next_version, timestamp=0,
              rules=None, key_hash=None, batch_segment_id=None, refs=None, old=None,
              data_bytes=None, n_reqs=None, out_capacity=None, stream=None):
        """A multi-write on the device (ramcrc_replay_table_write_device): the
        table is not changed; out becomes the log segment to walk (with
        out_cert) and add as the next batch.  data: uint8 CUDA, the keysAndValue
        images (data_bytes: its length, default data.numel()); reqs: CUDA holding
        n segments.WRITE_REQ_DTYPE records (24 bytes each, 8-byte aligned; n_reqs
        default: its bytes / 24); out: uint8 CUDA out, any alignment
        (out_capacity default out.numel()); out_cert: int32 CUDA [2] out
        (segments.CERT_DTYPE); parts: CUDA out, 12 bytes a request
        (segments.WRITE_PART_DTYPE), 4-byte aligned; summary: int64 CUDA [16] out
        (segments.WRITE_SUMMARY_DTYPE); rules, key_hash as read takes them;
        batch_segment_id: int64 CUDA [batches] or None; refs: int32 CUDA [n, 2]
        out or None; old: CUDA out as lookup's results or None.  Asynchronous."""
        nbytes = lambda x: x.numel() * x.element_size()
        if data_bytes is None:
            data_bytes = 0 if data is None else nbytes(data)
        if n_reqs is None:
            n_reqs = 0 if reqs is None else nbytes(reqs) // 24
        if out_capacity is None:
            out_capacity = 0 if out is None else nbytes(out)
        if out_capacity and (out is None or nbytes(out) < out_capacity):
            raise RamcrcError("ReplayTable.write: out is smaller than out_capacity")
        if n_reqs and (parts is None or nbytes(parts) < 12 * n_reqs):
            raise RamcrcError("ReplayTable.write: parts is smaller than the requests")
        if refs is not None and nbytes(refs) < 8 * n_reqs:
            raise RamcrcError("ReplayTable.write: refs is smaller than the requests")
        if old is not None and nbytes(old) < 32 * n_reqs:
            raise RamcrcError("ReplayTable.write: old is smaller than the requests")
        if rules is not None and nbytes(rules) < 16 * n_reqs:
            raise RamcrcError("ReplayTable.write: fewer rules than requests")
        if key_hash is not None and key_hash.numel() < n_reqs:
            raise RamcrcError("ReplayTable.write: fewer hashes than requests")
        if out_cert is None or nbytes(out_cert) < 8 or summary is None or nbytes(summary) < 128:
            raise RamcrcError("ReplayTable.write: out_cert or summary is missing or too small")
        rc = lib().ramcrc_replay_table_write_device(
            self._h, _ptr(data) if data_bytes else None, int(data_bytes), _ptr(reqs), int(n_reqs),
            _ptr(key_hash), _ptr(rules), int(next_version), int(timestamp), _ptr(batch_segment_id),
            _ptr(out) if out_capacity else None, int(out_capacity), _ptr(out_cert), _ptr(parts),
            _ptr(refs), _ptr(old), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_write_device")
        return out

    def remove(self, keys, reqs, out, out_cert, parts, summary, next_version, timestamp=0,
               rules=None, key_hash=None, batch_segment_id=None, refs=None, old=None,
               keys_bytes=None, n_reqs=None, out_capacity=None, stream=None):
        """A multi-remove on the device (ramcrc_replay_table_remove_device): the
        table is not changed; out becomes the log segment of tombstones to walk
        (with out_cert) and add as the next batch.  keys: uint8 CUDA, any
        alignment (keys_bytes: its length, default keys.numel()); reqs: CUDA
        holding n segments.LOOKUP_KEY_DTYPE records (24 bytes each, 8-byte
        aligned; n_reqs default: its bytes / 24); out: uint8 CUDA out, any
        alignment (out_capacity default out.numel()); out_cert: int32 CUDA [2]
        out (segments.CERT_DTYPE); parts: CUDA out, 12 bytes a request
        (segments.REMOVE_PART_DTYPE), 4-byte aligned; summary: int64 CUDA [12]
        out (segments.REMOVE_SUMMARY_DTYPE); rules, key_hash as read takes them;
        batch_segment_id: int64 CUDA [batches] or None; refs: int32 CUDA [n] out
        or None; old: CUDA out as lookup's results or None.  Asynchronous."""
        nbytes = lambda x: x.numel() * x.element_size()
        if keys_bytes is None:
            keys_bytes = 0 if keys is None else nbytes(keys)
        if n_reqs is None:
            n_reqs = 0 if reqs is None else nbytes(reqs) // 24
        if out_capacity is None:
            out_capacity = 0 if out is None else nbytes(out)
        if out_capacity and (out is None or nbytes(out) < out_capacity):
            raise RamcrcError("ReplayTable.remove: out is smaller than out_capacity")
        if n_reqs and (parts is None or nbytes(parts) < 12 * n_reqs):
            raise RamcrcError("ReplayTable.remove: parts is smaller than the requests")
        if refs is not None and nbytes(refs) < 4 * n_reqs:
            raise RamcrcError("ReplayTable.remove: refs is smaller than the requests")
        if old is not None and nbytes(old) < 32 * n_reqs:
            raise RamcrcError("ReplayTable.remove: old is smaller than the requests")
        if rules is not None and nbytes(rules) < 16 * n_reqs:
            raise RamcrcError("ReplayTable.remove: fewer rules than requests")
        if key_hash is not None and key_hash.numel() < n_reqs:
            raise RamcrcError("ReplayTable.remove: fewer hashes than requests")
        if out_cert is None or nbytes(out_cert) < 8 or summary is None or nbytes(summary) < 96:
            raise RamcrcError("ReplayTable.remove: out_cert or summary is missing or too small")
        rc = lib().ramcrc_replay_table_remove_device(
            self._h, _ptr(keys) if keys_bytes else None, int(keys_bytes), _ptr(reqs), int(n_reqs),
            _ptr(key_hash), _ptr(rules), int(next_version), int(timestamp), _ptr(batch_segment_id),
            _ptr(out) if out_capacity else None, int(out_capacity), _ptr(out_cert), _ptr(parts),
            _ptr(refs), _ptr(old), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_remove_device")
        return out

    def increment(self, keys, reqs, args, out, out_cert, parts, summary, next_version, timestamp=0,
                  rules=None, key_hash=None, batch_segment_id=None, refs=None, old=None,
                  keys_bytes=None, n_reqs=None, out_capacity=None, stream=None):
        """A multi-increment on the device
        (ramcrc_replay_table_increment_device): the table is not changed; out
        becomes the log segment of new objects and tombstones to walk (with
        out_cert) and add as the next batch.  keys, reqs as remove takes them;
        args: CUDA holding n segments.INCREMENT_ARG_DTYPE records (16 bytes
        each, 8-byte aligned); out: uint8 CUDA out, any alignment (out_capacity
        default out.numel()); out_cert: int32 CUDA [2] out (segments.CERT_DTYPE);
        parts: CUDA out, 20 bytes a request (segments.INCREMENT_PART_DTYPE),
        4-byte aligned; summary: int64 CUDA [18] out
        (segments.INCREMENT_SUMMARY_DTYPE); rules, key_hash as read takes them;
        batch_segment_id: int64 CUDA [batches] or None; refs: int32 CUDA [n, 2]
        out or None; old: CUDA out as lookup's results or None.  Asynchronous."""
        nbytes = lambda x: x.numel() * x.element_size()
        if keys_bytes is None:
            keys_bytes = 0 if keys is None else nbytes(keys)
        if n_reqs is None:
            n_reqs = 0 if reqs is None else nbytes(reqs) // 24
        if out_capacity is None:
            out_capacity = 0 if out is None else nbytes(out)
        if out_capacity and (out is None or nbytes(out) < out_capacity):
            raise RamcrcError("ReplayTable.increment: out is smaller than out_capacity")
        if n_reqs and (args is None or nbytes(args) < 16 * n_reqs):
            raise RamcrcError("ReplayTable.increment: fewer args than requests")
        if n_reqs and (parts is None or nbytes(parts) < 20 * n_reqs):
            raise RamcrcError("ReplayTable.increment: parts is smaller than the requests")
        if refs is not None and nbytes(refs) < 8 * n_reqs:
            raise RamcrcError("ReplayTable.increment: refs is smaller than the requests")
        if old is not None and nbytes(old) < 32 * n_reqs:
            raise RamcrcError("ReplayTable.increment: old is smaller than the requests")
        if rules is not None and nbytes(rules) < 16 * n_reqs:
            raise RamcrcError("ReplayTable.increment: fewer rules than requests")
        if key_hash is not None and key_hash.numel() < n_reqs:
            raise RamcrcError("ReplayTable.increment: fewer hashes than requests")
        if out_cert is None or nbytes(out_cert) < 8 or summary is None or nbytes(summary) < 144:
            raise RamcrcError("ReplayTable.increment: out_cert or summary is missing or too small")
        rc = lib().ramcrc_replay_table_increment_device(
            self._h, _ptr(keys) if keys_bytes else None, int(keys_bytes), _ptr(reqs), int(n_reqs),
            _ptr(args), _ptr(key_hash), _ptr(rules), int(next_version), int(timestamp),
            _ptr(batch_segment_id), _ptr(out) if out_capacity else None, int(out_capacity),
            _ptr(out_cert), _ptr(parts), _ptr(refs), _ptr(old), _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_increment_device")
        return out

    @staticmethod
    def clean_reserve(entries_caps):
        """The max_chunks argument of Context.reserve after which clean and
        clean_size over victims of these record-table capacities do not
        allocate (include/ramcrc.h, rule 11)."""
        caps = [int(x) for x in entries_caps]
        return 2 * (len(caps) + 16 + 16 * sum((x + 255) // 256 for x in caps))

    def clean_size(self, victims, summary, usage=None, stream=None):
        """What clean(victims) would need and move now
        (ramcrc_replay_table_clean_size_device); changes nothing.  victims: a
        sequence of batch numbers; summary: int64 CUDA [14] out
        (segments.CLEAN_SUMMARY_DTYPE); usage: int64 CUDA [n_victims, 4] out
        (segments.CLEAN_USAGE_DTYPE) or None.  Asynchronous."""
        vic = np.ascontiguousarray(victims, np.uint32).reshape(-1)
        nbytes = lambda x: x.numel() * x.element_size()
        if summary is None or nbytes(summary) < 112:
            raise RamcrcError("ReplayTable.clean_size: summary is missing or too small")
        if usage is not None and nbytes(usage) < 32 * vic.size:
            raise RamcrcError("ReplayTable.clean_size: usage is smaller than the victims")
        rc = lib().ramcrc_replay_table_clean_size_device(
            self._h, _c.c_void_p(vic.ctypes.data) if vic.size else None, vic.size, _ptr(usage),
            _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_clean_size_device")
        return summary

    def clean(self, victims, out, out_cert, out_status, out_entries, out_n_entries, out_work,
              summary, moved=None, usage=None, out_capacity=None, stream=None):
        """Clean batches out of the table on the device
        (ramcrc_replay_table_clean_device): the victims' live records move to
        out, which becomes the next batch with out_status (int32 CUDA [1, 4]),
        out_entries (int32 CUDA [cap, 4]), out_n_entries (int64 CUDA [1]) and
        out_work (int64 CUDA [cap]) as a walk and an add would leave them, and
        out_cert (int32 CUDA [2]) as certify would.  out: uint8 CUDA, 16-byte
        aligned (out_capacity, a multiple of 16; default out.numel()); moved:
        int32 CUDA [cap, 2] out (segments.REPLAY_REF_DTYPE) or None; usage,
        summary as clean_size takes them.  The outputs must stay allocated and
        unchanged like an added batch's; the table drops its references to the
        victims' tensors, which are the caller's again once the stream has
        passed the call.  Returns the survivor batch's number.  Asynchronous;
        survivors that do not fit spoil the table (Context.check())."""
        vic = np.ascontiguousarray(victims, np.uint32).reshape(-1)
        nbytes = lambda x: x.numel() * x.element_size()
        if out_capacity is None:
            out_capacity = 0 if out is None else nbytes(out)
        if out_capacity and (out is None or nbytes(out) < out_capacity):
            raise RamcrcError("ReplayTable.clean: out is smaller than out_capacity")
        ecap = 0 if out_entries is None else out_entries.shape[0]
        if ecap and (out_work is None or out_work.numel() < ecap):
            raise RamcrcError("ReplayTable.clean: out_work is smaller than the record table")
        if moved is not None and nbytes(moved) < 8 * ecap:
            raise RamcrcError("ReplayTable.clean: moved is smaller than the record table")
        if usage is not None and nbytes(usage) < 32 * vic.size:
            raise RamcrcError("ReplayTable.clean: usage is smaller than the victims")
        for name, x, need in (("out_cert", out_cert, 8), ("out_status", out_status, 16),
                              ("out_n_entries", out_n_entries, 8), ("summary", summary, 112)):
            if x is not None and nbytes(x) < need:
                raise RamcrcError(f"ReplayTable.clean: {name} is too small")
        batch = _c.c_uint32(0)
        rc = lib().ramcrc_replay_table_clean_device(
            self._h, _c.c_void_p(vic.ctypes.data) if vic.size else None, vic.size,
            _ptr(out) if out_capacity else None, int(out_capacity), _ptr(out_cert), _ptr(out_status),
            _ptr(out_entries), ecap, _ptr(out_n_entries), _ptr(out_work), _ptr(moved), _ptr(usage),
            _ptr(summary), _c.byref(batch), _stream(stream))
        _check(rc, "ramcrc_replay_table_clean_device")
        for b in vic:
            self._keep[int(b)] = None
        self._keep.append((out, out_status, out_entries, out_n_entries, None, out_work))
        return batch.value

    @staticmethod
    def migrate_reserve(entries_caps, max_segments):
        """The (max_chunks, max_entries) arguments of Context.reserve after
        which migrate over listed batches of these record-table capacities into
        max_segments outputs does not allocate (include/ramcrc.h, rule 8)."""
        caps = [int(x) for x in entries_caps]
        tiles = sum((x + 255) // 256 for x in caps)
        return 2 * (len(caps) + 40 + 8 * int(max_segments) + 8 * tiles), 128 * tiles

    def migrate(self, batches, table_id, out, out_capacity, max_segments, out_certs, out_counts, summary,
                first_hash=0, last_hash=0xFFFFFFFFFFFFFFFF, live_only=False, start=(0, 0),
                out_stride=None, sent=None, sent_cap=None, seg_first=None, flags=None, stream=None):
        """Migrate a tablet out of the table on the device
        (ramcrc_replay_table_migrate_device): the objects and tombstones of
        table_id with a record hash in [first_hash, last_hash], from the listed
        batches in order from the cursor `start` = (list index, record), packed
        into at most max_segments transfer segments.  out: uint8 CUDA, 16-byte
        aligned, output k at k * out_stride (default out_capacity; both
        multiples of 16); out_certs: int32 CUDA [max_segments, 2]; out_counts:
        int32 CUDA [max_segments, 4] (segments.MIGRATE_COUNT_DTYPE); summary:
        int64 CUDA [15] (segments.MIGRATE_SUMMARY_DTYPE); sent: int32 CUDA
        [sent_cap, 2] out (segments.REPLAY_REF_DTYPE) or None; seg_first: int64
        CUDA [max_segments] out or None.  The table does not change.
        Asynchronous; chain calls with the summary's cursor."""
        lst = np.ascontiguousarray(batches, np.uint32).reshape(-1)
        nbytes = lambda x: x.numel() * x.element_size()
        nseg = int(max_segments)
        stride = int(out_capacity if out_stride is None else out_stride)
        if flags is None:
            flags = MIGRATE_LIVE_ONLY if live_only else 0
        if nseg and out_capacity and (out is None or nbytes(out) < (nseg - 1) * stride + int(out_capacity)):
            raise RamcrcError("ReplayTable.migrate: out is smaller than its geometry")
        if sent is not None and sent_cap is None:
            sent_cap = nbytes(sent) // 8
        if sent is not None and nbytes(sent) < 8 * int(sent_cap):
            raise RamcrcError("ReplayTable.migrate: sent is smaller than sent_cap")
        for name, x, need in (("out_certs", out_certs, 8 * nseg), ("out_counts", out_counts, 16 * nseg),
                              ("seg_first", seg_first, 8 * nseg), ("summary", summary, 120)):
            if x is not None and nbytes(x) < need:
                raise RamcrcError(f"ReplayTable.migrate: {name} is too small")
        rc = lib().ramcrc_replay_table_migrate_device(
            self._h, _c.c_void_p(lst.ctypes.data) if lst.size else None, lst.size, int(table_id),
            int(first_hash), int(last_hash), int(flags), int(start[0]), int(start[1]),
            _ptr(out) if nseg and out_capacity else None, int(out_capacity), stride, nseg, _ptr(out_certs),
            _ptr(out_counts), _ptr(sent), int(sent_cap or 0) if sent is not None else 0, _ptr(seg_first),
            _ptr(summary), _stream(stream))
        _check(rc, "ramcrc_replay_table_migrate_device")
        return summary

    def receive_migration(self, data, seg_stride, seg_capacity, nseg, certs, status, entries, n_entries, work,
                          stream=None):
        """The receiving side of a migration (receiveMigrationData): walk the
        nseg transfer segments in `data` under their certificates
        (Context.segment_walk) and add them to this table (add).  status,
        entries, n_entries: the walk's tables, out; work as add takes it.
        Returns the batch number.  Asynchronous; a segment whose certificate
        does not match takes no part, and shows in status."""
        self._ctx.segment_walk(data, seg_stride, seg_capacity, nseg, certs, status, entries, n_entries,
                               stream=stream)
        return self.add(data, seg_stride, nseg, status, entries, n_entries, work, stream=stream)


# ------------------------------------------------------------ multi-GPU shard
def shard_range(nseg, nranks, rank):
    """[lo, hi) of segment indices rank `rank` of `nranks` owns (ramcrc_shard_range)."""
    lo, hi = _c.c_uint64(0), _c.c_uint64(0)
    _check(lib().ramcrc_shard_range(nseg, nranks, rank, _c.byref(lo), _c.byref(hi)),
           "ramcrc_shard_range")
    return lo.value, hi.value


def shard_unique_id():
    """128-byte RCCL unique id for ramcrc_shard_create_rank (bytes)."""
    buf = (_c.c_uint8 * 128)()
    _check(lib().ramcrc_shard_unique_id(buf), "ramcrc_shard_unique_id")
    return bytes(buf)


class _StdoutToStderr:
    """RCCL prints a version banner on stdout at communicator creation; a
    benchmark's stdout carries exactly one JSON line, so point fd 1 at
    stderr for the duration."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        os.dup2(self.saved, 1)
        os.close(self.saved)


class Shard:
    """The recovery-scan shard of libramcrc (ramcrc_shard_*): scan of each
    rank's contiguous segment range + one RCCL all-gather of the CRCs.

    Shard(devices=[0, 1, ...])          one process, several GPUs (ncclCommInitAll)
    Shard(uid=..., nranks=N, rank=r, device=d)   one process per GPU (ncclCommInitRank)
    """

    def __init__(self, devices=None, uid=None, nranks=None, rank=None, device=None):
        h = _c.c_void_p()
        if devices is not None:
            arr = (_c.c_int * len(devices))(*devices)
            with _StdoutToStderr():
                rc = lib().ramcrc_shard_create_all(arr, len(devices), _c.byref(h))
            _check(rc, "ramcrc_shard_create_all")
        else:
            if uid is None or len(uid) != 128:
                raise RamcrcError("Shard needs devices=[...] or a 128-byte uid")
            buf = (_c.c_uint8 * 128).from_buffer_copy(uid)
            with _StdoutToStderr():
                rc = lib().ramcrc_shard_create_rank(buf, int(nranks), int(rank), int(device),
                                                    _c.byref(h))
            _check(rc, "ramcrc_shard_create_rank")
        self._h = h
        self.nlocal = int(lib().ramcrc_shard_local_count(h))

    def info(self, k=0):
        """(rank, device, stream handle, ctx handle) of local rank k."""
        r, d = _c.c_int(0), _c.c_int(0)
        st, cx = _c.c_void_p(), _c.c_void_p()
        _check(lib().ramcrc_shard_info(self._h, k, _c.byref(r), _c.byref(d), _c.byref(st),
                                       _c.byref(cx)), "ramcrc_shard_info")
        return r.value, d.value, st.value, cx.value

    def set_timing(self, enable=True, k=0):
        _check(lib().ramcrc_ctx_set_timing(_c.c_void_p(self.info(k)[3]), 1 if enable else 0),
               "ramcrc_ctx_set_timing")

    def scan_time(self, k=0):
        ms, n = _c.c_double(0), _c.c_uint64(0)
        _check(lib().ramcrc_ctx_scan_time(_c.c_void_p(self.info(k)[3]), _c.byref(ms), _c.byref(n)),
               "ramcrc_ctx_scan_time")
        return ms.value, n.value

    def segments(self, shards, seg_bytes, nseg, outs=None, finalize=True):
        """shards[k]: local rank k's segment range (CUDA uint8 tensor); outs[k]
        (int32 CUDA [nseg]) or None for the shard's own buffers."""
        if len(shards) != self.nlocal or (outs is not None and len(outs) != self.nlocal):
            raise RamcrcError("one shard (and output) per local rank")
        sp = (_c.c_void_p * self.nlocal)(*[t.data_ptr() if t is not None else 0 for t in shards])
        op = None if outs is None else (_c.c_void_p * self.nlocal)(*[t.data_ptr() for t in outs])
        _check(lib().ramcrc_shard_segments(self._h, sp, seg_bytes, nseg, op,
                                           FINALIZE if finalize else 0), "ramcrc_shard_segments")

    def sync(self):
        _check(lib().ramcrc_shard_sync(self._h), "ramcrc_shard_sync")

    def results(self, nseg, k=0):
        out = np.zeros(nseg, dtype=np.uint32)
        _check(lib().ramcrc_shard_results(self._h, k, _c.c_void_p(out.ctypes.data), nseg),
               "ramcrc_shard_results")
        return out

    def close(self):
        if self._h:
            lib().ramcrc_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
