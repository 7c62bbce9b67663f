"""Recovery-segment verification on the GPU.

What a backup's RecoverySegmentBuilder::build and a recovery master's
ObjectManager::replaySegment do per replica, batched over many segments:

  1. Segment::checkMetadataIntegrity (src/Segment.cc:758-800) -- walk the
     length-prefixed entries, checksum their headers and lengths plus the
     certificate length, compare with the SegmentCertificate;
  2. for every object entry, Object::computeChecksum (src/Object.cc:805-819)
     compared with the checksum stored in its header
     (src/ObjectManager.cc:659-669).

Both run in libramcrc's kernels (ramcrc_segment_walk_device,
ramcrc_verify_objects_device); this module only allocates the tables and
builds synthetic segments shaped like nanobenchmarks/RecoverSegmentBenchmark.cc
(objects with 8-byte counter keys and splitmix64 value bytes) through the
host append path ramcrc_segment_fill_objects.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import ramcrc, workloads

SEG_OK = 1
SEG_PAST_CAPACITY = 2
SEG_PAST_LENGTH = 4
SEG_BAD_CHECKSUM = 8
SEG_TABLE_FULL = 16
SEG_CYCLE = 32
SEG_APPEND_FULL = 64    # ramcrc_append_status.flags: a placement did not fit
SEG_SOURCE_BAD = 128    # ramcrc_append_status.flags: the source segment failed its check
# ramcrc_placement, ramcrc_append_status, and the records and certificates they go with
PLACEMENT_DTYPE = np.dtype([("record", "<u4"), ("partition", "<u4")])
APPEND_STATUS_DTYPE = np.dtype([("flags", "<u4"), ("entries", "<u4")])
SEG_NO_HEADER = 512     # ramcrc_partition_status.flags: a placed record without a SEGHEADER
SEG_MALFORMED = 1024    # ramcrc_partition_status.flags: a record too short for its fields
# ramcrc_tablet and ramcrc_partition_status (ramcrc_recovery_partition_device / _host)
TABLET_DTYPE = np.dtype([("table_id", "<u8"), ("start_key_hash", "<u8"), ("end_key_hash", "<u8"),
                         ("ctime_segment_id", "<u8"), ("ctime_offset", "<u4"),
                         ("partition", "<u4")])
PARTITION_STATUS_DTYPE = np.dtype([("flags", "<u4"), ("placed", "<u4"), ("unplaced", "<u4"),
                                   ("dead", "<u4")])
# ramcrc_resolve_counts and the no-winner mark (ramcrc_replay_resolve_device / _host)
RESOLVE_COUNTS_DTYPE = np.dtype([("objects", "<u8"), ("tombstones", "<u8"), ("live_objects", "<u8"),
                                 ("live_tombstones", "<u8"), ("malformed", "<u8"),
                                 ("safe_version", "<u8")])
RESOLVE_NONE = 0xFFFFFFFF
# ramcrc_replay_ref and ramcrc_replay_table_stats (ramcrc_replay_table_*); "none" is
# {RESOLVE_NONE, RESOLVE_NONE}
REPLAY_REF_DTYPE = np.dtype([("batch", "<u4"), ("record", "<u4")])
REPLAY_TABLE_STATS_DTYPE = np.dtype([("keys", "<u8"), ("live_objects", "<u8"),
                                     ("live_tombstones", "<u8"), ("safe_version", "<u8"),
                                     ("batches", "<u8"), ("spoiled", "<u8")])
REPLAY_TABLE_MAX_BATCHES = 65536
# ramcrc_lookup_key, ramcrc_lookup_result, ramcrc_lookup_counts and the kinds
# (ramcrc_replay_table_lookup_device / _host)
LOOKUP_KEY_DTYPE = np.dtype([("table_id", "<u8"), ("key_off", "<u8"), ("key_len", "<u4"),
                             ("reserved", "<u4")])
LOOKUP_RESULT_DTYPE = np.dtype([("batch", "<u4"), ("record", "<u4"), ("version", "<u8"),
                                ("kind", "<u4"), ("segment", "<u4"), ("value_off", "<u4"),
                                ("value_len", "<u4")])
LOOKUP_COUNTS_DTYPE = np.dtype([("objects", "<u8"), ("tombstones", "<u8"), ("absent", "<u8"),
                                ("bad", "<u8"), ("spoiled", "<u8")])
LOOKUP_ABSENT, LOOKUP_OBJECT, LOOKUP_TOMBSTONE, LOOKUP_BAD_KEY = 0, 1, 2, 3
# ramcrc_reject_rules, ramcrc_read_summary, the flag, the not-returned mark and
# the statuses of a part (ramcrc_replay_table_read_device / _host; src/Status.h)
REJECT_RULES_DTYPE = np.dtype([("given_version", "<u8"), ("doesnt_exist", "u1"), ("exists", "u1"),
                               ("version_le_given", "u1"), ("version_ne_given", "u1"),
                               ("reserved", "<u4")])
READ_SUMMARY_DTYPE = np.dtype([("returned", "<u8"), ("reply_bytes", "<u8"), ("ok", "<u8"),
                               ("doesnt_exist", "<u8"), ("object_exists", "<u8"),
                               ("wrong_version", "<u8"), ("bad", "<u8"), ("value_bytes", "<u8"),
                               ("key_bytes", "<u8"), ("spoiled", "<u8")])
READ_PART_DTYPE = np.dtype([("status", "<u4"), ("version", "<u8"), ("length", "<u4")])   # packed
READ_VALUE_ONLY = 1
READ_NONE = 0xFFFFFFFFFFFFFFFF
STATUS_OK, STATUS_OBJECT_DOESNT_EXIST, STATUS_OBJECT_EXISTS = 0, 3, 4
STATUS_WRONG_VERSION, STATUS_REQUEST_FORMAT_ERROR = 5, 9
# ramcrc_hash_part, ramcrc_read_hashes_summary and the packed header of an
# object part (ramcrc_replay_table_read_hashes_device / _host); a hash that was
# not returned has off = READ_NONE
HASH_PART_DTYPE = np.dtype([("off", "<u8"), ("objects", "<u4"), ("reserved", "<u4")])
READ_HASHES_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "hashes", "objects", "objects_counted", "reply_bytes", "value_bytes", "key_bytes", "empty",
    "tombstones", "spoiled")])
READ_HASHES_OBJECT_DTYPE = np.dtype([("version", "<u8"), ("length", "<u4")])   # packed
# ramcrc_enum_frame (EnumerationIterator::Frame) and ramcrc_enumerate_summary
# (ramcrc_replay_table_enumerate_device / _host)
ENUM_FRAME_DTYPE = np.dtype([(n, "<u8") for n in (
    "tablet_start_hash", "tablet_end_hash", "num_buckets", "bucket_index", "bucket_next_hash")])
ENUMERATE_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "num_buckets", "next_bucket", "next_hash", "objects", "payload_bytes", "value_bytes", "key_bytes",
    "tombstones", "full", "stuck", "spoiled")])
ENUM_KEYS_ONLY = 1
ENUM_MAX_STALE = 8
# ramcrc_index_entry, ramcrc_index_build_summary, ramcrc_index_query,
# ramcrc_index_result and ramcrc_index_lookup_summary
# (ramcrc_replay_table_index_build_device / _host, ramcrc_index_lookup_device /
# _host); a query that was not answered has out_off = READ_NONE
INDEX_ENTRY_DTYPE = np.dtype([("prefix", "<u8"), ("pk_hash", "<u8"), ("key_off", "<u8"),
                              ("key_len", "<u4"), ("reserved", "<u4")])
INDEX_BUILD_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "n_entries", "key_bytes", "entries_needed", "key_bytes_needed", "objects_seen", "overflow",
    "spoiled")])
INDEX_QUERY_DTYPE = np.dtype([("first_off", "<u8"), ("last_off", "<u8"), ("first_allowed_hash", "<u8"),
                              ("first_len", "<u4"), ("last_len", "<u4"), ("max_hashes", "<u4"),
                              ("reserved", "<u4")])
INDEX_RESULT_DTYPE = np.dtype([("out_off", "<u8"), ("next_entry", "<u8"), ("next_key_hash", "<u8"),
                               ("next_key_off", "<u8"), ("num_hashes", "<u4"), ("next_key_len", "<u4"),
                               ("status", "<u4"), ("reserved", "<u4")])
INDEX_LOOKUP_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "served", "hashes", "bad", "maxed_out", "n_entries", "overflow_index")])
INDEX_OK, INDEX_BAD_QUERY, INDEX_NOT_SERVED = 0, 1, 2
# ramcrc_write_req, ramcrc_write_ref, ramcrc_write_summary, the packed
# MultiOp::Response::WritePart and ramcrc_seg_cert
# (ramcrc_replay_table_write_device / _host)
WRITE_REQ_DTYPE = np.dtype([("table_id", "<u8"), ("data_off", "<u8"), ("data_len", "<u4"),
                            ("reserved", "<u4")])
WRITE_PART_DTYPE = np.dtype([("status", "<u4"), ("version", "<u8")])   # packed
WRITE_REF_DTYPE = np.dtype([("object_off", "<u4"), ("tombstone_off", "<u4")])
WRITE_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "ok", "doesnt_exist", "object_exists", "wrong_version", "bad", "retry_duplicate", "retry_full",
    "tombstones", "allocated", "next_version", "out_bytes", "value_bytes", "key_bytes",
    "object_bytes", "tombstone_bytes", "spoiled")])
WRITE_REF_NONE = 0xFFFFFFFF
# the packed MultiOp::Response::RemovePart and ramcrc_remove_summary
# (ramcrc_replay_table_remove_device / _host); a request is a LOOKUP_KEY_DTYPE
# record and its reference one uint32, REMOVE_REF_NONE when nothing was written
REMOVE_PART_DTYPE = np.dtype([("status", "<u4"), ("version", "<u8")])   # packed
REMOVE_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "removed", "ok_absent", "doesnt_exist", "object_exists", "wrong_version", "bad",
    "retry_duplicate", "retry_full", "next_version", "out_bytes", "tombstone_bytes", "spoiled")])
REMOVE_REF_NONE = 0xFFFFFFFF
# ramcrc_increment_arg, the packed MultiOp::Response::IncrementPart and
# ramcrc_increment_summary (ramcrc_replay_table_increment_device / _host); a
# request is a LOOKUP_KEY_DTYPE record, its reference a WRITE_REF_DTYPE record.
# The double and the new value are kept as bits: a NaN's payload is data here.
INCREMENT_ARG_DTYPE = np.dtype([("add_int64", "<i8"), ("add_double_bits", "<u8")])
INCREMENT_PART_DTYPE = np.dtype([("status", "<u4"), ("version", "<u8"), ("value_bits", "<u8")])   # packed
INCREMENT_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "ok", "created", "doesnt_exist", "object_exists", "wrong_version", "invalid_object", "bad",
    "retry_duplicate", "retry_full", "tombstones", "allocated", "next_version", "out_bytes",
    "object_bytes", "tombstone_bytes", "value_bytes", "key_bytes", "spoiled")])
STATUS_INVALID_OBJECT = 22
# ramcrc_clean_usage and ramcrc_clean_summary (ramcrc_replay_table_clean_device / _host)
CLEAN_USAGE_DTYPE = np.dtype([(n, "<u8") for n in (
    "records", "live_objects", "live_tombstones", "live_bytes")])
CLEAN_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "victims", "records", "moved_objects", "moved_tombstones", "object_bytes", "tombstone_bytes",
    "dropped_objects", "dropped_tombstones", "dropped_other", "needed_bytes", "needed_records",
    "out_bytes", "batch", "spoiled")])
# ramcrc_migrate_count and ramcrc_migrate_summary (ramcrc_replay_table_migrate_device / _host)
MIGRATE_COUNT_DTYPE = np.dtype([(n, "<u4") for n in ("entries", "objects", "tombstones", "reserved")])
MIGRATE_SUMMARY_DTYPE = np.dtype([(n, "<u8") for n in (
    "next_index", "next_record", "done", "too_large", "segments_used", "sent_objects",
    "sent_tombstones", "sent_bytes", "payload_bytes", "records_read", "skipped_other",
    "skipped_table", "skipped_range", "skipped_dead", "spoiled")])
MIGRATE_LIVE_ONLY = 1
MIGRATE_MAX_CAPACITY = 1 << 28
MIGRATE_MAX_SEGMENTS = 65536
CERT_DTYPE =np.dtype([("head", "<u4"), ("checksum", "<u4")])
STATUS_RETRY = 17
# ramcrc_log_ref, ramcrc_sidelog_counts and the not-appended mark
# (ramcrc_replay_sidelog_device / _host)
LOG_REF_DTYPE = np.dtype([("segment", "<u4"), ("offset", "<u4")])
SIDELOG_COUNTS_DTYPE = np.dtype([("objects", "<u8"), ("tombstones", "<u8"), ("other", "<u8"),
                                 ("object_bytes", "<u8"), ("tombstone_bytes", "<u8"),
                                 ("short_tombstones", "<u8"), ("left_out", "<u8")])
LOG_REF_NONE = 0xFFFFFFFF
LOG_ENTRY_TYPE_SEGHEADER = 1    # src/LogEntryTypes.h:32
LOG_ENTRY_TYPE_RPCRESULT = 7    # src/LogEntryTypes.h:50
LOG_ENTRY_TYPE_OBJ = 2          # src/LogEntryTypes.h:35
LOG_ENTRY_TYPE_OBJTOMB = 3      # src/LogEntryTypes.h:38
LOG_ENTRY_TYPE_SAFEVERSION = 5  # src/LogEntryTypes.h:44
LOG_ENTRY_TYPE_PREP = 8         # src/LogEntryTypes.h:53
LOG_ENTRY_TYPE_PREPTOMB = 9     # src/LogEntryTypes.h:56
LOG_ENTRY_TYPE_TXDECISION = 10  # src/LogEntryTypes.h:59
LOG_ENTRY_TYPE_TXPLIST = 11     # src/LogEntryTypes.h:62
# Bytes a replayed record of each checked type must hold (ObjectManager::replaySegment,
# src/ObjectManager.cc:659-1100): Object::Header, ObjectTombstone::Header,
# ObjectSafeVersion::Header, PreparedOp::Header + Object::Header,
# PreparedOpTombstone::Header, TxDecisionRecord::Header, ParticipantList::Header.
REPLAY_HEADER_BYTES = {LOG_ENTRY_TYPE_OBJ: 24, LOG_ENTRY_TYPE_OBJTOMB: 32,
                       LOG_ENTRY_TYPE_SAFEVERSION: 12, LOG_ENTRY_TYPE_PREP: 56,
                       LOG_ENTRY_TYPE_PREPTOMB: 44, LOG_ENTRY_TYPE_TXDECISION: 48,
                       LOG_ENTRY_TYPE_TXPLIST: 24}

REPLAY_SEED = 0x5245504C   # "REPL": value bytes of segment i use seed REPLAY_SEED + i
OBJECT_OVERHEAD = 24 + 1 + 2 + 8   # Object::Header + KeyCount + CumulativeKeyLength + key
MIN_REPLAY_ENTRY = 1 + 1 + 12      # EntryHeader + 1 length byte + ObjectSafeVersion::Header


def lookup_queries(keys, align=1):
    """(key buffer uint8 [keys_bytes], queries LOOKUP_KEY_DTYPE [n]) for a list
    of (table_id, key bytes): the keys packed one behind the other, each at a
    multiple of `align`."""
    q = np.zeros(len(keys), LOOKUP_KEY_DTYPE)
    parts, at = [], 0
    for i, (table_id, key) in enumerate(keys):
        pad = -at % align
        q[i] = (int(table_id), at + pad, len(key), 0)
        parts.append(b"\0" * pad + bytes(key))
        at += pad + len(key)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), q


def keys_and_value(keys, value):
    """The keysAndValue image of an object (MultiOp::Request::WritePart's
    payload, Object's bytes behind its header): key count, cumulative key
    lengths, the keys, the value.  keys: a list of up to 255 byte strings."""
    cum, at = [], 0
    for k in keys:
        at += len(k)
        cum.append(at)
    return (bytes([len(keys)]) + np.asarray(cum, "<u2").tobytes() + b"".join(bytes(k) for k in keys)
            + bytes(value))


def write_requests(objects, align=1):
    """(data buffer uint8 [data_bytes], requests WRITE_REQ_DTYPE [n]) for a list
    of (table_id, keys, value): the keysAndValue images packed one behind the
    other, each at a multiple of `align`.  keys: a list of byte strings, or one
    byte string for a one-key object."""
    q = np.zeros(len(objects), WRITE_REQ_DTYPE)
    parts, at = [], 0
    for i, (table_id, keys, value) in enumerate(objects):
        if isinstance(keys, (bytes, bytearray)):
            keys = [keys]
        image = keys_and_value(keys, value)
        pad = -at % align
        q[i] = (int(table_id), at + pad, len(image), 0)
        parts.append(b"\0" * pad + image)
        at += pad + len(image)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), q


def double_bits(x):
    """The bits of a binary64: of a float, or an int that already is the bits."""
    if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
        return int(x) & 0xFFFFFFFFFFFFFFFF
    return int(np.array(x, "<f8").view("<u8"))


def increment_args(args):
    """INCREMENT_ARG_DTYPE [n] from one (add_int64, add_double) pair per
    request.  add_int64: any int, taken modulo 2^64; add_double: a float, or an
    int holding the bits of one (for a NaN with a payload, or -0.0)."""
    a = np.zeros(len(args), INCREMENT_ARG_DTYPE)
    for i, (add_int, add_double) in enumerate(args):
        v = int(add_int) & 0xFFFFFFFFFFFFFFFF
        a["add_int64"][i] = v - (1 << 64) if v >> 63 else v
        a["add_double_bits"][i] = double_bits(add_double)
    return a


def multi_increment_parts(parts, n=None):
    """A multi-increment's parts (bytes or a uint8 array of packed 20-byte
    records) as INCREMENT_PART_DTYPE [n]; its value_bits viewed as int64 or
    float64 is the part's newValue."""
    raw = np.ascontiguousarray(parts).view(np.uint8).reshape(-1).tobytes() \
        if not isinstance(parts, (bytes, bytearray)) else bytes(parts)
    n = len(raw) // 20 if n is None else int(n)
    if 20 * n > len(raw):
        raise ValueError("multi_increment_parts: fewer than n parts")
    return np.frombuffer(raw, INCREMENT_PART_DTYPE, n).copy()


def read_rules(rules):
    """REJECT_RULES_DTYPE [n] from one entry per query: None (no rule) or a
    dict with any of given_version, doesnt_exist, exists, version_le_given,
    version_ne_given (and reserved, which must stay 0 for a usable query)."""
    a = np.zeros(len(rules), REJECT_RULES_DTYPE)
    for i, r in enumerate(rules):
        for name, v in (r or {}).items():
            a[name][i] = int(v)
    return a


def multi_read_parts(reply, returned):
    """The first `returned` parts of a multi-read's reply (bytes or a uint8
    array) as (status, version, data bytes): a packed 16-byte READ_PART_DTYPE
    header each, followed by `length` data bytes when the status is OK."""
    raw = np.ascontiguousarray(reply, np.uint8).reshape(-1).tobytes() \
        if not isinstance(reply, (bytes, bytearray)) else bytes(reply)
    out, at = [], 0
    for _ in range(int(returned)):
        if at + 16 > len(raw):
            raise ValueError("multi_read_parts: the reply ends inside a header")
        status, version, length = (int(x) for x in np.frombuffer(raw, READ_PART_DTYPE, 1, at)[0])
        at += 16
        n = length if status == STATUS_OK else 0
        if at + n > len(raw):
            raise ValueError("multi_read_parts: the reply ends inside a part's data")
        out.append((status, version, raw[at:at + n]))
        at += n
    return out


def read_hashes_objects(reply, objects):
    """The first `objects` object parts of an indexed read's reply (bytes or a
    uint8 array) as (version, keys-and-value bytes): a packed 12-byte
    READ_HASHES_OBJECT_DTYPE header each, followed by `length` bytes."""
    raw = np.ascontiguousarray(reply, np.uint8).reshape(-1).tobytes() \
        if not isinstance(reply, (bytes, bytearray)) else bytes(reply)
    out, at = [], 0
    for _ in range(int(objects)):
        if at + 12 > len(raw):
            raise ValueError("read_hashes_objects: the reply ends inside a header")
        version, length = (int(x) for x in np.frombuffer(raw, READ_HASHES_OBJECT_DTYPE, 1, at)[0])
        at += 12
        if at + length > len(raw):
            raise ValueError("read_hashes_objects: the reply ends inside an object")
        out.append((version, raw[at:at + length]))
        at += length
    return out


def enumerate_objects(payload, payload_bytes):
    """The entries of an enumeration's payload (bytes or a uint8 array), of
    which payload_bytes are valid, as a list of bytes: a u32 little-endian
    length each, followed by that many bytes of the object's log entry."""
    raw = np.ascontiguousarray(payload, np.uint8).reshape(-1).tobytes() \
        if not isinstance(payload, (bytes, bytearray)) else bytes(payload)
    end = int(payload_bytes)
    if end > len(raw):
        raise ValueError("enumerate_objects: payload_bytes is past the payload")
    out, at = [], 0
    while at < end:
        if at + 4 > end:
            raise ValueError("enumerate_objects: the payload ends inside a length")
        length = int.from_bytes(raw[at:at + 4], "little")
        at += 4
        if at + length > end:
            raise ValueError("enumerate_objects: the payload ends inside an object")
        out.append(raw[at:at + length])
        at += length
    return out


def migrate_entries(segment, head):
    """The entries of a transfer segment (bytes or a uint8 array) whose
    certificate's length is `head`, as a list of (type, payload bytes):
    Segment's layout, a header byte (type | length bytes - 1 << 6), the
    little-endian length, the payload."""
    raw = np.ascontiguousarray(segment, np.uint8).reshape(-1).tobytes() \
        if not isinstance(segment, (bytes, bytearray)) else bytes(segment)
    end = int(head)
    if end > len(raw):
        raise ValueError("migrate_entries: head is past the segment")
    out, at = [], 0
    while at < end:
        lb = (raw[at] >> 6) + 1
        if at + 1 + lb > end:
            raise ValueError("migrate_entries: the segment ends inside an entry header")
        length = int.from_bytes(raw[at + 1:at + 1 + lb], "little")
        if at + 1 + lb + length > end:
            raise ValueError("migrate_entries: the segment ends inside a payload")
        out.append((raw[at] & 0x3F, raw[at + 1 + lb:at + 1 + lb + length]))
        at += 1 + lb + length
    return out


def enum_frames(frames):
    """ENUM_FRAME_DTYPE array from (tablet_start_hash, tablet_end_hash,
    num_buckets, bucket_index, bucket_next_hash) rows: the stale frames of an
    enumeration, at most ENUM_MAX_STALE of them, each num_buckets a power of
    two."""
    frames = list(frames)
    if len(frames) > ENUM_MAX_STALE:
        raise ValueError("enum_frames: more than ENUM_MAX_STALE frames")
    a = np.zeros(len(frames), ENUM_FRAME_DTYPE)
    for i, row in enumerate(frames):
        a[i] = tuple(int(v) for v in row)
        nb = int(a[i]["num_buckets"])
        if nb == 0 or nb & (nb - 1):
            raise ValueError("enum_frames: num_buckets must be a power of two")
    return a


def index_queries(ranges, align=1):
    """(key buffer uint8 [qkeys_bytes], queries INDEX_QUERY_DTYPE [n]) for a
    list of (first key, last key, first_allowed_hash, max_hashes): the keys
    packed one behind the other, each at a multiple of `align`.  An empty first
    key is below every entry, an empty last key above."""
    q = np.zeros(len(ranges), INDEX_QUERY_DTYPE)
    parts, at = [], 0
    for i, (first, last, first_allowed_hash, max_hashes) in enumerate(ranges):
        offs = []
        for key in (first, last):
            pad = -at % align
            offs.append(at + pad)
            parts.append(b"\0" * pad + bytes(key))
            at += pad + len(key)
        q[i] = (offs[0], offs[1], int(first_allowed_hash), len(first), len(last), int(max_hashes), 0)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), q


def index_lookup_hashes(out_hashes, results, index_keys=None):
    """A lookup's reply per query, from the packed hashes (uint64) and the
    INDEX_RESULT_DTYPE results: a list of (status, hashes uint64 [num_hashes],
    next key bytes or None: the range is exhausted, next_key_hash).  The next
    key is read from index_keys (the index's key copy) when that is given,
    else returned as (next_key_off, next_key_len).  A query that was not
    answered gives (status, an empty array, None, 0)."""
    out = np.ascontiguousarray(out_hashes).reshape(-1).view(np.uint64)
    results = np.ascontiguousarray(results).reshape(-1).view(INDEX_RESULT_DTYPE)
    keys = None if index_keys is None else np.ascontiguousarray(index_keys, np.uint8).reshape(-1)
    reply = []
    for r in results:
        status = int(r["status"])
        if status != INDEX_OK:
            reply.append((status, np.zeros(0, np.uint64), None, 0))
            continue
        at, n = int(r["out_off"]), int(r["num_hashes"])
        if at + n > out.size:
            raise ValueError("index_lookup_hashes: a result points past the hashes")
        nxt = None
        if int(r["next_key_len"]):
            o, ln = int(r["next_key_off"]), int(r["next_key_len"])
            nxt = (o, ln) if keys is None else keys[o:o + ln].tobytes()
        reply.append((status, out[at:at + n].copy(), nxt, int(r["next_key_hash"])))
    return reply


def tablets_array(rows):
    """TABLET_DTYPE array from (table_id, start_key_hash, end_key_hash,
    ctime_segment_id, ctime_offset, partition) rows."""
    a = np.zeros(len(rows), TABLET_DTYPE)
    for i, row in enumerate(rows):
        a[i] = tuple(int(v) for v in row)
    return a


def tablets_tensor(tablets, device="cuda"):
    """A tablet list (TABLET_DTYPE array, or rows for tablets_array) as the
    uint8 device tensor Context.recovery_partition takes."""
    import torch
    if not (isinstance(tablets, np.ndarray) and tablets.dtype == TABLET_DTYPE):
        tablets = tablets_array(tablets)
    raw = np.ascontiguousarray(tablets).view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, 40), dtype=torch.uint8, device=device)
    if raw.size:
        t[:raw.size] = torch.from_numpy(raw.copy()).to(device)
    return t[:raw.size] if raw.size else t[:0]


def entry_bytes(value_len):
    obj = OBJECT_OVERHEAD + value_len
    lb = 1 if obj < 1 << 8 else 2 if obj < 1 << 16 else 3 if obj < 1 << 24 else 4
    return 1 + lb + obj


def objects_per_segment(capacity, value_len):
    return capacity // entry_bytes(value_len)


def fill_segments_host(buf, nseg, capacity, value_len, first_key=0, stride=None, threads=8):
    """Turn nseg pre-filled segments of `buf` (numpy uint8; segment i at
    i*stride) into object segments.  Keys continue across segments as in
    RecoverSegmentBenchmark::run.  Returns certs uint32[nseg, 2] and the
    object counts."""
    stride = capacity if stride is None else stride
    per = objects_per_segment(capacity, value_len)
    certs = np.zeros((nseg, 2), np.uint32)
    counts = np.zeros(nseg, np.uint32)

    def one(i):
        seg = buf[i * stride: i * stride + capacity]
        n, length, ck = ramcrc.segment_fill_objects(seg, value_len, first_key + i * per)
        certs[i] = (length, ck)
        counts[i] = n

    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(one, range(nseg)))
    return certs, counts


def object_segments_host(nseg, capacity, value_len, seed=REPLAY_SEED, threads=8):
    """numpy buffer of nseg object segments (values = splitmix64 bytes of seed + i)."""
    buf = np.empty(nseg * capacity, np.uint8)

    def gen(i):
        buf[i * capacity:(i + 1) * capacity] = workloads.splitmix_bytes_np(seed + i, capacity)

    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(gen, range(nseg)))
    certs, counts = fill_segments_host(buf, nseg, capacity, value_len, threads=threads)
    return buf, certs, counts


class RecoveryVerify:
    """Device tables for walking and verifying batches of segments on one GPU.

    verify(d_segments, certs) returns the per-segment status tensor
    (int32 [nseg, 4]: flags, checksum, entries, bad_objects -- failed object,
    tombstone and safe-version checks) after both
    kernels ran on the current stream."""

    def __init__(self, ctx, nseg, capacity, stride=None, entries_cap=None, min_entry=None):
        self.ctx = ctx
        self.nseg = nseg
        self.capacity = capacity
        self.stride = capacity if stride is None else stride
        # Table sizing.  Every replayed record is at least a header byte, a
        # length byte and its type's header; the smallest is a safe version
        # (12 B, src/Object.h:402-427), so capacity // 14 + 1 records per
        # segment hold any segment -- but that worst case costs ~32 B of table
        # and scan scratch per 14 segment bytes (~15 GB for 512 x 8 MiB).
        #   entries_cap  fixed table; a walk that overflows it marks the
        #                segment TABLE_FULL (never OK) and check() raises;
        #   min_entry    fixed table sized for entries of at least that size;
        #   neither      a table for 128-byte entries on average that verify()
        #                grows (and walks again) when a walk finds more
        #                records -- at most once per batch shape.  verify() then
        #                waits for the walk's record count on every call, with
        #                or without check=True: no segment is left TABLE_FULL.
        self.grow = entries_cap is None and min_entry is None
        if entries_cap is None:
            per = self.GROW_START_ENTRY if self.grow else min_entry
            entries_cap = nseg * (capacity // per + 1)
        self._alloc(entries_cap)

    GROW_START_ENTRY = 128

    def _alloc(self, entries_cap):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        self.entries = torch.zeros((entries_cap, 4), dtype=torch.int32, device=dev)
        self.n_entries = torch.zeros(1, dtype=torch.int64, device=dev)
        self.obj_crc = torch.zeros(entries_cap, dtype=torch.int32, device=dev)
        self.status = torch.zeros((self.nseg, 4), dtype=torch.int32, device=dev)

    def walk(self, d_segments, d_certs, stream=None):
        self.ctx.segment_walk(d_segments, self.stride, self.capacity, self.nseg, d_certs,
                              self.status, self.entries, self.n_entries, stream=stream)
        return self.status

    def verify_objects(self, d_segments, stream=None):
        self.ctx.verify_objects(d_segments, self.stride, self.entries, self.n_entries,
                                self.obj_crc, self.status, stream=stream)
        return self.status

    def verify(self, d_segments, d_certs, stream=None, check=False):
        """Walk + per-record verify.  check=True waits for the stream and raises
        if the record table overflowed (some segment not verified) or a launch
        was refused.  A growing table (no entries_cap / min_entry given) always
        reads the walked record count back (a host sync), and when the walk
        found more records than the table holds it is enlarged and the batch
        walked again, so that verify(check=False) never returns segments left
        TABLE_FULL; fixed tables never sync unless check=True, and take the
        fused walk + verify call (ramcrc_replay_verify_device)."""
        if not self.grow:
            st = self.ctx.replay_verify(d_segments, self.stride, self.capacity, self.nseg, d_certs,
                                        self.status, self.entries, self.n_entries, self.obj_crc,
                                        stream=stream)
            if check:
                self.check(stream)
            return st
        self.walk(d_segments, d_certs, stream)
        self.ctx.check(stream)
        n = int(self.n_entries.item())
        if n > self.entries.shape[0]:
            self._alloc(n + n // 8 + self.nseg)
            self.walk(d_segments, d_certs, stream)
        st = self.verify_objects(d_segments, stream)
        if check:
            self.check(stream)
        return st

    def check(self, stream=None):
        self.ctx.check(stream)
        n = int(self.n_entries.item())
        if n > self.entries.shape[0]:
            raise ramcrc.RamcrcError(
                f"segment walk found {n} records but the table holds {self.entries.shape[0]}: "
                "segments marked TABLE_FULL were not verified")
