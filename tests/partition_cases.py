"""Records, tablets and the independent expectation for the recovery partition
tests (ramcrc_recovery_partition_host / _device).

The expectation restates the placement decision of RecoverySegmentBuilder::build
(src/RecoverySegmentBuilder.cc:74-201) and the rules of include/ramcrc.h in
plain Python over the record table and the source bytes, with its own
MurmurHash3 x64-128 written from the public definition (Key::getHash,
src/Key.cc:140-151).  Where a fixture under tests/golden holds the answer,
the tests compare with the fixture; this restatement covers everything else.
"""
import json
import os
import struct

import numpy as np

from ramcloud_amd import segments

import append_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1
FILL = 0xA5

SEGHEADER = segments.LOG_ENTRY_TYPE_SEGHEADER
OBJ = segments.LOG_ENTRY_TYPE_OBJ
OBJTOMB = segments.LOG_ENTRY_TYPE_OBJTOMB
LOGDIGEST = 4
SAFEVERSION = segments.LOG_ENTRY_TYPE_SAFEVERSION
RPCRESULT = segments.LOG_ENTRY_TYPE_RPCRESULT
PREP = segments.LOG_ENTRY_TYPE_PREP
PREPTOMB = segments.LOG_ENTRY_TYPE_PREPTOMB
TXDECISION = segments.LOG_ENTRY_TYPE_TXDECISION
TXPLIST = segments.LOG_ENTRY_TYPE_TXPLIST
PLACED = {OBJ, OBJTOMB, SAFEVERSION, RPCRESULT, PREP, PREPTOMB, TXDECISION, TXPLIST}


def load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


# ------------------------------------------------------------------ the hash
def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    return k ^ (k >> 33)


def key_hash(table_id, key):
    """Key::getHash: MurmurHash3 x64-128 of the key, seed = low 32 bits of the
    table id, first output word."""
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    h1 = h2 = table_id & 0xFFFFFFFF
    n = len(key)
    for i in range(0, n - n % 16, 16):
        k1, k2 = struct.unpack_from("<QQ", key, i)
        h1 ^= (_rotl((k1 * c1) & M64, 31) * c2) & M64
        h1 = ((_rotl(h1, 27) + h2) * 5 + 0x52dce729) & M64
        h2 ^= (_rotl((k2 * c2) & M64, 33) * c1) & M64
        h2 = ((_rotl(h2, 31) + h1) * 5 + 0x38495ab5) & M64
    tail = key[n - n % 16:]
    k1 = int.from_bytes(tail[:8], "little")
    k2 = int.from_bytes(tail[8:], "little")
    if len(tail) > 8:
        h2 ^= (_rotl((k2 * c2) & M64, 33) * c1) & M64
    if tail:
        h1 ^= (_rotl((k1 * c1) & M64, 31) * c2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return (_fmix(h1) + _fmix(h2)) & M64


# -------------------------------------------------------------- the records
# Payloads as the reference serializes them; checksum fields are left zero
# (the partitioner does not read them).
def seg_header(segment_id, log_id=99, capacity=1 << 23, cut=24):
    """SegmentHeader {logId, segmentId, capacity, checksum} (src/LogMetadata.h:35-61)."""
    return struct.pack("<QQII", log_id, segment_id, capacity, 0)[:cut]


def safe_version(version):
    return struct.pack("<QI", version, 0)   # src/Object.h:402-427


def obj(table_id, key, value=b"", num_keys=1, key_len=None, version=0):
    """Object::Header {checksum, timestamp, version, tableId}, KeyCount, one
    CumulativeKeyLength per key, the keys, the value (src/Object.h:137-181)."""
    key_len = len(key) if key_len is None else key_len
    lens = b"".join(struct.pack("<H", key_len) for _ in range(num_keys))
    return struct.pack("<IIQQB", 0, 0, version, table_id, num_keys) + lens + key + value


def tomb(table_id, key):
    """ObjectTombstone::Header {tableId, segmentId, objectVersion, timestamp,
    checksum} and the key (src/Object.h:285-336)."""
    return struct.pack("<QQQII", table_id, 0, 0, 0, 0) + key


def rpc_result(table_id, key_hash_, lease=0, rpc=0, ack=0, response=b""):
    """RpcResult::Header (src/RpcResult.h:75-126): 44 bytes."""
    return struct.pack("<QQQQQI", table_id, key_hash_, lease, rpc, ack, 0) + response


def prep(table_id, key, value=b"", **kw):
    """PreparedOp::Header (32 bytes, src/PreparedOp.h:63-94) and the object."""
    return struct.pack("<BQQQ3xI", 1, 1, 10, 10, 0) + obj(table_id, key, value, **kw)


def prep_tomb(table_id, key_hash_, lease=1, rpc=10):
    """PreparedOpTombstone::Header (src/PreparedOp.h:142-182): 44 bytes."""
    return struct.pack("<QQQQQI", table_id, key_hash_, lease, rpc, 0, 0)


def tx_decision(table_id, key_hash_, lease=0):
    """TxDecisionRecord::Header (src/TxDecisionRecord.h:62-138): 48 bytes."""
    return struct.pack("<QQQQIIQI", table_id, key_hash_, lease, 1, 0, 0, 100, 0)[:48]


def tx_plist(parts, count=None, lease=42, tx=9):
    """ParticipantList::Header {leaseId, transactionId, count, checksum} and
    {tableId, keyHash, rpcId} per participant (src/ParticipantList.h:81-112)."""
    count = len(parts) if count is None else count
    return struct.pack("<QQII", lease, tx, count, 0) + b"".join(
        struct.pack("<QQQ", t, h, r) for t, h, r in parts)


def entry(etype, payload, length_bytes=None):
    return ac.raw_entry(etype, payload, length_bytes)


def head_entries(segment_id=0, version=1):
    """How a head segment opens: SEGHEADER, a log digest, safe version 1."""
    return [entry(SEGHEADER, seg_header(segment_id)), entry(LOGDIGEST, struct.pack("<IQ", 1, 0)),
            entry(SAFEVERSION, safe_version(version))]


def tablets(rows):
    return segments.tablets_array(rows)


# ---------------------------------- cases shared by the host and GPU tests
# Tablet lookup: records 3 .. 26 store these hashes under table ids 1 and 2^32 + 1.
STORED_HASHES = [0, 1, 99, 100, 150, 200, 201, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, M64 - 1, M64]
TAB_BASE = [(1, 100, 200, 0, 0, 0), (1, (1 << 63) - 1, (1 << 63) + 5, 0, 0, 1),
            (1, M64, M64, 0, 0, 2), (1, 0, 0, 0, 0, 3), ((1 << 32) + 1, 100, 200, 0, 0, 4)]
TAB_OVERLAP = [(1, 0, M64, 0, 0, 5), (1, 100, 200, 0, 0, 6)]
# record -> partition under TAB_BASE: inclusive bounds, unsigned compare, the full table id
TAB_BASE_PLACED = {3 + 0: 3, 3 + 3: 0, 3 + 4: 0, 3 + 5: 0, 3 + 7: 1, 3 + 8: 1, 3 + 9: 1, 3 + 11: 2,
                   15 + 3: 4, 15 + 4: 4, 15 + 5: 4}


def stored_entries():
    return head_entries() + [entry(RPCRESULT, rpc_result(t, v))
                             for t in (1, (1 << 32) + 1) for v in STORED_HASHES]


# Position: one entry list per segment (segment 1 gets a bad certificate) under
# the tablet (1, 0, M64, ctime (7, 0), partition 1), and the status of each.
def position_lists():
    t1 = entry(OBJTOMB, tomb(1, b"k"))
    return [
        head_entries(7) + [t1],                                                # 0 placed
        head_entries(7) + [t1],                                                # 1 bad certificate
        [t1] + head_entries(7) + [t1],                                         # 2 record before the header
        [entry(SEGHEADER, seg_header(7, cut=19)), t1],                         # 3 19-byte header
        head_entries(6) + [t1, entry(SEGHEADER, seg_header((1 << 32) + 7)), t1],   # 4 dead, second header, alive
        [entry(LOGDIGEST, b"digest")] + head_entries(7) + [t1],                # 5 a skipped type first
        head_entries(7) + [t1, entry(SEGHEADER, seg_header(9, cut=19)), t1,
                           entry(OBJ, b"short")],                              # 6 a later header is short
        [entry(SAFEVERSION, safe_version(1))],                                 # 7 safe version, no header
        [entry(OBJ, b"short"), entry(LOGDIGEST, b"")],                         # 8 malformed only
    ]


POSITION_STATUS = [[1, 3, 0, 0], [128, 0, 0, 0], [512, 0, 0, 0], [512, 0, 0, 0], [1, 3, 0, 1],
                   [1, 3, 0, 0], [512 | 1024, 0, 0, 0], [512, 0, 0, 0], [1 | 1024, 0, 0, 0]]

# Fan-out: participant lists as records 3 .. 8 (then, on the GPU, one whose
# array passes the record) and a safe version, under tablets owned by
# partitions `own` and 0.
PLISTS = [[], [(1, 5, 0)], [(3, 5, 0)], [(1, 15, 0), (3, 1, 1), (1, 5, 2), (2, 7, 3), (1, 25, 4)],
          [(1, 5, k) for k in range(70)], [(9, 9, k) for k in range(70)]]


def fan_out_case(n_part, extra=()):
    """(entries, tablets, the placements between the two safe versions')."""
    own = min(2, n_part - 1)
    tabs = [(1, 0, 10, 9, 9, own), (1, 11, 20, 9, 9, 0), (2, 0, M64, 9, 9, own)]
    es = head_entries() + [entry(TXPLIST, tx_plist(q)) for q in PLISTS] + list(extra)
    es.append(entry(SAFEVERSION, safe_version(3)))
    return es, tabs, [[4, own], [6, 0], [6, own], [6, own]] + [[7, own]] * 70


def mixed_lists(nseg, fill_bytes, seed, tables=(1, 2, 3)):
    """nseg entry lists of about fill_bytes each: a head, then objects,
    tombstones, prepared ops, records with stored hashes, safe versions,
    participant lists and skipped types over a few tables, keys of 0 .. 40
    bytes."""
    rng = np.random.default_rng(seed)
    rand = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
    lists = []
    for s in range(nseg):
        es = head_entries(segment_id=10 + s)
        size = sum(len(e) for e in es)
        while size < fill_bytes:
            t = int(rng.choice(tables))
            key = rand(rng.integers(0, 41))
            k = int(rng.integers(0, 10))
            if k < 4:
                e = entry(OBJ, obj(t, key, rand(rng.choice([0, 5, 100, 300, 2000]))))
            elif k == 4:
                e = entry(OBJTOMB, tomb(t, key))
            elif k == 5:
                e = entry(PREP, prep(t, key, rand(rng.integers(0, 50))))
            elif k == 6:
                e = entry(int(rng.choice([RPCRESULT, PREPTOMB, TXDECISION])),
                          rpc_result(t, int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))))
            elif k == 7:
                e = entry(SAFEVERSION, safe_version(int(rng.integers(0, 100))))
            elif k == 8:
                e = entry(TXPLIST, tx_plist([(int(rng.choice(tables)), int(rng.integers(0, 1 << 63)) * 2, q)
                                             for q in range(int(rng.integers(0, 5)))]))
            else:
                e = entry(int(rng.choice([LOGDIGEST, 6])), rand(rng.integers(0, 30)))
            es.append(e)
            size += len(e)
        lists.append(es)
    return lists


def split_tablets(tables, n_tablets_per_table, n_part, ctime=(0, 0)):
    """Each table's hash space in equal ranges, partitions round robin."""
    rows = []
    step = (1 << 64) // n_tablets_per_table
    for t in tables:
        for i in range(n_tablets_per_table):
            end = M64 if i == n_tablets_per_table - 1 else (i + 1) * step - 1
            rows.append((t, i * step, end, ctime[0], ctime[1], (i + t) % n_part))
    return tablets(rows)


# ---------------------------------------------------------- the expectation
def expected(src, stride, table, status, tabs, n_part):
    """(placements [(record, partition)], key hashes, part status [n_seg, 4])
    for a table whose segments are contiguous runs."""
    n_seg = status.shape[0]
    src = np.asarray(src, np.uint8)
    tabs = [tuple(int(v) for v in t) for t in np.asarray(tabs, segments.TABLET_DTYPE).tolist()]
    place, hashes = [], [0] * table.shape[0]
    pstat = np.zeros((n_seg, 4), np.uint32)
    for s in range(n_seg):
        pstat[s, 0] = segments.SEG_OK if int(status[s, 0]) & segments.SEG_OK else segments.SEG_SOURCE_BAD

    def which(table_id, h):
        for t in tabs:
            if t[0] == table_id and t[1] <= h <= t[2]:
                return t
        return None

    rows = table.tolist()
    i = 0
    while i < len(rows):
        s = rows[i][0]
        j = i
        while j < len(rows) and rows[j][0] == s:
            j += 1
        run, i = range(i, j), j
        if pstat[s, 0] != segments.SEG_OK:
            continue
        seg_place, counts, flags = [], [0, 0, 0], 0
        header = None   # segment id of the latest usable SEGHEADER, or False
        for rec in run:
            _, off, ln, hdr = rows[rec]
            etype = hdr & 0x3F
            start = s * stride + off + 1 + ((hdr >> 6) & 3) + 1
            readable = not (hdr & 0x100) and off + 1 + ((hdr >> 6) & 3) + 1 + ln <= stride
            pay = src[start:start + ln].tobytes() if readable else b""
            if etype == SEGHEADER:
                header = int.from_bytes(pay[8:16], "little") if readable and ln >= 20 else False
                continue
            if etype not in PLACED:
                continue
            fields = None
            if not readable:
                pass
            elif etype == SAFEVERSION:
                fields = ("safe",)
            elif etype == TXPLIST:
                if ln >= 24:
                    count = int.from_bytes(pay[16:20], "little")
                    if 24 + 24 * count <= ln:
                        fields = ("plist", [struct.unpack_from("<QQ", pay, 24 + 24 * k)
                                            for k in range(count)])
            elif etype in (OBJ, PREP):
                o = 32 if etype == PREP else 0
                if ln >= o + 25:
                    tid = int.from_bytes(pay[o + 16:o + 24], "little")
                    nk = pay[o + 24]
                    if nk == 0:
                        fields = ("hash", tid, key_hash(tid, b""))
                    elif ln >= o + 27:
                        kl = int.from_bytes(pay[o + 25:o + 27], "little")
                        ko = o + 25 + 2 * nk
                        if ko + kl <= ln:
                            fields = ("hash", tid, key_hash(tid, pay[ko:ko + kl]))
            elif etype == OBJTOMB:
                if ln >= 32:
                    tid = int.from_bytes(pay[:8], "little")
                    fields = ("hash", tid, key_hash(tid, pay[32:]))
            elif ln >= 16:
                fields = ("hash",) + struct.unpack_from("<QQ", pay, 0)
            if fields is None:
                flags |= segments.SEG_MALFORMED
                continue
            if header is None or header is False:
                flags |= segments.SEG_NO_HEADER
            if fields[0] == "safe":
                seg_place += [(rec, p) for p in range(n_part)]
            elif fields[0] == "plist":
                for tid, h in fields[1]:
                    t = which(tid, h)
                    if t is not None:
                        seg_place.append((rec, t[5]))
            else:
                _, tid, h = fields
                hashes[rec] = h
                t = which(tid, h)
                if t is None:
                    counts[1] += 1
                elif header is None or header is False:
                    pass
                elif (header, off) >= (t[3], t[4]):
                    seg_place.append((rec, t[5]))
                else:
                    counts[2] += 1
        if flags & segments.SEG_NO_HEADER:
            pstat[s] = (flags, 0, 0, 0)
        else:
            pstat[s] = (segments.SEG_OK | flags, len(seg_place), counts[1], counts[2])
            place += seg_place
    return (np.array(place, np.uint32).reshape(-1, 2), np.array(hashes, np.uint64), pstat)


def walk_records(out, head):
    """(type, offset, length) of the entries in out[:head]."""
    recs, pos = [], 0
    while pos < head:
        hdr = int(out[pos])
        lb = (hdr >> 6) + 1
        ln = int.from_bytes(bytes(out[pos + 1:pos + 1 + lb]), "little")
        recs.append([hdr & 0x3F, pos, ln])
        pos += 1 + lb + ln
    assert pos == head
    return recs


# ------------------------------------------------ device calls (GPU tests)
# torch is imported where it is used, so the host tests import this module
# without it.
class Partitioned:
    """One ramcrc_recovery_partition_device call over an append_cases.Walked:
    every output pre-filled with 0xA5 bytes, read back after check()."""

    def __init__(self, ctx, w, tabs, n_part, place_cap, check=True):
        import torch
        tabs = tabs if isinstance(tabs, np.ndarray) else tablets(tabs)
        self.tabs, self.n_part, self.place_cap = tabs, n_part, place_cap
        dev = w.d.device
        fill = lambda shape, dt: torch.full(shape, FILL, dtype=torch.uint8, device=dev).view(dt)
        self.d_tabs = segments.tablets_tensor(tabs, dev)
        self.d_place = fill((max(place_cap, 1) * 8,), torch.int32).view(-1, 2)[:place_cap]
        self.d_n_place = fill((8,), torch.int64)
        self.d_hash = fill((w.d_entries.shape[0] * 8,), torch.int64)
        self.d_pstat = fill((w.nseg * 16,), torch.int32).view(-1, 4)
        ctx.recovery_partition(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, self.d_tabs,
                               n_part, self.d_place, self.d_n_place, self.d_pstat,
                               key_hash=self.d_hash, n_tablets=tabs.shape[0])
        if check:
            ctx.check()
            self.read()

    def read(self):
        self.need = int(self.d_n_place.item())
        self.place_all = self.d_place.cpu().numpy().view(np.uint32)
        self.place = self.place_all[:min(self.need, self.place_cap)]
        self.hash_all = self.d_hash.cpu().numpy().view(np.uint64)
        self.pstat = self.d_pstat.cpu().numpy().view(np.uint32)


def check_device(ctx, ramcrc, w, tabs, n_part, place_cap=None, exp=None, what=""):
    """One device call against the restatement and the host form: the list,
    the counters and the hashes equal exactly; slots past the list's end and
    hash slots past the table keep their 0xA5 fill."""
    tabs = tabs if isinstance(tabs, np.ndarray) else tablets(tabs)
    if exp is None:
        exp = expected(w.buf, w.cap, w.table, w.status, tabs, n_part)
    e_place, e_hash, e_stat = exp
    cap = e_place.shape[0] if place_cap is None else place_cap
    p = Partitioned(ctx, w, tabs, n_part, cap)
    n = w.table.shape[0]
    assert p.need == e_place.shape[0], (what, p.need, e_place.shape[0])
    assert np.array_equal(p.place, e_place[:cap]), (what, "placements")
    assert (p.place_all[p.place.shape[0]:] == 0xA5A5A5A5).all(), (what, "a slot past the list was written")
    assert np.array_equal(p.hash_all[:n], e_hash), (what, "hashes")
    assert (p.hash_all[n:] == 0xA5A5A5A5A5A5A5A5).all(), (what, "a hash slot past the table was written")
    assert np.array_equal(p.pstat, e_stat), (what, p.pstat.tolist(), e_stat.tolist())
    h_place, h_need, h_hash, h_stat = ramcrc.recovery_partition_host(
        w.buf, w.cap, w.nseg, w.status, w.table, tabs, n_part, place_cap=cap)
    assert h_need == p.need and np.array_equal(h_place, p.place), (what, "host and device lists differ")
    assert np.array_equal(h_hash, p.hash_all[:n]) and np.array_equal(h_stat, p.pstat), what
    return p


# ------------------------------------------------------------- host driver
def host_source(oracle, entry_lists, cap):
    """(buf, certs, status, table) of one segment per entry list, walked by the oracle."""
    buf, certs = ac.source_of(oracle, entry_lists, cap)
    status, table = ac.host_walk(oracle, buf, certs, len(entry_lists), cap)
    return buf, certs, status, table


def check_host(ramcrc, buf, cap, status, table, tabs, n_part, what=""):
    """The host form against the restatement; returns its outputs."""
    tabs = tabs if isinstance(tabs, np.ndarray) else tablets(tabs)
    place, need, hashes, pstat = ramcrc.recovery_partition_host(buf, cap, status.shape[0], status,
                                                                table, tabs, n_part)
    e_place, e_hash, e_stat = expected(buf, cap, table, status, tabs, n_part)
    assert need == e_place.shape[0], (what, need, e_place.shape[0])
    assert np.array_equal(place, e_place), (what, "placements")
    assert np.array_equal(hashes, e_hash), (what, "hashes")
    assert np.array_equal(pstat, e_stat), (what, pstat.tolist(), e_stat.tolist())
    return place, hashes, pstat
