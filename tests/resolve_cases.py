"""Records, cases and the independent expectation for the replay resolve tests
(ramcrc_replay_resolve_host / _device).

The expectation is a plain-Python sequential replay of
ObjectManager::replaySegment's object and tombstone branches
(src/ObjectManager.cc:632-867) with a dict for the master's hash table, over
the record table in table order: an object is discarded when its version is
<= the table's (:693), a tombstone only when it is < (:786).  Two tombstones
of one key and version -- the case the reference asserts away (:790-793) --
keep the earlier one, the library's own rule.  It yields key -> (version,
type, record).
"""
import struct

import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc

OBJ, OBJTOMB, SAFEVERSION = pc.OBJ, pc.OBJTOMB, pc.SAFEVERSION
NONE = segments.RESOLVE_NONE
FILL = 0xA5
KiB = 1024
M64 = (1 << 64) - 1
COUNT_NAMES = segments.RESOLVE_COUNTS_DTYPE.names


# -------------------------------------------------------------- the records
def obj(table_id, key, version, value=b"", **kw):
    """An object with a version (partition_cases.obj lays the header out)."""
    return pc.entry(OBJ, pc.obj(table_id, key, value, version=version, **kw))


def tomb(table_id, key, version):
    """ObjectTombstone::Header {tableId, segmentId, objectVersion, timestamp,
    checksum} and the key (src/Object.h:285-336)."""
    return pc.entry(OBJTOMB, struct.pack("<QQQII", table_id, 7, version, 0, 0) + key)


def record(etype, table_id, key, version, value=b""):
    return obj(table_id, key, version, value) if etype == OBJ else tomb(table_id, key, version)


# ---------------------------------------------------------- the expectation
def participants(src, stride, table, status):
    """Per record: ("rec", type, (table id, key), version), ("mal",), ("safe",
    version) or None, by the rules of include/ramcrc.h."""
    src = np.asarray(src, np.uint8)
    out = []
    for seg, off, ln, hdr in np.asarray(table).tolist():
        etype = hdr & 0x3F
        what = None
        if int(status[seg, 0]) & segments.SEG_OK and etype in (OBJ, OBJTOMB, SAFEVERSION):
            start = off + 1 + ((hdr >> 6) & 3) + 1
            readable = not (hdr & 0x100) and start + ln <= stride
            pay = src[seg * stride + start:seg * stride + start + ln].tobytes() if readable else b""
            if etype == SAFEVERSION:
                if readable and ln >= 12:
                    what = ("safe", int.from_bytes(pay[:8], "little"))
            elif etype == OBJ:
                what = ("mal",)
                if readable and ln >= 25:
                    tid = int.from_bytes(pay[16:24], "little")
                    ver = int.from_bytes(pay[8:16], "little")
                    nk = pay[24]
                    if nk == 0:
                        what = ("rec", OBJ, (tid, b""), ver)
                    elif ln >= 27:
                        kl = int.from_bytes(pay[25:27], "little")
                        ko = 25 + 2 * nk
                        if ko + kl <= ln:
                            what = ("rec", OBJ, (tid, pay[ko:ko + kl]), ver)
            else:
                what = ("mal",)
                if readable and ln >= 32:
                    what = ("rec", OBJTOMB, (int.from_bytes(pay[:8], "little"), pay[32:]),
                            int.from_bytes(pay[16:24], "little"))
        out.append(what)
    return out


def replay(parts, order=None):
    """The hash table after replaySegment took the participants in `order`
    (record indices; default: table order): key -> (version, type, record)."""
    table = {}
    for rec in range(len(parts)) if order is None else order:
        p = parts[rec]
        if p is None or p[0] != "rec":
            continue
        _, etype, key, ver = p
        cur = table.get(key)
        if etype == OBJ:
            if cur is not None and ver <= cur[0]:      # :693
                continue
        elif cur is not None:
            if ver < cur[0]:                           # :786
                continue
            if cur[1] == OBJTOMB and ver == cur[0]:    # :790-793 asserts it away; ours: the first stays
                continue
            # (an object at or below this version: the reference logs a
            # tombstone for it; at the same version that one stands in the
            # table, for the same key and version as this record, :831-834)
        table[key] = (ver, etype, rec)
    return table


def expected(src, stride, table, status, hashes=None):
    """(winner uint32 [n], live uint32 [m, 2], counts dict).  hashes: a
    caller's hash per record, which splits keys whose hashes differ."""
    parts = participants(src, stride, table, status)
    if hashes is not None:
        parts = [p if p is None or p[0] != "rec" else (p[0], p[1], p[2] + (int(hashes[i]),), p[3])
                 for i, p in enumerate(parts)]
    final = replay(parts)
    winner = np.full(len(parts), NONE, np.uint32)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    for i, p in enumerate(parts):
        if p is None:
            continue
        if p[0] == "mal":
            counts["malformed"] += 1
        elif p[0] == "safe":
            counts["safe_version"] = max(counts["safe_version"], p[1])
        else:
            counts["objects" if p[1] == OBJ else "tombstones"] += 1
            winner[i] = final[p[2]][2]
    live = np.flatnonzero(winner == np.arange(len(parts), dtype=np.uint32))
    for ver, etype, rec in final.values():
        counts["live_objects" if etype == OBJ else "live_tombstones"] += 1
    assert live.size == len(final)
    return winner, np.stack([live, np.zeros_like(live)], 1).astype(np.uint32).reshape(-1, 2), counts


def counts_dict(c):
    return {k: int(c[k]) for k in COUNT_NAMES}


# -------------------------------------------------------------------- cases
def reference_case(ref):
    """The fixture's cases as one segment, a key each; returns (entries, per
    case the index of its first record)."""
    es, first = [pc.entry(pc.SEGHEADER, pc.seg_header(1))], []
    for c in ref["cases"]:
        first.append(len(es))
        for t, key, ver in c["records"]:
            es.append(record(OBJ if t == "OBJ" else OBJTOMB, ref["table_id"], key.encode(), ver,
                             b"some guy"))
    return es, first


def mixed_lists(seed=5, nkeys=200, nseg=4):
    """nseg entry lists: about nkeys keys of 0 .. 40 bytes over three tables,
    1 .. 8 records each with versions 0 .. 3, spread over the segments in a
    seeded order; in between the records that take no part."""
    rng = np.random.default_rng(seed)
    rand = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
    keys = {(1, b"")}
    while len(keys) < nkeys:
        keys.add((int(rng.choice([1, 2, (1 << 32) + 1])), rand(rng.integers(0, 41))))
    recs = []
    for tid, key in sorted(keys):
        for _ in range(int(rng.integers(1, 9))):
            recs.append(record(OBJ if rng.random() < 0.6 else OBJTOMB, tid, key,
                               int(rng.integers(0, 4)), rand(rng.integers(0, 30))))
    tid, key = sorted(keys)[17]
    recs.append(pc.entry(OBJ, pc.obj(tid, key, b"v", num_keys=3, version=9)))   # its first key counts
    others = [pc.entry(SAFEVERSION, pc.safe_version(v)) for v in (0, 5, 1 << 40)]
    others += [pc.entry(pc.RPCRESULT, pc.rpc_result(1, 77)), pc.entry(pc.PREP, pc.prep(tid, key, b"p")),
               pc.entry(OBJ, pc.obj(1, b"short", key_len=6)), pc.entry(OBJTOMB, b"\0" * 16),
               pc.entry(SAFEVERSION, b"\xff" * 11), pc.entry(pc.LOGDIGEST, b"digest")]
    recs += others * 3
    order = rng.permutation(len(recs))
    lists = [[pc.entry(pc.SEGHEADER, pc.seg_header(10 + s))] for s in range(nseg)]
    for n, k in enumerate(order):
        lists[n % nseg].append(recs[k])
    # the segment whose certificate the tests damage would raise every answer
    lists[-1].append(pc.entry(SAFEVERSION, pc.safe_version(1 << 50)))
    lists[-1].append(obj(1, b"", 1 << 60))
    return lists


MIXED_BAD = 3   # the segment of mixed_lists that gets a bad certificate
MIXED_CAP = 64 * KiB


def key_residues(buf, stride, table, status):
    """The residues mod 16 at which the participants' keys start."""
    res = set()
    for (seg, off, ln, hdr), p in zip(np.asarray(table).tolist(),
                                      participants(buf, stride, table, status)):
        if p is not None and p[0] == "rec" and p[2][1]:
            start = seg * stride + off + 1 + ((hdr >> 6) & 3) + 1
            ko = 32 if p[1] == OBJTOMB else 25 + 2 * int(buf[start + 24])
            res.add((start + ko) % 16)
    return res


def collision_entries(seed=6):
    """300 records over 50 keys, among them pairs that differ only in the last
    byte, only in length (a prefix, and the empty key) and only in table id."""
    rng = np.random.default_rng(seed)
    keys = [(1, b""), (1, b"a"), (1, b"ab"), (1, b"ac"), (2, b"ab"), ((1 << 32) + 1, b"ab"),
            (1, b"0123456789abcdefX"), (1, b"0123456789abcdefY"), (1, b"0123456789abcdef"),
            (2, b"")]
    while len(keys) < 50:
        k = (1, rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes())
        if k not in keys:
            keys.append(k)
    es = [pc.entry(pc.SEGHEADER, pc.seg_header(1))]
    for n in range(300):
        tid, key = keys[n % 50] if n < 100 else keys[int(rng.integers(0, 50))]
        es.append(record(OBJ if rng.random() < 0.5 else OBJTOMB, tid, key, int(rng.integers(0, 5))))
    return es


def seed_collision_entries():
    """Table ids 1 and 2^32 + 1 with the same key bytes: Key::getHash is seeded
    with the low 32 bits, so the computed hashes are equal."""
    es = [pc.entry(pc.SEGHEADER, pc.seg_header(1))]
    for key in (b"", b"k", b"a key of some length"):
        assert pc.key_hash(1, key) == pc.key_hash((1 << 32) + 1, key)
        es += [obj(1, key, 3), obj((1 << 32) + 1, key, 2), tomb((1 << 32) + 1, key, 1), tomb(1, key, 3)]
    return es


WIDE = [0, (1 << 32) - 1, 1 << 32, 1 << 63, M64]


def wide_version_entries():
    """A key per ordered pair of WIDE: two objects, and a tombstone then an
    object."""
    es = [pc.entry(pc.SEGHEADER, pc.seg_header(1))]
    n = 0
    for a in WIDE:
        for b in WIDE:
            es += [obj(1, b"oo%d" % n, a), obj(1, b"oo%d" % n, b),
                   tomb(1, b"to%d" % n, a), obj(1, b"to%d" % n, b)]
            n += 1
    return es


def hot_key_entries(tombstones=True):
    """20,000 records of one key: objects of version 9, then (or not) ten
    tombstones of versions 9, 9, 8, 7, ..."""
    n_obj = 19990 if tombstones else 20000
    es = [obj(5, b"the hot key", 9)] * n_obj
    if tombstones:
        es += [tomb(5, b"the hot key", v) for v in (9, 9, 8, 7, 6, 5, 4, 3, 2, 1)]
    return es


def tiny_entries():
    return [obj(1, b"x", 1), tomb(1, b"x", 1), obj(1, b"y", 0)]


# ------------------------------------------------------------- host driver
def check_host(ramcrc, buf, cap, status, table, hashes=None, what=""):
    """The host form against the replay; returns (winner, live, counts)."""
    winner, live, need, counts = ramcrc.replay_resolve_host(buf, cap, status.shape[0], status, table,
                                                            key_hash=hashes)
    e_winner, e_live, e_counts = expected(buf, cap, table, status, hashes)
    assert np.array_equal(winner, e_winner), (what, "winners")
    assert need == e_live.shape[0] and np.array_equal(live, e_live), (what, "live list")
    assert counts_dict(counts) == e_counts, (what, counts_dict(counts), e_counts)
    return winner, live, counts_dict(counts)


# ------------------------------------------------ device calls (GPU tests)
class Resolved:
    """One ramcrc_replay_resolve_device call over an append_cases.Walked:
    every output pre-filled with 0xA5 bytes, read back after check()."""

    def __init__(self, ctx, w, hashes=None, live_cap=None, check=True, want_winner=True):
        import torch
        dev = w.d.device
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device=dev).view(dt)
        ecap = w.d_entries.shape[0]
        self.live_cap = ecap if live_cap is None else live_cap
        self.d_winner = fill((ecap + 4) * 4, torch.int32) if want_winner else None
        self.d_live = fill((self.live_cap + 4) * 8, torch.int32).view(-1, 2)
        self.d_n_live = fill(8, torch.int64)
        self.d_counts = fill(6 * 8, torch.int64)
        if isinstance(hashes, np.ndarray):
            h = np.zeros(ecap, np.uint64)
            h[:hashes.size] = hashes
            hashes = torch.from_numpy(h.view(np.int64)).to(dev)
        ctx.replay_resolve(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n,
                           self.d_live[:self.live_cap], self.d_n_live, self.d_counts,
                           key_hash=hashes, winner=self.d_winner)
        if check:
            ctx.check()
            self.read()

    def read(self):
        self.need = int(self.d_n_live.item())
        self.live_all = self.d_live.cpu().numpy().view(np.uint32)
        self.live = self.live_all[:min(self.need, self.live_cap)]
        self.winner_all = None if self.d_winner is None else self.d_winner.cpu().numpy().view(np.uint32)
        self.counts = counts_dict(self.d_counts.cpu().numpy().view(segments.RESOLVE_COUNTS_DTYPE)[0])


def check_device(ctx, ramcrc, w, hashes=None, live_cap=None, exp=None, what="", host=True):
    """One device call against the replay and the host form: winners, list and
    counters equal exactly; slots past the list's end and winner slots past
    the table keep their 0xA5 fill.  hashes: None, or a numpy uint64 array."""
    if exp is None:
        exp = expected(w.buf, w.cap, w.table, w.status, hashes)
    e_winner, e_live, e_counts = exp
    r = Resolved(ctx, w, hashes, live_cap)
    n = w.table.shape[0]
    cap = r.live_cap
    assert r.need == e_live.shape[0], (what, r.need, e_live.shape[0])
    assert np.array_equal(r.winner_all[:n], e_winner), (what, "winners")
    assert (r.winner_all[n:] == 0xA5A5A5A5).all(), (what, "a winner slot past the table was written")
    assert np.array_equal(r.live, e_live[:cap]), (what, "live list")
    assert (r.live_all[r.live.shape[0]:] == 0xA5A5A5A5).all(), (what, "a slot past the list was written")
    assert r.counts == e_counts, (what, r.counts, e_counts)
    if host:
        h_winner, h_live, h_need, h_counts = ramcrc.replay_resolve_host(
            w.buf, w.cap, w.nseg, w.status, w.table, key_hash=hashes, live_cap=cap)
        assert h_need == r.need and np.array_equal(h_live, r.live), (what, "host and device lists differ")
        assert np.array_equal(h_winner, r.winner_all[:n]) and counts_dict(h_counts) == r.counts, what
    return r


def host_source(oracle, entry_lists, cap, bad=()):
    """(buf, certs, status, table): one segment per entry list walked by the
    oracle; the segments in `bad` get a damaged certificate."""
    buf, certs = ac.source_of(oracle, entry_lists, cap)
    for s in bad:
        certs[s, 1] ^= 1
    status, table = ac.host_walk(oracle, buf, certs, len(entry_lists), cap)
    return buf, certs, status, table
