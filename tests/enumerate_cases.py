"""Cases and the expectation for one reply of a table enumeration against the
replay table (ramcrc_replay_table_enumerate_host / _device).

The expectation is plain Python: the lookup expectation of lookup_cases.py
(the sequential replay, held against the live query's winners) gives every
key's winner; a key's bucket is its record hash & (S - 1) -- the hash its adds
were given, Key::getHash otherwise --; a key is selected by its table id, the
hash range, the stale frames and, in the cursor's bucket, the cursor's hash
(Enumeration.cc's enumerateBucket, src/Enumeration.cc:58-108); the entries are
{u32 length, log entry} (appendObjectsToBuffer, :128-154) by ascending bucket
and {hash, batch, record}; whole buckets are kept while they end within
min(max_bytes, capacity), and the cursor's own bucket is cut before the first
entry of the first hash that does not fit (:302-332).  All of it is restated
here independently of the library.  The tests hold it against
tests/golden/enumerate_ref.json before any call is held against it.
"""
import ctypes
import struct

import numpy as np

from ramcloud_amd import segments

import clean_cases as cl
import lookup_cases as lc
import partition_cases as pc
import read_cases as rd
import read_hashes_cases as rh
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
FILL = lc.FILL
HUGE = 1 << 62
MAXH = (1 << 64) - 1
SUMMARY = segments.ENUMERATE_SUMMARY_DTYPE
SUMMARY_NAMES = SUMMARY.names
ZERO_SUMMARY = dict.fromkeys(SUMMARY_NAMES, 0)
SPOILED_SUMMARY = dict(ZERO_SUMMARY, spoiled=1)
PAD = 64
# The kernels' thresholds (read_hashes_cases.source_constants holds them
# against the sources): buckets per tile, the copy classes, and how many tiles
# one step of the one-workgroup scan takes.
TILE = rh.TILE
BIG_MIN = rh.BIG_MIN
GROUP_MIN = rh.GROUP_MIN
SCAN_PER = 2
T2 = (1 << 32) + 1


def source_constants():
    """kPartThreads, kAppBigMin, kAppGroupMin and kEnScanPer as the kernel
    sources state them."""
    import os
    import re
    out = rh.source_constants()
    csrc = os.path.join(os.path.dirname(os.path.abspath(segments.__file__)), "csrc")
    m = re.search(r"constexpr \w+ kEnScanPer = (\d+);", open(os.path.join(csrc, "dev_enumerate.inc")).read())
    assert m
    out["kEnScanPer"] = int(m.group(1))
    return out


def key_hash(key):
    return pc.key_hash(key[0], key[1])


def slots(key_cap):
    return cl.rc_slots(key_cap)


# ---------------------------------------------------------- the expectation
def hidden(frame, h):
    start, end, nb, idx, nxt = frame
    if not start <= h <= end:
        return False
    i = (h & 0xffffffffffff) & (nb - 1)
    return i < idx or (i == idx and h < nxt)


class Args:
    """One call's arguments."""

    def __init__(self, table_id, first=0, last=MAXH, bucket=0, next_hash=0, limit=0, stale=(), keys_only=False,
                 max_bytes=HUGE, capacity=None):
        self.table_id, self.first, self.last, self.bucket, self.next_hash = table_id, first, last, bucket, next_hash
        self.limit, self.stale, self.keys_only, self.max_bytes, self.capacity = limit, list(stale), keys_only, \
            max_bytes, capacity

    def but(self, **kw):
        a = Args(self.table_id)
        a.__dict__.update(self.__dict__)
        a.__dict__.update(kw)
        return a


class Want:
    """What a call must give.  exp, pays: read_cases.payloads' pair (or a clean
    model's results() and payloads()); hash_of: key -> its record hash; S: the
    table's slots."""

    def __init__(self, exp, pays, hash_of, S, a):
        end = a.limit or S
        buckets, tombs = {}, {}
        for key, res in exp.items():
            if key[0] != a.table_id:
                continue
            h = hash_of(key)
            b = h & (S - 1)
            if not a.bucket <= b < end or not a.first <= h <= a.last:
                continue
            if (b == a.bucket and h < a.next_hash) or any(hidden(f, h) for f in a.stale):
                continue
            if res[3] != lc.OBJECT:
                tombs[b] = tombs.get(b, 0) + 1
                continue
            pay = pays[key]
            vo, vl = lc.value_range(pay)
            length = vo if a.keys_only else len(pay)
            buckets.setdefault(b, []).append((h, res[0], res[1], struct.pack("<I", length) + pay[:length], vl,
                                              len(pay) - 24 - vl, key))
        for b in buckets:
            buckets[b].sort(key=lambda e: e[:3])   # {hash, batch, record}
        self.buckets = buckets
        self.total = sum(len(e[3]) for es in buckets.values() for e in es)
        self.capacity = min(a.max_bytes, self.total) if a.capacity is None else a.capacity
        lim = min(a.max_bytes, self.capacity)
        s = dict(ZERO_SUMMARY, num_buckets=S, next_bucket=end)
        sent = []
        self.starts, self.ends = [], []   # of every entry of the selection, were nothing cut
        at = 0
        for b in sorted(buckets):
            for e in buckets[b]:
                self.starts.append(at)
                at += len(e[3])
                self.ends.append(at)
        at = 0
        for b in sorted(set(buckets) | set(tombs)):
            es = buckets.get(b, [])
            size = sum(len(e[3]) for e in es)
            if at + size <= lim:
                sent += es
                at += size
                s["tombstones"] += tombs.get(b, 0)
                continue
            s["full"], s["next_bucket"] = 1, b
            if b == a.bucket:
                n, run = 0, 0
                while run + len(es[n][3]) <= lim:
                    run += len(es[n][3])
                    n += 1
                s["next_hash"] = es[n][0]
                while n and es[n - 1][0] == s["next_hash"]:
                    n -= 1
                sent += es[:n]
                s["stuck"] = int(n == 0)
            break
        self.payload = b"".join(e[3] for e in sent)
        self.keys = [e[6] for e in sent]
        self.entries = [e[3][4:] for e in sent]
        s["objects"], s["payload_bytes"] = len(sent), len(self.payload)
        s["value_bytes"], s["key_bytes"] = sum(e[4] for e in sent), sum(e[5] for e in sent)
        self.summary = s


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


# ------------------------------------------------------------------ drivers
class Got:
    """One call's outputs: payload (the bytes before payload_bytes), summary."""


def _finish(g):
    assert (g.payload_all[g.summary["payload_bytes"]:] == FILL).all(), "a byte at or past payload_bytes was written"
    assert (g.summary_past == FILL).all(), "a byte past the summary was written"
    g.payload = g.payload_all[:g.summary["payload_bytes"]].tobytes()
    return g


def host_raw(R, t, a, room, capacity, shift=0, stale_raw=None, flags=None):
    """ramcrc_replay_table_enumerate_host on buffers pre-filled with 0xA5; the
    summary and the frames lie at odd addresses (no alignment rule).  Returns
    (code, Got)."""
    g = Got()
    g.payload_all = np.full(room + PAD + shift, FILL, np.uint8)[shift:]
    sm = np.full(SUMMARY.itemsize + PAD + 1, FILL, np.uint8)[1:]
    frames = segments.enum_frames(a.stale) if stale_raw is None else stale_raw
    fr = np.zeros(frames.nbytes + 1, np.uint8)[1:]
    fr[:] = frames.view(np.uint8).reshape(-1)
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x.size else None
    code = R.lib().ramcrc_replay_table_enumerate_host(
        t._h, int(a.table_id), int(a.first), int(a.last), int(a.bucket), int(a.next_hash), int(a.limit), p(fr),
        frames.shape[0], (1 if a.keys_only else 0) if flags is None else flags,
        ctypes.c_void_p(g.payload_all.ctypes.data), int(capacity), int(a.max_bytes), p(sm))
    g.summary_raw = sm[:SUMMARY.itemsize].copy()
    g.summary = summary_dict(g.summary_raw.view(SUMMARY)[0])
    g.summary_past = sm[SUMMARY.itemsize:]
    return code, g


def host_call(R, t, a, room, capacity, shift=0):
    code, g = host_raw(R, t, a, room, capacity, shift)
    assert code == 0, code
    return _finish(g)


class Asked:
    """One ramcrc_replay_table_enumerate_device call: every output pre-filled
    with 0xA5 and longer than the call may write; the payload starts `shift`
    bytes into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, a, room, capacity, shift=0, check=True):
        import torch
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        assert capacity <= room + PAD
        self.d_payload = fill(room + PAD + shift)[shift:]
        self.d_sum = fill(SUMMARY.itemsize + PAD).view(torch.int64)
        t.enumerate(a.table_id, self.d_payload, self.d_sum, a.max_bytes, first_hash=a.first, last_hash=a.last,
                    bucket_index=a.bucket, bucket_next_hash=a.next_hash, bucket_limit=a.limit, stale=a.stale,
                    keys_only=a.keys_only, payload_capacity=capacity)
        if check:
            ctx.check()
            self.read()

    def read(self):
        sm = self.d_sum.cpu().numpy().view(np.uint8)
        self.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
        self.summary_past = sm[SUMMARY.itemsize:]
        self.payload_all = self.d_payload.cpu().numpy()
        return _finish(self)


def call(tab, a, room, capacity, shift=0):
    """The call on `tab` (a driver's table); on the device it is also held byte
    for byte against the host twin's."""
    R = tab.drv.ramcrc
    if not tab.drv.on_device:
        return host_call(R, tab.t, a, room, capacity, shift)
    g = Asked(tab.drv.ctx, tab.t, a, room, capacity, shift)
    h = host_call(R, tab.twin, a, room, capacity)
    assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
    assert h.payload == g.payload, ("host and device payloads differ", rd.first_difference(h.payload, g.payload))
    return g


class HostDriver(cl.HostDriver):
    pass


class DeviceDriver(cl.DeviceDriver):
    pass


def table(drv, key_cap, max_batches):
    tab = drv.table(key_cap, max_batches)
    tab.S = slots(key_cap)
    return tab


def ask(tab, ep, hash_of, a, what="", shift=0):
    """The call against the expectation.  Returns (the call's outputs, the Want)."""
    w = Want(ep[0], ep[1], hash_of, tab.S, a)
    room = min(w.capacity, w.total)
    g = call(tab, a, room, min(w.capacity, room + PAD), shift)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.payload == w.payload, (what, "payload bytes", rd.first_difference(g.payload, w.payload))
    assert segments.enumerate_objects(g.payload, g.summary["payload_bytes"]) == w.entries, what
    return g, w


def checked(tab):
    return rd.checked(tab)


def walk(tab, ep, hash_of, a, max_bytes, step, what=""):
    """The defining property: from cursor (0, 0) with a small max_bytes and
    `step` buckets a call until next_bucket == num_buckets; what is received is
    exactly the selection's object winners, each once and in the order of one
    unbounded call.  Returns the number of calls."""
    whole = Want(ep[0], ep[1], hash_of, tab.S, a.but(bucket=0, next_hash=0, limit=0, max_bytes=HUGE, capacity=None))
    got, keys, bucket, nxt, calls = [], [], 0, 0, 0
    while bucket < tab.S:
        limit = min(bucket + step, tab.S)
        mb = max_bytes
        while True:
            g, w = ask(tab, ep, hash_of, a.but(bucket=bucket, next_hash=nxt, limit=limit, max_bytes=mb), what=what)
            calls += 1
            if not g.summary["stuck"]:
                break
            assert g.summary["objects"] == 0 and g.summary["full"] == 1
            mb *= 2   # the caller's remedy: more room
        s = g.summary
        assert (s["next_bucket"], s["next_hash"]) > (bucket, nxt) or s["next_bucket"] == limit, (what, s)
        assert s["next_bucket"] <= limit and (s["next_hash"] == 0 or s["next_bucket"] == bucket)
        got += w.entries
        keys += w.keys
        bucket, nxt = s["next_bucket"], s["next_hash"]
        assert calls < 100000
    assert len(set(keys)) == len(keys), (what, "a key was sent twice")
    assert got == whole.entries and keys == whole.keys, (what, "the walk and the one call differ")
    want_keys = {k for k, r in ep[0].items() if k[0] == a.table_id and r[3] == lc.OBJECT and
                 a.first <= hash_of(k) <= a.last and not any(hidden(f, hash_of(k)) for f in a.stale)}
    assert set(keys) == want_keys, (what, "the walk's keys are not the table's object winners")
    return calls


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("enumerate_ref.json")


def golden_entries(sc):
    return [tc.head(1)] + [rc.obj(sc["table_id"], o["key"].encode(), 1 + n, o["value"].encode())
                           for n, o in enumerate(sc["objects"])]


def golden_args(sc):
    stale = [tuple(f[n] for n in segments.ENUM_FRAME_DTYPE.names) for f in sc["stale"]]
    return Args(sc["table_id"], stale=stale, keys_only=sc["keys_only"])


def check_expectation_against_golden(ref, drv):
    """The project's Key::getHash gives the constants the reference's test
    states, and the expectation alone -- no call -- gives what the reference's
    tests expect; returns how many scenarios."""
    for c in ref["key_hash_constants"]:
        assert pc.key_hash(c["table_id"], c["key"].encode()) == c["hash"], c
    assert ref["entry"] == {"length_bytes": 4, "object_header_bytes": 24}
    for sc in ref["scenarios"]:
        exp, pays = rd.payloads([drv.batch([golden_entries(sc)])])
        w = Want(exp, pays, key_hash, 64, golden_args(sc))
        assert [len(e) for e in w.entries] == sc["entry_lengths"], sc["name"]
        assert w.summary["payload_bytes"] == sc["payload_bytes"] and w.summary["full"] == 0
        assert sorted(k[1].decode() for k in w.keys) == sorted(sc["returned_keys"])
        again = Want(exp, pays, key_hash, 64, golden_args(sc).but(bucket=w.summary["next_bucket"],
                                                                  next_hash=w.summary["next_hash"]))
        assert again.summary["payload_bytes"] == sc["second_call_bytes"]
    return len(ref["scenarios"])


def case_goldens(drv):
    ref = golden()
    assert check_expectation_against_golden(ref, drv) == 3
    for sc in ref["scenarios"]:
        tab = table(drv, 32, 1)
        try:
            tab.add(drv.batch([golden_entries(sc)]))
            ep = checked(tab)
            a = golden_args(sc)
            g, w = ask(tab, ep, key_hash, a, what=sc["name"])
            assert g.summary["payload_bytes"] == sc["payload_bytes"] and g.summary["objects"] == len(sc["entry_lengths"])
            at = 0
            for n, length in enumerate(sc["entry_lengths"]):
                assert struct.unpack_from("<I", g.payload, at)[0] == length
                entry = g.payload[at + 4:at + 4 + length]
                key = w.keys[n][1].decode()
                o = next(o for o in sc["objects"] if o["key"] == key)
                assert struct.unpack_from("<Q", entry, 16)[0] == sc["table_id"]   # Object::Header: tableId at 16
                tail = key + ("" if sc["keys_only"] else o["value"])
                assert entry[24:] == b"\1" + struct.pack("<H", len(key)) + tail.encode(), sc["name"]
                at += 4 + length
            assert at == g.summary["payload_bytes"] and g.summary["next_bucket"] == g.summary["num_buckets"] == 64
            if sc["order_pinned"]:
                assert [k[1].decode() for k in w.keys] == sc["returned_keys"]
            g, w = ask(tab, ep, key_hash, a.but(bucket=g.summary["next_bucket"], next_hash=g.summary["next_hash"]),
                       what=(sc["name"], "second call"))
            assert g.summary["payload_bytes"] == sc["second_call_bytes"] and g.summary["full"] == 0
        finally:
            tab.close()


# ---------------------------------------------------------------- scenarios
def placed_table(drv, key_cap, groups, adds=1, extra=()):
    """A table whose keys are placed by caller hashes.  groups: (hash, table
    id, n, value length | None: a tombstone winner) -- n keys under one hash;
    the records go round-robin over `adds` batches.  Returns (tab, hash_of)."""
    lists = [[tc.head(1 + j)] for j in range(adds)]
    hs = [[0] for _ in range(adds)]
    hash_of = {}
    k = 0
    for gn, (h, tid, n, vl) in enumerate(groups):
        for i in range(n):
            key = (tid, b"placed %d of %x in group %d" % (i, h, gn))
            j = k % adds
            k += 1
            if vl is None:
                lists[j] += [rc.obj(tid, key[1], 1, b"dead"), rc.tomb(tid, key[1], 1)]
                hs[j] += [h, h]
            else:
                lists[j].append(rc.obj(tid, key[1], 2 + i, bytes([65 + i % 26]) * (vl + (i % 3 if vl else 0))))
                hs[j].append(h)
            hash_of[key] = h
    for key, h, es in extra:
        lists[0] += es
        hs[0] += [h] * len(es)
        hash_of[key] = h
    tab = table(drv, key_cap, adds)
    cap = max(64 * KiB, 2 * max(sum(len(e) for e in ls) for ls in lists))
    for ls, h in zip(lists, hs):
        tab.add(drv.batch([ls], cap=cap), np.array(h, np.uint64))
    return tab, hash_of.__getitem__


def every_cut(tab, ep, hash_of, a, what):
    """max_bytes at every entry's start, its end, and end +- 1, with the cursor
    in the first bucket that has an entry (the cut inside bucket_index) and
    before it (the cut at a later bucket)."""
    full = Want(ep[0], ep[1], hash_of, tab.S, a)
    assert full.summary["full"] == 0 and full.summary["objects"] == len(full.ends) > 0
    first = min(full.buckets)
    seen = set()
    for start, end in zip(full.starts, full.ends):
        for mb in (start, end - 1, end, end + 1):
            for bucket in {a.bucket, first}:
                g, w = ask(tab, ep, hash_of, a.but(bucket=bucket, max_bytes=mb), what=(what, mb, bucket))
                assert g.summary["payload_bytes"] <= mb
                seen.add((g.summary["full"], g.summary["stuck"], g.summary["next_hash"] != 0))
            g, w = ask(tab, ep, hash_of, a.but(capacity=mb), what=(what, "capacity", mb))
            assert g.summary["payload_bytes"] <= mb
    return seen


def case_buckets(drv, ns=(1, 2, 3, 40)):
    """1, 2, 3 and 40 keys in one bucket, in one add and over three; equal
    64-bit hashes of different keys next to other hashes of the same bucket; a
    neighbouring bucket whose keys lie on the same chain; tombstone winners;
    another table id on the chain.  Every cut, keys only, and the walk."""
    key_cap = 128
    S = slots(key_cap)
    assert S == TILE
    for n in ns:
        for adds in (1, 3):
            # bucket 7: n keys of hash 7, two of hash 7 + S, one of 7 + 5 * S; bucket 8 on the same chain;
            # a tombstone winner in 7, another table in 7 and 8
            groups = [(7, 1, n, 5), (8, 1, 2, 0), (7 + S, 1, 2, 9), (7, 2, 2, 3), (7 + 5 * S, 1, 1, 70),
                      (7, 1, 1, None), (8, 2, 1, 1), (200, 1, 1, 12)]
            tab, hash_of = placed_table(drv, key_cap, groups, adds)
            try:
                ep = checked(tab)
                what = ("buckets", n, adds)
                a = Args(1)
                g, w = ask(tab, ep, hash_of, a, what=what)
                assert g.summary["objects"] == n + 2 + 2 + 1 + 1 and g.summary["tombstones"] == 1
                hashes = [hash_of(k) for k in w.keys]
                assert hashes == sorted(hashes, key=lambda h: (h & (S - 1), h)) and hashes[-1] == 200
                g, w = ask(tab, ep, hash_of, Args(2), what=what)
                assert g.summary["objects"] == 3
                ask(tab, ep, hash_of, a.but(keys_only=True), what=what)
                seen = every_cut(tab, ep, hash_of, a, what)
                if n > 1:
                    assert {(1, 1, True), (1, 0, True), (1, 0, False), (0, 0, False)} <= seen, seen
                every_cut(tab, ep, hash_of, a.but(keys_only=True), what)
                # the cursor inside bucket 7: at, between and past its hashes
                for nh in (0, 7, 8, 7 + S, 7 + S + 1, 7 + 5 * S, 7 + 5 * S + 1, MAXH):
                    g, w = ask(tab, ep, hash_of, a.but(bucket=7, next_hash=nh), what=(what, "cursor", nh))
                    assert all(h >= nh or h & (S - 1) != 7 for h in (hash_of(k) for k in w.keys))
                for mb in (40, 100, 1000):
                    for step in (1, 3, S):
                        walk(tab, ep, hash_of, a, mb, step, what=(what, "walk", mb, step))
                walk(tab, ep, hash_of, a.but(keys_only=True), 64, 5, what=(what, "walk, keys only"))
            finally:
                tab.close()


def case_wrap_and_tile_edges(drv):
    """key_cap 32 (S = 64, less than a tile), 128 (exactly one), 129 (S = 512)
    and 3000 (S = 8192): a key with home S - 1 pushed round to slot 0 and on, a
    run of full buckets across every tile edge, the bucket limit at the
    edges."""
    for key_cap in (32, 128, 129, 3000):
        S = slots(key_cap)
        groups = [(S - 1, 1, 3, 4), (0, 1, 2, 6), (S - 2, 1, 1, 0), (1, 1, 1, 2)]
        for edge in range(TILE, S, TILE):
            groups += [(edge - 2, 1, 2, 3), (edge - 1, 1, 2, 1), (edge, 1, 1, 8), (edge + 1, 1, 2, 2)]
            if edge > 4 * TILE:
                break
        tab, hash_of = placed_table(drv, key_cap, groups, 2)
        try:
            ep = checked(tab)
            what = ("wrap", key_cap)
            a = Args(1)
            g, w = ask(tab, ep, hash_of, a, what=what)
            assert [hash_of(k) for k in w.keys[:2]] == [0, 0] and [hash_of(k) for k in w.keys[-3:]] == [S - 1] * 3
            g, w = ask(tab, ep, hash_of, a.but(bucket=S - 1), what=(what, "the last bucket"))
            assert g.summary["objects"] == 3
            g, w = ask(tab, ep, hash_of, a.but(bucket=S), what=(what, "past the last bucket"))
            assert g.summary == dict(ZERO_SUMMARY, num_buckets=S, next_bucket=S)
            limits = {1, 2, S - 1, S} | {e + d for e in range(TILE, S, TILE) for d in (-1, 0, 1) if e <= 5 * TILE}
            for limit in sorted(limits):
                g, w = ask(tab, ep, hash_of, a.but(limit=limit), what=(what, "limit", limit))
                assert g.summary["next_bucket"] == limit and g.summary["full"] == 0
                g, w = ask(tab, ep, hash_of, a.but(bucket=limit - 1, limit=limit), what=(what, "one bucket", limit))
            every_cut(tab, ep, hash_of, a, what)
            walk(tab, ep, hash_of, a, 60, TILE + 1, what=(what, "walk"))
            walk(tab, ep, hash_of, a, 50, S, what=(what, "walk, no limit"))
        finally:
            tab.close()


def case_every_limit(drv):
    """bucket_limit at every value, from every cursor bucket, for a small table."""
    tab, hash_of = placed_table(drv, 32, [(3, 1, 2, 4), (4, 1, 1, 0), (63, 1, 2, 1), (20, 1, 1, None), (21, 2, 1, 3)])
    try:
        ep = checked(tab)
        for bucket in (0, 3, 4, 5, 63):
            for limit in range(bucket, 65):
                if limit == 0:
                    continue
                g, w = ask(tab, ep, hash_of, Args(1, bucket=bucket, limit=limit), what=("limit", bucket, limit))
                assert g.summary["next_bucket"] == limit
    finally:
        tab.close()


def case_selection(drv):
    """Keys outside [first, last], first > last, table ids whose low 32 bits
    are equal (equal Key::getHash), and stale frames of other bucket counts."""
    es = rc.seed_collision_entries() + [rc.obj(1, b"both", 5, b"table one's"), rc.obj(T2, b"both", 6, b"the other's")]
    es += [rc.obj(1, b"range %d" % i, 1, b"r" * i) for i in range(40)]
    bs = [drv.batch(ls) for ls in tc.split_lists(es, at=9)]
    tab = table(drv, 128, 2)
    try:
        for b in bs:
            tab.add(b)
        ep = checked(tab)
        for tid in (1, T2, (2 << 32) + 1):
            g, w = ask(tab, ep, key_hash, Args(tid), what=("table", tid))
            assert all(k[0] == tid for k in w.keys)
        assert g.summary["objects"] == 0
        hs = sorted(key_hash(k) for k in ep[0] if k[0] == 1)
        for first, last in ((hs[5], hs[20]), (hs[5] + 1, hs[20] - 1), (hs[7], hs[7]), (hs[9], hs[8]), (0, hs[0]),
                            (hs[-1], MAXH), (MAXH, 0)):
            g, w = ask(tab, ep, key_hash, Args(1, first=first, last=last), what=("range", first, last))
            assert all(first <= key_hash(k) <= last for k in w.keys)
            if first > last:
                assert g.summary["objects"] == 0 and g.summary["tombstones"] == 0
        top = 1 << 63
        for stale in ([(0, MAXH, 1 << 16, 1 << 15, 0)], [(0, top - 1, 4, 4, 0)], [(top, MAXH, 2, 1, 1 << 63 | 1 << 40)],
                      [(0, top - 1, 1 << 20, 1 << 19, 0), (top, MAXH, 1, 0, hs[-10])],
                      [(0, MAXH, tab.S, 100, hs[3])] * 8, [(hs[4], hs[30], 8, 3, 0)]):
            a = Args(1, stale=stale)
            g, w = ask(tab, ep, key_hash, a, what=("stale", stale))
            assert 0 < g.summary["objects"] < 41 + 1
            walk(tab, ep, key_hash, a, 70, 9, what=("stale walk", stale))
        walk(tab, ep, key_hash, Args(1, first=hs[5], last=hs[30]), 80, 16, what="range walk")
    finally:
        tab.close()


def case_many_tiles(drv):
    """More tiles than one step of the one-workgroup scan takes: S = 2^18,
    1,024 tiles; entries in the first, the last and some tiles between, the
    cut in a tile of the second step."""
    key_cap = TILE * TILE * SCAN_PER + 1
    S = slots(key_cap)
    assert S // TILE > TILE * SCAN_PER
    step = TILE * TILE * SCAN_PER   # buckets a step of the scan
    homes = [0, 5, TILE, step - 1, step, step + 1, step + 7 * TILE + 3, S - TILE, S - 1]
    tab, hash_of = placed_table(drv, key_cap, [(h, 1, 2, 10) for h in homes])
    try:
        ep = checked(tab)
        a = Args(1)
        g, w = ask(tab, ep, hash_of, a, what="many tiles")
        assert g.summary["objects"] == 2 * len(homes)
        full = Want(ep[0], ep[1], hash_of, S, a)
        for n in (2, 6, 8, 10, 13, 16):
            g, w = ask(tab, ep, hash_of, a.but(max_bytes=full.ends[n] - 1), what=("many tiles, cut", n))
            assert g.summary["next_bucket"] == homes[n // 2] and g.summary["objects"] == n - n % 2
        g, w = ask(tab, ep, hash_of, a.but(bucket=step - 5, limit=step + 2 * TILE), what="many tiles, a window")
        assert g.summary["objects"] == 6
        walk(tab, ep, hash_of, a, 200, S // 3 + 1, what="many tiles, walk")
    finally:
        tab.close()


def case_size_classes(drv):
    """Objects of every copy class -- values of 0, 1 and 64 bytes, entries on
    either side of kAppBigMin and kAppGroupMin, one 100 KiB value -- in one
    bucket, in neighbouring buckets and with the payload at two bases; then
    sixteen small entries with the payload at every alignment 0 .. 15."""
    rng = np.random.default_rng(31)
    extra = []
    sizes = [0, 1, 64, BIG_MIN - 1, BIG_MIN, BIG_MIN + 1, GROUP_MIN - 1, GROUP_MIN, GROUP_MIN + 1, 100 * KiB]
    for n, size in enumerate(sizes):
        for h in (9, 300 + n):
            k = (1, b"class %d at %d" % (n, h))
            vl = size if n < 3 or n == 9 else size - 24 - 3 - len(k[1])   # the entry's length is `size`
            extra.append((k, h, [rc.obj(1, k[1], 1 + n, rng.integers(0, 256, vl, dtype=np.uint8).tobytes())]))
    steer = [((3, b"steer %02d" % n), 40 + n // 4, [rc.obj(3, b"steer %02d" % n, 1, bytes(range(n)))])
             for n in range(16)]
    tab, hash_of = placed_table(drv, 300, [], 1, extra + steer)
    try:
        ep = checked(tab)
        for keys_only in (False, True):
            for shift in (0, 5):
                g, w = ask(tab, ep, hash_of, Args(1, keys_only=keys_only), what=("classes", keys_only, shift),
                           shift=shift)
                assert g.summary["objects"] == 2 * len(sizes)
        g, w = ask(tab, ep, hash_of, Args(1), what="classes")
        lens = sorted(set(len(e) for e in w.entries))
        for edge in (BIG_MIN, GROUP_MIN):
            assert any(x < edge for x in lens) and any(x >= edge for x in lens)
        assert {BIG_MIN - 1, BIG_MIN, BIG_MIN + 1, GROUP_MIN - 1, GROUP_MIN, GROUP_MIN + 1} <= set(lens), lens
        for shift in range(16):   # every destination alignment
            g, w = ask(tab, ep, hash_of, Args(3), what=("residues", shift), shift=shift)
        full = Want(ep[0], ep[1], hash_of, tab.S, Args(3))
        assert len(full.starts) == 16 and full.starts[1] % 16 != 0   # (with the 16 shifts: every residue, every entry)
        walk(tab, ep, hash_of, Args(1), 3000, 50, what="classes walk")
    finally:
        tab.close()


def case_multi_key(drv):
    """Objects of 0, 1, 2 and 3 keys, and the object whose key table runs past
    its payload: with keys only its entry is its whole payload."""
    lists, want = lc.multi_key_lists()
    tab = table(drv, 64, 1)
    try:
        tab.add(drv.batch(lists))
        ep = checked(tab)
        for tid in (5, 6):
            for keys_only in (False, True):
                g, w = ask(tab, ep, key_hash, Args(tid, keys_only=keys_only), what=("multi-key", tid, keys_only))
                keys = [k for k in want if k[0] == tid]
                assert sorted(w.keys) == sorted(keys)
                assert g.summary["value_bytes"] == sum(len(want[k] or b"") for k in keys)
                for k, e in zip(w.keys, w.entries):
                    pay = ep[1][k]
                    assert e == (pay[:len(pay) - len(want[k] or b"")] if keys_only else pay)
        past = ep[1][(5, b"past")]
        g, w = ask(tab, ep, key_hash, Args(5, keys_only=True, first=key_hash((5, b"past")),
                                           last=key_hash((5, b"past"))), what="past")
        assert w.entries == [past] and g.summary["value_bytes"] == 0
    finally:
        tab.close()


def random_lists(rng, nbatches, nkeys):
    """Batches over one pool of keys of tables 1 and 2: objects of growing
    versions (overwrites), tombstones (removes), and keys that come once."""
    pool = [(1 + (i % 7 == 0), b"key %d" % i) for i in range(nkeys)]
    version = {}
    lists = []
    for j in range(nbatches):
        es = [tc.head(1 + j)]
        for i in rng.choice(nkeys, size=max(1, nkeys * 2 // 3), replace=False):
            tid, key = pool[int(i)]
            v = version.get((tid, key), 0) + 1
            version[(tid, key)] = v
            if rng.random() < 0.2 and j:
                es.append(rc.tomb(tid, key, v))
            else:
                es.append(rc.obj(tid, key, v, bytes(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8))))
        lists.append(es)
    return lists


def case_random_walks(drv, seed):
    """The defining property over a random table of several batches with
    overwrites and removes, before and after a clean: walked from (0, 0) with a
    small max_bytes and a small bucket_limit the entries received are exactly
    the table's object winners of table_id in [first, last], each once; the
    same with keys only; stats, a lookup of every key and live of every batch
    answer the same before and after."""
    rng = np.random.default_rng(seed)
    key_cap = [40, 129, 700][seed % 3]
    nkeys = key_cap * 3 // 4
    lists = random_lists(rng, 4, nkeys)
    tab, model = table(drv, key_cap, len(lists) + 3), cl.Model()
    try:
        for es in lists:
            cl.add(tab, model, drv.batch([es], cap=256 * KiB))
        for round_ in ("before the clean", "after the clean"):
            ep = (model.results(), model.payloads())
            keys = sorted(ep[0])
            snap = cl.snapshot(tab, model, keys)
            assert sum(r[3] == lc.TOMBSTONE for r in ep[0].values()) > 0
            hs = sorted(key_hash(k) for k in keys)
            for a in (Args(1), Args(2), Args(1, keys_only=True), Args(1, first=hs[len(hs) // 4], last=hs[-len(hs) // 4]),
                      Args(1, stale=[(0, MAXH, tab.S * 2, tab.S, 0)])):
                step = int(rng.integers(1, 20)) * max(1, tab.S // 256)
                calls = walk(tab, ep, key_hash, a, int(rng.integers(30, 200)), step, what=("random", seed, round_))
                assert calls >= tab.S // step
            g, w = ask(tab, ep, key_hash, Args(1), what=("random, one call", seed, round_))
            assert g.summary["tombstones"] == sum(r[3] == lc.TOMBSTONE and k[0] == 1 for k, r in ep[0].items())
            assert cl.snapshot(tab, model, keys) == snap, "the call changed what the table answers"
            if round_ == "before the clean":
                cl.clean(tab, model, drv, [0, 2], key_cap, what="enumerate", more=False, ties=True, scribble=False)
    finally:
        tab.close()


def case_read_only(drv, mixed):
    """The batches' arrays and d_work are byte-identical before and after
    calls, and so is everything the table's words answer."""
    tab = table(drv, 1000, 4)
    try:
        for m in mixed[:2]:
            tab.add(m)
        ep = checked(tab)
        before, arrays = tab.state(), rh.batch_arrays(tab)
        a, _ = ask(tab, ep, key_hash, Args(1), what="first")
        b, _ = ask(tab, ep, key_hash, Args(1), what="second")
        ask(tab, ep, key_hash, Args(1, max_bytes=300), what="cut")
        ask(tab, ep, key_hash, Args(1, bucket=5, limit=900, keys_only=True), what="keys only")
        assert rh.batch_arrays(tab) == arrays, "the call wrote to a batch's array or to d_work"
        assert a.payload == b.payload and a.summary["objects"] > 0 and tab.state() == before
        lc.lookup(tab, ep[0], sorted(ep[0]), what="lookups after the calls")
        tab.add(mixed[2])
        tab.add(mixed[3])
        ep4 = checked(tab)
        assert ep4[0] != ep[0]
        for tid in sorted({k[0] for k in ep4[0]}):
            ask(tab, ep4, key_hash, Args(tid), what=("after one more add", tid))
    finally:
        tab.close()
