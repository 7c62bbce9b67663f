"""Keys, cases and the expectation for the replay table's lookup by key
(ramcrc_replay_table_lookup_host / _device).

The expectation is plain Python: resolve_cases.participants over the
concatenation of the added batches and its sequential replay
(resolve_cases.replay) give key -> (version, type, record); the record's
payload gives where the value lies (Object::getValueOffset / getValueLength,
src/Object.cc:647-676).  The tests hold it against the live query's winners for
every participant (the defining property of include/ramcrc.h), and the library
against it.
"""
import struct

import numpy as np

from ramcloud_amd import segments

import partition_cases as pc
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
FILL = rc.FILL
FILL32 = tc.FILL32
NONE = segments.RESOLVE_NONE
KEY = segments.LOOKUP_KEY_DTYPE
RES = segments.LOOKUP_RESULT_DTYPE
COUNT_NAMES = segments.LOOKUP_COUNTS_DTYPE.names
ABSENT, OBJECT, TOMBSTONE, BAD_KEY = (segments.LOOKUP_ABSENT, segments.LOOKUP_OBJECT,
                                      segments.LOOKUP_TOMBSTONE, segments.LOOKUP_BAD_KEY)
SPOILED_COUNTS = dict(objects=0, tombstones=0, absent=0, bad=0, spoiled=1)


def no_result(kind):
    return (NONE, NONE, 0, kind, NONE, 0, 0)


# ---------------------------------------------------------- the expectation
def value_range(pay):
    """(offset, length) of an object's value in its payload, or (len(pay), 0)
    when the key table or the keys run past the payload."""
    nk = pay[24]
    at = 25
    if nk:
        at += 2 * nk
        if at > len(pay):
            return len(pay), 0
        at += int.from_bytes(pay[at - 2:at], "little")
        if at > len(pay):
            return len(pay), 0
    return at, len(pay) - at


def expectation(batches):
    """key (table id, key bytes) -> a LOOKUP_RESULT_DTYPE tuple, for the table
    after `batches` were added in this order."""
    if not batches:
        return {}
    buf, cap, _, status, table, bounds = tc.concat(batches)
    final = rc.replay(rc.participants(buf, cap, table, status))
    out = {}
    for key, (ver, etype, rec) in final.items():
        b = int(np.searchsorted(bounds, rec, "right") - 1)
        r = rec - int(bounds[b])
        seg, off, ln, hdr = (int(x) for x in batches[b].table[r])
        if etype == rc.OBJ:
            start = off + 1 + ((hdr >> 6) & 3) + 1
            at = seg * cap + start
            vo, vl = value_range(batches[b].buf[at:at + ln].tobytes())
            out[key] = (b, r, ver, OBJECT, seg, start + vo, vl)
        else:
            out[key] = (b, r, ver, TOMBSTONE, NONE, 0, 0)
    return out


def participant_keys(batches):
    """Per batch, per record: its key or None."""
    return [[p[2] if p is not None and p[0] == "rec" else None
             for p in rc.participants(b.buf, b.cap, b.table, b.status)] for b in batches]


def check_winners(exp, batches, winners):
    """The defining property: for every participant, the expectation of its
    key names what the live query wrote to d_winner; returns how many."""
    n = 0
    for keys, w in zip(participant_keys(batches), winners):
        for i, key in enumerate(keys):
            if key is None:
                assert tuple(w[i].tolist()) == (NONE, NONE)
            else:
                assert exp[key][:2] == tuple(w[i].tolist()), (key, exp[key], w[i])
                n += 1
    return n


def all_keys(batches):
    """Every distinct key of the batches, in a fixed order."""
    return sorted({k for ks in participant_keys(batches) for k in ks if k is not None})


def expected_results(exp, keys, bad=()):
    """LOOKUP_RESULT_DTYPE [n] for the (table id, key) list; the indices in
    `bad` are unusable queries."""
    out = np.zeros(len(keys), RES)
    for i, key in enumerate(keys):
        out[i] = no_result(BAD_KEY) if i in bad else exp.get((int(key[0]), bytes(key[1])), no_result(ABSENT))
    return out


def expected_counts(results):
    k = results["kind"]
    return dict(objects=int((k == OBJECT).sum()), tombstones=int((k == TOMBSTONE).sum()),
                absent=int((k == ABSENT).sum()), bad=int((k == BAD_KEY).sum()), spoiled=0)


def counts_dict(c):
    return {k: int(c[k]) for k in COUNT_NAMES}


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def value_bytes(batches, res):
    """The bytes a result of kind OBJECT points at."""
    b = batches[int(res["batch"])]
    at = int(res["segment"]) * b.cap + int(res["value_off"])
    return b.buf[at:at + int(res["value_len"])].tobytes()


# -------------------------------------------------------------------- cases
def multi_obj(table_id, keys, value=b"", version=0, cum=None):
    """An object with len(keys) keys: Object::Header, KeyCount, the cumulative
    key lengths (`cum` overrides them), the keys, the value."""
    c, total = [], 0
    for k in keys:
        total += len(k)
        c.append(total)
    c = c if cum is None else cum
    return pc.entry(rc.OBJ, struct.pack("<IIQQB", 0, 0, version, table_id, len(keys)) +
                    b"".join(struct.pack("<H", x) for x in c) + b"".join(keys) + value)


IDENTITY_LENGTHS = list(range(0, 18)) + [31, 32, 33]


def identity_keys():
    """Keys that differ only in table id (one of them only in the high 32
    bits), a key and its proper prefixes, the empty key, the lengths around
    the 16-byte loads."""
    body = bytes(range(1, 34))
    keys = [(1, body[:n]) for n in IDENTITY_LENGTHS]
    keys += [(2, body[:5]), ((1 << 32) + 1, body[:5]), (2, b""), ((7 << 32) + 2, b"")]
    return keys


def identity_lists():
    """Two batches: every identity key once as an object (its value names it)
    and some again as a tombstone or a newer object in batch 1."""
    keys = identity_keys()
    a = [tc.head(1)] + [rc.obj(t, k, 3, b"value of %d/%d" % (t, len(k))) for t, k in keys]
    b = [tc.head(2)]
    for n, (t, k) in enumerate(keys):
        if n % 3 == 0:
            b.append(rc.tomb(t, k, 4))
        elif n % 3 == 1:
            b.append(rc.obj(t, k, 9, b"newer"))
    return [a], [b]


def absent_neighbours(keys):
    """Keys that are not in `keys` but nearly: another table id (low or high
    half), one byte longer or shorter, the last byte changed."""
    have = set(keys)
    out = []
    for t, k in keys:
        for c in ((t + 1, k), (t ^ (1 << 40), k), (t, k + b"\0"), (t, k[:-1]), (t, k[:-1] + b"\xfe")):
            if c not in have and c not in out:
                out.append(c)
    return out


MULTI_VALUES = [b"", b"v", bytes(range(256)) + b"x" * 44]


def multi_key_lists():
    """Objects with 1, 2 and 3 keys and values of 0, 1 and 300 bytes; an
    object without a key; a three-key object whose cumulative lengths run past
    the payload.  Returns (lists, key -> value or None: no value)."""
    es, want = [tc.head(1)], {}
    for nk in (1, 2, 3):
        for v in MULTI_VALUES:
            first = b"mk %d %d" % (nk, len(v))
            es.append(multi_obj(5, [first, b"second key", b"3rd"][:nk], v, 2))
            want[(5, first)] = v
    es.append(multi_obj(6, [], b"the value of no key", 1))
    want[(6, b"")] = b"the value of no key"
    es.append(multi_obj(5, [b"past", b"x", b"y"], b"zz", 1, cum=[4, 5, 5000]))
    want[(5, b"past")] = None
    return [es], want


def same_slot_absent(keys, nslots, tries=200000):
    """An absent key whose Key::getHash lands on the home slot of one of
    `keys` (found by search)."""
    mask = nslots - 1
    homes = {pc.key_hash(t, k) & mask for t, k in keys}
    have = set(keys)
    for n in range(tries):
        c = (1, b"absent %d" % n)
        if c not in have and pc.key_hash(*c) & mask in homes:
            return c
    raise AssertionError("no absent key found on a claimed slot")


# ------------------------------------------------------------------ drivers
# The scenarios below run unchanged on the host and on the device: a driver
# makes batches and tables, a table adds, answers the live query and looks up.
class HostTab:
    def __init__(self, drv, key_cap, max_batches):
        self.drv, self.batches = drv, []
        self.t = drv.ramcrc.ReplayTableHost(key_cap, max_batches)

    def add(self, b, hashes=None):
        self.batches.append(b)
        return tc.host_add(self.t, b, hashes)

    def reset(self):
        self.t.reset()
        self.batches = []

    def close(self):
        self.t.close()

    def winners(self):
        return [self.t.live(j)[0] for j in range(len(self.batches))]

    def state(self):
        """Everything the table answers without a key, as bytes."""
        out = [np.array([self.t.stats()]).tobytes()]
        for j in range(len(self.batches)):
            winner, live, need, counts = self.t.live(j)
            out += [winner.tobytes(), live.tobytes(), np.array([counts]).tobytes(), str(need).encode()]
        return out

    def lookup_raw(self, kb, q, hashes=None, want_counts=True):
        res, counts = self.t.lookup(kb, q, key_hash=hashes)
        return res, counts_dict(counts)


class HostDriver:
    def __init__(self, ramcrc, oracle):
        self.ramcrc, self.oracle = ramcrc, oracle

    def batch(self, lists, cap=64 * KiB, bad=()):
        return tc.HostBatch(self.oracle, lists, cap, bad)

    def table(self, key_cap, max_batches):
        return HostTab(self, key_cap, max_batches)


class Looked:
    """One ramcrc_replay_table_lookup_device call: the key buffer uploaded at
    exactly its length, results and counts pre-filled with 0xA5 (four result
    slots and two words more than the call may write), read back after
    check()."""

    def __init__(self, ctx, t, kb, q, hashes=None, want_counts=True, check=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.n = n = q.shape[0]
        self.d_keys = torch.from_numpy(np.ascontiguousarray(kb)).cuda() if kb.size else None
        raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1)
        self.d_q = torch.from_numpy(raw.copy()).cuda().view(torch.int64) if n else None
        self.d_res = fill((n + 4) * 32, torch.int32)
        self.d_counts = fill(7 * 8, torch.int64) if want_counts else None
        if isinstance(hashes, np.ndarray):
            hashes = torch.from_numpy(hashes.astype(np.uint64).view(np.int64)).cuda()
        t.lookup(self.d_keys, self.d_q, self.d_res, counts=self.d_counts, key_hash=hashes,
                 keys_bytes=kb.size, n_queries=n)
        if check:
            ctx.check()
            self.read()

    def read(self):
        raw = self.d_res.cpu().numpy().view(np.uint8)
        self.results = raw[:self.n * 32].view(RES)
        self.past = raw[self.n * 32:].view(np.uint32)
        self.counts = self.count_past = None
        if self.d_counts is not None:
            c = self.d_counts.cpu().numpy()
            self.counts = counts_dict(c[:5].view(segments.LOOKUP_COUNTS_DTYPE)[0])
            self.count_past = c[5:].view(np.uint32)


class DeviceTab:
    """A table on the device with its twin on the host: every lookup is held
    against the twin's, and nothing past an output may be written."""

    def __init__(self, drv, key_cap, max_batches):
        self.drv, self.batches, self.added = drv, [], []
        self.t = drv.ramcrc.ReplayTable(drv.ctx, key_cap, max_batches)
        self.twin = drv.ramcrc.ReplayTableHost(key_cap, max_batches)

    def add(self, w, hashes=None):
        a = tc.Added(w, hashes)
        self.batches.append(w)
        self.added.append(a)
        n = a.add(self.t)
        assert n == self.twin.add(w.buf, w.cap, w.nseg, w.status, w.table, key_hash=hashes)
        return n

    def reset(self):
        self.t.reset()
        self.twin.reset()
        self.batches, self.added = [], []

    def close(self):
        self.t.close()
        self.twin.close()

    def _lives(self):
        return [tc.Live(self.drv.ctx, self.t, a) for a in self.added]

    def winners(self):
        return [r.winner_all[:w.table.shape[0]].reshape(-1).view(tc.REF)
                for r, w in zip(self._lives(), self.batches)]

    def state(self):
        out = [str(sorted(tc.device_stats(self.drv.ctx, self.t).items())).encode()]
        for r in self._lives():
            out += [r.winner_all.tobytes(), r.live_all.tobytes(), str(sorted(r.counts.items())).encode(),
                    str(r.need).encode()]
        return out

    def lookup_raw(self, kb, q, hashes=None, want_counts=True):
        r = Looked(self.drv.ctx, self.t, kb, q, hashes, want_counts)
        assert (r.past == FILL32).all(), "a result past the queries was written"
        assert not want_counts or (r.count_past == FILL32).all(), "a word past the counts was written"
        h_res, h_counts = self.twin.lookup(kb, q, key_hash=hashes)
        assert same(h_res, r.results), "host and device results differ"
        assert not want_counts or counts_dict(h_counts) == r.counts, "host and device counts differ"
        return r.results, r.counts


class DeviceDriver:
    def __init__(self, ramcrc, oracle, ctx):
        self.ramcrc, self.oracle, self.ctx = ramcrc, oracle, ctx

    def batch(self, lists, cap=64 * KiB, bad=()):
        import append_cases as ac
        buf, certs = ac.source_of(self.oracle, lists, cap)
        for s in bad:
            certs[s, 1] ^= 1
        return ac.Walked(self.ctx, buf, certs, cap, len(lists))

    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


def lookup(tab, exp, keys, hashes=None, what="", align=1, shift=0, want_counts=True):
    """The lookup of `keys` against the expectation; the key buffer has `shift`
    bytes in front of the first key.  Returns the results."""
    kb, q = segments.lookup_queries(keys, align)
    if shift:
        kb = np.concatenate([np.full(shift, 0xEE, np.uint8), kb])
        q["key_off"] += shift
    res, counts = tab.lookup_raw(kb, q, hashes, want_counts)
    want = expected_results(exp, keys)
    assert same(res, want), (what, [(k, r, w) for k, r, w in zip(keys, res, want) if r != w][:3])
    assert not want_counts or counts == expected_counts(want), (what, counts)
    return res


def checked_expectation(tab):
    """The expectation for the table as it stands, held against the live
    query's winners for every participant."""
    exp = expectation(tab.batches)
    n = check_winners(exp, tab.batches, tab.winners())
    assert n > 0 or not exp
    return exp


# ---------------------------------------------------------------- scenarios
def case_empty_and_fresh(drv):
    tab = drv.table(64, 2)
    keys = [(1, b""), (1, b"x"), (2, b"a longer key than sixteen bytes")]
    try:
        res = lookup(tab, {}, keys, what="empty")
        assert (res["kind"] == ABSENT).all()
        tab.add(drv.batch([[tc.head(1)] + rc.tiny_entries()]))
        exp = checked_expectation(tab)
        assert lookup(tab, exp, [(1, b"x"), (1, b"y")])["kind"].tolist() == [TOMBSTONE, OBJECT]
        tab.reset()
        assert (lookup(tab, {}, keys + [(1, b"y")], what="after the reset")["kind"] == ABSENT).all()
    finally:
        tab.close()


def case_relations(drv):
    """Every version relation and type pair across two and three batches,
    looked up after every add; the stale pick and its mirrors."""
    bs = [drv.batch([es]) for es in tc.relation_lists()]
    keys = all_keys(bs) + [(4, b"stale pick, never"), (99, b"pair 0")]
    stale = []
    tab = drv.table(2000, 3)
    try:
        for k, b in enumerate(bs):
            tab.add(b)
            exp = checked_expectation(tab)
            res = lookup(tab, exp, keys, what=("after add", k))
            stale.append({key: tuple(res[keys.index(key)].tolist())
                          for key in ((4, b"stale pick"), (4, b"stale pick, mirrored"),
                                      (4, b"stale pick, late"), (4, b"kept pick"))})
    finally:
        tab.close()
    a, b, c = stale
    k = (4, b"stale pick")
    assert (a[k][3], a[k][2], a[k][0]) == (TOMBSTONE, 5, 0) and (b[k][3], b[k][2], b[k][0]) == (OBJECT, 7, 1)
    k = (4, b"stale pick, mirrored")
    assert (a[k][3], a[k][2], a[k][0]) == (OBJECT, 5, 0) and (b[k][3], b[k][2], b[k][0]) == (TOMBSTONE, 7, 1)
    k = (4, b"stale pick, late")
    assert b[k] == a[k] and (c[k][3], c[k][2], c[k][0]) == (TOMBSTONE, 7, 2)
    k = (4, b"kept pick")
    assert a[k] == b[k] == c[k] and a[k][3] == OBJECT


def case_identity(drv):
    """Table ids, prefixes, the empty key, the lengths around the loads; every
    present key at every residue mod 16 in the key buffer."""
    bs = [drv.batch(ls) for ls in identity_lists()]
    tab = drv.table(256, 2)
    try:
        for b in bs:
            tab.add(b)
        exp = checked_expectation(tab)
        keys = identity_keys()
        assert all(k in exp for k in keys)
        near = absent_neighbours(keys)
        assert len(near) > len(keys)
        res = lookup(tab, exp, keys + near, what="identity")
        assert (res["kind"][:len(keys)] != ABSENT).all() and (res["kind"][len(keys):] == ABSENT).all()
        for n, key in enumerate(keys):
            if res["kind"][n] == OBJECT:
                assert value_bytes(bs, res[n]) in (b"newer", b"value of %d/%d" % (key[0], len(key[1])))
        for shift in range(16):
            lookup(tab, exp, keys, what=("residue", shift), align=16, shift=shift)
    finally:
        tab.close()


def case_longest_key(drv):
    """A key of 65,535 bytes, its prefix of 65,534 and a twin that differs in
    the last byte, in one segment of 256 KiB."""
    rng = np.random.default_rng(77)
    long = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    twin = long[:-1] + bytes([long[-1] ^ 1])
    b = drv.batch([[tc.head(1), rc.obj(3, long, 2, b"long's value"), rc.tomb(3, long[:-1], 6)]], cap=256 * KiB)
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        exp = checked_expectation(tab)
        res = lookup(tab, exp, [(3, long), (3, long[:-1]), (3, twin), (3, long[:16])], what="65,535", shift=3)
        assert res["kind"].tolist() == [OBJECT, TOMBSTONE, ABSENT, ABSENT]
        assert value_bytes([b], res[0]) == b"long's value"
    finally:
        tab.close()


def case_one_chain(drv):
    """Every caller hash is 7: the table is one probe chain over both batches.
    Present keys lie at its start, middle and end; absent keys walk all of it."""
    bs = [drv.batch(ls) for ls in tc.split_lists(rc.collision_entries())]
    tab = drv.table(64, 2)
    try:
        for b in bs:
            tab.add(b, np.full(b.table.shape[0], 7, np.uint64))
        exp = checked_expectation(tab)
        keys = all_keys(bs)
        assert len(keys) == 50
        keys = keys + [(1, b"not there"), (3, b""), (1, b"0123456789abcdefZ")]
        res = lookup(tab, exp, keys, np.full(len(keys), 7, np.uint64), "hash 7")
        assert (res["kind"][:50] != ABSENT).all() and (res["kind"][50:] == ABSENT).all()
    finally:
        tab.close()


def case_seed_collisions(drv):
    bs = [drv.batch(ls) for ls in tc.split_lists(rc.seed_collision_entries(), at=6)]
    tab = drv.table(64, 2)
    try:
        for b in bs:
            tab.add(b)
        exp = checked_expectation(tab)
        keys = all_keys(bs)
        assert len(keys) == 6
        lookup(tab, exp, keys + [((2 << 32) + 1, k) for _, k in keys[:3]], what="seed")
    finally:
        tab.close()


def mixed_batches(drv):
    return [drv.batch([es], rc.MIXED_CAP, bad=[0] if j == rc.MIXED_BAD else [])
            for j, es in enumerate(rc.mixed_lists())]


def case_mixed_hashes(drv, mixed):
    """Batch 0 added with the partition call's hashes, batch 1 with NULL; the
    lookup once with computed and once with given hashes."""
    bs = mixed[:2]
    tabs = pc.tablets([(tid, 0, tc.ALL, 0, 0, 0) for tid in (1, 2, (1 << 32) + 1)])
    _, _, h0, _ = drv.ramcrc.recovery_partition_host(bs[0].buf, bs[0].cap, 1, bs[0].status, bs[0].table,
                                                     tabs, 1)
    tab = drv.table(1000, 2)
    try:
        tab.add(bs[0], np.asarray(h0, np.uint64)[:bs[0].table.shape[0]])
        tab.add(bs[1])
        exp = checked_expectation(tab)
        keys = all_keys(bs) + [(1, b"no such key")]
        a = lookup(tab, exp, keys, what="computed")
        given = np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)
        b = lookup(tab, exp, keys, given, what="given")
        assert same(a, b)
    finally:
        tab.close()


def case_absent_on_a_claimed_slot(drv):
    keys = [(1, b"slot key %d" % n) for n in range(20)]
    b = drv.batch([[tc.head(1)] + [rc.obj(t, k, 1, b"v") for t, k in keys]])
    tab = drv.table(64, 1)   # 128 slots
    try:
        tab.add(b)
        exp = checked_expectation(tab)
        ghost = same_slot_absent(keys, 128)
        res = lookup(tab, exp, [ghost] + keys, what="a claimed slot")
        assert res["kind"][0] == ABSENT and (res["kind"][1:] == OBJECT).all()
    finally:
        tab.close()


def case_multi_key(drv):
    lists, want = multi_key_lists()
    b = drv.batch(lists)
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        exp = checked_expectation(tab)
        keys = sorted(want)
        assert set(keys) == set(exp)
        res = lookup(tab, exp, keys, what="multi-key")
        for key, r in zip(keys, res):
            assert r["kind"] == OBJECT
            if want[key] is None:
                _, off, ln, hdr = (int(x) for x in b.table[int(r["record"])])
                assert r["value_len"] == 0 and r["value_off"] == off + 1 + ((hdr >> 6) & 3) + 1 + ln
            else:
                assert value_bytes([b], r) == want[key], key
    finally:
        tab.close()


def case_bad_queries(drv):
    """Unusable queries among good ones; the last good key ends exactly at
    keys_bytes."""
    bs = [drv.batch(ls) for ls in identity_lists()]
    tab = drv.table(256, 2)
    try:
        for b in bs:
            tab.add(b)
        exp = checked_expectation(tab)
        good = identity_keys()[3:12]
        kb, q = segments.lookup_queries(good + [(1, b"absent")] + good[:4] + [good[-1]])
        n = len(good) + 1
        assert int(q["key_off"][-1] + q["key_len"][-1]) == kb.size
        q["key_len"][n] = 65536
        q["reserved"][n + 1] = 1
        q["key_off"][n + 2], q["key_len"][n + 2] = kb.size - 3, 4    # ends at keys_bytes + 1
        q["key_off"][n + 3] = (1 << 64) - 1
        keys = good + [(1, b"absent")] + good[:4] + [good[-1]]
        want = expected_results(exp, keys, bad=range(n, n + 4))
        for hashes in (None, np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)):
            res, counts = tab.lookup_raw(kb, q, hashes)
            assert same(res, want), [(k, r, w) for k, r, w in zip(keys, res, want) if r != w][:3]
            assert counts == expected_counts(want) and counts["bad"] == 4
            assert res["kind"][-1] != ABSENT and res["kind"][n - 1] == ABSENT
    finally:
        tab.close()


def case_duplicates(drv):
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        exp = checked_expectation(tab)
        res = lookup(tab, exp, [(1, b"y")] * 1000 + [(1, b"x")] * 3 + [(1, b"z")] * 5, what="duplicates")
        assert (res["kind"][:1000] == OBJECT).all() and len(set(res[:1000].tobytes()[i:i + 32]
                                                                 for i in range(0, 32000, 32))) == 1
    finally:
        tab.close()


def case_exhaustive(drv, mixed):
    """Four batches in two add orders: the lookup of every participant's own
    key names what the live query names."""
    for order in ([0, 1, 2, 3], [2, 0, 3, 1]):
        bs = [mixed[j] for j in order]
        tab = drv.table(1000, 4)
        try:
            for b in bs:
                tab.add(b)
            exp = checked_expectation(tab)
            winners = tab.winners()
            for b, ks, w in zip(bs, participant_keys(bs), winners):
                idx = [i for i, k in enumerate(ks) if k is not None]
                res = lookup(tab, exp, [ks[i] for i in idx], what=("exhaustive", order))
                assert np.array_equal(res["batch"], w["batch"][idx])
                assert np.array_equal(res["record"], w["record"][idx])
            assert len(exp) > 100
        finally:
            tab.close()


def case_read_only(drv, mixed):
    tab = drv.table(1000, 4)
    try:
        tab.add(mixed[0])
        tab.add(mixed[1])
        exp2 = checked_expectation(tab)
        keys = all_keys(mixed) + [(1, b"absent")]
        before = tab.state()
        a = lookup(tab, exp2, keys, what="first")
        b = lookup(tab, exp2, keys, what="second")
        assert same(a, b) and tab.state() == before
        # a lookup between two adds changes no later answer
        tab.add(mixed[2])
        tab.add(mixed[3])
        exp4 = checked_expectation(tab)
        lookup(tab, exp4, keys, what="after two more adds")
        fresh = drv.table(1000, 4)
        try:
            for m in mixed:
                fresh.add(m)
            assert fresh.state() == tab.state()
        finally:
            fresh.close()
    finally:
        tab.close()


def case_nullable_and_empty(drv):
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    hot = drv.batch([[tc.head(2), rc.obj(1, b"x", 9, b"the other table's")]])
    tab, other = drv.table(64, 1), drv.table(64, 1)
    try:
        tab.add(b)
        other.add(hot)
        exp, exp_o = checked_expectation(tab), checked_expectation(other)
        res, counts = tab.lookup_raw(np.zeros(0, np.uint8), np.zeros(0, KEY))
        assert res.shape[0] == 0 and counts == dict.fromkeys(COUNT_NAMES, 0)
        tab.lookup_raw(np.zeros(0, np.uint8), np.zeros(0, KEY), want_counts=False)
        lookup(tab, exp, [(1, b"x"), (1, b"q")], what="no counts", want_counts=False)
        # the empty key alone: an empty key buffer
        lookup(tab, exp, [(1, b"")], what="no key bytes")
        a = lookup(tab, exp, [(1, b"x")])
        o = lookup(other, exp_o, [(1, b"x")])
        assert a["kind"][0] == TOMBSTONE and o["kind"][0] == OBJECT and o["version"][0] == 9
        assert value_bytes([hot], o[0]) == b"the other table's"
    finally:
        tab.close()
        other.close()


def case_reference(drv):
    """The reference's own cases, their records one per batch: the lookup of a
    case's key gives the fixture's survivor."""
    ref = pc.load("replay_resolve_ref.json")
    lists, _ = tc.reference_lists(ref)
    bs = [drv.batch([es]) for es in lists]
    tab = drv.table(256, len(bs))
    try:
        for b in bs:
            tab.add(b)
        exp = checked_expectation(tab)
        keys = [(ref["table_id"], c["records"][0][1].encode()) for c in ref["cases"]]
        res = lookup(tab, exp, keys, what="reference")
        for c, r in zip(ref["cases"], res):
            sv = c["survivor"]
            assert r["kind"] == (OBJECT if sv["type"] == "OBJ" else TOMBSTONE), c["name"]
            assert r["version"] == sv["version"] and r["batch"] == sv["index"], c["name"]
    finally:
        tab.close()
