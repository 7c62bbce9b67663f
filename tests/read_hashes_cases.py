"""Cases and the expectation for an indexed read against the replay table
(ramcrc_replay_table_read_hashes_host / _device).

The expectation is plain Python: the lookup expectation of lookup_cases.py
(the sequential replay, held against the live query's winners) gives every
key's winner; a key answers asked hash h when its table id is the asked one
and its record hash -- the hash its adds were given, Key::getHash otherwise --
equals h; a hash's objects go in ascending winner {batch, record}, each as
{u64 version, u32 length} and the payload from byte 24
(ObjectManager::readHashes, src/ObjectManager.cc:179-265); the reply is cut
before the first hash that begins past max_length (:258-263) or ends past the
reply's capacity.  All of it is restated here independently of the library.
The tests hold it against tests/golden/read_hashes_ref.json before any call
is held against it.
"""
import ctypes
import struct

import numpy as np

from ramcloud_amd import segments

import clean_cases as cl
import lookup_cases as lc
import partition_cases as pc
import read_cases as rd
import replay_table_cases as tc
import resolve_cases as rc
import write_cases as wc

KiB = 1024
FILL = lc.FILL
FILL32 = lc.FILL32
HUGE = 1 << 62
NONE = segments.READ_NONE
PART = segments.HASH_PART_DTYPE
SUMMARY = segments.READ_HASHES_SUMMARY_DTYPE
SUMMARY_NAMES = SUMMARY.names
ZERO_SUMMARY = dict.fromkeys(SUMMARY_NAMES, 0)
SPOILED_SUMMARY = dict(ZERO_SUMMARY, spoiled=1)
PAD = 64
# The kernels' thresholds, which the tile-edge and size-class cases straddle:
# kPartThreads (dev_partition.inc), kAppBigMin and kAppGroupMin (dev_append.inc).
# test_the_cases_straddle_the_kernels_thresholds holds them against the sources.
TILE = 256          # hashes per tile
BIG_MIN = 2048      # data bytes from which a wave copies
GROUP_MIN = 65536   # data bytes from which the workgroup copies


def source_constants():
    """kPartThreads, kAppBigMin and kAppGroupMin as the kernel sources state them."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(segments.__file__)), "csrc")
    text = open(os.path.join(csrc, "dev_partition.inc")).read() + open(os.path.join(csrc, "dev_append.inc")).read()
    out = {}
    for name in ("kPartThreads", "kAppBigMin", "kAppGroupMin"):
        m = re.search(r"constexpr \w+ %s = ([0-9* ]+);" % name, text)
        assert m, name
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        out[name] = v
    return out


T2 = (1 << 32) + 1


def key_hash(key):
    return pc.key_hash(key[0], key[1])


# ---------------------------------------------------------- the expectation
class Want:
    """What a call must give.  exp, pays: read_cases.payloads' pair (or a clean
    model's results() and payloads()); hash_of: key -> its record hash."""

    def __init__(self, exp, pays, hash_of, table_id, asked, max_length=HUGE, capacity=None):
        by_hash, tombs = {}, {}
        for key, res in exp.items():
            if key[0] != table_id:
                continue
            h = hash_of(key)
            if res[3] == lc.OBJECT:
                by_hash.setdefault(h, []).append((res[0], res[1], res[2], pays[key]))
            else:
                tombs[h] = tombs.get(h, 0) + 1
        self.hash_bytes, self.hash_objects, self.starts, self.ends = [], [], [], []
        at = 0
        for h in asked:
            objs = sorted(by_hash.get(int(h), []), key=lambda o: o[:2])   # {batch, record}, batch first
            raw = b"".join(struct.pack("<QI", ver, len(pay) - 24) + pay[24:] for _, _, ver, pay in objs)
            self.hash_bytes.append(raw)
            self.hash_objects.append([(ver, pay[24:]) for _, _, ver, pay in objs])
            self.starts.append(at)
            at += len(raw)
            self.ends.append(at)
        self.total = at
        self.longest = max([len(x) for x in self.hash_bytes], default=0)
        # with room for max_length and the longest hash's parts, the reference's
        # rule alone decides
        self.capacity = min(max_length, self.total) + self.longest if capacity is None else capacity
        self.summary = dict(ZERO_SUMMARY)
        self.parts, self.objects, reply, open_ = [], [], [], True
        for q, h in enumerate(asked):
            if open_ and self.starts[q] <= max_length and self.ends[q] <= self.capacity:
                objs = self.hash_objects[q]
                self.parts.append((self.starts[q], len(objs), 0))
                self.objects += objs
                reply.append(self.hash_bytes[q])
                s = self.summary
                s["hashes"] += 1
                s["objects"] += len(objs)
                s["reply_bytes"] = self.ends[q]
                s["empty"] += not objs
                s["tombstones"] += tombs.get(int(h), 0)
                for _, data in objs:
                    vo, vl = lc.value_range(bytes(24) + data)
                    s["value_bytes"] += vl
                    s["key_bytes"] += len(data) - vl
            else:
                if open_:
                    # the first hash that is not returned stays in numObjects
                    self.summary["objects_counted"] = len(self.hash_objects[q])
                open_ = False
                self.parts.append((NONE, 0, 0))
        self.summary["objects_counted"] += self.summary["objects"]
        self.reply = b"".join(reply)
        assert len(self.reply) == self.summary["reply_bytes"]


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


# ------------------------------------------------------------------ drivers
class Got:
    """One call's outputs as numpy: reply (the bytes before reply_bytes), parts,
    summary."""


def _finish(g, n, want_parts):
    assert (g.reply_all[g.summary["reply_bytes"]:] == FILL).all(), "a byte at or past reply_bytes was written"
    assert (g.summary_past == FILL).all(), "a byte past the summary was written"
    g.reply = g.reply_all[:g.summary["reply_bytes"]].tobytes()
    g.parts = None
    if want_parts:
        assert (g.parts_all[16 * n:] == FILL).all(), "a byte past d_parts was written"
        g.parts = g.parts_all[:16 * n].view(PART)
    return g


def host_call(R, t, table_id, asked, room, capacity, max_length, want_parts=True, shift=0):
    """ramcrc_replay_table_read_hashes_host on buffers pre-filled with 0xA5; the
    hashes and parts lie at odd addresses (no alignment rule)."""
    n = len(asked)
    g = Got()
    g.reply_all = np.full(room + PAD + shift, FILL, np.uint8)[shift:]
    g.parts_all = np.full(16 * n + PAD + 1, FILL, np.uint8)[1:]
    sm = np.full(SUMMARY.itemsize + PAD + 1, FILL, np.uint8)[1:]
    hs = np.zeros(8 * n + 1, np.uint8)[1:]
    hs[:] = np.asarray(asked, np.uint64).view(np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None
    code = R.lib().ramcrc_replay_table_read_hashes_host(
        t._h, int(table_id), p(hs), n, 0, ctypes.c_void_p(g.reply_all.ctypes.data), int(capacity),
        int(max_length), p(g.parts_all) if want_parts else None, p(sm))
    assert code == 0, code
    g.summary = summary_dict(sm[:SUMMARY.itemsize].copy().view(SUMMARY)[0])
    g.summary_past = sm[SUMMARY.itemsize:]
    return _finish(g, n, want_parts)


class Asked:
    """One ramcrc_replay_table_read_hashes_device call: every output pre-filled
    with 0xA5 and longer than the call may write; the reply starts `shift`
    bytes into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, table_id, asked, room, capacity, max_length, want_parts=True, shift=0,
                 check=True):
        import torch
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        self.n = n = len(asked)
        self.want_parts = want_parts
        assert capacity <= room + PAD
        hs = np.asarray(asked, np.uint64).view(np.int64)
        self.d_hashes = torch.from_numpy(hs.copy()).cuda() if n else None
        self.d_reply = fill(room + PAD + shift)[shift:]
        self.d_parts = fill(16 * n + PAD).view(torch.int64) if want_parts else None
        self.d_sum = fill(SUMMARY.itemsize + PAD).view(torch.int64)
        t.read_hashes(table_id, self.d_hashes, self.d_reply, self.d_sum, max_length, parts=self.d_parts,
                      n_hashes=n, reply_capacity=capacity)
        if check:
            ctx.check()
            self.read()

    def read(self):
        sm = self.d_sum.cpu().numpy().view(np.uint8)
        self.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
        self.summary_past = sm[SUMMARY.itemsize:]
        self.reply_all = self.d_reply.cpu().numpy()
        self.parts_all = self.d_parts.cpu().numpy().view(np.uint8) if self.want_parts else None
        return _finish(self, self.n, self.want_parts)


def call(tab, table_id, asked, room, capacity, max_length, want_parts=True, shift=0):
    """The call on `tab` (a driver's table); on the device it is also held byte
    for byte against the host twin's."""
    R = tab.drv.ramcrc
    if not tab.drv.on_device:
        return host_call(R, tab.t, table_id, asked, room, capacity, max_length, want_parts, shift)
    g = Asked(tab.drv.ctx, tab.t, table_id, asked, room, capacity, max_length, want_parts, shift)
    h = host_call(R, tab.twin, table_id, asked, room, capacity, max_length, want_parts)
    assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
    assert h.reply == g.reply, ("host and device replies differ", rd.first_difference(h.reply, g.reply))
    assert not want_parts or lc.same(h.parts, g.parts), "host and device parts differ"
    return g


class HostDriver(cl.HostDriver):
    pass


class DeviceDriver(cl.DeviceDriver):
    pass


def ask(tab, ep, hash_of, table_id, asked, max_length=HUGE, capacity=None, what="", **kw):
    """The call against the expectation.  Returns (the call's outputs, the Want)."""
    exp, pays = ep
    asked = [int(h) for h in asked]
    w = Want(exp, pays, hash_of, table_id, asked, max_length, capacity)
    room = min(w.capacity, w.total)
    g = call(tab, table_id, asked, room, min(w.capacity, room + PAD), max_length, **kw)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.reply == w.reply, (what, "reply bytes", rd.first_difference(g.reply, w.reply))
    if g.parts is not None:
        assert [tuple(int(x) for x in p) for p in g.parts] == w.parts, (what, "parts")
    assert segments.read_hashes_objects(g.reply, g.summary["objects"]) == w.objects, what
    return g, w


def checked(tab):
    return rd.checked(tab)


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("read_hashes_ref.json")


def check_expectation_against_golden(ref):
    """The project's Key::getHash gives the constant the reference's test
    states, and a part's header is 12 bytes; returns how many scenarios."""
    for c in ref["key_hash_constants"]:
        assert pc.key_hash(c["table_id"], c["key"].encode()) == c["hash"], c
    assert ref["part_header"] == {"version_bytes": 8, "length_bytes": 4}
    assert struct.calcsize("<QI") == 12 == segments.READ_HASHES_OBJECT_DTYPE.itemsize
    return len(ref["scenarios"])


def case_goldens(drv):
    ref = golden()
    assert check_expectation_against_golden(ref) == 3
    for sc in ref["scenarios"]:
        tid = sc["table_id"]
        es = [tc.head(1)] + [lc.multi_obj(tid, [k.encode() for k in o["keys"]], o["value"].encode(), o["version"])
                             for o in sc["objects"]]
        tab = drv.table(64, 1)
        try:
            tab.add(drv.batch([es]))
            ep = checked(tab)
            asked = sc.get("ask_hashes") or [pc.key_hash(tid, k.encode()) for k in sc["ask"]]
            assert asked == [pc.key_hash(tid, k.encode()) for k in sc["ask"]]
            ml = HUGE if sc["max_length"] is None else sc["max_length"]
            g, w = ask(tab, ep, key_hash, tid, asked, max_length=ml, what=sc["name"])
            assert g.summary["hashes"] == sc["hashes"] and g.summary["objects"] == sc["objects_returned"]
            assert g.summary["objects_counted"] == sc["objects_returned"], sc["name"]
            at = 0
            for n in sc["order"]:
                o = sc["objects"][n]
                version, length = struct.unpack_from("<QI", g.reply, at)   # version, length, keys and value
                assert length == o["length"] and (version == o["version"] or not o["version_checked"])
                data = g.reply[at + 12:at + 12 + length]
                assert data[0] == len(o["keys"]) and data.endswith(o["value"].encode()), sc["name"]
                assert data[1 + 2 * len(o["keys"]):].startswith("".join(o["keys"]).encode())
                at += 12 + length
            assert at == g.summary["reply_bytes"]
        finally:
            tab.close()


# ---------------------------------------------------------------- scenarios
def table_hashes(exp, table_id, hash_of=key_hash):
    return [hash_of(k) for k in sorted(exp) if k[0] == table_id]


def case_relations(drv):
    """tc.relation_lists() across two and three batches, every table's hashes
    asked after every add: a newer object replaces the part, a winner tombstone
    silences the hash and counts, an object over a tombstone returns."""
    bs = [drv.batch([es]) for es in tc.relation_lists()]
    stale = key_hash((4, b"stale pick"))
    seen = []
    tab = drv.table(2000, 3)
    try:
        for k, b in enumerate(bs):
            tab.add(b)
            ep = checked(tab)
            tombs = 0
            for tid in sorted({key[0] for key in ep[0]}):
                asked = table_hashes(ep[0], tid) + [key_hash((tid, b"nobody's key"))]
                g, w = ask(tab, ep, key_hash, tid, asked, what=("after add", k, tid))
                tombs += g.summary["tombstones"]
                assert g.summary["hashes"] == len(asked) and g.summary["empty"] >= 1
            assert tombs == sum(r[3] == lc.TOMBSTONE for r in ep[0].values()) > 0
            g, w = ask(tab, ep, key_hash, 4, [stale], what=("stale pick", k))
            seen.append((g.summary["objects"], g.summary["tombstones"], [v for v, _ in w.objects]))
    finally:
        tab.close()
    assert seen == [(0, 1, []), (1, 0, [7]), (1, 0, [7])]


def fan_lists(n, adds):
    """n keys of table 1 (and three of table 2 with the same bytes) over `adds`
    batches; with three adds, key 0 gets a newer object and key 1 a tombstone in
    the last batch, so that winners do not lie in key order."""
    keys = [(1, b"fan %d" % i) for i in range(n)]
    lists = [[tc.head(1 + j)] for j in range(adds)]
    for i, (tid, key) in enumerate(keys):
        lists[i % adds].append(rc.obj(tid, key, 2, b"fan value %d " % i * (i % 5)))
    for i in range(min(n, 3)):
        lists[(i + 1) % adds].append(rc.obj(2, b"fan %d" % i, 1, b"another table's"))
    if adds > 1:
        lists[-1].append(rc.obj(1, b"fan 0", 3, b"newer"))
        if n > 1:
            lists[-1].append(rc.tomb(1, b"fan 1", 2))
    return lists


def case_fan_out(drv):
    """Every key is given caller hash 7: 1, 2, 3 and 40 keys, arriving in one
    add and split over three.  7 gives all the objects in the order of their
    winners; 8 and 7 + nslots (the same start slot, or a neighbouring chain)
    give nothing.  Then a second group with hash 8 on the same chain: each hash
    gets its own keys only."""
    key_cap = 64
    nslots = cl.rc_slots(key_cap)
    for n in (1, 2, 3, 40):
        for adds in (1, 3):
            bs = [drv.batch([es]) for es in fan_lists(n, adds)]
            tab = drv.table(key_cap, adds + 1)
            try:
                for b in bs:
                    tab.add(b, np.full(b.table.shape[0], 7, np.uint64))
                ep = checked(tab)
                seven = lambda key: 7
                what = ("fan-out", n, adds)
                g, w = ask(tab, ep, seven, 1, [7], what=what)
                live = [k for k, r in ep[0].items() if k[0] == 1 and r[3] == lc.OBJECT]
                assert g.summary["objects"] == len(live) == (n if adds == 1 or n == 1 else n - 1)
                refs = [ep[0][k][:2] for k in live]
                assert [v for v, _ in w.objects] == [ep[0][k][2] for _, k in sorted(zip(refs, live))]
                if adds == 3 and n == 40:   # the newer object of "fan 0" lies in the last batch: it goes last
                    assert w.objects[-1] == (3, ep[1][(1, b"fan 0")][24:]) and g.summary["tombstones"] == 1
                g, w = ask(tab, ep, seven, 1, [8, 7 + nslots, 7, 6], what=what)
                assert [p[1] for p in w.parts] == [0, 0, len(live), 0] and g.summary["empty"] == 3
                g, w = ask(tab, ep, seven, 2, [7], what=what)
                assert g.summary["objects"] == min(n, 3)
                # the second group: hash 8, the same chain
                more = [rc.obj(1, b"eight %d" % i, 1, b"8" * i) for i in range(5)]
                bm = drv.batch([[tc.head(9)] + more])
                tab.add(bm, np.full(bm.table.shape[0], 8, np.uint64))
                ep = checked(tab)
                both = lambda key: 8 if key[1].startswith(b"eight") else 7
                g, w = ask(tab, ep, both, 1, [7, 8, 9, 8], what=what)
                assert [p[1] for p in w.parts] == [len(live), 5, 0, 5]
            finally:
                tab.close()


def case_seed_collisions(drv):
    """The same key under table ids 1 and 2^32 + 1 has equal Key::getHash: each
    table_id gets its own object only."""
    es = rc.seed_collision_entries() + [rc.obj(1, b"both", 5, b"table one's"), rc.obj(T2, b"both", 6, b"the other's")]
    bs = [drv.batch(ls) for ls in tc.split_lists(es, at=6)]
    tab = drv.table(64, 2)
    try:
        for b in bs:
            tab.add(b)
        ep = checked(tab)
        h = pc.key_hash(1, b"both")
        assert h == pc.key_hash(T2, b"both")
        g, w = ask(tab, ep, key_hash, 1, [h], what="table 1")
        assert w.objects == [(5, ep[1][(1, b"both")][24:])]
        g, w = ask(tab, ep, key_hash, T2, [h], what="table 2^32 + 1")
        assert w.objects == [(6, ep[1][(T2, b"both")][24:])]
        g, w = ask(tab, ep, key_hash, (2 << 32) + 1, [h], what="a table nobody has")
        assert g.summary["objects"] == 0 and g.summary["empty"] == 1
        for tid in (1, T2):
            asked = table_hashes(ep[0], tid)
            g, w = ask(tab, ep, key_hash, tid, asked, what=("seed", tid))
            assert g.summary["objects"] + g.summary["tombstones"] == len(asked) == 4
    finally:
        tab.close()


def case_mixed_hashes(drv, mixed):
    """Batch 0 added with the partition call's hashes, batch 1 with NULL, and
    the other way round: the answers are those of Key::getHash throughout."""
    bs = mixed[:2]
    tabs = pc.tablets([(tid, 0, tc.ALL, 0, 0, 0) for tid in (1, 2, T2)])
    part = lambda b: np.asarray(drv.ramcrc.recovery_partition_host(b.buf, b.cap, 1, b.status, b.table, tabs, 1)[2],
                                np.uint64)[:b.table.shape[0]]
    replies = []
    for given in ((True, False), (False, True), (False, False), (True, True)):
        tab = drv.table(1000, 2)
        try:
            for b, gv in zip(bs, given):
                tab.add(b, part(b) if gv else None)
            ep = checked(tab)
            for tid in (1, 2, T2):
                asked = table_hashes(ep[0], tid) + [pc.key_hash(tid, b"no such key")]
                g, w = ask(tab, ep, key_hash, tid, asked, what=("mixed", given, tid))
                assert g.summary["objects"] + g.summary["tombstones"] == len(asked) - 1
                replies.append(g.reply)
        finally:
            tab.close()
    assert replies[:3] == replies[3:6] == replies[6:9] == replies[9:] and any(replies)


def case_after_a_clean(drv, mixed):
    """A table built with Key::getHash: after a clean the survivor has no
    stored hashes and the answers stay; after a write, a walk and an add of its
    output they follow the table."""
    key_cap = 2000
    tab, model = drv.table(key_cap, len(mixed) + 4), cl.Model()
    try:
        for b in mixed:
            cl.add(tab, model, b)
        tids = sorted({k[0] for k in model.win})
        before = {}
        for tid in tids:
            asked = table_hashes(model.results(), tid)
            g, w = ask(tab, (model.results(), model.payloads()), key_hash, tid, asked, what=("before", tid))
            before[tid] = (asked, g.reply)
            assert g.summary["objects"] > 0
        g, w = cl.clean(tab, model, drv, [0, 2], key_cap, what="read hashes", cap=mixed[0].cap, more=False,
                        ties=True, scribble=False)   # (the batches are the module's)
        assert w.summary["moved_objects"] > 0
        for tid in tids:
            asked, reply = before[tid]
            g, w = ask(tab, (model.results(), model.payloads()), key_hash, tid, asked, what=("after", tid))
            assert g.reply == reply, "a hash answers differently after the clean"
        exp = model.results()
        live = [k for k in sorted(exp) if exp[k][3] == lc.OBJECT and k[0] == tids[0]]
        objs = [(tid, key, b"rewritten %d" % n) for n, (tid, key) in enumerate(live[::3])]
        gw, ww = wc.write(tab, exp, objs, what="write", next_version=1 << 20)
        bw, bad = tab.batch_of(gw.out, gw.cert)
        assert bad == 0 and ww.summary["ok"] == len(objs)
        cl.add(tab, model, bw)
        asked = before[tids[0]][0]
        g, w = ask(tab, (model.results(), model.payloads()), key_hash, tids[0], asked, what="after the write")
        assert g.reply != before[tids[0]][1]
        assert sum(data.endswith(b"rewritten %d" % n) for n in range(len(objs)) for _, data in w.objects) >= len(objs)
    finally:
        tab.close()


def case_multi_key(drv):
    """Objects of 0, 1, 2 and 3 keys, and the object whose key table runs past
    its payload: it still sends its payload from byte 24."""
    lists, want = lc.multi_key_lists()
    tab = drv.table(64, 1)
    try:
        tab.add(drv.batch(lists))
        ep = checked(tab)
        for tid in (5, 6):
            keys = [k for k in sorted(want) if k[0] == tid]
            g, w = ask(tab, ep, key_hash, tid, [key_hash(k) for k in keys], what=("multi-key", tid))
            assert [data for _, data in w.objects] == [ep[1][k][24:] for k in keys]
            assert g.summary["value_bytes"] == sum(len(want[k] or b"") for k in keys)
            assert g.summary["key_bytes"] == sum(len(ep[1][k]) - 24 - len(want[k] or b"") for k in keys)
        past = ep[1][(5, b"past")][24:]
        g, w = ask(tab, ep, key_hash, 5, [key_hash((5, b"past"))], what="past")
        assert w.objects == [(1, past)] and past[0] == 3 and past.endswith(b"pastxyzz")
        assert g.summary["value_bytes"] == 0 and g.summary["key_bytes"] == len(past)
    finally:
        tab.close()


def data_len_value(key, data_len):
    """The value length that gives a one-key object `data_len` bytes of keys and value."""
    return data_len - 3 - len(key)


def case_alignment_and_size_classes(drv):
    """Data of every copy class in one request -- values of 0, 1 and 64 bytes,
    data lengths on either side of kAppBigMin and kAppGroupMin, one 100 KiB
    value -- in both orders and at two bases of the reply; then parts beginning
    at every residue mod 16, steered by the lengths before them."""
    rng = np.random.default_rng(31)
    es, keys = [tc.head(1)], []
    for n, dl in enumerate([None, None, None, BIG_MIN - 1, BIG_MIN, BIG_MIN + 1, GROUP_MIN - 1, GROUP_MIN,
                            GROUP_MIN + 1, None]):
        key = b"class %d" % n
        vl = [0, 1, 64][n] if n < 3 else 100 * KiB if dl is None else data_len_value(key, dl)
        es.append(rc.obj(1, key, 1 + n, rng.integers(0, 256, vl, dtype=np.uint8).tobytes()))
        keys.append((1, key))
    steer = [(3, b"steer %02d" % n) for n in range(16)]
    es += [rc.obj(3, k, 1, bytes(range(n))) for n, (_, k) in enumerate(steer)]
    tab = drv.table(64, 1)
    try:
        tab.add(drv.batch([es], cap=512 * KiB))
        ep = checked(tab)
        for order in (keys, keys[::-1]):
            for shift in (0, 5):
                g, w = ask(tab, ep, key_hash, 1, [key_hash(k) for k in order], what=("classes", shift), shift=shift)
                assert g.summary["objects"] == len(keys)
                assert sorted(len(d) for _, d in w.objects)[3:9] == [BIG_MIN - 1, BIG_MIN, BIG_MIN + 1,
                                                                     GROUP_MIN - 1, GROUP_MIN, GROUP_MIN + 1]
        # 16 consecutive lengths: the running offset takes every residue
        order = steer * 2 + steer[::-1]
        g, w = ask(tab, ep, key_hash, 3, [key_hash(k) for k in order], what="residues")
        assert {s % 16 for s in w.starts} == set(range(16))
        ask(tab, ep, key_hash, 3, [key_hash(k) for k in order], what="residues, shifted", shift=3)
    finally:
        tab.close()


def truncation_table(drv):
    """One batch under caller hashes: hash 100 + i has one object of i * 7
    value bytes (i < 8), hash 50 none (a tombstone), hash 60 three objects."""
    es, hs = [tc.head(1)], [0]
    for i in range(8):
        es.append(rc.obj(1, b"t%d" % i, 2 + i, b"v" * (i * 7)))
        hs.append(100 + i)
    es.append(rc.tomb(1, b"dead", 9))
    hs.append(50)
    for i in range(3):
        es.append(rc.obj(1, b"three %d" % i, 1, b"3" * (10 + i)))
        hs.append(60)
    hash_of = {(1, b"dead"): 50}
    hash_of.update({(1, b"t%d" % i): 100 + i for i in range(8)})
    hash_of.update({(1, b"three %d" % i): 60 for i in range(3)})
    tab = drv.table(64, 1)
    b = drv.batch([es])
    tab.add(b, np.array(hs, np.uint64))
    return tab, hash_of.__getitem__


def case_truncation(drv):
    """max_length one byte around every hash's start (start == max_length
    keeps the hash, start == max_length + 1 drops it), the overshoot past
    max_length, objects_counted when the dropped hash has 0, 1 and 3 objects,
    and the capacity rule on its own."""
    tab, hash_of = truncation_table(drv)
    try:
        ep = checked(tab)
        asked = [101, 60, 103, 50, 999, 60, 107, 100, 102, 50, 105, 60, 104]
        full = Want(ep[0], ep[1], hash_of, 1, asked)
        assert full.summary["hashes"] == len(asked) and full.summary["objects"] == 16
        counts = [len(o) for o in full.hash_objects]
        assert set(counts) == {0, 1, 3}
        dropped = set()
        for q in range(len(asked)):
            s = full.starts[q]
            for ml in (s, s - 1, s + 1):
                if ml < 0:
                    continue
                g, w = ask(tab, ep, hash_of, 1, asked, max_length=ml, what=("max_length", q, ml))
                n = g.summary["hashes"]
                assert n == sum(st <= ml for st in full.starts)
                assert w.capacity == min(ml, full.total) + full.longest   # the reference's rule alone decides
                assert g.summary["reply_bytes"] == (full.ends[n - 1] if n else 0)
                assert [p[0] for p in w.parts[n:]] == [NONE] * (len(asked) - n)
                extra = counts[n] if n < len(asked) else 0
                assert g.summary["objects_counted"] == g.summary["objects"] + extra
                if n < len(asked):
                    dropped.add(counts[n])
            g, w = ask(tab, ep, hash_of, 1, asked, max_length=s, what=("keeps", q))
            assert g.summary["hashes"] > q and g.summary["reply_bytes"] >= full.ends[q]
            if s and full.starts[q - 1] != s:
                g, w = ask(tab, ep, hash_of, 1, asked, max_length=s - 1, what=("drops", q))
                assert g.summary["hashes"] <= q
        assert dropped == {0, 1, 3}
        # the overshoot: the hash that begins at max_length is in the reply whole
        q = asked.index(60)
        g, w = ask(tab, ep, hash_of, 1, asked, max_length=full.starts[q], what="overshoot")
        assert g.summary["reply_bytes"] == full.ends[q] > full.starts[q] + 2 * 12
        assert g.reply[full.starts[q]:] == full.hash_bytes[q]
        # the capacity rule alone: max_length never cuts
        for q in range(len(asked)):
            for cap in (full.ends[q], full.ends[q] - 1, full.ends[q] + 1):
                if cap < 0:
                    continue
                g, w = ask(tab, ep, hash_of, 1, asked, capacity=cap, what=("capacity", q, cap))
                n = g.summary["hashes"]
                assert n == sum(e <= cap for e in full.ends) and g.summary["reply_bytes"] <= cap
        g, w = ask(tab, ep, hash_of, 1, asked, max_length=0, capacity=0, what="nothing fits")
        assert g.summary["hashes"] == 0 and g.summary["objects_counted"] == 1
        g, w = ask(tab, ep, hash_of, 1, [999, 50, 101], max_length=0, capacity=0, what="only empty hashes fit")
        assert g.summary["hashes"] == 2 and g.summary["empty"] == 2 and g.summary["objects_counted"] == 1
    finally:
        tab.close()


def case_tile_edges(drv):
    """255, 256, 257 and 513 hashes, cut inside a tile and exactly on a tile
    edge, by max_length and by the capacity."""
    tab, hash_of = truncation_table(drv)
    try:
        ep = checked(tab)
        pattern = [101, 60, 103, 50, 107, 999, 102]
        for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            asked = [pattern[i % len(pattern)] for i in range(n)]
            asked[-1] = 104   # (the last hash has bytes)
            full = Want(ep[0], ep[1], hash_of, 1, asked)
            g, w = ask(tab, ep, hash_of, 1, asked, what=("whole", n))
            assert g.summary["hashes"] == n
            cuts = {100, n - 1} | {c for c in (TILE - 1, TILE, TILE + 1, 2 * TILE) if c < n}
            for c in sorted(cuts):
                # hash c is the first one dropped (its start differs from the one before it)
                while full.starts[c] == full.starts[c - 1]:
                    c -= 1
                g, w = ask(tab, ep, hash_of, 1, asked, max_length=full.starts[c] - 1, what=("cut", n, c))
                assert g.summary["hashes"] == c
                while full.ends[c] == full.ends[c - 1]:
                    c += 1
                g, w = ask(tab, ep, hash_of, 1, asked, capacity=full.ends[c] - 1, what=("capacity cut", n, c))
                assert g.summary["hashes"] == c
    finally:
        tab.close()


def case_repeats(drv):
    """One hash asked 1,000 times: every copy sends its objects again."""
    tab, hash_of = truncation_table(drv)
    try:
        ep = checked(tab)
        g, w = ask(tab, ep, hash_of, 1, [105] * 1000 + [60] * 3, what="repeats")
        assert g.summary["objects"] == 1009 and len(set(w.hash_bytes[:1000])) == 1
        assert g.summary["reply_bytes"] == 1000 * (12 + 3 + 2 + 35) + 3 * len(w.hash_bytes[-1])
        g, w = ask(tab, ep, hash_of, 1, [60] * 300, max_length=5000, what="repeats of three objects, cut")
        assert 0 < g.summary["hashes"] < 300 and g.summary["objects_counted"] == g.summary["objects"] + 3
    finally:
        tab.close()


def case_nullable_and_empty(drv):
    """n_hashes = 0, NULL d_parts, a reply of no capacity, two tables on one
    context."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    hot = drv.batch([[tc.head(2), rc.obj(1, b"x", 9, b"the other table's")]])
    tab, other = drv.table(64, 1), drv.table(64, 1)
    try:
        tab.add(b)
        other.add(hot)
        ep, ep_o = checked(tab), checked(other)
        g = call(tab, 1, [], 0, 0, HUGE)
        assert g.summary == ZERO_SUMMARY and g.reply == b""
        g = call(tab, 1, [], 16, 16, 0, want_parts=False)
        assert g.summary == ZERO_SUMMARY
        hx, hy = pc.key_hash(1, b"x"), pc.key_hash(1, b"y")
        base, _ = ask(tab, ep, key_hash, 1, [hx, hy, 5], what="parts given")
        g, _ = ask(tab, ep, key_hash, 1, [hx, hy, 5], what="no parts", want_parts=False)
        assert g.reply == base.reply and g.summary == base.summary
        assert base.summary["tombstones"] == 1 and base.summary["objects"] == 1 and base.summary["empty"] == 2
        o, wo = ask(other, ep_o, key_hash, 1, [hx], what="the other table")
        assert wo.objects == [(9, b"\1\1\0x" + b"the other table's")]
    finally:
        tab.close()
        other.close()


def batch_arrays(tab):
    """Every array of every added batch that the table reads, as bytes: the
    segments, the walk's tables, the hashes and the work array (d_work)."""
    if not tab.drv.on_device:
        return [a.tobytes() for keep in tab.t._keep if keep is not None for a in keep if a is not None]
    out = []
    for a in tab.added:
        for x in (a.w.d, a.w.d_status, a.w.d_entries, a.w.d_n, a.d_work, a.d_hash):
            if x is not None:
                out.append(x.cpu().numpy().tobytes())
    return out


def case_read_only(drv, mixed):
    """The batches' arrays and d_work are byte-identical before and after
    calls, and so is everything the table's words answer (stats, live lists,
    winners); a call between two adds answers the earlier state and changes no
    later answer."""
    tab = drv.table(1000, 4)
    try:
        tab.add(mixed[0])
        tab.add(mixed[1])
        ep2 = checked(tab)
        asked = table_hashes(lc.expectation(mixed), 1) + [77]
        before, arrays = tab.state(), batch_arrays(tab)
        assert len(arrays) >= 8
        a, _ = ask(tab, ep2, key_hash, 1, asked, what="first")
        b, _ = ask(tab, ep2, key_hash, 1, asked, what="second")
        ask(tab, ep2, key_hash, 1, asked, max_length=1000, what="truncated")
        assert batch_arrays(tab) == arrays, "the call wrote to a batch's array or to d_work"
        assert a.reply == b.reply and tab.state() == before
        tab.add(mixed[2])
        tab.add(mixed[3])
        ep4 = checked(tab)
        c, _ = ask(tab, ep4, key_hash, 1, asked, what="after two more adds")
        assert c.reply != a.reply
        fresh = drv.table(1000, 4)
        try:
            for m in mixed:
                fresh.add(m)
            assert fresh.state() == tab.state()
            d, _ = ask(fresh, ep4, key_hash, 1, asked, what="a table that was never asked")
            assert c.reply == d.reply
        finally:
            fresh.close()
    finally:
        tab.close()
