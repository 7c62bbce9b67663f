"""Cases and the expectation for a secondary index over the replay table
(ramcrc_replay_table_index_build_host / _device, ramcrc_index_lookup_host /
_device).

The expectation is plain Python, restated independently of the library: the
lookup expectation of lookup_cases.py (the sequential replay, held against the
live query's winners) gives every key's winner; an object winner of the table
id whose payload holds a non-empty key `index_id` inside its bounds gives the
entry (that key, the primary key's record hash); the entries are sorted with
Python's own bytes order -- unsigned bytes over the common length, then the
shorter key first -- and then by hash; a query is two bisections
(IndexletManager::lookupIndexKeys, src/IndexletManager.cc:654-706).  The tests
hold it against tests/golden/index_ref.json before any call is held against
it.
"""
import bisect
import ctypes
import os
import re
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
PAD = 64
MAXH = (1 << 64) - 1
ENTRY, QUERY, RESULT = segments.INDEX_ENTRY_DTYPE, segments.INDEX_QUERY_DTYPE, segments.INDEX_RESULT_DTYPE
BSUM, LSUM = segments.INDEX_BUILD_SUMMARY_DTYPE, segments.INDEX_LOOKUP_SUMMARY_DTYPE
OK, BAD, NOT_SERVED = segments.INDEX_OK, segments.INDEX_BAD_QUERY, segments.INDEX_NOT_SERVED
NONE = segments.READ_NONE
ZERO_BSUM = dict.fromkeys(BSUM.names, 0)
ZERO_LSUM = dict.fromkeys(LSUM.names, 0)


def source_constants():
    """kPartThreads and kIxTile, the sort tile's entry count, as the kernel
    sources state them."""
    out = rh.source_constants()
    csrc = os.path.join(os.path.dirname(os.path.abspath(segments.__file__)), "csrc")
    m = re.search(r"constexpr \w+ kIxTile = (\d+);", open(os.path.join(csrc, "dev_index.inc")).read())
    assert m
    out["kIxTile"] = int(m.group(1))
    return out


def key_hash(key):
    return pc.key_hash(key[0], key[1])


def sdict(s, names):
    return {k: int(s[k]) for k in names}


# ---------------------------------------------------------- the expectation
def secondary_key(pay, index_id):
    """Key `index_id` of an object's payload, or None: it has no such key, the
    key is empty, or its key table or keys run past the payload."""
    nk = pay[24]
    if nk <= index_id:
        return None
    keys = 25 + 2 * nk
    if keys > len(pay):
        return None
    cum = [int.from_bytes(pay[25 + 2 * i:27 + 2 * i], "little") for i in range(nk)]
    if keys + cum[-1] > len(pay):
        return None
    start = cum[index_id - 1] if index_id else 0
    end = cum[index_id]
    if end <= start or end > cum[-1]:
        return None
    return bytes(pay[keys + start:keys + end])


def key_compare(a, b):
    """IndexKey::keyCompare (src/IndexKey.cc:41-59) as the reference has it,
    the empty second key's rule included: the sign."""
    if not b:
        return -1
    m = min(len(a), len(b))
    if a[:m] != b[:m]:
        return -1 if a[:m] < b[:m] else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def prefix_of(key):
    return int.from_bytes(key[:8].ljust(8, b"\0"), "big")


class WantIndex:
    """What a build must give.  pairs: [(secondary key, pk hash)] unsorted."""

    def __init__(self, pairs, objects_seen, ecap=None, kcap=None):
        self.pairs = sorted(pairs)   # bytes order, then the hash
        need, kneed = len(pairs), sum(len(k) for k, _ in pairs)
        self.ecap = need if ecap is None else ecap
        self.kcap = kneed if kcap is None else kcap
        over = need > self.ecap or kneed > self.kcap
        self.summary = dict(ZERO_BSUM, entries_needed=need, key_bytes_needed=kneed, objects_seen=objects_seen,
                            overflow=int(over), n_entries=0 if over else need, key_bytes=0 if over else kneed)
        if over:
            self.pairs = []
        self.entries = [(prefix_of(k), h, k, len(k), 0) for k, h in self.pairs]
        self.hashes = [h for _, h in self.pairs]


def index_pairs(ep, hash_of, table_id, index_id):
    """([(secondary key, pk hash)], objects seen) from the lookup expectation
    and the winners' payloads."""
    exp, pays = ep
    pairs, seen = [], 0
    for key, res in exp.items():
        if key[0] != table_id or res[3] != lc.OBJECT:
            continue
        seen += 1
        k = secondary_key(pays[key], index_id)
        if k is not None:
            pairs.append((k, hash_of(key)))
    return pairs, seen


def expect_lookup(pairs, ranges, out_capacity=None, bad=(), dead=False):
    """What a lookup over the sorted `pairs` must give: ([(status, [hashes],
    next key or None, next hash)], summary)."""
    keys = [k for k, _ in pairs]
    reply, sm, open_, at = [], dict(ZERO_LSUM, n_entries=0 if dead else len(pairs), overflow_index=int(dead)), not dead, 0
    for i, (first, last, fah, mx) in enumerate(ranges):
        if not open_:
            reply.append((NOT_SERVED, [], None, 0))
            continue
        if i in bad:
            reply.append((BAD, [], None, 0))
            sm["served"] += 1
            sm["bad"] += 1
            continue
        lo = bisect.bisect_left(pairs, (bytes(first), fah))
        hi = bisect.bisect_right(keys, bytes(last)) if last else len(pairs)
        cnt = max(hi - lo, 0)
        num = min(cnt, mx)
        if out_capacity is not None and at + num > out_capacity:
            open_ = False
            reply.append((NOT_SERVED, [], None, 0))
            continue
        nxt = pairs[lo + num] if cnt > mx else (None, 0)
        reply.append((OK, [h for _, h in pairs[lo:lo + num]], nxt[0], nxt[1]))
        at += num
        sm["served"] += 1
        sm["hashes"] += num
        sm["maxed_out"] += cnt > mx
    return reply, sm


# ------------------------------------------------------------------ drivers
class HostDriver(cl.HostDriver):
    pass


class DeviceDriver(cl.DeviceDriver):
    pass


def normalized(entries, keys):
    """Entries with key_off dereferenced: (prefix, pk_hash, key bytes, key_len,
    reserved)."""
    out = []
    for e in entries:
        o, ln = int(e["key_off"]), int(e["key_len"])
        out.append((int(e["prefix"]), int(e["pk_hash"]), keys[o:o + ln].tobytes(), ln, int(e["reserved"])))
    return out


class Built:
    """One build's outputs as numpy: summary, entries (normalized), hashes, the
    raw arrays cut to what was written (raw_entries, raw_hashes, raw_keys); on
    the device also `index`, the ramcrc.Index of the tensors."""


def _finish_build(g):
    s = g.summary
    n, kb = s["n_entries"], s["key_bytes"]
    assert (g.entries_all[32 * n:] == FILL).all(), "a byte past the entries was written"
    assert (g.hashes_all[8 * n:] == FILL).all(), "a byte past the hashes was written"
    assert (g.keys_all[kb:] == FILL).all(), "a byte at or past key_bytes was written"
    assert (g.summary_past == FILL).all(), "a byte past the summary was written"
    g.raw_entries = g.entries_all[:32 * n].copy().view(ENTRY)
    g.raw_hashes = g.hashes_all[:8 * n].copy().view(np.uint64)
    g.raw_keys = g.keys_all[:kb].copy()
    g.entries = normalized(g.raw_entries, g.raw_keys)
    g.hashes = [int(h) for h in g.raw_hashes]
    # the keys lie back to back from 0
    spans = sorted((int(e["key_off"]), int(e["key_len"])) for e in g.raw_entries)
    at = 0
    for o, ln in spans:
        assert o == at, "the keys do not lie back to back"
        at += ln
    assert at == kb
    return g


def host_build_raw(R, t, table_id, index_id, ecap, kcap, null=False):
    """ramcrc_replay_table_index_build_host on buffers pre-filled with 0xA5 at
    odd addresses (no alignment rule).  Returns (code, Built)."""
    g = Built()
    g.entries_all = np.full(32 * ecap + PAD + 1, FILL, np.uint8)[1:]
    g.hashes_all = np.full(8 * ecap + PAD + 1, FILL, np.uint8)[1:]
    g.keys_all = np.full(kcap + PAD + 1, FILL, np.uint8)[1:]
    sm = np.full(BSUM.itemsize + PAD + 1, FILL, np.uint8)[1:]
    p = lambda x: None if null else ctypes.c_void_p(x.ctypes.data)
    code = R.lib().ramcrc_replay_table_index_build_host(t._h, int(table_id), int(index_id), p(g.entries_all), int(ecap),
                                                        p(g.hashes_all), p(g.keys_all), int(kcap),
                                                        ctypes.c_void_p(sm.ctypes.data))
    g.summary = sdict(sm[:BSUM.itemsize].copy().view(BSUM)[0], BSUM.names)
    g.summary_past = sm[BSUM.itemsize:]
    return code, g


def host_build(R, t, table_id, index_id, ecap, kcap, null=False):
    code, g = host_build_raw(R, t, table_id, index_id, ecap, kcap, null)
    assert code == 0, code
    return _finish_build(g)


class DevBuilt(Built):
    """One ramcrc_replay_table_index_build_device call: every output pre-filled
    with 0xA5 and longer than the call may write.  Read back after check()."""

    def __init__(self, ctx, t, table_id, index_id, ecap, kcap, null=False, check=True):
        import torch
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        self.d_entries, self.d_hashes = fill(32 * ecap + PAD), fill(8 * ecap + PAD).view(torch.int64)
        self.d_keys, self.d_sum = fill(kcap + PAD), fill(BSUM.itemsize + PAD).view(torch.int64)
        n = None if null else 1
        self.index = t.index_build(table_id, index_id, n and self.d_entries, n and self.d_hashes, n and self.d_keys,
                                   self.d_sum, entry_capacity=ecap, keys_capacity=kcap)
        self.index.entries, self.index.hashes, self.index.index_keys = self.d_entries, self.d_hashes, self.d_keys
        if check:
            ctx.check()
            self.read()

    def read(self):
        sm = self.d_sum.cpu().numpy().view(np.uint8)
        self.summary = sdict(sm[:BSUM.itemsize].view(BSUM)[0], BSUM.names)
        self.summary_past = sm[BSUM.itemsize:]
        self.entries_all = self.d_entries.cpu().numpy()
        self.hashes_all = self.d_hashes.cpu().numpy().view(np.uint8)
        self.keys_all = self.d_keys.cpu().numpy()
        return _finish_build(self)


def build_call(tab, table_id, index_id, ecap, kcap, null=False):
    """The build on `tab` (a driver's table); on the device it is also held
    against the host twin's: the same summary, the same entries with key_off
    dereferenced, the same hashes."""
    R = tab.drv.ramcrc
    if not tab.drv.on_device:
        return host_build(R, tab.t, table_id, index_id, ecap, kcap, null)
    g = DevBuilt(tab.drv.ctx, tab.t, table_id, index_id, ecap, kcap, null)
    h = host_build(R, tab.twin, table_id, index_id, ecap, kcap, null)
    assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
    assert h.entries == g.entries, ("host and device entries differ", first_diff(h.entries, g.entries))
    assert h.hashes == g.hashes, "host and device hashes differ"
    return g


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return len(a), len(b)


def build(tab, want, table_id, index_id, what=""):
    """The sizing call, then the build at want's capacities, against `want`."""
    g0 = build_call(tab, table_id, index_id, 0, 0, null=True)
    need = dict(want.summary, n_entries=0, key_bytes=0,
                overflow=int(want.summary["entries_needed"] > 0 or want.summary["key_bytes_needed"] > 0))
    assert g0.summary == need, (what, "the sizing call", g0.summary, need)
    g = build_call(tab, table_id, index_id, want.ecap, want.kcap)
    assert g.summary == want.summary, (what, g.summary, want.summary)
    assert g.entries == want.entries, (what, "entries", first_diff(g.entries, want.entries))
    assert g.hashes == want.hashes, (what, "hashes")
    return g


class Reply:
    """One lookup's outputs: reply [(status, [hashes], next key or None, next
    hash)], summary, and the raw arrays."""


def _finish_lookup(g, n, built):
    s = g.summary
    assert (g.out_all[8 * s["hashes"]:] == FILL).all(), "a word at or past `hashes` was written"
    assert (g.results_all[48 * n:] == FILL).all(), "a byte past the results was written"
    assert (g.summary_past == FILL).all(), "a byte past the summary was written"
    g.results = g.results_all[:48 * n].copy().view(RESULT)
    g.out = g.out_all[:8 * s["hashes"]].copy().view(np.uint64)
    g.reply = []
    for r in g.results:
        assert int(r["reserved"]) == 0
        if int(r["status"]) != OK:
            assert tuple(int(x) for x in r) == (NONE, 0, 0, 0, 0, 0, int(r["status"]), 0)
    for st, hs, nxt, nh in segments.index_lookup_hashes(g.out, g.results, built.raw_keys):
        g.reply.append((st, [int(h) for h in hs], nxt, nh))
    for r, rep in zip(g.results, g.reply):
        if rep[2] is not None:
            e = built.raw_entries[int(r["next_entry"])]
            assert (int(e["pk_hash"]), int(e["key_off"]), int(e["key_len"])) == (
                int(r["next_key_hash"]), int(r["next_key_off"]), int(r["next_key_len"]))
        elif int(r["status"]) == OK:
            assert (int(r["next_entry"]), int(r["next_key_hash"]), int(r["next_key_off"])) == (0, 0, 0)
    return g


def host_lookup(R, built, kb, q, ocap, summary_raw=None):
    """ramcrc_index_lookup_host over built's raw arrays, on buffers pre-filled
    with 0xA5 at odd addresses."""
    n = q.shape[0]
    g = Reply()
    g.out_all = np.full(8 * ocap + PAD + 1, FILL, np.uint8)[1:]
    g.results_all = np.full(48 * n + PAD + 1, FILL, np.uint8)[1:]
    sm = np.full(LSUM.itemsize + PAD + 1, FILL, np.uint8)[1:]
    odd = lambda a: np.concatenate([np.zeros(1, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])[1:]
    bs = np.zeros(1, BSUM)
    for k, v in built.summary.items():
        bs[0][k] = v
    arrs = [odd(built.raw_entries), odd(built.raw_hashes), odd(built.raw_keys), odd(bs), odd(kb), odd(q)]
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x.size else None
    code = R.lib().ramcrc_index_lookup_host(p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), p(arrs[4]), kb.size,
                                            p(arrs[5]), n, p(g.out_all) if ocap else None, int(ocap),
                                            p(g.results_all) if n else None, p(sm))
    assert code == 0, code
    g.summary = sdict(sm[:LSUM.itemsize].copy().view(LSUM)[0], LSUM.names)
    g.summary_past = sm[LSUM.itemsize:]
    return _finish_lookup(g, n, built)


class DevReply(Reply):
    """One ramcrc_index_lookup_device call over a DevBuilt's tensors."""

    def __init__(self, ctx, built, kb, q, ocap, check=True):
        import torch
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        self.n = n = q.shape[0]
        self.built = built
        self.d_qkeys = torch.from_numpy(np.ascontiguousarray(kb)).cuda() if kb.size else None
        raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1)
        self.d_q = torch.from_numpy(raw.copy()).cuda().view(torch.int64) if n else None
        self.d_out = fill(8 * ocap + PAD).view(torch.int64)
        self.d_res = fill(48 * n + PAD).view(torch.int64)
        self.d_sum = fill(LSUM.itemsize + PAD).view(torch.int64)
        ctx.index_lookup(built.index, self.d_qkeys, self.d_q, self.d_out, self.d_res, self.d_sum, qkeys_bytes=kb.size,
                         n_queries=n, out_capacity=ocap)
        if check:
            ctx.check()
            self.read()

    def read(self):
        sm = self.d_sum.cpu().numpy().view(np.uint8)
        self.summary = sdict(sm[:LSUM.itemsize].view(LSUM)[0], LSUM.names)
        self.summary_past = sm[LSUM.itemsize:]
        self.out_all = self.d_out.cpu().numpy().view(np.uint8)
        self.results_all = self.d_res.cpu().numpy().view(np.uint8)
        return _finish_lookup(self, self.n, self.built)


def lookup_raw(drv, built, kb, q, ocap):
    """The lookup over a build; on the device it is also held byte for byte
    against the host form over the same index."""
    if not drv.on_device:
        return host_lookup(drv.ramcrc, built, kb, q, ocap)
    g = DevReply(drv.ctx, built, kb, q, ocap)
    h = host_lookup(drv.ramcrc, built, kb, q, ocap)
    assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
    assert lc.same(h.results, g.results), "host and device results differ"
    assert lc.same(h.out, g.out), "host and device hashes differ"
    return g


def lookup(drv, built, pairs, ranges, out_capacity=None, what="", align=1, dead=False):
    """The lookup of `ranges` against the expectation over the sorted pairs."""
    kb, q = segments.index_queries(ranges, align)
    want, sm = expect_lookup(sorted(pairs), ranges, out_capacity, dead=dead)
    ocap = sm["hashes"] + 3 if out_capacity is None else out_capacity
    g = lookup_raw(drv, built, kb, q, ocap)
    assert g.summary == sm, (what, g.summary, sm)
    assert g.reply == want, (what, first_diff(g.reply, want))
    return g


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("index_ref.json")


def check_expectation_against_golden(ref):
    """key_compare against every pair of the reference's test, and the
    expectation's lookup against every query of its scenarios; returns how many
    scenarios."""
    for c in ref["key_compare"]:
        assert key_compare(c["a"].encode(), c["b"].encode()) == c["sign"], c
        if c["a"] and c["b"]:   # for non-empty keys it is Python's bytes order
            a, b = c["a"].encode(), c["b"].encode()
            assert ((a > b) - (a < b)) == c["sign"], c
    for sc in ref["scenarios"]:
        pairs = sorted((e["key"].encode(), e["hash"]) for e in sc["entries"])
        for qy in sc["queries"]:
            reply, sm = expect_lookup(pairs, [golden_range(qy)])
            check_golden_reply(reply[0], qy, sc["name"])
    return len(ref["scenarios"])


def golden_range(qy):
    return (qy["first"].encode(), qy["last"].encode(), qy["first_allowed_hash"], qy["max_hashes"])


def check_golden_reply(rep, qy, what):
    st, hashes, nxt, nh = rep
    assert st == OK and hashes == qy["hashes"], (what, rep, qy)
    if qy["next_key_length"] is not None:
        assert nxt == qy["next_key"].encode() and len(nxt) == qy["next_key_length"] and nh == qy["next_key_hash"], what
    else:
        assert len(hashes) < qy["max_hashes"] and nxt is None and nh == 0, what


def hashed_table(drv, key_cap, objects, adds=1):
    """A table of two-key objects added with given hashes.  objects: (table id,
    secondary key, pk hash); the primary keys are made up.  Returns the
    table."""
    lists = [[tc.head(1 + j)] for j in range(adds)]
    hs = [[0] for _ in range(adds)]
    for n, (tid, sk, h) in enumerate(objects):
        j = n % adds
        lists[j].append(lc.multi_obj(tid, [b"pk %d" % n, sk], b"v%d" % n, 1))
        hs[j].append(h)
    tab = drv.table(key_cap, adds)
    cap = max(64 * KiB, 2 * max(sum(len(e) for e in ls) for ls in lists))
    cap += -cap % 16
    for ls, h in zip(lists, hs):
        tab.add(drv.batch([ls], cap=cap), np.array(h, np.uint64))
    return tab


def case_goldens(drv):
    """Every golden scenario, realised as objects whose batch is added with
    the scenario's hashes."""
    ref = golden()
    assert check_expectation_against_golden(ref) == 8
    tid, iid = ref["table_id"], ref["index_id"]
    for sc in ref["scenarios"]:
        pairs = [(e["key"].encode(), e["hash"]) for e in sc["entries"]]
        tab = hashed_table(drv, 64, [(tid, k, h) for k, h in pairs])
        try:
            b = build(tab, WantIndex(pairs, len(pairs)), tid, iid, what=sc["name"])
            ranges = [golden_range(qy) for qy in sc["queries"]]
            g = lookup(drv, b, pairs, ranges, what=sc["name"])
            for rep, qy in zip(g.reply, sc["queries"]):
                check_golden_reply(rep, qy, sc["name"])
        finally:
            tab.close()


# ---------------------------------------------------------------- scenarios
def sort_objects(n):
    """3n objects whose slot is their number (hash & mask): table 1's keys
    arrive ascending, table 2's descending, table 3's all equal with the hashes
    descending."""
    objs = []
    for i in range(n):
        objs.append((1, b"key %08d" % i, 3 * i))
        objs.append((2, b"key %08d" % (n - i), (i << 40) | (3 * i + 1)))
        objs.append((3, b"the one key", ((n - i) << 40) | (3 * i + 2)))
    return objs


def case_sort(drv, n, extra=0):
    """n entries a table id (see sort_objects), built at entry_capacity n +
    extra."""
    objs = sort_objects(n)
    tab = hashed_table(drv, max(64, 3 * n), objs)
    try:
        for tid in (1, 2, 3):
            pairs = [(sk, h) for t, sk, h in objs if t == tid]
            w = WantIndex(pairs, n, ecap=n + extra, kcap=sum(len(k) for k, _ in pairs) + extra)
            b = build(tab, w, tid, 1, what=("sort", n, tid))
            if n:
                ranges = [(pairs[0][0], pairs[-1][0], 0, 5), (b"", b"", 0, n), (w.pairs[n // 2][0], b"", w.pairs[n // 2][1], 3)]
                lookup(drv, b, pairs, ranges, what=("sort lookup", n, tid))
    finally:
        tab.close()


def comparator_keys():
    body = bytes(range(65, 65 + 26)) * 12
    keys = [body[:n] for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 300)]
    keys += [b"ABCDEFGHx", b"ABCDEFGHy", body[:299] + b"\x00", body[:299] + b"\xff"]   # differ at byte 9 / the last
    keys += [b"pre", b"prefix", b"prefix-of-another", b"prefix-of-another-key"]           # prefixes, below and above 8
    for c in (0x00, 0x7f, 0x80, 0xff):
        keys += [bytes([c]), bytes([c]) + b"tail", b"12345678" + bytes([c]), b"12345678" + bytes([c]) + b"z"]
    keys += [b"1234567", b"12345678", b"1234567\x00", b"\x00\x00"]   # zero padding against a real 0x00
    return keys


def case_comparator(drv):
    """Every key of comparator_keys once, some twice with distinct hashes
    (two that differ only in bit 63), and two entries equal in key and hash."""
    keys = comparator_keys()
    objs = [(1, k, 0x1000 + 7 * n) for n, k in enumerate(keys)]
    objs += [(1, b"ABCDEFGHx", 5), (1, b"ABCDEFGHx", 5 | (1 << 63)), (1, b"pre", MAXH), (1, b"pre", 0)]
    objs += [(1, b"twice the same", 77), (1, b"twice the same", 77)]
    tab = hashed_table(drv, 256, objs, adds=2)
    try:
        pairs = [(k, h) for _, k, h in objs]
        b = build(tab, WantIndex(pairs, len(pairs)), 1, 1, what="comparator")
        ranges = [(k, k, 0, 100) for k in sorted(set(keys))]
        ranges += [(b"ABCDEFGH", b"ABCDEFGHz", 0, 100), (b"\x7f", b"\x80", 0, 100), (b"12345678", b"12345678\xff", 0, 100),
                   (b"pre", b"pre", 1, 100), (b"ABCDEFGHx", b"ABCDEFGHx", 1 << 63, 100)]
        lookup(drv, b, pairs, ranges, what="comparator lookups")
        for al in (1, 8, 16):
            lookup(drv, b, pairs, ranges[:9], what=("aligned", al), align=al)
    finally:
        tab.close()


def selection_lists():
    """lc.multi_key_lists() (table 5: one, two and three keys, a broken key
    table; table 6: no key) and table 7: an empty secondary key between two
    others, an overwritten object whose newer version has another key, a
    tombstone winner, an object after its tombstone."""
    lists, _ = lc.multi_key_lists()
    a = lists[0] + [
        lc.multi_obj(7, [b"gap", b"before", b"", b"after"], b"v", 1),
        lc.multi_obj(7, [b"moved", b"old place"], b"v", 1),
        lc.multi_obj(7, [b"dead", b"buried"], b"v", 1),
        lc.multi_obj(7, [b"back", b"first life"], b"v", 1),
        lc.multi_obj(7, [b"shrinks", b"ab", b"c"], b"v", 1, cum=[7, 9, 8]),
        lc.multi_obj((7 << 32) + 7, [b"gap", b"another table"], b"v", 1)]
    b = [tc.head(2), lc.multi_obj(7, [b"moved", b"new place", b"and a third"], b"w", 2), rc.tomb(7, b"dead", 1),
         rc.tomb(7, b"back", 1), lc.multi_obj(7, [b"back", b"second life"], b"w", 2)]
    return [a], [b]


def case_selection(drv):
    tab = drv.table(64, 2)
    try:
        for ls in selection_lists():
            tab.add(drv.batch(ls))
        ep = rd.checked(tab)
        seen = {}
        for tid in (5, 6, 7, (7 << 32) + 7, 99):
            for iid in (1, 2, 3, 4, 300):
                pairs, n = index_pairs(ep, key_hash, tid, iid)
                b = build(tab, WantIndex(pairs, n), tid, iid, what=("selection", tid, iid))
                seen[(tid, iid)] = sorted(k for k, _ in pairs)
                lookup(tab.drv, b, pairs, [(b"", b"", 0, 100)], what=("selection", tid, iid))
        assert seen[(5, 1)] == [b"second key"] * 6 and seen[(5, 2)] == [b"3rd"] * 3 and seen[(5, 3)] == []
        assert seen[(6, 1)] == [] and seen[(99, 1)] == []
        assert seen[(7, 1)] == [b"before", b"new place", b"second life"]
        assert seen[(7, 2)] == [b"and a third"] and seen[(7, 3)] == [b"after"]
        assert seen[((7 << 32) + 7, 1)] == [b"another table"]
    finally:
        tab.close()


def case_capacity(drv):
    """entry_capacity and keys_capacity one short: overflow and nothing
    written; exactly enough: the index."""
    objs = [(1, b"k%d" % i * (1 + i % 4), 100 + i) for i in range(40)]
    tab = hashed_table(drv, 64, objs)
    try:
        pairs = [(k, h) for _, k, h in objs]
        kb = sum(len(k) for k, _ in pairs)
        for ecap, kcap in ((39, kb), (40, kb - 1), (0, kb), (40, 0), (39, kb - 1)):
            w = WantIndex(pairs, 40, ecap=ecap, kcap=kcap)
            g = build_call(tab, 1, 1, ecap, kcap)
            assert g.summary == w.summary and g.summary["overflow"] == 1 and g.entries == [], (ecap, kcap, g.summary)
            lookup(tab.drv, g, [], [(b"", b"", 0, 10), (b"k1", b"k1", 0, 10)], what="an overflowed build", dead=True)
        build(tab, WantIndex(pairs, 40), 1, 1, what="exactly enough")
        build(tab, WantIndex(pairs, 40, ecap=41, kcap=kb + 1), 1, 1, what="one more")
    finally:
        tab.close()


def lookup_table(drv):
    """Runs of equal keys with several hashes among single keys."""
    objs = []
    for i in range(30):
        objs.append((1, b"single %02d" % i, 1000 + i))
    for h in (10, 20, 30, 40):
        objs.append((1, b"run", h))
    for h in (5, 6):
        objs.append((1, b"single 10", h))
    return objs


def case_lookup(drv):
    objs = lookup_table(drv)
    tab = hashed_table(drv, 64, objs)
    try:
        pairs = [(k, h) for _, k, h in objs]
        b = build(tab, WantIndex(pairs, len(pairs)), 1, 1, what="lookup table")
        n = len(pairs)
        run = [(b"run", b"run", fah, 100) for fah in (0, 9, 10, 11, 25, 40, 41, MAXH)]
        lookup(drv, b, pairs, run, what="first_allowed_hash around a run")
        edges = [(b"", b"", 0, 100), (b"", b"run", 0, 100), (b"run", b"", 0, 100), (b"single 20", b"single 10", 0, 100),
                 (b"zzz", b"", 0, 100), (b"", b"\x00", 0, 100), (b"", b"", MAXH, 100)]
        lookup(drv, b, pairs, edges, what="empty keys, first above last")
        whole = (b"single 00", b"single 29", 0)
        maxes = [whole + (m,) for m in (0, 1, 32, 31, 33)] + [(b"run", b"run", 0, m) for m in (0, 1, 3, 4, 5)]
        g = lookup(drv, b, pairs, maxes, what="max_hashes")
        assert g.summary["maxed_out"] == 6 and n == 36
        lookup(drv, b, pairs, run[:3] * 3 + maxes + run[:3], what="repeats")
        # out_capacity cutting at every boundary of a small batch, and inside
        small = [(b"run", b"run", 0, 100), (b"nothing here", b"nothing here", 0, 100), whole + (5,), (b"", b"", 0, 2)]
        _, sm = expect_lookup(sorted(pairs), small)
        for cap in range(sm["hashes"] + 2):
            lookup(drv, b, pairs, small, out_capacity=cap, what=("out_capacity", cap))
        lookup(drv, b, pairs, [], what="no queries")
        # bad queries among good ones
        ranges = [(b"run", b"run", 0, 100), (b"single 03", b"single 05", 0, 100)] * 3
        kb, q = segments.index_queries(ranges)
        q["first_off"][1] = kb.size + 1
        q["last_len"][2] = 65536
        q["reserved"][3] = 1
        q["last_off"][4] = kb.size - 2   # its 3 or 9 bytes end past the buffer
        bad = {1, 2, 3, 4}
        want, sm = expect_lookup(sorted(pairs), ranges, bad=bad)
        g = lookup_raw(drv, b, kb, q, sm["hashes"] + 1)
        assert g.summary == sm and g.reply == want and sm["bad"] == 4
        want, sm = expect_lookup(sorted(pairs), ranges, out_capacity=5, bad=bad)
        g = lookup_raw(drv, b, kb, q, 5)
        assert g.summary == sm and g.reply == want and sm["served"] == 5
        # many queries: more than a tile, more than a step of the scan's tiles
        T = source_constants()["kPartThreads"]
        many = [(b"single %02d" % (i % 30), b"single %02d" % (i % 30 + i % 3), 0, 1 + i % 4) for i in range(2 * T + 3)]
        _, sm = expect_lookup(sorted(pairs), many)
        for cap in (None, sm["hashes"] // 2, 1):
            lookup(drv, b, pairs, many, out_capacity=cap, what=("many", cap))
    finally:
        tab.close()


def case_long_runs(drv):
    """A range longer than the workgroup's threshold for a long run."""
    T = source_constants()["kPartThreads"]
    objs = [(1, b"long run", 10 + i) for i in range(2 * T + 5)] + [(1, b"m", 1), (1, b"a", 2)]
    tab = hashed_table(drv, 1024, objs)
    try:
        pairs = [(k, h) for _, k, h in objs]
        b = build(tab, WantIndex(pairs, len(pairs)), 1, 1, what="long runs")
        ranges = [(b"", b"", 0, 10000), (b"long run", b"long run", 0, T), (b"long run", b"long run", 0, T - 1),
                  (b"long run", b"long run", 10 + T, 10000), (b"a", b"a", 0, 1)]
        lookup(drv, b, pairs, ranges, what="long runs")
    finally:
        tab.close()


def random_lists(rng, nbatches, nkeys):
    """Batches over one pool of primary keys of tables 1 and 2: two- and
    three-key objects of growing versions whose secondary keys come from a
    small pool (overwrites move a key), and tombstones."""
    pool = [(1 + (i % 7 == 0), b"key %d" % i) for i in range(nkeys)]
    second = [b"s%02d" % i * (1 + i % 5) for i in range(max(4, nkeys // 3))]
    version, lists = {}, []
    for j in range(nbatches):
        es = [tc.head(1 + j)]
        for i in rng.choice(nkeys, size=max(1, nkeys * 2 // 3), replace=False):
            tid, key = pool[int(i)]
            v = version.get((tid, key), 0) + 1
            version[(tid, key)] = v
            if rng.random() < 0.2 and j:
                es.append(rc.tomb(tid, key, v))
            else:
                ks = [key] + [second[int(rng.integers(len(second)))] for _ in range(int(rng.integers(0, 3)))]
                es.append(lc.multi_obj(tid, ks, bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)), v))
        lists.append(es)
    return lists


def case_chain(drv, seed):
    """Build, then lookup, then read_hashes of the returned hashes: the objects
    returned are exactly the live objects of the table id whose key index_id
    lies in the range, held against a plain filter over the expectation's
    winners.  Before and after a clean; the index built before the clean still
    answers from its own key copy afterwards."""
    rng = np.random.default_rng(seed)
    key_cap = [40, 129, 700][seed % 3]
    lists = random_lists(rng, 4, key_cap * 3 // 4)
    tab, model = drv.table(key_cap, len(lists) + 3), cl.Model()
    try:
        for es in lists:
            cl.add(tab, model, drv.batch([es], cap=256 * KiB))
        old = None
        for round_ in ("before the clean", "after the clean"):
            ep = (model.results(), model.payloads())
            for tid, iid in ((1, 1), (1, 2), (2, 1)):
                pairs, seen = index_pairs(ep, key_hash, tid, iid)
                b = build(tab, WantIndex(pairs, seen), tid, iid, what=("chain", seed, round_, tid, iid))
                sk = sorted({k for k, _ in pairs})
                lo, hi = (sk[len(sk) // 4], sk[-1 - len(sk) // 4]) if sk else (b"a", b"b")
                ranges = [(lo, hi, 0, 10000), (b"", b"", 0, 10000), (lo, lo, 0, 10000)]
                g = lookup(drv, b, pairs, ranges, what=("chain lookup", seed, round_))
                for (first, last, _, _), rep in zip(ranges, g.reply):
                    want_keys = {k for k, r in ep[0].items() if k[0] == tid and r[3] == lc.OBJECT and
                                 in_range(secondary_key(ep[1][k], iid), first, last)}
                    asked = rep[1]
                    _, w = rh.ask(tab, ep, key_hash, tid, asked, what=("chain read_hashes", seed, round_))
                    got = [data for _, data in w.objects]
                    assert sorted(got) == sorted(ep[1][k][24:] for k in want_keys), (seed, round_, tid, iid)
                if (tid, iid) == (1, 1) and round_ == "before the clean":
                    old = (b, pairs, ranges, g.reply)
            if round_ == "before the clean":
                cl.clean(tab, model, drv, [0, 2], key_cap, what="index", more=False, ties=True)
            else:
                b, pairs, ranges, reply = old
                assert lookup(drv, b, pairs, ranges, what="the old index after the clean").reply == reply
    finally:
        tab.close()


def in_range(k, first, last):
    return k is not None and k >= first and (not last or k <= last)


def case_read_only(drv, mixed):
    """The batches' arrays and d_work are byte-identical before and after
    builds, and so is everything the table's words answer."""
    tab = drv.table(1000, 4)
    try:
        for m in mixed[:2]:
            tab.add(m)
        tab.add(drv.batch(selection_lists()[0]))
        ep = rd.checked(tab)
        before, arrays = tab.state(), rh.batch_arrays(tab)
        for tid, iid in ((7, 1), (5, 1), (1, 1), (7, 2)):
            pairs, seen = index_pairs(ep, key_hash, tid, iid)
            build(tab, WantIndex(pairs, seen), tid, iid, what=("read-only", tid, iid))
        assert rh.batch_arrays(tab) == arrays, "the build wrote to a batch's array or to d_work"
        assert tab.state() == before
        lc.lookup(tab, ep[0], sorted(ep[0]), what="lookups after the builds")
    finally:
        tab.close()
