"""Batches, cases and the expectation for the replay table tests
(ramcrc_replay_table_* on the host and on the device).

The expectation is the defining property of include/ramcrc.h: concatenate the
added batches' record tables in add order (segment numbers offset by the
earlier batches' n_seg), take ramcrc_replay_resolve_host's answer for that
one table -- itself held against resolve_cases.expected, the plain-Python
sequential replay -- and map every global record index back to {batch,
record}.  Every batch of a test has the same segment stride.
"""
import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc
import resolve_cases as rc

KiB = 1024
MiB = 1 << 20
FILL = rc.FILL
FILL32 = 0xA5A5A5A5
NONE = segments.RESOLVE_NONE
REF = segments.REPLAY_REF_DTYPE
STAT_NAMES = segments.REPLAY_TABLE_STATS_DTYPE.names
ALL = (1 << 64) - 1


class HostBatch:
    """One batch for the host form: the fields of append_cases.Walked the
    helpers below read."""

    def __init__(self, oracle, lists, cap, bad=()):
        self.buf, self.certs, self.status, self.table = rc.host_source(oracle, lists, cap, bad)
        self.cap, self.nseg = cap, len(lists)


# ---------------------------------------------------------- the expectation
def concat(batches):
    """(buf, cap, nseg, status, table, bounds): the batches as one walk;
    bounds[j] is the global index of batch j's record 0."""
    cap = batches[0].cap
    assert all(b.cap == cap for b in batches)
    tables, off = [], 0
    for b in batches:
        t = np.array(b.table, np.uint32).reshape(-1, 4)
        t[:, 0] += off
        off += b.nseg
        tables.append(t)
    bounds = np.cumsum([0] + [t.shape[0] for t in tables])
    return (np.concatenate([b.buf[:b.nseg * cap] for b in batches]), cap, off,
            np.concatenate([b.status[:b.nseg] for b in batches]), np.concatenate(tables), bounds)


def refs(winner, bounds):
    """Global winners as REPLAY_REF records."""
    out = np.zeros(winner.shape[0], REF)
    out["batch"] = out["record"] = NONE
    has = winner != NONE
    b = np.searchsorted(bounds, winner[has], "right") - 1
    out["batch"][has] = b
    out["record"][has] = winner[has] - bounds[b]
    return out


def expect(ramcrc, batches, hashes=None, python=True):
    """Per batch (winner REF [n], live uint32 [m, 2], counts dict) after the
    batches were added in this order.  hashes: per batch an array or None,
    all or none.  python: hold the one-call against the plain-Python replay
    too (slow for many records)."""
    buf, cap, nseg, status, table, bounds = concat(batches)
    h = None if hashes is None or hashes[0] is None else np.concatenate(
        [np.asarray(x, np.uint64)[:b.table.shape[0]] for x, b in zip(hashes, batches)])
    winner, _, _, counts = ramcrc.replay_resolve_host(buf, cap, nseg, status, table, key_hash=h)
    if python:
        e_winner, _, e_counts = rc.expected(buf, cap, table, status, h)
        assert np.array_equal(winner, e_winner) and rc.counts_dict(counts) == e_counts
    ref = refs(winner, bounds)
    out = []
    for j, b in enumerate(batches):
        lo, hi = int(bounds[j]), int(bounds[j + 1])
        w = winner[lo:hi]
        live = np.flatnonzero(w == np.arange(lo, hi, dtype=np.uint32)).astype(np.uint32)
        types = table[lo:hi, 3][live] & 0x3F
        _, _, _, own = ramcrc.replay_resolve_host(b.buf, cap, b.nseg, b.status, b.table)
        c = dict(objects=int(own["objects"]), tombstones=int(own["tombstones"]),
                 live_objects=int((types == rc.OBJ).sum()), live_tombstones=int((types == rc.OBJTOMB).sum()),
                 malformed=int(own["malformed"]), safe_version=int(counts["safe_version"]))
        out.append((ref[lo:hi], np.stack([live, np.zeros_like(live)], 1).reshape(-1, 2), c))
    return out


def table_stats(exp, n_batches=None):
    """The stats a table must report after the adds `exp` describes."""
    return dict(keys=sum(e[2]["live_objects"] + e[2]["live_tombstones"] for e in exp),
                live_objects=sum(e[2]["live_objects"] for e in exp),
                live_tombstones=sum(e[2]["live_tombstones"] for e in exp),
                safe_version=exp[0][2]["safe_version"] if exp else 0,
                batches=len(exp) if n_batches is None else n_batches, spoiled=0)


def stats_dict(s):
    return {k: int(s[k]) for k in STAT_NAMES}


SPOILED_STATS = dict(keys=0, live_objects=0, live_tombstones=0, safe_version=0, batches=0, spoiled=1)
ZERO_COUNTS = dict.fromkeys(rc.COUNT_NAMES, 0)


def survivors(batches, lives):
    """key -> (version, type) of the records the per-batch live lists keep."""
    out = {}
    for b, live in zip(batches, lives):
        parts = rc.participants(b.buf, b.cap, b.table, b.status)
        for rec in np.asarray(live).reshape(-1, 2)[:, 0].tolist():
            _, etype, key, ver = parts[rec]
            assert key not in out, "a key with two survivors"
            out[key] = (ver, etype)
    return out


def replayed(batches):
    """key -> (version, type) by the sequential replay of the concatenation."""
    buf, cap, _, status, table, _ = concat(batches)
    return {k: v[:2] for k, v in rc.replay(rc.participants(buf, cap, table, status)).items()}


# -------------------------------------------------------------------- cases
def head(seg_id=1):
    return pc.entry(pc.SEGHEADER, pc.seg_header(seg_id))


STALE_AT = 900   # the record of batch 0 that an equal object at record 3 of batch 1 must not replace


def relation_lists():
    """Three entry lists, a batch each.  Per key one record in each of two or
    three batches: the later record's version lower / equal / higher, all four
    type pairs, every pair of batches; a key that only batch 1 has; the stale
    pick (a tombstone of version 5 in batch 0, an object of version 7 in batch
    1) with its mirrors; an object of version 7 at record STALE_AT of batch 0
    against one at record 3 of batch 1; rc.WIDE versions across batches."""
    lists = [[head(20 + b)] for b in range(3)]
    # batch 1, records 1 .. 3: two fillers and the late equal object
    lists[1] += [rc.obj(1, b"only in batch 1", 4), rc.obj(1, b"filler", 1), rc.obj(9, b"same v7", 7)]
    n = 0
    for ta in (rc.OBJ, rc.OBJTOMB):
        for tb in (rc.OBJ, rc.OBJTOMB):
            for dv in (-1, 0, 1):
                for x, y in ((0, 1), (0, 2), (1, 2)):
                    key = b"pair %d" % n
                    lists[x].append(rc.record(ta, 2, key, 5, b"first"))
                    lists[y].append(rc.record(tb, 2, key, 5 + dv, b"second"))
                    n += 1
                for dv2 in (-1, 0, 1):
                    key = b"triple %d" % n
                    lists[0].append(rc.record(ta, 3, key, 5))
                    lists[1].append(rc.record(tb, 3, key, 5 + dv))
                    lists[2].append(rc.record(ta if dv2 else tb, 3, key, 5 + dv + dv2))
                    n += 1
    lists[0].append(rc.tomb(4, b"stale pick", 5))
    lists[1].append(rc.obj(4, b"stale pick", 7))
    lists[0].append(rc.obj(4, b"stale pick, mirrored", 5))
    lists[1].append(rc.tomb(4, b"stale pick, mirrored", 7))
    lists[0].append(rc.tomb(4, b"stale pick, late", 5))
    lists[2].append(rc.obj(4, b"stale pick, late", 7))
    lists[2].append(rc.tomb(4, b"stale pick, late", 7))
    lists[0].append(rc.obj(4, b"kept pick", 7))
    lists[1].append(rc.tomb(4, b"kept pick", 5))
    k = 0
    for a in rc.WIDE:
        for b in rc.WIDE:
            lists[0].append(rc.obj(5, b"oo%d" % k, a))
            lists[1].append(rc.obj(5, b"oo%d" % k, b))
            lists[1].append(rc.tomb(5, b"to%d" % k, a))
            lists[2].append(rc.obj(5, b"to%d" % k, b))
            k += 1
    assert len(lists[0]) < STALE_AT
    lists[0] += [rc.obj(6, b"pad %d" % i, 1) for i in range(STALE_AT - len(lists[0]))]
    lists[0].append(rc.obj(9, b"same v7", 7))
    assert sum(len(e) for e in lists[0]) < 60 * KiB
    return lists


def check_relations(batches, exp):
    """What relation_lists promises, read off the full expectation."""
    b0, b1 = batches[0], batches[1]
    assert exp[0][0][STALE_AT].tolist() == (0, STALE_AT) == exp[1][0][3].tolist()
    for b, e in zip(batches, exp):
        parts = rc.participants(b.buf, b.cap, b.table, b.status)
        for i, p in enumerate(parts):
            if p is None:
                continue
            wb, wr = e[0][i].tolist()
            if p[2] == (4, b"stale pick"):
                assert (wb, int(batches[wb].table[wr, 3]) & 0x3F) == (1, rc.OBJ)
            if p[2] == (4, b"stale pick, mirrored"):
                assert (wb, int(batches[wb].table[wr, 3]) & 0x3F) == (1, rc.OBJTOMB)
            if p[2] == (4, b"stale pick, late"):
                assert (wb, int(batches[wb].table[wr, 3]) & 0x3F) == (2, rc.OBJTOMB)
            if p[2] == (4, b"kept pick"):
                assert wb == 0
            if p[2] == (1, b"only in batch 1"):
                assert (wb, wr) == (1, i)
    assert b0.table.shape[0] == STALE_AT + 1 and b1.table.shape[0] > 3


def split_lists(entries, at=None):
    """One entry list (a SEGHEADER first) as two batches' lists."""
    at = len(entries) // 2 if at is None else at
    return [entries[:at]], [[head(2)] + entries[at:]]


def reference_lists(ref):
    """The fixture's cases, each case's records one per batch in the
    fixture's order: (lists per batch, per batch the case of every record)."""
    depth = max(len(c["records"]) for c in ref["cases"])
    lists = [[head(30 + k)] for k in range(depth)]
    which = [[None] for _ in range(depth)]
    for n, c in enumerate(ref["cases"]):
        for k, (t, key, ver) in enumerate(c["records"]):
            lists[k].append(rc.record(rc.OBJ if t == "OBJ" else rc.OBJTOMB, ref["table_id"],
                                      key.encode(), ver, b"some guy"))
            which[k].append(n)
    return lists, which


def check_reference(ref, which, exp, batches):
    for k, cases in enumerate(which):
        for i, n in enumerate(cases):
            if n is None:
                continue
            c = ref["cases"][n]
            sv = c["survivor"]
            wb, wr = exp[k][0][i].tolist()
            assert wb == sv["index"] and which[wb][wr] == n, c["name"]
            assert int(batches[wb].table[wr, 3]) & 0x3F == (rc.OBJ if sv["type"] == "OBJ" else rc.OBJTOMB)
    assert sum(e[1].shape[0] for e in exp) == len(ref["cases"])


def capacity_lists(nkeys):
    """One list: a SEGHEADER, then two records for each of nkeys keys."""
    es = [head(1)]
    for k in range(nkeys):
        es += [rc.obj(7, b"cap key %d" % k, 2), rc.tomb(7, b"cap key %d" % k, 1)]
    return es


# ------------------------------------------------------------- host driver
def host_add(t, b, hashes=None):
    return t.add(b.buf, b.cap, b.nseg, b.status, b.table, key_hash=hashes)


def check_host(t, exp, what=""):
    """Every batch's live() and the stats against the expectation; returns
    the answers."""
    got = []
    for j, (e_winner, e_live, e_counts) in enumerate(exp):
        winner, live, need, counts = t.live(j)
        assert np.array_equal(winner, e_winner), (what, j, "winners")
        assert need == e_live.shape[0] and np.array_equal(live, e_live), (what, j, "live list")
        assert rc.counts_dict(counts) == e_counts, (what, j, rc.counts_dict(counts), e_counts)
        got.append((winner, live, rc.counts_dict(counts)))
    assert stats_dict(t.stats()) == table_stats(exp), (what, stats_dict(t.stats()), table_stats(exp))
    return got


# ------------------------------------------------ device calls (GPU tests)
class Added:
    """One batch on the device: an append_cases.Walked with its work array
    (pre-filled with 0xA5) and, after add(), its number."""

    def __init__(self, w, hashes=None):
        import torch
        self.w = w
        ecap = w.d_entries.shape[0]
        self.d_work = torch.full((ecap * 8 + 32,), FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
        if isinstance(hashes, np.ndarray):
            h = np.zeros(ecap, np.uint64)
            h[:hashes.size] = hashes
            hashes = torch.from_numpy(h.view(np.int64)).cuda()
        self.d_hash = hashes
        self.batch = None

    def add(self, t):
        w = self.w
        self.batch = t.add(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, self.d_work,
                           key_hash=self.d_hash)
        return self.batch


class Live:
    """One ramcrc_replay_table_live_device call: every output pre-filled with
    0xA5 bytes, read back after check()."""

    def __init__(self, ctx, t, a, live_cap=None, check=True, want_winner=True):
        import torch
        ecap = a.w.d_entries.shape[0]
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.live_cap = ecap if live_cap is None else live_cap
        self.d_winner = fill((ecap + 4) * 8, torch.int32).view(-1, 2) if want_winner else None
        self.d_live = fill((self.live_cap + 4) * 8, torch.int32).view(-1, 2)
        self.d_n_live = fill(8, torch.int64)
        self.d_counts = fill(6 * 8, torch.int64)
        t.live(a.batch, self.d_live[:self.live_cap], self.d_n_live, self.d_counts, winner=self.d_winner)
        if check:
            ctx.check()
            self.read()

    def read(self):
        self.need = int(self.d_n_live.item())
        self.live_all = self.d_live.cpu().numpy().view(np.uint32)
        self.live = self.live_all[:min(self.need, self.live_cap)]
        self.winner_all = None if self.d_winner is None else \
            self.d_winner.cpu().numpy().view(np.uint32).reshape(-1, 2)
        self.counts = rc.counts_dict(self.d_counts.cpu().numpy().view(segments.RESOLVE_COUNTS_DTYPE)[0])


def device_stats(ctx, t):
    import torch
    d = torch.full((6 * 8 + 16,), FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    t.stats(d)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert (got[6:].view(np.uint32) == FILL32).all(), "a word past the stats was written"
    return stats_dict(got[:6].view(segments.REPLAY_TABLE_STATS_DTYPE)[0])


def check_device(ctx, t, added, exp, what="", live_cap=None, stats=True):
    """live() of every added batch against the expectation: winners, list and
    counters equal exactly; slots past the list's end and winner slots past
    the table keep their 0xA5 fill.  Returns the Live objects."""
    got = []
    for a, (e_winner, e_live, e_counts) in zip(added, exp):
        r = Live(ctx, t, a, live_cap)
        n = a.w.table.shape[0]
        cap = r.live_cap
        tag = (what, a.batch)
        assert r.need == e_live.shape[0], (tag, r.need, e_live.shape[0])
        assert np.array_equal(r.winner_all[:n].reshape(-1).view(REF), e_winner), (tag, "winners")
        assert (r.winner_all[n:] == FILL32).all(), (tag, "a winner slot past the table was written")
        assert np.array_equal(r.live, e_live[:cap]), (tag, "live list")
        assert (r.live_all[r.live.shape[0]:] == FILL32).all(), (tag, "a slot past the list was written")
        assert r.counts == e_counts, (tag, r.counts, e_counts)
        got.append(r)
    if stats:
        s = device_stats(ctx, t)
        assert s == table_stats(exp), (what, s, table_stats(exp))
    return got


class Concat:
    """The batches as one walk on the device, for the one-call resolve
    (resolve_cases.Resolved reads these fields)."""

    def __init__(self, ws):
        import torch
        self.buf, self.cap, self.nseg, self.status, self.table, _ = concat(ws)
        self.d = torch.from_numpy(self.buf).cuda()
        self.d_status = torch.from_numpy(self.status.view(np.int32)).cuda()
        self.d_entries = torch.zeros((self.table.shape[0] + 8, 4), dtype=torch.int32, device="cuda")
        self.d_entries[:self.table.shape[0]] = torch.from_numpy(self.table.view(np.int32)).cuda()
        self.d_n = torch.tensor([self.table.shape[0]], dtype=torch.int64, device="cuda")
