"""Scenarios for ramcrc_replay_table_migrate_device / _host (include/ramcrc.h),
run on the host by test_replay_table_migrate_host.py and on the GPU by
test_gpu_replay_table_migrate.py.

The expectation is the plain Python of Model.expect below: it walks the listed
batches in order from the cursor, classifies every record by the header's rule
2 over resolve_cases.participants and the clean model's winners, packs the sent
ones greedily and takes every certificate from the oracle.  It is held against
tests/golden/migrate_ref.json (what the reference's own tests state) before it
is used for anything else.  Every call's outputs start as 0xA5 bytes and are
checked at and past every head and past segments_used; the device driver feeds
a host table the same batches and compares every output with the host form's,
byte for byte."""
import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import clean_cases as cc
import lookup_cases as lc
import partition_cases as pc
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
FILL = 0xA5
PAD = 64
M64 = (1 << 64) - 1
SUMMARY = segments.MIGRATE_SUMMARY_DTYPE
COUNT = segments.MIGRATE_COUNT_DTYPE
NAMES = SUMMARY.names
OBJ, OBJTOMB = pc.OBJ, pc.OBJTOMB
ZERO = dict.fromkeys(NAMES, 0)
TILE = 256   # dev_migrate.inc: records per tile (kPartThreads)


def summary_dict(s):
    return {k: int(s[k]) for k in NAMES}


# ---------------------------------------------------------- the expectation
class Plain:
    def __init__(self, buf, cap, status, table, hashes=None):
        self.buf, self.cap, self.nseg = buf, cap, 1
        self.status, self.table, self.hashes = status, table, hashes


class Want:
    pass


class Model(cc.Model):
    """The clean model (key -> winner) with the hashes the batches were added
    with, and the migration by the header's rules."""

    def hashes_of(self, n):
        return getattr(self.batches[n], "hashes", None)

    def classes(self, n, table_id, first, last, live_only):
        """Per record of batch n: (class name, type, payload length, payload)."""
        b = self.batches[n]
        hs = self.hashes_of(n)
        out = []
        for r, p in enumerate(rc.participants(b.buf, b.cap, b.table, b.status)):
            seg, off, ln, hdr = (int(x) for x in b.table[r])
            if p is None or p[0] != "rec":
                out.append(("skipped_other", hdr & 0x3F, ln, None))
                continue
            _, etype, key, ver = p
            h = int(hs[r]) if hs is not None else pc.key_hash(key[0], key[1])
            if key[0] != table_id:
                k = "skipped_table"
            elif not first <= h <= last:
                k = "skipped_range"
            elif live_only and self.win[key][1][1:] != (n, r):
                k = "skipped_dead"
            else:
                k = "sent"
            at = seg * b.cap + off + 1 + ((hdr >> 6) & 3) + 1
            out.append((k, etype, ln, b.buf[at:at + ln].tobytes() if k == "sent" else None))
        return out

    def expect(self, oracle, lst, table_id, cap, nseg, first=0, last=M64, live_only=False, start=(0, 0),
               sent_cap=None):
        w = Want()
        sm = dict(ZERO, next_index=len(lst), done=1)
        segs, counts, sent, seg_first = [], [], [], []
        stop = False
        for v in range(start[0], len(lst)):
            cls = self.classes(lst[v], table_id, first, last, live_only)
            for r in range(start[1] if v == start[0] else 0, len(cls)):
                k, etype, ln, pay = cls[r]
                if k == "sent":
                    lb = ac.len_bytes(ln)
                    size = 1 + lb + ln
                    big = size > cap
                    opens = not segs or len(segs[-1]) + size > cap
                    if big or (sent_cap is not None and len(sent) == sent_cap) or (opens and len(segs) == nseg):
                        sm.update(next_index=v, next_record=r, done=0, too_large=int(big))
                        stop = True
                        break
                    if opens:
                        seg_first.append(len(sent))
                        segs.append(bytearray())
                        counts.append([0, 0, 0, 0])
                    segs[-1] += bytes([etype | ((lb - 1) << 6)]) + ln.to_bytes(lb, "little") + pay
                    counts[-1][0] += 1
                    counts[-1][1 if etype == OBJ else 2] += 1
                    sm["sent_objects" if etype == OBJ else "sent_tombstones"] += 1
                    sm["sent_bytes"] += size
                    sm["payload_bytes"] += ln
                    sent.append((lst[v], r))
                else:
                    sm[k] += 1
                sm["records_read"] += 1
            if stop:
                break
        sm["segments_used"] = len(segs)
        w.summary, w.segs, w.sent, w.seg_first = sm, [bytes(s) for s in segs], sent, seg_first
        w.counts = [tuple(c) for c in counts]
        w.certs = [ac.expected_cert(oracle, s) for s in w.segs]
        return w


# ----------------------------------------------------------------- outputs
class Got:
    pass


def split(cap, stride, nseg, out, certs, counts, sent, seg_first, sm):
    """One call's outputs (arrays that started as 0xA5 bytes) as a Got; nothing
    at or past a head, past segments_used or past the sent entries is written."""
    u8 = lambda a: np.zeros(0, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = Got()
    sm = u8(sm)
    g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
    assert (sm[SUMMARY.itemsize:] == FILL).all(), "a word past the summary was written"
    used = g.summary["segments_used"]
    assert used <= nseg
    out, certs, counts, first = u8(out), u8(certs), u8(counts), u8(seg_first)
    g.certs = [tuple(int(x) for x in c) for c in certs[:8 * used].view(np.uint32).reshape(-1, 2)]
    g.counts = [tuple(int(x) for x in c) for c in counts[:16 * used].view(np.uint32).reshape(-1, 4)]
    g.seg_first = [int(x) for x in first[:8 * used].view(np.uint64)]
    g.segs = []
    for k, (head, _) in enumerate(g.certs):
        assert head <= cap, "a head past the capacity"
        g.segs.append(out[k * stride:k * stride + head].tobytes())
        end = (k + 1) * stride if k + 1 < nseg else out.size
        assert (out[k * stride + head:end] == FILL).all(), "a byte at or past a head was written"
    assert (out[used * stride:] == FILL).all(), "an output past segments_used was written"
    assert (certs[8 * used:] == FILL).all() and (counts[16 * used:] == FILL).all(), \
        "a certificate or a count past segments_used was written"
    assert (first[8 * used:] == FILL).all(), "a first index past segments_used was written"
    n = g.summary["sent_objects"] + g.summary["sent_tombstones"]
    g.sent = None
    if sent is not None:
        s = u8(sent)
        g.sent = [tuple(int(x) for x in p) for p in s[:8 * n].view(np.uint32).reshape(-1, 2)]
        assert (s[8 * n:] == FILL).all(), "a reference past the sent entries was written"
    return g


def same_got(a, b, what=""):
    for f in ("summary", "segs", "certs", "counts", "seg_first", "sent"):
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def check(g, w, what=""):
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.segs == w.segs, (what, "the transfer segments' bytes")
    assert g.certs == w.certs, (what, g.certs, w.certs)
    assert g.counts == w.counts and g.seg_first == w.seg_first, (what, g.counts, w.counts)
    if g.sent is not None:
        assert g.sent == w.sent, (what, "d_sent")


def rounded(n):
    return max(16, -(-n // 16) * 16)


# ------------------------------------------------------------------ drivers
class HostTab:
    """A host table, the model beside it.  add() takes entry lists (one segment
    each); hashes: None (computed), "true" or "fake" (a caller's hashes: the
    key's own, or its complement -- the same for equal keys, so the table holds
    the same keys, and different from what the call would compute)."""
    device = False

    def __init__(self, drv, key_cap=4096, max_batches=16):
        self.drv, self.key_cap = drv, key_cap
        self.t = drv.ramcrc.ReplayTableHost(key_cap, max_batches)
        self.model = Model()

    def close(self):
        self.t.close()

    def source(self, lists, cap, bad=(), damage=()):
        buf, certs = ac.source_of(self.drv.oracle, lists, cap)
        for s in bad:
            certs[s, 1] ^= 1
        return buf, certs

    @staticmethod
    def hashes_for(kind, b):
        if kind is None:
            return None
        hs = np.zeros(b.table.shape[0], np.uint64)
        for r, p in enumerate(rc.participants(b.buf, b.cap, b.table, b.status)):
            if p is not None and p[0] == "rec":
                h = pc.key_hash(p[2][0], p[2][1])
                hs[r] = h if kind == "true" else h ^ M64
            else:
                hs[r] = 0x5A5A5A5A5A5A5A5A
        return hs

    def add(self, lists, cap=64 * KiB, bad=(), hashes=None, damage=()):
        buf, certs = self.source(lists, cap, bad)
        status, table = ac.host_walk(self.drv.oracle, buf, certs, len(lists), cap)
        for rec, how in damage:
            ac.damage_record(table, rec, how, cap)
        b = Plain(buf, cap, status, table)
        b.nseg = len(lists)
        b.hashes = self.hashes_for(hashes, b)
        n = self.t.add(buf, cap, b.nseg, status, table, key_hash=b.hashes)
        assert n == self.model.add(b)
        return n

    def clean(self, victims):
        sz = self.model.size(victims).summary
        cap, ecap = rounded(sz["needed_bytes"]), max(sz["needed_records"], 1)
        o = self.t.clean(victims, cap, ecap)
        w = self.model.clean(self.drv.oracle, victims, cap, ecap)
        assert o["batch"] == w.summary["batch"] and o["out"][:len(w.out)].tobytes() == w.out
        return o["batch"]

    def call(self, lst, table_id, cap, nseg, first=0, last=M64, live_only=False, start=(0, 0), stride=None,
             sent_cap="all", flags=None):
        stride = cap if stride is None else stride
        o = self.t.migrate(lst, table_id, cap, nseg, first_hash=first, last_hash=last, live_only=live_only,
                           start=start, out_stride=stride, want_sent=sent_cap is not None,
                           sent_cap=None if sent_cap in ("all", None) else sent_cap, fill=FILL, flags=flags)
        return split(cap, stride, nseg, o["out"], o["certs"], o["counts"], o["sent"], o["seg_first"],
                     np.array([o["summary"]]))

    def migrate(self, lst, table_id, cap, nseg, what="", **kw):
        """The call, held against the model."""
        g = self.call(lst, table_id, cap, nseg, **kw)
        m = {k: v for k, v in kw.items() if k in ("first", "last", "live_only", "start")}
        sc = kw.get("sent_cap", "all")
        w = self.model.expect(self.drv.oracle, list(lst), table_id, cap, nseg,
                              sent_cap=sc if isinstance(sc, int) else None, **m)
        check(g, w, what)
        return g

    def einval(self, *a, **kw):
        R = self.drv.ramcrc
        try:
            HostTab.call(self, *a, **kw)
        except R.RamcrcError as e:
            return e.code == R.EINVAL
        return False

    def lookup(self, keys):
        kb, q = segments.lookup_queries(keys)
        return self.t.lookup(kb, q)[0]

    def receive(self, g, cap, stride=None):
        """The receiving side into this table: walk the transfer segments under
        their certificates, every one must be OK, then add."""
        n = len(g.segs)
        buf = np.zeros(max(n, 1) * cap, np.uint8)
        for k, s in enumerate(g.segs):
            buf[k * cap:k * cap + len(s)] = np.frombuffer(s, np.uint8)
        certs = np.array(g.certs, np.uint32).reshape(-1, 2)
        status, table = ac.host_walk(self.drv.oracle, buf, certs, n, cap)
        assert n == 0 or ((status[:, 0] == segments.SEG_OK).all() and
                          status[:, 1].tolist() == [c[1] for c in g.certs]), status
        b = Plain(buf, cap, status, table)
        b.nseg = n
        if n:
            self.t.add(buf, cap, n, status, table)
            self.model.add(b)
        return b


class HostDriver:
    def __init__(self, ramcrc, oracle):
        self.ramcrc, self.oracle = ramcrc, oracle

    def tab(self, key_cap=4096, max_batches=16):
        return HostTab(self, key_cap, max_batches)


class DeviceTab(HostTab):
    """A table on the device with its twin on the host: every migration is
    held against the twin's, byte for byte."""
    device = True

    def __init__(self, drv, key_cap=4096, max_batches=16):
        self.drv, self.key_cap = drv, key_cap
        self.t = drv.ramcrc.ReplayTable(drv.ctx, key_cap, max_batches)
        self.twin = drv.ramcrc.ReplayTableHost(key_cap, max_batches)
        self.model = Model()
        self.added = []

    def close(self):
        self.t.close()
        self.twin.close()

    def add(self, lists, cap=64 * KiB, bad=(), hashes=None, damage=()):
        import torch
        buf, certs = self.source(lists, cap, bad)
        w = ac.Walked(self.drv.ctx, buf, certs, cap, len(lists))
        for rec, how in damage:
            ac.damage_record(w.table, rec, how, cap)
            w.d_entries[:w.table.shape[0]] = torch.from_numpy(w.table.view(np.int32)).cuda()
        b = Plain(buf, cap, w.status, w.table)
        b.nseg = len(lists)
        b.hashes = self.hashes_for(hashes, b)
        a = tc.Added(w, b.hashes)
        n = a.add(self.t)
        self.added.append(a)
        assert n == self.twin.add(buf, cap, b.nseg, w.status, w.table, key_hash=b.hashes) == self.model.add(b)
        return n

    def clean(self, victims):
        import torch
        sz = self.model.size(victims).summary
        cap, ecap = rounded(sz["needed_bytes"]), max(sz["needed_records"], 1)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
        o = dict(out=z(cap, torch.uint8), cert=z(2, torch.int32), status=z(4, torch.int32).view(1, 4),
                 entries=z(4 * ecap, torch.int32).view(-1, 4), n=z(1, torch.int64), work=z(ecap, torch.int64),
                 summary=z(14, torch.int64))
        n = self.t.clean(victims, o["out"], o["cert"], o["status"], o["entries"], o["n"], o["work"], o["summary"],
                         out_capacity=cap)
        self.drv.ctx.check()
        h = self.twin.clean(victims, cap, ecap)
        w = self.model.clean(self.drv.oracle, victims, cap, ecap)
        assert n == h["batch"] == w.summary["batch"]
        assert o["out"].cpu().numpy()[:len(w.out)].tobytes() == w.out
        self.added.append(o)
        return n

    def launch(self, lst, table_id, cap, nseg, first=0, last=M64, live_only=False, start=(0, 0), stride=None,
               sent_cap="all", flags=None, stream=None):
        """The device call alone, on outputs of 0xA5 bytes; returns the tensors."""
        import torch
        stride = cap if stride is None else stride
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        if sent_cap == "all":
            sent_cap = sum(self.model.batches[n].table.shape[0] for n in lst
                           if n < len(self.model.batches) and self.model.batches[n] is not None)
        d = dict(out=fill(nseg * stride + PAD, torch.uint8), certs=fill(8 * nseg + PAD, torch.int32),
                 counts=fill(16 * nseg + PAD, torch.int32), first=fill(8 * nseg + PAD, torch.int64),
                 summary=fill(SUMMARY.itemsize + PAD, torch.int64),
                 sent=None if sent_cap is None else fill(8 * sent_cap + PAD, torch.int32))
        self.t.migrate(lst, table_id, d["out"], cap, nseg, d["certs"], d["counts"], d["summary"], first_hash=first,
                       last_hash=last, live_only=live_only, start=start, out_stride=stride, sent=d["sent"],
                       sent_cap=sent_cap, seg_first=d["first"], flags=flags, stream=stream)
        d.update(cap=cap, stride=stride, nseg=nseg)
        return d

    @staticmethod
    def read(d):
        c = lambda x: None if x is None else x.cpu().numpy()
        return split(d["cap"], d["stride"], d["nseg"], c(d["out"]), c(d["certs"]), c(d["counts"]), c(d["sent"]),
                     c(d["first"]), c(d["summary"]))

    def call(self, lst, table_id, cap, nseg, **kw):
        d = self.launch(lst, table_id, cap, nseg, **kw)
        self.drv.ctx.check()
        g = self.read(d)
        t, self.t = self.t, self.twin
        try:
            h = HostTab.call(self, lst, table_id, cap, nseg, **kw)
        finally:
            self.t = t
        same_got(g, h, "device against host")
        return g

    def einval(self, *a, **kw):
        """Both forms refuse, the device form before any launch."""
        R = self.drv.ramcrc
        try:
            self.launch(*a, **kw)
            return False
        except R.RamcrcError as e:
            if e.code != R.EINVAL:
                return False
        t, self.t = self.t, self.twin
        try:
            return HostTab.einval(self, *a, **kw)
        finally:
            self.t = t

    def lookup(self, keys):
        kb, q = segments.lookup_queries(keys)
        res = lc.Looked(self.drv.ctx, self.t, kb, q).results
        assert lc.same(res, self.twin.lookup(kb, q)[0])
        return res

    def receive(self, g, cap, stride=None):
        """walk -> add on the device, of the bytes the migration wrote."""
        n = len(g.segs)
        buf = np.zeros(max(n, 1) * cap, np.uint8)
        for k, s in enumerate(g.segs):
            buf[k * cap:k * cap + len(s)] = np.frombuffer(s, np.uint8)
        certs = np.array(g.certs, np.uint32).reshape(-1, 2)
        if n == 0:
            return None
        w = ac.Walked(self.drv.ctx, buf, certs, cap, n, min_entry=27)
        assert (w.status[:, 0] == segments.SEG_OK).all() and w.status[:, 1].tolist() == [c[1] for c in g.certs]
        b = Plain(buf, cap, w.status, w.table)
        b.nseg = n
        a = tc.Added(w)
        a.add(self.t)
        self.added.append(a)
        self.twin.add(buf, cap, n, w.status, w.table)
        self.model.add(b)
        return b


class DeviceDriver:
    def __init__(self, ramcrc, oracle, ctx):
        self.ramcrc, self.oracle, self.ctx = ramcrc, oracle, ctx

    def tab(self, key_cap=4096, max_batches=16):
        return DeviceTab(self, key_cap, max_batches)


# -------------------------------------------------------------------- cases
def head(seg_id=1):
    return pc.entry(pc.SEGHEADER, pc.seg_header(seg_id))


def check_fixture(drv, ref):
    """The model and both forms against what the reference's tests state."""
    for c in ref["cases"]:
        tab = drv.tab(64, 2)
        try:
            es = [head()]
            for r in c["records"]:
                if r["type"] == "OBJ":
                    es.append(rc.obj(r["table_id"], r["key"].encode(), r["version"], r["value"].encode()))
                else:
                    assert r["type"] == "RPCRESULT"
                    es.append(pc.entry(pc.RPCRESULT, pc.rpc_result(r["table_id"], 0, response=b"\0" * r["response_bytes"])))
                    assert len(es[-1]) - 2 == r["payload_bytes"]
            tab.add([es], 4 * KiB)
            g = tab.migrate([0], c["table_id"], 1024, 4, first=c["first_hash"], last=c["last_hash"], what=c["name"])
            e = c["expect"]
            assert g.summary["sent_objects"] == e["objects"] and g.summary["sent_tombstones"] == e["tombstones"]
            assert g.summary["payload_bytes"] == e["payload_bytes"], c["name"]
            assert g.summary["skipped_other"] == 1 + e["skipped_other"], c["name"]   # (the SEGHEADER)
            assert g.summary["done"] == 1
            if "reference_total_bytes" in c:
                assert c["reference_total_bytes"] == e["payload_bytes"] + e["skipped_other_bytes"]
        finally:
            tab.close()


COUNTS = (0, 257, 255, 256, 3 * TILE + 5, 1)   # records of table ids 100 .. 105, in this order; the last: one tile


def count_lists():
    """One segment (COUNT_CAP bytes): per count n of COUNTS n objects of table
    id 100 + its index, group after group, so that a table id's records start
    and end at any place of a tile and the last id's only record lies in the
    last tile; among them one object of each id with another high half.  One
    segment, because a walk's record order across segments is unspecified and
    the log order of this batch has to be the same in every run."""
    es = [head()]
    for t, n in enumerate(COUNTS):
        es += [rc.obj(100 + t, b"count %d %d" % (t, i), 1 + i % 3, b"v%d" % i) for i in range(n)]
        es.append(rc.obj((100 + t) | (1 << 32), b"count %d 0" % t, 1, b"other half"))
    return [es]


COUNT_CAP = 128 * KiB


def case_counts(drv):
    """0, 1, 255, 256, 257 and 3 * 256 + 5 selected records; selected records
    only in the last tile; a listed batch without records; three and more table
    ids in one table and ids that differ in the high half only; many cuts."""
    tab = drv.tab(4096, 4)
    try:
        lists = count_lists()
        assert tab.add(lists, COUNT_CAP) == 0
        assert tab.add([[]], 4 * KiB) == 1           # no records at all
        assert tab.add([[head(3)]], 4 * KiB, hashes="true") == 2
        n_rec = tab.model.batches[0].table.shape[0]
        assert n_rec > 6 * TILE and (n_rec - 2) // TILE == (n_rec - 1) // TILE   # the last id's record: in the last tile
        for t, n in enumerate(COUNTS):
            g = tab.migrate([1, 0, 2], 100 + t, 512, 80, what=("count", n))
            assert g.summary["sent_objects"] == n and g.summary["done"] == 1
            assert g.summary["records_read"] == n_rec + 1
            assert g.summary["segments_used"] == len(g.segs) and (n < 100 or len(g.segs) > 8)
        g = tab.migrate([0], 100 | (1 << 32), 4 * KiB, 2, what="the other high half")
        assert g.summary["sent_objects"] == 1
        g = tab.migrate([1, 2], 100, 512, 2, what="only batches without a selected record")
        assert g.summary["segments_used"] == 0 and g.summary["done"] == 1 and g.summary["records_read"] == 1
    finally:
        tab.close()


def case_boundaries(drv):
    """A cut exactly on a tile boundary and on a batch boundary: 64-byte
    entries, 4 per 256-byte output.  Batch 0: the SEGHEADER, three objects of
    another table, then 252 + 8 selected ones, so that the 64th output begins
    with record 256 (a tile's first) and the last one is full at the batch's
    end; batch 1 holds 9 more."""
    mk = lambda b, i: rc.obj(7, b"key %04d %05d" % (b, i), 1, b"%021d" % i)    # 1 + 1 + 27 + 14 + 21 = 64
    tab = drv.tab(1024, 4)
    try:
        assert len(mk(0, 0)) == 64
        tab.add([[head()] + [rc.obj(8, b"other %d" % i, 1) for i in range(3)] + [mk(0, i) for i in range(252 + 8)]],
                64 * KiB)
        tab.add([[mk(1, i) for i in range(9)]], 4 * KiB)
        g = tab.migrate([0, 1], 7, 256, 80, what="cuts at a tile's and a batch's end")
        assert all(c[0] == 4 for c in g.counts[:-1]) and g.counts[-1][0] == 1
        firsts = {g.sent[f] for f in g.seg_first}
        assert (0, TILE) in firsts, "a cut before a tile's first record"
        assert (1, 0) in firsts, "a cut on the batch boundary"
    finally:
        tab.close()


def case_entry_sizes(drv):
    """An entry that exactly fills an output fits; one byte more opens the
    next; payloads of 255 / 256 and 65,535 / 65,536 bytes (the length-byte
    steps); a source entry with more length bytes than minimal is rebuilt; an
    entry larger than an output in the middle: too_large, the cursor on it,
    the earlier outputs sealed; an OVERLONG record takes no part."""
    sized = lambda key, n, ver=1: rc.obj(7, key, ver, b"s" * (n - (2 if n < 258 else 3 if n < 65539 else 4) - 27 - len(key)))
    tab = drv.tab(256, 8)
    try:
        a, b, c = sized(b"k64a", 64), sized(b"k64b", 64), sized(b"k65c", 65)
        assert (len(a), len(b), len(c)) == (64, 64, 65)
        tab.add([[head(), a, b, c, sized(b"k63d", 63)]], 4 * KiB)
        g = tab.migrate([0], 7, 128, 4, what="exactly full")
        assert [x[0] for x in g.certs] == [128, 128] and g.counts[0][0] == 2
        g = tab.migrate([0], 7, 64, 4, what="one byte too many")
        assert g.summary["too_large"] == 1 and (g.summary["next_index"], g.summary["next_record"]) == (0, 3)
        assert g.summary["segments_used"] == 2 and g.summary["done"] == 0
        g = tab.migrate([0], 7, 64, 4, start=(0, 4), what="behind the large entry")
        assert g.summary["done"] == 1 and g.summary["sent_objects"] == 1
        # the length-byte steps, and a header that is rebuilt
        wide = pc.entry(OBJ, pc.obj(7, b"wide header", b"w" * 40, version=1), length_bytes=3)
        steps = [sized(b"p%d" % n, n + ac.len_bytes(n) + 1) for n in (255, 256, 65535, 65536)]
        tab.add([[head(2), wide] + steps], 256 * KiB)
        g = tab.migrate([1], 7, 65552, 8, what="length-byte steps")
        assert g.summary["sent_objects"] == 5 and g.summary["done"] == 1
        ents = [e for s, c in zip(g.segs, g.certs) for e in segments.migrate_entries(s, c[0])]
        assert [len(p) for _, p in ents] == [len(wide) - 4, 255, 256, 65535, 65536]
        assert g.segs[0][0] == OBJ and g.segs[0][1] == len(wide) - 4, "the header was copied, not rebuilt"
        g = tab.migrate([1], 7, 4 * KiB, 8, what="a large entry in the middle")
        assert g.summary["too_large"] == 1 and g.summary["next_record"] == 4 and g.summary["segments_used"] == 1
        # OVERLONG
        tab.add([[head(3), a, b]], 4 * KiB, damage=[(2, "overlong_flag")])
        g = tab.migrate([2], 7, 128, 4, what="an overlong record")
        assert g.summary["sent_objects"] == 1 and g.summary["skipped_other"] == 2 and g.summary["too_large"] == 0
    finally:
        tab.close()


def case_hash_range(drv):
    """A hash equal to first_hash, equal to last_hash, one below and one
    above; first > last; the full range; batches added with a caller's hashes
    (which are not the keys' own) and without."""
    keys = [b"range key %d" % i for i in range(40)]
    tab = drv.tab(256, 4)
    try:
        tab.add([[head()] + [rc.obj(9, k, 2, b"computed") for k in keys[:20]] +
                 [rc.tomb(9, k, 3) for k in keys[5:10]]], 16 * KiB)
        tab.add([[head(2)] + [rc.obj(9, k, 2, b"given") for k in keys[20:]]], 16 * KiB, hashes="fake")
        # the record hashes: the keys' own in batch 0, the caller's in batch 1
        eff = [pc.key_hash(9, k) ^ (0 if i < 20 else M64) for i, k in enumerate(keys)]
        assert len(set(eff)) == 40
        for part in (sorted(eff[:20]), sorted(eff[20:])):
            lo, hi = part[3], part[12]
            for first, last in ((lo, hi), (lo + 1, hi), (lo, hi - 1), (lo + 1, hi - 1), (lo, lo), (hi, hi), (hi, lo)):
                g = tab.migrate([0, 1], 9, 256, 40, first=first, last=last, what=("range", first, last))
                n = sum(first <= h <= last for h in eff)
                assert g.summary["sent_objects"] == n, (first, last, g.summary)
                assert n >= (10 if (first, last) == (lo, hi) else 0) and (first <= last or n == 0)
        g = tab.migrate([0, 1], 9, 256, 40, what="the full range")
        assert g.summary["sent_objects"] == 40 and g.summary["sent_tombstones"] == 5
        assert g.summary["skipped_range"] == 0
    finally:
        tab.close()


def case_liveness(drv):
    """Both modes over replay_table_cases.relation_lists (overwrites, tombstone
    winners, equal-version ties), before and after a clean: the survivor batch
    is listed, a victim in the list is EINVAL."""
    tab = drv.tab(4096, 8)
    try:
        for es in tc.relation_lists():
            tab.add([es], 64 * KiB)
        for tid in (2, 3, 4, 5):
            for live in (False, True):
                g = tab.migrate([0, 1, 2], tid, 1024, 64, live_only=live, what=("relations", tid, live))
                assert g.summary["done"] == 1 and (live or g.summary["skipped_dead"] == 0)
                if live:
                    wins = sum(1 for k, (_, rank) in tab.model.win.items() if k[0] == tid)
                    assert g.summary["sent_objects"] + g.summary["sent_tombstones"] == wins
                    assert g.summary["skipped_dead"] > 0
        before = {tid: tab.call([0, 1, 2], tid, 1024, 64, live_only=True) for tid in (2, 5)}
        n = tab.clean([0, 1])
        assert n == 3
        for tid in (2, 5):
            for live in (False, True):
                g = tab.migrate([3, 2], tid, 1024, 64, live_only=live, what=("after the clean", tid, live))
            # the winners are the same records, wherever they lie now
            ents = lambda x: sorted(e for s, c in zip(x.segs, x.certs) for e in segments.migrate_entries(s, c[0]))
            assert ents(g) == ents(before[tid])
        assert tab.einval([3, 0], 2, 1024, 4) and tab.einval([1], 2, 1024, 4)
    finally:
        tab.close()


def foreign_lists():
    h = pc.key_hash(7, b"foreign")
    good = lambda i: rc.obj(7, b"good %d" % i, 1, b"v")
    others = [pc.entry(pc.RPCRESULT, pc.rpc_result(7, h, response=b"\0" * 12)), pc.entry(pc.PREP, pc.prep(7, b"foreign", b"p")),
              pc.entry(pc.PREPTOMB, pc.prep_tomb(7, h)), pc.entry(pc.TXDECISION, pc.tx_decision(7, h)),
              pc.entry(pc.TXPLIST, pc.tx_plist([(7, h, 1)])), pc.entry(pc.SAFEVERSION, pc.safe_version(9)),
              pc.entry(pc.LOGDIGEST, b"digest"),
              pc.entry(OBJ, pc.obj(7, b"short", key_len=6)), pc.entry(OBJTOMB, b"\0" * 16)]   # malformed
    a = [head()]
    for i, o in enumerate(others):
        a += [good(i), o]
    return [a, [head(2)] + [good(100 + i) for i in range(5)], [head(3), good(200), rc.tomb(7, b"good 0", 1)]]


def case_foreign(drv):
    """Segments without RAMCRC_SEG_OK, malformed records and the other record
    types among the selected: none is sent, all count as skipped_other."""
    tab = drv.tab(256, 4)
    try:
        lists = foreign_lists()
        tab.add(lists, 8 * KiB, bad=(1,))
        for live in (False, True):
            g = tab.migrate([0], 7, 256, 16, live_only=live, what=("foreign", live))
            # (the tombstone of "good 0" has its object's version and wins)
            assert g.summary["sent_objects"] == 10 - live and g.summary["sent_tombstones"] == 1
            assert g.summary["skipped_dead"] == int(live)
            assert g.summary["skipped_other"] == 3 + 9 + 5 and g.summary["done"] == 1
            for s, c in zip(g.segs, g.certs):
                assert all(t in (OBJ, OBJTOMB) for t, _ in segments.migrate_entries(s, c[0]))
    finally:
        tab.close()


def cursor_lists():
    o = lambda t, k, v=1: rc.obj(t, b"cursor %d" % k, v, b"value %d" % k)
    return [[head(), o(7, 0), o(8, 1), o(7, 2), rc.tomb(7, b"cursor 0", 1), pc.entry(pc.SAFEVERSION, pc.safe_version(3))],
            [],
            [o(7, 3), o(7, 4, 2), o(9, 5), o(7, 6), o(7, 4, 1), o(7, 7)]]


def case_cursor(drv):
    """max_segments 0, 1, exactly enough and one more; every start cursor of a
    small scenario; K calls of one output each, chained by the cursor, write
    what one call with K outputs writes, and their counters add up; sent_cap
    short by one stops the call as a full output does."""
    tab = drv.tab(256, 4)
    try:
        for es in cursor_lists():
            tab.add([es], 4 * KiB)
        lst = [0, 1, 2]
        for live in (False, True):
            whole = tab.migrate(lst, 7, 96, 16, live_only=live, what="one call")
            K = whole.summary["segments_used"]
            assert K >= 3 and whole.summary["done"] == 1
            for nseg in (0, 1, K - 1, K, K + 1):
                g = tab.migrate(lst, 7, 96, nseg, live_only=live, what=("max_segments", nseg))
                assert g.summary["done"] == int(nseg >= K) and g.segs == whole.segs[:nseg]
            # the chain
            at, segs, certs, sent, total = (0, 0), [], [], [], dict(ZERO)
            for _ in range(K + 2):
                g = tab.migrate(lst, 7, 96, 1, live_only=live, start=at, what=("chained", at))
                segs += g.segs
                certs += g.certs
                sent += g.sent
                for k in NAMES[4:]:
                    total[k] += g.summary[k]
                at = (g.summary["next_index"], g.summary["next_record"])
                if g.summary["done"]:
                    break
            assert g.summary["done"] == 1 and at == (3, 0)
            assert segs == whole.segs and certs == whole.certs and sent == whole.sent
            assert total == dict(whole.summary, next_index=0, next_record=0, done=0, too_large=0)
            # every start cursor
            for v, n in enumerate([6, 0, 6]):
                for r in range(n + 1):
                    tab.migrate(lst, 7, 96, 2, live_only=live, start=(v, r), what=("start", v, r))
            g = tab.migrate(lst, 7, 96, 2, start=(3, 0), what="the end's cursor")
            assert g.summary["done"] == 1 and g.summary["records_read"] == 0
            # d_sent short by one
            n = whole.summary["sent_objects"] + whole.summary["sent_tombstones"]
            g = tab.migrate(lst, 7, 96, 16, live_only=live, sent_cap=n - 1, what="sent_cap short by one")
            assert g.summary["done"] == 0 and g.summary["too_large"] == 0 and g.sent == whole.sent[:-1]
            assert (g.summary["next_index"], g.summary["next_record"]) == whole.sent[-1]
            g = tab.migrate(lst, 7, 96, 16, live_only=live, sent_cap=None, what="no d_sent")
            assert g.segs == whole.segs
        assert tab.einval(lst, 7, 96, 2, start=(4, 0)) and tab.einval(lst, 7, 96, 2, start=(3, 1))
        # (the host form knows the batch's records, the device form its entries_cap)
        assert tab.einval(lst, 7, 96, 2, start=(0, 4 * KiB if tab.device else 7))
    finally:
        tab.close()


def case_arguments(drv):
    """The EINVAL list of rules 1, 2 and 7."""
    tab = drv.tab(64, 4)
    try:
        tab.add([[head(), rc.obj(7, b"k", 1, b"v")]], 4 * KiB)
        tab.add([[head(2)]], 4 * KiB)
        assert tab.migrate([0, 1], 7, 64, 2).summary["sent_objects"] == 1
        for lst in ([], [0, 0], [2], [0, 1, 0]):
            assert tab.einval(lst, 7, 64, 2), lst
        assert tab.einval([0], 7, 64, 2, flags=2) and tab.einval([0], 7, 64, 2, flags=0x80000001)
        assert tab.einval([0], 7, 72, 2) and tab.einval([0], 7, 64, 2, stride=72) and tab.einval([0], 7, 64, 2, stride=48)
        assert tab.einval([0], 7, segments.MIGRATE_MAX_CAPACITY + 16, 1)
        assert tab.migrate([0, 1], 7, 64, 2, stride=128).summary["done"] == 1
    finally:
        tab.close()


def case_spoiled(drv):
    """On a spoiled table only the summary is written, zero with spoiled = 1."""
    tab = drv.tab(2, 4)
    try:
        es = [head()] + [rc.obj(7, b"spoil %d" % i, 1) for i in range(3)]   # three keys, key_cap 2
        R = drv.ramcrc
        try:
            tab.add([es], 4 * KiB)
        except R.RamcrcError:   # (the host form refuses the add that spoils its table)
            pass
        if tab.device:
            try:
                drv.ctx.check()
            except R.RamcrcError:
                pass
        g = tab.call([0], 7, 64, 2)
        assert g.summary == dict(ZERO, spoiled=1) and g.segs == [] and g.sent == []
    finally:
        tab.close()


def chain_lists(seed):
    """Four batches' entry lists with overwrites and tombstones over three
    table ids (resolve_cases.mixed_lists), one list a batch."""
    return rc.mixed_lists(seed=seed, nkeys=120, nseg=4)


def answers(tab, keys):
    """key -> (kind, version, value bytes) as the table answers now."""
    res = tab.lookup(keys)
    out = {}
    for key, r in zip(keys, res):
        kind = int(r["kind"])
        val = b""
        if kind == lc.OBJECT:
            b = tab.model.batches[int(r["batch"])]
            at = int(r["segment"]) * b.cap + int(r["value_off"])
            val = b.buf[at:at + int(r["value_len"])].tobytes()
        out[key] = (kind, int(r["version"]) if kind != lc.ABSENT else 0, val)
    return out


def case_chain(drv, seed):
    """table -> transfer segments with certificates -> walk -> add -> read."""
    src = drv.tab(4096, 8)
    dsts = []
    try:
        for es in chain_lists(seed):
            src.add([es], 64 * KiB)
        lst = [0, 1, 2, 3]
        keys = sorted(src.model.win)
        tid = 1
        mine = [k for k in keys if k[0] == tid]
        hs = sorted(pc.key_hash(*k) for k in mine)
        mid = hs[len(hs) // 2]
        want_src = answers(src, keys)
        absent = (lc.ABSENT, 0, b"")
        # keys with several records of their winner's version and type
        seen = {}
        for b in src.model.batches:
            for p in rc.participants(b.buf, b.cap, b.table, b.status):
                if p is not None and p[0] == "rec":
                    seen[p[2], p[3], p[1]] = seen.get((p[2], p[3], p[1]), 0) + 1
        tied = {k for k, (ver, rank) in src.model.win.items() if seen[k, ver, OBJ if rank[0] else OBJTOMB] > 1}
        assert tied and len(tied) < len(keys)
        for first, last in ((0, mid), (mid + 1, M64)):
            inside = lambda k: k[0] == tid and first <= pc.key_hash(*k) <= last
            got = []
            for live in (False, True):
                g = src.migrate(lst, tid, 512, 64, first=first, last=last, live_only=live,
                                what=("chain", seed, live))
                assert g.summary["done"] == 1 and g.summary["segments_used"] > 1
                if live:
                    assert g.summary["sent_objects"] + g.summary["sent_tombstones"] == sum(1 for k in keys if inside(k))
                dst = drv.tab(4096, 4)
                dsts.append(dst)
                dst.receive(g, 512)
                a = answers(dst, keys)
                for k in keys:
                    # (among several sent records of the winner's version and type the
                    # destination keeps the first its walk lists, and a walk's order
                    # across segments is unspecified: the value is pinned without such a tie)
                    n = 2 if k in tied and not live else 3
                    assert a[k][:n] == (want_src[k] if inside(k) else absent)[:n], (seed, live, k, a[k], want_src[k])
                got.append(a)
            assert all(got[0][k][:2] == got[1][k][:2] and (k in tied or got[0][k] == got[1][k]) for k in keys)
        # the two ranges partition the source's keys of the table id
        lo, hi = dsts[0], dsts[2]
        alo, ahi = answers(lo, mine), answers(hi, mine)
        for k in mine:
            assert (alo[k] == absent) != (ahi[k] == absent), k
    finally:
        src.close()
        for d in dsts:
            d.close()
