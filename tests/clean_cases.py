"""Scenarios for ramcrc_replay_table_clean_device / _host and their clean_size
forms (include/ramcrc.h), run on the host by test_replay_table_clean_host.py and
on the GPU by test_gpu_replay_table_clean.py.

The expectation is the plain Python of Model below: the table as a dictionary
key -> (version, rank), fed by add with replay's rule and by clean with the
rules of the header.  It is pinned by properties against calls that are
already pinned to the reference (lookup, read, live, the walk, the oracle's
certificate):
  P1  lookup, read, live and stats answer the same before and after, victim
      references mapped through d_moved;
  P2  a fresh table fed the remaining batches and the walked survivor answers
      every key with the same kind and version (and value, without ties);
  P3  certificate, status, record table and count are the walk's over d_out;
  P4  with every victim array overwritten, the answers stay, and a further
      add is resolved against the moved keys;
  P5  nothing is written past the head, past the count or to a victim array,
      and clean_size changes nothing."""
import ctypes

import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import lookup_cases as lc
import partition_cases as pc
import read_cases as rd
import remove_cases as mc
import replay_table_cases as tc
import resolve_cases as rc
import write_cases as wc

KiB = 1024
FILL = 0xA5
FILL32 = 0xA5A5A5A5
PAD = 64
NONE = segments.RESOLVE_NONE
USAGE = segments.CLEAN_USAGE_DTYPE
SUMMARY = segments.CLEAN_SUMMARY_DTYPE
SUMMARY_NAMES = SUMMARY.names
TILE = 256   # dev_clean.inc: records per tile of the mark pass
OBJ, OBJTOMB = pc.OBJ, pc.OBJTOMB


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


ZERO_SUMMARY = dict.fromkeys(SUMMARY_NAMES, 0)
SPOILED_SUMMARY = dict(ZERO_SUMMARY, spoiled=1)


# ---------------------------------------------------------- the expectation
class Plain:
    """A batch as the expectation reads it: buf, cap, nseg, status, table."""

    def __init__(self, buf, cap, status, table):
        self.buf, self.cap, self.nseg = buf, cap, 1
        self.status, self.table = status, table


EMPTY = Plain(np.zeros(16, np.uint8), 16, np.array([[1, 0, 0, 0]], np.uint32), np.zeros((0, 4), np.uint32))


class Want:
    """What one clean must write."""


class Model:
    """The table by the header's rules.  batches[n]: batch n as added, None
    once cleaned; win: key -> (version, (is_object, batch, record))."""

    def __init__(self):
        self.batches, self.win, self.safe = [], {}, 0

    def add(self, b):
        n = len(self.batches)
        self.batches.append(b)
        for r, p in enumerate(rc.participants(b.buf, b.cap, b.table, b.status)):
            if p is not None and p[0] == "safe":
                self.safe = max(self.safe, p[1])
            if p is None or p[0] != "rec":
                continue
            _, etype, key, ver = p
            rank = (etype == OBJ, n, r)
            cur = self.win.get(key)
            if cur is None or ver > cur[0] or (ver == cur[0] and rank < cur[1]):
                self.win[key] = (ver, rank)
        return n

    def results(self):
        """key -> a LOOKUP_RESULT_DTYPE tuple."""
        out = {}
        for key, (ver, (is_obj, b, r)) in self.win.items():
            bt = self.batches[b]
            seg, off, ln, hdr = (int(x) for x in bt.table[r])
            if is_obj:
                start = off + 1 + ((hdr >> 6) & 3) + 1
                at = seg * bt.cap + start
                vo, vl = lc.value_range(bt.buf[at:at + ln].tobytes())
                out[key] = (b, r, ver, lc.OBJECT, seg, start + vo, vl)
            else:
                out[key] = (b, r, ver, lc.TOMBSTONE, NONE, 0, 0)
        return out

    def payloads(self):
        out = {}
        for key, (_, (is_obj, b, r)) in self.win.items():
            if is_obj:
                bt = self.batches[b]
                seg, off, ln, hdr = (int(x) for x in bt.table[r])
                at = seg * bt.cap + off + 1 + ((hdr >> 6) & 3) + 1
                out[key] = bt.buf[at:at + ln].tobytes()
        return out

    def live(self, n):
        """(winner REF [records], live record indices) of batch n."""
        b = self.batches[n]
        parts = rc.participants(b.buf, b.cap, b.table, b.status)
        winner = np.zeros(len(parts), tc.REF)
        winner["batch"] = winner["record"] = NONE
        live = []
        for r, p in enumerate(parts):
            if p is None or p[0] != "rec":
                continue
            _, wb, wr = self.win[p[2]][1]
            winner[r] = (wb, wr)
            if (wb, wr) == (n, r):
                live.append(r)
        return winner, live

    def stats(self):
        objs = sum(1 for _, rank in self.win.values() if rank[0])
        return dict(keys=len(self.win), live_objects=objs, live_tombstones=len(self.win) - objs,
                    safe_version=self.safe, batches=len(self.batches), spoiled=0)

    def size(self, victims):
        """usage and the summary of clean_size; the live records in order."""
        w = Want()
        w.usage = np.zeros(len(victims), USAGE)
        sm = dict(ZERO_SUMMARY, victims=len(victims))
        w.live = []   # (batch, record, entry bytes, row, key, version, is_object)
        for v, n in enumerate(victims):
            b = self.batches[n]
            parts = rc.participants(b.buf, b.cap, b.table, b.status)
            w.usage[v]["records"] = len(parts)
            for r, p in enumerate(parts):
                seg, off, ln, hdr = (int(x) for x in b.table[r])
                if p is None or p[0] != "rec":
                    sm["dropped_other"] += 1
                    continue
                _, etype, key, ver = p
                kind = "objects" if etype == OBJ else "tombstones"
                if self.win[key][1][1:] != (n, r):
                    sm["dropped_" + kind] += 1
                    continue
                size = 1 + ((hdr >> 6) & 3) + 1 + ln
                at = seg * b.cap + off
                w.live.append((n, r, b.buf[at:at + size].tobytes(), (ln, hdr), key, ver, etype == OBJ))
                w.usage[v]["live_" + kind] += 1
                w.usage[v]["live_bytes"] += size
                sm["moved_" + kind] += 1
                sm[kind[:-1] + "_bytes"] += ln
        sm["records"] = int(w.usage["records"].sum())
        sm["needed_bytes"] = sm["out_bytes"] = int(w.usage["live_bytes"].sum())
        sm["needed_records"] = len(w.live)
        assert sm["records"] == sm["needed_records"] + sm["dropped_objects"] + sm["dropped_tombstones"] + \
            sm["dropped_other"]
        w.summary = sm
        return w

    def clean(self, oracle, victims, cap, ecap):
        """The Want of clean(victims); the model moves on when it fits."""
        w = self.size(victims)
        N = len(self.batches)
        w.fit = w.summary["needed_bytes"] <= cap and w.summary["needed_records"] <= ecap
        if not w.fit:
            w.summary = dict(SPOILED_SUMMARY, needed_bytes=w.summary["needed_bytes"],
                             needed_records=w.summary["needed_records"])
            return w
        w.summary["batch"] = N
        w.out = b"".join(x[2] for x in w.live)
        w.table = np.zeros((len(w.live), 4), np.uint32)
        w.moved = np.zeros(len(w.live), tc.REF)
        at = 0
        for j, (n, r, blob, (ln, hdr), key, ver, is_obj) in enumerate(w.live):
            w.table[j] = (0, at, ln, hdr)
            w.moved[j] = (n, r)
            self.win[key] = (ver, (is_obj, N, j))
            at += len(blob)
        w.cert = ac.expected_cert(oracle, w.out)
        w.status = np.array([[segments.SEG_OK, w.cert[1], len(w.live), 0]], np.uint32)
        buf = np.zeros(max(cap, 16), np.uint8)
        buf[:len(w.out)] = np.frombuffer(w.out, np.uint8)
        for n in victims:
            self.batches[n] = None
        self.batches.append(Plain(buf, max(cap, 16), w.status, w.table))
        return w


# ------------------------------------------------------------------ drivers
class Got:
    """One clean's outputs, read back."""


def _split(g, cap, ecap, nvic, out, cert, status, entries, n_entries, work, moved, usage, sm):
    u8 = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    sm = u8(sm)
    g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
    g.summary_past = sm[SUMMARY.itemsize:]
    g.out_all = u8(out)
    g.cert_raw, g.status_raw, g.n_raw = u8(cert), u8(status), u8(n_entries)
    g.entries_all, g.work_all, g.moved_all = u8(entries), u8(work), u8(moved)
    g.usage_all = u8(usage)
    g.usage = None if usage is None else g.usage_all[:nvic * 32].view(USAGE)
    ok = not g.summary["spoiled"]
    head = g.summary["out_bytes"] if ok else 0
    n = g.summary["needed_records"] if ok else 0
    g.out = g.out_all[:head].tobytes()
    g.cert = tuple(int(x) for x in g.cert_raw[:8].view(np.uint32))
    g.status = g.status_raw[:16].view(np.uint32).reshape(1, 4)
    g.n = int(g.n_raw[:8].view(np.uint64)[0])
    g.table = g.entries_all[:16 * n].view(np.uint32).reshape(-1, 4)
    g.work = g.work_all[:8 * n].view(np.uint64)
    g.moved = None if moved is None else g.moved_all[:8 * n].view(tc.REF)
    # P5: nothing at or past the head, past the count or past a record
    assert (g.out_all[head:] == FILL).all(), "a byte at or past the head was written"
    assert (g.entries_all[16 * n:] == FILL).all(), "a row past the survivors was written"
    assert (g.work_all[8 * n:] == FILL).all(), "a work word past the survivors was written"
    assert moved is None or (g.moved_all[8 * n:] == FILL).all(), "a reference past the survivors was written"
    assert (g.summary_past == FILL).all() and (g.cert_raw[8:] == FILL).all(), "a word past a record was written"
    assert (g.status_raw[16:] == FILL).all() and (g.n_raw[8:] == FILL).all(), "a word past a record was written"
    assert usage is None or (g.usage_all[nvic * 32:] == FILL).all(), "a usage past the victims was written"
    if not ok:
        for a in (g.cert_raw, g.status_raw, g.n_raw):
            assert (a == FILL).all(), "a spoiled or refused clean wrote more than its summary"
    return g


def _stub(cap):
    """What stands in tab.batches for a cleaned batch: no records, its stride."""
    return Plain(EMPTY.buf, cap, EMPTY.status, EMPTY.table)


class HostTab(mc.HostTab):
    def _init_clean(self):
        if not hasattr(self, "retired"):
            self.retired = set()

    def clean_size_raw(self, victims, want_usage=True):
        vic = np.ascontiguousarray(victims, np.uint32)
        usage = np.full(32 * len(vic) + PAD, FILL, np.uint8) if want_usage else None
        sm = np.full(SUMMARY.itemsize + PAD, FILL, np.uint8)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None
        R = self.drv.ramcrc
        R._check(R.lib().ramcrc_replay_table_clean_size_host(self.t._h, p(vic), len(vic), p(usage), p(sm)),
                 "ramcrc_replay_table_clean_size_host")
        g = Got()
        g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
        g.usage = None if usage is None else usage[:32 * len(vic)].view(USAGE)
        assert (sm[SUMMARY.itemsize:] == FILL).all() and (usage is None or (usage[32 * len(vic):] == FILL).all())
        return g

    def victim_arrays(self, victims):
        """The arrays of the victims that the table reads, as the wrapper keeps them."""
        return [a for n in victims for a in self.t._keep[n] if a is not None]

    def clean_raw(self, victims, cap, ecap, want_moved=True, scribble=True):
        """The call on arrays pre-filled with 0xA5; then (P5) the victims'
        arrays are unchanged and (P4) overwritten with 0xA5."""
        self._init_clean()
        arrays = self.victim_arrays(victims)
        before = [a.tobytes() for a in arrays]
        works = {n: self.t._keep[n][4].copy() for n in victims}
        g = Got()
        R = self.drv.ramcrc
        try:
            o = self.t.clean(victims, cap, ecap, want_moved=want_moved, fill=FILL)
            g.refused = False
        except R.RamcrcError as e:
            assert e.code == R.EINVAL and hasattr(e, "outputs"), e
            o = e.outputs
            g.refused = True
        _split(g, cap, ecap, len(victims), o["out"], np.array([o["cert"]]), o["status"], o["entries"],
               o["n_entries"], o["work"], o["moved"], o["usage"], np.array([o["summary"]]))
        g.batch, g.keep = o["batch"], o
        assert [a.tobytes() for a in arrays] == before, "a victim's array was written"
        if not g.summary["spoiled"]:
            if want_moved:
                old = np.array([works[int(b)][int(r)] for b, r in g.moved.tolist()], np.uint64)
                assert np.array_equal(g.work, old), "a survivor's work word is not its old slot"
            if scribble:
                for a in arrays:
                    a.view(np.uint8).reshape(-1)[:] = FILL
            self._retire(victims, Plain(o["out"] if cap else EMPTY.buf, max(cap, 16), g.status, g.table))
        return g

    def _retire(self, victims, survivor):
        for n in victims:
            self.retired.add(n)
            self.batches[n] = _stub(self.batches[n].cap)
        self.batches.append(survivor)

    def survivor_of(self, out, cert, cap):
        """The survivor walked by the oracle as one segment of `cap` bytes under
        the call's certificate, and the count of its bad checksums."""
        b = tc.HostBatch.__new__(tc.HostBatch)
        b.buf = np.zeros(cap, np.uint8)
        b.buf[:len(out)] = np.frombuffer(out, np.uint8)
        b.certs = np.array([cert], np.uint32)
        b.status, b.table = ac.host_walk(self.drv.oracle, b.buf, b.certs, 1, cap)
        b.cap, b.nseg = cap, 1
        bad, _, _ = self.drv.oracle.verify_objects(b.buf, cap, b.table, 1)
        return b, bad

    def live_of(self, n):
        winner, live, need, counts = self.t.live(n)
        assert need == live.shape[0]
        return winner, live[:, 0].tolist(), rc.counts_dict(counts)

    def stats_now(self):
        return tc.stats_dict(self.t.stats())

    def raises_on_live(self, n):
        try:
            self.t.live(n)
        except self.drv.ramcrc.RamcrcError as e:
            return e.code == self.drv.ramcrc.EINVAL
        return False

    def einval_clean(self, victims):
        """Does clean(victims) return RAMCRC_EINVAL before it takes a number?"""
        try:
            self.t.clean(victims, 4 * KiB, 64)
        except self.drv.ramcrc.RamcrcError as e:
            return e.code == self.drv.ramcrc.EINVAL and not hasattr(e, "outputs")
        return False


class HostDriver(mc.HostDriver):
    on_device = False

    def table(self, key_cap, max_batches):
        t = HostTab(self, key_cap, max_batches)
        t._init_clean()
        return t


class Cleaned:
    """One ramcrc_replay_table_clean_device call: every output pre-filled with
    0xA5 and longer than the call may write."""

    def __init__(self, ctx, t, victims, cap, ecap, want_moved=True, want_usage=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.nvic = len(victims)
        self.d_out = fill(cap + PAD, torch.uint8)
        self.d_cert = fill(8 + PAD, torch.int32)
        self.d_status = fill(16 + PAD, torch.int32)
        self.d_entries = fill(16 * ecap + PAD, torch.int32).view(-1, 4)
        self.d_n = fill(8 + PAD, torch.int64)
        self.d_work = fill(8 * ecap + PAD, torch.int64)
        self.d_moved = fill(8 * ecap + PAD, torch.int32).view(-1, 2) if want_moved else None
        self.d_usage = fill(32 * self.nvic + PAD, torch.int64) if want_usage else None
        self.d_sum = fill(SUMMARY.itemsize + PAD, torch.int64)
        self.batch = t.clean(victims, self.d_out, self.d_cert, self.d_status, self.d_entries[:ecap], self.d_n,
                             self.d_work, self.d_sum, moved=self.d_moved, usage=self.d_usage, out_capacity=cap)
        self.cap, self.ecap = cap, ecap

    def read(self):
        u8 = lambda x: None if x is None else x.cpu().numpy().view(np.uint8).reshape(-1)
        return _split(self, self.cap, self.ecap, self.nvic, u8(self.d_out), u8(self.d_cert), u8(self.d_status),
                      u8(self.d_entries), u8(self.d_n), u8(self.d_work), u8(self.d_moved), u8(self.d_usage),
                      u8(self.d_sum))


class Survivor:
    """The survivor batch as append_cases.Walked presents a walked one."""

    def __init__(self, g):
        self.d, self.cap, self.nseg = g.d_out, max(g.cap, 16), 1
        self.d_status, self.d_entries, self.d_n = g.d_status, g.d_entries[:g.ecap], g.d_n
        self.buf = np.zeros(self.cap, np.uint8)
        self.buf[:len(g.out)] = np.frombuffer(g.out, np.uint8)
        self.status, self.table = g.status, g.table


class DeviceTab(mc.DeviceTab):
    """A table on the device with its twin on the host: every clean is held
    against the twin's, byte for byte."""

    def __init__(self, drv, key_cap, max_batches):
        mc.DeviceTab.__init__(self, drv, key_cap, max_batches)
        self.host.__class__ = HostTab
        self.host.retired = self.retired = set()

    def clean_size_raw(self, victims, want_usage=True):
        import torch
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
        d_usage = fill(32 * len(victims) + PAD) if want_usage else None
        d_sum = fill(SUMMARY.itemsize + PAD)
        self.t.clean_size(victims, d_sum, usage=d_usage)
        self.drv.ctx.check()
        sm = d_sum.cpu().numpy().view(np.uint8)
        g = Got()
        g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
        assert (sm[SUMMARY.itemsize:] == FILL).all()
        g.usage = None
        if want_usage:
            us = d_usage.cpu().numpy().view(np.uint8)
            g.usage = us[:32 * len(victims)].view(USAGE)
            assert (us[32 * len(victims):] == FILL).all()
        h = self.host.clean_size_raw(victims, want_usage)
        assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
        assert not want_usage or lc.same(h.usage, g.usage), "host and device usage differ"
        return g

    def victim_tensors(self, victims):
        out = []
        for n in victims:
            a = self.added[n]
            out += [x for x in (a.w.d, a.w.d_status, a.w.d_entries, a.w.d_n, a.d_work, a.d_hash) if x is not None]
        return out

    def clean_raw(self, victims, cap, ecap, want_moved=True, scribble=True):
        import torch
        R = self.drv.ramcrc
        tensors = self.victim_tensors(victims)
        before = [x.clone() for x in tensors]
        g = Cleaned(self.drv.ctx, self.t, victims, cap, ecap, want_moved)
        try:
            self.drv.ctx.check()
            g.refused = False
        except R.RamcrcError as e:
            assert e.code == R.EREFUSED, e
            g.refused = True
        g.read()
        assert all(torch.equal(x, y) for x, y in zip(tensors, before)), "a victim's array was written"
        h = self.host.clean_raw(victims, cap, ecap, want_moved, scribble)   # (retires in the shared lists)
        assert h.refused == g.refused and h.batch == g.batch
        assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
        assert lc.same(h.usage, g.usage), "host and device usage differ"
        if g.summary["spoiled"]:
            return g
        assert h.out == g.out, ("host and device survivors differ", rd.first_difference(h.out, g.out))
        assert h.cert == g.cert and lc.same(h.status, g.status) and h.n == g.n
        assert lc.same(h.table, g.table), "host and device record tables differ"
        assert not want_moved or lc.same(h.moved, g.moved), "host and device old references differ"
        if want_moved:
            works = {n: self.added[n].d_work.cpu().numpy().view(np.uint64) for n in victims}
            old = np.array([works[int(b)][int(r)] for b, r in g.moved.tolist()], np.uint64)
            assert np.array_equal(g.work, old), "a survivor's work word is not its old slot"
        if scribble:
            for x in tensors:
                x.view(torch.uint8).fill_(FILL)
        a = tc.Added.__new__(tc.Added)
        a.w, a.d_work, a.d_hash, a.batch = Survivor(g), g.d_work, None, g.batch
        self.batches[-1] = a.w   # (the twin appended its own view of the same bytes)
        while len(self.added) < g.batch:
            self.added.append(None)
        self.added.append(a)
        return g

    def survivor_of(self, out, cert, cap):
        """The survivor walked and checked by ramcrc_replay_verify_device as one
        segment of `cap` bytes under the call's certificate."""
        import torch
        buf = np.zeros(cap, np.uint8)
        buf[:len(out)] = np.frombuffer(out, np.uint8)
        w = ac.Walked(self.drv.ctx, buf, np.array([cert], np.uint32), cap, 1)
        dc = torch.from_numpy(np.array([cert], np.uint32).view(np.int32)).cuda()
        st = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        crc = torch.zeros(max(1, w.d_entries.shape[0]), dtype=torch.int32, device="cuda")
        self.drv.ctx.replay_verify(w.d, cap, cap, 1, dc, st, w.d_entries.clone(), w.d_n.clone(), crc)
        self.drv.ctx.check()
        st = st.cpu().numpy().view(np.uint32)
        assert st[0, 0] == w.status[0, 0] and st[0, 2] == w.status[0, 2]
        return w, int(st[0, 3])

    def live_of(self, n):
        r = tc.Live(self.drv.ctx, self.t, self.added[n])
        recs = self.batches[n].table.shape[0]
        h = self.host.live_of(n)
        winner = r.winner_all[:recs].reshape(-1).view(tc.REF)
        assert np.array_equal(winner, h[0]) and r.live[:, 0].tolist() == h[1] and r.counts == h[2]
        return winner, r.live[:, 0].tolist(), r.counts

    def stats_now(self):
        s = tc.device_stats(self.drv.ctx, self.t)
        assert s == self.host.stats_now()
        return s

    def raises_on_live(self, n):
        import torch
        z = torch.zeros(64, dtype=torch.int64, device="cuda")
        try:
            self.t.live(n, z[:8].view(torch.int32).view(-1, 2), z[8:9], z[16:22])
        except self.drv.ramcrc.RamcrcError as e:
            return e.code == self.drv.ramcrc.EINVAL and self.host.raises_on_live(n)
        return False

    def einval_clean(self, victims):
        try:
            Cleaned(self.drv.ctx, self.t, victims, 4 * KiB, 64)
        except self.drv.ramcrc.RamcrcError as e:
            return e.code == self.drv.ramcrc.EINVAL and self.host.einval_clean(victims)
        return False


class DeviceDriver(mc.DeviceDriver):
    on_device = True

    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


# ------------------------------------------------------------- the properties
def absent_keys(tab, keys, key_cap):
    """Keys nobody carries, one of them on an occupied slot."""
    out = [(1, b"nobody has this key"), (77, b"")]
    if keys:
        out.append(lc.same_slot_absent(keys, int(rc_slots(key_cap))))
    return [k for k in out if k not in set(keys)]


def rc_slots(key_cap):
    s = 64
    while s < 2 * key_cap:
        s <<= 1
    return s


def check_answers(tab, model, key_cap, what=""):
    """P1's queries against the model: lookup, read, live, stats."""
    exp = model.results()
    keys = sorted(exp)
    keys = keys + absent_keys(tab, keys, key_cap)
    res = lc.lookup(tab, exp, keys, what=what + " lookup")
    rd.read(tab, (exp, model.payloads()), keys, what=what + " read")
    for n, b in enumerate(model.batches):
        if b is None:
            assert tab.raises_on_live(n), (what, "live on a cleaned batch", n)
            continue
        winner, live, counts = tab.live_of(n)
        e_winner, e_live = model.live(n)
        assert np.array_equal(winner, e_winner), (what, n, "winners")
        assert live == e_live, (what, n, "live list")
    assert tab.stats_now() == model.stats(), (what, tab.stats_now(), model.stats())
    return keys, res


def snapshot(tab, model, keys):
    """Everything the table answers, as bytes (P5: clean_size changes nothing)."""
    kb, q = segments.lookup_queries(keys)
    res, counts = tab.lookup_raw(kb, q)
    out = [res.tobytes(), str(sorted(tab.stats_now().items()))]
    for n, b in enumerate(model.batches):
        if b is not None:
            w, live, counts = tab.live_of(n)
            out += [w.tobytes(), str(live), str(sorted(counts.items()))]
    return out


def check_fresh(tab, model, drv, key_cap, survivor, ties):
    """P2: the remaining batches and the walked survivor, added to a fresh
    table in number order, answer every key with the same kind and version."""
    fresh = drv.table(key_cap, len(model.batches) + 1)
    try:
        for n, b in enumerate(model.batches[:-1]):
            if b is not None:
                fresh.add(b if not drv.on_device else tab.added[n].w)
        fresh.add(survivor)
        mine = model.results()
        keys = sorted(mine)
        kb, q = segments.lookup_queries(keys)
        res, _ = fresh.lookup_raw(kb, q)
        assert fresh.stats_now()["keys"] == len(keys), "the remaining log has other keys than the table"
        pays = model.payloads()
        for key, r in zip(keys, res):
            assert (int(r["kind"]), int(r["version"])) == (mine[key][3], mine[key][2]), key
            if not ties and mine[key][3] == lc.OBJECT:
                vo, vl = lc.value_range(pays[key])
                assert lc.value_bytes(fresh.batches, r) == pays[key][vo:vo + vl], key
    finally:
        fresh.close()


def bad_sources(oracle, sources, moved):
    """How many of the moved records fail the oracle's checksum pass where they
    lie in their victims (sources: batch number -> the batch): the clean moves
    entries byte for byte, so the survivor must have exactly as many."""
    total = 0
    for n, b in sources.items():
        rows = [r for v, r in moved.tolist() if v == n]
        if rows:
            total += oracle.verify_objects(b.buf, b.cap, np.ascontiguousarray(b.table[rows]), b.nseg)[0]
    return total


def one_more_add(tab, model, drv, w, what):
    """P4's last step: a batch that overwrites moved keys and a key that
    stayed (one by a tombstone of the winner's version) and brings a new key
    is resolved through the re-pointed picks and claims."""
    moved_keys = sorted({x[4] for x in w.live})
    stayed = sorted(k for k in model.win if k not in set(moved_keys))
    es = []
    for i, key in enumerate(moved_keys[-3:] + stayed[-1:]):
        ver = model.win[key][0]
        es.append(rc.tomb(key[0], key[1], ver) if i == 1 else rc.obj(key[0], key[1], ver + 1, b"after the clean"))
    es.append(rc.obj(9, b"new after clean %d" % len(model.batches), 1, b"n"))
    n = add(tab, model, drv.batch([es], cap=4 * KiB))
    check_answers(tab, model, tab.key_cap_, what + " after one more add")
    return n


def clean(tab, model, drv, victims, key_cap, cap=None, ecap=None, what="", ties=False, more=True, **kw):
    """One clean_size and one clean of `victims` against the model, with P1 to
    P5 around them; more: P4's further add (it takes the next batch number).
    cap, ecap: default exactly what clean_size says (cap rounded up to 16).
    Returns (the call's outputs, the Want)."""
    tab.key_cap_ = key_cap
    sources = {n: model.batches[n] for n in victims}
    before = model.results()
    keys, _ = check_answers(tab, model, key_cap, what + " before")
    snap = snapshot(tab, model, keys)
    ws = model.size(victims)
    gs = tab.clean_size_raw(victims)
    assert gs.summary == ws.summary, (what, "clean_size", gs.summary, ws.summary)
    assert lc.same(gs.usage, ws.usage), (what, "clean_size usage")
    assert snapshot(tab, model, keys) == snap, "clean_size changed the table"
    cap = -(-ws.summary["needed_bytes"] // 16) * 16 if cap is None else cap
    ecap = ws.summary["needed_records"] if ecap is None else ecap
    w = model.clean(drv.oracle, victims, cap, ecap)
    want_bad = bad_sources(drv.oracle, sources, w.moved) if w.fit else 0   # (before the victims are overwritten)
    g = tab.clean_raw(victims, cap, ecap, **kw)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert lc.same(g.usage, w.usage), (what, "usage")
    assert g.refused == (not w.fit)
    if not w.fit:
        return g, w
    assert g.batch == w.summary["batch"]
    assert g.out == w.out, (what, "survivor bytes", rd.first_difference(g.out, w.out))
    assert g.cert == w.cert, (what, "certificate against the oracle", g.cert, w.cert)
    assert lc.same(g.status, w.status) and g.n == len(w.live), (what, "status and count")
    assert lc.same(g.table, w.table), (what, "record table")
    assert g.moved is None or lc.same(g.moved, w.moved), (what, "old references")
    # P3: what the existing walk writes for d_out (one segment of out_capacity
    # bytes) under the certificate, and what the checksum pass finds there
    walked, bad = tab.survivor_of(g.out, g.cert, max(cap, 16))
    assert lc.same(walked.status[0, :3], g.status[0, :3]), (what, "the walk's status")
    assert lc.same(walked.table, g.table), (what, "the walk's record table")
    assert bad == want_bad, (what, "bad_objects of the survivor", bad, want_bad)
    g.bad_objects = bad
    check_fresh(tab, model, drv, key_cap, walked, ties)
    # P1 and P4: the answers are the same (the victims' arrays are 0xA5 by now)
    after = model.results()
    moved = {tuple(x): (g.batch, j) for j, x in enumerate(w.moved.tolist())}
    for key, r in before.items():
        want = moved.get(r[:2], r[:2]) + r[2:4]
        assert after[key][:4] == want, (what, key, "a key answers differently after the clean")
    check_answers(tab, model, key_cap, what + " after")
    if more:
        one_more_add(tab, model, drv, w, what)
    return g, w


def add(tab, model, b):
    n = tab.add(b)
    assert n == model.add(b), "the batch numbers of the table and the model differ"
    return n


# ---------------------------------------------------------------- scenarios
def relation_lists():
    """Four batches; one key per relation of winner and claimant to the
    victims {0, 2} (batches 1 and 3 stay)."""
    o, t, h = rc.obj, rc.tomb, tc.head
    b0 = [h(1),
          o(1, b"win and claim in victim 0", 5, b"v0"),
          o(1, b"claim in 0, winner stays in 1", 1, b"old"),
          o(1, b"claim in 0, winner in victim 2", 1, b"old"),
          o(1, b"victims only", 1, b"a"),
          o(1, b"removed: object in 0, winner tombstone in 2", 3, b"gone"),
          o(1, b"non-winner tombstone follows in 2", 9, b"stays the winner"),
          o(1, b"claim in 0, winner in 3", 2, b"old"),
          o(2, b"", 4, b"the empty key"),
          t(1, b"tombstone wins and moves", 6)]
    b1 = [h(2),
          o(1, b"claim in 0, winner stays in 1", 2, b"new in 1"),
          o(1, b"claim stays in 1, winner in victim 2", 1, b"old"),
          o(1, b"only in 1", 1, b"untouched")]
    b2 = [h(3),
          o(1, b"claim in 0, winner in victim 2", 2, b"new in 2"),
          o(1, b"victims only", 2, b"b"),
          t(1, b"removed: object in 0, winner tombstone in 2", 3),
          t(1, b"non-winner tombstone follows in 2", 8),
          o(1, b"claim stays in 1, winner in victim 2", 7, b"new in 2"),
          o(1, b"born in 2", 1, b"x" * 300)]
    b3 = [h(4),
          o(1, b"claim in 0, winner in 3", 3, b"new in 3"),
          o(1, b"only in 3", 1, b"")]
    return [b0, b1, b2, b3]


def case_relations(drv):
    key_cap = 64
    tab, model = drv.table(key_cap, 10), Model()
    try:
        for es in relation_lists():
            add(tab, model, drv.batch([es], cap=4 * KiB))
        g, w = clean(tab, model, drv, [0, 2], key_cap, what="relations", more=False)   # (the add below is this one's)
        sm = w.summary
        assert sm["moved_tombstones"] == 2 and sm["dropped_tombstones"] == 1 and sm["dropped_objects"] == 5
        assert sm["dropped_other"] == 2 and sm["moved_objects"] == 7 and sm["batch"] == 4
        # P4: one more batch overwrites a moved key, a key whose claim was re-pointed, and adds a new one
        more = [tc.head(5), rc.obj(1, b"win and claim in victim 0", 6, b"newer"),
                rc.tomb(1, b"claim in 0, winner in victim 2", 2), rc.obj(1, b"after the clean", 1, b"n"),
                rc.obj(1, b"victims only", 2, b"an equal version loses to the moved one")]
        add(tab, model, drv.batch([more], cap=4 * KiB))
        check_answers(tab, model, key_cap, "after one more add")
        # the survivor batch is a victim of a later clean, with a batch that stayed
        clean(tab, model, drv, [4, 1], key_cap, what="second clean", ties=True)
        left = [n for n, b in enumerate(model.batches) if b is not None]
        assert left == [3, 5, 6, 7]
        clean(tab, model, drv, [6, 3, 5, 7], key_cap, what="third clean, everything that is left", ties=True)
        assert model.stats()["batches"] == 10
    finally:
        tab.close()


def case_tile_edges(drv):
    """TILE - 1, TILE and TILE + 1 survivors; a victim without a live record
    between two that have some; all live; none live."""
    key_cap = 2048
    for nlive in (TILE - 1, TILE, TILE + 1):
        tab, model = drv.table(key_cap, 8), Model()
        try:
            first = [rc.obj(3, b"k%04d" % i, 1, b"v%d" % i) for i in range(nlive)]
            dead = [rc.obj(4, b"d%04d" % i, 1, b"dead") for i in range(300)]
            last = [rc.obj(3, b"z%04d" % i, 1, b"") for i in range(3)]
            kill = [rc.tomb(4, b"d%04d" % i, 1) for i in range(300)]
            for es in (first, dead, last, kill):
                add(tab, model, drv.batch([es], cap=32 * KiB))
            g, w = clean(tab, model, drv, [0, 1, 2], key_cap, what="tile edge %d" % nlive, more=False)
            assert int(w.usage["records"][0]) == int(w.usage["live_objects"][0]) == nlive
            assert w.summary["needed_records"] == nlive + 3 and int(w.usage["live_objects"][1]) == 0
            assert w.summary["dropped_objects"] == 300
            # all live: the survivor and the tombstones
            g, w = clean(tab, model, drv, [4, 3], key_cap, what="all live")
            assert w.summary["needed_records"] == w.summary["records"] == nlive + 303
        finally:
            tab.close()
    tab, model = drv.table(key_cap, 8), Model()
    try:
        add(tab, model, drv.batch([[tc.head(1)] + [rc.obj(3, b"k%d" % i, 1, b"v") for i in range(5)]], cap=4 * KiB))
        add(tab, model, drv.batch([[rc.tomb(3, b"k%d" % i, 1) for i in range(5)]], cap=4 * KiB))
        g, w = clean(tab, model, drv, [0], key_cap, what="none live")
        assert g.out == b"" and g.n == 0 and w.summary["needed_bytes"] == 0
        assert g.cert == ac.expected_cert(drv.oracle, b""), "the certificate of an empty segment"
        clean(tab, model, drv, [2, 1], key_cap, what="an empty survivor as a victim")
    finally:
        tab.close()


def shape_lists():
    """Victim entries whose live records meet every source offset mod 16 with
    every destination offset mod 16, and payloads of one, two and three length
    bytes; the dead records are killed by a later batch."""
    es, kill = [], []
    src = dst = 0
    n = 0

    def sized(table, key, size, version=1):
        """An object entry of exactly `size` bytes."""
        base = len(rc.obj(table, key, version, b""))
        e = rc.obj(table, key, version, b"\x5a" * (size - base))
        if len(e) != size:   # (the value crossed a length-byte boundary)
            e = rc.obj(table, key, version, b"\x5a" * (size - base - (len(e) - size)))
        assert len(e) == size, (len(e), size)
        return e

    for s in range(16):
        for d in range(16):
            # a live record that brings dst to d, a dead one that brings src to s
            e = sized(5, b"pad%03d" % n, 48 + (d - dst - 48) % 16)
            es.append(e)
            src += len(e)
            dst += len(e)
            e = sized(6, b"dead%03d" % n, 48 + (s - src - 48) % 16)
            es.append(e)
            kill.append(rc.tomb(6, b"dead%03d" % n, 1))
            src += len(e)
            assert src % 16 == s and dst % 16 == d
            e = sized(7, b"live%03d" % n, 40 + (n * 7) % 90)
            es.append(e)
            src += len(e)
            dst += len(e)
            n += 1
    big = []
    for ln in (255, 256, 65535, 65536):
        pay = pc.obj(8, b"L%d" % ln, b"", version=1)
        big.append(pc.entry(OBJ, pay + bytes((i * 31 + ln) & 0xFF for i in range(ln - len(pay)))))
        big.append(rc.tomb(8, b"T%d" % ln, ln))
    big.append(pc.entry(OBJ, b""))                       # payload length 0: malformed, dropped
    big.append(ac.raw_entry(OBJ, pc.obj(8, b"wide length", b"three length bytes for 60", version=1), 3))
    return es, kill, big


def case_entry_shapes(drv):
    key_cap = 2048
    cap = 256 * KiB
    tab, model = drv.table(key_cap, 8), Model()
    try:
        es, kill, big = shape_lists()
        add(tab, model, drv.batch([es], cap=cap))
        add(tab, model, drv.batch([big], cap=cap))
        add(tab, model, drv.batch([kill], cap=cap))
        g, w = clean(tab, model, drv, [0, 1], key_cap, what="entry shapes")
        pairs = set()
        for (n, r), row in zip(w.moved.tolist(), w.table.tolist()):
            if n == 0:
                pairs.add((int(model_offset(es, r)) % 16, row[1] % 16))
        assert len(pairs) == 256, "not every source residue met every destination residue"
        assert w.summary["dropped_other"] == 1 and w.summary["dropped_objects"] == 256
        assert sorted({(row[3] >> 6) + 1 for row in w.table.tolist()}) == [1, 2, 3]
    finally:
        tab.close()


def model_offset(es, r):
    return sum(len(e) for e in es[:r])


def case_non_participants(drv):
    """Safe versions, transaction records, malformed records and the records
    of a segment without RAMCRC_SEG_OK are dropped_other."""
    key_cap = 64
    tab, model = drv.table(key_cap, 4), Model()
    try:
        good = [tc.head(1), pc.entry(pc.SAFEVERSION, pc.safe_version(41)), rc.obj(1, b"a", 1, b"va"),
                pc.entry(pc.PREP, pc.prep(1, b"p")), pc.entry(pc.TXDECISION, pc.tx_decision(1, 5)),
                pc.entry(pc.RPCRESULT, pc.rpc_result(1, 5)), pc.entry(pc.TXPLIST, pc.tx_plist([(1, 5, 0)])),
                pc.entry(pc.PREPTOMB, pc.prep_tomb(1, 5)), pc.entry(OBJ, b"short"), pc.entry(OBJTOMB, b"x" * 31),
                rc.tomb(1, b"b", 2)]
        bad = [tc.head(2), rc.obj(1, b"in a bad segment", 9, b"never seen")]
        add(tab, model, drv.batch([good, bad], cap=4 * KiB, bad=(1,)))
        g, w = clean(tab, model, drv, [0], key_cap, what="non-participants")
        assert w.summary["dropped_other"] == 11 and w.summary["records"] == 13
        assert w.summary["moved_objects"] == 1 and w.summary["moved_tombstones"] == 1
        assert model.stats()["safe_version"] == 41
    finally:
        tab.close()


def case_space(drv):
    """Exact capacities fit (every clean() above); 16 bytes short and one
    record short spoil the table and write nothing; a reset revives it."""
    key_cap = 64
    es = [[tc.head(1)] + [rc.obj(1, b"key %d" % i, 1, b"value %d" % i) for i in range(20)],
          [rc.obj(1, b"key 3", 2, b"newer")]]
    for short in ("bytes", "records"):
        tab, model = drv.table(key_cap, 4), Model()
        try:
            for e in es:
                add(tab, model, drv.batch([e], cap=4 * KiB))
            ws = model.size([0])
            need, recs = ws.summary["needed_bytes"], ws.summary["needed_records"]
            assert recs == 19
            cap = -(-need // 16) * 16
            cap, ecap = (cap - 16, recs) if short == "bytes" else (cap, recs - 1)
            g, w = clean(tab, model, drv, [0], key_cap, cap=cap, ecap=ecap, what="short of " + short)
            assert g.refused and g.summary == dict(SPOILED_SUMMARY, needed_bytes=need, needed_records=recs)
            assert (g.out_all == FILL).all() and (g.entries_all == FILL).all() and (g.work_all == FILL).all()
            # spoiled: a clean writes only its summary, and still takes its number
            g2 = tab.clean_raw([1], 4 * KiB, 64)
            assert g2.summary == SPOILED_SUMMARY and g2.batch == 3 and not g2.refused
            assert (g2.usage_all == FILL).all() and (g2.out_all == FILL).all()
            s = tab.clean_size_raw([2])
            assert s.summary == SPOILED_SUMMARY and (np.ascontiguousarray(s.usage).view(np.uint8) == FILL).all()
            tab.reset()
            tab.retired.clear()
            model = Model()
            for e in es:
                add(tab, model, drv.batch([e], cap=4 * KiB))
            clean(tab, model, drv, [0], key_cap, what="after the reset")
        finally:
            tab.close()


def case_handle_state(drv):
    """The RAMCRC_EINVAL of rule 1, live on a cleaned batch, and the numbers
    running out at max_batches."""
    key_cap = 64
    R = drv.ramcrc
    tab, model = drv.table(key_cap, 4), Model()
    try:
        for i in range(3):
            add(tab, model, drv.batch([[tc.head(i), rc.obj(1, b"k", i + 1, b"v%d" % i)]], cap=4 * KiB))
        before = tab.stats_now()
        for victims in ([], [0, 0], [1, 2, 1], [3], [0xFFFFFFFF]):
            assert tab.einval_clean(victims), victims
            try:
                tab.clean_size_raw(victims)
                raise AssertionError("no RAMCRC_EINVAL for victims %r" % (victims,))
            except R.RamcrcError as e:
                assert e.code == R.EINVAL, victims
        assert tab.stats_now() == before
        clean(tab, model, drv, [0], key_cap, what="the last number", more=False)
        assert tab.raises_on_live(0)
        assert tab.einval_clean([0]) and tab.einval_clean([1, 0]), "a cleaned batch was taken as a victim again"
        try:
            tab.clean_size_raw([0])
            raise AssertionError("a cleaned batch was sized as a victim again")
        except R.RamcrcError as e:
            assert e.code == R.EINVAL
        # max_batches numbers are in use: clean_size still answers, clean does not
        s = tab.clean_size_raw([1, 2])
        assert s.summary == model.size([1, 2]).summary
        assert tab.einval_clean([1]), "a fifth number was given out"
        check_answers(tab, model, key_cap, "after the refused calls")
        assert tab.stats_now()["batches"] == 4
    finally:
        tab.close()


def case_many_victims(drv):
    """More victims than one launch of the victim list carries (384), in a
    shuffled order, some of them without a record."""
    nb, key_cap = 392, 1024
    tab, model = drv.table(key_cap, nb + 2), Model()
    try:
        for i in range(nb):
            es = [] if i % 50 == 7 else [rc.obj(2, b"key %d" % (i % 300), 1 + i // 300, b"value %d" % i)]
            add(tab, model, drv.batch([es], cap=256))
        order = np.random.default_rng(4).permutation(nb).tolist()
        victims = [b for b in order if b not in (3, 391)]
        assert len(victims) > 384
        g, w = clean(tab, model, drv, victims, key_cap, what="many victims")
        assert w.summary["victims"] == nb - 2 and w.summary["dropped_objects"] > 80
        assert [int(x) for x in w.moved["batch"]] == [b for b in victims if int(w.usage["live_objects"][victims.index(b)])]
    finally:
        tab.close()


def case_closing_the_loop(drv, mixed):
    """Replicas, adds, write, walk, add, remove, walk, add; clean_size; clean of
    every batch but the last; read; a write over a moved key and over a removed
    key; a second clean whose victims include the first survivor."""
    key_cap = 2000
    tab, model = drv.table(key_cap, len(mixed) + 8), Model()
    try:
        for b in mixed:
            add(tab, model, b)
        exp = model.results()
        live_keys = [k for k in sorted(exp) if exp[k][3] == lc.OBJECT]
        objs = [(tid, key, b"rewritten %d" % n) for n, (tid, key) in enumerate(live_keys[::4])]
        gw, ww = wc.write(tab, exp, objs, what="write", next_version=1 << 20)
        assert ww.summary["ok"] == len(objs)
        bw, bad = tab.batch_of(gw.out, gw.cert)
        assert bad == 0
        add(tab, model, bw)
        exp = model.results()
        gone = live_keys[1::4]
        gr, wr = mc.remove(tab, exp, gone, what="remove", next_version=1 << 21)
        assert wr.summary["removed"] == len(gone)
        br, bad = tab.batch_of(gr.out, gr.cert)
        assert bad == 0
        last = add(tab, model, br)
        victims = list(range(last))
        g, w = clean(tab, model, drv, victims, key_cap, what="loop", cap=mixed[0].cap)
        assert w.summary["moved_objects"] > len(objs) and w.summary["dropped_tombstones"] > 0
        # (clean() held the survivor's bad_objects against the victims' own.)  The
        # objects the write made carry their checksums and keep them through the move
        assert g.bad_objects <= w.summary["needed_records"] - len(objs)
        exp = model.results()
        moved_key, removed_key = live_keys[0], gone[0]
        assert exp[moved_key][0] == g.batch and exp[removed_key][3] == lc.TOMBSTONE
        nv = 5
        gw, ww = wc.write(tab, exp, [moved_key + (b"over a moved key",), removed_key + (b"over a removed key",)],
                          what="write after the clean", next_version=nv)
        tv = exp[removed_key][2]
        assert ww.versions[0] == exp[moved_key][2] + 1, "old plus one"
        assert ww.versions[1] > tv and ww.versions[1] in (max(nv, tv + 1), max(nv + 1, tv + 1)), "above the tombstone"
        bw, bad = tab.batch_of(gw.out, gw.cert)
        nw = add(tab, model, bw)
        check_answers(tab, model, key_cap, "after the second write")
        clean(tab, model, drv, [g.batch, last], key_cap, what="second clean", cap=mixed[0].cap)
        assert model.batches[nw] is not None
    finally:
        tab.close()
