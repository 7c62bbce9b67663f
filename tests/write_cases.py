"""Requests, cases and the expectation for the replay table's multi-write
(ramcrc_replay_table_write_host / _device).

The expectation is plain Python: the loop of include/ramcrc.h over
lookup_cases.expectation (the plain-Python replay of the added batches), with
CRCs from the oracle.  It is held against tests/golden/multi_write_ref.json
before any library call.  The scenarios run unchanged on the host and on the
device: a driver makes batches and tables; a table adds, looks up, reads and
writes; the output of a write is walked with its certificate and added as the
next batch.  Every output is pre-filled with 0xA5 and checked past its end.
"""
import ctypes

import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import lookup_cases as lc
import partition_cases as pc
import read_cases as rd
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
FILL, FILL32 = rd.FILL, rd.FILL32
M64 = (1 << 64) - 1
NONE = segments.WRITE_REF_NONE
REQ, PART, REF = segments.WRITE_REQ_DTYPE, segments.WRITE_PART_DTYPE, segments.WRITE_REF_DTYPE
SUMMARY = segments.WRITE_SUMMARY_DTYPE
SUMMARY_NAMES = SUMMARY.names
OK, DOESNT_EXIST, EXISTS, WRONG_VERSION, FORMAT_ERROR = (rd.OK, rd.DOESNT_EXIST, rd.EXISTS,
                                                         rd.WRONG_VERSION, rd.FORMAT_ERROR)
RETRY = segments.STATUS_RETRY
STATUS_FIELD = {DOESNT_EXIST: "doesnt_exist", EXISTS: "object_exists", WRONG_VERSION: "wrong_version"}
SPOILED_SUMMARY = dict(dict.fromkeys(SUMMARY_NAMES, 0), spoiled=1)
TS = 0x5EC0D5A7       # the timestamp of every write below
PAD = 64              # bytes of 0xA5 behind every output
OUT_CAP = 256 * KiB   # the output's allocation where a case does not size it


# ---------------------------------------------------------- the expectation
def first_key(img):
    """(offset, length) of the first key in a keysAndValue image, or None for
    an image ramcrc_part::parse would not take behind a 24-byte header."""
    if len(img) < 1:
        return None
    nk = img[0]
    if nk == 0:
        return 1, 0
    if len(img) < 3:
        return None
    kl = int.from_bytes(img[1:3], "little")
    off = 1 + 2 * nk
    return (off, kl) if off + kl <= len(img) else None


def value_len(img):
    return lc.value_range(bytes(24) + bytes(img))[1]


def object_entry(oracle, table_id, version, ts, img):
    body = ts.to_bytes(4, "little") + version.to_bytes(8, "little") + table_id.to_bytes(8, "little") + img
    return ac.raw_entry(pc.OBJ, oracle.crc32c(np.frombuffer(body, np.uint8)).to_bytes(4, "little") + body)


def tombstone_entry(oracle, table_id, segment_id, version, ts, key):
    head = table_id.to_bytes(8, "little") + segment_id.to_bytes(8, "little") + \
        version.to_bytes(8, "little") + ts.to_bytes(4, "little")
    ck = oracle.crc32c(np.frombuffer(head + key, np.uint8))
    return ac.raw_entry(pc.OBJTOMB, head + ck.to_bytes(4, "little") + key)


class Want:
    """What a write of (data, reqs) must produce against the lookup
    expectation `exp` (key -> LOOKUP_RESULT tuple)."""

    def __init__(self, oracle, exp, data, reqs, rules=None, next_version=1, ts=TS, seg_ids=None,
                 cap=OUT_CAP):
        data = bytes(np.ascontiguousarray(data, np.uint8))
        n = reqs.shape[0]
        self.parts = np.zeros(n, PART)
        self.refs = np.zeros(n, REF)
        self.old = np.zeros(n, lc.RES)
        self.versions = {}   # request -> the written version
        sm = dict.fromkeys(SUMMARY_NAMES, 0)
        out, seen, top, is_open = bytearray(), set(), 0, True
        for i in range(n):
            table_id, off, ln, reserved = (int(x) for x in reqs[i])
            r = (rules[i] if rules is not None else None) or {}
            status, version, ref, res, key = FORMAT_ERROR, 0, (NONE, NONE), lc.no_result(lc.BAD_KEY), None
            if not (reserved or r.get("reserved") or off + ln > len(data) or 24 + ln > 0xFFFFFFFF):
                img = data[off:off + ln]
                key = first_key(img)
            if key is None:
                sm["bad"] += 1
            else:
                kb = img[key[0]:key[0] + key[1]]
                res = exp.get((table_id, kb), lc.no_result(lc.ABSENT))
                if (table_id, kb) in seen:
                    status = RETRY
                    sm["retry_duplicate"] += 1
                else:
                    seen.add((table_id, kb))
                    cur = res[2] if res[3] == lc.OBJECT else 0
                    status, version = rd.reject(r, cur), cur
                    if status != OK:
                        sm[STATUS_FIELD[status]] += 1
                    else:
                        a = (next_version + sm["allocated"]) & M64
                        if cur:
                            v = (cur + 1) & M64
                        else:
                            v = (res[2] + 1) & M64 if res[3] == lc.TOMBSTONE and res[2] >= a else a
                            sm["allocated"] += 1
                            if v != a:
                                top = max(top, (v + 1) & M64)
                        blob = object_entry(oracle, table_id, v, ts, img)
                        t_at = len(out) + len(blob)
                        if cur:
                            seg_id = 0 if seg_ids is None else (int(seg_ids[res[0]]) + res[4]) & M64
                            blob += tombstone_entry(oracle, table_id, seg_id, cur, ts, kb)
                        if is_open and len(out) + len(blob) <= cap:
                            ref = (len(out), t_at if cur else NONE)
                            out += blob
                            vl = value_len(img)
                            sm["ok"] += 1
                            sm["tombstones"] += 1 if cur else 0
                            sm["value_bytes"] += vl
                            sm["key_bytes"] += ln - vl
                            sm["object_bytes"] += 24 + ln
                            sm["tombstone_bytes"] += 32 + len(kb) if cur else 0
                            version = v
                            self.versions[i] = v
                        else:
                            is_open = False
                            status = RETRY
                            sm["retry_full"] += 1
            self.parts[i] = (status, version)
            self.refs[i] = ref
            self.old[i] = res
        sm["out_bytes"] = len(out)
        sm["next_version"] = max((next_version + sm["allocated"]) & M64, top)
        self.out = bytes(out)
        self.cert = ac.expected_cert(oracle, self.out)
        self.summary = sm


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


# ------------------------------------------------------------------ drivers
class Got:
    """The outputs of one write, read back."""


def _check_got(g, n, cap):
    assert (g.out_all[min(g.summary["out_bytes"], cap):] == FILL).all(), "a byte at or past the head was written"
    assert (g.parts_past == FILL).all(), "a part past the requests was written"
    assert g.refs_past is None or (g.refs_past == FILL).all(), "a reference past the requests was written"
    assert g.old_past is None or (g.old_past == FILL).all(), "a result past the requests was written"
    assert (g.summary_past == FILL).all() and (g.cert_past == FILL).all(), "a word past a record was written"


def _split(g, n, cap, out, cert, parts, refs, old, sm):
    g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
    g.summary_past = sm[SUMMARY.itemsize:]
    g.out_all = out
    g.out = out[:min(g.summary["out_bytes"], out.size)].tobytes()
    g.cert = tuple(int(x) for x in cert[:8].view(np.uint32))
    g.cert_past = cert[8:]
    g.parts, g.parts_past = parts[:12 * n].view(PART), parts[12 * n:]
    g.refs = g.refs_past = g.old = g.old_past = None
    if refs is not None:
        g.refs, g.refs_past = refs[:8 * n].view(REF), refs[8 * n:]
    if old is not None:
        g.old, g.old_past = old[:32 * n].view(lc.RES), old[32 * n:]
    return g


def _room(n, cap):
    return min(cap, OUT_CAP if cap > (1 << 31) else cap)


class HostTab(rd.HostTab):
    def write_raw(self, data, reqs, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                  want_refs=True, want_old=True, shift=0, room=None):
        """The call itself, on pre-filled arrays (the wrapper allocates its own:
        case_goldens goes through it)."""
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        fill = lambda k: np.full(k, FILL, np.uint8)
        data = np.ascontiguousarray(data, np.uint8)
        raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(-1).copy()
        rl = segments.read_rules(rules).view(np.uint8).reshape(-1).copy() if rules is not None and n else None
        hs = np.ascontiguousarray(hashes, np.uint64) if hashes is not None else None
        sg = np.ascontiguousarray(seg_ids, np.uint64) if seg_ids is not None else None
        out, cert, parts = fill(room + PAD + shift)[shift:], fill(8 + PAD), fill(12 * n + PAD)
        refs = fill(8 * n + PAD) if want_refs else None
        old = fill(32 * n + PAD) if want_old else None
        sm = fill(SUMMARY.itemsize + PAD)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None
        L = self.drv.ramcrc.lib()
        self.drv.ramcrc._check(L.ramcrc_replay_table_write_host(
            self.t._h, p(data), data.size, p(raw), n, p(hs), p(rl), next_version, ts, p(sg), p(out), cap,
            p(cert), p(parts), p(refs), p(old), p(sm)), "ramcrc_replay_table_write_host")
        g = _split(Got(), n, cap, out, cert, parts, refs, old, sm)
        if not g.summary["spoiled"]:
            _check_got(g, n, cap)
        return g

    def batch_of(self, out, cert):
        """The output of a write as the next batch: walked with its certificate."""
        cap = self.batches[0].cap if self.batches else 64 * KiB   # (the expectation takes one stride)
        assert len(out) <= cap
        b = tc.HostBatch.__new__(tc.HostBatch)
        b.buf = np.zeros(cap, np.uint8)
        b.buf[:len(out)] = np.frombuffer(out, np.uint8)
        b.certs = np.array([cert], np.uint32)
        b.status, b.table = ac.host_walk(self.drv.oracle, b.buf, b.certs, 1, cap)
        b.cap, b.nseg = cap, 1
        bad, _, _ = self.drv.oracle.verify_objects(b.buf, cap, b.table, 1)
        return b, bad


class HostDriver(rd.HostDriver):
    def table(self, key_cap, max_batches):
        return HostTab(self, key_cap, max_batches)


class Written:
    """One ramcrc_replay_table_write_device call: every output pre-filled with
    0xA5 and longer than the call may write; the output starts `shift` bytes
    into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, data, reqs, cap, room, next_version=1, ts=TS, rules=None, hashes=None,
                 seg_ids=None, want_refs=True, want_old=True, shift=0, check=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.n = n = reqs.shape[0]
        self.cap = cap
        data = np.ascontiguousarray(data, np.uint8)
        self.d_data = torch.from_numpy(data).cuda() if data.size else None
        raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(-1)
        self.d_q = torch.from_numpy(raw.copy()).cuda().view(torch.int64) if n else None
        self.d_rules = None
        if rules is not None and n:
            rl = segments.read_rules(rules).view(np.uint8).reshape(-1)
            self.d_rules = torch.from_numpy(rl.copy()).cuda().view(torch.int64)
        u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()
        self.d_hash = u64(hashes) if hashes is not None else None
        self.d_seg = u64(seg_ids) if seg_ids is not None else None
        self.d_out = fill(room + PAD + shift, torch.uint8)[shift:]
        self.d_cert = fill(8 + PAD, torch.int32)
        self.d_parts = fill(12 * n + PAD, torch.int32)
        self.d_refs = fill(8 * n + PAD, torch.int32) if want_refs else None
        self.d_old = fill(32 * n + PAD, torch.int32) if want_old else None
        self.d_sum = fill(SUMMARY.itemsize + PAD, torch.int64)
        t.write(self.d_data, self.d_q, self.d_out if room + PAD + shift > shift else None, self.d_cert,
                self.d_parts, self.d_sum, next_version, ts, rules=self.d_rules, key_hash=self.d_hash,
                batch_segment_id=self.d_seg, refs=self.d_refs, old=self.d_old, data_bytes=data.size,
                n_reqs=n, out_capacity=cap)
        if check:
            ctx.check()
            self.read()

    def read(self):
        u8 = lambda x: None if x is None else x.cpu().numpy().view(np.uint8).reshape(-1)
        _split(self, self.n, self.cap, u8(self.d_out), u8(self.d_cert), u8(self.d_parts), u8(self.d_refs),
               u8(self.d_old), u8(self.d_sum))


class DeviceTab(rd.DeviceTab):
    """A table on the device with its twin on the host: every write is held
    against the twin's, byte for byte."""

    def __init__(self, drv, key_cap, max_batches):
        rd.DeviceTab.__init__(self, drv, key_cap, max_batches)
        self.host.__class__ = HostTab

    def write_raw(self, data, reqs, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                  want_refs=True, want_old=True, shift=0, room=None):
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        g = Written(self.drv.ctx, self.t, data, reqs, cap, room, next_version, ts, rules, hashes, seg_ids,
                    want_refs, want_old, shift)
        if g.summary["spoiled"]:
            return g
        _check_got(g, n, cap)
        h = self.host.write_raw(data, reqs, cap, next_version, ts, rules, hashes, seg_ids, want_refs,
                                want_old, room=room)
        assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
        assert h.out == g.out, ("host and device outputs differ", rd.first_difference(h.out, g.out))
        assert h.cert == g.cert, ("host and device certificates differ", h.cert, g.cert)
        assert lc.same(h.parts, g.parts), "host and device parts differ"
        assert not want_refs or lc.same(h.refs, g.refs), "host and device references differ"
        assert not want_old or lc.same(h.old, g.old), "host and device old results differ"
        return g

    def batch_of(self, out, cert):
        """The output as the next batch: ramcrc_replay_verify_device with the
        call's certificate."""
        import torch
        cap = self.batches[0].cap if self.batches else 64 * KiB   # (the expectation takes one stride)
        assert len(out) <= cap
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


class DeviceDriver(rd.DeviceDriver):
    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


def write(tab, exp, objects, what="", align=1, shift=0, packed=None, cap=OUT_CAP, next_version=1,
          rules=None, seg_ids=None, **kw):
    """The write of `objects` ((table id, keys, value) each) against the lookup
    expectation; `packed`: the (data buffer, requests) to send instead.  The
    old results are held against a lookup's, bit for bit.  Returns (the call's
    outputs, the Want)."""
    data, reqs = packed if packed is not None else segments.write_requests(objects, align)
    if shift:
        data = np.concatenate([np.full(shift, 0xEE, np.uint8), data])
        reqs = reqs.copy()
        reqs["data_off"] += shift
    w = Want(tab.drv.oracle, exp, data, reqs, rules, next_version, TS, seg_ids, cap)
    g = tab.write_raw(data, reqs, cap, next_version, TS, rules, seg_ids=seg_ids, **kw)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.out == w.out, (what, "output bytes", rd.first_difference(g.out, w.out))
    assert g.cert == w.cert, (what, "certificate", g.cert, w.cert)
    assert lc.same(g.parts, w.parts), (what, "parts", g.parts[:8], w.parts[:8])
    assert g.refs is None or lc.same(g.refs, w.refs), (what, "references")
    assert g.old is None or lc.same(g.old, w.old), (what, "old results")
    return g, w


def add_output(tab, g, w):
    """Walk the output with its certificate and add it as the next batch."""
    b, bad = tab.batch_of(g.out, g.cert)
    assert int(b.status[0, 0]) == segments.SEG_OK, "the certificate does not seal the output"
    assert b.table.shape[0] == w.summary["ok"] + w.summary["tombstones"] and bad == 0
    return tab.add(b)


def checked(tab):
    """The lookup expectation for the table as it stands, held against the
    live query's winners."""
    return lc.checked_expectation(tab)


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("multi_write_ref.json")


def check_expectation_against_golden(oracle, ref):
    """Every step of every golden scenario through the plain-Python
    expectation alone: a dict stands in for the table, as each step's entries
    are what the next step's lookup finds.  Returns how many steps."""
    steps = 0
    for sc in ref["scenarios"]:
        exp, batch = {}, 0
        for st in sc["steps"]:
            if "tombstone" in st:   # the scenario puts a tombstone into the table
                tid, key, ver = st["tombstone"]
                exp[(tid, key.encode())] = (batch, 0, ver, lc.TOMBSTONE, NONE, 0, 0)
                batch += 1
                continue
            objs = [(tid, key.encode(), value.encode()) for tid, key, value in st["objects"]]
            data, reqs = segments.write_requests(objs)
            w = Want(oracle, exp, data, reqs, st.get("rules"), st["next_version"])
            assert [int(x) for x in w.parts["status"]] == st["status"], (sc["name"], st)
            assert [int(x) for x in w.parts["version"]] == st["version"], (sc["name"], st)
            for name, v in st.get("summary", {}).items():
                assert w.summary[name] == v, (sc["name"], name, w.summary)
            if "entry_bytes" in st:
                sizes, at = [], 0
                while at < len(w.out):
                    lb = (w.out[at] >> 6) + 1
                    sizes.append(int.from_bytes(w.out[at + 1:at + 1 + lb], "little"))
                    at += 1 + lb + sizes[-1]
                assert sizes == st["entry_bytes"], (sc["name"], sizes)
            for i, (tid, key, value) in enumerate(objs):
                if i in w.versions:
                    exp[(tid, key)] = (batch, i, w.versions[i], lc.OBJECT, 0, 0, len(value))
            batch += 1
            steps += 1
    return steps


def case_goldens(drv):
    """Each step is one call followed by walk and add."""
    ref = golden()
    assert check_expectation_against_golden(drv.oracle, ref) == ref["steps"]
    for sc in ref["scenarios"]:
        tab = drv.table(64, 16)
        try:
            for st in sc["steps"]:
                if "tombstone" in st:
                    tid, key, ver = st["tombstone"]
                    tab.add(drv.batch([[tc.head(1), rc.tomb(tid, key.encode(), ver)]]))
                    continue
                exp = checked(tab) if tab.batches else {}
                objs = [(tid, key.encode(), value.encode()) for tid, key, value in st["objects"]]
                g, w = write(tab, exp, objs, what=sc["name"], rules=st.get("rules"),
                             next_version=st["next_version"])
                assert [int(x) for x in g.parts["status"]] == st["status"]
                assert [int(x) for x in g.parts["version"]] == st["version"]
                assert all(g.summary[k] == v for k, v in st.get("summary", {}).items())
                if g.summary["ok"]:
                    add_output(tab, g, w)
                    after = checked(tab)
                    for i, (tid, key, value) in enumerate(objs):
                        if i in w.versions:
                            res = after[(tid, key)]
                            assert res[2] == w.versions[i] and res[3] == lc.OBJECT
        finally:
            tab.close()
    # the wrapper, once: its own arrays, the same bytes
    if isinstance(drv, HostDriver) or not hasattr(drv, "ctx"):
        t = drv.ramcrc.ReplayTableHost(64, 2)
        try:
            data, reqs = segments.write_requests([(1, b"key0", b"item0"), (1, [b"a", b"bc"], b"v")])
            out, cert, parts, refs, old, sm = t.write(data, reqs, 4096, 7, TS, want_old=True)
            w = Want(drv.oracle, {}, data, reqs, None, 7, TS, None, 4096)
            assert out[:len(w.out)].tobytes() == w.out and not out[len(w.out):].any()
            assert (int(cert["head"]), int(cert["checksum"])) == w.cert and summary_dict(sm) == w.summary
            assert lc.same(parts, w.parts) and lc.same(refs, w.refs) and lc.same(old, w.old)
        finally:
            t.close()


# ------------------------------------------------------------ closing the loop
def mixed_requests(exp, seed=21):
    """Writes over lookup_cases.mixed_batches: every third key of the table
    (objects and tombstones), and as many new keys."""
    rng = np.random.default_rng(seed)
    keys = sorted(exp)[::3]
    objs = [(tid, key, rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes())
            for tid, key in keys]
    objs += [(5, b"new key %d" % n, b"value %d" % n) for n in range(len(keys))]
    order = rng.permutation(len(objs)).tolist()
    return [objs[i] for i in order]


def case_closing_the_loop(drv, mixed):
    tab = drv.table(2000, len(mixed) + 1)
    try:
        for b in mixed:
            tab.add(b)
        exp = checked(tab)
        before_live = [w.tolist() for w in tab.winners()]
        objs = mixed_requests(exp)
        seg_ids = 1000 * (1 + np.arange(len(mixed), dtype=np.uint64))
        g, w = write(tab, exp, objs, what="loop", next_version=1 << 40, seg_ids=seg_ids)
        assert w.summary["ok"] == len(objs) and 0 < w.summary["tombstones"] < len(objs)
        new_batch = add_output(tab, g, w)
        assert new_batch == len(mixed)
        after, pays = rd.checked(tab)
        written = {}
        for i, (tid, key, value) in enumerate(objs):
            written[(tid, key)] = (i, value)
            res = after[(tid, key)]
            # the new batch, d_refs' record, version v
            assert res[0] == new_batch and res[2] == w.versions[i] and res[3] == lc.OBJECT
            seg, off, ln, hdr = (int(x) for x in tab.batches[new_batch].table[res[1]])
            assert off == int(g.refs[i]["object_off"])
        for key, res in exp.items():
            if key not in written:
                assert after[key] == res, "a key the write did not name answers differently"
        keys = sorted(after)
        looked = lc.lookup(tab, after, keys, what="after the add")
        got, _ = rd.read(tab, (after, pays), keys, value_only=True, what="after the add")
        parts = segments.multi_read_parts(got.reply, got.summary["returned"])
        for key, res, (status, version, value) in zip(keys, looked, parts):
            if key in written:
                assert (status, version, value) == (OK, w.versions[written[key][0]], written[key][1])
                assert lc.value_bytes(tab.batches, res) == written[key][1]
        # the old batches' live lists no longer name the replaced objects
        replaced = {(exp[k][0], exp[k][1]) for k in written if k in exp}
        for j, win in enumerate(tab.winners()[:len(mixed)]):
            live = {(j, r) for r, (wb, wr) in enumerate(win.tolist()) if (wb, wr) == (j, r)}
            assert not (live & replaced)
            assert live == {(j, r) for r, (wb, wr) in enumerate(before_live[j]) if (wb, wr) == (j, r)} - replaced
    finally:
        tab.close()


# ---------------------------------------------------------------- the rules
GIVEN = rd.GIVEN


def case_reject_rules(drv):
    """Every rule against cur in {0 (absent), an object, 0 (a tombstone)}."""
    versions = rd.RULE_VERSIONS[1:]
    lists = [tc.head(1)] + [rc.obj(1, b"obj %d" % i, v, b"old") for i, v in enumerate(versions)]
    lists += [rc.tomb(1, b"tomb %d" % i, v) for i, v in enumerate(versions)]
    tab = drv.table(256, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        objs, rules = [], []
        for bits in range(16):
            r = {name: (bits >> k) & 1 for k, name in enumerate(rd.RULE_BITS)}
            r["given_version"] = GIVEN
            for i in range(len(versions)):
                for kind in ("obj", "tomb", "none"):
                    objs.append((1, b"%s %d" % (kind.encode(), i) + (b" r%d" % bits if kind == "none" else b""),
                                 b"new value"))
                    rules.append(dict(r))
            write(tab, exp, objs[-3 * len(versions):], what=("rules", bits),
                  rules=rules[-3 * len(versions):], next_version=GIVEN + 3)
        # non-boolean rule bytes, and rules given for some requests only
        objs = [(1, b"obj 1", b"x"), (1, b"obj 2", b"y"), (1, b"none", b"z")]
        g, w = write(tab, exp, objs, what="bytes",
                     rules=[dict(exists=0x80), None, dict(doesnt_exist=2)], next_version=9)
        assert [int(s) for s in g.parts["status"]] == [EXISTS, OK, DOESNT_EXIST]
    finally:
        tab.close()


# ----------------------------------------------------------------- versions
def case_versions(drv):
    nv = 1000
    lists = [tc.head(1)] + [rc.obj(1, b"have %d" % i, 10 + i, b"o") for i in range(6)]
    lists += [rc.tomb(1, b"late tomb", nv + 5), rc.tomb(1, b"early tomb", nv - 1), rc.tomb(1, b"edge tomb", nv + 2),
              rc.obj(1, b"version zero", 0, b"z"), rc.obj(1, b"top version", M64 - 1, b"t")]
    tab = drv.table(256, 3)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        # new keys interleaved with overwrites: consecutive allocated versions in request order
        objs = []
        for i in range(6):
            objs += [(1, b"fresh %d" % i, b"f"), (1, b"have %d" % i, b"h")]
        g, w = write(tab, exp, objs, what="interleaved", next_version=nv)
        assert [int(v) for v in g.parts["version"]] == [x for i in range(6) for x in (nv + i, 11 + i)]
        assert g.summary["allocated"] == 6 and g.summary["next_version"] == nv + 6
        # a tombstone winner at next_version + 5 forces v = tv + 1 and the summary's next_version;
        # one below next_version does not; the edge one meets a == tv after two allocations
        objs = [(1, b"fresh a", b""), (1, b"late tomb", b"l"), (1, b"early tomb", b"e"), (1, b"edge tomb", b"g"),
                (1, b"fresh b", b"")]
        g, w = write(tab, exp, objs, what="tombstones", next_version=nv)
        assert [int(v) for v in g.parts["version"]] == [nv, nv + 6, nv + 2, nv + 3, nv + 4]
        assert g.summary["allocated"] == 5 and g.summary["next_version"] == nv + 7
        assert g.summary["tombstones"] == 0
        add_output(tab, g, w)
        after = checked(tab)
        assert after[(1, b"late tomb")][2:4] == (nv + 6, lc.OBJECT)
        # an object winner of version 0 is VERSION_NONEXISTENT: allocated, no tombstone;
        # the version before the last
        objs = [(1, b"version zero", b"again"), (1, b"top version", b"up")]
        g, w = write(tab, after, objs, what="zero", next_version=3)
        assert [int(v) for v in g.parts["version"]] == [3, M64] and g.summary["tombstones"] == 1
        assert g.summary["allocated"] == 1
        rules = [dict(doesnt_exist=1), None]
        g, w = write(tab, after, objs, what="zero, rejected", next_version=3, rules=rules)
        assert [tuple(int(x) for x in p) for p in g.parts] == [(DOESNT_EXIST, 0), (OK, M64)]
    finally:
        tab.close()


# --------------------------------------------------------------- duplicates
def case_duplicates(drv):
    others = [(2, b"other %d" % i, b"v%d" % i) for i in range(24)]
    lists = [tc.head(1), rc.obj(1, b"hot", 4, b"old"), rc.obj(2, b"other 3", 8, b"old")]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        rng = np.random.default_rng(3)
        objs = [(1, b"hot", b"copy %d" % i) for i in range(1000)] + others
        order = rng.permutation(len(objs)).tolist()
        objs = [objs[i] for i in order]
        g, w = write(tab, exp, objs, what="hot")
        assert g.summary["ok"] == 25 and g.summary["retry_duplicate"] == 999 and g.summary["tombstones"] == 2
        first = next(i for i, o in enumerate(objs) if o[1] == b"hot")
        assert tuple(int(x) for x in g.parts[first]) == (OK, 5)
        # a first occurrence that is rejected: its copies still get RETRY
        objs = [(1, b"hot", b"a"), (1, b"hot", b"b"), (2, b"other 1", b"c"), (1, b"hot", b"d")]
        g, w = write(tab, exp, objs, what="rejected first", rules=[dict(exists=1), None, None, None])
        assert [tuple(int(x) for x in p) for p in g.parts] == [(EXISTS, 4), (RETRY, 0), (OK, 1), (RETRY, 0)]
        # a bad request does not count as a first
        data, reqs = segments.write_requests(objs)
        reqs["reserved"][0] = 1
        g, w = write(tab, exp, None, what="bad first", packed=(data, reqs))
        assert [tuple(int(x) for x in p) for p in g.parts] == [(FORMAT_ERROR, 0), (OK, 5), (OK, 1), (RETRY, 0)]
        # the same bytes under another table id, and a key that is a prefix, are other keys
        objs = [(1, b"hot", b""), (3, b"hot", b""), (1, b"ho", b""), (1, b"hot", b"")]
        g, w = write(tab, exp, objs, what="identity")
        assert [int(s) for s in g.parts["status"]] == [OK, OK, OK, RETRY]
    finally:
        tab.close()


# ------------------------------------------------------ sizes and alignment
OBJECT_PAYLOADS = [27, 28, 255, 256, 257, 65535, 65536, 70000]
KEY_LENGTHS = [0, 1, 223, 224, 65503]


def case_sizes(drv):
    """The length-byte steps of both entries, and the copy's size classes."""
    rng = np.random.default_rng(8)
    blob = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    keys = {kl: blob(kl) for kl in KEY_LENGTHS}
    lists = [tc.head(1)] + [rc.obj(1, k, 7, b"old") for k in keys.values()]
    pkey = lambda n: (b"k%d" % n)[:n - 27]   # (payload 27: one key, empty)
    lists += [rc.obj(2, pkey(n), 3, b"old") for n in OBJECT_PAYLOADS]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists], cap=512 * KiB))
        exp = checked(tab)
        objs = []
        for n in OBJECT_PAYLOADS:   # payload = 24 + 1 + 2 + key + value
            objs.append((2, pkey(n), blob(n - 27 - len(pkey(n)))))
        for kl, key in keys.items():
            objs.append((1, [key] if kl else [], blob(40)))
        objs += [(3, b"", blob(2047 - 3)), (3, b"x", blob(2048 - 4)), (3, b"y", blob(2049 - 4))]
        g, w = write(tab, exp, objs, what="sizes", cap=1 << 20, room=1 << 20)
        assert g.summary["ok"] == len(objs) and g.summary["tombstones"] == len(OBJECT_PAYLOADS) + len(KEY_LENGTHS)
        sizes = []
        at = 0
        while at < len(g.out):
            lb = (g.out[at] >> 6) + 1
            sizes.append(int.from_bytes(g.out[at + 1:at + 1 + lb], "little"))
            at += 1 + lb + sizes[-1]
        assert sizes[0:2 * len(OBJECT_PAYLOADS):2] == OBJECT_PAYLOADS
        assert {255, 256, 65535} <= set(sizes[1::2][len(OBJECT_PAYLOADS):len(OBJECT_PAYLOADS) + len(KEY_LENGTHS)])
        add_output(tab, g, w)
        checked(tab)
    finally:
        tab.close()


def case_alignment(drv):
    """data_off and the output head at every residue mod 16: the requests'
    sizes step the head through the residues, `shift` the data and the output
    allocation."""
    rng = np.random.default_rng(12)
    lists = [tc.head(1)] + [rc.obj(1, b"al %d" % i, 2, b"old") for i in range(0, 40, 2)]
    tab = drv.table(128, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        objs = [(1, b"al %d" % i, rng.integers(0, 256, 5 + (7 * i) % 90, dtype=np.uint8).tobytes())
                for i in range(40)]
        for shift in range(16):
            g, w = write(tab, exp, objs, what=("alignment", shift), shift=shift, seg_ids=[shift << 40])
            heads = {int(r["object_off"]) % 16 for r in g.refs} | {int(r["tombstone_off"]) % 16 for r in g.refs
                                                                   if int(r["tombstone_off"]) != NONE}
            assert shift or len(heads) == 16, heads
        for align in (4, 16):
            write(tab, exp, objs, what=("aligned", align), align=align)
    finally:
        tab.close()


def case_multi_key(drv):
    """The first key is the object's identity; the other keys are copied."""
    lists = [tc.head(1), lc.multi_obj(1, [b"first", b"second"], b"old", 6), rc.obj(1, b"second", 9, b"other")]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        objs = [(1, [b"first", b"2nd", b"third key"], b"new value"), (1, [b"second", b"first"], b"s"),
                (1, [b"", b"not empty"], b"e"), (1, [b"first", b"x"], b"dup")]
        g, w = write(tab, exp, objs, what="multi")
        assert [tuple(int(x) for x in p) for p in g.parts] == [(OK, 7), (OK, 10), (OK, 1), (RETRY, 0)]
        assert g.summary["key_bytes"] == sum(1 + 2 * len(k) + sum(map(len, k)) for _, k, _ in objs[:3])
        add_output(tab, g, w)
        after, pays = rd.checked(tab)
        got, _ = rd.read(tab, (after, pays), [(1, b"first"), (1, b"second"), (1, b"")], what="multi")
        parts = segments.multi_read_parts(got.reply, 3)
        assert [p[2] for p in parts] == [segments.keys_and_value(k, v) for _, k, v in objs[:3]]
    finally:
        tab.close()


# -------------------------------------------------------------------- space
def case_space(drv):
    lists = [tc.head(1)] + [rc.obj(1, b"sp %d" % i, 5, b"old") for i in range(0, 12, 2)]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        objs = [(1, b"sp %d" % i, b"v" * (10 + i)) for i in range(12)]
        objs.insert(9, (1, b"sp 0", b"a duplicate behind the cut"))
        data, reqs = segments.write_requests(objs)
        reqs["reserved"][12] = 3                                    # "sp 11": a bad request behind the cut
        rules = [None] * len(objs)
        rules[11] = dict(exists=1)                                  # "sp 10": rejected behind the cut
        full = Want(drv.oracle, exp, data, reqs, rules, 50)
        ends = sorted({int(r["object_off"]) for r in full.refs if int(r["object_off"]) != NONE} | {len(full.out)})
        t6 = int(full.refs[6]["tombstone_off"])
        assert t6 != NONE
        for cap in (ends[5], ends[5] - 1, t6 + 3, 0, len(full.out), len(full.out) - 1):
            g, w = write(tab, exp, None, what=("space", cap), packed=(data, reqs), rules=rules, cap=cap,
                         next_version=50)
            st = [int(s) for s in g.parts["status"]]
            assert st[9] == RETRY and st[11] == EXISTS and st[12] == FORMAT_ERROR
            assert tuple(int(x) for x in g.parts[11]) == (EXISTS, 5)
            if cap < len(full.out):
                assert g.summary["retry_full"] > 0
                assert g.summary["allocated"] == full.summary["allocated"], "allocateVersion runs before the space check"
            assert g.summary["ok"] + g.summary["retry_full"] == full.summary["ok"]
    finally:
        tab.close()


# ------------------------------------------------------------- bad requests
def case_bad_requests(drv):
    lists = [tc.head(1), rc.obj(1, b"good", 2, b"old")]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        good = (1, b"good", b"value")
        objs = [good] + [(1, b"key %d" % i, b"v") for i in range(12)] + [(1, [], b"no key")]
        data, reqs = segments.write_requests(objs)
        rules = [None] * len(objs)
        reqs["reserved"][1] = 1
        rules[2] = dict(reserved=1, exists=1)
        reqs["data_off"][3] = data.size - 3                  # runs 1 byte past the buffer
        reqs["data_off"][4] = M64 - 2                        # the sum overflows
        reqs["data_off"][5] = data.size + 1
        reqs["data_len"][6] = 0xFFFFFFFF - 23                # 24 + data_len does not fit 32 bits
        reqs["data_len"][7] = 0                              # data_len < 1
        reqs["data_len"][8] = 2                              # nk > 0 and data_len < 3
        reqs["data_len"][9] = 1 + 2 + 4                      # 1 + 2 nk + cum[0] > data_len by one
        tail = np.frombuffer(b"\x02\x03\x00\x04\x00abc", np.uint8)   # two keys, the first runs to the end: usable
        short = np.frombuffer(b"\x02\x03\x00\x04\x00ab", np.uint8)   # the first key is cut short
        reqs["data_off"][10], reqs["data_len"][10] = data.size, tail.size
        reqs["data_off"][11], reqs["data_len"][11] = data.size + tail.size, short.size
        data = np.concatenate([data, tail, short])
        reqs["data_off"][12], reqs["data_len"][12] = data.size - 1, 1   # the last byte: a key count of 'b'
        g, w = write(tab, exp, None, what="bad", packed=(data, reqs), rules=rules)
        st = [int(s) for s in g.parts["status"]]
        assert st == [OK] + [FORMAT_ERROR] * 9 + [OK, FORMAT_ERROR, FORMAT_ERROR, OK], st
        assert (g.parts["version"][1:10] == 0).all() and g.summary["bad"] == 11
        assert int(g.old[13]["kind"]) == lc.ABSENT and int(g.old[1]["kind"]) == lc.BAD_KEY
        # an empty data buffer: every request is bad or empty-keyed
        reqs = np.zeros(2, REQ)
        reqs["data_len"][1] = 1
        g, w = write(tab, exp, None, what="no data", packed=(np.zeros(0, np.uint8), reqs))
        assert [int(s) for s in g.parts["status"]] == [FORMAT_ERROR, FORMAT_ERROR]
    finally:
        tab.close()


# ------------------------------------------------------- nullable and empty
def case_nullable_and_empty(drv):
    lists = [tc.head(1), rc.obj(1, b"have", 2, b"old"), rc.obj(2, b"too", 3, b"old")]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        tab.add(drv.batch([[tc.head(2)], [tc.head(3), rc.obj(1, b"second", 1, b"old")]]))
        exp = checked(tab)
        objs = [(1, b"have", b"new"), (2, b"too", b"n"), (1, b"second", b"s"), (1, b"fresh", b"f")]
        # every nullable argument NULL, then all given
        g0, w0 = write(tab, exp, objs, what="all NULL", want_refs=False, want_old=False)
        hashes = np.array([pc.key_hash(t, k) for t, k, _ in objs], np.uint64)
        g1, w1 = write(tab, exp, objs, what="all given", rules=[None] * 4, hashes=hashes,
                       seg_ids=[0x1122334455667788, 7 << 32])
        assert g0.refs is None and g0.old is None and g0.out != g1.out and len(g0.out) == len(g1.out)
        # the segment id bytes of every tombstone: batch 0 segment 0, batch 0 segment 0, batch 1 segment 1
        ids = [int.from_bytes(g1.out[int(r["tombstone_off"]) + 2 + 8:][:8], "little") for r in g1.refs[:3]]
        assert ids == [0x1122334455667788, 0x1122334455667788, (7 << 32) + 1]
        assert all(int.from_bytes(g0.out[int(r["tombstone_off"]) + 2 + 8:][:8], "little") == 0 for r in w0.refs[:3])
        # no requests: a zeroed summary with next_version passed through, the certificate of an empty segment
        g, w = write(tab, exp, [], what="empty", next_version=77)
        assert g.summary == dict(dict.fromkeys(SUMMARY_NAMES, 0), next_version=77) and g.out == b""
        assert g.cert == ac.expected_cert(drv.oracle, b"")
        # next_version = 0
        data, reqs = segments.write_requests(objs)
        try:
            tab.write_raw(data, reqs, 4096, 0)
        except drv.ramcrc.RamcrcError as e:
            assert e.code == drv.ramcrc.EINVAL
        else:
            raise AssertionError("next_version = 0 was accepted")
    finally:
        tab.close()


def case_spoiled(drv):
    tab = drv.table(4, 2)
    try:
        b = drv.batch([tc.capacity_lists(8)])
        try:
            tab.add(b)
        except drv.ramcrc.RamcrcError:
            pass
        data, reqs = segments.write_requests([(1, b"k", b"v")])
        g = tab.write_raw(data, reqs, 4096)
        assert g.summary == SPOILED_SUMMARY
        for a in (g.out_all, g.cert_past, g.parts, g.parts_past, g.refs, g.old):
            assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all()
        assert all(x == FILL32 for x in g.cert)
    finally:
        tab.close()


# ---------------------------------------------------------------- read-only
def case_read_only(drv, mixed):
    tab = drv.table(2000, len(mixed))
    try:
        for b in mixed:
            tab.add(b)
        exp = checked(tab)
        before = tab.state()
        keys = sorted(exp)
        looked = lc.lookup(tab, exp, keys, what="before")
        write(tab, exp, mixed_requests(exp), what="read-only", next_version=9)
        assert tab.state() == before, "a write without an add changed the table"
        assert lc.same(lc.lookup(tab, exp, keys, what="after"), looked)
    finally:
        tab.close()
