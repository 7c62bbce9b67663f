"""Requests, cases and the expectation for the replay table's multi-remove
(ramcrc_replay_table_remove_host / _device).

The expectation is plain Python: the loop of include/ramcrc.h over
lookup_cases.expectation (the plain-Python replay of the added batches), with
CRCs from the oracle.  It is held against tests/golden/multi_remove_ref.json
before any library call.  The scenarios run unchanged on the host and on the
device: a driver makes batches and tables; a table adds, looks up, reads,
writes and removes; the output of a remove is walked with its certificate and
added as the next batch.  Every output is pre-filled with 0xA5 and checked
past its end.
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
import write_cases as wc

KiB = 1024
FILL, FILL32 = rd.FILL, rd.FILL32
M64 = (1 << 64) - 1
NONE = segments.REMOVE_REF_NONE
PART, SUMMARY = segments.REMOVE_PART_DTYPE, segments.REMOVE_SUMMARY_DTYPE
SUMMARY_NAMES = SUMMARY.names
OK, DOESNT_EXIST, EXISTS, WRONG_VERSION, FORMAT_ERROR = (rd.OK, rd.DOESNT_EXIST, rd.EXISTS,
                                                         rd.WRONG_VERSION, rd.FORMAT_ERROR)
RETRY = segments.STATUS_RETRY
STATUS_FIELD = {DOESNT_EXIST: "doesnt_exist", EXISTS: "object_exists", WRONG_VERSION: "wrong_version",
                OK: "ok_absent"}
SPOILED_SUMMARY = dict(dict.fromkeys(SUMMARY_NAMES, 0), spoiled=1)
TS = 0x7E40BE5D       # the timestamp of every remove below
PAD = 64              # bytes of 0xA5 behind every output
OUT_CAP = 256 * KiB   # the output's allocation where a case does not size it
LANE_KEY_MAX = 36     # dev_remove.inc: up to here a lane writes a tombstone, a group of 8 beyond


# ---------------------------------------------------------- the expectation
class Want:
    """What a remove of (key buffer, reqs) must produce against the lookup
    expectation `exp` (key -> LOOKUP_RESULT tuple)."""

    def __init__(self, oracle, exp, kb, reqs, rules=None, next_version=1, ts=TS, seg_ids=None, cap=OUT_CAP):
        kb = bytes(np.ascontiguousarray(kb, np.uint8))
        n = reqs.shape[0]
        self.parts = np.zeros(n, PART)
        self.refs = np.zeros(n, np.uint32)
        self.old = np.zeros(n, lc.RES)
        self.removed = {}   # request -> the removed version
        sm = dict.fromkeys(SUMMARY_NAMES, 0)
        out, seen, top, is_open = bytearray(), set(), 0, True
        for i in range(n):
            table_id, off, ln, reserved = (int(x) for x in reqs[i])
            r = (rules[i] if rules is not None else None) or {}
            status, version, ref, res = FORMAT_ERROR, 0, NONE, lc.no_result(lc.BAD_KEY)
            if ln > 65535 or reserved or r.get("reserved") or off > len(kb) or off + ln > len(kb):
                sm["bad"] += 1
            else:
                key = kb[off:off + ln]
                res = exp.get((table_id, key), lc.no_result(lc.ABSENT))
                if (table_id, key) in seen:
                    status = RETRY
                    sm["retry_duplicate"] += 1
                else:
                    seen.add((table_id, key))
                    found = res[3] == lc.OBJECT   # (the entry's type, not its version)
                    cur = res[2] if found else 0
                    status, version = rd.reject(r, cur), cur
                    if not found or status != OK:
                        sm[STATUS_FIELD[status]] += 1
                    else:
                        seg_id = 0 if seg_ids is None else (int(seg_ids[res[0]]) + res[4]) & M64
                        blob = wc.tombstone_entry(oracle, table_id, seg_id, cur, ts, key)
                        if is_open and len(out) + len(blob) <= cap:
                            ref = len(out)
                            out += blob
                            sm["removed"] += 1
                            sm["tombstone_bytes"] += 32 + ln
                            top = max(top, cur)
                            self.removed[i] = cur
                        else:
                            is_open = False
                            status = RETRY
                            sm["retry_full"] += 1
            self.parts[i] = (status, version)
            self.refs[i] = ref
            self.old[i] = res
        sm["out_bytes"] = len(out)
        sm["next_version"] = max(next_version, (top + 1) & M64)
        self.out = bytes(out)
        self.cert = ac.expected_cert(oracle, self.out)
        self.summary = sm


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


def entry_sizes(out):
    """The payload lengths of the entries of an output."""
    sizes, at = [], 0
    while at < len(out):
        lb = (out[at] >> 6) + 1
        sizes.append(int.from_bytes(out[at + 1:at + 1 + lb], "little"))
        at += 1 + lb + sizes[-1]
    return sizes


# ------------------------------------------------------------------ drivers
class Got:
    """The outputs of one remove, read back."""


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
        g.refs, g.refs_past = refs[:4 * n].view(np.uint32), refs[4 * n:]
    if old is not None:
        g.old, g.old_past = old[:32 * n].view(lc.RES), old[32 * n:]
    return g


class HostTab(wc.HostTab):
    def remove_raw(self, kb, reqs, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                   want_refs=True, want_old=True, shift=0, room=None):
        """The call itself, on pre-filled arrays (the wrapper allocates its own:
        case_goldens goes through it)."""
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        fill = lambda k: np.full(k, FILL, np.uint8)
        kb = np.ascontiguousarray(kb, np.uint8)
        raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(-1).copy()
        rl = segments.read_rules(rules).view(np.uint8).reshape(-1).copy() if rules is not None and n else None
        hs = np.ascontiguousarray(hashes, np.uint64) if hashes is not None else None
        sg = np.ascontiguousarray(seg_ids, np.uint64) if seg_ids is not None else None
        out, cert, parts = fill(room + PAD + shift)[shift:], fill(8 + PAD), fill(12 * n + PAD)
        refs = fill(4 * n + PAD) if want_refs else None
        old = fill(32 * n + PAD) if want_old else None
        sm = fill(SUMMARY.itemsize + PAD)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None
        L = self.drv.ramcrc.lib()
        self.drv.ramcrc._check(L.ramcrc_replay_table_remove_host(
            self.t._h, p(kb), kb.size, p(raw), n, p(hs), p(rl), next_version, ts, p(sg), p(out), cap,
            p(cert), p(parts), p(refs), p(old), p(sm)), "ramcrc_replay_table_remove_host")
        g = _split(Got(), n, cap, out, cert, parts, refs, old, sm)
        if not g.summary["spoiled"]:
            _check_got(g, n, cap)
        return g


class HostDriver(wc.HostDriver):
    def table(self, key_cap, max_batches):
        return HostTab(self, key_cap, max_batches)


class Removed:
    """One ramcrc_replay_table_remove_device call: every output pre-filled with
    0xA5 and longer than the call may write; the output starts `shift` bytes
    into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, kb, reqs, cap, room, next_version=1, ts=TS, rules=None, hashes=None,
                 seg_ids=None, want_refs=True, want_old=True, shift=0, check=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.n = n = reqs.shape[0]
        self.cap = cap
        kb = np.ascontiguousarray(kb, np.uint8)
        self.d_keys = torch.from_numpy(kb).cuda() if kb.size else None
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
        self.d_refs = fill(4 * n + PAD, torch.int32) if want_refs else None
        self.d_old = fill(32 * n + PAD, torch.int32) if want_old else None
        self.d_sum = fill(SUMMARY.itemsize + PAD, torch.int64)
        t.remove(self.d_keys, self.d_q, self.d_out, self.d_cert, self.d_parts, self.d_sum, next_version, ts,
                 rules=self.d_rules, key_hash=self.d_hash, batch_segment_id=self.d_seg, refs=self.d_refs,
                 old=self.d_old, keys_bytes=kb.size, n_reqs=n, out_capacity=cap)
        if check:
            ctx.check()
            self.read()

    def read(self):
        u8 = lambda x: None if x is None else x.cpu().numpy().view(np.uint8).reshape(-1)
        _split(self, self.n, self.cap, u8(self.d_out), u8(self.d_cert), u8(self.d_parts), u8(self.d_refs),
               u8(self.d_old), u8(self.d_sum))


class DeviceTab(wc.DeviceTab):
    """A table on the device with its twin on the host: every remove is held
    against the twin's, byte for byte."""

    def __init__(self, drv, key_cap, max_batches):
        wc.DeviceTab.__init__(self, drv, key_cap, max_batches)
        self.host.__class__ = HostTab

    def remove_raw(self, kb, reqs, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                   want_refs=True, want_old=True, shift=0, room=None):
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        g = Removed(self.drv.ctx, self.t, kb, reqs, cap, room, next_version, ts, rules, hashes, seg_ids,
                    want_refs, want_old, shift)
        if g.summary["spoiled"]:
            return g
        _check_got(g, n, cap)
        h = self.host.remove_raw(kb, reqs, cap, next_version, ts, rules, hashes, seg_ids, want_refs,
                                 want_old, room=room)
        assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
        assert h.out == g.out, ("host and device outputs differ", rd.first_difference(h.out, g.out))
        assert h.cert == g.cert, ("host and device certificates differ", h.cert, g.cert)
        assert lc.same(h.parts, g.parts), "host and device parts differ"
        assert not want_refs or lc.same(h.refs, g.refs), "host and device references differ"
        assert not want_old or lc.same(h.old, g.old), "host and device old results differ"
        return g


class DeviceDriver(wc.DeviceDriver):
    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


def remove(tab, exp, keys, what="", align=1, shift=0, packed=None, cap=OUT_CAP, next_version=1,
           rules=None, seg_ids=None, **kw):
    """The remove of `keys` ((table id, key) each) against the lookup
    expectation; `packed`: the (key buffer, requests) to send instead.  Returns
    (the call's outputs, the Want)."""
    kb, reqs = packed if packed is not None else segments.lookup_queries(keys, align)
    if shift:
        kb = np.concatenate([np.full(shift, 0xEE, np.uint8), kb])
        reqs = reqs.copy()
        reqs["key_off"] += shift
    w = Want(tab.drv.oracle, exp, kb, reqs, rules, next_version, TS, seg_ids, cap)
    g = tab.remove_raw(kb, reqs, cap, next_version, TS, rules, seg_ids=seg_ids, **kw)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.out == w.out, (what, "output bytes", rd.first_difference(g.out, w.out))
    assert g.cert == w.cert, (what, "certificate", g.cert, w.cert)
    assert lc.same(g.parts, w.parts), (what, "parts", g.parts[:8], w.parts[:8])
    assert g.refs is None or lc.same(g.refs, w.refs), (what, "references")
    assert g.old is None or lc.same(g.old, w.old), (what, "old results")
    if len(g.out) <= (tab.batches[0].cap if tab.batches else 64 * KiB):   # (one stride holds it)
        walked(tab, g, w)
    return g, w


def walked(tab, g, w):
    """The output as a batch: walked with the call's own certificate, every
    tombstone's checksum verified."""
    b, bad = tab.batch_of(g.out, g.cert)
    assert int(b.status[0, 0]) == segments.SEG_OK, "the certificate does not seal the output"
    assert b.table.shape[0] == w.summary["removed"] and bad == 0
    return b


def add_output(tab, g, w):
    """Walk the output with its certificate and add it as the next batch."""
    return tab.add(walked(tab, g, w))


def checked(tab):
    return lc.checked_expectation(tab) if tab.batches else {}


def read_status(tab, keys):
    """The status and version a read answers for each key."""
    got, _ = rd.read(tab, rd.checked(tab), keys, what="read")
    return [(p[0], p[1]) for p in segments.multi_read_parts(got.reply, got.summary["returned"])]


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("multi_remove_ref.json")


def check_expectation_against_golden(oracle, ref):
    """Every step of every golden scenario through the plain-Python
    expectation alone: a dict stands in for the table, as each step's entries
    are what the next step's lookup finds.  Returns how many remove steps."""
    steps = 0
    for sc in ref["scenarios"]:
        exp, batch = {}, 0
        for st in sc["steps"]:
            if "objects" in st:     # the scenario stores objects
                sizes = [24 + 1 + 2 + len(key) + len(value) for _, key, value, _ in st["objects"]]
                assert st.get("object_bytes", sizes) == sizes, (sc["name"], sizes)
                for i, (tid, key, value, ver) in enumerate(st["objects"]):
                    exp[(tid, key.encode())] = (batch, i, ver, lc.OBJECT, 0, 0, len(value))
            elif "tombstone" in st:   # the scenario stores a tombstone
                tid, key, ver = st["tombstone"]
                exp[(tid, key.encode())] = (batch, 0, ver, lc.TOMBSTONE, lc.NONE, 0, 0)
            elif "read" in st:
                tid, key = st["read"]
                res = exp.get((tid, key.encode()), lc.no_result(lc.ABSENT))
                assert (OK if res[3] == lc.OBJECT else DOESNT_EXIST) == st["status"], (sc["name"], st)
                continue
            else:
                keys = [(tid, key.encode()) for tid, key in st["keys"]]
                kb, reqs = segments.lookup_queries(keys)
                w = Want(oracle, exp, kb, reqs, st.get("rules"), st["next_version"])
                assert [int(x) for x in w.parts["status"]] == st["status"], (sc["name"], st)
                assert [int(x) for x in w.parts["version"]] == st["version"], (sc["name"], st)
                for name, v in st.get("summary", {}).items():
                    assert w.summary[name] == v, (sc["name"], name, w.summary)
                if "entry_bytes" in st:
                    assert entry_sizes(w.out) == st["entry_bytes"], (sc["name"], entry_sizes(w.out))
                if "old_kind" in st:
                    assert [int(x) for x in w.old["kind"]] == st["old_kind"]
                # a tombstone of the object's version wins at the add
                for i, ver in w.removed.items():
                    exp[keys[i]] = (batch, i, ver, lc.TOMBSTONE, lc.NONE, 0, 0)
                steps += 1
                if not w.removed:
                    continue
            batch += 1
    return steps


def case_goldens(drv):
    """Each remove step is one call followed by walk and add."""
    ref = golden()
    assert check_expectation_against_golden(drv.oracle, ref) == ref["steps"]
    for sc in ref["scenarios"]:
        tab = drv.table(64, 16)
        try:
            for st in sc["steps"]:
                if "objects" in st:
                    tab.add(drv.batch([[tc.head(1)] + [rc.obj(tid, key.encode(), ver, value.encode())
                                                       for tid, key, value, ver in st["objects"]]]))
                elif "tombstone" in st:
                    tid, key, ver = st["tombstone"]
                    tab.add(drv.batch([[tc.head(1), rc.tomb(tid, key.encode(), ver)]]))
                elif "read" in st:
                    tid, key = st["read"]
                    assert read_status(tab, [(tid, key.encode())])[0][0] == st["status"], (sc["name"], st)
                else:
                    keys = [(tid, key.encode()) for tid, key in st["keys"]]
                    g, w = remove(tab, checked(tab), keys, what=sc["name"], rules=st.get("rules"),
                                  next_version=st["next_version"])
                    assert [int(x) for x in g.parts["status"]] == st["status"]
                    assert [int(x) for x in g.parts["version"]] == st["version"]
                    assert all(g.summary[k] == v for k, v in st.get("summary", {}).items())
                    assert "entry_bytes" not in st or entry_sizes(g.out) == st["entry_bytes"]
                    assert "old_kind" not in st or [int(x) for x in g.old["kind"]] == st["old_kind"]
                    if g.summary["removed"]:
                        add_output(tab, g, w)
                        after = checked(tab)
                        for i, ver in w.removed.items():
                            assert after[keys[i]][2:4] == (ver, lc.TOMBSTONE)
        finally:
            tab.close()
    # the wrapper, once: its own arrays, the same bytes
    if not hasattr(drv, "ctx"):
        b = drv.batch([[tc.head(1), rc.obj(1, b"key0", 5, b"item0")]])
        t = drv.ramcrc.ReplayTableHost(64, 2)
        try:
            tc.host_add(t, b)
            exp = lc.expectation([b])
            kb, reqs = segments.lookup_queries([(1, b"key0"), (1, b"gone")])
            out, cert, parts, refs, old, sm = t.remove(kb, reqs, 4096, 3, TS, want_old=True)
            w = Want(drv.oracle, exp, kb, reqs, None, 3, TS, None, 4096)
            assert out[:len(w.out)].tobytes() == w.out and not out[len(w.out):].any()
            assert (int(cert["head"]), int(cert["checksum"])) == w.cert and summary_dict(sm) == w.summary
            assert lc.same(parts, w.parts) and lc.same(refs, w.refs) and lc.same(old, w.old)
            assert w.summary["removed"] == 1 and w.summary["ok_absent"] == 1 and w.summary["next_version"] == 6
        finally:
            t.close()


# ------------------------------------------------------------ closing the loop
def case_closing_the_loop(drv, mixed):
    """Remove, walk, add: the lookup says TOMBSTONE with the removed version,
    the read says STATUS_OBJECT_DOESNT_EXIST; a write over the removed keys
    takes max(next_version, cur + 1) and, walked and added, is read back."""
    tab = drv.table(2000, len(mixed) + 2)
    try:
        for b in mixed:
            tab.add(b)
        exp = checked(tab)
        rng = np.random.default_rng(23)
        keys = sorted(exp)[::3] + [(5, b"never there %d" % n) for n in range(40)]
        keys = [keys[i] for i in rng.permutation(len(keys)).tolist()]
        seg_ids = 1000 * (1 + np.arange(len(mixed), dtype=np.uint64))
        g, w = remove(tab, exp, keys, what="loop", next_version=5, seg_ids=seg_ids)
        n_obj = sum(1 for k in keys if exp.get(k, lc.no_result(lc.ABSENT))[3] == lc.OBJECT)
        assert 0 < n_obj < len(keys) and w.summary["removed"] == n_obj == len(w.removed)
        assert w.summary["ok_absent"] == len(keys) - n_obj
        # d_old is the lookup's answer, bit for bit
        assert lc.same(g.old, lc.lookup(tab, exp, keys, what="old"))
        new_batch = add_output(tab, g, w)
        assert new_batch == len(mixed)
        after = checked(tab)
        for i, key in enumerate(keys):
            if i in w.removed:
                res = after[key]
                assert res[0] == new_batch and res[2:4] == (w.removed[i], lc.TOMBSTONE)
                seg, off, ln, hdr = (int(x) for x in tab.batches[new_batch].table[res[1]])
                assert off == int(g.refs[i])
            else:
                assert after.get(key) == exp.get(key), "a key nothing was written for answers differently"
        for key, res in exp.items():
            if key not in set(keys):
                assert after[key] == res, "a key the remove did not name answers differently"
        lc.lookup(tab, after, keys, what="after the add")
        gone = [keys[i] for i in sorted(w.removed)]
        assert all(s == (DOESNT_EXIST, 0) for s in read_status(tab, gone))
        # a second remove finds nothing
        g2, w2 = remove(tab, after, gone, what="again", next_version=5)
        assert w2.summary["ok_absent"] == len(gone) and g2.out == b""
        # the write over the removed keys: the tombstone rule
        nv = 2
        gone.sort(key=lambda k: -after[k][2])   # the highest removed version first: above next_version
        objs = [(tid, key, b"back %d" % n) for n, (tid, key) in enumerate(gone)]
        gw, ww = wc.write(tab, after, objs, what="write over removed", next_version=nv)
        assert ww.summary["ok"] == len(gone) and ww.summary["tombstones"] == 0
        alloc = 0
        for n, (tid, key) in enumerate(gone):
            cur = after[(tid, key)][2]
            a = nv + alloc
            alloc += 1
            assert int(gw.parts["version"][n]) == max(a, cur + 1) == ww.versions[n]
        assert ww.versions[0] == after[gone[0]][2] + 1 > nv and ww.versions[len(gone) - 1] == nv + len(gone) - 1
        wc.add_output(tab, gw, ww)
        final, pays = rd.checked(tab)
        got, _ = rd.read(tab, (final, pays), gone, value_only=True, what="after the write")
        parts = segments.multi_read_parts(got.reply, got.summary["returned"])
        assert [(p[0], p[1], p[2]) for p in parts] == [(OK, ww.versions[n], objs[n][2]) for n in range(len(gone))]
    finally:
        tab.close()


# ---------------------------------------------------------------- the rules
GIVEN = rd.GIVEN


def case_reject_rules(drv):
    """Every rule against found (versions around the given one, and 0), a
    tombstone and an absent key; bad rules among good ones."""
    versions = rd.RULE_VERSIONS
    lists = [tc.head(1)] + [rc.obj(1, b"obj %d" % i, v, b"old") for i, v in enumerate(versions)]
    lists += [rc.tomb(1, b"tomb %d" % i, v) for i, v in enumerate(versions)]
    tab = drv.table(256, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        assert exp[(1, b"obj 0")][2:4] == (0, lc.OBJECT)
        for bits in range(16):
            r = {name: (bits >> k) & 1 for k, name in enumerate(rd.RULE_BITS)}
            r["given_version"] = GIVEN
            keys = [(1, b"%s %d" % (kind, i)) for i in range(len(versions)) for kind in (b"obj", b"tomb", b"none")]
            g, w = remove(tab, exp, keys, what=("rules", bits), rules=[dict(r) for _ in keys],
                          next_version=GIVEN + 3)
            for j, (tid, key) in enumerate(keys):
                st, ver = (int(x) for x in g.parts[j])
                if not key.startswith(b"obj"):
                    assert (st, ver) == (DOESNT_EXIST if r["doesnt_exist"] else OK, 0)
                    assert int(g.refs[j]) == NONE
                else:
                    cur = versions[j // 3]
                    assert (st, ver) == (rd.reject(r, cur), cur) and (int(g.refs[j]) != NONE) == (st == OK)
        # non-boolean rule bytes, rules given for some requests only, bad rules among good ones
        keys = [(1, b"obj 1"), (1, b"obj 2"), (1, b"none"), (1, b"obj 3"), (1, b"obj 4")]
        g, w = remove(tab, exp, keys, what="bytes", next_version=9,
                      rules=[dict(exists=0x80), None, dict(doesnt_exist=2), dict(reserved=1, exists=1), None])
        assert [int(s) for s in g.parts["status"]] == [EXISTS, OK, DOESNT_EXIST, FORMAT_ERROR, OK]
        assert int(g.old[3]["kind"]) == lc.BAD_KEY and g.summary["bad"] == 1
    finally:
        tab.close()


# ---------------------------------------------------------------- version 0
def case_version_zero(drv):
    """An object of version 0 is found: its tombstone of version 0 wins at the
    add; with doesnt_exist it is STATUS_OBJECT_DOESNT_EXIST.  The top version
    leaves next_version alone."""
    lists = [tc.head(1), rc.obj(1, b"zero", 0, b"z"), rc.obj(1, b"zero too", 0, b"y"),
             rc.obj(1, b"top", M64, b"t"), rc.obj(1, b"high", 1 << 40, b"h")]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        keys = [(1, b"zero"), (1, b"zero too")]
        g, w = remove(tab, exp, keys, what="zero", rules=[None, dict(doesnt_exist=1)], next_version=7)
        assert [tuple(int(x) for x in p) for p in g.parts] == [(OK, 0), (DOESNT_EXIST, 0)]
        assert g.summary["removed"] == 1 and g.summary["next_version"] == 7 and int(g.refs[0]) == 0
        add_output(tab, g, w)
        after = checked(tab)
        assert after[(1, b"zero")][2:4] == (0, lc.TOMBSTONE) and after[(1, b"zero too")][3] == lc.OBJECT
        assert read_status(tab, keys)[0] == (DOESNT_EXIST, 0)
        g, w = remove(tab, after, [(1, b"top")], what="top", next_version=7)
        assert tuple(int(x) for x in g.parts[0]) == (OK, M64) and g.summary["next_version"] == 7
        g, w = remove(tab, after, [(1, b"high"), (1, b"zero too")], what="high", next_version=7)
        assert g.summary["next_version"] == (1 << 40) + 1
        g, w = remove(tab, after, [(1, b"high")], what="below", next_version=(1 << 40) + 2)
        assert g.summary["next_version"] == (1 << 40) + 2
    finally:
        tab.close()


# --------------------------------------------------------------- duplicates
def case_duplicates(drv):
    others = [(2, b"other %d" % i) for i in range(24)]
    lists = [tc.head(1), rc.obj(1, b"hot", 4, b"old"), rc.obj(2, b"other 3", 8, b"old"), rc.obj(3, b"hot", 6)]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        rng = np.random.default_rng(3)
        keys = [(1, b"hot")] * 1000 + others
        keys = [keys[i] for i in rng.permutation(len(keys)).tolist()]
        g, w = remove(tab, exp, keys, what="hot")
        assert g.summary["removed"] == 2 and g.summary["retry_duplicate"] == 999 and g.summary["ok_absent"] == 23
        first = keys.index((1, b"hot"))
        assert tuple(int(x) for x in g.parts[first]) == (OK, 4)
        # a first occurrence that is rejected: its copies still get RETRY
        keys = [(1, b"hot"), (1, b"hot"), (2, b"other 3"), (1, b"hot")]
        g, w = remove(tab, exp, keys, what="rejected first", rules=[dict(exists=1), None, None, None])
        assert [tuple(int(x) for x in p) for p in g.parts] == [(EXISTS, 4), (RETRY, 0), (OK, 8), (RETRY, 0)]
        # a bad request does not count as a first
        kb, reqs = segments.lookup_queries(keys)
        reqs["reserved"][0] = 1
        g, w = remove(tab, exp, None, what="bad first", packed=(kb, reqs))
        assert [tuple(int(x) for x in p) for p in g.parts] == [(FORMAT_ERROR, 0), (OK, 4), (OK, 8), (RETRY, 0)]
        # a first occurrence that is cut: its copies still get RETRY with version 0
        keys = [(2, b"other 3"), (1, b"hot"), (1, b"hot"), (2, b"other 3")]
        g, w = remove(tab, exp, keys, what="cut first", cap=2 + 32 + 7 + 2 + 32 + 2)
        assert [tuple(int(x) for x in p) for p in g.parts] == [(OK, 8), (RETRY, 4), (RETRY, 0), (RETRY, 0)]
        assert g.summary["retry_full"] == 1 and g.summary["retry_duplicate"] == 2
        # the same bytes under another table id, and a key that is a prefix, are other keys
        keys = [(1, b"hot"), (3, b"hot"), (1, b"ho"), (1, b"hot")]
        g, w = remove(tab, exp, keys, what="identity")
        assert [tuple(int(x) for x in p) for p in g.parts] == [(OK, 4), (OK, 6), (OK, 0), (RETRY, 0)]
    finally:
        tab.close()


# ------------------------------------------------------ sizes and alignment
KEY_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, LANE_KEY_MAX - 1, LANE_KEY_MAX, LANE_KEY_MAX + 1, LANE_KEY_MAX + 8,
               223, 224, 65503, 65504, 65535]


def case_key_lengths(drv):
    """The length-byte steps of the entry header (payload 255 / 256 and 65,535
    / 65,536) and both sides of the lane / group class bound."""
    rng = np.random.default_rng(8)
    keys = [(1, rng.integers(0, 256, kl, dtype=np.uint8).tobytes()) for kl in KEY_LENGTHS]
    lists = [[tc.head(1)] + [rc.obj(1, k, 7 + i, b"old") for i, (_, k) in enumerate(keys[:-3])]]
    lists += [[tc.head(2 + i), rc.obj(1, k, 100 + i, b"o")] for i, (_, k) in enumerate(keys[-3:])]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch(lists, cap=128 * KiB))
        exp = checked(tab)
        order = rng.permutation(len(keys)).tolist()
        for ks in (keys, [keys[i] for i in order]):
            g, w = remove(tab, exp, ks, what="key lengths", cap=512 * KiB, room=512 * KiB,
                          seg_ids=[0x0102030405060708])
            assert g.summary["removed"] == len(keys)
            assert sorted(entry_sizes(g.out)) == [32 + kl for kl in KEY_LENGTHS]
            assert {255, 256, 65535, 65536} <= set(entry_sizes(g.out))
    finally:
        tab.close()
    # walked and added: one stride holds the output
    tab = drv.table(64, 2)
    try:
        short = [k for k in keys if len(k[1]) < 300]
        tab.add(drv.batch([[tc.head(1)] + [rc.obj(1, k, 7 + i, b"old") for i, (_, k) in enumerate(short)]]))
        exp = checked(tab)
        g, w = remove(tab, exp, short, what="short key lengths")
        add_output(tab, g, w)
        after = checked(tab)
        assert all(after[k][3] == lc.TOMBSTONE for k in short)
    finally:
        tab.close()


def case_alignment(drv):
    """Every key at source byte offsets 0 to 15 and every entry at destination
    byte offsets 0 to 15: the keys' lengths step the key buffer and the head
    through the residues, `shift` moves the key buffer and the output
    allocation; both classes of key length."""
    rng = np.random.default_rng(5)   # (a seed whose lengths reach every residue in both classes)
    lengths = [int(rng.integers(1, LANE_KEY_MAX + 1)) if rng.random() < 0.6 else int(rng.integers(LANE_KEY_MAX + 1, 90))
               for _ in range(120)]
    keys = [(1, bytes([i]) + rng.integers(0, 256, n - 1, dtype=np.uint8).tobytes()) for i, n in enumerate(lengths)]
    lists = [tc.head(1)] + [rc.obj(1, k, 2 + i, b"old") for i, (_, k) in enumerate(keys) if i % 3]
    tab = drv.table(256, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        for shift in range(16):
            g, w = remove(tab, exp, keys, what=("alignment", shift), shift=shift, seg_ids=[shift << 40])
            kb, reqs = segments.lookup_queries(keys)
            written = [j for j in range(len(keys)) if int(g.refs[j]) != NONE]
            for lo, hi in ((0, LANE_KEY_MAX), (LANE_KEY_MAX + 1, 1 << 16)):
                cls = [j for j in written if lo <= lengths[j] <= hi]
                assert {int(g.refs[j]) % 16 for j in cls} == set(range(16)), ("destinations", shift, lo)
                assert shift or {int(reqs["key_off"][j]) % 16 for j in cls} == set(range(16)), ("sources", lo)
        for align in (4, 16):
            remove(tab, exp, keys, what=("aligned", align), align=align)
    finally:
        tab.close()


# -------------------------------------------------------------------- space
def case_space(drv):
    """Capacity 0, one byte short of the first entry, the cut at requests 255,
    256 and 257 of 600 and exactly on an entry's end; requests that write
    nothing keep their status behind the cut."""
    n = 600
    keys = [(1, b"sp %d" % i) for i in range(n)]
    absent, rejected, bad, dup = {3, 300, 590}, {5, 400, 595}, {7, 420, 598}, {9: 2, 450: 1, 599: 0}
    lists = [tc.head(1)] + [rc.obj(1, k, 5 + i, b"old") for i, (_, k) in enumerate(keys) if i not in absent]
    tab = drv.table(2048, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        for i, j in dup.items():
            keys[i] = keys[j]
        kb, reqs = segments.lookup_queries(keys)
        rules = [None] * n
        for i in rejected:
            rules[i] = dict(exists=1)
        for i in bad:
            reqs["reserved"][i] = 9
        full = Want(drv.oracle, exp, kb, reqs, rules, 50)
        quiet = absent | rejected | bad | set(dup)
        assert full.summary["removed"] == n - len(quiet)
        start = lambda i: int(full.refs[i])
        first = min(i for i in range(n) if i not in quiet)
        caps = [0, start(first) + 34 + len(keys[first][1]) - 1, len(full.out), len(full.out) - 1]
        for i in (255, 256, 257):
            assert i not in quiet
            caps += [start(i) + 5, start(i), start(i) - 1]   # inside entry i, on the end of the one before, inside that
        for cap in caps:
            g, w = remove(tab, exp, None, what=("space", cap), packed=(kb, reqs), rules=rules, cap=cap,
                          next_version=50)
            st = [int(s) for s in g.parts["status"]]
            assert all(st[i] == OK and int(g.parts["version"][i]) == 0 for i in absent)
            assert all(st[i] == EXISTS and int(g.parts["version"][i]) == 5 + i for i in rejected)
            assert all(st[i] == FORMAT_ERROR for i in bad) and all(st[i] == RETRY for i in dup)
            cut = [i for i in range(n) if i not in quiet and start(i) + 34 + len(keys[i][1]) > cap]
            assert all(st[i] == RETRY and int(g.parts["version"][i]) == 5 + i and int(g.refs[i]) == NONE
                       for i in cut)
            assert g.summary["retry_full"] == len(cut)
            assert g.summary["removed"] + g.summary["retry_full"] == full.summary["removed"]
            top = max([5 + i for i in range(n) if i not in quiet and i not in cut], default=0)
            assert g.summary["next_version"] == max(50, top + 1)
    finally:
        tab.close()


def case_counts(drv):
    """n_reqs = 0, 1, 255, 256, 257: the tile's edge."""
    keys = [(1, b"count %d" % i) for i in range(257)]
    lists = [tc.head(1)] + [rc.obj(1, k, 1 + i, b"v") for i, (_, k) in enumerate(keys) if i % 5]
    tab = drv.table(1024, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        for n in (0, 1, 255, 256, 257):
            ks = keys[257 - n:]
            g, w = remove(tab, exp, ks, what=("count", n), next_version=77)
            assert g.summary["removed"] + g.summary["ok_absent"] == n
            if n == 0:
                assert g.summary == dict(dict.fromkeys(SUMMARY_NAMES, 0), next_version=77) and g.out == b""
                assert g.cert == ac.expected_cert(drv.oracle, b"")
    finally:
        tab.close()


# ------------------------------------------------------------- bad requests
def case_bad_requests(drv):
    lists = [tc.head(1), rc.obj(1, b"good", 2, b"old"), rc.obj(1, b"", 3, b"empty key")]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        keys = [(1, b"good")] + [(1, b"key %d" % i) for i in range(6)] + [(1, b""), (1, b"last")]
        kb, reqs = segments.lookup_queries(keys)
        rules = [None] * len(keys)
        reqs["reserved"][1] = 1
        rules[2] = dict(reserved=1, exists=1)
        reqs["key_off"][3] = kb.size - 3                     # runs 1 byte past the buffer
        reqs["key_off"][4] = M64 - 2                         # the sum overflows
        reqs["key_off"][5] = kb.size + 1
        reqs["key_len"][6] = 65536                           # KeyLength is 16 bits
        g, w = remove(tab, exp, None, what="bad", packed=(kb, reqs), rules=rules)
        st = [int(s) for s in g.parts["status"]]
        assert st == [OK] + [FORMAT_ERROR] * 6 + [OK, OK], st
        assert (g.parts["version"][1:7] == 0).all() and g.summary["bad"] == 6 and g.summary["removed"] == 2
        assert int(g.old[8]["kind"]) == lc.ABSENT and all(int(g.old[i]["kind"]) == lc.BAD_KEY for i in range(1, 7))
        # an empty key buffer: the empty key is a key
        reqs = np.zeros(2, lc.KEY)
        reqs["table_id"], reqs["key_len"][1] = 1, 1
        g, w = remove(tab, exp, None, what="no keys", packed=(np.zeros(0, np.uint8), reqs))
        assert [tuple(int(x) for x in p) for p in g.parts] == [(OK, 3), (FORMAT_ERROR, 0)]
    finally:
        tab.close()


# ------------------------------------------------------- nullable and empty
def case_nullable(drv):
    """Each nullable argument on its own, all NULL and all given."""
    lists = [tc.head(1), rc.obj(1, b"have", 2, b"old"), rc.obj(2, b"too", 3, b"old")]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        tab.add(drv.batch([[tc.head(2)], [tc.head(3), rc.obj(1, b"second", 1, b"old")]]))
        exp = checked(tab)
        keys = [(1, b"have"), (2, b"too"), (1, b"second"), (1, b"fresh")]
        hashes = np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)
        seg_ids = [0x1122334455667788, 7 << 32]
        g0, w0 = remove(tab, exp, keys, what="all NULL", want_refs=False, want_old=False)
        g1, w1 = remove(tab, exp, keys, what="all given", rules=[None] * 4, hashes=hashes, seg_ids=seg_ids)
        assert g0.refs is None and g0.old is None and g0.out != g1.out and len(g0.out) == len(g1.out)
        # the segment id bytes of every tombstone: batch 0 segment 0 twice, batch 1 segment 1
        ids = [int.from_bytes(g1.out[int(r) + 2 + 8:][:8], "little") for r in g1.refs[:3]]
        assert ids == [0x1122334455667788, 0x1122334455667788, (7 << 32) + 1]
        assert all(int.from_bytes(g0.out[int(r) + 2 + 8:][:8], "little") == 0 for r in w0.refs[:3])
        for kw in (dict(rules=[None, dict(exists=1), None, None]), dict(hashes=hashes), dict(seg_ids=seg_ids),
                   dict(want_refs=False), dict(want_old=False)):
            remove(tab, exp, keys, what=("one given or missing", sorted(kw)), **kw)
        # next_version = 0
        kb, reqs = segments.lookup_queries(keys)
        try:
            tab.remove_raw(kb, reqs, 4096, 0)
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
        kb, reqs = segments.lookup_queries([(1, b"k")])
        g = tab.remove_raw(kb, reqs, 4096)
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
        g, w = remove(tab, exp, keys, what="read-only", next_version=9)
        assert w.summary["removed"] > 0 and w.summary["ok_absent"] > 0
        assert tab.state() == before, "a remove without an add changed the table"
        assert lc.same(lc.lookup(tab, exp, keys, what="after"), looked)
    finally:
        tab.close()
