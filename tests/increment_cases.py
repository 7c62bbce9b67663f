"""Requests, cases and the expectation for the replay table's multi-increment
(ramcrc_replay_table_increment_host / _device).

The expectation is plain Python: the loop of include/ramcrc.h over
lookup_cases.expectation (the plain-Python replay of the added batches) and the
old value's bytes in the batches, the sum in numpy float64, entries and CRCs as
write_cases.py builds them.  It is held against
tests/golden/multi_increment_ref.json before any library call.  The scenarios
run unchanged on the host and on the device: a driver makes batches and tables;
a table adds, looks up, reads, writes, removes and increments; the output of an
increment is walked with its certificate and added as the next batch.  Every
increment whose requests a write can express is also held against the merged
write of the images of the new values: the same output bytes, certificate,
references, old results and the parts' status and version.  Every output is
pre-filled with 0xA5 and checked past its end.
"""
import ctypes
import struct

import numpy as np

from ramcloud_amd import segments

import append_cases as ac
import lookup_cases as lc
import partition_cases as pc
import read_cases as rd
import remove_cases as rm
import replay_table_cases as tc
import resolve_cases as rc
import write_cases as wc

KiB = 1024
FILL, FILL32 = rd.FILL, rd.FILL32
M64 = (1 << 64) - 1
NONE = segments.WRITE_REF_NONE
PART, SUMMARY, REF = segments.INCREMENT_PART_DTYPE, segments.INCREMENT_SUMMARY_DTYPE, segments.WRITE_REF_DTYPE
SUMMARY_NAMES = SUMMARY.names
OK, DOESNT_EXIST, EXISTS, WRONG_VERSION, FORMAT_ERROR = (rd.OK, rd.DOESNT_EXIST, rd.EXISTS,
                                                         rd.WRONG_VERSION, rd.FORMAT_ERROR)
RETRY, INVALID = segments.STATUS_RETRY, segments.STATUS_INVALID_OBJECT
STATUS_FIELD = {DOESNT_EXIST: "doesnt_exist", EXISTS: "object_exists", WRONG_VERSION: "wrong_version",
                INVALID: "invalid_object"}
SPOILED_SUMMARY = dict(dict.fromkeys(SUMMARY_NAMES, 0), spoiled=1)
TS = 0x1AC4E3E7       # the timestamp of every increment below
PAD = 64              # bytes of 0xA5 behind every output
OUT_CAP = 256 * KiB   # the output's allocation where a case does not size it
LANE_KEY_MAX = 36     # dev_increment.inc: up to here a lane writes the entries, a group of 8 beyond
NAN = 0x7FF8000000000000
bits = segments.double_bits


def i64(x):
    """The 8 value bytes of an integer (modulo 2^64) or of a float."""
    return struct.pack("<d", x) if isinstance(x, float) else (int(x) & M64).to_bytes(8, "little")


# ---------------------------------------------------------- the expectation
def py_sum(old, add_int, add_double_bits):
    """Step 5 on bits, with numpy float64 for the floating-point addition."""
    new = old
    if add_int & M64:
        new = (new + add_int) & M64
    inc = np.array([add_double_bits], "<u8").view("<f8")[0]
    if inc != 0.0:   # (false for -0.0, true for a NaN)
        with np.errstate(all="ignore"):
            r = np.array([new], "<u8").view("<f8")[0] + inc
        new = NAN if np.isnan(r) else int(np.array([r], "<f8").view("<u8")[0])
    return new


def old_value(batches, res):
    """The 8 bytes a lookup result of kind OBJECT points at, as an integer."""
    b = batches[res[0]]
    at = res[4] * b.cap + res[5]
    return int.from_bytes(b.buf[at:at + 8].tobytes(), "little")


def image(key, new):
    return segments.keys_and_value([key], new.to_bytes(8, "little"))


class Want:
    """What an increment of (key buffer, reqs, args) must produce against the
    lookup expectation `exp` (key -> LOOKUP_RESULT tuple) of `batches`."""

    def __init__(self, oracle, exp, batches, kb, reqs, args, rules=None, next_version=1, ts=TS, seg_ids=None,
                 cap=OUT_CAP):
        kb = bytes(np.ascontiguousarray(kb, np.uint8))
        n = reqs.shape[0]
        self.parts = np.zeros(n, PART)
        self.refs = np.zeros(n, REF)
        self.old = np.zeros(n, lc.RES)
        self.versions, self.bits = {}, {}   # request -> the written version, the new value (computed)
        sm = dict.fromkeys(SUMMARY_NAMES, 0)
        out, seen, top, is_open = bytearray(), set(), 0, True
        for i in range(n):
            table_id, off, ln, reserved = (int(x) for x in reqs[i])
            add_int, add_dbl = int(args["add_int64"][i]) & M64, int(args["add_double_bits"][i])
            r = (rules[i] if rules is not None else None) or {}
            status, version, ref, res, new = FORMAT_ERROR, 0, (NONE, NONE), lc.no_result(lc.BAD_KEY), 0
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
                    found = res[3] == lc.OBJECT
                    cur = res[2] if found else 0
                    status, version = rd.reject(r, cur), cur
                    if status == OK and found and res[6] != 8:
                        status = INVALID
                    if status != OK:
                        sm[STATUS_FIELD[status]] += 1
                    else:
                        new = py_sum(old_value(batches, res) if found else 0, add_int, add_dbl)
                        self.bits[i] = new
                        img = image(key, new)
                        a = (next_version + sm["allocated"]) & M64
                        if cur:
                            v = (cur + 1) & M64
                        else:
                            v = (res[2] + 1) & M64 if res[3] == lc.TOMBSTONE and res[2] >= a else a
                            sm["allocated"] += 1
                            if v != a:
                                top = max(top, (v + 1) & M64)
                        blob = wc.object_entry(oracle, table_id, v, ts, img)
                        t_at = len(out) + len(blob)
                        if cur:
                            seg_id = 0 if seg_ids is None else (int(seg_ids[res[0]]) + res[4]) & M64
                            blob += wc.tombstone_entry(oracle, table_id, seg_id, cur, ts, key)
                        if is_open and len(out) + len(blob) <= cap:
                            ref = (len(out), t_at if cur else NONE)
                            out += blob
                            sm["ok"] += 1
                            sm["created"] += 0 if cur else 1
                            sm["tombstones"] += 1 if cur else 0
                            sm["value_bytes"] += 8
                            sm["key_bytes"] += 3 + ln
                            sm["object_bytes"] += 24 + len(img)
                            sm["tombstone_bytes"] += 32 + ln if cur else 0
                            version = v
                            self.versions[i] = v
                        else:
                            is_open = False
                            status = RETRY
                            sm["retry_full"] += 1
            self.parts[i] = (status, version, new if status == OK else add_dbl)
            self.refs[i] = ref
            self.old[i] = res
        sm["out_bytes"] = len(out)
        sm["next_version"] = max((next_version + sm["allocated"]) & M64, top)
        self.out = bytes(out)
        self.cert = ac.expected_cert(oracle, self.out)
        self.summary = sm


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


entry_sizes = rm.entry_sizes


# ------------------------------------------------------------------ drivers
class Got:
    """The outputs of one increment, read back."""


_check_got = wc._check_got


def _split(g, n, cap, out, cert, parts, refs, old, sm):
    g.summary = summary_dict(sm[:SUMMARY.itemsize].view(SUMMARY)[0])
    g.summary_past = sm[SUMMARY.itemsize:]
    g.out_all = out
    g.out = out[:min(g.summary["out_bytes"], out.size)].tobytes()
    g.cert = tuple(int(x) for x in cert[:8].view(np.uint32))
    g.cert_past = cert[8:]
    g.parts, g.parts_past = parts[:20 * n].view(PART), parts[20 * n:]
    g.refs = g.refs_past = g.old = g.old_past = None
    if refs is not None:
        g.refs, g.refs_past = refs[:8 * n].view(REF), refs[8 * n:]
    if old is not None:
        g.old, g.old_past = old[:32 * n].view(lc.RES), old[32 * n:]
    return g


class HostTab(rm.HostTab):
    def increment_raw(self, kb, reqs, args, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                      want_refs=True, want_old=True, shift=0, room=None):
        """The call itself, on pre-filled arrays (the wrapper allocates its own:
        case_goldens goes through it)."""
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        fill = lambda k: np.full(k, FILL, np.uint8)
        kb = np.ascontiguousarray(kb, np.uint8)
        raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(-1).copy()
        ar = np.ascontiguousarray(args).view(np.uint8).reshape(-1).copy()
        rl = segments.read_rules(rules).view(np.uint8).reshape(-1).copy() if rules is not None and n else None
        hs = np.ascontiguousarray(hashes, np.uint64) if hashes is not None else None
        sg = np.ascontiguousarray(seg_ids, np.uint64) if seg_ids is not None else None
        out, cert, parts = fill(room + PAD + shift)[shift:], fill(8 + PAD), fill(20 * n + PAD)
        refs = fill(8 * n + PAD) if want_refs else None
        old = fill(32 * n + PAD) if want_old else None
        sm = fill(SUMMARY.itemsize + PAD)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None
        L = self.drv.ramcrc.lib()
        self.drv.ramcrc._check(L.ramcrc_replay_table_increment_host(
            self.t._h, p(kb), kb.size, p(raw), n, p(ar), p(hs), p(rl), next_version, ts, p(sg), p(out), cap,
            p(cert), p(parts), p(refs), p(old), p(sm)), "ramcrc_replay_table_increment_host")
        g = _split(Got(), n, cap, out, cert, parts, refs, old, sm)
        if not g.summary["spoiled"]:
            _check_got(g, n, cap)
        return g


class HostDriver(rm.HostDriver):
    def table(self, key_cap, max_batches):
        return HostTab(self, key_cap, max_batches)


class Incremented:
    """One ramcrc_replay_table_increment_device call: every output pre-filled
    with 0xA5 and longer than the call may write; the output starts `shift`
    bytes into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, kb, reqs, args, cap, room, next_version=1, ts=TS, rules=None, hashes=None,
                 seg_ids=None, want_refs=True, want_old=True, shift=0, check=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.n = n = reqs.shape[0]
        self.cap = cap
        kb = np.ascontiguousarray(kb, np.uint8)
        self.d_keys = torch.from_numpy(kb).cuda() if kb.size else None
        raw = np.ascontiguousarray(reqs).view(np.uint8).reshape(-1)
        self.d_q = torch.from_numpy(raw.copy()).cuda().view(torch.int64) if n else None
        ar = np.ascontiguousarray(args).view(np.uint8).reshape(-1)
        self.d_args = torch.from_numpy(ar.copy()).cuda().view(torch.int64) if n else None
        self.d_rules = None
        if rules is not None and n:
            rl = segments.read_rules(rules).view(np.uint8).reshape(-1)
            self.d_rules = torch.from_numpy(rl.copy()).cuda().view(torch.int64)
        u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()
        self.d_hash = u64(hashes) if hashes is not None else None
        self.d_seg = u64(seg_ids) if seg_ids is not None else None
        self.d_out = fill(room + PAD + shift, torch.uint8)[shift:]
        self.d_cert = fill(8 + PAD, torch.int32)
        self.d_parts = fill(20 * n + PAD, torch.int32)
        self.d_refs = fill(8 * n + PAD, torch.int32) if want_refs else None
        self.d_old = fill(32 * n + PAD, torch.int32) if want_old else None
        self.d_sum = fill(SUMMARY.itemsize + PAD, torch.int64)
        t.increment(self.d_keys, self.d_q, self.d_args, self.d_out, self.d_cert, self.d_parts, self.d_sum,
                    next_version, ts, rules=self.d_rules, key_hash=self.d_hash, batch_segment_id=self.d_seg,
                    refs=self.d_refs, old=self.d_old, keys_bytes=kb.size, n_reqs=n, out_capacity=cap)
        if check:
            ctx.check()
            self.read()

    def read(self):
        u8 = lambda x: None if x is None else x.cpu().numpy().view(np.uint8).reshape(-1)
        _split(self, self.n, self.cap, u8(self.d_out), u8(self.d_cert), u8(self.d_parts), u8(self.d_refs),
               u8(self.d_old), u8(self.d_sum))


def same_outputs(h, g, want_refs=True, want_old=True, what="host and device"):
    assert h.summary == g.summary, (what, "summaries differ", h.summary, g.summary)
    assert h.out == g.out, (what, "outputs differ", rd.first_difference(h.out, g.out))
    assert h.cert == g.cert, (what, "certificates differ", h.cert, g.cert)
    assert lc.same(h.parts, g.parts), (what, "parts differ")
    assert not want_refs or lc.same(h.refs, g.refs), (what, "references differ")
    assert not want_old or lc.same(h.old, g.old), (what, "old results differ")


class DeviceTab(rm.DeviceTab):
    """A table on the device with its twin on the host: every increment is held
    against the twin's, byte for byte."""

    def __init__(self, drv, key_cap, max_batches):
        rm.DeviceTab.__init__(self, drv, key_cap, max_batches)
        self.host.__class__ = HostTab

    def increment_raw(self, kb, reqs, args, cap, next_version=1, ts=TS, rules=None, hashes=None, seg_ids=None,
                      want_refs=True, want_old=True, shift=0, room=None):
        n = reqs.shape[0]
        room = min(cap, OUT_CAP) if room is None else room
        g = Incremented(self.drv.ctx, self.t, kb, reqs, args, cap, room, next_version, ts, rules, hashes, seg_ids,
                        want_refs, want_old, shift)
        if g.summary["spoiled"]:
            return g
        _check_got(g, n, cap)
        h = self.host.increment_raw(kb, reqs, args, cap, next_version, ts, rules, hashes, seg_ids, want_refs,
                                    want_old, room=room)
        same_outputs(h, g, want_refs, want_old)
        return g


class DeviceDriver(rm.DeviceDriver):
    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


def held_to_the_write(tab, g, w, kb, reqs, rules, next_version, seg_ids, cap, what, **kw):
    """The merged write of the images of the new values, with the same rules,
    next_version, timestamp, segment ids and capacity, gives the same output,
    certificate, references, old results and the parts' status and version.
    Only for a request list the write can express: no unusable request (the
    write's are unusable for other reasons) and no invalid object."""
    st = w.parts["status"]
    if ((st == FORMAT_ERROR) | (st == INVALID)).any():
        return False
    kbb = bytes(np.ascontiguousarray(kb, np.uint8))
    objs = []
    for i in range(reqs.shape[0]):
        tid, off, ln, _ = (int(x) for x in reqs[i])
        objs.append((tid, [kbb[off:off + ln]], w.bits.get(i, 0).to_bytes(8, "little")))
    data, wreqs = segments.write_requests(objs)
    kw = {k: v for k, v in kw.items() if k in ("want_refs", "want_old", "room", "hashes")}
    gw = tab.write_raw(data, wreqs, cap, next_version, TS, rules, seg_ids=seg_ids, **kw)
    assert gw.out == g.out, (what, "the write's output differs", rd.first_difference(gw.out, g.out))
    assert gw.cert == g.cert, (what, "the write's certificate differs")
    assert g.refs is None or lc.same(gw.refs, g.refs), (what, "the write's references differ")
    assert g.old is None or lc.same(gw.old, g.old), (what, "the write's old results differ")
    assert np.array_equal(gw.parts["status"], g.parts["status"]), (what, "the write's statuses differ")
    assert np.array_equal(gw.parts["version"], g.parts["version"]), (what, "the write's versions differ")
    for name in wc.SUMMARY_NAMES:
        assert gw.summary[name] == g.summary[name], (what, "the write's summary differs", name)
    return True


def increment(tab, exp, keys, args, what="", align=1, shift=0, packed=None, cap=OUT_CAP, next_version=1,
              rules=None, seg_ids=None, equiv=True, **kw):
    """The increment of `keys` ((table id, key) each) by `args` ((add_int64,
    add_double) each) against the lookup expectation; `packed`: the (key
    buffer, requests) to send instead.  Returns (the call's outputs, the
    Want)."""
    kb, reqs = packed if packed is not None else segments.lookup_queries(keys, align)
    if not isinstance(args, np.ndarray):
        args = segments.increment_args(args)
    if shift:
        kb = np.concatenate([np.full(shift, 0xEE, np.uint8), kb])
        reqs = reqs.copy()
        reqs["key_off"] += shift
    w = Want(tab.drv.oracle, exp, tab.batches, kb, reqs, args, rules, next_version, TS, seg_ids, cap)
    g = tab.increment_raw(kb, reqs, args, cap, next_version, TS, rules, seg_ids=seg_ids, shift=shift, **kw)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.out == w.out, (what, "output bytes", rd.first_difference(g.out, w.out))
    assert g.cert == w.cert, (what, "certificate", g.cert, w.cert)
    assert lc.same(g.parts, w.parts), (what, "parts", g.parts[:8], w.parts[:8])
    assert g.refs is None or lc.same(g.refs, w.refs), (what, "references")
    assert g.old is None or lc.same(g.old, w.old), (what, "old results")
    w.held_to_the_write = equiv and held_to_the_write(tab, g, w, kb, reqs, rules, next_version, seg_ids, cap,
                                                      what, **kw)
    return g, w


def add_output(tab, g, w):
    """Walk the output with its certificate (every checksum verified) and add
    it as the next batch."""
    return wc.add_output(tab, g, w)


def checked(tab):
    return lc.checked_expectation(tab) if tab.batches else {}


def read_values(tab, keys):
    """(status, version, value bytes) a value-only read answers for each key."""
    got, _ = rd.read(tab, rd.checked(tab), keys, value_only=True, what="read")
    return [(p[0], p[1], p[2]) for p in segments.multi_read_parts(got.reply, got.summary["returned"])]


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("multi_increment_ref.json")


def golden_value(v):
    """A golden's value: an integer, or {"double": x}."""
    return bits(float(v["double"])) if isinstance(v, dict) else int(v) & M64


class _Stored:
    """A batch of the expectation alone: the value bytes a result points at."""

    def __init__(self, values):
        self.cap = 1 << 20
        self.buf = np.zeros(8 * len(values) + 8, np.uint8)
        for i, v in enumerate(values):
            self.buf[8 * i:8 * i + len(v)] = np.frombuffer(v, np.uint8)


def check_expectation_against_golden(oracle, ref):
    """Every step of every golden scenario through the plain-Python
    expectation alone: a dict and the stored values stand in for the table, as
    each step's entries are what the next step's lookup finds.  Returns how
    many increment steps."""
    steps = 0
    for sc in ref["scenarios"]:
        exp, batches = {}, []
        for st in sc["steps"]:
            if "objects" in st:     # the scenario stores objects: [table id, key, value hex, version]
                vals = [bytes.fromhex(v) for _, _, v, _ in st["objects"]]
                for i, (tid, key, _, ver) in enumerate(st["objects"]):
                    exp[(tid, key.encode())] = (len(batches), i, ver, lc.OBJECT, 0, 8 * i, len(vals[i]))
                batches.append(_Stored(vals))
                continue
            keys = [(tid, key.encode()) for tid, key in st["keys"]]
            kb, reqs = segments.lookup_queries(keys)
            args = segments.increment_args([(a, float(d)) for a, d in st["args"]])
            w = Want(oracle, exp, batches, kb, reqs, args, st.get("rules"), st["next_version"])
            assert [int(x) for x in w.parts["status"]] == st["status"], (sc["name"], st)
            assert [int(x) for x in w.parts["version"]] == st["version"], (sc["name"], st)
            for i, v in enumerate(st.get("value", [])):
                assert v is None or int(w.parts["value_bits"][i]) == golden_value(v), (sc["name"], i, st)
            for name, v in st.get("summary", {}).items():
                assert w.summary[name] == v, (sc["name"], name, w.summary)
            vals = [w.bits[i].to_bytes(8, "little") for i in sorted(w.versions)]
            for n, i in enumerate(sorted(w.versions)):
                exp[keys[i]] = (len(batches), n, w.versions[i], lc.OBJECT, 0, 8 * n, 8)
            if vals:
                batches.append(_Stored(vals))
            steps += 1
    return steps


def case_goldens(drv):
    """Each increment step is one call followed by walk and add; the value is
    then read back."""
    ref = golden()
    assert check_expectation_against_golden(drv.oracle, ref) == ref["steps"]
    for sc in ref["scenarios"]:
        tab = drv.table(64, 16)
        try:
            for st in sc["steps"]:
                if "objects" in st:
                    tab.add(drv.batch([[tc.head(1)] + [rc.obj(tid, key.encode(), ver, bytes.fromhex(value))
                                                       for tid, key, value, ver in st["objects"]]]))
                    continue
                keys = [(tid, key.encode()) for tid, key in st["keys"]]
                g, w = increment(tab, checked(tab), keys, [(a, float(d)) for a, d in st["args"]], what=sc["name"],
                                 rules=st.get("rules"), next_version=st["next_version"])
                assert [int(x) for x in g.parts["status"]] == st["status"]
                assert [int(x) for x in g.parts["version"]] == st["version"]
                for i, v in enumerate(st.get("value", [])):
                    assert v is None or int(g.parts["value_bits"][i]) == golden_value(v)
                assert all(g.summary[k] == v for k, v in st.get("summary", {}).items())
                if g.summary["ok"]:
                    add_output(tab, g, w)
                    served = sorted(w.versions)
                    assert read_values(tab, [keys[i] for i in served]) == \
                        [(OK, w.versions[i], w.bits[i].to_bytes(8, "little")) for i in served]
        finally:
            tab.close()
    # the wrapper, once: its own arrays, the same bytes
    if not hasattr(drv, "ctx"):
        b = drv.batch([[tc.head(1), rc.obj(1, b"key0", 5, i64(40))]])
        t = drv.ramcrc.ReplayTableHost(64, 2)
        try:
            tc.host_add(t, b)
            exp = lc.expectation([b])
            kb, reqs = segments.lookup_queries([(1, b"key0"), (1, b"new")])
            args = segments.increment_args([(2, 0.0), (0, 1.5)])
            out, cert, parts, refs, old, sm = t.increment(kb, reqs, args, 4096, 3, TS, want_old=True)
            w = Want(drv.oracle, exp, [b], kb, reqs, args, None, 3, TS, None, 4096)
            assert out[:len(w.out)].tobytes() == w.out and not out[len(w.out):].any()
            assert (int(cert["head"]), int(cert["checksum"])) == w.cert and summary_dict(sm) == w.summary
            assert lc.same(parts, w.parts) and lc.same(refs, w.refs) and lc.same(old, w.old)
            assert [tuple(int(x) for x in p) for p in segments.multi_increment_parts(parts.tobytes())] == \
                [(OK, 6, 42), (OK, 3, bits(1.5))]
            assert w.summary["ok"] == 2 and w.summary["created"] == 1 and w.summary["next_version"] == 4
        finally:
            t.close()


# ------------------------------------------------------------ closing the loop
def case_closing_the_loop(drv):
    """Increment, walk with the certificate (every checksum good), add: a read
    returns the new 8 bytes.  A second increment accumulates, takes version +
    1, and its tombstone names the first output's batch.  A remove, then an
    increment: the key is re-created from zero at the version the write's
    tombstone rule gives."""
    keys = [(1, b"ctr %d" % i) for i in range(40)] + [(2, b"fresh %d" % i) for i in range(10)]
    lists = [tc.head(1)] + [rc.obj(1, k, 10 + i, i64(1000 + i)) for i, (_, k) in enumerate(keys[:40])]
    tab = drv.table(256, 6)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        rng = np.random.default_rng(31)
        order = rng.permutation(len(keys)).tolist()
        ks = [keys[i] for i in order]
        seg_ids = np.array([1000, 2000, 3000, 4000, 5000, 6000], np.uint64)
        g, w = increment(tab, exp, ks, [(i + 1, 0.0) for i in order], what="first", next_version=200,
                         seg_ids=seg_ids)
        assert w.summary["ok"] == 50 and w.summary["tombstones"] == 40 and w.summary["created"] == 10
        assert w.held_to_the_write
        assert lc.same(g.old, lc.lookup(tab, exp, ks, what="old"))   # d_old is the lookup's answer
        first = add_output(tab, g, w)
        assert first == 1
        want = []
        for n, i in enumerate(order):
            ver = 11 + i if i < 40 else w.versions[n]
            want.append((OK, ver, i64((1000 + i if i < 40 else 0) + i + 1)))
        assert sorted(w.versions[n] for n, i in enumerate(order) if i >= 40) == list(range(200, 210))
        assert read_values(tab, ks) == want
        # the second increment accumulates on the first's output
        exp = checked(tab)
        assert all(exp[k][0] == first for k in ks)
        g2, w2 = increment(tab, exp, ks, [(0, 0.5) for _ in ks], what="second", next_version=210, seg_ids=seg_ids)
        assert w2.summary["ok"] == 50 and w2.summary["tombstones"] == 50 and w2.summary["allocated"] == 0
        for n in range(len(ks)):
            assert int(g2.parts["version"][n]) == want[n][1] + 1
            old = np.frombuffer(want[n][2], "<f8")[0]
            assert int(g2.parts["value_bits"][n]) == bits(float(old + 0.5))
            # the tombstone's segment id: the first output's batch, segment 0
            t_at = int(g2.refs["tombstone_off"][n])
            assert int.from_bytes(g2.out[t_at + 2 + 8:][:8], "little") == 2000
            assert int.from_bytes(g2.out[t_at + 2 + 16:][:8], "little") == want[n][1]
        add_output(tab, g2, w2)
        # remove, then increment: re-created from zero, version by the tombstone rule
        exp = checked(tab)
        gone = ks[:8]
        gr, wr = rm.remove(tab, exp, gone, what="remove", next_version=210)
        assert wr.summary["removed"] == 8
        rm.add_output(tab, gr, wr)
        exp = checked(tab)
        assert all(exp[k][3] == lc.TOMBSTONE for k in gone)
        nv = 5   # a stale safe version: the tombstone rule must lift every version
        g3, w3 = increment(tab, exp, gone, [(7, 0.0)] * 8, what="after the remove", next_version=nv)
        assert w3.summary["ok"] == w3.summary["created"] == w3.summary["allocated"] == 8
        assert w3.summary["tombstones"] == 0
        for n, k in enumerate(gone):
            assert int(g3.parts["version"][n]) == exp[k][2] + 1 > nv + n
            assert int(g3.parts["value_bits"][n]) == 7
        assert w3.summary["next_version"] == max(exp[k][2] for k in gone) + 2
        add_output(tab, g3, w3)
        assert read_values(tab, gone) == [(OK, exp[k][2] + 1, i64(7)) for k in gone]
    finally:
        tab.close()


# ------------------------------------------------------------------ the sum
F = lambda x: bits(float(x))
DBL_MAX, INF = 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000
# (name, old bits, add_int64, add_double bits, the new bits)
SUMS = [
    ("INT64_MAX + 1 wraps", (1 << 63) - 1, 1, 0, 1 << 63),
    ("UINT64 wraps to 0", M64, 1, 0, 0),
    ("a negative increment", 5, -7, 0, (-2) & M64),
    ("INT64_MIN - 1 wraps", 1 << 63, -1, 0, (1 << 63) - 1),
    ("integer first, then the double on the resulting bits", F(1.5), 2, F(2.0), F(3.5) + 1),
    ("integer first, and the double's tie goes to even", F(1.5), 1, F(2.0), F(3.5)),
    ("both, from zero", 0, 0x4000000000000000, F(1.0), F(3.0)),
    ("add_double 0.0 adds nothing", 5, 0, F(0.0), 5),
    ("add_double -0.0 adds nothing", 5, 0, 0x8000000000000000, 5),
    ("-0.0 leaves a NaN payload alone", 0x7FF0000000000123, 0, 0x8000000000000000, 0x7FF0000000000123),
    ("1.0 + 2^-53: the tie goes to even", F(1.0), 0, F(2.0 ** -53), F(1.0)),
    ("1.0 + 2^-52", F(1.0), 0, F(2.0 ** -52), 0x3FF0000000000001),
    ("1.0 + 3 * 2^-54 rounds up", F(1.0), 0, F(3 * 2.0 ** -54), 0x3FF0000000000001),
    ("2^-1074 + 2^-1074", 1, 0, 1, 2),
    ("a subnormal plus a subnormal", 3, 0, 5, 8),
    ("subnormals into the normal range", 0x000FFFFFFFFFFFFF, 0, 1, 0x0010000000000000),
    ("a subnormal difference", 0x0010000000000000, 0, 0x800FFFFFFFFFFFFF, 1),
    ("DBL_MAX + DBL_MAX", DBL_MAX, 0, DBL_MAX, INF),
    ("inf + -inf", INF, 0, INF | 1 << 63, NAN),
    ("a NaN old value", 0xFFF8000000000001, 0, F(1.0), NAN),
    ("a signalling NaN old value", 0x7FF0000000000001, 0, F(1.0), NAN),
    ("a NaN increment", F(2.0), 0, 0xFFF0000000000555, NAN),
    ("a NaN increment on an absent key", None, 0, 0x7FF8000000000001, NAN),
    ("an absent key, integer", None, -1, 0, M64),
    ("an absent key, double", None, 0, F(-2.5), F(-2.5)),
    ("an absent key, nothing added", None, 0, 0, 0),
    ("x + -x is +0.0", F(2.5), 0, F(-2.5), 0),
]


def case_sum(drv):
    """The sum against numpy float64 (py_sum) and against the bits written
    down above."""
    for name, old, a, d, new in SUMS:
        assert py_sum(old or 0, a, d) == new, name
    lists = [tc.head(1)] + [rc.obj(1, b"sum %d" % i, 3 + i, i64(s[1])) for i, s in enumerate(SUMS)
                            if s[1] is not None]
    tab = drv.table(128, 3)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        keys = [(1, b"sum %d" % i) for i in range(len(SUMS))]
        g, w = increment(tab, exp, keys, [(s[2], s[3]) for s in SUMS], what="sums", next_version=1000)
        assert (g.parts["status"] == OK).all() and w.held_to_the_write
        for i, s in enumerate(SUMS):
            assert int(g.parts["value_bits"][i]) == s[4], (s[0], hex(int(g.parts["value_bits"][i])))
        add_output(tab, g, w)
        assert [v for _, _, v in read_values(tab, keys)] == [s[4].to_bytes(8, "little") for s in SUMS]
    finally:
        tab.close()


# ------------------------------------------------------------- the statuses
GIVEN = rd.GIVEN
ARG = (1, 2.5)   # both summands: a part's third field tells the new value from add_double


def case_reject_rules(drv):
    """Every rule against an absent key, a tombstone, an object of version 0
    and objects of versions around the given one; the third field of every
    part."""
    versions = rd.RULE_VERSIONS
    lists = [tc.head(1)] + [rc.obj(1, b"obj %d" % i, v, i64(100 + i)) for i, v in enumerate(versions)]
    lists += [rc.tomb(1, b"tomb %d" % i, v) for i, v in enumerate(versions)]
    tab = drv.table(256, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        assert exp[(1, b"obj 0")][2:4] == (0, lc.OBJECT)
        for rb in range(16):
            r = {name: (rb >> k) & 1 for k, name in enumerate(rd.RULE_BITS)}
            r["given_version"] = GIVEN
            keys = [(1, b"%s %d" % (kind, i)) for i in range(len(versions)) for kind in (b"obj", b"tomb", b"none")]
            nv = GIVEN + 3
            g, w = increment(tab, exp, keys, [ARG] * len(keys), what=("rules", rb), rules=[dict(r) for _ in keys],
                             next_version=nv)
            assert w.held_to_the_write
            for j, (tid, key) in enumerate(keys):
                st, ver, third = (int(x) for x in g.parts[j])
                if not key.startswith(b"obj"):
                    # no other rule applies to a key that is not there
                    assert st == (DOESNT_EXIST if r["doesnt_exist"] else OK), (rb, key)
                    assert st == OK or (ver, third) == (0, bits(2.5))
                    assert st != OK or (third == py_sum(0, 1, bits(2.5)) and g.refs["tombstone_off"][j] == NONE)
                else:
                    cur = versions[j // 3]
                    assert st == rd.reject(r, cur), (rb, key)
                    if st == OK:
                        assert ver == (cur + 1 if cur else w.versions[j]) and third == py_sum(100 + j // 3, 1, bits(2.5))
                        assert (int(g.refs["tombstone_off"][j]) != NONE) == (cur != 0)
                    else:
                        assert (ver, third) == (cur, bits(2.5)) and int(g.refs["object_off"][j]) == NONE
        # non-boolean rule bytes, rules given for some requests only, bad rules among good ones
        keys = [(1, b"obj 1"), (1, b"obj 2"), (1, b"none"), (1, b"obj 3"), (1, b"obj 4")]
        g, w = increment(tab, exp, keys, [ARG] * 5, what="bytes", next_version=9,
                         rules=[dict(exists=0x80), None, dict(doesnt_exist=2), dict(reserved=1, exists=1), None])
        assert [int(s) for s in g.parts["status"]] == [EXISTS, OK, DOESNT_EXIST, FORMAT_ERROR, OK]
        assert int(g.old[3]["kind"]) == lc.BAD_KEY and g.summary["bad"] == 1
        assert [int(x) for x in g.parts["value_bits"][[0, 2, 3]]] == [bits(2.5)] * 3
    finally:
        tab.close()


VALUE_LENGTHS = [0, 4, 7, 9, 8, 16]


def case_invalid_object(drv):
    """value_len of 0, 4, 7, 9 and 8; the rules come first; an object of
    version 0; the tombstone of an invalid object is never written."""
    lists = [tc.head(1)] + [rc.obj(1, b"len %d" % n, 20 + n, bytes(range(1, n + 1))) for n in VALUE_LENGTHS]
    lists += [rc.obj(1, b"zero", 0, b"four"), rc.obj(1, b"zero 8", 0, i64(9))]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        keys = [(1, b"len %d" % n) for n in VALUE_LENGTHS]
        g, w = increment(tab, exp, keys, [ARG] * len(keys), what="lengths", next_version=50)
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == \
            [(OK if n == 8 else INVALID, 20 + n + (n == 8)) for n in VALUE_LENGTHS]
        assert g.summary["invalid_object"] == 5 and g.summary["ok"] == 1 and g.summary["tombstones"] == 1
        assert all(int(g.parts["value_bits"][i]) == bits(2.5) for i, n in enumerate(VALUE_LENGTHS) if n != 8)
        assert entry_sizes(g.out) == [24 + 11 + 5, 32 + 5]
        # rejectOperation comes before the length test
        g, w = increment(tab, exp, keys[:2], [ARG] * 2, what="rules first", next_version=50,
                         rules=[dict(exists=1), dict(version_le_given=1, given_version=1)])
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(EXISTS, 20), (INVALID, 24)]
        # an object of version 0: found, so its length counts; with 8 bytes it is added to and allocates
        zk = [(1, b"zero"), (1, b"zero 8"), (1, b"zero 8")]
        g, w = increment(tab, exp, zk, [ARG] * 3, what="version 0", next_version=50)
        assert [tuple(int(x) for x in p) for p in g.parts] == \
            [(INVALID, 0, bits(2.5)), (OK, 50, py_sum(9, 1, bits(2.5))), (RETRY, 0, bits(2.5))]
        assert g.summary["created"] == 1 and g.summary["allocated"] == 1
        g, w = increment(tab, exp, zk[:2], [ARG] * 2, what="version 0, must exist", next_version=50,
                         rules=[dict(doesnt_exist=1)] * 2)
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(DOESNT_EXIST, 0)] * 2
    finally:
        tab.close()


def case_duplicates(drv):
    others = [(2, b"other %d" % i) for i in range(24)]
    lists = [tc.head(1), rc.obj(1, b"hot", 4, i64(10)), rc.obj(2, b"other 3", 8, i64(20)), rc.obj(3, b"hot", 6, i64(30)),
             rc.obj(1, b"short", 2, b"abc")]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        rng = np.random.default_rng(3)
        keys = [(1, b"hot")] * 1000 + others
        keys = [keys[i] for i in rng.permutation(len(keys)).tolist()]
        g, w = increment(tab, exp, keys, [(n + 1, 0.0) for n in range(len(keys))], what="hot")
        assert g.summary["ok"] == 25 and g.summary["retry_duplicate"] == 999 and g.summary["created"] == 23
        first = keys.index((1, b"hot"))
        assert tuple(int(x) for x in g.parts[first]) == (OK, 5, 10 + first + 1)   # not chained: the first one's sum
        # a first occurrence that is rejected, or invalid: its copies still get RETRY
        keys = [(1, b"hot"), (1, b"hot"), (2, b"other 3"), (1, b"hot"), (1, b"short"), (1, b"short")]
        g, w = increment(tab, exp, keys, [ARG] * 6, what="rejected first", rules=[dict(exists=1)] + [None] * 5)
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == \
            [(EXISTS, 4), (RETRY, 0), (OK, 9), (RETRY, 0), (INVALID, 2), (RETRY, 0)]
        # a rejected copy behind a served first: RETRY all the same
        g, w = increment(tab, exp, keys[:2], [ARG] * 2, what="rejected copy", rules=[None, dict(exists=1)])
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(OK, 5), (RETRY, 0)]
        # a bad request does not count as a first
        kb, reqs = segments.lookup_queries(keys[:4])
        reqs["reserved"][0] = 1
        g, w = increment(tab, exp, None, [ARG] * 4, what="bad first", packed=(kb, reqs))
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(FORMAT_ERROR, 0), (OK, 5), (OK, 9), (RETRY, 0)]
        # a first occurrence that is cut: its copies still get RETRY with version 0
        keys = [(2, b"other 3"), (1, b"hot"), (1, b"hot"), (2, b"other 3")]
        one = 2 + 24 + 11 + 7 + 2 + 32 + 7
        g, w = increment(tab, exp, keys, [ARG] * 4, what="cut first", cap=one + 10)
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(OK, 9), (RETRY, 4), (RETRY, 0), (RETRY, 0)]
        assert g.summary["retry_full"] == 1 and g.summary["retry_duplicate"] == 2
        # the same bytes under another table id, and a key that is a prefix, are other keys
        keys = [(1, b"hot"), (3, b"hot"), (1, b"ho"), (1, b"hot")]
        g, w = increment(tab, exp, keys, [ARG] * 4, what="identity", next_version=77)
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(OK, 5), (OK, 7), (OK, 77), (RETRY, 0)]
    finally:
        tab.close()


# ------------------------------------------------------ sizes and alignment
# around the lane / group class bound; 220 / 221: the object's payload passes
# 0xFF; 223 / 224: the tombstone's; 65,535: three length bytes
KEY_LENGTHS = [0, 1, 7, 8, 9, LANE_KEY_MAX - 1, LANE_KEY_MAX, LANE_KEY_MAX + 1, LANE_KEY_MAX + 8, 220, 221, 222, 223,
               224, 225, 65535]


def case_key_lengths(drv):
    rng = np.random.default_rng(8)
    keys = [(1, rng.integers(0, 256, kl, dtype=np.uint8).tobytes()) for kl in KEY_LENGTHS]
    lists = [[tc.head(1)] + [rc.obj(1, k, 7 + i, i64(i)) for i, (_, k) in enumerate(keys[:-1])]]
    lists += [[tc.head(2), rc.obj(1, keys[-1][1], 100, i64(5))]]
    tab = drv.table(64, 2)
    try:
        tab.add(drv.batch(lists, cap=128 * KiB))
        exp = checked(tab)
        order = rng.permutation(len(keys)).tolist()
        for ks in (keys, [keys[i] for i in order]):
            g, w = increment(tab, exp, ks, [(3, 0.0)] * len(ks), what="key lengths", cap=512 * KiB, room=512 * KiB,
                             seg_ids=[0x0102030405060708])
            assert g.summary["ok"] == g.summary["tombstones"] == len(keys) and w.held_to_the_write
            sizes = entry_sizes(g.out)
            assert sorted(sizes[0::2]) == [35 + kl for kl in KEY_LENGTHS]
            assert sorted(sizes[1::2]) == [32 + kl for kl in KEY_LENGTHS]
            assert {255, 256, 257} <= set(sizes[0::2]) and {255, 256, 257} <= set(sizes[1::2])
        # created: the object alone
        fresh = [(9, k) for _, k in keys]
        g, w = increment(tab, exp, fresh, [(0, 1.0)] * len(keys), what="created key lengths", cap=512 * KiB,
                         room=512 * KiB)
        assert g.summary["created"] == len(keys) and entry_sizes(g.out) == [35 + kl for kl in KEY_LENGTHS]
    finally:
        tab.close()
    # walked and added: one stride holds the output
    tab = drv.table(64, 2)
    try:
        short = [k for k in keys if len(k[1]) < 300]
        tab.add(drv.batch([[tc.head(1)] + [rc.obj(1, k, 7 + i, i64(i)) for i, (_, k) in enumerate(short)]]))
        exp = checked(tab)
        g, w = increment(tab, exp, short, [(3, 0.0)] * len(short), what="short key lengths")
        add_output(tab, g, w)
        assert read_values(tab, short) == [(OK, 8 + i, i64(i + 3)) for i in range(len(short))]
    finally:
        tab.close()


def case_value_alignment(drv):
    """The old value at every residue mod 16 in its segment, and as the last 8
    bytes of a segment: the key lengths step the values through the residues,
    and a filler object brings the last entry to the segment's end."""
    cap = 4 * KiB
    es = [tc.head(1)]
    keys = []
    at = len(es[0])
    for i in range(48):
        # the value of entry i at residue i mod 16: 29 bytes and the key lie in front of it
        keys.append((1, b"v%02d" % i + b"k" * ((i - at - 29 - 3) % 16)))
        es.append(rc.obj(1, keys[-1][1], 2 + i, i64(0x0807060504030201 * (i + 1))))
        at += len(es[-1])
    last = (1, b"the last one")
    tail = rc.obj(1, last[1], 99, i64(0xF1F2F3F4F5F6F7F8))
    used = sum(len(e) for e in es) + len(tail)
    fill = cap - used - (1 + 2 + 24 + 3 + 4)   # a two-length-byte entry with the key "fill"
    assert fill > 256
    es += [rc.obj(1, b"fill", 1, bytes(fill)), tail]
    assert sum(len(e) for e in es) == cap
    tab = drv.table(128, 2)
    try:
        tab.add(drv.batch([es], cap=cap))
        exp = checked(tab)
        assert {exp[k][5] % 16 for k in keys} == set(range(16))
        assert exp[last][5] + 8 == cap
        ks = keys + [last]
        g, w = increment(tab, exp, ks, [(1, 0.0)] * len(ks), what="value alignment")
        assert g.summary["ok"] == len(ks)
        assert int(g.parts["value_bits"][-1]) == 0xF1F2F3F4F5F6F7F9
        assert all(int(g.parts["value_bits"][i]) == (0x0807060504030201 * (i + 1) + 1) & M64 for i in range(48))
    finally:
        tab.close()


def case_alignment(drv):
    """Every key at source byte offsets 0 to 15 and every entry at destination
    byte offsets 0 to 15: the keys' lengths step the key buffer and the head
    through the residues, `shift` moves the key buffer and the output
    allocation; both classes of key length."""
    rng = np.random.default_rng(5)
    lengths = [int(rng.integers(1, LANE_KEY_MAX + 1)) if rng.random() < 0.6 else int(rng.integers(LANE_KEY_MAX + 1, 90))
               for _ in range(160)]
    keys = [(1, bytes([i]) + rng.integers(0, 256, n - 1, dtype=np.uint8).tobytes()) for i, n in enumerate(lengths)]
    lists = [tc.head(1)] + [rc.obj(1, k, 2 + i, i64(i * i)) for i, (_, k) in enumerate(keys) if i % 3]
    tab = drv.table(512, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        args = [(i, 0.25) for i in range(len(keys))]
        kb, reqs = segments.lookup_queries(keys)
        classes = ((0, LANE_KEY_MAX), (LANE_KEY_MAX + 1, 1 << 16))
        seen = {(lo, what): set() for lo, _ in classes for what in ("object", "tombstone", "key")}
        for shift in range(16):
            g, w = increment(tab, exp, keys, args, what=("alignment", shift), shift=shift, seg_ids=[shift << 40],
                             equiv=shift in (0, 7))
            for lo, hi in classes:
                cls = [j for j in range(len(keys)) if lo <= lengths[j] <= hi]
                tombs = [j for j in cls if int(g.refs["tombstone_off"][j]) != NONE]
                # (the allocations are aligned: the residues of the addresses)
                seen[lo, "object"] |= {(shift + int(g.refs["object_off"][j])) % 16 for j in cls}
                seen[lo, "tombstone"] |= {(shift + int(g.refs["tombstone_off"][j])) % 16 for j in tombs}
                seen[lo, "key"] |= {(shift + int(reqs["key_off"][j])) % 16 for j in tombs}
        assert all(s == set(range(16)) for s in seen.values()), seen
        for align in (4, 16):
            increment(tab, exp, keys, args, what=("aligned", align), align=align)
    finally:
        tab.close()


# -------------------------------------------------------------------- space
def case_space(drv):
    """Capacity 0, one byte short of the first request, exactly at the head,
    the cut at requests 255, 256 and 257 of 600, between an object and its
    tombstone's worth of space; requests that write nothing keep their status
    behind the cut; an allocated version is consumed by a request that is
    cut."""
    n = 600
    keys = [(1, b"sp %d" % i) for i in range(n)]
    absent, rejected, bad, dup = {3, 300, 590}, {5, 400, 595}, {7, 420, 598}, {9: 2, 450: 1, 599: 0}
    invalid = {11, 258}
    lists = [tc.head(1)] + [rc.obj(1, k, 5 + i, b"bad" if i in invalid else i64(i)) for i, (_, k) in enumerate(keys)
                            if i not in absent]
    tab = drv.table(2048, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        for i, j in dup.items():
            keys[i] = keys[j]
        kb, reqs = segments.lookup_queries(keys)
        args = segments.increment_args([(1, 0.0)] * n)
        rules = [None] * n
        for i in rejected:
            rules[i] = dict(exists=1)
        for i in bad:
            reqs["reserved"][i] = 9
        full = Want(drv.oracle, exp, tab.batches, kb, reqs, args, rules, 50)
        quiet = rejected | bad | set(dup) | invalid
        assert full.summary["ok"] == n - len(quiet) and full.summary["created"] == len(absent)
        start = lambda i: int(full.refs["object_off"][i])
        size = lambda i: 2 + 24 + 11 + len(keys[i][1]) + (0 if i in absent else 2 + 32 + len(keys[i][1]))
        first = min(i for i in range(n) if i not in quiet)
        caps = [0, start(first) + size(first) - 1, len(full.out), len(full.out) - 1]
        for i in (255, 256, 257):
            assert i not in quiet and i not in absent
            # inside object i, between it and its tombstone, one short of the tombstone's end, on the end of the
            # request before, inside that
            caps += [start(i) + 5, int(full.refs["tombstone_off"][i]), start(i) + size(i) - 1, start(i), start(i) - 1]
        caps += [start(300) + size(300) - 1, start(300) + size(300)]   # a created object: cut, and exactly fitting
        for cap in caps:
            g, w = increment(tab, exp, None, args, what=("space", cap), packed=(kb, reqs), rules=rules, cap=cap,
                             next_version=50, equiv=False)
            st = [int(s) for s in g.parts["status"]]
            assert all(st[i] == EXISTS and int(g.parts["version"][i]) == 5 + i for i in rejected)
            assert all(st[i] == INVALID and int(g.parts["version"][i]) == 5 + i for i in invalid)
            assert all(st[i] == FORMAT_ERROR for i in bad) and all(st[i] == RETRY for i in dup)
            cut = [i for i in range(n) if i not in quiet and start(i) + size(i) > cap]
            assert all(st[i] == RETRY and int(g.refs["object_off"][i]) == NONE and
                       int(g.refs["tombstone_off"][i]) == NONE and
                       int(g.parts["version"][i]) == (0 if i in absent else 5 + i) for i in cut)
            assert g.summary["retry_full"] == len(cut) and g.summary["out_bytes"] <= cap
            assert g.summary["ok"] + g.summary["retry_full"] == full.summary["ok"]
            assert g.summary["allocated"] == len(absent) and g.summary["next_version"] == 50 + len(absent)
            fit = [i for i in sorted(absent) if i not in cut]
            assert [int(g.parts["version"][i]) for i in fit] == [50 + sorted(absent).index(i) for i in fit]
        # the write sees the same cut (its requests carry no unusable ones: those are left out here)
        good = [i for i in range(n) if i not in bad and i not in invalid]
        kb2, reqs2 = segments.lookup_queries([keys[i] for i in good])
        for cap in (caps[1], caps[4], caps[5], caps[6]):
            g, w = increment(tab, exp, None, args[:len(good)], what=("space, write", cap), packed=(kb2, reqs2),
                             rules=[rules[i] for i in good], cap=cap, next_version=50)
            assert w.held_to_the_write
    finally:
        tab.close()


def case_counts(drv):
    """n_reqs = 0, 1, 255, 256, 257 and 3 * 256 + 1: the tile's edges."""
    keys = [(1, b"count %d" % i) for i in range(769)]
    lists = [tc.head(1)] + [rc.obj(1, k, 1 + i, i64(i)) for i, (_, k) in enumerate(keys) if i % 5]
    tab = drv.table(2048, 2)
    try:
        tab.add(drv.batch([lists]))
        exp = checked(tab)
        for n in (0, 1, 255, 256, 257, 769):
            ks = keys[769 - n:]
            g, w = increment(tab, exp, ks, [(2, 0.0)] * n, what=("count", n), next_version=77)
            assert g.summary["ok"] == n and w.held_to_the_write
            if n == 0:
                assert g.summary == dict(dict.fromkeys(SUMMARY_NAMES, 0), next_version=77) and g.out == b""
                assert g.cert == ac.expected_cert(drv.oracle, b"")
    finally:
        tab.close()


# ------------------------------------------------------------- bad requests
def case_bad_requests(drv):
    lists = [tc.head(1), rc.obj(1, b"good", 2, i64(1)), rc.obj(1, b"", 3, i64(2))]
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
        g, w = increment(tab, exp, None, [ARG] * len(keys), what="bad", packed=(kb, reqs), rules=rules)
        st = [int(s) for s in g.parts["status"]]
        assert st == [OK] + [FORMAT_ERROR] * 6 + [OK, OK], st
        assert (g.parts["version"][1:7] == 0).all() and g.summary["bad"] == 6 and g.summary["ok"] == 3
        assert (g.parts["value_bits"][1:7] == bits(2.5)).all()
        assert int(g.old[8]["kind"]) == lc.ABSENT and all(int(g.old[i]["kind"]) == lc.BAD_KEY for i in range(1, 7))
        # an empty key buffer: the empty key is a key
        reqs = np.zeros(2, lc.KEY)
        reqs["table_id"], reqs["key_len"][1] = 1, 1
        g, w = increment(tab, exp, None, [ARG] * 2, what="no keys", packed=(np.zeros(0, np.uint8), reqs))
        assert [tuple(int(x) for x in p)[:2] for p in g.parts] == [(OK, 4), (FORMAT_ERROR, 0)]
    finally:
        tab.close()


# ------------------------------------------------------- nullable and empty
def case_nullable(drv):
    """Each nullable argument on its own, all NULL and all given; the EINVAL
    cases both forms share."""
    lists = [tc.head(1), rc.obj(1, b"have", 2, i64(1)), rc.obj(2, b"too", 3, i64(2))]
    tab = drv.table(64, 3)
    try:
        tab.add(drv.batch([lists]))
        tab.add(drv.batch([[tc.head(2)], [tc.head(3), rc.obj(1, b"second", 1, i64(3))]]))
        exp = checked(tab)
        keys = [(1, b"have"), (2, b"too"), (1, b"second"), (1, b"fresh")]
        args = [ARG] * 4
        hashes = np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)
        seg_ids = [0x1122334455667788, 7 << 32]
        g0, w0 = increment(tab, exp, keys, args, what="all NULL", want_refs=False, want_old=False)
        g1, w1 = increment(tab, exp, keys, args, what="all given", rules=[None] * 4, hashes=hashes, seg_ids=seg_ids)
        assert g0.refs is None and g0.old is None and g0.out != g1.out and len(g0.out) == len(g1.out)
        ids = [int.from_bytes(g1.out[int(r) + 2 + 8:][:8], "little") for r in g1.refs["tombstone_off"][:3]]
        assert ids == [0x1122334455667788, 0x1122334455667788, (7 << 32) + 1]
        for kw in (dict(rules=[None, dict(exists=1), None, None]), dict(hashes=hashes), dict(seg_ids=seg_ids),
                   dict(want_refs=False), dict(want_old=False)):
            increment(tab, exp, keys, args, what=("one given or missing", sorted(kw)), **kw)
        kb, reqs = segments.lookup_queries(keys)
        try:
            tab.increment_raw(kb, reqs, segments.increment_args(args), 4096, 0)
        except drv.ramcrc.RamcrcError as e:
            assert e.code == drv.ramcrc.EINVAL
        else:
            raise AssertionError("next_version = 0 was accepted")
    finally:
        tab.close()


def case_host_einval(drv):
    """The host form's RAMCRC_EINVAL list."""
    L, R = drv.ramcrc.lib(), drv.ramcrc
    t = R.ReplayTableHost(64, 1)
    try:
        z = np.full(1024, FILL, np.uint8)
        at = lambda o: ctypes.c_void_p(z.ctypes.data + o)
        good = dict(t=t._h, keys=at(0), reqs=at(32), args=at(64), nv=1, out=at(112), cap=64, cert=at(176),
                    parts=at(192), summary=at(256), n=1)
        z[32:56] = 0
        for change in (dict(t=None), dict(nv=0), dict(summary=None), dict(cert=None), dict(reqs=None), dict(args=None),
                       dict(parts=None), dict(out=None), dict(keys=None), dict(n=0xFFFFFFFF)):
            a = dict(good, **change)
            rc_ = L.ramcrc_replay_table_increment_host(a["t"], a["keys"], 16, a["reqs"], a["n"], a["args"], None, None,
                                                       a["nv"], 0, None, a["out"], a["cap"], a["cert"], a["parts"],
                                                       None, None, a["summary"])
            assert rc_ == R.EINVAL, change
        assert (z[:32] == FILL).all() and (z[56:] == FILL).all()
    finally:
        t.close()


def case_spoiled(drv):
    tab = drv.table(4, 2)
    try:
        b = drv.batch([tc.capacity_lists(8)])
        try:
            tab.add(b)
        except drv.ramcrc.RamcrcError:
            pass
        kb, reqs = segments.lookup_queries([(1, b"k")])
        g = tab.increment_raw(kb, reqs, segments.increment_args([ARG]), 4096)
        assert g.summary == SPOILED_SUMMARY
        for a in (g.out_all, g.cert_past, g.parts, g.parts_past, g.refs, g.old):
            assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all()
        assert all(x == FILL32 for x in g.cert)
    finally:
        tab.close()


# ------------------------------------------------------- many requests, numpy
class Large:
    """Many requests of 8-byte keys against a table whose objects have 64-byte
    values and version 0 (segments.object_segments_host), with numpy's
    expectation of the parts, the references and the summary.

    q, want, kb: lookup queries, every second one a present key, with the
    lookup's answers and the key buffer (8 bytes a query).  Every 97th request
    repeats the one before it.  A write first puts 8-byte values over three
    fifths of the present keys (write_requests; walked and added, that batch
    wins); versions_written() takes the versions its parts report.  An
    increment then finds an 8-byte value there (a 45-byte object entry and a
    42-byte tombstone entry), an invalid object for the other present keys, and
    creates the absent ones (45 bytes); the capacity cuts the output inside its
    last tenth."""

    def __init__(self, q, want, kb):
        self.nq = nq = q.shape[0]
        i = np.arange(nq)
        self.dup = i % 97 == 96
        self.src = src = np.where(self.dup, i - 1, i)
        self.kb = kb
        self.reqs = q[src].copy()
        self.hit = want["kind"][src] == lc.OBJECT
        assert (want["version"][src] == 0).all()
        self.sample = self.hit & (src % 10 < 6)
        self.old = (src.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
        self.add_int = (i.astype(np.uint64) * np.uint64(0x0123456789ABCDEF))
        self.add_dbl = np.where(i % 3 == 0, 0.5, 0.0)
        self.args = np.zeros(nq, segments.INCREMENT_ARG_DTYPE)
        self.args["add_int64"], self.args["add_double_bits"] = self.add_int.view(np.int64), self.add_dbl.view(np.uint64)
        self.keys8 = np.ascontiguousarray(kb).reshape(-1, 8)[src]
        self.first = np.flatnonzero(self.sample & ~self.dup)   # each key of the sample once
        # the sum
        new = self.old * self.sample + self.add_int
        with np.errstate(all="ignore"):
            summed = (new.view(np.float64) + self.add_dbl).view(np.uint64)
        summed = np.where(np.isnan(summed.view(np.float64)), np.uint64(NAN), summed)
        self.bits = np.where(self.add_dbl != 0, summed, new)

    def images(self, rows, values):
        """(data, write requests) for the keysAndValue images of `rows`."""
        n = rows.shape[0]
        img = np.zeros((n, 19), np.uint8)
        img[:, 0], img[:, 1] = 1, 8
        img[:, 3:11] = self.keys8[rows]
        img[:, 11:] = np.ascontiguousarray(values).view(np.uint8).reshape(-1, 8)
        wreqs = np.zeros(n, segments.WRITE_REQ_DTYPE)
        wreqs["table_id"], wreqs["data_off"], wreqs["data_len"] = self.reqs["table_id"][rows], 19 * np.arange(n), 19
        return img.reshape(-1), wreqs

    def write_requests(self):
        return self.images(self.first, self.old[self.first])

    def expect(self, versions_written, nv):
        """versions_written: the versions of the first write's parts; nv: the
        increment's next_version."""
        nq, dup, hit, sample = self.nq, self.dup, self.hit, self.sample
        wver = np.zeros(nq, np.uint64)
        wver[self.first] = versions_written
        wver = np.where(dup, np.roll(wver, 1), wver)
        assert (wver[sample] != 0).all()
        served = ~dup
        invalid = served & hit & ~sample
        reach = served & ~invalid
        size = np.where(reach, np.where(sample, 87, 45), 0).astype(np.int64)
        ends = np.cumsum(size)
        self.cap = cap = int(ends[nq * 19 // 20]) + 7
        fits = reach & (ends <= cap)
        self.first_out = int(np.flatnonzero(reach & ~fits)[0])
        created = reach & ~hit
        rank = (np.cumsum(created) - created).astype(np.uint64)
        cur = np.where(sample, wver, np.uint64(0))
        self.parts = np.zeros(nq, PART)
        self.parts["status"] = np.where(dup | (reach & ~fits), RETRY, np.where(invalid, INVALID, OK))
        self.parts["version"] = np.where(fits, np.where(sample, cur + np.uint64(1), np.uint64(nv) + rank),
                                         np.where(dup, np.uint64(0), cur))
        self.parts["value_bits"] = np.where(fits, self.bits, self.add_dbl.view(np.uint64))
        self.refs = np.zeros(nq, REF)
        self.refs["object_off"] = np.where(fits, ends - size, NONE)
        self.refs["tombstone_off"] = np.where(fits & sample, ends - 42, NONE)
        self.head = int(ends[fits][-1])
        self.n_ok, self.n_tomb = int(fits.sum()), int((fits & sample).sum())
        n_ok, n_t = self.n_ok, self.n_tomb
        self.summary = dict(dict.fromkeys(SUMMARY_NAMES, 0), ok=n_ok, created=n_ok - n_t,
                            invalid_object=int(invalid.sum()), retry_duplicate=int(dup.sum()),
                            retry_full=int((reach & ~fits).sum()), tombstones=n_t, allocated=int(created.sum()),
                            next_version=nv + int(created.sum()), out_bytes=self.head, object_bytes=43 * n_ok,
                            tombstone_bytes=40 * n_t, value_bytes=8 * n_ok, key_bytes=11 * n_ok)
        assert n_t > nq // 5 and n_ok - n_t > nq // 3 and self.summary["retry_full"] > 0
        assert self.summary["invalid_object"] > nq // 10
        self.keep = np.flatnonzero(~(hit & ~sample))   # the requests a write can express

    def held(self, g, looked, what=""):
        assert g.summary == self.summary, (what, g.summary, self.summary)
        assert lc.same(g.parts, self.parts), (what, "parts")
        assert lc.same(g.refs, self.refs), (what, "references")
        assert lc.same(g.old, looked), (what, "old results")

    def held_to_the_write(self, g, gw):
        """g: the increment of the kept requests; gw: the write of the images
        of their new values (self.images(self.keep, self.bits[self.keep]))."""
        assert g.summary["invalid_object"] == 0 and g.summary["retry_full"] > 0
        assert gw.out == g.out and gw.cert == g.cert and lc.same(gw.refs, g.refs) and lc.same(gw.old, g.old)
        assert np.array_equal(gw.parts["status"], g.parts["status"])
        assert np.array_equal(gw.parts["version"], g.parts["version"])
        assert all(gw.summary[k] == g.summary[k] for k in wc.SUMMARY_NAMES)


def object_queries(buf, cap, table, nq, seed=9):
    """(key buffer, queries, the lookup's answers) for nq queries against one
    batch of segments.object_segments_host objects with 64-byte values, walked
    into `table`: every second one a present key in a shuffled order, the
    others the same keys under a table id no record has."""
    t = np.asarray(table).astype(np.int64)
    pay = t[:, 1] + 1 + ((t[:, 3] >> 6) & 3) + 1
    at = t[:, 0] * cap + pay
    field = lambda o, n: buf[(at + o)[:, None] + np.arange(n)].copy().view("<u8").reshape(-1)
    table_id, version, key = field(16, 8), field(8, 8), field(27, 8)
    rec = np.random.default_rng(seed).permutation(t.shape[0])[:nq // 2]
    hit = np.arange(nq) % 2 == 0
    q = np.zeros(nq, lc.KEY)
    q["key_len"] = 8
    q["key_off"] = 8 * np.arange(nq)
    q["table_id"][hit] = table_id[rec]
    q["table_id"][~hit] = table_id[rec] ^ (1 << 40)
    keys = np.zeros(nq, "<u8")
    keys[hit] = keys[~hit] = key[rec]
    want = np.zeros(nq, lc.RES)
    want[:] = lc.no_result(lc.ABSENT)
    h = np.flatnonzero(hit)
    want["batch"][h], want["record"][h], want["version"][h] = 0, rec, version[rec]
    want["kind"][h], want["segment"][h] = lc.OBJECT, t[rec, 0]
    want["value_off"][h], want["value_len"][h] = pay[rec] + 35, t[rec, 2] - 35
    return keys.view(np.uint8), q, want


def case_large_on_the_host(drv):
    """The numpy expectation of the GPU suite's large case, on the host at a
    hundredth of its size: held against the host form, which the other cases
    hold against the plain-Python expectation."""
    cap = 64 * KiB
    buf, certs, counts = segments.object_segments_host(4, cap, 64)
    b = tc.HostBatch.__new__(tc.HostBatch)
    b.buf, b.certs, b.cap, b.nseg = buf, certs, cap, 4
    b.status, b.table = ac.host_walk(drv.oracle, buf, certs, 4, cap)
    nq = 2500
    assert b.table.shape[0] == int(counts.sum()) > nq // 2
    kb, q, want = object_queries(buf, cap, b.table, nq)
    tab = drv.table(4096, 3)
    try:
        tab.add(b)
        res, _ = tab.lookup_raw(kb, q)
        assert lc.same(res, want)
        L = Large(q, want, kb)
        data, wreqs = L.write_requests()
        nv = 1 << 33
        gw = tab.write_raw(data, wreqs, cap, nv, TS)
        ns = L.first.shape[0]
        assert gw.summary["ok"] == gw.summary["allocated"] == ns and gw.summary["out_bytes"] == 45 * ns
        wb, bad = tab.batch_of(gw.out, gw.cert)
        assert bad == 0 and tab.add(wb) == 1
        nv += ns + 5
        L.expect(gw.parts["version"], nv)
        looked, _ = tab.lookup_raw(kb, L.reqs)
        g = tab.increment_raw(kb, L.reqs, L.args, L.cap, nv, TS, room=L.cap)
        L.held(g, looked)
        g = tab.increment_raw(kb, L.reqs[L.keep], L.args[L.keep], L.cap, nv, TS, room=L.cap)
        data, wreqs = L.images(L.keep, L.bits[L.keep])
        L.held_to_the_write(g, tab.write_raw(data, wreqs, L.cap, nv, TS, room=L.cap))
    finally:
        tab.close()


# ---------------------------------------------------------------- read-only
def case_read_only(drv, mixed):
    """The table's words are unchanged after the call (the mixed batches hold
    values of other lengths: invalid objects among the served)."""
    tab = drv.table(2000, len(mixed))
    try:
        for b in mixed:
            tab.add(b)
        exp = checked(tab)
        before = tab.state()
        keys = sorted(exp) + [(77, b"not there %d" % i) for i in range(20)]
        looked = lc.lookup(tab, exp, keys, what="before")
        g, w = increment(tab, exp, keys, [ARG] * len(keys), what="read-only", next_version=9)
        assert w.summary["created"] > 0 and w.summary["ok"] + w.summary["invalid_object"] == len(keys)
        assert tab.state() == before, "an increment without an add changed the table"
        assert lc.same(lc.lookup(tab, exp, keys, what="after"), looked)
    finally:
        tab.close()
