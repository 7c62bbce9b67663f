"""Cases and the expectation for a multi-read against the replay table
(ramcrc_replay_table_read_host / _device).

The expectation is plain Python: the lookup expectation of lookup_cases.py
(the sequential replay, held against the live query's winners), then the status
of readObject and rejectOperation (src/ObjectManager.cc:324-369, :2893-2907),
the part bytes (MultiOp::Response::ReadPart and the object's keys and value or
its value, src/WireFormat.h:1140-1155, src/Object.cc:279-291) and the
truncation of MasterService::multiRead (src/MasterService.cc:1364-1375),
restated here independently of the library.  The tests hold it against
tests/golden/multi_read_ref.json before any call is held against it.
"""
import struct

import numpy as np

from ramcloud_amd import segments

import lookup_cases as lc
import partition_cases as pc
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
FILL = lc.FILL
FILL32 = lc.FILL32
FILL64 = 0xA5A5A5A5A5A5A5A5
HUGE = 1 << 62
NONE = segments.READ_NONE
OK, DOESNT_EXIST, EXISTS, WRONG_VERSION, FORMAT_ERROR = (
    segments.STATUS_OK, segments.STATUS_OBJECT_DOESNT_EXIST, segments.STATUS_OBJECT_EXISTS,
    segments.STATUS_WRONG_VERSION, segments.STATUS_REQUEST_FORMAT_ERROR)
SUMMARY_NAMES = segments.READ_SUMMARY_DTYPE.names
STATUS_FIELD = {OK: "ok", DOESNT_EXIST: "doesnt_exist", EXISTS: "object_exists",
                WRONG_VERSION: "wrong_version", FORMAT_ERROR: "bad"}
RULE_BITS = ("doesnt_exist", "exists", "version_le_given", "version_ne_given")
SPOILED_SUMMARY = dict(dict.fromkeys(SUMMARY_NAMES, 0), spoiled=1)


# ---------------------------------------------------------- the expectation
def reject(rules, version):
    """rejectOperation: `rules` a dict (missing entries are 0) or None."""
    r = rules or {}
    if version == 0:
        return DOESNT_EXIST if r.get("doesnt_exist") else OK
    if r.get("exists"):
        return EXISTS
    if r.get("version_le_given") and version <= r.get("given_version", 0):
        return WRONG_VERSION
    if r.get("version_ne_given") and version != r.get("given_version", 0):
        return WRONG_VERSION
    return OK


def payloads(batches):
    """key -> the payload bytes of its winner when that is an object."""
    exp = lc.expectation(batches)
    out = {}
    for key, (b, r, _, kind, _, _, _) in exp.items():
        if kind == lc.OBJECT:
            seg, off, ln, hdr = (int(x) for x in batches[b].table[r])
            at = seg * batches[b].cap + off + 1 + ((hdr >> 6) & 3) + 1
            out[key] = batches[b].buf[at:at + ln].tobytes()
    return exp, out


def one_part(exp, pays, key, rules, value_only, bad=False):
    """(status, version, data, value bytes, key bytes) of one query."""
    if bad or (rules or {}).get("reserved"):
        return FORMAT_ERROR, 0, b"", 0, 0
    found = exp.get((int(key[0]), bytes(key[1])))
    if found is None or found[3] != lc.OBJECT:
        return DOESNT_EXIST, 0, b"", 0, 0
    version = found[2]
    status = reject(rules, version)
    if status != OK:
        return status, version, b"", 0, 0
    pay = pays[(int(key[0]), bytes(key[1]))]
    vo, vl = lc.value_range(pay)
    data = pay[vo:vo + vl] if value_only else pay[24:]
    return OK, version, data, vl, len(pay) - 24 - vl


class Want:
    """What a read must give: reply bytes, part offsets, summary, parts."""

    def __init__(self, exp, pays, keys, rules, value_only, cap, bad=()):
        self.parts, self.off, self.ends = [], [], []
        self.summary = dict.fromkeys(SUMMARY_NAMES, 0)
        reply, at, open_ = [], 0, True
        for i, key in enumerate(keys):
            status, version, data, vb, kb = one_part(exp, pays, key, rules[i] if rules else None,
                                                     value_only, i in bad)
            part = struct.pack("<IQI", status, version, len(data)) + data
            self.ends.append((self.ends[-1] if self.ends else 0) + len(part))
            if open_ and at + len(part) <= cap:
                self.off.append(at)
                self.parts.append((status, version, data))
                reply.append(part)
                at += len(part)
                self.summary["returned"] += 1
                self.summary[STATUS_FIELD[status]] += 1
                self.summary["value_bytes"] += vb
                self.summary["key_bytes"] += kb
            else:
                open_ = False
                self.off.append(NONE)
        self.summary["reply_bytes"] = at
        self.reply = b"".join(reply)
        assert len(self.reply) == at


def summary_dict(s):
    return {k: int(s[k]) for k in SUMMARY_NAMES}


def longest_payload(batches):
    return max([int(b.table[:, 2].max()) for b in batches if b.table.shape[0]], default=0)


# ------------------------------------------------------------------ drivers
class Got:
    """One call's outputs as numpy: reply (the bytes before reply_bytes),
    part_off, results, summary."""


def _check_got(g, n, want_off, want_res):
    assert (g.reply_all[g.summary["reply_bytes"]:] == FILL).all(), "a byte at or past reply_bytes was written"
    assert (g.summary_past == FILL32).all(), "a word past the summary was written"
    if want_off:
        assert (g.off_all[n:] == FILL64).all(), "a word past part_off was written"
    if want_res:
        assert (g.res_all[n * 32:] == FILL).all(), "a result past the queries was written"


class HostTab(lc.HostTab):
    def read_raw(self, kb, q, cap, rules=None, value_only=False, hashes=None, want_off=True,
                 want_res=True, shift=0):
        """ramcrc_replay_table_read_host on buffers pre-filled with 0xA5."""
        import ctypes
        n = q.shape[0]
        g = Got()
        room = min(cap, n * (16 + longest_payload(self.batches)))
        g.reply_all = np.full(room + 64 + shift, FILL, np.uint8)[shift:]
        g.off_all = np.full(n + 4, FILL64, np.uint64)
        g.res_all = np.full((n + 4) * 32, FILL, np.uint8)
        sm = np.full(12, FILL64, np.uint64)
        kb = np.ascontiguousarray(kb, np.uint8)
        q = np.ascontiguousarray(q)
        rl = None if rules is None else np.ascontiguousarray(segments.read_rules(rules))
        hs = None if hashes is None else np.ascontiguousarray(hashes, np.uint64)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None
        rcode = self.drv.ramcrc.lib().ramcrc_replay_table_read_host(
            self.t._h, p(kb), kb.size, p(q), n, p(hs), p(rl), 1 if value_only else 0,
            ctypes.c_void_p(g.reply_all.ctypes.data), cap, p(g.off_all) if want_off else None,
            p(g.res_all) if want_res else None, p(sm))
        assert rcode == 0, rcode
        g.summary = summary_dict(sm[:10].view(segments.READ_SUMMARY_DTYPE)[0])
        g.summary_past = sm[10:].view(np.uint32)
        _check_got(g, n, want_off, want_res)
        g.reply = g.reply_all[:g.summary["reply_bytes"]].tobytes()
        g.off = g.off_all[:n] if want_off else None
        g.results = g.res_all[:n * 32].view(lc.RES) if want_res else None
        return g


class HostDriver(lc.HostDriver):
    def table(self, key_cap, max_batches):
        return HostTab(self, key_cap, max_batches)


class Read:
    """One ramcrc_replay_table_read_device call: every output pre-filled with
    0xA5 and longer than the call may write; the reply starts `shift` bytes
    into its allocation.  Read back after check()."""

    def __init__(self, ctx, t, kb, q, cap, room, rules=None, value_only=False, hashes=None,
                 want_off=True, want_res=True, shift=0, check=True):
        import torch
        fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
        self.n = n = q.shape[0]
        self.want_off, self.want_res = want_off, want_res
        self.d_keys = torch.from_numpy(np.ascontiguousarray(kb)).cuda() if kb.size else None
        raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1)
        self.d_q = torch.from_numpy(raw.copy()).cuda().view(torch.int64) if n else None
        self.d_rules = None
        if rules is not None and n:
            rl = segments.read_rules(rules).view(np.uint8).reshape(-1)
            self.d_rules = torch.from_numpy(rl.copy()).cuda().view(torch.int64)
        if isinstance(hashes, np.ndarray):
            hashes = torch.from_numpy(hashes.astype(np.uint64).view(np.int64)).cuda()
        self.d_reply = fill(room + 64 + shift, torch.uint8)[shift:]
        self.d_off = fill((n + 4) * 8, torch.int64) if want_off else None
        self.d_res = fill((n + 4) * 32, torch.int32) if want_res else None
        self.d_sum = fill(12 * 8, torch.int64)
        if cap <= room + 64:
            t.read(self.d_keys, self.d_q, self.d_reply, self.d_sum, rules=self.d_rules,
                   value_only=value_only, part_off=self.d_off, results=self.d_res, key_hash=hashes,
                   keys_bytes=kb.size, n_queries=n, reply_cap=cap)
        else:   # a limit beyond any buffer: the call itself, without the wrapper's size check
            from ramcloud_amd import ramcrc
            ptr = lambda x: None if x is None else x.data_ptr()
            ramcrc._check(ramcrc.lib().ramcrc_replay_table_read_device(
                t._h, ptr(self.d_keys), kb.size, ptr(self.d_q), n, ptr(hashes), ptr(self.d_rules),
                1 if value_only else 0, ptr(self.d_reply), cap, ptr(self.d_off), ptr(self.d_res),
                ptr(self.d_sum), torch.cuda.current_stream().cuda_stream), "read")
        if check:
            ctx.check()
            self.read()

    def read(self):
        n = self.n
        sm = self.d_sum.cpu().numpy().view(np.uint64)
        self.summary = summary_dict(sm[:10].view(segments.READ_SUMMARY_DTYPE)[0])
        self.summary_past = sm[10:].view(np.uint32)
        self.reply_all = self.d_reply.cpu().numpy()
        self.off_all = self.d_off.cpu().numpy().view(np.uint64) if self.want_off else None
        self.res_all = self.d_res.cpu().numpy().view(np.uint8) if self.want_res else None
        self.reply = self.reply_all[:min(self.summary["reply_bytes"], self.reply_all.size)].tobytes()
        self.off = self.off_all[:n] if self.want_off else None
        self.results = self.res_all[:n * 32].view(lc.RES) if self.want_res else None


class DeviceTab(lc.DeviceTab):
    """A table on the device with its twin on the host: every read is held
    against the twin's, byte for byte."""

    def __init__(self, drv, key_cap, max_batches):
        lc.DeviceTab.__init__(self, drv, key_cap, max_batches)
        self.host = HostTab.__new__(HostTab)
        self.host.drv, self.host.t, self.host.batches = drv, self.twin, self.batches

    def reset(self):
        lc.DeviceTab.reset(self)
        self.host.batches = self.batches

    def read_raw(self, kb, q, cap, rules=None, value_only=False, hashes=None, want_off=True,
                 want_res=True, shift=0):
        n = q.shape[0]
        room = min(cap, n * (16 + longest_payload(self.batches)))
        g = Read(self.drv.ctx, self.t, kb, q, cap, room, rules, value_only, hashes, want_off, want_res,
                 shift)
        _check_got(g, n, want_off, want_res)
        h = self.host.read_raw(kb, q, cap, rules, value_only, hashes, want_off, want_res)
        assert h.summary == g.summary, ("host and device summaries differ", h.summary, g.summary)
        assert h.reply == g.reply, "host and device replies differ"
        assert not want_off or np.array_equal(h.off, g.off), "host and device part offsets differ"
        assert not want_res or lc.same(h.results, g.results), "host and device results differ"
        return g


class DeviceDriver(lc.DeviceDriver):
    def table(self, key_cap, max_batches):
        return DeviceTab(self, key_cap, max_batches)


def read(tab, exp_pays, keys, cap=HUGE, rules=None, value_only=False, hashes=None, bad=(), what="",
         align=1, shift=0, packed=None, **kw):
    """The read of `keys` against the expectation; `packed`: the (key buffer,
    queries) to send instead of packing `keys`.  The results are held against
    a lookup's, bit for bit.  Returns (the call's outputs, the Want)."""
    exp, pays = exp_pays
    kb, q = packed if packed is not None else segments.lookup_queries(keys, align)
    if shift:
        kb = np.concatenate([np.full(shift, 0xEE, np.uint8), kb])
        q = q.copy()
        q["key_off"] += shift
    if "reply_shift" in kw:
        kw["shift"] = kw.pop("reply_shift")
    g = tab.read_raw(kb, q, cap, rules, value_only, hashes, **kw)
    w = Want(exp, pays, keys, rules, value_only, cap, bad)
    assert g.summary == w.summary, (what, g.summary, w.summary)
    assert g.reply == w.reply, (what, "reply bytes", first_difference(g.reply, w.reply))
    if g.off is not None:
        assert g.off.tolist() == w.off, (what, "part offsets")
    if g.results is not None:
        looked, _ = tab.lookup_raw(kb, q, hashes)
        assert lc.same(g.results, looked), (what, "results differ from the lookup's")
    assert segments.multi_read_parts(g.reply, g.summary["returned"]) == w.parts, what
    return g, w


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return len(a), len(b), n


def checked(tab):
    """(lookup expectation, payloads) for the table as it stands, the former
    held against the live query's winners."""
    exp, pays = payloads(tab.batches)
    assert lc.check_winners(exp, tab.batches, tab.winners()) > 0 or not exp
    return exp, pays


# ------------------------------------------------------------------ goldens
def golden():
    return pc.load("multi_read_ref.json")


def check_expectation_against_golden(ref):
    """reject() against every line of the reference's rejectOperation test;
    returns how many lines."""
    for line in ref["reject"]:
        assert reject(line["rules"], line["version"]) == line["status"], line
    return len(ref["reject"])


def scenario_lists(sc):
    """One entry list for a golden scenario: objects written in order, versions
    as the reference's test sees them."""
    return [tc.head(1)] + [rc.obj(sc["table_id"], k.encode(), ver, v.encode())
                           for k, v, ver in sc["objects"]]


def case_goldens(drv):
    ref = golden()
    assert check_expectation_against_golden(ref) == 9
    # every line of rejectOperation, through the library: an object of the
    # line's version, read under the line's rules
    lines = ref["reject"]
    es = [tc.head(1)] + [rc.obj(1, b"line %d" % n, ln["version"], b"v") for n, ln in enumerate(lines)]
    tab = drv.table(64, 1)
    try:
        tab.add(drv.batch([es]))
        g, w = read(tab, checked(tab), [(1, b"line %d" % n) for n in range(len(lines))],
                    rules=[ln["rules"] for ln in lines], what="rejectOperation")
        assert [p[0] for p in w.parts] == [ln["status"] for ln in lines]
    finally:
        tab.close()
    for sc in ref["scenarios"]:
        tab = drv.table(64, 1)
        try:
            tab.add(drv.batch([scenario_lists(sc)]))
            ep = checked(tab)
            keys = [(sc["table_id"], k.encode()) for k in sc["queries"]]
            for value_only in (False, True):
                g, w = read(tab, ep, keys, value_only=value_only, what=sc["name"])
                for part, line in zip(w.parts, sc["parts"]):
                    assert part[0] == line["status"], sc["name"]
                    if line["status"] == OK:
                        assert part[1] == line["version"] and part[2].endswith(line["value"].encode())
                        assert value_only or len(part[2]) == line["length"], sc["name"]
            for c in sc.get("caps", []):
                g, w = read(tab, ep, keys, cap=c["reply_cap"], what=(sc["name"], c))
                assert g.summary["returned"] == c["returned"], (sc["name"], c)
        finally:
            tab.close()


# ---------------------------------------------------------------- scenarios
def case_relations(drv):
    """tc.relation_lists() across two and three batches, read after every add
    in both modes: a tombstone winner is status 3, the stale pick goes from 3
    to OK."""
    bs = [drv.batch([es]) for es in tc.relation_lists()]
    keys = lc.all_keys(bs) + [(4, b"stale pick, never")]
    stale = keys.index((4, b"stale pick"))
    seen = []
    tab = drv.table(2000, 3)
    try:
        for k, b in enumerate(bs):
            tab.add(b)
            ep = checked(tab)
            g, w = read(tab, ep, keys, what=("after add", k))
            read(tab, ep, keys, value_only=True, what=("value only, after add", k))
            seen.append(w.parts[stale][:2])
            tombs = [i for i, key in enumerate(keys) if ep[0].get(key, (0,) * 4)[3] == lc.TOMBSTONE]
            assert tombs and all(w.parts[i] == (DOESNT_EXIST, 0, b"") for i in tombs)
            assert w.parts[-1] == (DOESNT_EXIST, 0, b"")
    finally:
        tab.close()
    assert seen[0] == (DOESNT_EXIST, 0) and seen[1] == (OK, 7) and seen[2] == (OK, 7)


GIVEN = 0x400000001
RULE_VERSIONS = [0, 1, GIVEN - 1, GIVEN, GIVEN + 1, 1 << 63]


def case_reject_rules(drv):
    """Every rule bit alone and combined against versions 0, 1, given - 1,
    given, given + 1 and 2^63; a bit is set when its byte is not 0; no rules
    at all."""
    es = [tc.head(1)] + [rc.obj(1, b"version %d" % n, v, b"value %d" % n)
                         for n, v in enumerate(RULE_VERSIONS)]
    keys, rules = [], []
    for mask in range(16):
        for n in range(len(RULE_VERSIONS)):
            keys.append((1, b"version %d" % n))
            r = {name: (0x80 if mask == 15 else 1) for b, name in enumerate(RULE_BITS) if mask >> b & 1}
            r["given_version"] = GIVEN
            rules.append(r)
    tab = drv.table(64, 1)
    try:
        tab.add(drv.batch([es]))
        ep = checked(tab)
        g, w = read(tab, ep, keys, rules=rules, what="rules")
        st = lambda mask, n: w.parts[mask * len(RULE_VERSIONS) + n][0]
        assert [st(0, n) for n in range(6)] == [OK] * 6
        assert st(1, 0) == DOESNT_EXIST and [st(1, n) for n in range(1, 6)] == [OK] * 5
        assert st(2, 0) == OK and [st(2, n) for n in range(1, 6)] == [EXISTS] * 5
        assert [st(4, n) for n in range(6)] == [OK, WRONG_VERSION, WRONG_VERSION, WRONG_VERSION, OK, OK]
        assert [st(8, n) for n in range(6)] == [OK, WRONG_VERSION, WRONG_VERSION, OK, WRONG_VERSION,
                                                WRONG_VERSION]
        assert [st(15, n) for n in range(6)] == [DOESNT_EXIST] + [EXISTS] * 5
        # a rejected object keeps its version and sends no data
        assert w.parts[2 * 6 + 3] == (EXISTS, GIVEN, b"") and w.parts[1 * 6 + 0] == (DOESNT_EXIST, 0, b"")
        assert set(g.summary[f] > 0 for f in ("ok", "doesnt_exist", "object_exists", "wrong_version")) == {True}
        read(tab, ep, keys, rules=rules, value_only=True, what="rules, value only")
        g, w = read(tab, ep, keys, rules=None, what="no rules")
        assert g.summary["ok"] == len(keys)
    finally:
        tab.close()


def case_multi_key(drv):
    """Objects of 0, 1, 2 and 3 keys with values of 0, 1 and 300 bytes, and
    the object whose keys run past its payload: value-only gives length 0,
    keys-and-value still sends the payload from 24."""
    lists, want = lc.multi_key_lists()
    b = drv.batch(lists)
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        ep = checked(tab)
        keys = sorted(want)
        g, w = read(tab, ep, keys, value_only=True, what="values")
        for key, part in zip(keys, w.parts):
            assert part[0] == OK and part[2] == (want[key] or b""), key
        g, w = read(tab, ep, keys, what="keys and values")
        for key, part in zip(keys, w.parts):
            assert part[0] == OK and part[2] == ep[1][key][24:] and len(part[2]) >= 1
            if want[key] is not None:
                assert part[2].endswith(want[key])
        past = w.parts[keys.index((5, b"past"))][2]
        assert past[0] == 3 and past.endswith(b"pastxyzz")
        assert g.summary["value_bytes"] == sum(len(v or b"") for v in want.values())
        assert g.summary["key_bytes"] == sum(len(ep[1][k]) - 24 - len(want[k] or b"") for k in keys)
    finally:
        tab.close()


def alignment_lists():
    """Objects with values of 0 .. 80 bytes under keys of 4 .. 16 bytes, so that
    values and payloads begin at every residue mod 16; then 16 steering objects
    with values of 0 .. 15 bytes."""
    es = [tc.head(1)]
    for n in range(81):
        es.append(rc.obj(2, b"al%02d" % n + b"k" * (n * 7 % 13), 1 + n, bytes((n + j) & 0xFF for j in range(n))))
    for n in range(16):
        es.append(rc.obj(3, b"steer %02d" % n, 1, b"s" * n))
    return [es]


def case_alignment(drv):
    """Data lengths 0 .. 80; all 16 x 16 (source, destination) residues of a
    part's data, the destination steered by the previous part's length, at two
    bases of the reply; every present key at every residue of the key buffer."""
    b = drv.batch(alignment_lists())
    tab = drv.table(256, 1)
    try:
        tab.add(b)
        ep = checked(tab)
        exp, pays = ep
        targets = [k for k in sorted(exp) if k[0] == 2]
        steers = [(3, b"steer %02d" % n) for n in range(16)]
        assert [lc.value_range(pays[k])[1] for k in targets] == list(range(81))
        read(tab, ep, targets, value_only=True, what="lengths 0..80")
        read(tab, ep, targets, what="lengths 0..80 with keys")
        for value_only in (True, False):
            size = lambda k: 16 + len(one_part(exp, pays, k, None, value_only)[2])

            def src_res(key):   # where the part's data begins in its segment buffer, mod 16
                _, r, _, _, seg, voff, _ = exp[key]
                _, off, _, hdr = (int(x) for x in b.table[r])
                return (seg * b.cap + (voff if value_only else off + 1 + ((hdr >> 6) & 3) + 1 + 24)) % 16
            by_res = {}
            for k in targets:
                if size(k) - 16 >= 40:   # a few granules and both edges
                    by_res.setdefault(src_res(k), k)
            assert sorted(by_res) == list(range(16)), sorted(by_res)
            steer_by = {size(k) % 16: k for k in steers}
            assert len(steer_by) == 16
            keys, at, pairs = [], 0, set()
            for s in range(16):
                for d in range(16):
                    k = steer_by[(d - at) % 16]
                    keys.append(k)
                    at += size(k)
                    assert at % 16 == d   # the target's header, and its data 16 bytes on
                    pairs.add((s, d))
                    keys.append(by_res[s])
                    at += size(by_res[s])
            assert len(pairs) == 256
            for reply_shift in (0, 5):
                read(tab, ep, keys, value_only=value_only, what=("residues", value_only, reply_shift),
                     reply_shift=reply_shift)
        present = targets[::9] + [steers[7]]
        for shift in range(16):
            read(tab, ep, present, what=("key residue", shift), align=16, shift=shift)
    finally:
        tab.close()


SIZE_CLASSES = [15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 200 * KiB]


def case_size_classes(drv):
    """Values around every threshold of the copy (lane groups up to 256 bytes
    and below 2 KiB, a wave below 64 KiB, the workgroup from there) in one
    request, in both orders and both modes."""
    rng = np.random.default_rng(23)
    es = [tc.head(1)] + [rc.obj(1, b"size %d" % n, 1, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                         for n in SIZE_CLASSES]
    b = drv.batch([es], cap=512 * KiB)
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        ep = checked(tab)
        keys = [(1, b"size %d" % n) for n in SIZE_CLASSES]
        for order in (keys, keys[::-1]):
            for value_only in (True, False):
                g, w = read(tab, ep, order, value_only=value_only, what=("size classes", value_only))
                assert g.summary["ok"] == len(keys) and g.summary["value_bytes"] == sum(SIZE_CLASSES)
    finally:
        tab.close()


def case_truncation(drv):
    """A 12-part request (objects of several lengths, absent keys, a
    tombstone, a rejected object) under every limit that matters."""
    es = [tc.head(1)] + [rc.obj(1, b"t%d" % n, 2 + n, b"v" * ln) for n, ln in
                         enumerate([0, 1, 15, 16, 17, 40, 300, 5])] + [rc.tomb(1, b"dead", 9)]
    keys = [(1, b"t0"), (1, b"t6"), (1, b"absent"), (1, b"t1"), (1, b"t2"), (1, b"dead"), (1, b"t3"),
            (1, b"t7"), (1, b"t4"), (1, b"absent 2"), (1, b"t5"), (1, b"t1")]
    rules = [None] * 12
    rules[7] = dict(exists=1)
    tab = drv.table(64, 1)
    try:
        tab.add(drv.batch([es]))
        ep = checked(tab)
        full = Want(ep[0], ep[1], keys, rules, False, HUGE)
        assert len(full.ends) == 12 and full.summary["returned"] == 12
        errors = [i for i, p in enumerate(full.parts) if p[0] != OK]
        assert errors == [2, 5, 7, 9]
        caps = [0, 15, 16, HUGE] + full.ends + [e - 1 for e in full.ends]
        for cap in caps:
            g, w = read(tab, ep, keys, cap=cap, rules=rules, what=("cap", cap))
            n = g.summary["returned"]
            assert n == sum(e <= cap for e in full.ends)
            assert g.summary["reply_bytes"] == (full.ends[n - 1] if n else 0)
            assert g.off[n:].tolist() == [NONE] * (12 - n)
        # the first part that is not returned is a 16-byte error part
        g, w = read(tab, ep, keys, cap=full.ends[2] - 1, rules=rules, value_only=True, what="value only")
        g, w = read(tab, ep, keys, cap=full.ends[2] - 1, rules=rules)
        assert g.summary["returned"] == 2 and full.ends[2] - full.ends[1] == 16
    finally:
        tab.close()


def case_bad_queries(drv):
    """The four unusable queries of the lookup and a nonzero `reserved` in the
    rules, among good ones: status 9 each, and the call goes on."""
    bs = [drv.batch(ls) for ls in lc.identity_lists()]
    tab = drv.table(256, 2)
    try:
        for b in bs:
            tab.add(b)
        ep = checked(tab)
        good = lc.identity_keys()[3:12]
        keys = good + [(1, b"absent")] + good[:5] + [good[-1]]
        kb, q = segments.lookup_queries(keys)
        n = len(good) + 1
        q["key_len"][n] = 65536
        q["reserved"][n + 1] = 1
        q["key_off"][n + 2], q["key_len"][n + 2] = kb.size - 3, 4    # ends at keys_bytes + 1
        q["key_off"][n + 3] = (1 << 64) - 1
        rules = [None] * len(keys)
        rules[n + 4] = dict(reserved=1)
        rules[0] = dict(reserved=0x80000000, exists=1)
        for hashes in (None, np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)):
            g, w = read(tab, ep, keys, rules=rules, hashes=hashes, bad=range(n, n + 4), packed=(kb, q),
                        what="bad queries")
            assert g.summary["bad"] == 6 and g.summary["returned"] == len(keys)
            assert w.parts[n + 4] == (FORMAT_ERROR, 0, b"") and w.parts[-1][0] in (OK, DOESNT_EXIST)
            # the rules' reserved word is not the query's: the lookup result stands
            assert g.results["kind"][n + 4] != lc.BAD_KEY and (g.results["kind"][n:n + 4] == lc.BAD_KEY).all()
    finally:
        tab.close()


def case_duplicates(drv):
    """One key 1,000 times: every copy gets its own part and its own data."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries() + [rc.obj(1, b"dup", 3, b"thirty-seven bytes of a value, twice.")]])
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        ep = checked(tab)
        g, w = read(tab, ep, [(1, b"dup")] * 1000 + [(1, b"x")] * 3, value_only=True, what="duplicates")
        assert g.summary["ok"] == 1000 and g.summary["doesnt_exist"] == 3
        assert len(set(w.parts[:1000])) == 1 and g.summary["reply_bytes"] == 1000 * (16 + 37) + 48
    finally:
        tab.close()


def case_nullable_and_empty(drv):
    """n_queries = 0, each nullable argument NULL in turn, two tables on one
    context."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    hot = drv.batch([[tc.head(2), rc.obj(1, b"x", 9, b"the other table's")]])
    tab, other = drv.table(64, 1), drv.table(64, 1)
    try:
        tab.add(b)
        other.add(hot)
        ep, ep_o = checked(tab), checked(other)
        g = tab.read_raw(np.zeros(0, np.uint8), np.zeros(0, lc.KEY), HUGE)
        assert g.summary == dict.fromkeys(SUMMARY_NAMES, 0) and g.reply == b""
        g = tab.read_raw(np.zeros(0, np.uint8), np.zeros(0, lc.KEY), 0, want_off=False, want_res=False)
        assert g.summary == dict.fromkeys(SUMMARY_NAMES, 0)
        keys = [(1, b"x"), (1, b"y"), (1, b"q")]
        given = np.array([pc.key_hash(t, k) for t, k in keys], np.uint64)
        base, _ = read(tab, ep, keys, rules=[None] * 3, hashes=given, what="everything given")
        for kw in (dict(hashes=given), dict(rules=[None] * 3), dict(want_off=False), dict(want_res=False),
                   dict(want_off=False, want_res=False)):
            g, _ = read(tab, ep, keys, what=("nullable", sorted(kw)), **kw)
            assert g.reply == base.reply and g.summary == base.summary
        read(tab, ep, [(1, b"")], what="no key bytes")
        a, _ = read(tab, ep, [(1, b"x")], value_only=True)
        o, wo = read(other, ep_o, [(1, b"x")], value_only=True)
        assert a.summary["doesnt_exist"] == 1 and wo.parts == [(OK, 9, b"the other table's")]
    finally:
        tab.close()
        other.close()


def case_read_only(drv, mixed):
    """Stats, live lists and winners are bit-identical before and after reads;
    a read between two adds changes no later answer."""
    tab = drv.table(1000, 4)
    try:
        tab.add(mixed[0])
        tab.add(mixed[1])
        ep2 = checked(tab)
        keys = lc.all_keys(mixed) + [(1, b"absent")]
        before = tab.state()
        a, _ = read(tab, ep2, keys, what="first")
        b, _ = read(tab, ep2, keys, what="second")
        read(tab, ep2, keys, value_only=True, cap=1000, what="truncated")
        assert a.reply == b.reply and tab.state() == before
        tab.add(mixed[2])
        tab.add(mixed[3])
        ep4 = checked(tab)
        c, _ = read(tab, ep4, keys, what="after two more adds")
        fresh = drv.table(1000, 4)
        try:
            for m in mixed:
                fresh.add(m)
            assert fresh.state() == tab.state()
            d, _ = read(fresh, ep4, keys, what="a table that was never read")
            assert c.reply == d.reply
        finally:
            fresh.close()
    finally:
        tab.close()
