"""ramcrc_recovery_partition_device: key hash, tablet lookup and liveness for
every walked record on the GPU (the placement decision of
RecoverySegmentBuilder::build, src/RecoverySegmentBuilder.cc:74-201).

The record table comes from ctx.segment_walk on the device.  The device list,
counters and hashes must equal the host form's and partition_cases.expected's
(plain Python) exactly; the hash test compares with the reference's own hashes
in tests/golden/key_hash_ref.json and the chain test with the
RecoverySegmentBuilderTest scenarios of recovery_build_ref.json.  Every output
is pre-filled with 0xA5, so a write past the list's end shows."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc
from append_cases import Walked, _u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20
ALL = (1 << 64) - 1
OK, BAD, MAL = segments.SEG_OK, segments.SEG_SOURCE_BAD, segments.SEG_MALFORMED
TABLE_IDS = [0, 1, 82, (1 << 32) + 1, ALL]


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. hash
def _hash_segment(cases):
    """Objects whose keys (fixture keys of 0 .. 64 bytes) start at every
    residue mod 16 -- the value of the record before pads the next key into
    place -- then tombstones and objects with the long fixture keys, a key
    that ends with its record and one that runs a byte past it."""
    sweep = {len(k) // 2: (t, bytes.fromhex(k), h) for t, k, h in cases[3:72]}   # by key length
    # [type, table id, key, value length, expected hash, wanted residue]
    recs = [[pc.OBJ, *sweep[n][:2], 0, sweep[n][2], r] for n in range(65) for r in range(16)]
    for n in (255, 256, 4095, 65535):
        t, key, h = sweep[n]
        recs.append([pc.OBJ if n == 256 else pc.OBJTOMB, t, key, 3, h, None])
    t33, key, h = sweep[33]
    recs.append([pc.OBJ, t33, key, 0, h, None])                # the key ends with the record
    es, want, pos = [pc.entry(pc.SEGHEADER, pc.seg_header(3))], [0], 26
    payload = lambda ty, t, key, v: pc.obj(t, key, b"\x5a" * v) if ty == pc.OBJ else pc.tomb(t, key)
    for i, (ty, t, key, v, h, r) in enumerate(recs):
        if r is not None:
            # the previous object's value grows until this key starts at residue r
            pty, pt, pkey, pv = recs[i - 1][:4] if i else (None, None, None, None)
            base = pos - len(es[-1]) if i else pos
            for pad in range(40):
                prev = pc.entry(pty, payload(pty, pt, pkey, pv + pad)) if i else \
                    pc.entry(pc.LOGDIGEST, b"\0" * pad)
                start = base + len(prev) + 2 + 27   # 1 length byte: these payloads stay below 256
                if start % 16 == r:
                    break
            else:
                raise AssertionError("no pad found")
            if i:
                pos -= len(es[-1])
                es[-1] = prev
            else:
                es.append(prev)
                want.append(0)
            pos += len(prev)
        e = pc.entry(ty, payload(ty, t, key, v))
        es.append(e)
        want.append(h)
        pos += len(e)
    es.append(pc.entry(pc.OBJ, pc.obj(t33, key, key_len=len(key) + 1)))   # a byte past it: malformed
    want.append(0)
    return es, want


def test_hash(ctx, ramcrc, oracle_mod):
    cases = pc.load("key_hash_ref.json")["cases"]
    es, want = _hash_segment(cases)
    cap = 256 * KiB
    buf, certs = ac.source_of(oracle_mod, [es], cap)
    w = Walked(ctx, buf, certs, cap, 1)
    assert w.table.shape[0] == len(want) and w.status[0, 0] == OK
    seen = set()   # (key length, residue of the key's first byte) of the one-length-byte objects
    for _, off, ln, hdr in w.table.tolist():
        if hdr == pc.OBJ:
            seen.add((int(buf[off + 2 + 25]) | int(buf[off + 2 + 26]) << 8, (off + 2 + 27) % 16))
    assert {(n, r) for n in range(65) for r in range(16)} <= seen
    p = pc.check_device(ctx, ramcrc, w, pc.split_tablets(TABLE_IDS, 2, 3), 3, what="hash")
    assert p.hash_all[:len(want)].tolist() == want
    assert p.pstat[0, 0] == OK | MAL and p.pstat[0, 2] == 0


# ------------------------------------------------------------- 2. tablets
@pytest.fixture(scope="module")
def stored(ctx, oracle_mod):
    buf, certs = ac.source_of(oracle_mod, [pc.stored_entries()], 64 * KiB)
    return Walked(ctx, buf, certs, 64 * KiB, 1)


TAB_BASE, TAB_OVERLAP = pc.TAB_BASE, pc.TAB_OVERLAP
TAB_MANY = [(999, i, i, 0, 0, i % 7) for i in range(299)]   # with one more: past the LDS staging


@pytest.mark.parametrize("name,tabs", [
    ("none", []), ("one", TAB_BASE[:1]), ("base", TAB_BASE), ("overlap_ab", TAB_OVERLAP + TAB_BASE),
    ("overlap_ba", TAB_OVERLAP[::-1] + TAB_BASE), ("staged_256", TAB_MANY[:251] + TAB_BASE),
    ("global_300", TAB_MANY + TAB_OVERLAP[1:]), ("global_302", TAB_MANY[:150] + TAB_OVERLAP[::-1]
                                                  + TAB_MANY[150:] + TAB_BASE[4:])])
def test_tablets(ctx, ramcrc, stored, name, tabs):
    p = pc.check_device(ctx, ramcrc, stored, tabs, 7, what=name)
    got = dict(p.place[7:].tolist())
    if name == "base":
        assert got == pc.TAB_BASE_PLACED
    elif name in ("overlap_ab", "overlap_ba", "global_302"):
        assert got[3 + 4] == (5 if name == "overlap_ab" else 6) and got[3 + 8] == 5
    elif name == "global_300":
        assert got == {3 + 3: 6, 3 + 4: 6, 3 + 5: 6}


# ------------------------------------------------------------- 3. fan-out
@pytest.mark.parametrize("n_part", [1, 3, 64, 600])
def test_fan_out(ctx, ramcrc, oracle_mod, n_part):
    past = pc.entry(pc.TXPLIST, pc.tx_plist([(1, 5, 0)] * 3, count=4))   # its array passes the record
    es, tabs, body = pc.fan_out_case(n_part, extra=[past])
    buf, certs = ac.source_of(oracle_mod, [es], 64 * KiB)
    w = Walked(ctx, buf, certs, 64 * KiB, 1)
    p = pc.check_device(ctx, ramcrc, w, tabs, n_part, what=n_part)
    assert p.place[n_part:-n_part].tolist() == body
    assert p.place[-n_part:].tolist() == [[10, q] for q in range(n_part)]
    assert p.pstat.tolist() == [[OK | MAL, 2 * n_part + 74, 0, 0]]


# ------------------------------------------------------------ 4. position
def test_position(ctx, ramcrc, oracle_mod):
    cap = 64 * KiB
    ref = pc.load("recovery_build_ref.json")["is_entry_alive"]
    cid, coff = ref["ctime"]
    tabs = pc.tablets([(1, 0, ALL, 7, 0, 1), (2, 0, ALL, cid, coff, 0)])
    lists = pc.position_lists()
    alive = []
    for seg_id, off, ok in ref["cases"] + [[(1 << 32) + cid, 0, True]]:
        hdr = pc.entry(pc.SEGHEADER, pc.seg_header(seg_id))
        off = max(off, len(hdr) + 3)
        lists.append([hdr, pc.entry(pc.LOGDIGEST, b"\0" * (off - len(hdr) - 3)),
                      pc.entry(pc.OBJTOMB, pc.tomb(2, b"1"))])
        alive.append(ok)
    buf, certs = ac.source_of(oracle_mod, lists, cap)
    certs[1, 1] ^= 1
    w = Walked(ctx, buf, certs, cap, len(lists))
    p = pc.check_device(ctx, ramcrc, w, tabs, 2, what="position")
    assert p.pstat[:9].tolist() == pc.POSITION_STATUS
    assert p.pstat[9:].tolist() == [[OK, int(a), 0, int(not a)] for a in alive]


# ---------------------------------------------------------------- 5. scan
def _object_segments(nseg, cap, value_len=64):
    """nseg segments of a SEGHEADER and objects {table 1, 8-byte counter key}."""
    tmpl = np.frombuffer(pc.entry(pc.OBJ, pc.obj(1, b"\0" * 8, b"\x33" * value_len)), np.uint8)
    head = np.frombuffer(pc.entry(pc.SEGHEADER, pc.seg_header(4)), np.uint8)
    per = (cap - head.size) // tmpl.size
    buf = np.zeros(nseg * cap, np.uint8)
    for s in range(nseg):
        body = np.tile(tmpl, (per, 1))
        body[:, 2 + 27:2 + 35] = (np.arange(per, dtype=np.uint64) + s * per).view(np.uint8).reshape(per, 8)
        buf[s * cap:s * cap + head.size] = head
        buf[s * cap + head.size:s * cap + head.size + per * tmpl.size] = body.reshape(-1)
    return buf, per, head.size + per * tmpl.size


@pytest.fixture(scope="module")
def scan_case(ctx, oracle_mod):
    cap, nseg = 1 * MiB, 4
    buf, per, length = _object_segments(nseg, cap)
    _, ck, _, _ = oracle_mod.check_metadata(buf[:cap], length, 0, capacity=cap, table_cap=cap + 1)
    certs = np.array([(length, ck)] * nseg, np.uint32)
    w = Walked(ctx, buf, certs, cap, nseg, min_entry=64)
    tabs = pc.split_tablets([1], 64, 8)
    tabs["ctime_segment_id"][::5] = 5    # every fifth tablet was created later: its records are dead
    exp = pc.expected(buf, cap, w.table, w.status, tabs, 8)
    assert w.table.shape[0] == nseg * (per + 1) > 40000 and 0 < exp[0].shape[0] < nseg * per
    return w, tabs, exp


@pytest.mark.parametrize("ncu", [0, 1, 3])
def test_scan(ramcrc, oracle_mod, scan_case, ncu):
    """About 41,000 records (several scan tiles of 1,024) on a default context
    and on contexts sized for 1 and 3 CUs; place_cap equal to the need, and one
    less: the list stops at the capacity, the append refuses, and the context
    takes a valid call after it."""
    w, tabs, exp = scan_case
    need = exp[0].shape[0]
    c = ramcrc.Context(0)
    try:
        if ncu:
            c.set_cus(ncu)
        p = pc.check_device(c, ramcrc, w, tabs, 8, exp=exp, what=("exact", ncu))
        assert p.need == need and p.place.shape[0] == need
        short = pc.check_device(c, ramcrc, w, tabs, 8, place_cap=need - 1, exp=exp, what=("short", ncu))
        assert short.need == need and short.place.shape[0] == need - 1
        out_cap = 64 * KiB
        n_out = w.nseg * 8
        out = torch.full((n_out * out_cap,), ac.FILL, dtype=torch.uint8, device="cuda")
        o_certs = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
        o_stat = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
        c.recovery_append(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, short.d_place,
                          short.d_n_place, 8, out, out_cap, out_cap, o_certs, o_stat)
        with pytest.raises(ramcrc.RamcrcError) as e:
            c.check()
        assert e.value.code == ramcrc.EREFUSED
        assert (out == ac.FILL).all() and (o_certs == ac.PATTERN).all()
        pc.check_device(c, ramcrc, w, tabs, 8, exp=exp, what=("again", ncu))
    finally:
        c.close()


# --------------------------------------------------------------- 6. chain
def _chain(ctx, ramcrc, oracle, w, tabs, n_part, out_cap, what):
    """walk -> partition -> append on the device against the host chain."""
    e_place = pc.expected(w.buf, w.cap, w.table, w.status, tabs, n_part)[0]
    p = pc.Partitioned(ctx, w, tabs, n_part, e_place.shape[0] + 5, check=False)
    n_out = w.nseg * n_part
    out = torch.full((n_out * out_cap,), ac.FILL, dtype=torch.uint8, device="cuda")
    o_certs = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    o_stat = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    ctx.recovery_append(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, p.d_place, p.d_n_place,
                        n_part, out, out_cap, out_cap, o_certs, o_stat)
    ctx.check()
    p.read()
    h_place, _, _, h_pstat = ramcrc.recovery_partition_host(w.buf, w.cap, w.nseg, w.status, w.table,
                                                            tabs, n_part)
    assert np.array_equal(p.place, h_place) and np.array_equal(p.place, e_place), what
    assert np.array_equal(p.pstat, h_pstat), what
    h_out = np.full(n_out * out_cap, ac.FILL, np.uint8)
    h_certs, h_stat = ramcrc.recovery_append_host(w.buf, w.cap, w.nseg, w.status, w.table, h_place,
                                                  n_part, h_out, out_cap, out_cap)
    got = out.cpu().numpy()
    assert np.array_equal(got, h_out), (what, "bytes")
    assert np.array_equal(_u32(o_certs), h_certs) and np.array_equal(_u32(o_stat), h_stat), what
    exp = ac.expected(w.buf, w.cap, w.table, w.status, h_place, w.nseg, n_part, out_cap)
    ac.check_outputs(oracle, exp, got, out_cap, out_cap, _u32(o_certs), _u32(o_stat), what)
    return got, _u32(o_certs), p


def test_chain_build_fixture(ctx, ramcrc, oracle_mod):
    """The three RecoverySegmentBuilderTest scenarios, one source segment
    each: every output's (type, offset, length) sequence is the fixture's."""
    ref = pc.load("recovery_build_ref.json")
    cap = 64 * KiB
    tabs = pc.tablets(ref["tablets"])
    for sc in ref["scenarios"]:
        es = [pc.entry(t, bytes.fromhex(b)) for t, b in sc["entries"]]
        buf, certs = ac.source_of(oracle_mod, [es], cap)
        w = Walked(ctx, buf, certs, cap, 1)
        got, o_certs, _ = _chain(ctx, ramcrc, oracle_mod, w, tabs, sc["n_part"], cap, sc["name"])
        for q in range(sc["n_part"]):
            assert pc.walk_records(got[q * cap:(q + 1) * cap], int(o_certs[q, 0])) == sc["outputs"][q]


def test_chain_mixed(ctx, ramcrc, oracle_mod):
    """Mixed segments over three tables into 8 partitions; one source segment
    with a damaged certificate contributes nothing."""
    cap, nseg = 64 * KiB, 6
    buf, certs = ac.source_of(oracle_mod, pc.mixed_lists(nseg, 48 * KiB, 81), cap)
    certs[3, 1] ^= 1
    w = Walked(ctx, buf, certs, cap, nseg)
    tabs = pc.split_tablets([1, 2], 5, 8, ctime=(12, 100))
    _, _, p = _chain(ctx, ramcrc, oracle_mod, w, tabs, 8, cap, "mixed")
    assert p.pstat[3].tolist() == [BAD, 0, 0, 0]
    assert (p.pstat[[0, 1, 2, 4, 5], 0] == OK).all() and p.pstat[:, 1].sum() == p.need > 100
    assert p.pstat[:2, 3].sum() > 0 and p.pstat[:, 2].sum() > 0   # dead (segments 10, 11) and unplaced (table 3)


# --------------------------------------------------------------- 7. state
def test_state(ramcrc, oracle_mod):
    """One context through many small segments, few large ones, the small ones
    again, then another tablet list: nothing of an earlier call shows."""
    c = ramcrc.Context(0)
    try:
        a_buf, a_certs = ac.source_of(oracle_mod, pc.mixed_lists(24, 12 * KiB, 91), 16 * KiB)
        b_buf, b_certs = ac.source_of(oracle_mod, pc.mixed_lists(2, 200 * KiB, 92), 256 * KiB)
        wa = Walked(c, a_buf, a_certs, 16 * KiB, 24)
        wb = Walked(c, b_buf, b_certs, 256 * KiB, 2)
        t1 = pc.split_tablets([1, 2, 3], 4, 5, ctime=(11, 0))
        t2 = pc.split_tablets([3, 1], 300, 2)
        pa = pc.check_device(c, ramcrc, wa, t1, 5, what="A")
        pc.check_device(c, ramcrc, wb, t1, 5, what="B")
        pa2 = pc.check_device(c, ramcrc, wa, t1, 5, what="A again")
        assert np.array_equal(pa.place, pa2.place)
        pc.check_device(c, ramcrc, wa, t2, 2, what="other tablets")
        pc.check_device(c, ramcrc, wb, t2, 2, what="B, other tablets")
    finally:
        c.close()


@pytest.mark.parametrize("variant", ["partition_at_n_part", "n_part_zero", "segment_at_n_seg",
                                     "second_run"])
def test_refusals(ctx, ramcrc, oracle_mod, variant):
    """The device form refuses what the host form returns EINVAL for: only
    *d_n_place (0) is written, check() raises EREFUSED, and the context takes a
    valid call after it."""
    cap = 64 * KiB
    lists = [pc.head_entries() + [pc.entry(pc.OBJTOMB, pc.tomb(1, b"k"))] for _ in range(2)]
    buf, certs = ac.source_of(oracle_mod, lists, cap)
    w = Walked(ctx, buf, certs, cap, 2)
    good = [(1, 0, ALL, 0, 0, 1)]
    tabs, n_part = good, 2
    saved = w.d_entries[:8].clone()
    if variant == "partition_at_n_part":
        tabs = good + [(5, 0, 0, 0, 0, 2)]
    elif variant == "n_part_zero":
        n_part, tabs = 0, []
    elif variant == "segment_at_n_seg":
        w.d_entries[7, 0] = 2
    else:
        first = int(w.table[0, 0])
        w.d_entries[7, 0] = first   # the other segment's last record
    p = pc.Partitioned(ctx, w, tabs, n_part, 16, check=False)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ctx.check()
    assert e.value.code == ramcrc.EREFUSED
    p.read()
    assert p.need == 0 and (p.place_all == 0xA5A5A5A5).all() and (p.pstat == 0xA5A5A5A5).all()
    w.d_entries[:8] = saved
    pc.check_device(ctx, ramcrc, w, good, 2, what="after the refusal")
