"""ramcrc_replay_resolve_device: which replayed objects and tombstones a
recovery master keeps (ObjectManager::replaySegment, src/ObjectManager.cc:
632-867), for every walked record on the GPU.

The record table comes from ctx.segment_walk on the device.  The winners, the
live list and the counters must equal the host form's and
resolve_cases.expected's (a plain-Python sequential replay) exactly; the
reference's own test cases come from tests/golden/replay_resolve_ref.json.
Every output is pre-filled with 0xA5, so a write past the list's end shows."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc
import resolve_cases as rc
from append_cases import Walked, _u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


def _walked(ctx, oracle, lists, cap, bad=()):
    buf, certs = ac.source_of(oracle, lists, cap)
    for s in bad:
        certs[s, 1] ^= 1
    return Walked(ctx, buf, certs, cap, len(lists))


@pytest.fixture(scope="module")
def mixed(ctx, oracle_mod):
    """(walked, expectation): computed once, shared, left unchanged."""
    w = _walked(ctx, oracle_mod, rc.mixed_lists(), rc.MIXED_CAP, bad=[rc.MIXED_BAD])
    return w, rc.expected(w.buf, w.cap, w.table, w.status)


@pytest.fixture(scope="module")
def hot(ctx, oracle_mod):
    w = _walked(ctx, oracle_mod, [rc.hot_key_entries()], 1 * MiB)
    return w, rc.expected(w.buf, w.cap, w.table, w.status)


# ------------------------------------------------- 1. reference scenarios
def test_reference_scenarios(ctx, ramcrc, oracle_mod):
    ref = pc.load("replay_resolve_ref.json")
    es, first = rc.reference_case(ref)
    w = _walked(ctx, oracle_mod, [es], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, what="reference")
    for c, at in zip(ref["cases"], first):
        n, sv = len(c["records"]), c["survivor"]
        assert r.winner_all[at:at + n].tolist() == [at + sv["index"]] * n, c["name"]
        assert int(w.table[at + sv["index"], 3]) & 0x3F == (rc.OBJ if sv["type"] == "OBJ" else rc.OBJTOMB)
    assert r.need == len(ref["cases"])


# ---------------------------------------------------------------- 2. mixed
def test_mixed(ctx, ramcrc, mixed):
    w, exp = mixed
    assert w.status[rc.MIXED_BAD, 0] & segments.SEG_OK == 0
    assert rc.key_residues(w.buf, w.cap, w.table, w.status) == set(range(16))
    r = rc.check_device(ctx, ramcrc, w, exp=exp, what="mixed")
    assert r.counts["safe_version"] == 1 << 40 and r.counts["malformed"] >= 1
    assert r.counts["live_objects"] > 20 and r.counts["live_tombstones"] > 20
    # without d_winner the list and the counters are the same
    q = rc.Resolved(ctx, w, want_winner=False)
    assert q.need == r.need and np.array_equal(q.live, r.live) and q.counts == r.counts


# ----------------------------------------------------------- 3. collisions
def test_collisions_with_equal_hashes(ctx, ramcrc, oracle_mod):
    """(a) Every caller hash is 7: one probe chain holds all 50 keys, so every
    record meets keys that differ from its own only in the last byte, only in
    length (a prefix, the empty key) or only in table id."""
    w = _walked(ctx, oracle_mod, [rc.collision_entries()], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, hashes=np.full(w.table.shape[0], 7, np.uint64), what="hash 7")
    assert r.counts["objects"] + r.counts["tombstones"] == 300 and r.need == 50


def test_collisions_of_the_seed(ctx, ramcrc, oracle_mod):
    """(b) NULL hashes, table ids 1 and 2^32 + 1 with the same key bytes: the
    computed hashes are equal, the keys stay two."""
    w = _walked(ctx, oracle_mod, [rc.seed_collision_entries()], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, what="seed")
    assert r.live[:, 0].tolist() == [2, 4, 6, 8, 10, 12]


def test_caller_hashes_split_keys(ctx, ramcrc, oracle_mod):
    w = _walked(ctx, oracle_mod, [rc.tiny_entries()], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, hashes=np.array([1, 2, 3], np.uint64), what="split")
    assert r.winner_all[:3].tolist() == [0, 1, 2]


# ---------------------------------------------------------- 4. hash source
def test_hash_source(ctx, ramcrc, oracle_mod, mixed):
    """The partition call's d_key_hash (one tablet per table covering
    everything) and NULL give identical outputs.  The hashes computed inside
    the call are no output; they come from the device function the partition
    call writes d_key_hash with, which is compared with key_hash_ref.json here
    for an object and a tombstone of every fixture key below 64 KiB, and the
    resolve of those records must agree with and without them."""
    w, exp = mixed
    tabs = pc.tablets([(t, 0, ALL, 0, 0, 0) for t in (1, 2, (1 << 32) + 1)])
    p = pc.Partitioned(ctx, w, tabs, 1, w.table.shape[0] + 8)
    given = rc.Resolved(ctx, w, hashes=p.d_hash)
    null = rc.Resolved(ctx, w)
    n = w.table.shape[0]
    assert np.array_equal(given.winner_all, null.winner_all) and np.array_equal(null.winner_all[:n], exp[0])
    assert np.array_equal(given.live_all, null.live_all) and given.need == null.need == exp[1].shape[0]
    assert given.counts == null.counts == exp[2]

    cases = [(t, bytes.fromhex(k), h) for t, k, h in pc.load("key_hash_ref.json")["cases"]
             if len(k) // 2 < 60000]
    es = [pc.entry(pc.SEGHEADER, pc.seg_header(1))]
    for t, key, _ in cases:
        es += [rc.obj(t, key, 1), rc.tomb(t, key, 2)]
    wf = _walked(ctx, oracle_mod, [es], 2 * MiB)
    tabs = pc.tablets([(t, 0, ALL, 0, 0, 0) for t in sorted({t for t, _, _ in cases})])
    pf = pc.Partitioned(ctx, wf, tabs, 1, 8)
    want = [0] + [h for _, _, h in cases for _ in range(2)]
    assert pf.hash_all[:len(want)].tolist() == want
    e = rc.expected(wf.buf, wf.cap, wf.table, wf.status)
    a = rc.check_device(ctx, ramcrc, wf, exp=e, what="fixture keys, computed")
    b = rc.Resolved(ctx, wf, hashes=pf.d_hash)
    assert np.array_equal(a.winner_all, b.winner_all) and np.array_equal(a.live_all, b.live_all)
    # every key keeps its tombstone (equal keys of the fixture keep the first)
    assert (wf.table[a.live[:, 0], 3] & 0x3F == rc.OBJTOMB).all()


# ------------------------------------------------------ 5. 64-bit versions
def test_wide_versions(ctx, ramcrc, oracle_mod):
    """Versions from {0, 2^32 - 1, 2^32, 2^63, 2^64 - 1}: a truncated or a
    signed compare fails."""
    w = _walked(ctx, oracle_mod, [rc.wide_version_entries()], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, what="wide")
    n = 0
    for a in rc.WIDE:
        for b in rc.WIDE:
            at = 1 + 4 * n
            assert r.winner_all[at] == r.winner_all[at + 1] == (at + 1 if b > a else at), (a, b)
            assert r.winner_all[at + 2] == r.winner_all[at + 3] == (at + 3 if b > a else at + 2), (a, b)
            n += 1


# ---------------------------------------------------------- 6. one hot key
def test_one_hot_key(ctx, ramcrc, oracle_mod, hot):
    w, exp = hot
    r = rc.check_device(ctx, ramcrc, w, exp=exp, what="hot")
    assert w.table.shape[0] == 20000 and (r.winner_all[:20000] == 19990).all()
    assert r.live.tolist() == [[19990, 0]] and r.counts["live_tombstones"] == 1
    w2 = _walked(ctx, oracle_mod, [rc.hot_key_entries(tombstones=False)], 1 * MiB)
    r2 = rc.check_device(ctx, ramcrc, w2, what="hot objects")
    assert (r2.winner_all[:20000] == 0).all() and r2.live.tolist() == [[0, 0]]


# ---------------------------------------------------------- 7. small grids
@pytest.fixture(scope="module")
def grid_case(ctx):
    cap, nseg = 8 * MiB, 3
    buf, certs, counts = segments.object_segments_host(2, cap, 64)
    buf = np.concatenate([buf, buf[:cap]])
    certs = np.concatenate([certs, certs[:1]])
    w = Walked(ctx, buf, certs, cap, nseg, min_entry=64)
    per = int(counts[0])
    assert per == counts[1] > 80000 and w.table.shape[0] == 3 * per and (w.status[:, 0] == 1).all()
    # the analytic answer: the walk keeps a segment's records together and in
    # offset order, so record k of segment 2 and record k of segment 0 are
    # twins, and the one whose run comes first in the table wins (segment 0's)
    seg = w.table[:, 0]
    first = {s: int(np.flatnonzero(seg == s)[0]) for s in range(3)}
    lo, hi = sorted((0, 2), key=first.get)
    winner = np.arange(3 * per, dtype=np.uint32)
    winner[first[hi]:first[hi] + per] = np.arange(first[lo], first[lo] + per, dtype=np.uint32)
    live = np.flatnonzero(seg != hi).astype(np.uint32)
    e_counts = dict(objects=3 * per, tombstones=0, live_objects=2 * per, live_tombstones=0,
                    malformed=0, safe_version=0)
    return w, (winner, np.stack([live, np.zeros_like(live)], 1), e_counts)


@pytest.mark.parametrize("ncu", [0, 1, 3])
def test_small_grids(ramcrc, grid_case, ncu):
    """Two 8 MiB segments of 64-byte objects (83,055 records each, all keys
    distinct) and a byte copy of the first: every record of segments 0 and 1
    is live, every record of segment 2 has its twin of segment 0 as winner.

    249,165 records, so the table has 524,288 slots and there are 244 tiles of
    1,024.  Grids are capped at 8 workgroups of 256 threads per CU.  At 1 CU
    that is 8 workgroups, 2,048 threads: k_res_zero loops 768 times over the
    slots' 1,572,864 words, k_res_insert and k_res_pick 122 times over the
    records, and k_res_tiles and k_res_emit take 31 tiles per workgroup.  At 3
    CUs, 24
    workgroups and 6,144 threads: 256 and 41 passes, and 11 tiles per
    workgroup.  k_res_scan is one workgroup by design (244 tiles in one step
    of 256).  At the default size (256 CUs, 2,048 workgroups) only k_res_zero
    still wraps; 974 workgroups cover the records."""
    w, exp = grid_case
    c = ramcrc.Context(0)
    try:
        if ncu:
            c.set_cus(ncu)
        r = rc.check_device(c, ramcrc, w, exp=exp, what=("grids", ncu), host=(ncu == 0))
        assert r.need == exp[1].shape[0]
    finally:
        c.close()


# -------------------------------------------------------- 8. list capacity
def _append(c, w, r, out_cap):
    n_out = w.nseg
    out = torch.full((n_out * out_cap,), ac.FILL, dtype=torch.uint8, device="cuda")
    o_certs = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    o_stat = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    c.recovery_append(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, r.d_live[:r.live_cap],
                      r.d_n_live, 1, out, out_cap, out_cap, o_certs, o_stat)
    return out, o_certs, o_stat


def test_list_capacity(ramcrc, mixed):
    """live_cap one less than needed, then 0: the needed count is reported,
    nothing is written past the cap, and the append that follows refuses."""
    w, exp = mixed
    need = exp[1].shape[0]
    c = ramcrc.Context(0)
    try:
        for cap in (need - 1, 0):
            r = rc.check_device(c, ramcrc, w, live_cap=cap, exp=exp, what=("cap", cap))
            assert r.need == need and r.live.shape[0] == cap
            out, o_certs, _ = _append(c, w, r, w.cap)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            assert (out == ac.FILL).all() and (o_certs == ac.PATTERN).all()
        rc.check_device(c, ramcrc, w, exp=exp, what="after the refused appends")
    finally:
        c.close()


# -------------------------------------------------------------- 9. refusal
def test_refusal(ctx, ramcrc, oracle_mod):
    """A record with segment = n_seg: EREFUSED, *d_n_live = 0 and zeroed counts
    are the only outputs; a valid call on the same context follows."""
    lists = [[pc.entry(pc.SEGHEADER, pc.seg_header(s))] + rc.tiny_entries() for s in range(2)]
    w = _walked(ctx, oracle_mod, lists, 64 * KiB)
    saved = w.d_entries[:8].clone()
    w.d_entries[6, 0] = 2
    r = rc.Resolved(ctx, w, check=False)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ctx.check()
    assert e.value.code == ramcrc.EREFUSED
    r.read()
    assert r.need == 0 and not any(r.counts.values())
    assert (r.live_all == 0xA5A5A5A5).all() and (r.winner_all == 0xA5A5A5A5).all()
    w.d_entries[:8] = saved
    rc.check_device(ctx, ramcrc, w, what="after the refusal")


# ---------------------------------------- 10. one context, changing shapes
def test_state(ramcrc, oracle_mod, mixed, hot):
    """The mixed case, the hot key, a table of 3 records, the mixed case
    again, on one context: a table not cleared between calls fails here."""
    c = ramcrc.Context(0)
    try:
        wm, em = mixed
        wh, eh = hot
        a = rc.check_device(c, ramcrc, wm, exp=em, what="mixed")
        rc.check_device(c, ramcrc, wh, exp=eh, what="hot", host=False)
        wt = _walked(c, oracle_mod, [rc.tiny_entries()], 64 * KiB)
        t = rc.check_device(c, ramcrc, wt, what="tiny")
        assert t.winner_all[:3].tolist() == [1, 1, 2]
        b = rc.check_device(c, ramcrc, wm, exp=em, what="mixed again")
        assert np.array_equal(a.winner_all, b.winner_all) and np.array_equal(a.live, b.live)
    finally:
        c.close()


# --------------------------------------------------------------- 11. chain
def test_chain(ctx, ramcrc, oracle_mod, mixed):
    """Walk -> verify -> resolve -> append with n_part = 1: every output
    passes a walk with RAMCRC_SEG_OK, holds exactly the live records of its
    source segment in offset order, and equals ramcrc_recovery_append_host
    over the host form's list byte for byte."""
    w, exp = mixed
    crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
    st = w.d_status.clone()
    ctx.verify_objects(w.d, w.cap, w.d_entries, w.d_n, crc, st)
    r = rc.Resolved(ctx, w, check=False)
    out, o_certs, o_stat = _append(ctx, w, r, w.cap)
    ctx.check()
    r.read()
    assert np.array_equal(r.live, exp[1])
    h_winner, h_live, _, _ = ramcrc.replay_resolve_host(w.buf, w.cap, w.nseg, w.status, w.table)
    h_out = np.full(w.nseg * w.cap, ac.FILL, np.uint8)
    h_certs, h_stat = ramcrc.recovery_append_host(w.buf, w.cap, w.nseg, w.status, w.table, h_live, 1,
                                                  h_out, w.cap, w.cap)
    got = out.cpu().numpy()
    assert np.array_equal(got, h_out), "bytes"
    assert np.array_equal(_u32(o_certs), h_certs) and np.array_equal(_u32(o_stat), h_stat)
    e = ac.expected(w.buf, w.cap, w.table, w.status, h_live, w.nseg, 1, w.cap)
    ac.check_outputs(oracle_mod, e, got, w.cap, w.cap, _u32(o_certs), _u32(o_stat), "chain")
    # the outputs on the device pass the device walk too, and hold the live records
    ok = [s for s in range(w.nseg) if s != rc.MIXED_BAD]
    w2 = Walked(ctx, got, _u32(o_certs), w.cap, w.nseg, d_buf=out)
    assert (w2.status[ok, 0] == segments.SEG_OK).all()
    for s in ok:
        src = w.table[r.live[:, 0]]
        src = src[src[:, 0] == s]
        dst = w2.table[w2.table[:, 0] == s]
        assert dst.shape[0] == src.shape[0] == _u32(o_stat)[s, 1] > 0
        assert np.array_equal(dst[:, 2], src[:, 2]) and (np.diff(src[:, 1].astype(np.int64)) > 0).all()
        assert np.array_equal(dst[:, 3] & 0x3F, src[:, 3] & 0x3F)


# -------------------------------------------------------- 12. empty inputs
def test_empty_inputs(ctx, ramcrc, oracle_mod):
    w = _walked(ctx, oracle_mod, [[pc.entry(pc.SEGHEADER, pc.seg_header(1)),
                                   pc.entry(pc.LOGDIGEST, b"d")]], 64 * KiB)
    r = rc.check_device(ctx, ramcrc, w, what="no participants")
    assert r.need == 0 and not any(r.counts.values()) and (r.winner_all[:2] == rc.NONE).all()
    w.d_n.zero_()
    w.table = w.table[:0]
    r = rc.check_device(ctx, ramcrc, w, what="no records")
    assert r.need == 0 and not any(r.counts.values()) and (r.winner_all == 0xA5A5A5A5).all()
