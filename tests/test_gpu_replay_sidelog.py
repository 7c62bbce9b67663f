"""ramcrc_replay_sidelog_device: the append at one partition made a side log
on the GPU -- kept tombstones rewritten (segmentId 0, the call's timestamp, a
checksum recomputed from the bytes), a reference per placement, counters
(ObjectManager::replaySegment, src/ObjectManager.cc:720-734, :840-867).

The record tables come from ctx.segment_walk on the device; the expectation
from sidelog_cases (the plain-Python append, its tombstones patched in Python
with the oracle's CRC32C; the outputs walked and verified by the oracle).
Every output is pre-filled with 0xA5, so a write at or past a head, past a
list's end or by a refused call shows.  Every case also runs the host form and
the plain append on the device and compares the bytes."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import replay_table_cases as tc
import sidelog_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cases(ctx, ramcrc, oracle_mod, name):
    """The host tests' cases, with their remarks on what each must contain."""
    case = sc.CASES[name](oracle_mod)
    w = sc.walked(ctx, oracle_mod, case)
    r, exp = sc.check_device(ctx, ramcrc, oracle_mod, w, case)
    c = exp["counts"]
    if name == "key_lengths":
        lens = set(w.table[(w.table[:, 3] & 0x3F) == sc.OBJTOMB, 2].tolist())
        assert {255, 256, 65535, 65536} <= lens and c["tombstones"] == len(sc.KEY_LENGTHS)
    elif name == "alignment":
        assert w.d.data_ptr() % 16 == 0 and r.d_out.data_ptr() % 16 == case.lead
        live = case.live_of(w.table)
        assert len(sc.alignment_pairs(case, w.table, live, r.refs, r.d_out.data_ptr())) == 256
    elif name == "special":
        assert (c["tombstones"], c["short_tombstones"], c["objects"]) == (3, 1, 2)
    elif name == "capacity_last_fits":
        assert r.ostat.tolist() == [[segments.SEG_APPEND_FULL, 4]] and c["left_out"] == 2
        assert r.certs[0, 0] == case.out_capacity
    elif name == "capacity_first_left_out":
        assert r.ostat.tolist() == [[segments.SEG_APPEND_FULL, 3]] and c["left_out"] == 3
        assert r.refs[3:].tolist() == [[sc.NONE] * 2] * 3
    elif name == "bad_source":
        assert r.ostat[1].tolist() == [segments.SEG_SOURCE_BAD, 0] and c["left_out"] > 0
    elif name == "empty_list":
        assert c == dict.fromkeys(sc.COUNT_NAMES, 0)


def test_without_refs_and_without_segments(ctx, ramcrc, oracle_mod):
    """d_refs = NULL; n_seg = 0 returns at once and writes nothing."""
    case = sc.mixed(oracle_mod)
    w = sc.walked(ctx, oracle_mod, case)
    sc.check_device(ctx, ramcrc, oracle_mod, w, case, want_refs=False, plain=False)
    live = case.live_of(w.table)
    r = sc.SideLog(ctx, w, live, case.out_capacity, case.out_stride)
    pat = lambda n: torch.full((n, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    certs, stat, counts = pat(1), pat(1), torch.full((7,), 5, dtype=torch.int64, device="cuda")
    ctx.replay_sidelog(w.d, w.cap, 0, w.d_status, w.d_entries, w.d_n, r.d_live, r.d_n, sc.TS, r.d_out,
                       case.out_stride, case.out_capacity, certs, stat, counts)
    ctx.check()
    assert (ac._u32(certs) == ac.PATTERN).all() and (counts.cpu().numpy() == 5).all()


@pytest.mark.parametrize("variant", sc.REFUSALS + ["n_live_over_cap"])
def test_refusals(ctx, ramcrc, oracle_mod, variant):
    """Every refusal of the append and a partition that is not 0:
    RAMCRC_EREFUSED from check(), none of d_out, d_out_certs, d_out_status,
    d_refs, d_counts written, and a following valid call is correct."""
    case = sc.mixed(oracle_mod, seed=39, nseg=2, n=40)
    w = sc.walked(ctx, oracle_mod, case)
    good = case.live_of(w.table)
    kw = {}
    if variant == "n_live_over_cap":
        bad, bad_table = good, w.table
        kw = dict(live_cap=good.shape[0] - 1, n_live=good.shape[0])
    else:
        bad, bad_table = sc.refusal(variant, w.table, good, 2)
    changed = np.flatnonzero((bad_table != w.table).any(axis=1))
    for rec in changed:
        w.d_entries[int(rec)] = torch.from_numpy(bad_table[rec].view(np.int32)).cuda()
    r = sc.SideLog(ctx, w, bad, case.out_capacity, case.out_stride, **kw)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ctx.check()
    assert e.value.code == ramcrc.EREFUSED
    assert r.untouched()
    ctx.check()   # the refusal was taken
    for rec in changed:
        w.d_entries[int(rec)] = torch.from_numpy(w.table[rec].view(np.int32)).cuda()
    sc.check_device(ctx, ramcrc, oracle_mod, w, case, live=good)


def test_argument_checks(ctx, ramcrc, oracle_mod):
    case = sc.special(oracle_mod)
    w = sc.walked(ctx, oracle_mod, case)
    live = case.live_of(w.table)
    with pytest.raises(ramcrc.RamcrcError) as e:   # out_stride < out_capacity
        sc.SideLog(ctx, w, live, 4096, 4080)
    assert e.value.code == ramcrc.EINVAL
    r = sc.SideLog(ctx, w, live, case.out_capacity, case.out_stride)
    ctx.check()
    args = (w.d, w.cap, 1, w.d_status, w.d_entries, w.d_n, r.d_live, r.d_n, sc.TS)
    with pytest.raises(ramcrc.RamcrcError) as e:   # no counts
        ctx.replay_sidelog(*args, r.d_out, case.out_stride, case.out_capacity, r.d_certs, r.d_stat, None)
    assert e.value.code == ramcrc.EINVAL
    with pytest.raises(ramcrc.RamcrcError) as e:   # the outputs inside the source
        ctx.replay_sidelog(*args, w.d[w.cap // 2:], w.cap // 2, 1024, r.d_certs, r.d_stat, r.d_counts)
    assert e.value.code == ramcrc.EINVAL
    ctx.check()


@pytest.fixture(scope="module")
def small_grid(oracle_mod):
    """The source and, once, the expectation: of one replica, repeated."""
    nseg = 10
    buf, certs, cap = sc.small_grid_source(oracle_mod, nseg)
    status, table = ac.host_walk(oracle_mod, buf[:cap], certs[:1], 1, cap)
    live = np.array([(r, 0) for r in range(table.shape[0]) if r % 7], np.uint32)
    out_capacity = cap // 2   # the outputs fill up
    one = sc.expected(oracle_mod, buf[:cap], cap, table, status, live, 1, out_capacity)
    return buf, certs, cap, nseg, live, out_capacity, one


def test_small_grids(ramcrc, small_grid):
    """1- and 3-CU grids over about 250,000 short tombstones and objects, so
    that every grid-stride loop wraps many times, between two default-grid
    calls on the same context: four identical results, the expected ones."""
    buf, certs, cap, nseg, live1, out_capacity, one = small_grid
    ctx = ramcrc.Context(0)
    w = ac.Walked(ctx, buf, certs, cap, nseg, min_entry=34)
    n1 = w.table.shape[0] // nseg
    assert w.table.shape[0] > 240000 and (w.table[:n1, 0] == w.table[0, 0]).all()
    # the walk fixes no order across segments: the list follows the table's runs
    live = np.concatenate([live1 + (k * n1, 0) for k in range(nseg)]).astype(np.uint32)
    e_out = np.full(out_capacity, sc.FILL, np.uint8)
    e_out[:len(one["outs"][0])] = np.frombuffer(bytes(one["outs"][0]), np.uint8)
    assert one["flags"][0] == segments.SEG_APPEND_FULL and one["counts"]["left_out"] > 1000
    results = []
    for ncu in (0, 1, 3, 0):
        ctx.set_cus(ncu)
        r = sc.SideLog(ctx, w, live, out_capacity, out_capacity)
        ctx.check()
        r.read()
        assert sc.counts_dict(r.counts) == {k: v * nseg for k, v in one["counts"].items()}, ncu
        out = r.out.reshape(nseg, out_capacity)
        refs = r.refs.reshape(nseg, -1, 2)
        for k in range(nseg):
            seg = int(w.table[k * n1, 0])
            assert np.array_equal(out[seg], e_out), (ncu, seg)
            e_refs = one["refs"].copy()
            e_refs[e_refs[:, 0] != sc.NONE, 0] = seg
            assert np.array_equal(refs[k], e_refs), (ncu, k)
        assert (r.ostat == [segments.SEG_APPEND_FULL, one["entries"][0]]).all()
        assert (r.certs[:, 0] == len(one["outs"][0])).all() and len(set(r.certs[:, 1].tolist())) == 1
        results.append((r.out, r.certs, r.refs))
    ctx.close()
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))


def test_chain_on_one_context(ctx, ramcrc, oracle_mod):
    """replay verify -> two replay-table adds -> live queries -> a side log
    per batch -> walk and verify of the outputs, all on one context.  The
    survivors read back from the outputs through d_refs are the replay's."""
    cap = 64 * sc.KiB
    lists = sc.chain_lists(oracle_mod)
    ws = []
    for ls in lists:
        buf, certs = ac.source_of(oracle_mod, ls, cap)
        w = ac.Walked(ctx, buf, certs, cap, len(ls))
        d_certs = torch.from_numpy(certs.view(np.int32)).cuda()
        crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
        ctx.replay_verify(w.d, cap, cap, w.nseg, d_certs, w.d_status, w.d_entries, w.d_n, crc)
        ctx.check()
        w.status = ac._u32(w.d_status)
        w.table = np.ascontiguousarray(ac._u32(w.d_entries[:int(w.d_n.item())]))
        assert (w.status[:, 0] == segments.SEG_OK).all() and (w.status[:, 3] == 0).all()
        ws.append(w)
    t = ramcrc.ReplayTable(ctx, 4096, 4)
    added = [tc.Added(w) for w in ws]
    for a in added:
        a.add(t)
    lives = [tc.Live(ctx, t, a) for a in added]
    got = {}
    for w, lv in zip(ws, lives):
        case = sc.Case([], cap, lv.live)
        r, exp = sc.check_device(ctx, ramcrc, oracle_mod, w, case, what="chain")
        assert exp["counts"]["left_out"] == 0
        # the outputs pass the device's own walk and replay checks
        n_out = w.nseg
        st = torch.zeros((n_out, 4), dtype=torch.int32, device="cuda")
        ent = torch.zeros((n_out * (cap // 2 + 1), 4), dtype=torch.int32, device="cuda")
        n = torch.zeros(1, dtype=torch.int64, device="cuda")
        crc = torch.zeros(ent.shape[0], dtype=torch.int32, device="cuda")
        ctx.replay_verify(r.d_out, case.out_stride, cap, n_out, r.d_certs, st, ent, n, crc)
        ctx.check()
        st = ac._u32(st)
        assert (st[:, 0] == segments.SEG_OK).all() and (st[:, 3] == 0).all()
        assert int(n.item()) == lv.live.shape[0]
        part = sc.read_survivors(r.out, case.out_stride, r.refs)
        assert not set(part) & set(got)
        got.update(part)
    t.close()
    assert got == tc.survivors(ws, [lv.live for lv in lives]) == tc.replayed(ws)


def test_repeated_calls(ctx, ramcrc, oracle_mod):
    """Two calls of different shapes, then the first shape again, on one
    context, each against its own expectation."""
    a, b = sc.mixed(oracle_mod), sc.key_lengths(oracle_mod)
    wa, wb = sc.walked(ctx, oracle_mod, a), sc.walked(ctx, oracle_mod, b)
    ra, exp = sc.check_device(ctx, ramcrc, oracle_mod, wa, a, what="A")
    sc.check_device(ctx, ramcrc, oracle_mod, wb, b, what="B")
    again, _ = sc.check_device(ctx, ramcrc, oracle_mod, wa, a, exp=exp, what="A again")
    assert np.array_equal(ra.out, again.out)
