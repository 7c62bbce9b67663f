"""ramcrc_replay_sidelog_host: what ObjectManager::replaySegment hands to
sideLog->append for every record it keeps (src/ObjectManager.cc:720-734,
:840-867), on the host.  The record tables come from the oracle's
checkMetadataIntegrity restatement; the expectation from sidelog_cases (the
plain-Python append, its tombstones patched in Python with the oracle's
CRC32C).  Every output region, and the bytes before the first, are pre-filled
with 0xA5, so a write at or past a head shows."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import replay_table_cases as tc
import sidelog_cases as sc


def test_dtypes_match_the_abi():
    assert segments.LOG_REF_DTYPE.itemsize == 8 and segments.SIDELOG_COUNTS_DTYPE.itemsize == 56
    assert segments.SIDELOG_COUNTS_DTYPE.names == (
        "objects", "tombstones", "other", "object_bytes", "tombstone_bytes", "short_tombstones",
        "left_out")
    assert segments.LOG_REF_NONE == 0xFFFFFFFF


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cases(ramcrc, oracle_mod, name):
    case = sc.CASES[name](oracle_mod)
    r = sc.run_host(ramcrc, oracle_mod, case)
    c, table, live = r["counts"], r["table"], r["live"]
    if name == "key_lengths":
        lens = set(table[(table[:, 3] & 0x3F) == sc.OBJTOMB, 2].tolist())
        assert lens == {32 + k for k in sc.KEY_LENGTHS} and {255, 256, 65535, 65536} <= lens
        assert c["tombstones"] == len(sc.KEY_LENGTHS) and c["left_out"] == 0
    elif name == "alignment":
        assert len(sc.alignment_pairs(case, table, live, r["refs"], r["base"])) == 256
    elif name == "mixed":
        assert min(c["objects"], c["tombstones"], c["other"]) > 10 and live.shape[0] < table.shape[0]
    elif name == "special":
        assert (c["tombstones"], c["short_tombstones"], c["objects"]) == (3, 1, 2)
        # the idempotent one: the bytes it had
        rec = 2
        src = int(table[rec, 1]) + 2
        dst = int(r["refs"][rec, 1]) + 2
        buf = sc.host_source(oracle_mod, case)[0]
        assert np.array_equal(r["out"][dst:dst + 36], buf[src:src + 36])
    elif name == "capacity_last_fits":
        assert r["ostat"].tolist() == [[segments.SEG_APPEND_FULL, 4]] and c["left_out"] == 2
        assert r["certs"][0, 0] == case.out_capacity and r["refs"][4:].tolist() == [[sc.NONE] * 2] * 2
    elif name == "capacity_first_left_out":
        assert r["ostat"].tolist() == [[segments.SEG_APPEND_FULL, 3]] and c["left_out"] == 3
        assert (c["tombstones"], c["objects"]) == (1, 2)
        assert r["refs"][3:].tolist() == [[sc.NONE] * 2] * 3
    elif name == "bad_source":
        assert r["ostat"][1].tolist() == [segments.SEG_SOURCE_BAD, 0]
        mine = table[live[:, 0], 0] == 1
        assert mine.any() and (r["refs"][mine] == sc.NONE).all() and (r["refs"][~mine] != sc.NONE).all()
        assert c["left_out"] == int(mine.sum())
    elif name == "empty_list":
        assert c == dict.fromkeys(sc.COUNT_NAMES, 0) and (r["certs"][:, 0] == 0).all()


def test_without_refs_and_without_segments(ramcrc, oracle_mod):
    """d_refs = NULL gives the same outputs; n_seg = 0 writes nothing."""
    case = sc.mixed(oracle_mod)
    a = sc.run_host(ramcrc, oracle_mod, case)
    b = sc.run_host(ramcrc, oracle_mod, case, want_refs=False)
    assert b["refs"] is None and np.array_equal(a["out"], b["out"]) and a["counts"] == b["counts"]
    out = np.full(64, sc.FILL, np.uint8)
    none = np.zeros((0, 4), np.uint32)
    _, _, refs, counts = ramcrc.replay_sidelog_host(np.zeros(0, np.uint8), 0, 0, none, none,
                                                    np.zeros((0, 2), np.uint32), sc.TS, out, 64, 64)
    assert (out == sc.FILL).all() and sc.counts_dict(counts) == dict.fromkeys(sc.COUNT_NAMES, 0)


@pytest.mark.parametrize("variant", sc.REFUSALS)
def test_refusals(ramcrc, oracle_mod, variant):
    """Every refusal of the append and a partition that is not 0: EINVAL and
    nothing written; a valid call after it."""
    case = sc.mixed(oracle_mod, seed=39, nseg=2, n=40)
    buf, certs, status, table = sc.host_source(oracle_mod, case)
    good = case.live_of(table)
    bad, bad_table = sc.refusal(variant, table, good, 2)
    out = np.full(2 * case.out_stride, sc.FILL, np.uint8)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ramcrc.replay_sidelog_host(buf, case.cap, 2, status, bad_table, bad, sc.TS, out,
                                   case.out_stride, case.out_capacity)
    assert e.value.code == ramcrc.EINVAL
    assert (out == sc.FILL).all()
    case.live = good
    sc.run_host(ramcrc, oracle_mod, case)


def test_argument_checks(ramcrc, oracle_mod):
    case = sc.special(oracle_mod)
    buf, certs, status, table = sc.host_source(oracle_mod, case)
    live = case.live_of(table)
    out = np.full(case.cap, sc.FILL, np.uint8)
    with pytest.raises(ramcrc.RamcrcError) as e:   # out_stride < out_capacity
        ramcrc.replay_sidelog_host(buf, case.cap, 1, status, table, live, sc.TS, out, case.cap - 16,
                                   case.cap)
    assert e.value.code == ramcrc.EINVAL
    with pytest.raises(ramcrc.RamcrcError) as e:   # the outputs inside the source
        ramcrc.replay_sidelog_host(buf, case.cap, 1, status, table, live, sc.TS, buf[case.cap // 2:],
                                   case.cap // 2, 1024)
    assert e.value.code == ramcrc.EINVAL
    assert (out == sc.FILL).all()


def test_timestamp_is_the_argument(ramcrc, oracle_mod):
    """Another timestamp: the same bytes but the timestamps and checksums."""
    case = sc.special(oracle_mod)
    buf, certs, status, table = sc.host_source(oracle_mod, case)
    live = case.live_of(table)
    outs = []
    for ts in (0, 0xFFFFFFFF):
        out = np.full(case.out_stride, sc.FILL, np.uint8)
        got = ramcrc.replay_sidelog_host(buf, case.cap, 1, status, table, live, ts, out,
                                         case.out_stride, case.out_capacity)
        exp = sc.expected(oracle_mod, buf, case.cap, table, status, live, 1, case.out_capacity, ts)
        sc.check(oracle_mod, exp, buf, case.cap, table, live, out, case.out_stride, case.out_capacity,
                 got[0], got[1], got[2], got[3], case.bad)
        outs.append(out)
    assert not np.array_equal(outs[0], outs[1])


def test_chain(ramcrc, oracle_mod):
    """Two replay-table adds, the live lists, a side log per batch: the
    survivors read back from the outputs through the references are the
    replay's, and every output passes the oracle's walk and verify."""
    cap = 64 * sc.KiB
    batches = [tc.HostBatch(oracle_mod, lists, cap) for lists in sc.chain_lists(oracle_mod)]
    t = ramcrc.ReplayTableHost(4096, 4)
    for b in batches:
        tc.host_add(t, b)
    lives = [t.live(j)[1] for j in range(2)]
    got = {}
    for b, live in zip(batches, lives):
        case = sc.Case([], cap, live)
        out = np.full(b.nseg * cap, sc.FILL, np.uint8)
        r = ramcrc.replay_sidelog_host(b.buf, cap, b.nseg, b.status, b.table, live, sc.TS, out, cap, cap)
        exp = sc.expected(oracle_mod, b.buf, cap, b.table, b.status, live, b.nseg, cap)
        sc.check(oracle_mod, exp, b.buf, cap, b.table, live, out, cap, cap, *r, what="chain")
        assert sc.counts_dict(r[3])["left_out"] == 0 and case.live_of(b.table).shape == live.shape
        part = sc.read_survivors(out, cap, r[2])
        assert not set(part) & set(got)
        got.update(part)
    t.close()
    assert got == tc.survivors(batches, lives) == tc.replayed(batches)


def test_repeated_calls(ramcrc, oracle_mod):
    """Two shapes, then the first again."""
    a, b = sc.mixed(oracle_mod), sc.key_lengths(oracle_mod)
    ra = sc.run_host(ramcrc, oracle_mod, a)
    sc.run_host(ramcrc, oracle_mod, b)
    again = sc.run_host(ramcrc, oracle_mod, a)
    assert np.array_equal(ra["out"], again["out"])
