"""ramcrc_recovery_append_host: the append loop of RecoverySegmentBuilder::build
(src/RecoverySegmentBuilder.cc:61-203) over a caller's placement list, on the
host.  The record tables come from the oracle's checkMetadataIntegrity
restatement; the expected bytes and certificates from append_cases (plain
Python over the table and the source bytes).  Every output region is
pre-filled with 0xA5, so a write at or past the head shows."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import segment_cases

KiB = 1024


def _run(ramcrc, oracle, buf, certs, cap, nseg, place, n_part, out_capacity, out_stride=None,
         what="", edit=None):
    status, table = ac.host_walk(oracle, buf, certs, nseg, cap)
    if edit is not None:
        edit(table)   # a hand-edited record, as a caller's own table may hold
    if callable(place):
        place = place(table)
    place = np.ascontiguousarray(place, np.uint32).reshape(-1, 2)
    out_stride = out_stride or (out_capacity + 15) // 16 * 16
    out = np.full(nseg * n_part * out_stride, ac.FILL, np.uint8)
    got_certs, got_stat = ramcrc.recovery_append_host(buf, cap, nseg, status, table, place, n_part,
                                                      out, out_stride, out_capacity)
    exp = ac.expected(buf, cap, table, status, place, nseg, n_part, out_capacity)
    ac.check_outputs(oracle, exp, out, out_stride, out_capacity, got_certs, got_stat, what)
    return table, place, out, got_certs, got_stat


def test_dtypes_match_the_abi():
    assert segments.PLACEMENT_DTYPE.itemsize == 8 and segments.APPEND_STATUS_DTYPE.itemsize == 8
    assert segments.SEG_APPEND_FULL == 64 and segments.SEG_SOURCE_BAD == 128


def test_reference_goldens(ramcrc, oracle_mod, golden):
    """Case 1: SegmentTest's "hi", "yo!" and empty certificates."""
    buf, certs, cap = ac.golden_source(golden)
    all_records = lambda t: [(r, 0) for r in range(t.shape[0])]
    _, _, _, got, stat = _run(ramcrc, oracle_mod, buf, certs, cap, 3, all_records, 1, 4 * KiB)
    assert got.tolist() == certs.tolist()
    assert stat.tolist() == [[segments.SEG_OK, 1], [segments.SEG_OK, 1], [segments.SEG_OK, 0]]


def test_mixed_entries(ramcrc, oracle_mod):
    """Case 2: objects of 24 B .. 200 KiB, tombstones, type 9; drops, records in
    every partition, records twice in one."""
    cap, nseg, n_part = 256 * KiB, 6, 5
    buf, certs, counts = segment_cases.mixed_segments(oracle_mod, nseg, cap)
    table, place, _, _, stat = _run(ramcrc, oracle_mod, buf, certs, cap, nseg,
                                    lambda t: ac.mixed_placements(t, n_part, 7), n_part, cap)
    assert table.shape[0] == counts.sum() and place.shape[0] > table.shape[0]
    assert (stat[:, 0] == segments.SEG_OK).all()


def test_every_alignment(ramcrc, oracle_mod):
    """Case 3: all 256 (source, destination) residues mod 16."""
    cap, n_part = 256 * KiB, 3
    buf, certs = ac.alignment_source(oracle_mod, cap)
    table, place, _, _, _ = _run(ramcrc, oracle_mod, buf, certs, cap, 1,
                                 lambda t: ac.alignment_placements(t, n_part), n_part, cap)
    assert len(ac.alignment_pairs(table, place, n_part, cap)) == 256
    assert set(table[:, 2].tolist()) == set(range(81))


def test_length_byte_boundaries(ramcrc, oracle_mod):
    """Case 4: 255, 256, 65,535 and 65,536 bytes; a source entry with a
    non-minimal length field is written in the 1-byte form."""
    cap = 1024 * KiB
    buf, certs = ac.boundary_source(oracle_mod, cap)
    place = lambda t: [(r, p) for r in range(t.shape[0]) for p in ((0, 1) if r % 2 else (1,))]
    table, _, out, _, _ = _run(ramcrc, oracle_mod, buf, certs, cap, 1, place, 2, cap)
    assert table[1].tolist()[2:] == [10, segments.LOG_ENTRY_TYPE_OBJ | (1 << 6)]
    assert table[6].tolist()[2:] == [33, segments.LOG_ENTRY_TYPE_OBJ | (3 << 6)]
    # output 0 holds records 1, 3, 5, 7: the 10-byte payload first, 1 length byte
    assert out[:2].tolist() == [segments.LOG_ENTRY_TYPE_OBJ, 10]
    assert sorted(set(table[:, 2].tolist())) == [0, 1, 10, 33, 255, 256, 257, 2047, 2048, 65535, 65536]


def test_capacity(ramcrc, oracle_mod):
    """Case 5: an exact fit is appended; one byte short is refused, with every
    later placement of that output (a 0-length one too)."""
    buf, certs, cap, place, n_part, out_capacity = ac.capacity_case(oracle_mod)
    _, _, _, got, stat = _run(ramcrc, oracle_mod, buf, certs, cap, 1, place, n_part, out_capacity)
    assert stat.tolist() == [[segments.SEG_OK, 3], [segments.SEG_APPEND_FULL, 2]]
    assert got[:, 0].tolist() == [out_capacity, 102 + 303]


def test_bad_source(ramcrc, oracle_mod):
    """Case 6: a source whose certificate fails contributes nothing."""
    nseg, cap, n_part = 4, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 61)
    certs = certs.copy()
    certs[2, 1] ^= 1
    _, _, _, got, stat = _run(ramcrc, oracle_mod, buf, certs, cap, nseg,
                              lambda t: ac.mixed_placements(t, n_part, 8), n_part, cap)
    empty = ac.expected_cert(oracle_mod, b"")
    for k in range(nseg * n_part):
        if k // n_part == 2:
            assert tuple(got[k]) == empty and tuple(stat[k]) == (segments.SEG_SOURCE_BAD, 0)
        else:
            assert stat[k, 0] == segments.SEG_OK
    for s in (0, 1, 3):   # (the expectation above pins their bytes; here: they are not empty)
        assert stat[s * n_part:(s + 1) * n_part, 1].sum() > 0


@pytest.mark.parametrize("variant", ["decreasing", "record_at_n_entries", "partition_at_n_part",
                                     "segment_at_n_seg", "second_run"])
def test_refusals(ramcrc, oracle_mod, variant):
    """Case 7 (the host form takes a plain count, so it has no n_place >
    place_cap variant): EINVAL, nothing written, and a valid call after it.
    The last two damage the table, not the list: a placed record whose segment
    field is n_seg, and placed records that visit segment 0, then 1, then 0
    again (the device form refuses a table whose segments are not contiguous
    runs)."""
    nseg, cap, n_part = 2, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 71)
    status, table = ac.host_walk(oracle_mod, buf, certs, nseg, cap)
    good = ac.mixed_placements(table, n_part, 9)
    bad = good.copy()
    bad_table = table.copy()
    mid = bad.shape[0] // 2
    if variant == "decreasing":
        bad[mid, 0] = bad[mid - 1, 0] - 1
    elif variant == "record_at_n_entries":
        bad[-1, 0] = table.shape[0]
    elif variant == "partition_at_n_part":
        bad[mid, 1] = n_part
    elif variant == "segment_at_n_seg":
        bad_table[bad[mid, 0], 0] = nseg
    else:
        assert table[bad[0, 0], 0] == 0 and table[bad[-1, 0], 0] == 1
        assert bad[-2, 0] != bad[-1, 0] and table[bad[-2, 0], 0] == 1
        bad_table[bad[-1, 0], 0] = 0
    out = np.full(nseg * n_part * cap, ac.FILL, np.uint8)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ramcrc.recovery_append_host(buf, cap, nseg, status, bad_table, bad, n_part, out, cap, cap)
    assert e.value.code == ramcrc.EINVAL
    assert (out == ac.FILL).all()
    _run(ramcrc, oracle_mod, buf, certs, cap, nseg, good, n_part, cap)


@pytest.mark.parametrize("damage", ["overlong_flag", "payload_past_stride"])
def test_record_that_never_fits(ramcrc, oracle_mod, damage):
    """A mid-run record flagged RAMCRC_SEG_ENTRY_OVERLONG, or whose length was
    edited so that its payload runs past seg_stride, placed in partition 0 of
    segment 0 with later records behind it: it "never fits" (include/ramcrc.h),
    so that output is APPEND_FULL and holds only the records before it, while
    the other partitions and the other segment get everything placed in them
    (_run checks the bytes against append_cases.expected)."""
    nseg, cap, n_part = 2, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 75)
    where = {}

    def edit(table):
        n0 = int((table[:, 0] == 0).sum())
        rec = n0 // 2 // n_part * n_part   # placed in partition 0
        assert 0 < rec < n0 - n_part
        ac.damage_record(table, rec, damage, cap)
        where["rec"], where["n0"] = rec, n0

    place = lambda t: [(r, r % n_part) for r in range(t.shape[0])]
    table, place, _, _, stat = _run(ramcrc, oracle_mod, buf, certs, cap, nseg, place, n_part, cap,
                                    edit=edit)
    rec, n0, n = where["rec"], where["n0"], table.shape[0]
    assert stat[0].tolist() == [segments.SEG_APPEND_FULL, rec // n_part]
    assert stat[1].tolist() == [segments.SEG_OK, len(range(1, n0, n_part))]
    assert stat[2].tolist() == [segments.SEG_OK, len(range(2, n0, n_part))]
    assert (stat[n_part:, 0] == segments.SEG_OK).all() and stat[n_part:, 1].sum() == n - n0


def test_argument_checks(ramcrc, oracle_mod):
    nseg, cap = 1, 64 * KiB
    buf, certs = ac.small_mixed(oracle_mod, nseg, 72)
    status, table = ac.host_walk(oracle_mod, buf, certs, nseg, cap)
    place = np.zeros((1, 2), np.uint32)
    out = np.full(cap, ac.FILL, np.uint8)
    for n_part, stride, capacity in ((0, cap, cap), (1, cap - 16, cap)):
        with pytest.raises(ramcrc.RamcrcError) as e:
            ramcrc.recovery_append_host(buf, cap, nseg, status, table, place, n_part, out,
                                        stride, capacity)
        assert e.value.code == ramcrc.EINVAL
    with pytest.raises(ramcrc.RamcrcError) as e:   # the outputs inside the source
        ramcrc.recovery_append_host(buf, cap, nseg, status, table, place, 1, buf[cap // 2:],
                                    cap // 2, 1024)
    assert e.value.code == ramcrc.EINVAL
    assert (out == ac.FILL).all()


def test_degenerate_inputs(ramcrc, oracle_mod):
    """Case 10: no placements; and n_part = 1 with every record placed, where
    the output equals the source's [0, segment_length)."""
    nseg, cap = 3, 64 * KiB
    buf, certs = ac.small_mixed(oracle_mod, nseg, 73)
    _, _, _, got, stat = _run(ramcrc, oracle_mod, buf, certs, cap, nseg,
                              np.zeros((0, 2), np.uint32), 4, cap)
    assert (stat == [segments.SEG_OK, 0]).all() and (got[:, 0] == 0).all()
    all_records = lambda t: [(r, 0) for r in range(t.shape[0])]
    _, _, out, got, _ = _run(ramcrc, oracle_mod, buf, certs, cap, nseg, all_records, 1, cap)
    assert got.tolist() == certs.tolist()
    for i in range(nseg):
        n = int(certs[i, 0])
        assert np.array_equal(out[i * cap:i * cap + n], buf[i * cap:i * cap + n])


def test_many_partitions(ramcrc, oracle_mod):
    """More partitions than the device scan keeps in LDS (512), small outputs:
    several of them fill up."""
    nseg, cap, n_part, out_capacity = 2, 64 * KiB, 600, 256
    buf, certs = ac.small_mixed(oracle_mod, nseg, 74)
    _, _, _, _, stat = _run(ramcrc, oracle_mod, buf, certs, cap, nseg,
                            lambda t: ac.mixed_placements(t, n_part, 10), n_part, out_capacity)
    assert (stat[:, 0] == segments.SEG_APPEND_FULL).any() and (stat[:, 0] == segments.SEG_OK).any()
