"""ramcrc_recovery_append_device: walked records appended into per-partition
recovery segments on the GPU, with their certificates from the same pass
(RecoverySegmentBuilder::build's append loop, src/RecoverySegmentBuilder.cc:61-203).

The record table comes from ctx.segment_walk on the device; the expected bytes
and certificates from append_cases (plain Python over the table that was read
back and the source bytes, the certificate from the oracle's
checkMetadataIntegrity restatement).  Every output region is pre-filled with
0xA5 and every certificate and status word with a pattern, so a write at or
past a head, or by a refused call, shows.  Every case also runs the host form
and asserts byte-identical outputs."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import segment_cases
from append_cases import PATTERN, Walked, _append, _launch, _u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


def test_reference_goldens(ctx, ramcrc, oracle_mod, golden):
    """Case 1: the certificates of src/SegmentTest.cc:159, 373, 369."""
    buf, certs, cap = ac.golden_source(golden)
    w = Walked(ctx, buf, certs, cap, 3)
    all_records = lambda t: [(r, 0) for r in range(t.shape[0])]
    _, _, got, stat = _append(ctx, ramcrc, oracle_mod, w, all_records, 1, 4 * KiB)
    assert got.tolist() == certs.tolist()
    assert sorted(stat[:, 1].tolist()) == [0, 1, 1]


@pytest.fixture(scope="module")
def mixed(ctx, oracle_mod):
    cap, nseg = 256 * KiB, 6
    buf, certs, _ = segment_cases.mixed_segments(oracle_mod, nseg, cap)
    w = Walked(ctx, buf, certs, cap, nseg)
    place = ac.mixed_placements(w.table, 5, 7)
    exp = ac.expected(buf, cap, w.table, w.status, place, nseg, 5, cap)
    return w, place, exp


@pytest.fixture(scope="module")
def aligned(ctx, oracle_mod):
    cap = 256 * KiB
    buf, certs = ac.alignment_source(oracle_mod, cap)
    return Walked(ctx, buf, certs, cap, 1)


def test_mixed_entries(ctx, ramcrc, oracle_mod, mixed):
    """Case 2; ramcrc_segments_certify_device on the outputs returns the same
    certificates."""
    w, place, exp = mixed
    n_part, cap = 5, w.cap
    _, d_out, certs, stat = _append(ctx, ramcrc, oracle_mod, w, place, n_part, cap, exp=exp)
    assert (stat[:, 0] == segments.SEG_OK).all() and stat[:, 1].sum() == place.shape[0]
    n_out = w.nseg * n_part
    heads = torch.from_numpy(np.ascontiguousarray(certs[:, 0]).view(np.int32)).cuda()
    again = torch.zeros((n_out, 2), dtype=torch.int32, device="cuda")
    flags = torch.zeros(n_out, dtype=torch.int32, device="cuda")
    ctx.certify(d_out, cap, cap, n_out, heads, again, flags)
    ctx.check()
    assert np.array_equal(_u32(again), certs)
    assert (_u32(flags) == segments.SEG_OK).all()


def test_every_alignment(ctx, ramcrc, oracle_mod, aligned):
    """Case 3: all 256 (source, destination) residues mod 16, lengths 0 .. 80."""
    n_part = 3
    place, _, _, _ = _append(ctx, ramcrc, oracle_mod, aligned,
                             lambda t: ac.alignment_placements(t, n_part), n_part, aligned.cap)
    assert aligned.d.data_ptr() % 16 == 0
    assert len(ac.alignment_pairs(aligned.table, place, n_part, aligned.cap)) == 256
    assert set(aligned.table[:, 2].tolist()) == set(range(81))


def test_length_byte_boundaries(ctx, ramcrc, oracle_mod):
    """Case 4."""
    cap = 1024 * KiB
    buf, certs = ac.boundary_source(oracle_mod, cap)
    w = Walked(ctx, buf, certs, cap, 1)
    place = lambda t: [(r, p) for r in range(t.shape[0]) for p in ((0, 1) if r % 2 else (1,))]
    _, d_out, _, _ = _append(ctx, ramcrc, oracle_mod, w, place, 2, cap)
    assert w.table[1].tolist()[2:] == [10, segments.LOG_ENTRY_TYPE_OBJ | (1 << 6)]
    assert d_out[:2].tolist() == [segments.LOG_ENTRY_TYPE_OBJ, 10]
    assert {255, 256, 65535, 65536} <= set(w.table[:, 2].tolist())


def test_capacity(ctx, ramcrc, oracle_mod):
    """Case 5."""
    buf, certs, cap, place, n_part, out_capacity = ac.capacity_case(oracle_mod)
    w = Walked(ctx, buf, certs, cap, 1)
    _, _, got, stat = _append(ctx, ramcrc, oracle_mod, w, place, n_part, out_capacity)
    assert stat.tolist() == [[segments.SEG_OK, 3], [segments.SEG_APPEND_FULL, 2]]
    assert got[:, 0].tolist() == [out_capacity, 102 + 303]


def test_bad_source(ctx, ramcrc, oracle_mod):
    """Case 6."""
    nseg, cap, n_part = 4, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 61)
    certs = certs.copy()
    certs[2, 1] ^= 1
    w = Walked(ctx, buf, certs, cap, nseg)
    assert [int(f) & segments.SEG_OK for f in w.status[:, 0]] == [1, 1, 0, 1]
    _, _, got, stat = _append(ctx, ramcrc, oracle_mod, w,
                              lambda t: ac.mixed_placements(t, n_part, 8), n_part, cap)
    empty = ac.expected_cert(oracle_mod, b"")
    for k in range(2 * n_part, 3 * n_part):
        assert tuple(got[k]) == empty and tuple(stat[k]) == (segments.SEG_SOURCE_BAD, 0)
    for s in (0, 1, 3):
        assert (stat[s * n_part:(s + 1) * n_part, 0] == segments.SEG_OK).all()
        assert stat[s * n_part:(s + 1) * n_part, 1].sum() > 0


@pytest.mark.parametrize("variant", ["decreasing", "record_at_n_entries", "partition_at_n_part",
                                     "n_place_over_cap", "segment_at_n_seg", "second_run"])
def test_refusals(ctx, ramcrc, oracle_mod, variant):
    """Case 7: RAMCRC_EREFUSED from check(), nothing written, and a following
    valid call on the same context is correct.  The last two damage the
    device's record table, not the list: a placed record whose segment field
    is n_seg, and placed records that visit segment 0, then 1, then 0 again
    (the table's segments are not contiguous runs); the table is put back for
    the valid call."""
    nseg, cap, n_part = 2, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 71)
    w = Walked(ctx, buf, certs, cap, nseg)
    good = ac.mixed_placements(w.table, n_part, 9)
    bad = good.copy()
    mid = bad.shape[0] // 2
    kw = {}
    edited = None
    if variant == "decreasing":
        bad[mid, 0] = bad[mid - 1, 0] - 1
    elif variant == "record_at_n_entries":
        bad[-1, 0] = w.table.shape[0]
    elif variant == "partition_at_n_part":
        bad[mid, 1] = n_part
    elif variant == "n_place_over_cap":
        kw = dict(place_cap=bad.shape[0] - 1, n_place=bad.shape[0])
    elif variant == "segment_at_n_seg":
        edited = int(bad[mid, 0])
        w.d_entries[edited, 0] = nseg
    else:
        # (the walk fixes no order across segments: the first run's segment,
        # 0 or 1, is the one that comes back at the end of the list)
        edited = int(bad[-1, 0])
        first, last = int(w.table[bad[0, 0], 0]), int(w.table[edited, 0])
        assert first != last and bad[-2, 0] != edited and w.table[bad[-2, 0], 0] == last
        w.d_entries[edited, 0] = first
    d_out, d_certs, d_stat = _launch(ctx, w, bad, n_part, cap, cap, **kw)
    with pytest.raises(ramcrc.RamcrcError) as e:
        ctx.check()
    assert e.value.code == ramcrc.EREFUSED
    assert bool((d_out == ac.FILL).all())
    assert (_u32(d_certs) == PATTERN).all() and (_u32(d_stat) == PATTERN).all()
    ctx.check()   # the refusal was taken
    if edited is not None:
        w.d_entries[edited, 0] = int(w.table[edited, 0])
    _append(ctx, ramcrc, oracle_mod, w, good, n_part, cap)


@pytest.mark.parametrize("damage", ["overlong_flag", "payload_past_stride"])
def test_record_that_never_fits(ctx, ramcrc, oracle_mod, damage):
    """A mid-run record of a real walk table flagged RAMCRC_SEG_ENTRY_OVERLONG,
    or with a length edited so that its payload runs past seg_stride (the same
    edit in the device table and the copy read back), placed in partition 0
    with later records behind it: it never fits (include/ramcrc.h), so that
    output is APPEND_FULL with only the records before it, and the other
    partitions and the other segment get everything placed in them."""
    nseg, cap, n_part = 2, 64 * KiB, 3
    buf, certs = ac.small_mixed(oracle_mod, nseg, 75)
    w = Walked(ctx, buf, certs, cap, nseg)
    n = w.table.shape[0]
    seg = int(w.table[0, 0])                      # the segment whose run comes first
    n0 = int((w.table[:, 0] == seg).sum())
    assert (w.table[:n0, 0] == seg).all()
    rec = n0 // 2 // n_part * n_part              # placed in partition 0
    assert 0 < rec < n0 - n_part
    ac.damage_record(w.table, rec, damage, cap)
    w.d_entries[rec] = torch.from_numpy(w.table[rec].view(np.int32)).cuda()
    place = [(r, r % n_part) for r in range(n)]
    _, _, _, stat = _append(ctx, ramcrc, oracle_mod, w, place, n_part, cap)
    k = seg * n_part
    assert stat[k].tolist() == [segments.SEG_APPEND_FULL, rec // n_part]
    assert stat[k + 1].tolist() == [segments.SEG_OK, len(range(1, n0, n_part))]
    assert stat[k + 2].tolist() == [segments.SEG_OK, len(range(2, n0, n_part))]
    rest = np.delete(stat, [k, k + 1, k + 2], axis=0)
    assert (rest[:, 0] == segments.SEG_OK).all() and rest[:, 1].sum() == n - n0


def test_unaligned_outputs(ctx, ramcrc, oracle_mod, aligned):
    """"d_out and out_stride are free" (include/ramcrc.h): case 3 again with
    d_out three bytes into its allocation and out_stride = out_capacity + 7,
    so every output starts at another residue mod 16.  The three bytes before
    d_out and every stride gap keep the fill (check_outputs looks at each
    whole stride past the head), and the host form gives the same bytes."""
    w, n_part, lead = aligned, 3, 3
    out_capacity = w.cap
    out_stride = out_capacity + 7
    place = ac.alignment_placements(w.table, n_part)
    d_place = torch.from_numpy(place.view(np.int32)).cuda()
    d_np = torch.tensor([place.shape[0]], dtype=torch.int64, device="cuda")
    n_out = w.nseg * n_part
    whole = torch.full((lead + n_out * out_stride,), ac.FILL, dtype=torch.uint8, device="cuda")
    d_out = whole[lead:]
    assert d_out.data_ptr() % 16 == lead
    d_certs = torch.full((n_out, 2), PATTERN, dtype=torch.int32, device="cuda")
    d_stat = torch.full((n_out, 2), PATTERN, dtype=torch.int32, device="cuda")
    ctx.recovery_append(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, d_place, d_np, n_part,
                        d_out, out_stride, out_capacity, d_certs, d_stat)
    ctx.check()
    got = whole.cpu().numpy()
    assert (got[:lead] == ac.FILL).all()
    out, certs, stat = got[lead:], _u32(d_certs), _u32(d_stat)
    exp = ac.expected(w.buf, w.cap, w.table, w.status, place, w.nseg, n_part, out_capacity)
    ac.check_outputs(oracle_mod, exp, out, out_stride, out_capacity, certs, stat)
    assert (stat[:, 0] == segments.SEG_OK).all() and stat[:, 1].sum() == place.shape[0]
    h_out = np.full(out.size, ac.FILL, np.uint8)
    h_certs, h_stat = ramcrc.recovery_append_host(w.buf, w.cap, w.nseg, w.status, w.table, place,
                                                  n_part, h_out, out_stride, out_capacity)
    assert np.array_equal(h_out, out)
    assert np.array_equal(h_certs, certs) and np.array_equal(h_stat, stat)


def test_one_context_changing_shapes(ctx, ramcrc, oracle_mod, mixed, aligned):
    """Case 8: call A (case 2), call B (case 3 with another n_part), A again;
    each against its own expectation."""
    w, place, exp = mixed
    _append(ctx, ramcrc, oracle_mod, w, place, 5, w.cap, exp=exp, what="A")
    _append(ctx, ramcrc, oracle_mod, aligned, lambda t: ac.alignment_placements(t, 7, seed=23), 7,
            aligned.cap, what="B")
    _append(ctx, ramcrc, oracle_mod, w, place, 5, w.cap, exp=exp, what="A again")


@pytest.mark.parametrize("value_len", [64, 1024])
def test_dense_full_size_segments(ctx, ramcrc, oracle_mod, value_len):
    """Case 9: 2 x 8 MiB of fill_objects entries (about 80,000 records each at
    64 B), partition = record index mod 4; the expectation is built vectorised
    (every entry has the same size and minimal length bytes, so an output is
    the concatenation of its records' source entries)."""
    nseg, cap, n_part, out_capacity = 2, 8 * MiB, 4, 4 * MiB
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, certs=dc)
    buf = d.cpu().numpy()
    eb = segments.entry_bytes(value_len)
    w = Walked(ctx, buf, _u32(dc), cap, nseg, min_entry=eb, d_buf=d)
    n = w.table.shape[0]
    assert n == nseg * per and (value_len != 64 or per > 75000)
    place = np.stack([np.arange(n), np.arange(n) % n_part], 1).astype(np.uint32)
    outs, counts = [], []
    lane = np.arange(eb, dtype=np.int64)
    for s in range(nseg):
        for p in range(n_part):
            idx = np.nonzero((w.table[:, 0] == s) & (np.arange(n) % n_part == p))[0]
            start = s * cap + w.table[idx, 1].astype(np.int64)
            outs.append(buf[(start[:, None] + lane[None, :]).reshape(-1)].tobytes())
            counts.append(idx.size)
    exp = (outs, [segments.SEG_OK] * len(outs), counts)
    _append(ctx, ramcrc, oracle_mod, w, place, n_part, out_capacity, exp=exp)


def test_degenerate_inputs(ctx, ramcrc, oracle_mod):
    """Case 10."""
    nseg, cap = 3, 64 * KiB
    buf, certs = ac.small_mixed(oracle_mod, nseg, 73)
    w = Walked(ctx, buf, certs, cap, nseg)
    _, _, got, stat = _append(ctx, ramcrc, oracle_mod, w, np.zeros((0, 2), np.uint32), 4, cap)
    assert (stat == [segments.SEG_OK, 0]).all() and (got[:, 0] == 0).all()
    all_records = lambda t: [(r, 0) for r in range(t.shape[0])]
    _, d_out, got, _ = _append(ctx, ramcrc, oracle_mod, w, all_records, 1, cap)
    assert got.tolist() == certs.tolist()
    out = d_out.cpu().numpy()
    for i in range(nseg):
        n = int(certs[i, 0])
        assert np.array_equal(out[i * cap:i * cap + n], buf[i * cap:i * cap + n])


def test_many_partitions(ctx, ramcrc, oracle_mod):
    """More partitions than the scan keeps in LDS (512): its states live in
    the context's scratch; small outputs, several fill up."""
    nseg, cap, n_part, out_capacity = 2, 64 * KiB, 600, 256
    buf, certs = ac.small_mixed(oracle_mod, nseg, 74)
    w = Walked(ctx, buf, certs, cap, nseg)
    _, _, _, stat = _append(ctx, ramcrc, oracle_mod, w,
                            lambda t: ac.mixed_placements(t, n_part, 10), n_part, out_capacity)
    assert (stat[:, 0] == segments.SEG_APPEND_FULL).any() and (stat[:, 0] == segments.SEG_OK).any()


@pytest.mark.parametrize("n_part", [8, 64])
def test_eight_scan_waves_per_segment(ctx, ramcrc, oracle_mod, aligned, n_part):
    """From 8 partitions on, a small batch gets 8 scan waves per source
    segment, each owning every eighth partition (1 and 8 partitions each
    here), with the states in LDS."""
    _append(ctx, ramcrc, oracle_mod, aligned,
            lambda t: ac.alignment_placements(t, n_part, seed=29 + n_part), n_part, 64 * KiB)


def test_argument_checks(ctx, ramcrc, oracle_mod, aligned):
    w = aligned
    place = np.zeros((1, 2), np.uint32)
    for n_part, stride, capacity in ((0, 4096, 4096), (1, 4080, 4096)):
        with pytest.raises(ramcrc.RamcrcError) as e:
            _launch(ctx, w, place, n_part, capacity, stride)
        assert e.value.code == ramcrc.EINVAL
    d_place = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    d_np = torch.ones(1, dtype=torch.int64, device="cuda")
    res = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(ramcrc.RamcrcError) as e:   # the outputs inside the source
        ctx.recovery_append(w.d, w.cap, 1, w.d_status, w.d_entries, w.d_n, d_place, d_np, 1,
                            w.d[w.cap // 2:], w.cap // 2, 1024, res, res.clone())
    assert e.value.code == ramcrc.EINVAL
    with pytest.raises(ramcrc.RamcrcError) as e:   # a null pointer
        ctx.recovery_append(w.d, w.cap, 1, w.d_status, w.d_entries, w.d_n, d_place, d_np, 1,
                            None, 4096, 4096, res, res.clone())
    assert e.value.code == ramcrc.EINVAL
    ctx.check()
