"""The device entry points on contexts sized for 1 and 3 CUs.

Every launch grid is capped by the context's CU count (ramcrc_ctx_set_cus) and
work beyond the cap goes round a grid-stride or persistent loop.  At the 256
CUs of a default context the caps are so high that the shapes of the other GPU
tests pass most of these loops once; a context sized for one CU (three: not a
power of two, so the work does not divide evenly) makes inputs of a few MiB
wrap each of them several times.  set_cus only sizes grids, so the launches
run on the default stream without a CU mask.  Every result must still equal
the oracle's bit for bit, and, for the table cases, what a default context
gives for the same input (a mismatch then says which side is wrong).

Each docstring gives the arithmetic that shows its loop wraps, at 1 / 3 CUs.
"""
import contextlib

import numpy as np
import pytest

from ramcloud_amd import segments, workloads

import append_cases as ac
import segment_cases
from append_cases import Walked, _append

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20
NCU = pytest.mark.parametrize("ncu", [1, 3], ids=["ncu1", "ncu3"])


@contextlib.contextmanager
def sized_context(ramcrc, ncu, **options):
    """A fresh context with set_cus(ncu) (0: every CU), closed afterwards."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    try:
        c.set_cus(ncu)
        for name, value in options.items():
            if name == "serial_walk":
                c.set_serial_walk(value)
            else:
                c.set_option(getattr(ramcrc, name), value)
        yield c
    finally:
        c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_u32(a):
    return _dev(np.ascontiguousarray(a, np.uint32).view(np.int32))


def _dev_u64(a):
    return _dev(np.ascontiguousarray(a, np.uint64).view(np.int64))


def _u32(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _aligned_slice(nbytes, shift=0):
    """nbytes of device memory starting `shift` bytes past a 2 MiB boundary."""
    over = torch.empty(nbytes + 4 * MiB, dtype=torch.uint8, device="cuda")
    a = -over.data_ptr() % (2 * MiB) + shift
    return over[a:a + nbytes]


def _differs(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


# ------------------------------------------------ 1. aligned segment fast path
# (seg_bytes, nseg).  ramcrc_segments_device takes the largest chunk shift s in
# 18 .. 20 for which the base and seg_bytes are multiples of 2^s and, while
# growing, (seg_bytes >> (s + 1)) * nseg >= 2 * waves, waves = 16 * ncu:
#   256 KiB x 40   shift 18 / 18 (not a multiple of 512 KiB): 40 chunks
#   1 MiB x 64     shift 20 / 19 (128, 64 >= 32; 128 >= 96 > 64): 64 / 128 chunks
#   2 MiB x 33     shift 20 / 19 (132, 66 >= 32; 132 >= 96 > 66): 66 / 132 chunks
#   1 MiB x 24     shift 19 / 18 (48 >= 32 > 24; 48 < 96): 48 / 96 chunks
#   1.5 MiB x 30   shift 19 / 18 (90 >= 32, not a multiple of 1 MiB; 90 < 96):
#                  90 / 180 chunks, 3 / 6 per segment
# The one k_chunks workgroup per CU has 16 waves, each taking chunk g, g + 16
# * ncu, ...: 2.5 to 5.6 chunks per wave at one CU, 0.8 to 3.75 at three.
SEGMENT_SHAPES = [(256 * KiB, 40), (1 * MiB, 64), (2 * MiB, 33), (1 * MiB, 24), (3 * MiB // 2, 30)]
SEGMENT_BYTES = 66 * MiB


@pytest.fixture(scope="module")
def segment_case(oracle_mod):
    host = oracle_mod.splitmix_bytes(0x53474D54, SEGMENT_BYTES)
    rng = np.random.default_rng(181920)
    want = {}
    for seg_bytes, nseg in SEGMENT_SHAPES:
        assert seg_bytes * nseg <= SEGMENT_BYTES
        off = np.arange(nseg, dtype=np.uint64) * seg_bytes
        ln = np.full(nseg, seg_bytes, np.uint64)
        init = rng.integers(0, 2 ** 32, nseg, dtype=np.uint64).astype(np.uint32)
        want[seg_bytes, nseg] = (init, oracle_mod.entries(host, off, ln),
                                 oracle_mod.entries(host, off, ln, init=init, finalize=False))
    return host, want


@NCU
def test_aligned_segments_chunk_shifts(ramcrc, segment_case, ncu):
    """ramcrc_segments_device's fast path at chunk shifts 18, 19 and 20 (the
    table at SEGMENT_SHAPES: 40 to 90 chunks over 16 waves at one CU, 40 to
    180 over 48 at three), default initial state with finalized output and
    random initial states with raw output; then the same bytes from a base
    256 KiB past a 2 MiB boundary, which is no multiple of 512 KiB and pins
    shift 18 (40 to 264 chunks)."""
    host, want = segment_case
    with sized_context(ramcrc, ncu) as ctx:
        for shift in (0, 256 * KiB):
            base = _aligned_slice(SEGMENT_BYTES, shift)
            assert base.data_ptr() % (2 * MiB) == shift
            base.copy_(torch.from_numpy(host))
            for (seg_bytes, nseg), (init, w_fin, w_raw) in want.items():
                out = torch.zeros(nseg, dtype=torch.int32, device="cuda")
                ctx.segments(base, seg_bytes, nseg, out)
                assert np.array_equal(_u32(out), w_fin), (shift, seg_bytes, nseg,
                                                          _differs(_u32(out), w_fin))
                ctx.segments(base, seg_bytes, nseg, out, init=_dev_u32(init), finalize=False)
                assert np.array_equal(_u32(out), w_raw), (shift, seg_bytes, nseg, "raw",
                                                          _differs(_u32(out), w_raw))
            ctx.check()


# ------------------------------------------- 2. binned and planned, 100,000
N_TABLE = 100_000


@pytest.fixture(scope="module")
def table_case(oracle_mod):
    """The first 100,000 config-3 entries (100 B / 1 KiB / 4 KiB, packed), and
    for the batch call the same table with about 40 lengths made large."""
    lens = workloads.entry_lengths(N_TABLE)
    offs = workloads.packed_offsets(lens)
    total = int(lens.sum())
    host = workloads.splitmix_bytes_np(workloads.ENTRY_SEED, total)
    rng = np.random.default_rng(100000)
    init = rng.integers(0, 2 ** 32, N_TABLE, dtype=np.uint64).astype(np.uint32)
    # large buffers: the ends of the table, the first and last entry of 1,024-
    # entry plan groups, and spread through the rest; unaligned, overlapping
    where = [0, N_TABLE - 1, 1023, 1024, 2047, 2048, 50 * 1024 - 1, 50 * 1024, 97 * 1024 - 1,
             97 * 1024, 97 * 1024 + 1]
    where += [int(i) for i in rng.choice(np.arange(3000, 96000), 29, replace=False)]
    big = [65535, 65536, 262145] + [int(x) for x in rng.integers(65536, 3 * MiB // 2, len(where) - 3)]
    lens2, offs2 = lens.copy(), offs.copy()
    for i, n in zip(where, big):
        lens2[i] = n
        offs2[i] = int(rng.integers(0, total - n)) | 1
    assert len(set(where)) == len(where) == 40 and int((offs2 + lens2).max()) <= total
    want = {}
    for fin in (True, False):
        want["entries", fin] = oracle_mod.entries(host, offs, lens, init=init, finalize=fin)
        want["batch", fin] = want["entries", fin]
        want["batch_large", fin] = oracle_mod.entries(host, offs2, lens2, init=init, finalize=fin)
    return host, {"entries": (offs, lens), "batch": (offs, lens), "batch_large": (offs2, lens2)}, \
        init, want


def _run_table(ctx, case):
    host, tables, init, want = case
    base, d_init = _dev(host), _dev_u32(init)
    got = {}
    for name, (offs, lens) in tables.items():
        d_off, d_len = _dev_u64(offs), _dev_u64(lens)
        for fin in (True, False):
            out = torch.zeros(N_TABLE, dtype=torch.int32, device="cuda")
            getattr(ctx, name.split("_")[0])(base, d_off, d_len, out, init=d_init, finalize=fin)
            got[name, fin] = _u32(out)
    ctx.check()
    return got


@pytest.fixture(scope="module")
def table_default_grid(ramcrc, table_case):
    with sized_context(ramcrc, 0) as ctx:
        return _run_table(ctx, table_case)


@NCU
def test_table_of_100000_buffers(ramcrc, table_case, table_default_grid, ncu):
    """ramcrc_entries_device and ramcrc_batch_device over 100,000 buffers with
    random initial states, raw and finalized; the batch call also with 40
    buffers of 64 KiB .. 1.5 MiB (65,535, 65,536 and 262,145 among them) at the
    table's ends and at plan-group boundaries.  At 1 / 3 CUs:
      k_bin_count, k_bin_scatter   25 tiles of 4,096 entries over 8 / 24
                                   workgroups (3.1 / 1.04 tiles each)
      k_plan_count                 98 groups of 1,024 over 4 / 12 workgroups
      k_combine<.., true>          391 workgroups' worth of 256 entries over
                                   16 / 48
      k_chunks                     the 39 large buffers' 1 to 7 chunks each, 144 in
                                   all, over 16 / 48 waves
      k_entries                    one workgroup per CU over 108 MB
    Equal to the oracle and to a default context's output."""
    want = table_case[3]
    with sized_context(ramcrc, ncu) as ctx:
        got = _run_table(ctx, table_case)
    for key in want:
        assert np.array_equal(table_default_grid[key], want[key]), \
            ("default grid against the oracle", key, _differs(table_default_grid[key], want[key]))
        assert np.array_equal(got[key], want[key]), \
            ("small grid against the oracle", key, _differs(got[key], want[key]))
        assert np.array_equal(got[key], table_default_grid[key]), key


# -------------------------------------------------- 3 and 4. walk and verify
def _live_objects(buf, cap, table, status):
    ok_seg = (status[:, 0] & segments.SEG_OK) != 0
    return ((table[:, 3] & 0x13F) == segments.LOG_ENTRY_TYPE_OBJ) & (table[:, 2] >= 24) \
        & ok_seg[table[:, 0]]


def _replay_records(buf, cap, table, status):
    return segment_cases.replay_crc_mask(buf, cap, table)


def _record_order(table):
    """Records across segments come in no fixed order (include/ramcrc.h):
    compare by (segment, offset, length)."""
    return np.lexsort((table[:, 2], table[:, 1], table[:, 0]))


class WalkCase:
    """Segments with the oracle's status words, record table (sorted by
    segment and offset) and CRCs of the checked records."""

    def __init__(self, oracle, buf, certs, cap, live):
        self.buf, self.certs, self.cap, self.nseg = buf, np.ascontiguousarray(certs), cap, certs.shape[0]
        self.status, table, crc = segment_cases.oracle_walk(oracle, buf, certs, self.nseg, cap=cap)
        order = _record_order(table)
        self.table = table[order]
        self.live = live(buf, cap, self.table, self.status)
        self.crc = crc[order][self.live]
        self.entries_cap = self.table.shape[0] + 1024

    def run(self, ctx, fused):
        d, dc = _dev(self.buf), _dev_u32(self.certs)
        rv = segments.RecoveryVerify(ctx, self.nseg, self.cap, entries_cap=self.entries_cap)
        if fused:
            rv.verify(d, dc, check=True)
        else:
            rv.walk(d, dc)
            rv.verify_objects(d)
            rv.check()
        torch.cuda.synchronize()
        n = int(rv.n_entries.item())
        assert n <= self.entries_cap
        table, crc = _u32(rv.entries[:n]), _u32(rv.obj_crc[:n])
        order = _record_order(table)
        return _u32(rv.status).copy(), table[order], crc[order]

    def check(self, got, what):
        status, table, crc = got
        bad = np.nonzero((status != self.status).any(axis=1))[0]
        assert bad.size == 0, (what, [(int(s), status[s].tolist(), self.status[s].tolist())
                                      for s in bad[:4]])
        assert table.shape == self.table.shape, (what, table.shape, self.table.shape)
        bad = np.nonzero((table != self.table).any(axis=1))[0]
        assert bad.size == 0, (what, [(table[i].tolist(), self.table[i].tolist()) for i in bad[:4]])
        assert np.array_equal(crc[self.live], self.crc), \
            (what, _differs(crc[self.live], self.crc))


# the calls of cases 3 and 4: split (walk, then verify) and fused, by context options
SPLIT_PARALLEL = ("split, parallel walk", False, {})
SPLIT_SERIAL = ("split, serial walk", False, {"serial_walk": True})
FUSED = [("fused, verify-in-walk %d" % m, True, {"OPT_VERIFY_IN_WALK": m}) for m in (0, 1, 2)]


def _run_walks(ramcrc, case, ncu, calls):
    out = {}
    for what, fused, options in calls:
        with sized_context(ramcrc, ncu, **options) as ctx:
            out[what] = case.run(ctx, fused)
    return out


@pytest.fixture(scope="module")
def object_case(oracle_mod):
    """70 segments of 256 KiB with 2,595 objects of 64-byte values each: two
    value bytes and one stored checksum flipped in different segments, and
    one certificate checksum (that segment's records are inactive)."""
    nseg, cap = 70, 256 * KiB
    buf, certs, counts = segments.object_segments_host(nseg, cap, 64)
    assert (counts == 2595).all()
    eb = segments.entry_bytes(64)
    buf[7 * cap + 100 * eb + eb - 2] ^= 0x10      # a value byte
    buf[66 * cap + 2500 * eb + eb - 40] ^= 0x01   # another, in a late segment
    buf[33 * cap + 1300 * eb + 2 + 1] ^= 0x04     # a stored checksum (payload byte 1)
    certs[20, 1] ^= 0x8000
    case = WalkCase(oracle_mod, buf, certs, cap, _live_objects)
    bad = np.zeros(nseg, np.uint32)
    bad[[7, 66, 33]] = 1
    assert np.array_equal(case.status[:, 3], bad) and case.table.shape[0] == 70 * 2595 > 32768
    assert not case.status[20, 0] & segments.SEG_OK and (np.delete(case.status[:, 0], 20) == 1).all()
    return case


@pytest.fixture(scope="module")
def object_default_grid(ramcrc, object_case):
    return _run_walks(ramcrc, object_case, 0, [SPLIT_PARALLEL, FUSED[1]])


@NCU
def test_walk_verify_181650_records(ramcrc, object_case, object_default_grid, ncu):
    """Walk, object verify and the fused replay call over 70 segments and
    181,650 records, damaged as object_case says: split calls with the parallel
    and the serial walker, the fused call with RAMCRC_OPT_VERIFY_IN_WALK 0, 1
    and 2, a table of n + 1,024 records.  At 1 / 3 CUs:
      k_walk_fix, k_seg_walk       70 segments over 64 / 70 waves (the cap is
                                   64 * ncu: a second round at one CU only)
      k_walk_sync                  70 * 4 parts of 64 KiB in workgroups of 4
                                   waves: 70 workgroups' worth over 8 / 24
      k_walk_copy                  capped at 32 / 96 workgroups, k_walk_copyv
                                   at 16 / 48 workgroups of 4 part-waves
      k_bin_count (records, the    45 tiles of 4,096 records over 8 / 24
      prefetched nr[] pipeline),   workgroups: 5 to 6 / about 2 rounds; the
      k_bin_scatter                inactive segment's records are counted in
                                   a later round
      k_plan_count                 179 groups over 4 / 12 workgroups
      k_combine<.., true>, k_obj_compare   714 workgroups' worth over 16 / 48
    Status words (bad_objects included), the record table and the CRCs of the
    live objects equal the oracle's and a default context's."""
    got = _run_walks(ramcrc, object_case, ncu, [SPLIT_PARALLEL, SPLIT_SERIAL] + FUSED)
    for what, g in object_default_grid.items():
        object_case.check(g, "default grid, " + what)
    for what, g in got.items():
        object_case.check(g, "%d CUs, %s" % (ncu, what))
    for what, ref in object_default_grid.items():
        for k in range(2):
            assert np.array_equal(got[what][k], ref[k]), (what, k)
        assert np.array_equal(got[what][2][object_case.live], ref[2][object_case.live]), what


@pytest.fixture(scope="module")
def kind_cases(oracle_mod, golden):
    """(name, case): the damage batch, the replay mix, and 150 mixed segments
    of 64 KiB (11,839 records of random types and sizes with random payloads:
    junk headers for the fix-up's re-walks in more than 64 segments)."""
    buf, certs, cases = segment_cases.build_batch(oracle_mod)
    damage = WalkCase(oracle_mod, buf, certs, segment_cases.CAPACITY, _live_objects)
    assert damage.live.sum() > 1000
    buf, certs, bad, _ = segment_cases.build_replay_mix(oracle_mod, golden)
    mix = WalkCase(oracle_mod, buf, certs, segment_cases.CAPACITY, _replay_records)
    assert np.array_equal(mix.status[:, 3], bad) and int(bad.sum()) > 0
    buf, certs, counts = segment_cases.mixed_segments(oracle_mod, 150, 64 * KiB, seed=92)
    mixed = WalkCase(oracle_mod, buf, certs, 64 * KiB, _replay_records)
    assert mixed.table.shape[0] == int(counts.sum()) > 10000
    assert (mixed.status[:, 0] == segments.SEG_OK).all()
    return {"damage_batch": damage, "replay_mix": mix, "mixed_150": mixed}


@NCU
@pytest.mark.parametrize("name", ["damage_batch", "replay_mix", "mixed_150"])
def test_every_entry_kind(ramcrc, kind_cases, name, ncu):
    """segment_cases.build_batch (33 segments: clean, damaged values,
    checksums and certificates, overruns, the offset wrap, the cycle, ...),
    build_replay_mix (8 segments of every replayed type, valid and damaged)
    and 150 mixed segments of 64 KiB, as test_walk_verify_damage_batch and
    test_walk_verify_replay_mix run them, through the split calls (both
    walkers) and the fused call with RAMCRC_OPT_VERIFY_IN_WALK 0 and 2.  The 150 segments
    exceed k_walk_fix's and k_seg_walk's 64 waves at one CU (2.3 rounds; 192
    at three, no wrap); every batch has more records than one 4,096-record
    binning tile and 1,024-record plan group, and its large objects' chunks go
    over 16 / 48 waves."""
    case = kind_cases[name]
    got = _run_walks(ramcrc, case, ncu, [SPLIT_PARALLEL, SPLIT_SERIAL, FUSED[0], FUSED[2]])
    for what, g in got.items():
        case.check(g, "%s, %d CUs, %s" % (name, ncu, what))


# ------------------------------------------------------------ 5. write path
@pytest.fixture(scope="module")
def assemble_case(oracle_mod):
    """40,000 serialized objects of the config-3 lengths, packed three bytes
    apart from an odd offset; some shorter than Object::Header (left alone),
    some of exactly 24 bytes, a few past 64 KiB."""
    n = 40_000
    lens = workloads.entry_lengths(n, seed=40000).astype(np.uint64)
    rng = np.random.default_rng(5)
    for length, count in ((0, 5), (3, 5), (23, 20), (24, 30), (64 * KiB + 20, 3), (300_000, 3)):
        lens[rng.choice(n, count, replace=False)] = length
    lens[0], lens[n - 1], lens[1023], lens[1024] = 23, 24, 300_000, 64 * KiB + 20
    offs = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1] + np.uint64(3), out=offs[1:])
    offs += np.uint64(5)
    host = oracle_mod.splitmix_bytes(0x41534D42, int(offs[-1] + lens[-1]) + 16)
    live = lens >= 24
    want = np.zeros(n, np.uint32)
    want[live] = oracle_mod.entries(host, offs[live] + np.uint64(4), lens[live] - np.uint64(4))
    after = host.copy()
    idx = (offs[live][:, None].astype(np.int64) + np.arange(4)).reshape(-1)
    after[idx] = np.ascontiguousarray(want[live]).view(np.uint8)
    assert (~live).sum() >= 30 and (lens == 24).sum() >= 30 and (lens > 64 * KiB).sum() >= 6
    return host, offs, lens, want, after


@NCU
@pytest.mark.parametrize("with_out", [True, False], ids=["out", "no_out"])
def test_assemble_40000_objects(ramcrc, assemble_case, with_out, ncu):
    """ramcrc_assemble_objects_device: every header checksum and, with `out`,
    every reported one against the oracle's CRC of bytes [4, length); no other
    byte of the buffer changes (test_assemble_device_edge_lengths' checks).
    10 binning tiles over 8 / 24 workgroups, 40 plan groups over 4 / 12, 157
    wide-combine workgroups' worth over 16 / 48; the 8 objects past 64 KiB have
    1 or 2 chunks each for the 16 / 48 waves."""
    host, offs, lens, want, after = assemble_case
    d = _dev(host.copy())
    out = torch.full((lens.size,), -1, dtype=torch.int32, device="cuda") if with_out else None
    with sized_context(ramcrc, ncu) as ctx:
        ctx.assemble_objects(d, _dev_u64(offs), _dev_u64(lens), out)
        ctx.check()
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    bad = np.nonzero(got != after)[0]
    assert bad.size == 0, [(int(p), int(got[p]), int(after[p])) for p in bad[:8]]
    if with_out:
        assert np.array_equal(_u32(out), want), _differs(_u32(out), want)


# -------------------------------------------------------- 6. recovery append
@pytest.fixture(scope="module")
def append_sources(oracle_mod):
    """20 mixed segments of 256 KiB and 40 of 64 KiB, each with the oracle's
    walk; and the expectations the two grids share."""
    out = {}
    for cap, nseg, seed in ((256 * KiB, 20, 91), (64 * KiB, 40, 93)):
        buf, certs, _ = segment_cases.mixed_segments(oracle_mod, nseg, cap, seed=seed)
        status, table = ac.host_walk(oracle_mod, buf, certs, nseg, cap)
        out[cap] = (buf, certs, status, table)
    return out, {}


# (segment capacity, segments, partitions, output capacity, placement seed)
APPEND_SHAPES = {"four_partitions": (256 * KiB, 20, 4, 256 * KiB, 7),
                 "states_in_scratch": (256 * KiB, 20, 600, 4096, 11),
                 "four_scan_waves": (256 * KiB, 3, 8, 256 * KiB, 13),
                 "forty_segments": (64 * KiB, 40, 4, 64 * KiB, 17),
                 "forty_segments_scratch": (64 * KiB, 40, 520, 1024, 19)}


@NCU
@pytest.mark.parametrize("shape", list(APPEND_SHAPES))
def test_recovery_append(ramcrc, oracle_mod, append_sources, shape, ncu):
    """ramcrc_recovery_append_device on records walked by the same small-grid
    context, through append_cases._append: bytes, certificates and status
    against append_cases.expected, the fill intact past every head, the host
    form byte-identical.  At 1 / 3 CUs:
      four_partitions    20 segments, 4 partitions, 6,560 placements of 6,026
                         records: k_app_scan has nown = 1 (40 > 16) / 2 (40 <=
                         48 < 80), so 20 / 40 waves' worth over 16 / 40 waves,
                         and at one CU four waves take a second segment with
                         the LDS states of their first; k_app_mark and
                         k_app_copy 26 tiles of 256 placements over 8 / 24
                         workgroups (the copy's nbig[] double buffer from the
                         second tile on: 367 placed payloads of 2 KiB or more,
                         6 of 64 KiB or more)
      states_in_scratch  600 partitions, 4 KiB outputs: the scan states in
                         global scratch, several outputs full; more than 700
                         placement tiles
      four_scan_waves    3 segments, 8 partitions: nown = 4 at one CU (12 <= 16
                         < 24), 8 at three
      forty_segments     40 segments of 64 KiB, 4 partitions: nown = 1 / 1 (80 >
                         48), 40 waves' worth over 16 / 40: two and a half
                         rounds at one CU (eight waves take a third segment,
                         its states in the same LDS)
      forty_segments_scratch   the same source with 520 partitions and 1 KiB
                         outputs: that loop with the states in global scratch."""
    sources, cache = append_sources
    cap, nseg, n_part, out_capacity, seed = APPEND_SHAPES[shape]
    buf, certs, status, table = sources[cap]
    with sized_context(ramcrc, ncu) as ctx:
        w = Walked(ctx, buf[:nseg * cap], certs[:nseg], cap, nseg)
        order = np.lexsort((w.table[:, 1], w.table[:, 0]))
        assert np.array_equal(w.status[:, :3], status[:nseg, :3])
        assert np.array_equal(w.table[order], table[table[:, 0] < nseg])
        place = ac.mixed_placements(w.table, n_part, seed)
        payload = w.table[place[:, 0], 2]
        if shape == "four_partitions":
            assert place.shape[0] > 3 * 2048
            assert (payload >= 2048).sum() > 0 and (payload >= 64 * KiB).sum() > 0
        key = (shape, w.table.tobytes())   # the expectation is the same for both grids
        if key not in cache:
            cache[key] = ac.expected(buf, cap, w.table, w.status, place, nseg, n_part, out_capacity)
        _, _, _, stat = _append(ctx, ramcrc, oracle_mod, w, place, n_part, out_capacity,
                                exp=cache[key], what=shape)
    # (the walk fixes no order across segments, so the seeded placements, and
    # with them which outputs fill up, may differ from run to run; _append has
    # checked every output against the expectation for the list it got)
    if shape.endswith("_scratch"):
        assert (stat[:, 0] == segments.SEG_APPEND_FULL).sum() > 10
        assert (stat[:, 0] == segments.SEG_OK).sum() > 10
