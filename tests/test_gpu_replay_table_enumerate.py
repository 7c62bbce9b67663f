"""ramcrc_replay_table_enumerate_device: one reply of a table enumeration packed
on the GPU (k_en_size, k_en_scan, k_en_gather), MasterService::enumerate
(src/MasterService.cc:409-456) over Enumeration::complete
(src/Enumeration.cc:269-351).

The scenarios are enumerate_cases.py's, the ones
test_replay_table_enumerate_host.py runs on the host: every batch is walked by
ctx.segment_walk, the expectation (plain Python, held against the goldens and
the live query's winners) is what every device call is held against, and a host
table fed the same batches must give the same bytes.  Payload and summary are
pre-filled with 0xA5 and checked past their ends."""
import numpy as np
import pytest

from ramcloud_amd import segments

import enumerate_cases as en
import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = en.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return en.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv):
    en.case_goldens(drv)


@pytest.mark.parametrize("n", [1, 2, 3, 40])
def test_buckets_of_n_keys_and_every_cut(drv, n):
    en.case_buckets(drv, ns=(n,))


def test_wrap_and_tile_edges(drv):
    en.case_wrap_and_tile_edges(drv)


def test_bucket_limit_at_every_value(drv):
    en.case_every_limit(drv)


def test_selection(drv):
    en.case_selection(drv)


def test_more_tiles_than_a_step_of_the_scan(drv):
    en.case_many_tiles(drv)


def test_alignment_and_size_classes(drv):
    """Every copy class, and the payload at every destination alignment 0-15."""
    en.case_size_classes(drv)


def test_multi_key_objects_and_broken_key_tables(drv):
    en.case_multi_key(drv)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_cursor_walk_gives_every_object_once(drv, seed):
    en.case_random_walks(drv, seed)


def test_read_only(drv, mixed):
    """The call leaves lookups, live lists, stats and every batch array unchanged."""
    en.case_read_only(drv, mixed)


# --------------------------------------------------------------- grid size
@pytest.mark.parametrize("ncu", [1, 2, 3])
def test_small_grids(ramcrc, oracle_mod, ncu):
    """Grids sized for 1, 2 and 3 CUs (8 workgroups of 256 lanes a CU): at
    S = 8192 the 32 tiles of buckets take a 1-CU grid four passes; the walks,
    the cuts at every entry and the bucket limits at the tile edges against the
    expectation and the host form."""
    c = ramcrc.Context(0)
    try:
        c.set_cus(ncu)
        en.case_wrap_and_tile_edges(en.DeviceDriver(ramcrc, oracle_mod, c))
    finally:
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_spoiled_tables(ramcrc, oracle_mod):
    """Spoiled by a bad segment number and by the key capacity: the pre-filled
    payload stays untouched, the summary is zero with spoiled = 1, the call
    raises no refusal of its own, and after the reset the table answers
    again."""
    c = ramcrc.Context(0)
    drv = en.DeviceDriver(ramcrc, oracle_mod, c)
    try:
        b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad.d_entries[2, 0] = 1   # = n_seg
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        for first, spoiler, tid in ((b, bad, 1), (full, more, 7)):
            tab = en.table(drv, 64, 4)
            try:
                tab.add(first)
                g, _ = en.ask(tab, en.checked(tab), en.key_hash, en.Args(tid), what="before")
                assert g.summary["objects"] >= 1
                tc.Added(spoiler).add(tab.t)
                with pytest.raises(ramcrc.RamcrcError) as e:
                    c.check()
                assert e.value.code == ramcrc.EREFUSED
                for a in (en.Args(tid), en.Args(tid, bucket=3, limit=9, keys_only=True), en.Args(tid, bucket=128)):
                    g = en.Asked(c, tab.t, a, 256, 256)   # check() passes
                    assert g.summary == en.SPOILED_SUMMARY and (g.payload_all == FILL).all()
                tab.reset()
                tab.add(first)
                en.ask(tab, en.checked(tab), en.key_hash, en.Args(tid), what="after the reset")
            finally:
                tab.close()
    finally:
        c.close()


def test_bad_arguments(ctx, ramcrc):
    """Unknown flags, missing or misaligned arrays, a cursor or a limit past
    the table, too many or unusable stale frames are EINVAL before any launch:
    nothing is written and the context stays clean."""
    t = ramcrc.ReplayTable(ctx, 64, 1)   # S = 128
    try:
        z = torch.full((512,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        fr = np.zeros(9, segments.ENUM_FRAME_DTYPE)
        fr["num_buckets"] = 4
        bad_fr = fr.copy()
        bad_fr["num_buckets"][1] = 12
        zero_fr = fr.copy()
        zero_fr["num_buckets"][0] = 0
        good = dict(bucket=0, limit=0, stale=None, n_stale=0, flags=0, payload=z[64:128], cap=64, summary=z[192:280])
        assert p(good["summary"]) % 8 == 0
        cases = [dict(flags=2), dict(flags=1 << 31), dict(summary=None), dict(summary=z[196:284]), dict(payload=None),
                 dict(bucket=129), dict(bucket=5, limit=4), dict(limit=129), dict(stale=fr, n_stale=9),
                 dict(stale=None, n_stale=1), dict(stale=bad_fr, n_stale=2), dict(stale=zero_fr, n_stale=1)]
        L = ramcrc.lib().ramcrc_replay_table_enumerate_device
        call = lambda a: L(t._h, 1, 0, en.MAXH, a["bucket"], 0, a["limit"],
                           None if a["stale"] is None else a["stale"].ctypes.data, a["n_stale"], a["flags"],
                           p(a["payload"]), a["cap"], 64, p(a["summary"]), None)
        for change in cases:
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(call(dict(good, **change)), "enumerate")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
        for change in (dict(), dict(bucket=128), dict(bucket=5, limit=5), dict(limit=128), dict(stale=fr, n_stale=8),
                       dict(payload=None, cap=0), dict(flags=1)):
            assert call(dict(good, **change)) == 0, change
        ctx.check()
        s = z[192:280].cpu().numpy().view(segments.ENUMERATE_SUMMARY_DTYPE)[0]
        assert en.summary_dict(s) == dict(en.ZERO_SUMMARY, num_buckets=128, next_bucket=128)
    finally:
        t.close()


def test_the_call_does_not_allocate_after_reserve(ramcrc, oracle_mod):
    """After ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(S / 256), 0) no call on the
    table takes scratch, as the header states."""
    c2 = ramcrc.Context(0)   # a context that has reserved nothing yet
    drv = en.DeviceDriver(ramcrc, oracle_mod, c2)
    tab = None
    try:
        key_cap = 3000
        S = en.slots(key_cap)
        tab, hash_of = en.placed_table(drv, key_cap, [(5, 1, 3, 30), (S - 1, 1, 2, 7), (4000, 1, 1, 100)])
        ep = en.checked(tab)
        c2.reserve(32 + 16 * -(-S // 256), 0)
        before = ramcrc.scratch_allocations()
        g, w = en.ask(tab, ep, hash_of, en.Args(1), what="the whole table")
        en.ask(tab, ep, hash_of, en.Args(1, bucket=5, max_bytes=80), what="a cut")
        assert ramcrc.scratch_allocations() == before
        assert g.summary["objects"] == 6
    finally:
        if tab is not None:
            tab.close()
        c2.close()
