"""ramcrc_replay_table_lookup_device: what the replay table on the GPU holds
for a key (k_rtab_lookup), the batched form of ObjectManager::lookup /
readObject (src/ObjectManager.cc:2704-2741, :325-369).

The scenarios are lookup_cases.py's, the ones test_replay_table_lookup_host.py
runs on the host: every batch is walked by ctx.segment_walk, the expectation
(the plain-Python replay) is held against the device live query's d_winner for
every participant, and every device lookup against the expectation and against
a host table fed the same batches.  Results and counts are pre-filled with
0xA5, so a write past an end shows; the key buffer is uploaded at exactly
keys_bytes."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc
from append_cases import Walked

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20
FILL32 = lc.FILL32


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return lc.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_empty_and_fresh_tables(drv):
    lc.case_empty_and_fresh(drv)


def test_version_relations_across_batches(drv):
    lc.case_relations(drv)


def test_key_identity(drv):
    lc.case_identity(drv)


def test_the_longest_key(drv):
    lc.case_longest_key(drv)


def test_one_probe_chain(drv):
    lc.case_one_chain(drv)


def test_collisions_of_the_seed(drv):
    lc.case_seed_collisions(drv)


def test_given_and_computed_hashes_mix(drv, mixed):
    lc.case_mixed_hashes(drv, mixed)


def test_an_absent_key_on_a_claimed_slot(drv):
    lc.case_absent_on_a_claimed_slot(drv)


def test_multi_key_objects(drv):
    lc.case_multi_key(drv)


def test_bad_queries_among_good_ones(drv):
    lc.case_bad_queries(drv)


def test_duplicates(drv):
    lc.case_duplicates(drv)


def test_exhaustive_cross_check(drv, mixed):
    lc.case_exhaustive(drv, mixed)


def test_read_only(drv, mixed):
    lc.case_read_only(drv, mixed)


def test_nullable_and_empty_arguments(drv):
    lc.case_nullable_and_empty(drv)


def test_reference_scenarios(drv):
    lc.case_reference(drv)


# --------------------------------------------------------------- grid size
@pytest.fixture(scope="module")
def grid_case(ctx, ramcrc):
    """The 249,165-record table of test_gpu_replay_table.py's small-grid test
    (two 8 MiB segments of 64-byte objects, then a copy of the first), and
    250,000 queries: every second one a key of batch 0 in a shuffled order,
    the others the same keys under a table id no record has."""
    cap = 8 * MiB
    buf, certs, counts = segments.object_segments_host(2, cap, 64)
    w0 = Walked(ctx, buf, certs, cap, 2, min_entry=64)
    w1 = Walked(ctx, buf[:cap].copy(), certs[:1], cap, 1, min_entry=64)
    per = int(counts[0])
    n0 = 2 * per
    assert w0.table.shape[0] == n0 and w1.table.shape[0] == per and 3 * per == 249165
    t = w0.table.astype(np.int64)
    pay = t[:, 1] + 1 + ((t[:, 3] >> 6) & 3) + 1
    at = t[:, 0] * cap + pay
    assert (buf[at + 24] == 1).all() and (buf[at + 25] == 8).all() and (buf[at + 26] == 0).all()
    field = lambda o, n: buf[(at + o)[:, None] + np.arange(n)].copy().view("<u8").reshape(-1)
    table_id, version, key = field(16, 8), field(8, 8), field(27, 8)
    assert np.unique(np.stack([table_id, key], 1), axis=0).shape[0] == n0, "the keys are distinct"
    nq = 250000
    rec = np.random.default_rng(9).permutation(n0)[:nq // 2]
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
    assert (want["value_len"][h] == 64).all()
    twin = ramcrc.ReplayTableHost(3 * per, 2)
    for w in (w0, w1):
        twin.add(w.buf, w.cap, w.nseg, w.status, w.table)
    h_res, h_counts = twin.lookup(keys.view(np.uint8), q)
    twin.close()
    assert lc.same(h_res, want) and lc.counts_dict(h_counts) == lc.expected_counts(want)
    return [w0, w1], 3 * per, keys.view(np.uint8), q, want


def test_small_grids(ramcrc, grid_case):
    """250,000 queries, half hits and half misses, against the 249,165-record
    table (524,288 slots) at 1 and 3 CUs between two default-grid calls.

    The grid is capped at 8 workgroups of 256 lanes per CU.  At 1 CU that is 8
    workgroups, 2,048 lanes: k_rtab_lookup loops 123 times over the queries, the
    last pass with 144 lanes of one workgroup, and 8 workgroups meet at the
    counter line.  At 3 CUs, 24 workgroups and 6,144 lanes: 41 passes, the last
    with 4,240 queries.  At the default size (256 CUs) 977 workgroups take one
    tile each, the last one 144 queries."""
    ws, key_cap, kb, q, want = grid_case
    c = ramcrc.Context(0)
    t = None
    try:
        t = ramcrc.ReplayTable(c, key_cap, 2)
        for a in [tc.Added(w) for w in ws]:
            a.add(t)
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            r =lc.Looked(c, t, kb, q)
            assert lc.same(r.results, want), ("grid", ncu)
            assert r.counts == lc.expected_counts(want) and (r.past == FILL32).all()
            assert (r.count_past == FILL32).all()
    finally:
        if t is not None:
            t.close()
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_spoiled_tables(ramcrc, oracle_mod):
    """Spoiled by a bad segment number and by the key capacity: the pre-filled
    results stay untouched, the counts are {0, 0, 0, 0, 1}, the lookup raises
    no refusal of its own, and after the reset the table answers again."""
    c = ramcrc.Context(0)
    drv = lc.DeviceDriver(ramcrc, oracle_mod, c)
    keys = [(1, b"x"), (7, b"cap key 3"), (1, b"absent")]
    kb, q = segments.lookup_queries(keys)
    try:
        b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad.d_entries[2, 0] = 1   # = n_seg
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        for first, spoiler in ((b, bad), (full, more)):
            tab = drv.table(64, 4)
            try:
                tab.add(first)
                lc.lookup(tab, lc.checked_expectation(tab), keys, what="before")
                tc.Added(spoiler).add(tab.t)
                with pytest.raises(ramcrc.RamcrcError) as e:
                    c.check()
                assert e.value.code == ramcrc.EREFUSED
                r = lc.Looked(c, tab.t, kb, q)   # its check() passes: nothing is refused anew
                assert r.counts == lc.SPOILED_COUNTS and (r.count_past == FILL32).all()
                assert (r.results.view(np.uint32) == FILL32).all() and (r.past == FILL32).all()
                r = lc.Looked(c, tab.t, kb, q, want_counts=False)
                assert (r.results.view(np.uint32) == FILL32).all()
                tab.reset()
                tab.add(first)
                lc.lookup(tab, lc.checked_expectation(tab), keys, what="after the reset")
            finally:
                tab.close()
    finally:
        c.close()


# ---------------------------------------------------------------- the chain
def test_chain(ctx, ramcrc, drv):
    """verify -> two adds -> lookup -> the value bytes at {batch, segment,
    value_off, value_len} on the device: they are what the test wrote for the
    key's newest object."""
    rng = np.random.default_rng(41)
    newest, lists = {}, [[tc.head(1)], [tc.head(2)], [tc.head(3)], [tc.head(4)]]
    for n in range(120):
        key = (1 + n % 3, b"chain key %d" % n)
        for ver in rng.permutation(4)[:int(rng.integers(1, 4))].tolist():
            value = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            lists[int(rng.integers(0, 4))].append(rc.obj(key[0], key[1], ver, value))
            if key not in newest or ver > newest[key][0]:
                newest[key] = (ver, value)
    dead = (2, b"chain key 7")
    lists[3].append(rc.tomb(dead[0], dead[1], 9))
    ws = [drv.batch(lists[:2]), drv.batch(lists[2:])]
    t = ramcrc.ReplayTable(ctx, 1000, 2)
    try:
        for w in ws:
            crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
            ctx.verify_objects(w.d, w.cap, w.d_entries, w.d_n, crc, w.d_status.clone())
            tc.Added(w).add(t)
        keys = sorted(newest)
        kb, q = segments.lookup_queries(keys)
        r = lc.Looked(ctx, t, kb, q)
        n_obj = 0
        for key, res in zip(keys, r.results):
            if key == dead:
                assert res["kind"] == lc.TOMBSTONE and res["version"] == 9
                continue
            w = ws[int(res["batch"])]
            at = int(res["segment"]) * w.cap + int(res["value_off"])
            got = w.d[at:at + int(res["value_len"])].cpu().numpy().tobytes()
            assert res["kind"] == lc.OBJECT and (int(res["version"]), got) == newest[key], key
            n_obj += 1
        assert r.counts == dict(objects=n_obj, tombstones=1, absent=0, bad=0, spoiled=0) and n_obj == 119
    finally:
        t.close()


def test_bad_arguments(ctx, ramcrc):
    """Misaligned queries or results and missing arrays are EINVAL before any
    launch."""
    t = ramcrc.ReplayTable(ctx, 64, 1)
    try:
        z = torch.zeros(64, dtype=torch.uint8, device="cuda")
        for queries, results in ((z[4:28], z[32:]), (z[:24], z[40:]), (None, z[32:]), (z[:24], None)):
            with pytest.raises(ramcrc.RamcrcError) as e:
                lib_rc = ramcrc.lib().ramcrc_replay_table_lookup_device(
                    t._h, None, 0, None if queries is None else queries.data_ptr(), 1, None,
                    None if results is None else results.data_ptr(), None, None)
                ramcrc._check(lib_rc, "lookup")
            assert e.value.code == ramcrc.EINVAL
        ctx.check()
    finally:
        t.close()
