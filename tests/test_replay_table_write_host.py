"""ramcrc_replay_table_write_host: a multi-write against the replay table on
the host, the loop of MasterService::multiWrite (src/MasterService.cc:1523-1601)
over ObjectManager::writeObject (src/ObjectManager.cc:1181-1350).  The
expectation is the plain Python of write_cases.py, held against
tests/golden/multi_write_ref.json and, through lookup_cases.py, against the
live query's winners before a call is held against it.  The device tests
(test_gpu_replay_table_write.py) run the same scenarios."""
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import write_cases as wc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return wc.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_and_helpers_match_the_abi():
    assert segments.WRITE_REQ_DTYPE.itemsize == 24 and segments.WRITE_PART_DTYPE.itemsize == 12
    assert segments.WRITE_REF_DTYPE.itemsize == 8 and segments.WRITE_SUMMARY_DTYPE.itemsize == 128
    assert segments.WRITE_SUMMARY_DTYPE.names == (
        "ok", "doesnt_exist", "object_exists", "wrong_version", "bad", "retry_duplicate", "retry_full",
        "tombstones", "allocated", "next_version", "out_bytes", "value_bytes", "key_bytes", "object_bytes",
        "tombstone_bytes", "spoiled")
    assert segments.keys_and_value([b"ab", b"c"], b"xyz") == b"\x02\x02\x00\x03\x00abcxyz"
    assert segments.keys_and_value([], b"v") == b"\x00v"
    data, reqs = segments.write_requests([(7, b"k", b"value"), ((1 << 63) + 1, [b"a", b"bc"], b"")], align=16)
    assert data.tobytes() == b"\x01\x01\x00kvalue" + bytes(7) + b"\x02\x01\x00\x03\x00abc"
    assert [tuple(int(x) for x in r) for r in reqs] == [(7, 0, 9, 0), ((1 << 63) + 1, 16, 8, 0)]


def test_the_expectation_matches_the_goldens(oracle_mod):
    ref = wc.golden()
    assert wc.check_expectation_against_golden(oracle_mod, ref) == ref["steps"] == 13
    assert [s["name"] for s in ref["scenarios"]] == ["writeObject", "multiWrite_basics", "multiWrite_rejectRules",
                                                     "write_basics", "write_safeVersionNumberUpdate"]


def test_goldens(drv):
    wc.case_goldens(drv)


def test_closing_the_loop(drv, mixed):
    wc.case_closing_the_loop(drv, mixed)


def test_reject_rules(drv):
    wc.case_reject_rules(drv)


def test_versions(drv):
    wc.case_versions(drv)


def test_duplicates(drv):
    wc.case_duplicates(drv)


def test_entry_sizes(drv):
    wc.case_sizes(drv)


def test_alignment(drv):
    wc.case_alignment(drv)


def test_multi_key_objects(drv):
    wc.case_multi_key(drv)


def test_space(drv):
    wc.case_space(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    wc.case_bad_requests(drv)


def test_nullable_and_empty_arguments(drv):
    wc.case_nullable_and_empty(drv)


def test_a_spoiled_table(drv):
    wc.case_spoiled(drv)


def test_read_only(drv, mixed):
    wc.case_read_only(drv, mixed)
