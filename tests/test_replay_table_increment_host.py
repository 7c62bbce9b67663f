"""ramcrc_replay_table_increment_host: a multi-increment against the replay
table on the host, the loop of MasterService::multiIncrement
(src/MasterService.cc:1277-1330) over incrementObject (:678-790).  The
expectation is the plain Python of increment_cases.py, held against
tests/golden/multi_increment_ref.json and, through lookup_cases.py, against the
live query's winners before a call is held against it; every call a write can
express is also held against the merged ramcrc_replay_table_write_host.  The
device tests (test_gpu_replay_table_increment.py) run the same scenarios."""
import numpy as np
import pytest

from ramcloud_amd import segments

import increment_cases as ic
import lookup_cases as lc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return ic.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_match_the_abi():
    assert segments.INCREMENT_ARG_DTYPE.itemsize == 16 and segments.INCREMENT_PART_DTYPE.itemsize == 20
    assert segments.INCREMENT_SUMMARY_DTYPE.itemsize == 144
    assert segments.INCREMENT_SUMMARY_DTYPE.names == (
        "ok", "created", "doesnt_exist", "object_exists", "wrong_version", "invalid_object", "bad",
        "retry_duplicate", "retry_full", "tombstones", "allocated", "next_version", "out_bytes", "object_bytes",
        "tombstone_bytes", "value_bytes", "key_bytes", "spoiled")
    assert segments.STATUS_INVALID_OBJECT == 22


def test_increment_args_and_parts():
    a = segments.increment_args([(-1, 1.5), ((1 << 64) - 2, -0.0), (1 << 63, 0x7FF8000000000001), (0, 0)])
    assert a["add_int64"].tolist() == [-1, -2, -(1 << 63), 0]
    assert a["add_double_bits"].tolist() == [0x3FF8000000000000, 1 << 63, 0x7FF8000000000001, 0]
    raw = np.zeros(2, segments.INCREMENT_PART_DTYPE)
    raw[0], raw[1] = (0, 7, 42), (22, 3, 0x3FF8000000000000)
    p = segments.multi_increment_parts(raw.tobytes() + b"\xA5" * 7)
    assert [tuple(int(x) for x in r) for r in p] == [(0, 7, 42), (22, 3, 0x3FF8000000000000)]
    assert p["value_bits"].view("<f8")[1] == 1.5
    with pytest.raises(ValueError):
        segments.multi_increment_parts(raw.tobytes(), 3)


def test_the_expectation_matches_the_goldens(oracle_mod):
    ref = ic.golden()
    assert ic.check_expectation_against_golden(oracle_mod, ref) == ref["steps"] == 14
    assert [s["name"] for s in ref["scenarios"]] == [
        "increment_basic", "increment_create", "increment_rejectRules", "increment_invalidObject",
        "multiIncrement_basics", "multiIncrement_rejectRules"]


def test_goldens(drv):
    ic.case_goldens(drv)


def test_closing_the_loop(drv):
    ic.case_closing_the_loop(drv)


def test_the_sum(drv):
    ic.case_sum(drv)


def test_reject_rules(drv):
    ic.case_reject_rules(drv)


def test_invalid_object(drv):
    ic.case_invalid_object(drv)


def test_duplicates(drv):
    ic.case_duplicates(drv)


def test_key_lengths(drv):
    ic.case_key_lengths(drv)


def test_value_alignment(drv):
    ic.case_value_alignment(drv)


def test_alignment(drv):
    ic.case_alignment(drv)


def test_space(drv):
    ic.case_space(drv)


def test_counts(drv):
    ic.case_counts(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    ic.case_bad_requests(drv)


def test_nullable_arguments(drv):
    ic.case_nullable(drv)


def test_bad_arguments(drv):
    ic.case_host_einval(drv)


def test_a_spoiled_table(drv):
    ic.case_spoiled(drv)


def test_the_large_case_at_a_hundredth(drv):
    ic.case_large_on_the_host(drv)


def test_read_only(drv, mixed):
    ic.case_read_only(drv, mixed)
