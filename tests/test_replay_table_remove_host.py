"""ramcrc_replay_table_remove_host: a multi-remove against the replay table on
the host, the loop of MasterService::multiRemove (src/MasterService.cc:1435-1505)
over ObjectManager::removeObject (src/ObjectManager.cc:405-491).  The
expectation is the plain Python of remove_cases.py, held against
tests/golden/multi_remove_ref.json and, through lookup_cases.py, against the
live query's winners before a call is held against it.  The device tests
(test_gpu_replay_table_remove.py) run the same scenarios."""
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import remove_cases as rm


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return rm.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_match_the_abi():
    assert segments.REMOVE_PART_DTYPE.itemsize == 12 and segments.REMOVE_SUMMARY_DTYPE.itemsize == 96
    assert segments.REMOVE_SUMMARY_DTYPE.names == (
        "removed", "ok_absent", "doesnt_exist", "object_exists", "wrong_version", "bad", "retry_duplicate",
        "retry_full", "next_version", "out_bytes", "tombstone_bytes", "spoiled")
    assert segments.REMOVE_REF_NONE == 0xFFFFFFFF


def test_the_expectation_matches_the_goldens(oracle_mod):
    ref = rm.golden()
    assert rm.check_expectation_against_golden(oracle_mod, ref) == ref["steps"] == 13
    assert [s["name"] for s in ref["scenarios"]] == [
        "removeObject", "removeObject_returnRemovedObj", "multiRemove_basics", "multiRemove_rejectRules",
        "remove_rejectRules", "remove_objectAlreadyDeletedRejectRules", "remove_objectAlreadyDeleted"]


def test_goldens(drv):
    rm.case_goldens(drv)


def test_closing_the_loop(drv, mixed):
    rm.case_closing_the_loop(drv, mixed)


def test_reject_rules(drv):
    rm.case_reject_rules(drv)


def test_version_zero(drv):
    rm.case_version_zero(drv)


def test_duplicates(drv):
    rm.case_duplicates(drv)


def test_key_lengths(drv):
    rm.case_key_lengths(drv)


def test_alignment(drv):
    rm.case_alignment(drv)


def test_space(drv):
    rm.case_space(drv)


def test_counts(drv):
    rm.case_counts(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    rm.case_bad_requests(drv)


def test_nullable_arguments(drv):
    rm.case_nullable(drv)


def test_a_spoiled_table(drv):
    rm.case_spoiled(drv)


def test_read_only(drv, mixed):
    rm.case_read_only(drv, mixed)
