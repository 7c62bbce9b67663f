"""ramcrc_replay_table_migrate_host: a tablet migration's source side on the
host (MasterService::migrateTablet, src/MasterService.cc:1084-1225, over
migrateSingleLogEntry, :935-1073).  The expectation is the plain Python of
migrate_cases.py, held first against tests/golden/migrate_ref.json (what the
reference's tests state), then against the oracle's walk and certificate.  The
device tests (test_gpu_replay_table_migrate.py) run the same scenarios."""
import pytest

from ramcloud_amd import segments

import migrate_cases as mg
import partition_cases as pc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return mg.HostDriver(ramcrc, oracle_mod)


def test_dtypes_match_the_abi():
    assert segments.MIGRATE_COUNT_DTYPE.itemsize == 16 and segments.MIGRATE_SUMMARY_DTYPE.itemsize == 120
    assert segments.MIGRATE_SUMMARY_DTYPE.names == (
        "next_index", "next_record", "done", "too_large", "segments_used", "sent_objects", "sent_tombstones",
        "sent_bytes", "payload_bytes", "records_read", "skipped_other", "skipped_table", "skipped_range",
        "skipped_dead", "spoiled")


def test_migrate_entries_parses_a_segment():
    seg = pc.entry(pc.OBJ, b"a" * 300) + pc.entry(pc.OBJTOMB, b"b" * 40, length_bytes=2)
    assert segments.migrate_entries(seg + b"\xa5" * 8, len(seg)) == [(pc.OBJ, b"a" * 300), (pc.OBJTOMB, b"b" * 40)]
    with pytest.raises(ValueError):
        segments.migrate_entries(seg, len(seg) - 1)


def test_reference_fixture(drv):
    mg.check_fixture(drv, pc.load("migrate_ref.json"))


def test_counts(drv):
    mg.case_counts(drv)


def test_boundaries(drv):
    mg.case_boundaries(drv)


def test_entry_sizes(drv):
    mg.case_entry_sizes(drv)


def test_hash_range(drv):
    mg.case_hash_range(drv)


def test_liveness(drv):
    mg.case_liveness(drv)


def test_foreign_records(drv):
    mg.case_foreign(drv)


def test_cursor(drv):
    mg.case_cursor(drv)


def test_arguments(drv):
    mg.case_arguments(drv)


def test_spoiled(drv):
    mg.case_spoiled(drv)


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_chain(drv, seed):
    mg.case_chain(drv, seed)
