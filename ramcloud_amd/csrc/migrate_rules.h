// The per-record rules of ramcrc_replay_table_migrate_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_migrate.inc) and the
// host form (ramcrc_host.cc): which records of a listed batch a tablet
// migration sends (MasterService::migrateSingleLogEntry,
// src/MasterService.cc:935-1073), what a sent record takes in a transfer
// segment, when a segment is closed, and how the records that are not sent are
// counted.  Rules marked "ours" are decisions the batch form has to make and
// the reference does not.  The callers differ only in how they reach the slot
// words and the record's key.
#pragma once

#include <stdint.h>

#include "clean_rules.h"
#include "write_rules.h"

namespace ramcrc_mig {

constexpr uint32_t kKnownFlags = RAMCRC_MIGRATE_LIVE_ONLY;

// What a record is to the call.  The tests are made in this order, and the
// first that fails names the class.
enum Class : uint32_t {
    kNotRead = 0,        // before the start cursor or behind the batch's records
    kSentObject = 1,
    kSentTombstone = 2,
    kSkippedOther = 3,   // never took part in its add: other types (ours: RpcResult and the
                         // transaction records stay with the master), malformed and overlong
                         // records, records of a segment without RAMCRC_SEG_OK
    kSkippedTable = 4,   // some bit of the 64-bit table id differs (:966-969)
    kSkippedRange = 5,   // the record hash lies outside [first_hash, last_hash] (:971-974)
    kSkippedDead = 6,    // live-only mode (ours): not its key's winner now
};

// The selection.  `participant`: the record's work word names a slot;
// `winner`: clean's rule 2 for this record (only asked in live-only mode).
RAMCRC_PART_HD Class classify(bool participant, uint32_t header, uint64_t record_table, uint64_t table_id,
                              uint64_t hash, uint64_t first_hash, uint64_t last_hash, uint32_t flags,
                              bool winner)
{
    if (!participant)
        return kSkippedOther;
    if (record_table != table_id)
        return kSkippedTable;
    if (hash < first_hash || hash > last_hash)
        return kSkippedRange;
    if ((flags & RAMCRC_MIGRATE_LIVE_ONLY) && !winner)
        return kSkippedDead;
    return (header & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ ? kSentObject : kSentTombstone;
}

RAMCRC_PART_HD bool sent(uint32_t k) { return k == kSentObject || k == kSentTombstone; }

// A sent entry: Segment::append(type, payload, length) builds a fresh
// EntryHeader, so the length bytes are the minimal ones whatever the source
// had.
RAMCRC_PART_HD uint32_t meta_bytes(uint32_t length) { return 1 + ramcrc_write::len_bytes(length); }
RAMCRC_PART_HD uint64_t entry_bytes(uint32_t length) { return uint64_t(meta_bytes(length)) + length; }

// Metadata byte b of a sent entry of `type`.
RAMCRC_PART_HD uint32_t meta_byte(uint32_t type, uint32_t length, uint32_t b)
{
    return b == 0 ? ((type & 0x3f) | ((ramcrc_write::len_bytes(length) - 1) << 6))
                  : (length >> (8 * (b - 1))) & 0xFFu;
}

// The scratch word of a record: its class and, for a sent one, its payload
// length.  A length above kLenMask is kept as kLenMask + 1: such an entry fits
// no output (out_capacity <= RAMCRC_MIGRATE_MAX_CAPACITY).
constexpr uint32_t kClassShift = 29;
constexpr uint32_t kLenMask = (1u << kClassShift) - 1;
static_assert(RAMCRC_MIGRATE_MAX_CAPACITY <= kLenMask, "a kept length decides whether the entry fits");

RAMCRC_PART_HD uint32_t pack(uint32_t k, uint32_t length)
{
    return (k << kClassShift) | (sent(k) ? (length > kLenMask ? kLenMask : length) : 0u);
}
RAMCRC_PART_HD uint32_t packed_class(uint32_t w) { return w >> kClassShift; }
RAMCRC_PART_HD uint32_t packed_length(uint32_t w) { return w & kLenMask; }

// Does an entry never fit, not even an empty output (:1061-1065)?
RAMCRC_PART_HD bool too_large(uint64_t entry, uint64_t out_capacity) { return entry > out_capacity; }

// The greedy cut: does an entry of `entry` bytes close a segment whose head is
// `head` (:1047-1049, Segment::append's failure)?
RAMCRC_PART_HD bool closes(uint64_t head, uint64_t entry, uint64_t out_capacity)
{
    return head + entry > out_capacity;
}

}  // namespace ramcrc_mig
