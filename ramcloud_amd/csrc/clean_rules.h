// The per-record rules of ramcrc_replay_table_clean_device / _host and of
// their clean_size forms (include/ramcrc.h), shared by the device kernels
// (dev_clean.inc) and the host form (ramcrc_host.cc): which records of a
// victim batch are live (ObjectManager::relocateObject's test,
// src/ObjectManager.cc:2953-2968, and the hashReferenceExists half of
// relocateTombstone, :3187-3203), what a record takes in the survivor segment,
// how the others are counted, whether the survivors fit, and what a moved
// winner's pick and a re-pointed claim become.  Rules marked "ours" are
// decisions the batch form has to make and the reference does not.  The
// callers differ only in how they reach the slot words.
#pragma once

#include <stdint.h>

#include "resolve_rules.h"

namespace ramcrc_clean {

constexpr uint64_t kNoSlot = ~0ull;   // a work word: the record took no part in its add

// The rank a pick stands for: is_object << 48 | batch << 32 | record.
RAMCRC_PART_HD uint64_t rank_of(bool is_object, uint32_t batch, uint64_t record)
{
    return (uint64_t(is_object) << 48) | (uint64_t(batch) << 32) | record;
}

RAMCRC_PART_HD uint32_t rank_batch(uint64_t rank) { return uint32_t(rank >> 32) & 0xFFFFu; }
RAMCRC_PART_HD uint32_t rank_record(uint64_t rank) { return uint32_t(rank); }

// Live: the record took part in its add and its slot's winner names it.  Ours:
// this is the whole test for a tombstone too -- one that is not its key's
// winner is dropped whether or not the segment it names still exists (the
// reference keeps it while log.segmentExists, :3184, because its hash table
// holds no tombstones; here the key's winner stays in the table).
RAMCRC_PART_HD bool live(uint64_t work, uint64_t winner_rank, uint32_t batch, uint64_t record)
{
    return work != kNoSlot && rank_batch(winner_rank) == batch && rank_record(winner_rank) == record;
}

// What a record is to the summary.
enum Class : uint32_t {
    kLiveObject = 0,
    kLiveTombstone = 1,
    kDroppedObject = 2,      // a participant that is not its key's winner
    kDroppedTombstone = 3,
    kDroppedOther = 4,       // never took part: other types, malformed, records of a segment
                             // without RAMCRC_SEG_OK (ours: RpcResult and transaction records
                             // are not relocated)
};

RAMCRC_PART_HD Class classify(uint64_t work, uint64_t winner_rank, uint32_t batch, uint64_t record,
                              uint32_t header)
{
    if (work == kNoSlot)
        return kDroppedOther;
    const bool obj = (header & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ;
    if (live(work, winner_rank, batch, record))
        return obj ? kLiveObject : kLiveTombstone;
    return obj ? kDroppedObject : kDroppedTombstone;
}

// An entry's metadata bytes (the header byte and the length bytes as the source
// has them) and all its bytes: the survivor is the source's entry byte for byte.
RAMCRC_PART_HD uint32_t meta_bytes(uint32_t header) { return 1 + ((header >> 6) & 3) + 1; }
RAMCRC_PART_HD uint64_t entry_bytes(uint32_t header, uint32_t length)
{
    return uint64_t(meta_bytes(header)) + length;
}

// Metadata byte b of an entry.
RAMCRC_PART_HD uint32_t meta_byte(uint32_t header, uint32_t length, uint32_t b)
{
    return b == 0 ? (header & 0xFFu) : (length >> (8 * (b - 1))) & 0xFFu;
}

// Ours: all survivors go to one segment and one record table, or none does.
RAMCRC_PART_HD bool fits(uint64_t needed_bytes, uint64_t needed_records, uint64_t out_capacity,
                         uint64_t out_entries_cap)
{
    return needed_bytes <= out_capacity && needed_records <= out_entries_cap;
}

// The claim that names record {batch, record}.
RAMCRC_PART_HD uint64_t claim_of(uint32_t batch, uint64_t record)
{
    return (uint64_t(batch) << 32) | (record + 1);
}

RAMCRC_PART_HD uint32_t claim_batch(uint64_t claim) { return uint32_t(claim >> 32); }
RAMCRC_PART_HD uint64_t claim_record(uint64_t claim) { return (claim & 0xFFFFFFFFull) - 1; }

// Ours: a claim that named a victim's record names the key's winner after the
// call -- a participant of the same key, which lies in the survivor batch or
// in a batch that stays.
RAMCRC_PART_HD uint64_t claim_after(uint64_t winner_rank_after)
{
    return claim_of(rank_batch(winner_rank_after), rank_record(winner_rank_after));
}

}  // namespace ramcrc_clean
