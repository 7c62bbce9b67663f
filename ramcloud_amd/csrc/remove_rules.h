// The per-request rules of ramcrc_replay_table_remove_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_remove.inc) and the
// host form (ramcrc_host.cc): which requests are usable, what a request's
// lookup and its RejectRules make of it (ObjectManager::removeObject,
// src/ObjectManager.cc:405-491), the tombstone's entry and the caller's safe
// version after the call.  The lookup, rejectOperation and the entry's sizes
// and header bytes are lookup_rules.h's, read_rules.h's and write_rules.h's,
// unchanged.  The callers differ only in how they read the key bytes.
#pragma once

#include <stdint.h>

#include "write_rules.h"

namespace ramcrc_remove {

using ramcrc_write::kNone;
using ramcrc_write::kStatusRetry;
using ramcrc_write::kTombHeader;

constexpr uint32_t kPartBytes = 12;   // MultiOp::Response::RemovePart, packed

// The tests of a request that read neither the key buffer nor the table: the
// lookup's own, and the rules' reserved word.
RAMCRC_PART_HD bool bad_request(uint64_t key_off, uint32_t key_len, uint32_t reserved, bool bad_rules,
                                uint64_t keys_bytes)
{
    return bad_rules || ramcrc_look::bad_query(key_off, key_len, reserved, keys_bytes);
}

// What becomes of the first usable request of its key, before the space check.
struct Outcome {
    uint32_t status;    // of a request that does not reach the tombstone
    uint64_t version;   // the part's: the object's, 0 without one
    bool reach;         // goes on to the tombstone (status is STATUS_OK)
};

// `kind` and `version`: the key's winner as the lookup returns it.  Only an
// object is found (:430-436: the entry's type, not its version); absent and a
// tombstone are VERSION_NONEXISTENT to rejectOperation (:437-441).
RAMCRC_PART_HD Outcome outcome(uint32_t kind, uint64_t version, const ramcrc_read::Rules& r)
{
    if (kind != RAMCRC_LOOKUP_OBJECT)
        return Outcome{ramcrc_read::reject(r, 0), 0ull, false};
    const uint32_t st = ramcrc_read::reject(r, version);
    return Outcome{st, version, st == ramcrc_read::kStatusOk};
}

// Bytes the tombstone of a key of key_len bytes takes in the segment, its
// payload, and its metadata bytes.
RAMCRC_PART_HD uint32_t tomb_len(uint32_t key_len)
{
    return kTombHeader + key_len;
}

RAMCRC_PART_HD uint64_t tomb_size(uint32_t key_len)
{
    return ramcrc_write::entry_size(tomb_len(key_len));
}

RAMCRC_PART_HD uint32_t tomb_meta(uint32_t key_len)
{
    return 1 + ramcrc_write::len_bytes(tomb_len(key_len));
}

// The safe version after the call (:487): top is the highest version among
// the written tombstones, 0 without one.  uint64_t arithmetic: a version of
// 2^64 - 1 leaves next_version as it was.
RAMCRC_PART_HD uint64_t next_version(uint64_t next_version_in, uint64_t top)
{
    return top + 1 > next_version_in ? top + 1 : next_version_in;
}

}  // namespace ramcrc_remove
