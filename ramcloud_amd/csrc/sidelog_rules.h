// The per-record rules of ramcrc_replay_sidelog_device / _host
// (include/ramcrc.h), shared by the device kernel (dev_sidelog.inc) and the
// host form (ramcrc_host.cc): which appended records are rewritten, which
// bytes of a kept tombstone change (ObjectManager::replaySegment,
// src/ObjectManager.cc:845-851) and which bytes its checksum covers
// (ObjectTombstone::computeChecksum, src/Object.cc:1042-1057).
#pragma once

#include <stdint.h>

#include "partition_rules.h"
#include "ramcrc.h"

namespace ramcrc_sl {

// ObjectTombstone::Header (src/Object.h:285-338): tableId, segmentId,
// objectVersion, timestamp, checksum; the key follows.
constexpr uint32_t kTombHeaderBytes = 32;
constexpr uint32_t kSegmentIdAt = 8, kSegmentIdBytes = 8;
constexpr uint32_t kTimestampAt = 24;
constexpr uint32_t kChecksumAt = 28;   // the checksum covers [0, 28) and [32, length)

enum Kind : uint32_t { kObject = 0, kTombstone = 1, kShortTombstone = 2, kOther = 3 };

// What the side log does with an appended record of `type` and payload
// `length`: only kTombstone is rewritten, everything else is copied.
RAMCRC_PART_HD Kind kind(uint32_t type, uint32_t length)
{
    if (type == RAMCRC_LOG_ENTRY_TYPE_OBJ)
        return kObject;
    if (type == RAMCRC_LOG_ENTRY_TYPE_OBJTOMB)
        return length >= kTombHeaderBytes ? kTombstone : kShortTombstone;
    return kOther;
}

// Byte m of the checksummed message (m < length - 4) is payload byte at(m).
RAMCRC_PART_HD uint32_t at(uint32_t m) { return m < kChecksumAt ? m : m + 4; }

// Is payload byte b (b < kChecksumAt) one the rewrite replaces, and by what?
RAMCRC_PART_HD bool stamped(uint32_t b, uint32_t timestamp, uint32_t& value)
{
    if (b >= kSegmentIdAt && b < kSegmentIdAt + kSegmentIdBytes) {
        value = 0;
        return true;
    }
    if (b >= kTimestampAt && b < kTimestampAt + 4) {
        value = (timestamp >> (8 * (b - kTimestampAt))) & 0xFFu;
        return true;
    }
    return false;
}

}  // namespace ramcrc_sl
