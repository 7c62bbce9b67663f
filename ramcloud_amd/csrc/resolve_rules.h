// The per-record rules of ramcrc_replay_resolve_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_resolve.inc) and the
// host form (ramcrc_host.cc): which records take part, where their version
// lies, which of two records of one key replay keeps
// (ObjectManager::replaySegment, src/ObjectManager.cc:671-734, :766-867), and
// the size of the grouping table.  The record's key fields are
// partition_rules.h's (ramcrc_part::parse).  The callers differ only in how
// they read payload bytes.
#pragma once

#include <stdint.h>

#include "partition_rules.h"
#include "ramcrc.h"

namespace ramcrc_res {

constexpr uint32_t kObjVersionAt = 8;       // Object::Header::version (src/Object.h:171)
constexpr uint32_t kTombVersionAt = 16;     // ObjectTombstone::Header::objectVersion (:324)
constexpr uint32_t kSafeVersionBytes = 12;  // ObjectSafeVersion::Header (:402-427)
constexpr uint64_t kMinSlots = 64;

// Is `type` one whose fate replay decides by key and version?
RAMCRC_PART_HD bool resolved_type(uint32_t type)
{
    return type == RAMCRC_LOG_ENTRY_TYPE_OBJ || type == RAMCRC_LOG_ENTRY_TYPE_OBJTOMB;
}

// The version of a participant (a record ramcrc_part::parse calls kKeyed, so
// the bytes are inside its payload).
template <typename Rd>
RAMCRC_PART_HD uint64_t version(uint32_t type, const Rd& rd)
{
    return rd.u64(type == RAMCRC_LOG_ENTRY_TYPE_OBJ ? kObjVersionAt : kTombVersionAt);
}

// Among records of one key and one version the lowest rank is kept: a
// tombstone before an object (:693 discards an object at <=, :786 a tombstone
// only at <), then the lowest record index.
RAMCRC_PART_HD uint64_t rank(uint32_t type, uint64_t index)
{
    return (uint64_t(type == RAMCRC_LOG_ENTRY_TYPE_OBJ) << 32) | index;
}

// Does the record (va, ra) replace (vb, rb) as its key's winner?  Versions
// compare unsigned over all 64 bits.
RAMCRC_PART_HD bool beats(uint64_t va, uint64_t ra, uint64_t vb, uint64_t rb)
{
    return va > vb || (va == vb && ra < rb);
}

// Slots of the open-addressed grouping table for n records: a power of two,
// load at most 0.5.
RAMCRC_PART_HD uint64_t slots_for(uint64_t n)
{
    uint64_t s = kMinSlots;
    while (s < 2 * n)
        s <<= 1;
    return s;
}

}  // namespace ramcrc_res
