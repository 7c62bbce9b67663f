// The per-record rules of ramcrc_recovery_partition_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_partition.inc) and the
// host form (ramcrc_host.cc): which fields of a record RecoverySegmentBuilder::
// build reads (src/RecoverySegmentBuilder.cc:74-201), whichPartition
// (:330-343) and isEntryAlive (:300-307).  The callers differ only in how they
// read payload bytes and tablets.
#pragma once

#include <stdint.h>

#include "ramcrc.h"

#if defined(__HIPCC__)
#define RAMCRC_PART_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RAMCRC_PART_HD inline
#endif

namespace ramcrc_part {

constexpr uint32_t kNoTablet = 0xFFFFFFFFu;
constexpr uint32_t kSegHeaderBytes = 20;   // through SegmentHeader::capacity (src/LogMetadata.h:51-61)
constexpr uint32_t kSegIdAt = 8;
constexpr uint32_t kPartyBytes = 24;       // WireFormat::TxParticipant {tableId, keyHash, rpcId}
constexpr uint32_t kPlistHeader = 24;      // ParticipantList::Header (src/ParticipantList.h:81-112)
constexpr uint32_t kPlistCountAt = 16;

enum Kind : uint32_t {
    kIgnored = 0,      // a type build skips
    kSafeVersion,      // every partition
    kPlist,            // one placement per owned participant
    kKeyed,            // the key [key_off, key_off + key_len) is hashed
    kStored,           // the record stores its hash
    kMalformed
};

struct Parsed {
    uint32_t kind;
    uint32_t key_off, key_len;   // kKeyed
    uint32_t count;              // kPlist: participants
    uint64_t table_id;           // kKeyed, kStored
    uint64_t hash;               // kStored
};

// Is `type` one build places (src/RecoverySegmentBuilder.cc:82-89)?
RAMCRC_PART_HD bool placed_type(uint32_t type)
{
    return type == RAMCRC_LOG_ENTRY_TYPE_OBJ || type == RAMCRC_LOG_ENTRY_TYPE_OBJTOMB ||
           type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION || type == RAMCRC_LOG_ENTRY_TYPE_RPCRESULT ||
           type == RAMCRC_LOG_ENTRY_TYPE_PREP || type == RAMCRC_LOG_ENTRY_TYPE_PREPTOMB ||
           type == RAMCRC_LOG_ENTRY_TYPE_TXDECISION || type == RAMCRC_LOG_ENTRY_TYPE_TXPLIST;
}

// The fields of a record of `type` with `len` payload bytes; rd.u8/u16/u32/u64(o)
// read little-endian at payload byte o and are called only for bytes inside
// the payload.  `readable`: the payload lies inside its segment.
template <typename Rd>
RAMCRC_PART_HD Parsed parse(uint32_t type, uint32_t len, bool readable, const Rd& rd)
{
    Parsed p{kIgnored, 0u, 0u, 0u, 0ull, 0ull};
    if (!placed_type(type))
        return p;
    p.kind = kMalformed;
    if (!readable)
        return p;
    if (type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION) {
        p.kind = kSafeVersion;
    } else if (type == RAMCRC_LOG_ENTRY_TYPE_TXPLIST) {
        if (len < kPlistHeader)
            return p;
        p.count = rd.u32(kPlistCountAt);
        if (uint64_t(kPlistHeader) + uint64_t(kPartyBytes) * p.count > len)
            return p;
        p.kind = kPlist;
    } else if (type == RAMCRC_LOG_ENTRY_TYPE_OBJ || type == RAMCRC_LOG_ENTRY_TYPE_PREP) {
        // Object::Header is 24 bytes, tableId its last 8; then KeyCount and the
        // CumulativeKeyLength array; PreparedOp::Header is 32 bytes before it
        const uint32_t o = type == RAMCRC_LOG_ENTRY_TYPE_PREP ? 32u : 0u;
        if (len < o + 25)
            return p;
        p.table_id = rd.u64(o + 16);
        const uint32_t nk = rd.u8(o + 24);
        if (nk) {
            if (len < o + 27)
                return p;
            p.key_len = rd.u16(o + 25);
            p.key_off = o + 25 + 2 * nk;
            if (uint64_t(p.key_off) + p.key_len > len)
                return p;
        }
        p.kind = kKeyed;
    } else if (type == RAMCRC_LOG_ENTRY_TYPE_OBJTOMB) {
        if (len < 32)
            return p;
        p.table_id = rd.u64(0);
        p.key_off = 32;
        p.key_len = len - 32;
        p.kind = kKeyed;
    } else {   // RPCRESULT, PREPTOMB, TXDECISION
        if (len < 16)
            return p;
        p.table_id = rd.u64(0);
        p.hash = rd.u64(8);
        p.kind = kStored;
    }
    return p;
}

// whichPartition: the first tablet in list order that holds (table_id, hash);
// tab(i) returns tablet i.
template <typename Tab>
RAMCRC_PART_HD uint32_t which_tablet(uint64_t table_id, uint64_t hash, uint32_t n_tablets,
                                     const Tab& tab)
{
    for (uint32_t i = 0; i < n_tablets; i++) {
        const ramcrc_tablet t = tab(i);
        if (t.table_id == table_id && t.start_key_hash <= hash && t.end_key_hash >= hash)
            return i;
    }
    return kNoTablet;
}

// isEntryAlive: LogPosition's order, segment id first, then offset.
RAMCRC_PART_HD bool alive(uint64_t seg_id, uint32_t offset, const ramcrc_tablet& t)
{
    return seg_id > t.ctime_segment_id || (seg_id == t.ctime_segment_id && offset >= t.ctime_offset);
}

}  // namespace ramcrc_part
