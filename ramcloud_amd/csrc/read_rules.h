// The per-query rules of ramcrc_replay_table_read_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_replay_table.inc) and
// the host form (ramcrc_host.cc): the status of a part (readObject,
// src/ObjectManager.cc:324-369, and rejectOperation, :2893-2907), the bytes
// that follow its header in both modes (appendKeysAndValueToBuffer,
// src/Object.cc:279-291, or the value alone) and its size.  The lookup that
// comes first is lookup_rules.h's.  The callers differ only in how they read
// the rules and the payload bytes.
#pragma once

#include <stdint.h>

#include "lookup_rules.h"
#include "ramcrc.h"

namespace ramcrc_read {

// src/Status.h
constexpr uint32_t kStatusOk = 0;
constexpr uint32_t kStatusDoesntExist = 3;
constexpr uint32_t kStatusExists = 4;
constexpr uint32_t kStatusWrongVersion = 5;
constexpr uint32_t kStatusFormatError = 9;

constexpr uint32_t kPartHeader = 16;   // MultiOp::Response::ReadPart, packed
constexpr uint32_t kObjHeader = 24;    // Object::Header: keys and value begin behind it

// A query's RejectRules as two little-endian words: the given version, then
// doesnt_exist, exists, version_le_given, version_ne_given a byte each (any
// nonzero byte is set, as the reference tests them) and `reserved` above.
struct Rules {
    uint64_t given, bits;
};

RAMCRC_PART_HD Rules no_rules()
{
    return Rules{0ull, 0ull};
}

RAMCRC_PART_HD bool bad_rules(const Rules& r)
{
    return (r.bits >> 32) != 0;
}

// rejectOperation, in its order.
RAMCRC_PART_HD uint32_t reject(const Rules& r, uint64_t version)
{
    const bool doesnt_exist = (r.bits & 0xFFull) != 0, exists = (r.bits & 0xFF00ull) != 0;
    const bool le = (r.bits & 0xFF0000ull) != 0, ne = (r.bits & 0xFF000000ull) != 0;
    if (version == 0)   // VERSION_NONEXISTENT
        return doesnt_exist ? kStatusDoesntExist : kStatusOk;
    if (exists)
        return kStatusExists;
    if (le && version <= r.given)
        return kStatusWrongVersion;
    if (ne && version != r.given)
        return kStatusWrongVersion;
    return kStatusOk;
}

// The status of the part that answers a lookup of `kind`; *version is the
// lookup's on entry and the part's on return.  `bad`: the query or its rules
// are unusable.
RAMCRC_PART_HD uint32_t status(bool bad, uint32_t kind, const Rules& r, uint64_t* version)
{
    if (bad || kind == RAMCRC_LOOKUP_BAD_KEY) {
        *version = 0;
        return kStatusFormatError;
    }
    if (kind != RAMCRC_LOOKUP_OBJECT) {   // absent or a tombstone: before any rule
        *version = 0;
        return kStatusDoesntExist;
    }
    return reject(r, *version);
}

struct Data {
    uint32_t off, len;   // from payload byte 0
};

// The bytes behind the header of a STATUS_OK part: of a winning object whose
// payload has `len` bytes (a participant: len >= 25) and whose value lies at
// `v` (lookup_rules.h's object_value).
RAMCRC_PART_HD Data data_range(uint32_t flags, uint32_t len, const ramcrc_look::Value& v)
{
    if (flags & RAMCRC_READ_VALUE_ONLY)
        return Data{v.off, v.len};
    return Data{kObjHeader, len - kObjHeader};
}

// Bytes a part takes in the reply.
RAMCRC_PART_HD uint64_t part_size(uint32_t status, uint32_t data_len)
{
    return uint64_t(kPartHeader) + (status == kStatusOk ? data_len : 0u);
}

// readKeyBytes of an OK part: keysAndValueLength - valueLength.
RAMCRC_PART_HD uint32_t key_bytes(uint32_t len, const ramcrc_look::Value& v)
{
    return len - kObjHeader - v.len;
}

// The 16 header bytes as two little-endian words.
RAMCRC_PART_HD void header_words(uint32_t status, uint64_t version, uint32_t length, uint64_t* w0,
                                 uint64_t* w1)
{
    *w0 = uint64_t(status) | (version << 32);
    *w1 = (version >> 32) | (uint64_t(length) << 32);
}

}  // namespace ramcrc_read
