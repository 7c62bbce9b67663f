// The per-query rules of ramcrc_replay_table_lookup_device / _host
// (include/ramcrc.h), shared by the device kernel (dev_replay_table.inc) and
// the host form (ramcrc_host.cc): which queries are unusable, and where the
// value of a winning object lies (Object::getValueOffset / getValueLength,
// src/Object.cc:647-676).  Key identity, hashes, versions and winners are the
// table's (resolve_rules.h, partition_rules.h).  The callers differ only in
// how they read payload bytes.
#pragma once

#include <stdint.h>

#include "partition_rules.h"
#include "ramcrc.h"

namespace ramcrc_look {

constexpr uint32_t kMaxKeyLen = 65535;   // KeyLength is 16 bits (src/Key.h)
constexpr uint32_t kKeyCountAt = 24;     // Object: KeyCount behind the 24-byte header
constexpr uint32_t kNone = 0xFFFFFFFFu;

// Is the query unusable?  key_off + key_len is taken in 64 bits, overflow
// included: an offset past keys_bytes fails the first test, so the
// subtraction of the second cannot wrap.
RAMCRC_PART_HD bool bad_query(uint64_t key_off, uint32_t key_len, uint32_t reserved,
                              uint64_t keys_bytes)
{
    return key_len > kMaxKeyLen || reserved != 0 || key_off > keys_bytes ||
           keys_bytes - key_off < key_len;
}

struct Value {
    uint32_t off, len;   // from payload byte 0
};

// The value of an object whose payload has `len` bytes (a participant: len >=
// 25, and with keys the first key lies inside the payload).  The value begins
// behind the key count, the cumulative key lengths and the keys, whose total
// is the last cumulative length.  A key table or keys that run past the
// payload -- possible only with more than one key -- give no value: {len, 0},
// getValueLength() == 0 when fillKeyOffsets fails.  Only payload bytes are
// read.
template <typename Rd>
RAMCRC_PART_HD Value object_value(uint32_t len, const Rd& rd)
{
    const uint32_t nk = rd.u8(kKeyCountAt);
    uint32_t at = kKeyCountAt + 1;
    if (nk) {
        at += 2 * nk;
        if (at > len)
            return Value{len, 0u};
        at += rd.u16(at - 2);
        if (at > len)
            return Value{len, 0u};
    }
    return Value{at, len - at};
}

// The answer to a query nothing was found for (ABSENT, BAD_KEY).
RAMCRC_PART_HD ramcrc_lookup_result no_result(uint32_t kind)
{
    return ramcrc_lookup_result{ramcrc_replay_ref{kNone, kNone}, 0ull, kind, kNone, 0u, 0u};
}

}  // namespace ramcrc_look
