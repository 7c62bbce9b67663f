// The per-hash rules of ramcrc_replay_table_read_hashes_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_read_hashes.inc) and
// the host form (ramcrc_host.cc): the size of an object part
// (ObjectManager::readHashes, src/ObjectManager.cc:179-265), its 12 header
// bytes, the order of one hash's objects, the cut (:258-263) and what a hash
// adds to the summary.  The callers differ only in how they walk the chain and
// read the payload bytes.
#pragma once

#include <stdint.h>

#include "lookup_rules.h"
#include "ramcrc.h"

namespace ramcrc_rh {

constexpr uint32_t kPartHeader = 12;   // {u64 version, u32 length}, packed (:243-245)
constexpr uint32_t kObjHeader = 24;    // Object::Header: keys and value begin behind it

// The bytes behind the header: the payload [24, len) of a winning object (a
// participant: len >= 25), as appendKeysAndValueToBuffer writes them.
RAMCRC_PART_HD uint32_t data_len(uint32_t len)
{
    return len - kObjHeader;
}

// Bytes an object part takes in the reply.
RAMCRC_PART_HD uint64_t part_size(uint32_t len)
{
    return uint64_t(kPartHeader) + data_len(len);
}

// readKeyBytes of a part: keysAndValueLength - valueLength.
RAMCRC_PART_HD uint32_t key_bytes(uint32_t len, const ramcrc_look::Value& v)
{
    return len - kObjHeader - v.len;
}

// Byte b (0 .. 11) of a part's header.
RAMCRC_PART_HD uint8_t header_byte(uint64_t version, uint32_t length, uint32_t b)
{
    return b < 8 ? uint8_t(version >> (8 * b)) : uint8_t(length >> (8 * (b - 8)));
}

// The objects of one hash go in ascending order of this: the winner's batch,
// then its record (the pick's rank without the type bit).
RAMCRC_PART_HD uint64_t order_of(uint32_t batch, uint32_t record)
{
    return (uint64_t(batch) << 32) | record;
}

// Is a hash whose parts are [start, end) returned, given that every hash
// before it was?  The reference tests the length before the hash (:258), so
// the reply may pass max_length by one hash's parts; the reply buffer here
// does not grow, so the parts must also end within it.  Both tests are
// monotone in the hash's index: the returned hashes are a prefix.
RAMCRC_PART_HD bool returned(uint64_t start, uint64_t end, uint64_t max_length, uint64_t capacity)
{
    return start <= max_length && end <= capacity;
}

// A whole run of hashes that ends at `end` is returned when this holds: the
// last one of them begins at or before `end`.
RAMCRC_PART_HD bool run_returned(uint64_t end, uint64_t max_length, uint64_t capacity)
{
    return end <= max_length && end <= capacity;
}

// What one hash found on its chain.
struct Found {
    uint64_t bytes;        // of its parts
    uint64_t objects;      // matching keys whose winner is an object
    uint64_t tombstones;   // matching keys whose winner is a tombstone
    uint64_t value_bytes, key_bytes;
};

RAMCRC_PART_HD Found nothing()
{
    return Found{0ull, 0ull, 0ull, 0ull, 0ull};
}

// One more object, of payload length len with its value at v.
RAMCRC_PART_HD void add_object(Found* f, uint32_t len, const ramcrc_look::Value& v)
{
    f->bytes += part_size(len);
    f->objects++;
    f->value_bytes += v.len;
    f->key_bytes += key_bytes(len, v);
}

// A returned hash in the summary.
RAMCRC_PART_HD void count_returned(ramcrc_read_hashes_summary* s, const Found& f)
{
    s->hashes++;
    s->objects += f.objects;
    s->reply_bytes += f.bytes;
    s->value_bytes += f.value_bytes;
    s->key_bytes += f.key_bytes;
    s->tombstones += f.tombstones;
    s->empty += f.objects == 0;
}

}  // namespace ramcrc_rh
