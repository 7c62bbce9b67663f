// The rules of ramcrc_replay_table_enumerate_device / _host (include/ramcrc.h),
// shared by the device kernels (dev_enumerate.inc) and the host form
// (ramcrc_host.cc): a key's bucket (HashTable::findBucketIndex,
// src/HashTable.cc:489-495), which keys a call selects
// (Enumeration.cc's enumerateBucket, src/Enumeration.cc:58-108), an entry's
// length and size (appendObjectsToBuffer, :128-154), the order of a bucket's
// entries and the cut of the bucket the call began in (:318-332).  The callers
// differ only in how they walk the chain and read the payload bytes.
#pragma once

#include <stdint.h>

#include "lookup_rules.h"
#include "ramcrc.h"

namespace ramcrc_en {

constexpr uint32_t kLengthBytes = 4;              // an entry's u32 length
constexpr uint64_t kBucketHashBits = 0xffffffffffffull;   // findBucketIndex uses the low 48 bits

// The bucket of hash h in a table of `buckets` (a power of two).
RAMCRC_PART_HD uint64_t bucket_of(uint64_t h, uint64_t buckets)
{
    return (h & kBucketHashBits) & (buckets - 1);
}

// Is a stale frame usable?
RAMCRC_PART_HD bool bad_frame(const ramcrc_enum_frame& f)
{
    return f.num_buckets == 0 || (f.num_buckets & (f.num_buckets - 1)) != 0;
}

// Does stale frame f hide hash h: was it sent while that frame was the top?
RAMCRC_PART_HD bool hidden(const ramcrc_enum_frame& f, uint64_t h)
{
    if (h < f.tablet_start_hash || h > f.tablet_end_hash)
        return false;
    const uint64_t idx = bucket_of(h, f.num_buckets);
    return idx < f.bucket_index || (idx == f.bucket_index && h < f.bucket_next_hash);
}

// What a call selects, apart from the table id.
struct Select {
    uint64_t first_hash, last_hash;
    uint64_t bucket_index, bucket_next_hash;   // the top frame's cursor
    uint64_t n_stale;
    ramcrc_enum_frame stale[RAMCRC_ENUM_MAX_STALE];
};

// Is hash h, whose home is bucket b, selected?
RAMCRC_PART_HD bool selected(const Select& s, uint64_t b, uint64_t h)
{
    if (h < s.first_hash || h > s.last_hash)
        return false;
    if (b == s.bucket_index && h < s.bucket_next_hash)
        return false;
    for (uint32_t k = 0; k < s.n_stale; k++)
        if (hidden(s.stale[k], h))
            return false;
    return true;
}

// Of a selected hash h of bucket b: is it sent, where bucket_index was cut
// (`cut`) before the first entry of hash cut_hash?
RAMCRC_PART_HD bool before_cut(const Select& s, uint64_t b, uint64_t h, bool cut, uint64_t cut_hash)
{
    return !(cut && b == s.bucket_index && h >= cut_hash);
}

// The `length` of the entry of an object whose payload has len bytes and whose
// value lies at v: the whole payload, or with RAMCRC_ENUM_KEYS_ONLY the bytes
// before the value.
RAMCRC_PART_HD uint32_t entry_length(uint32_t flags, uint32_t len, const ramcrc_look::Value& v)
{
    return (flags & RAMCRC_ENUM_KEYS_ONLY) ? v.off : len;
}

// Bytes an entry takes in the payload.
RAMCRC_PART_HD uint64_t entry_size(uint32_t length)
{
    return uint64_t(kLengthBytes) + length;
}

// Byte b (0 .. 3) of an entry's length.
RAMCRC_PART_HD uint8_t length_byte(uint32_t length, uint32_t b)
{
    return uint8_t(length >> (8 * b));
}

// readKeyBytes of an entry's object: keysAndValueLength - valueLength.
RAMCRC_PART_HD uint32_t key_bytes(uint32_t len, const ramcrc_look::Value& v)
{
    return len - 24 - v.len;
}

// The entries of a bucket go in ascending {hash, order}; order: the winner's
// batch, then its record.
RAMCRC_PART_HD uint64_t order_of(uint32_t batch, uint32_t record)
{
    return (uint64_t(batch) << 32) | record;
}

// Is {h, o} at or above {fh, fo}?
RAMCRC_PART_HD bool at_or_above(uint64_t h, uint64_t o, uint64_t fh, uint64_t fo)
{
    return h > fh || (h == fh && o >= fo);
}

// Is {h, o} below {bh, bo}?
RAMCRC_PART_HD bool below(uint64_t h, uint64_t o, uint64_t bh, uint64_t bo)
{
    return h < bh || (h == bh && o < bo);
}

// lim: no entry ends past it.
RAMCRC_PART_HD uint64_t limit(uint64_t max_bytes, uint64_t capacity)
{
    return max_bytes < capacity ? max_bytes : capacity;
}

// What one bucket holds of the selection.
struct Found {
    uint64_t bytes;        // of its entries
    uint64_t objects;      // selected keys whose winner is an object
    uint64_t tombstones;   // selected keys whose winner is a tombstone
    uint64_t value_bytes, key_bytes;
};

RAMCRC_PART_HD Found nothing()
{
    return Found{0ull, 0ull, 0ull, 0ull, 0ull};
}

// One more object, of payload length len with its value at v.
RAMCRC_PART_HD void add_object(Found* f, uint32_t flags, uint32_t len, const ramcrc_look::Value& v)
{
    f->bytes += entry_size(entry_length(flags, len, v));
    f->objects++;
    f->value_bytes += v.len;
    f->key_bytes += key_bytes(len, v);
}

// The cut of bucket_index itself, fed its entries in ascending {hash, order}:
// the leading entries that end at or before lim are sent, less the ones that
// share the hash of the first entry not sent (a resume with h >= next_hash
// then sends nothing twice).
struct Cut {
    Found sent;          // what is sent
    Found run;           // what the entries before the current hash's first one come to
    uint64_t run_hash;   // the current hash
    uint64_t next_hash;
    uint32_t any, done;
};

RAMCRC_PART_HD Cut cut_begin()
{
    return Cut{nothing(), nothing(), 0ull, 0ull, 0u, 0u};
}

// The next entry; false: it is the first one not sent, and c->sent and
// c->next_hash stand.
RAMCRC_PART_HD bool cut_entry(Cut* c, uint64_t lim, uint64_t h, uint32_t flags, uint32_t len,
                              const ramcrc_look::Value& v)
{
    if (!c->any || h != c->run_hash) {
        c->run = c->sent;
        c->run_hash = h;
        c->any = 1;
    }
    Found next = c->sent;
    add_object(&next, flags, len, v);
    if (next.bytes > lim) {
        c->sent = c->run;
        c->next_hash = h;
        c->done = 1;
        return false;
    }
    c->sent = next;
    return true;
}

}  // namespace ramcrc_en
