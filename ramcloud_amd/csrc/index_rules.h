// The rules of ramcrc_replay_table_index_build_device / _host and
// ramcrc_index_lookup_device / _host (include/ramcrc.h), shared by the device
// kernels (dev_index.inc) and the host forms (ramcrc_host.cc): which key of an
// object gets an entry (MasterService::requestInsertIndexEntries,
// src/MasterService.cc:1993-2032), an entry's prefix, the order of the entries
// (IndexKey::keyCompare, src/IndexKey.cc:41-59, then pKHash: key_less,
// src/btreeRamCloud/Btree.h:1978-1985), the two searches of
// IndexletManager::lookupIndexKeys (src/IndexletManager.cc:654-706) and which
// queries are unusable.  The callers differ only in how they read bytes.
#pragma once

#include <stdint.h>

#include "lookup_rules.h"
#include "ramcrc.h"

namespace ramcrc_ix {

constexpr uint32_t kPrefixBytes = 8;
constexpr uint32_t kPadLen = 0xFFFFFFFFu;   // key_len of a sort tile's padding: above every entry

// Key `index` of an object whose payload has len bytes (a participant: len >=
// 25), from payload byte 0.  len == 0: the object gets no entry -- it has no
// such key, the key is empty, or its key table or keys run past the payload
// (lookup_rules.h's rule for a broken key table, which gives no value either).
struct KeyAt {
    uint32_t off, len;
};

template <typename Rd>
RAMCRC_PART_HD KeyAt key_at(uint32_t len, const Rd& rd, uint32_t index)
{
    const uint32_t kc = ramcrc_look::kKeyCountAt;
    const uint32_t nk = rd.u8(kc);
    if (nk <= index)
        return KeyAt{0u, 0u};
    const uint32_t keys = kc + 1 + 2 * nk;
    if (keys > len)
        return KeyAt{0u, 0u};
    const uint32_t all = rd.u16(keys - 2);   // the last cumulative length
    if (keys + all > len)
        return KeyAt{0u, 0u};
    const uint32_t start = index ? rd.u16(kc + 1 + 2 * (index - 1)) : 0u;
    const uint32_t end = rd.u16(kc + 1 + 2 * index);
    if (end <= start || end > all)
        return KeyAt{0u, 0u};
    return KeyAt{keys + start, end - start};
}

// The first 8 bytes of a key as a big-endian integer, zero-padded on the
// right: prefixes that differ order their keys as memcmp does.
template <typename Bytes>
RAMCRC_PART_HD uint64_t prefix_of(const Bytes& k, uint32_t len)
{
    uint64_t p = 0;
    for (uint32_t b = 0; b < kPrefixBytes; b++)
        p = (p << 8) | (b < len ? uint64_t(k[b]) : 0ull);
    return p;
}

// A key as the comparator sees it: prefix and length at hand, the bytes from
// byte 8 behind `tail` (read only for equal prefixes where both keys are
// longer than 8, and never at or past len).
template <typename Bytes>
struct KeyRef {
    uint64_t prefix;
    uint32_t len;
    Bytes tail;   // tail[i]: byte 8 + i
};

// keyCompare as it orders non-empty keys: memcmp over the common length,
// unsigned, then the shorter key first; an empty key is below every other
// (ours: the reference's rule for an empty second key is no order, and the
// lookup handles an empty last key by itself).  Returns <0, 0, >0.
template <typename A, typename B>
RAMCRC_PART_HD int key_compare(const KeyRef<A>& a, const KeyRef<B>& b)
{
    if (a.prefix != b.prefix)
        return a.prefix < b.prefix ? -1 : 1;
    const uint32_t m = a.len < b.len ? a.len : b.len;
    // equal prefixes: the common bytes below 8 are equal, zero padding included
    for (uint32_t i = kPrefixBytes; i < m; i++) {
        const uint32_t x = a.tail[i - kPrefixBytes], y = b.tail[i - kPrefixBytes];
        if (x != y)
            return x < y ? -1 : 1;
    }
    return a.len < b.len ? -1 : a.len > b.len ? 1 : 0;
}

// The order of the entries: key, then hash.
template <typename A, typename B>
RAMCRC_PART_HD bool entry_less(const KeyRef<A>& a, uint64_t ah, const KeyRef<B>& b, uint64_t bh)
{
    const int c = key_compare(a, b);
    return c < 0 || (c == 0 && ah < bh);
}

RAMCRC_PART_HD ramcrc_index_entry make_entry(uint64_t prefix, uint64_t pk_hash, uint64_t key_off, uint32_t key_len)
{
    return ramcrc_index_entry{prefix, pk_hash, key_off, key_len, 0u};
}

// Do the entries and their keys fit?
RAMCRC_PART_HD bool overflow(uint64_t entries_needed, uint64_t key_bytes_needed, uint64_t entry_capacity,
                             uint64_t keys_capacity)
{
    return entries_needed > entry_capacity || key_bytes_needed > keys_capacity;
}

// Is a query unusable?  Both key ranges as the lookup tests its one.
RAMCRC_PART_HD bool bad_query(const ramcrc_index_query& q, uint64_t qkeys_bytes)
{
    return ramcrc_look::bad_query(q.first_off, q.first_len, q.reserved, qkeys_bytes) ||
           ramcrc_look::bad_query(q.last_off, q.last_len, 0u, qkeys_bytes);
}

// The two searches over n entries in the build's order.  `less_first(i)`: is
// entry i below {first key, first_allowed_hash}; `above_last(i)`: does entry
// i's key compare greater than the last key.  Both are monotone in i.
template <typename Pred>
RAMCRC_PART_HD uint64_t first_false(uint64_t n, const Pred& pred)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pred(mid))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// What a query's range [lo, hi) returns.
struct Answer {
    uint64_t lo;
    uint32_t num;      // min(hi - lo, max_hashes)
    uint32_t more;     // 1: hi - lo > max_hashes, entry lo + num is the next one
};

RAMCRC_PART_HD Answer answer(uint64_t lo, uint64_t hi, uint32_t max_hashes)
{
    const uint64_t cnt = hi > lo ? hi - lo : 0ull;
    if (cnt > max_hashes)
        return Answer{lo, max_hashes, 1u};
    return Answer{lo, uint32_t(cnt), 0u};
}

// The result of a query that is not answered (BAD_QUERY, NOT_SERVED).
RAMCRC_PART_HD ramcrc_index_result no_result(uint32_t status)
{
    return ramcrc_index_result{RAMCRC_READ_NONE, 0ull, 0ull, 0ull, 0u, 0u, status, 0u};
}

// Is a query whose hashes are [off, off + num) served?  Monotone in the
// query's index: the served queries are a prefix.
RAMCRC_PART_HD bool served(uint64_t off, uint32_t num, uint64_t out_capacity)
{
    return off + num <= out_capacity;
}

}  // namespace ramcrc_ix
