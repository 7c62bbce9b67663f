// The per-request rules of ramcrc_replay_table_increment_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_increment.inc) and the
// host form (ramcrc_host.cc): what a request's lookup and its RejectRules make
// of it (MasterService::incrementObject, src/MasterService.cc:678-790, over
// readObject, src/ObjectManager.cc:340-351), the sum, the keysAndValue image of
// the object it writes and the third field of its part.  Which requests are
// usable is remove_rules.h's test; the lookup, rejectOperation, the version and
// the entries' sizes and header bytes are lookup_rules.h's, read_rules.h's and
// write_rules.h's, unchanged.  The callers differ only in how they read the key
// bytes and the old value.
#pragma once

#include <stdint.h>

#include "remove_rules.h"

namespace ramcrc_increment {

using ramcrc_remove::bad_request;
using ramcrc_write::kNone;
using ramcrc_write::kStatusRetry;

constexpr uint32_t kStatusInvalidObject = 22;   // src/Status.h
constexpr uint32_t kPartBytes = 20;             // MultiOp::Response::IncrementPart, packed
constexpr uint32_t kValueBytes = 8;             // int64_t and double (:692-696)
constexpr uint32_t kImagePrefix = 3;            // the image's bytes in front of the key
constexpr uint64_t kNaN = 0x7FF8000000000000ull;

// What becomes of the first usable request of its key, before the space check.
struct Outcome {
    uint32_t status;   // of a request that does not reach the write
    uint64_t cur;      // the write's cur, and a rejected part's version
    bool reach;        // goes on to the sum and the write (status is STATUS_OK)
};

// `kind`, `version`, `value_len`: the key's winner as the lookup returns it.
// Absent and a tombstone are VERSION_NONEXISTENT to rejectOperation, which then
// tests doesnt_exist alone (:697, :707-712); an object goes through it whole,
// then through the length test (:716-722; ours: lengths below 8 too).
RAMCRC_PART_HD Outcome outcome(uint32_t kind, uint64_t version, uint32_t value_len,
                               const ramcrc_read::Rules& r)
{
    const bool obj = kind == RAMCRC_LOOKUP_OBJECT;
    const uint64_t cur = obj ? version : 0ull;
    const uint32_t st = ramcrc_read::reject(r, cur);
    if (st != ramcrc_read::kStatusOk)
        return Outcome{st, cur, false};
    if (obj && value_len != kValueBytes)
        return Outcome{kStatusInvalidObject, cur, false};
    return Outcome{ramcrc_read::kStatusOk, cur, true};
}

RAMCRC_PART_HD double as_double(uint64_t bits)
{
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}

RAMCRC_PART_HD uint64_t as_bits(double d)
{
    uint64_t bits;
    __builtin_memcpy(&bits, &d, 8);
    return bits;
}

// The sum (:741-749) on the old value's bits: the integer first, wrapping, then
// the double on the resulting bits.  One IEEE binary64 addition, round to
// nearest even, subnormals kept: there is no product to contract it with, the
// pragma says so to the compiler, and neither build passes a flag that flushes
// f64 subnormals.  Ours: every NaN result is kNaN.
RAMCRC_PART_HD uint64_t sum(uint64_t old_bits, uint64_t add_int64, uint64_t add_double_bits)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint64_t bits = old_bits;
    if (add_int64 != 0)
        bits += add_int64;
    const double inc = as_double(add_double_bits);
    if (inc != 0.0) {   // -0.0 adds nothing; a NaN does add
        bits = as_bits(as_double(bits) + inc);
        if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull)
            bits = kNaN;
    }
    return bits;
}

// The keysAndValue image (:752-756, Object::appendKeysAndValueToBuffer with one
// key): {u8 1, u16 key_len, the key, the 8 new bytes}.
RAMCRC_PART_HD uint32_t image_len(uint32_t key_len)
{
    return kImagePrefix + key_len + kValueBytes;
}

RAMCRC_PART_HD uint32_t image_prefix_byte(uint32_t b, uint32_t key_len)
{
    return b == 0 ? 1u : (key_len >> (8 * (b - 1))) & 0xFFu;
}

// Byte m of the new object's checksummed bytes [4, end): header bytes [4, 24),
// the image's prefix, then the key (key_byte(k) reads key byte k and is called
// only for k < key_len), then the new value.
template <typename KeyByte>
RAMCRC_PART_HD uint32_t object_byte(uint32_t m, uint32_t key_len, uint32_t timestamp, uint64_t version,
                                    uint64_t table_id, uint64_t new_bits, const KeyByte& key_byte)
{
    constexpr uint32_t kHead = ramcrc_write::kObjHeader - 4;
    if (m < kHead)
        return ramcrc_write::obj_header_byte(4 + m, timestamp, version, table_id);
    if (m < kHead + kImagePrefix)
        return image_prefix_byte(m - kHead, key_len);
    if (m < kHead + kImagePrefix + key_len)
        return key_byte(m - kHead - kImagePrefix);
    return uint32_t(new_bits >> (8 * (m - kHead - kImagePrefix - key_len))) & 0xFFu;
}

// The part's third field: the new value of a STATUS_OK part; otherwise the bits
// of the request's add_double, which :1319-1320 assign last.
RAMCRC_PART_HD uint64_t part_value(uint32_t status, uint64_t new_bits, uint64_t add_double_bits)
{
    return status == ramcrc_read::kStatusOk ? new_bits : add_double_bits;
}

}  // namespace ramcrc_increment
