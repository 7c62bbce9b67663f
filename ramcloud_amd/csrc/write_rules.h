// The per-request rules of ramcrc_replay_table_write_device / _host
// (include/ramcrc.h), shared by the device kernels (dev_write.inc) and the host
// form (ramcrc_host.cc): which requests are usable and where their first key
// lies (ramcrc_part::parse over the object the request becomes), the new
// version (ObjectManager::writeObject, src/ObjectManager.cc:1245-1246, and our
// tombstone rule), the sizes of the entries Segment::append writes, and the
// header words of the object and of the tombstone.  The lookup and
// rejectOperation that come first are lookup_rules.h's and read_rules.h's.
// The callers differ only in how they read the data bytes.
#pragma once

#include <stdint.h>

#include "read_rules.h"

namespace ramcrc_write {

constexpr uint32_t kStatusRetry = 17;   // src/Status.h
constexpr uint32_t kPartBytes = 12;     // MultiOp::Response::WritePart, packed
constexpr uint32_t kObjHeader = 24;     // Object::Header
constexpr uint32_t kTombHeader = 32;    // ObjectTombstone::Header
constexpr uint32_t kNone = 0xFFFFFFFFu;

// The tests of a request that read neither the data buffer nor the table.
// data_off + data_len is taken in 64 bits, overflow included, as
// ramcrc_look::bad_query takes a key's.
RAMCRC_PART_HD bool bad_request(uint64_t data_off, uint32_t data_len, uint32_t reserved,
                                bool bad_rules, uint64_t data_bytes)
{
    return reserved != 0 || bad_rules || data_off > data_bytes || data_bytes - data_off < data_len ||
           data_len > 0xFFFFFFFFu - kObjHeader;
}

struct Key {
    bool ok;
    uint32_t off, len;   // from data byte 0
};

// The first key of the object a request's data becomes: ramcrc_part::parse of
// an OBJ record with the 24-byte header in front of the data.  rd.u8/u16(o)
// read data byte o and are called only for bytes inside the data.
template <typename Rd>
RAMCRC_PART_HD Key first_key(uint32_t data_len, const Rd& rd)
{
    if (data_len < 1)
        return Key{false, 0u, 0u};
    const uint32_t nk = rd.u8(0);
    if (nk == 0)
        return Key{true, 1u, 0u};   // the empty key
    if (data_len < 3)
        return Key{false, 0u, 0u};
    const uint32_t kl = rd.u16(1), off = 1 + 2 * nk;
    if (uint64_t(off) + kl > data_len)
        return Key{false, 0u, 0u};
    return Key{true, off, kl};
}

// writeValueBytes' value: Object::getValueLength of that object (lookup_rules.h's
// object_value with the header taken off).
template <typename Rd>
RAMCRC_PART_HD uint32_t value_len(uint32_t data_len, const Rd& rd)
{
    const uint32_t nk = rd.u8(0);
    uint64_t at = 1;
    if (nk) {
        at += 2 * nk;
        if (at > data_len)
            return 0u;
        at += rd.u16(uint32_t(at) - 2);
        if (at > data_len)
            return 0u;
    }
    return data_len - uint32_t(at);
}

// The new object's version.  cur: the winning object's version, 0 when the
// winner is a tombstone or there is none; a: the next allocated version, used
// only when cur == 0.  Ours: a tombstone winner of version tv >= a gives tv + 1.
RAMCRC_PART_HD uint64_t new_version(uint64_t cur, bool tomb, uint64_t tv, uint64_t a)
{
    if (cur != 0)
        return cur + 1;
    return tomb && tv >= a ? tv + 1 : a;
}

// The EntryHeader constructor's choice of length bytes (src/Segment.h:134-149).
RAMCRC_PART_HD uint32_t len_bytes(uint32_t len)
{
    return len < 0x100u ? 1u : len < 0x10000u ? 2u : len < 0x1000000u ? 3u : 4u;
}

// Bytes an entry of `len` payload bytes takes in the segment.
RAMCRC_PART_HD uint64_t entry_size(uint32_t len)
{
    return uint64_t(1) + len_bytes(len) + len;
}

// Bytes a served request appends: the object, then the tombstone of the object
// it replaces.
RAMCRC_PART_HD uint64_t request_size(uint32_t data_len, bool tomb, uint32_t key_len)
{
    return entry_size(kObjHeader + data_len) + (tomb ? entry_size(kTombHeader + key_len) : 0ull);
}

// An entry's metadata: the header byte and the length bytes, little-endian in
// one word; *n: how many bytes.
RAMCRC_PART_HD uint64_t entry_meta(uint32_t type, uint32_t len, uint32_t* n)
{
    const uint32_t lb = len_bytes(len);
    *n = 1 + lb;
    return uint64_t(type | ((lb - 1) << 6)) | (uint64_t(len) << 8);
}

// Bytes [4, 24) of the object's header: timestamp, version, table id.
RAMCRC_PART_HD uint32_t obj_header_byte(uint32_t b, uint32_t timestamp, uint64_t version, uint64_t table_id)
{
    if (b < 8)
        return (timestamp >> (8 * (b - 4))) & 0xFFu;
    if (b < 16)
        return uint32_t(version >> (8 * (b - 8))) & 0xFFu;
    return uint32_t(table_id >> (8 * (b - 16))) & 0xFFu;
}

// Bytes [0, 28) of the tombstone's header: table id, segment id, the replaced
// object's version, timestamp.
RAMCRC_PART_HD uint32_t tomb_header_byte(uint32_t b, uint64_t table_id, uint64_t segment_id,
                                         uint64_t version, uint32_t timestamp)
{
    if (b < 8)
        return uint32_t(table_id >> (8 * b)) & 0xFFu;
    if (b < 16)
        return uint32_t(segment_id >> (8 * (b - 8))) & 0xFFu;
    if (b < 24)
        return uint32_t(version >> (8 * (b - 16))) & 0xFFu;
    return (timestamp >> (8 * (b - 24))) & 0xFFu;
}

}  // namespace ramcrc_write
