// Host-side CRC32C for the synchronous Crc32C::update() path.
//
// RAMCloud keeps update() synchronous and on the caller's thread
// (src/Crc32C.h:200-206); the 1-5 byte metadata updates of Segment::append
// (src/Segment.cc:211,218) and the per-object checksums on the write path must
// never wait on a GPU.  This file provides that host path behind the C ABI:
//
//   ramcrc_update_hw  SSE4.2 crc32 instruction.  The reference runs one
//                     dependency chain (src/Crc32C.h:52-84), bound by the
//                     3-cycle crc32q latency; here three independent chains
//                     run over three adjacent 8 KiB blocks and are merged with
//                     X^n operator tables (raw(0,A||B) = X^|B|(raw(0,A)) ^
//                     raw(0,B)), so the core issues one crc32q per cycle.
//   ramcrc_update_sw  slicing-by-8 like softwareCrc32C (src/Crc32C.h:96-153),
//                     tables generated from the polynomial at compile time.
#include "ramcrc.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "gf2.h"
#include "murmur3.h"
#include "partition_rules.h"
#include "lookup_rules.h"
#include "read_rules.h"
#include "read_hashes_rules.h"
#include "enumerate_rules.h"
#include "index_rules.h"
#include "resolve_rules.h"
#include "sidelog_rules.h"
#include "write_rules.h"
#include "remove_rules.h"
#include "increment_rules.h"
#include "clean_rules.h"
#include "migrate_rules.h"

namespace {

using ramcrc::ByteTable;
using ramcrc::OpTable;

struct Slice8 {
    uint32_t t[8][256];
};

constexpr Slice8 make_slice8()
{
    Slice8 s{};
    const ByteTable b = ramcrc::make_byte_table();
    for (int i = 0; i < 256; i++)
        s.t[0][i] = b.t[i];
    for (int i = 0; i < 256; i++) {
        uint32_t c = s.t[0][i];
        for (int k = 1; k < 8; k++) {
            c = s.t[0][c & 0xFF] ^ (c >> 8);
            s.t[k][i] = c;
        }
    }
    return s;
}

constexpr uint64_t kStreamBlock = 8192;  // bytes per interleaved chain
constexpr Slice8 kSlice = make_slice8();
constexpr OpTable kShift1 = ramcrc::make_op(kStreamBlock);
constexpr OpTable kShift2 = ramcrc::make_op(2 * kStreamBlock);

inline uint64_t ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint16_t ld16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }

#if defined(__x86_64__) || defined(__i386__)
__attribute__((target("sse4.2"))) uint32_t hw_chain(uint32_t s, const uint8_t* p, uint64_t n)
{
    uint64_t c = s;
    for (; n >= 8; n -= 8, p += 8)
        c = __builtin_ia32_crc32di(c, ld64(p));
    s = static_cast<uint32_t>(c);
    if (n & 4) {
        s = __builtin_ia32_crc32si(s, ld32(p));
        p += 4;
    }
    if (n & 2) {
        s = __builtin_ia32_crc32hi(s, ld16(p));
        p += 2;
    }
    if (n & 1)
        s = __builtin_ia32_crc32qi(s, *p);
    return s;
}

__attribute__((target("sse4.2"))) uint32_t hw_update(uint32_t s, const uint8_t* p, uint64_t n)
{
    while (n >= 3 * kStreamBlock) {
        uint64_t c0 = s, c1 = 0, c2 = 0;
        const uint8_t* p1 = p + kStreamBlock;
        const uint8_t* p2 = p + 2 * kStreamBlock;
        for (uint64_t i = 0; i < kStreamBlock; i += 8) {
            c0 = __builtin_ia32_crc32di(c0, ld64(p + i));
            c1 = __builtin_ia32_crc32di(c1, ld64(p1 + i));
            c2 = __builtin_ia32_crc32di(c2, ld64(p2 + i));
        }
        s = ramcrc::apply_op(kShift2, static_cast<uint32_t>(c0)) ^
            ramcrc::apply_op(kShift1, static_cast<uint32_t>(c1)) ^ static_cast<uint32_t>(c2);
        p += 3 * kStreamBlock;
        n -= 3 * kStreamBlock;
    }
    return hw_chain(s, p, n);
}
#endif

uint32_t sw_update(uint32_t crc, const uint8_t* p, uint64_t n)
{
    uint64_t lead = (4u - (reinterpret_cast<uintptr_t>(p) & 3u)) & 3u;
    if (lead > n)
        lead = n;
    for (uint64_t i = 0; i < lead; i++)
        crc = kSlice.t[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    n -= lead;
    for (uint64_t k = n >> 3; k > 0; k--, p += 8) {
        const uint32_t lo = crc ^ ld32(p);
        const uint32_t hi = ld32(p + 4);
        crc = kSlice.t[7][lo & 0xFF] ^ kSlice.t[6][(lo >> 8) & 0xFF] ^
              kSlice.t[5][(lo >> 16) & 0xFF] ^ kSlice.t[4][lo >> 24] ^
              kSlice.t[3][hi & 0xFF] ^ kSlice.t[2][(hi >> 8) & 0xFF] ^
              kSlice.t[1][(hi >> 16) & 0xFF] ^ kSlice.t[0][hi >> 24];
    }
    for (uint64_t i = 0; i < (n & 7); i++)
        crc = kSlice.t[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return crc;
}

bool detect_hw()
{
#if defined(__x86_64__) || defined(__i386__)
    return __builtin_cpu_supports("sse4.2");
#else
    return false;
#endif
}

const bool g_have_hw = detect_hw();

}  // namespace

extern "C" {

uint32_t ramcrc_update_hw(uint32_t state, const void* data, uint64_t nbytes)
{
#if defined(__x86_64__) || defined(__i386__)
    if (g_have_hw)
        return hw_update(state, static_cast<const uint8_t*>(data), nbytes);
#endif
    return sw_update(state, static_cast<const uint8_t*>(data), nbytes);
}

uint32_t ramcrc_update_sw(uint32_t state, const void* data, uint64_t nbytes)
{
    return sw_update(state, static_cast<const uint8_t*>(data), nbytes);
}

uint32_t ramcrc_update(uint32_t state, const void* data, uint64_t nbytes)
{
    return ramcrc_update_hw(state, data, nbytes);
}

int ramcrc_cpu_has_hw(void) { return g_have_hw ? 1 : 0; }

const uint32_t* ramcrc_slice8_tables(void) { return &kSlice.t[0][0]; }

uint32_t ramcrc_shift(uint32_t state, uint64_t nbytes)
{
    return ramcrc::mulmod(state, ramcrc::xpow8(nbytes));
}

uint32_t ramcrc_combine(uint32_t raw_a, uint32_t raw_b, uint64_t len_b)
{
    return ramcrc_shift(raw_a, len_b) ^ raw_b;
}

// The append path of RecoverSegmentBenchmark::run
// (nanobenchmarks/RecoverSegmentBenchmark.cc:131-146): Object(key, value,
// version 0, timestamp 0) serialised by Object::assembleForLog
// (src/Object.cc:213-218) -- Header{checksum, timestamp, version, tableId}
// (src/Object.h:137-182), KeyCount 1, CumulativeKeyLength 8, the 8-byte key
// (src/Object.cc:107-141), the value -- appended by Segment::append
// (src/Segment.cc:197-228) while hasSpaceFor (:136-154) holds.
int ramcrc_segment_fill_objects(uint8_t* seg, uint32_t capacity, uint32_t value_len,
                                uint64_t first_key, uint32_t* n_objects, ramcrc_seg_cert* cert)
{
    if (!seg || !cert)
        return RAMCRC_EINVAL;
    const uint64_t objlen64 = 24 + 1 + 2 + 8 + uint64_t(value_len);
    if (objlen64 > 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    const uint32_t objlen = uint32_t(objlen64);
    const uint32_t lb = objlen < 0x100u ? 1 : objlen < 0x10000u ? 2 : objlen < 0x1000000u ? 3 : 4;
    const uint8_t hdr = uint8_t(RAMCRC_LOG_ENTRY_TYPE_OBJ | ((lb - 1) << 6));
    const uint64_t entry = 1 + lb + uint64_t(objlen);
    uint32_t head = 0, n = 0, meta = 0xFFFFFFFFu;
    uint64_t key = first_key;
    while (entry <= uint64_t(capacity) - head) {
        uint8_t* e = seg + head;
        e[0] = hdr;
        for (uint32_t k = 0; k < lb; k++)
            e[1 + k] = uint8_t(objlen >> (8 * k));
        meta = ramcrc_update(meta, e, 1 + lb);   // Segment's running metadata checksum
        uint8_t* o = e + 1 + lb;
        memset(o + 4, 0, 20);                    // timestamp, version, tableId
        o[24] = 1;                               // KeyCount
        o[25] = 8;                               // CumulativeKeyLength (LE)
        o[26] = 0;
        for (int k = 0; k < 8; k++)
            o[27 + k] = uint8_t(key >> (8 * k));
        const uint32_t ck = ~ramcrc_update(0xFFFFFFFFu, o + 4, objlen - 4);   // Object::computeChecksum
        for (int k = 0; k < 4; k++)
            o[k] = uint8_t(ck >> (8 * k));
        head += uint32_t(entry);
        n++;
        key++;
    }
    memset(seg + head, 0, capacity - head);
    uint8_t lenle[4];
    for (int k = 0; k < 4; k++)
        lenle[k] = uint8_t(head >> (8 * k));
    cert->segment_length = head;
    cert->checksum = ~ramcrc_update(meta, lenle, 4);   // Segment::getAppendedLength
    if (n_objects)
        *n_objects = n;
    return RAMCRC_OK;
}

// The append loop of RecoverySegmentBuilder::build
// (src/RecoverySegmentBuilder.cc:61-203) over a caller's placement list: one
// Segment::append (src/Segment.cc:197-228) per placement, into the recovery
// segment (source segment, partition), while hasSpaceFor (:136-154) holds.
// Two passes over the list: the first checks it, so a refused call writes
// nothing.  pdst (nullable, one per placement): the offset of the placement's
// entry header in its output, or 0xFFFFFFFF when it was not appended, as the
// device keeps it (AppDesc::pdst) -- what the side log builds on.
}  // extern "C"

namespace {
constexpr uint32_t kNotAppended = 0xFFFFFFFFu;

int append_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                uint64_t n_entries, const ramcrc_placement* place, uint64_t n_place,
                uint32_t n_part, void* out, uint64_t out_stride, uint32_t out_capacity,
                ramcrc_seg_cert* out_certs, ramcrc_append_status* out_status, uint32_t* pdst)
{
    if (n_part == 0 || out_stride < out_capacity || n_seg > 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (n_seg == 0)
        return RAMCRC_OK;
    if (!base || !status || !out || !out_certs || !out_status || (n_entries && !entries) ||
        (n_place && !place))
        return RAMCRC_EINVAL;
    const uint64_t n_out = n_seg * n_part;   // < 2^64: both below 2^32
    if ((seg_stride && n_seg > UINT64_MAX / seg_stride) ||
        (out_stride && n_out > UINT64_MAX / out_stride))
        return RAMCRC_EINVAL;
    const uintptr_t sb = reinterpret_cast<uintptr_t>(base), ob = reinterpret_cast<uintptr_t>(out);
    const uint64_t src_bytes = n_seg * seg_stride, out_bytes = n_out * out_stride;
    if (sb < ob + out_bytes && ob < sb + src_bytes)
        return RAMCRC_EINVAL;   // the outputs would overwrite the source
    if (n_place) {
        // a segment's placements are one run of the list, as k_app_mark demands
        // (a table whose segments are not contiguous runs is not a walk's)
        uint8_t* const seen = static_cast<uint8_t*>(calloc((n_seg + 7) / 8, 1));
        if (!seen)
            return RAMCRC_ENOMEM;
        bool ok = true;
        for (uint64_t i = 0; i < n_place && ok; i++) {
            ok = place[i].record < n_entries && place[i].partition < n_part &&
                 (!i || place[i].record >= place[i - 1].record) &&
                 entries[place[i].record].segment < n_seg;
            if (!ok)
                break;
            const uint32_t seg = entries[place[i].record].segment;
            if (!i || entries[place[i - 1].record].segment != seg) {
                ok = !(seen[seg >> 3] & (1u << (seg & 7)));
                seen[seg >> 3] |= uint8_t(1u << (seg & 7));
            }
        }
        free(seen);
        if (!ok)
            return RAMCRC_EINVAL;
    }
    uint8_t* const o = static_cast<uint8_t*>(out);
    for (uint64_t k = 0; k < n_out; k++) {
        // head 0, a fresh Crc32C; the running state is kept in the certificate
        out_certs[k] = ramcrc_seg_cert{0u, 0xFFFFFFFFu};
        out_status[k] = ramcrc_append_status{
            (status[k / n_part].flags & RAMCRC_SEG_OK) ? RAMCRC_SEG_OK : RAMCRC_SEG_SOURCE_BAD, 0u};
    }
    for (uint64_t i = 0; i < n_place; i++) {
        const ramcrc_seg_entry& r = entries[place[i].record];
        const uint64_t k = uint64_t(r.segment) * n_part + place[i].partition;
        if (pdst)
            pdst[i] = kNotAppended;
        if (out_status[k].flags != RAMCRC_SEG_OK)
            continue;   // bad source, or full: nothing more is appended
        const uint32_t len = r.length;
        const uint32_t lb = len < 0x100u ? 1 : len < 0x10000u ? 2 : len < 0x1000000u ? 3 : 4;
        const uint64_t src = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
        const uint32_t head = out_certs[k].segment_length;
        if ((r.header & RAMCRC_SEG_ENTRY_OVERLONG) || src + len > seg_stride ||
            uint64_t(head) + 1 + lb + len > out_capacity) {
            out_status[k].flags = RAMCRC_SEG_APPEND_FULL;
            continue;
        }
        uint8_t* e = o + k * out_stride + head;
        e[0] = uint8_t((r.header & 0x3f) | ((lb - 1) << 6));
        for (uint32_t b = 0; b < lb; b++)
            e[1 + b] = uint8_t(len >> (8 * b));
        out_certs[k].checksum = ramcrc_update(out_certs[k].checksum, e, 1 + lb);
        memcpy(e + 1 + lb, static_cast<const uint8_t*>(base) + r.segment * seg_stride + src, len);
        out_certs[k].segment_length = head + 1 + lb + len;
        out_status[k].entries++;
        if (pdst)
            pdst[i] = head;
    }
    for (uint64_t k = 0; k < n_out; k++) {
        uint8_t lenle[4];
        for (int b = 0; b < 4; b++)
            lenle[b] = uint8_t(out_certs[k].segment_length >> (8 * b));
        out_certs[k].checksum = ~ramcrc_update(out_certs[k].checksum, lenle, 4);
    }
    return RAMCRC_OK;
}
}  // namespace

extern "C" {

int ramcrc_recovery_append_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                                const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                                uint64_t n_entries, const ramcrc_placement* place, uint64_t n_place,
                                uint32_t n_part, void* out, uint64_t out_stride,
                                uint32_t out_capacity, ramcrc_seg_cert* out_certs,
                                ramcrc_append_status* out_status)
{
    return append_host(base, seg_stride, n_seg, status, entries, n_entries, place, n_place, n_part,
                       out, out_stride, out_capacity, out_certs, out_status, nullptr);
}

// ObjectManager::replaySegment's sideLog->append of every kept record
// (src/ObjectManager.cc:720-734, :840-867): the append at one partition, then
// one pass over the list that rewrites the appended tombstones in the output
// (:845-851), notes the references and counts (sidelog_rules.h).
int ramcrc_replay_sidelog_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                               const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                               uint64_t n_entries, const ramcrc_placement* live, uint64_t n_live,
                               uint32_t timestamp, void* out, uint64_t out_stride,
                               uint32_t out_capacity, ramcrc_seg_cert* out_certs,
                               ramcrc_append_status* out_status, ramcrc_log_ref* refs,
                               ramcrc_sidelog_counts* counts)
{
    if (!counts || n_live > 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (n_seg == 0)
        return out_stride < out_capacity ? RAMCRC_EINVAL : RAMCRC_OK;
    std::vector<uint32_t> pdst;
    try {
        pdst.resize(n_live);
    } catch (const std::bad_alloc&) {
        return RAMCRC_ENOMEM;
    }
    const int rc = append_host(base, seg_stride, n_seg, status, entries, n_entries, live, n_live, 1,
                               out, out_stride, out_capacity, out_certs, out_status, pdst.data());
    if (rc)
        return rc;
    ramcrc_sidelog_counts c{};
    for (uint64_t i = 0; i < n_live; i++) {
        const ramcrc_seg_entry& r = entries[live[i].record];
        const bool app = pdst[i] != kNotAppended;
        if (refs)
            refs[i] = app ? ramcrc_log_ref{r.segment, pdst[i]}
                          : ramcrc_log_ref{RAMCRC_LOG_REF_NONE, RAMCRC_LOG_REF_NONE};
        if (!app) {
            c.left_out++;
            continue;
        }
        const uint32_t len = r.length;
        switch (ramcrc_sl::kind(r.header & 0x3f, len)) {
        case ramcrc_sl::kObject:
            c.objects++;
            c.object_bytes += len;
            break;
        case ramcrc_sl::kShortTombstone:
            c.short_tombstones++;
            break;
        case ramcrc_sl::kOther:
            c.other++;
            break;
        case ramcrc_sl::kTombstone: {
            c.tombstones++;
            c.tombstone_bytes += len;
            const uint32_t lb = len < 0x100u ? 1 : len < 0x10000u ? 2 : len < 0x1000000u ? 3 : 4;
            uint8_t* t = static_cast<uint8_t*>(out) + r.segment * out_stride + pdst[i] + 1 + lb;
            for (uint32_t b = 0; b < ramcrc_sl::kChecksumAt; b++) {
                uint32_t v;
                if (ramcrc_sl::stamped(b, timestamp, v))
                    t[b] = uint8_t(v);
            }
            uint32_t ck = ramcrc_update(0xFFFFFFFFu, t, ramcrc_sl::kChecksumAt);
            ck = ~ramcrc_update(ck, t + ramcrc_sl::kTombHeaderBytes, len - ramcrc_sl::kTombHeaderBytes);
            for (int b = 0; b < 4; b++)
                t[ramcrc_sl::kChecksumAt + b] = uint8_t(ck >> (8 * b));
            break;
        }
        }
    }
    *counts = c;
    return RAMCRC_OK;
}

// RecoverySegmentBuilder::build's placement decision on the host: one pass
// over the table in record order, the rules of partition_rules.h.
int ramcrc_recovery_partition_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                                   const ramcrc_seg_status* status,
                                   const ramcrc_seg_entry* entries, uint64_t n_entries,
                                   const ramcrc_tablet* tablets, uint32_t n_tablets,
                                   uint32_t n_part, ramcrc_placement* place, uint64_t place_cap,
                                   uint64_t* n_place, uint64_t* key_hash,
                                   ramcrc_partition_status* part_status)
{
    namespace rp = ramcrc_part;
    if (n_part == 0 || n_seg >= 0xFFFFFFFFull || n_entries >= 0xFFFFFFFFull ||
        place_cap >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (!n_place || (n_seg && (!base || !status || !part_status)) || (n_entries && !entries) ||
        (place_cap && !place) || (n_tablets && !tablets))
        return RAMCRC_EINVAL;
    if (seg_stride && n_seg > UINT64_MAX / seg_stride)
        return RAMCRC_EINVAL;
    for (uint32_t t = 0; t < n_tablets; t++)
        if (tablets[t].partition >= n_part)
            return RAMCRC_EINVAL;
    if (n_entries) {
        // every segment's records are one run of the table, as k_part_heads demands
        uint8_t* const seen = static_cast<uint8_t*>(calloc((n_seg + 7) / 8 + 1, 1));
        if (!seen)
            return RAMCRC_ENOMEM;
        bool ok = true;
        for (uint64_t i = 0; i < n_entries && ok; i++) {
            const uint32_t seg = entries[i].segment;
            ok = seg < n_seg;
            if (ok && (!i || entries[i - 1].segment != seg)) {
                ok = !(seen[seg >> 3] & (1u << (seg & 7)));
                seen[seg >> 3] |= uint8_t(1u << (seg & 7));
            }
        }
        free(seen);
        if (!ok)
            return RAMCRC_EINVAL;
    }
    struct Rd {
        const uint8_t* pay;
        uint32_t u8(uint32_t o) const { return pay[o]; }
        uint32_t u16(uint32_t o) const { return ld16(pay + o); }
        uint32_t u32(uint32_t o) const { return ld32(pay + o); }
        uint64_t u64(uint32_t o) const { return ld64(pay + o); }
    };
    const auto tab = [&](uint32_t t) -> const ramcrc_tablet& { return tablets[t]; };
    const uint8_t* const b = static_cast<const uint8_t*>(base);
    for (uint64_t s = 0; s < n_seg; s++)
        part_status[s] = ramcrc_partition_status{
            (status[s].flags & RAMCRC_SEG_OK) ? RAMCRC_SEG_OK : RAMCRC_SEG_SOURCE_BAD, 0u, 0u, 0u};
    uint64_t np = 0;
    for (uint64_t i = 0; i < n_entries;) {
        const uint32_t seg = entries[i].segment;
        ramcrc_partition_status& st = part_status[seg];
        bool have = false;   // a usable SEGHEADER before the record
        uint64_t seg_id = 0;
        // build DIEs at a placed record without a header: such a segment
        // places nothing, so this is settled before anything is written
        bool no_header = false;
        for (uint64_t j = i; j < n_entries && entries[j].segment == seg && !no_header &&
                             (status[seg].flags & RAMCRC_SEG_OK); j++) {
            const ramcrc_seg_entry& r = entries[j];
            const uint64_t pay = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
            const bool readable = !(r.header & RAMCRC_SEG_ENTRY_OVERLONG) && pay + r.length <= seg_stride;
            if ((r.header & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_SEGHEADER) {
                have = readable && r.length >= rp::kSegHeaderBytes;
                continue;
            }
            const uint32_t kind =
                rp::parse(r.header & 0x3f, r.length, readable, Rd{b + seg * seg_stride + pay}).kind;
            no_header = !have && kind != rp::kIgnored && kind != rp::kMalformed;
        }
        have = false;
        const auto emit = [&](uint64_t rec, uint32_t part) {
            if (no_header)
                return;
            if (np < place_cap)
                place[np] = ramcrc_placement{uint32_t(rec), part};
            np++;
        };
        for (; i < n_entries && entries[i].segment == seg; i++) {
            const ramcrc_seg_entry& r = entries[i];
            const uint32_t type = r.header & 0x3f;
            const uint64_t pay = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
            const bool readable = !(r.header & RAMCRC_SEG_ENTRY_OVERLONG) && pay + r.length <= seg_stride;
            if (key_hash)
                key_hash[i] = 0;
            if (type == RAMCRC_LOG_ENTRY_TYPE_SEGHEADER) {
                have = readable && r.length >= rp::kSegHeaderBytes;
                if (have)
                    seg_id = ld64(b + seg * seg_stride + pay + rp::kSegIdAt);
                continue;
            }
            if (!(status[seg].flags & RAMCRC_SEG_OK))
                continue;
            const Rd rd{b + seg * seg_stride + pay};
            const rp::Parsed p = rp::parse(type, r.length, readable, rd);
            if (p.kind == rp::kIgnored)
                continue;
            if (p.kind == rp::kMalformed) {
                st.flags |= RAMCRC_SEG_MALFORMED;
                continue;
            }
            if (p.kind == rp::kSafeVersion) {
                for (uint32_t q = 0; q < n_part; q++)
                    emit(i, q);
                st.placed += n_part;
            } else if (p.kind == rp::kPlist) {
                for (uint32_t q = 0; q < p.count; q++) {
                    const uint32_t o = rp::kPlistHeader + rp::kPartyBytes * q;
                    const uint32_t t = rp::which_tablet(rd.u64(o), rd.u64(o + 8), n_tablets, tab);
                    if (t != rp::kNoTablet) {
                        emit(i, tablets[t].partition);
                        st.placed++;
                    }
                }
            } else {
                const uint64_t hash = p.kind == rp::kKeyed
                                          ? ramcrc::key_hash(p.table_id, rd.pay + p.key_off, p.key_len)
                                          : p.hash;
                if (key_hash)
                    key_hash[i] = hash;
                const uint32_t t = rp::which_tablet(p.table_id, hash, n_tablets, tab);
                if (t == rp::kNoTablet) {
                    st.unplaced++;
                } else if (!have) {
                    // (counted nowhere: the segment places nothing)
                } else if (!rp::alive(seg_id, r.offset, tablets[t])) {
                    st.dead++;
                } else {
                    emit(i, tablets[t].partition);
                    st.placed++;
                }
            }
        }
        if (no_header)
            st = ramcrc_partition_status{RAMCRC_SEG_NO_HEADER | (st.flags & RAMCRC_SEG_MALFORMED), 0u,
                                         0u, 0u};
    }
    *n_place = np;
    return RAMCRC_OK;
}

// ObjectManager::replaySegment's newest-wins decision on the host: one pass
// over the table in record order into an open-addressed table of the keys
// (the rules of resolve_rules.h), then the verdicts.
int ramcrc_replay_resolve_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                               const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                               uint64_t n_entries, const uint64_t* key_hash, uint32_t* winner,
                               ramcrc_placement* live, uint64_t live_cap, uint64_t* n_live,
                               ramcrc_resolve_counts* counts)
{
    namespace rp = ramcrc_part;
    namespace rr = ramcrc_res;
    if (n_seg >= 0xFFFFFFFFull || n_entries >= 0xFFFFFFFFull || live_cap >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (!n_live || !counts || (n_seg && (!base || !status)) || (n_entries && !entries) ||
        (live_cap && !live))
        return RAMCRC_EINVAL;
    if (seg_stride && n_seg > UINT64_MAX / seg_stride)
        return RAMCRC_EINVAL;
    for (uint64_t i = 0; i < n_entries; i++)
        if (entries[i].segment >= n_seg)
            return RAMCRC_EINVAL;
    struct Rd {
        const uint8_t* pay;
        uint32_t u8(uint32_t o) const { return pay[o]; }
        uint32_t u16(uint32_t o) const { return ld16(pay + o); }
        uint32_t u32(uint32_t o) const { return ld32(pay + o); }
        uint64_t u64(uint32_t o) const { return ld64(pay + o); }
    };
    struct Rec {   // a participant
        uint64_t table_id, version, hash;
        const uint8_t* key;
        uint32_t key_len;
        uint64_t slot;   // ~0: no participant
    };
    struct Slot {
        uint32_t first;   // 1 + the record that claimed the slot (its key is the slot's), 0: empty
        uint32_t best;    // the key's winner so far
    };
    const uint64_t nslots = rr::slots_for(n_entries), mask = nslots - 1;
    Rec* const recs = static_cast<Rec*>(calloc(n_entries ? n_entries : 1, sizeof(Rec)));
    Slot* const slots = static_cast<Slot*>(calloc(nslots, sizeof(Slot)));
    if (!recs || !slots) {
        free(recs);
        free(slots);
        return RAMCRC_ENOMEM;
    }
    const uint8_t* const b = static_cast<const uint8_t*>(base);
    ramcrc_resolve_counts ct{0, 0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n_entries; i++) {
        const ramcrc_seg_entry& r = entries[i];
        const uint32_t type = r.header & 0x3f;
        recs[i].slot = ~0ull;
        if (!(status[r.segment].flags & RAMCRC_SEG_OK))
            continue;
        const uint64_t pay = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
        const bool readable = !(r.header & RAMCRC_SEG_ENTRY_OVERLONG) && pay + r.length <= seg_stride;
        const Rd rd{b + r.segment * seg_stride + pay};
        if (type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION) {
            if (readable && r.length >= rr::kSafeVersionBytes && rd.u64(0) > ct.safe_version)
                ct.safe_version = rd.u64(0);
            continue;
        }
        if (!rr::resolved_type(type))
            continue;
        const rp::Parsed p = rp::parse(type, r.length, readable, rd);
        if (p.kind == rp::kMalformed) {
            ct.malformed++;
            continue;
        }
        (type == RAMCRC_LOG_ENTRY_TYPE_OBJ ? ct.objects : ct.tombstones)++;
        Rec& me = recs[i];
        me.table_id = p.table_id;
        me.key = rd.pay + p.key_off;
        me.key_len = p.key_len;
        me.version = rr::version(type, rd);
        me.hash = key_hash ? key_hash[i] : ramcrc::key_hash(me.table_id, me.key, me.key_len);
        for (uint64_t s = me.hash & mask;; s = (s + 1) & mask) {   // load <= 0.5: the chain ends
            Slot& sl = slots[s];
            if (!sl.first) {
                sl.first = uint32_t(i) + 1;
                sl.best = uint32_t(i);
                me.slot = s;
                break;
            }
            const Rec& k = recs[sl.first - 1];
            if (k.hash != me.hash || k.table_id != me.table_id || k.key_len != me.key_len ||
                (me.key_len && memcmp(k.key, me.key, me.key_len)))
                continue;
            const Rec& w = recs[sl.best];
            if (rr::beats(me.version, rr::rank(type, i), w.version,
                          rr::rank(entries[sl.best].header & 0x3f, sl.best)))
                sl.best = uint32_t(i);
            me.slot = s;
            break;
        }
    }
    uint64_t nl = 0;
    for (uint64_t i = 0; i < n_entries; i++) {
        const uint32_t w = recs[i].slot == ~0ull ? RAMCRC_RESOLVE_NONE : slots[recs[i].slot].best;
        if (winner)
            winner[i] = w;
        if (w != i)
            continue;
        ((entries[i].header & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ ? ct.live_objects
                                                                  : ct.live_tombstones)++;
        if (nl < live_cap)
            live[nl] = ramcrc_placement{uint32_t(i), 0u};
        nl++;
    }
    free(recs);
    free(slots);
    *n_live = nl;
    *counts = ct;
    return RAMCRC_OK;
}

// ----------------------------------------------------------------------------
// The persistent replay table on the host (ramcrc_replay_table_*_host): the
// one-call's pass, one batch at a time into a table that stays.  A slot keeps
// its claimant's key fields (pointers into the caller's segments, which the
// lifetime rule keeps valid) and the key's winner so far.
struct ramcrc_replay_table_host {
    struct Slot {
        uint64_t claim;   // batch << 32 | record + 1 of the claimant, 0: empty
        uint64_t table_id;
        const uint8_t* key;
        uint32_t key_len;
        uint64_t version, rank;   // the winner so far (rank: is_object << 48 | batch << 32 | record)
    };
    struct Batch {
        const uint64_t* work;
        uint64_t n;
        uint64_t objects, tombstones, malformed;
        const uint8_t* base;   // the batch's segments and record table: a lookup reads its winner's record
        uint64_t stride;
        const ramcrc_seg_entry* entries;
        bool retired;          // cleaned out (ramcrc_replay_table_clean_host): nothing of it is read
        const uint64_t* key_hash = nullptr;   // the caller's hashes; null: none (the survivor of a clean)
    };
    uint64_t key_cap = 0, keys = 0, safe_version = 0;
    uint32_t max_batches = 0;
    bool spoiled = false;
    std::vector<Slot> slots;
    std::vector<Batch> batches;
};

int ramcrc_replay_table_create_host(uint64_t key_cap, uint32_t max_batches,
                                    ramcrc_replay_table_host** out)
{
    if (!out)
        return RAMCRC_EINVAL;
    *out = nullptr;
    if (key_cap >= 0xFFFFFFFFull || max_batches == 0 || max_batches > RAMCRC_REPLAY_TABLE_MAX_BATCHES)
        return RAMCRC_EINVAL;
    try {
        ramcrc_replay_table_host* t = new ramcrc_replay_table_host();
        t->key_cap = key_cap;
        t->max_batches = max_batches;
        try {
            t->slots.assign(ramcrc_res::slots_for(key_cap), ramcrc_replay_table_host::Slot{});
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_destroy_host(ramcrc_replay_table_host* t)
{
    delete t;
    return RAMCRC_OK;
}

int ramcrc_replay_table_reset_host(ramcrc_replay_table_host* t)
{
    if (!t)
        return RAMCRC_EINVAL;
    t->slots.assign(t->slots.size(), ramcrc_replay_table_host::Slot{});
    t->batches.clear();
    t->keys = t->safe_version = 0;
    t->spoiled = false;
    return RAMCRC_OK;
}

int ramcrc_replay_table_add_host(ramcrc_replay_table_host* t, const void* base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* status,
                                 const ramcrc_seg_entry* entries, uint64_t n_entries,
                                 const uint64_t* key_hash, uint64_t* work, uint32_t* batch)
{
    namespace rp = ramcrc_part;
    namespace rr = ramcrc_res;
    if (!t || n_seg >= 0xFFFFFFFFull || n_entries >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if ((n_seg && (!base || !status)) || (n_entries && (!entries || !work)))
        return RAMCRC_EINVAL;
    if (seg_stride && n_seg > UINT64_MAX / seg_stride)
        return RAMCRC_EINVAL;
    if (t->batches.size() >= t->max_batches)
        return RAMCRC_EINVAL;
    const uint64_t bno = t->batches.size();
    try {
        t->batches.push_back(ramcrc_replay_table_host::Batch{
            work, n_entries, 0, 0, 0, static_cast<const uint8_t*>(base), seg_stride, entries, false});
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    t->batches.back().key_hash = key_hash;
    if (batch)
        *batch = uint32_t(bno);
    if (t->spoiled)
        return RAMCRC_EINVAL;
    for (uint64_t i = 0; i < n_entries; i++)
        if (entries[i].segment >= n_seg) {
            t->spoiled = true;
            return RAMCRC_EINVAL;
        }
    struct Rd {
        const uint8_t* pay;
        uint32_t u8(uint32_t o) const { return pay[o]; }
        uint32_t u16(uint32_t o) const { return ld16(pay + o); }
        uint32_t u32(uint32_t o) const { return ld32(pay + o); }
        uint64_t u64(uint32_t o) const { return ld64(pay + o); }
    };
    ramcrc_replay_table_host::Batch& bt = t->batches.back();
    const uint8_t* const b = static_cast<const uint8_t*>(base);
    const uint64_t mask = t->slots.size() - 1;
    for (uint64_t i = 0; i < n_entries; i++) {
        const ramcrc_seg_entry& r = entries[i];
        const uint32_t type = r.header & 0x3f;
        work[i] = ~0ull;
        if (!(status[r.segment].flags & RAMCRC_SEG_OK))
            continue;
        const uint64_t pay = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
        const bool readable = !(r.header & RAMCRC_SEG_ENTRY_OVERLONG) && pay + r.length <= seg_stride;
        const Rd rd{b + r.segment * seg_stride + pay};
        if (type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION) {
            if (readable && r.length >= rr::kSafeVersionBytes && rd.u64(0) > t->safe_version)
                t->safe_version = rd.u64(0);
            continue;
        }
        if (!rr::resolved_type(type))
            continue;
        const rp::Parsed p = rp::parse(type, r.length, readable, rd);
        if (p.kind == rp::kMalformed) {
            bt.malformed++;
            continue;
        }
        const bool is_obj = type == RAMCRC_LOG_ENTRY_TYPE_OBJ;
        (is_obj ? bt.objects : bt.tombstones)++;
        const uint8_t* const key = rd.pay + p.key_off;
        const uint64_t version = rr::version(type, rd);
        const uint64_t rank = (uint64_t(is_obj) << 48) | (bno << 32) | i;
        const uint64_t hash = key_hash ? key_hash[i] : ramcrc::key_hash(p.table_id, key, p.key_len);
        uint64_t s = hash & mask, step = 0;
        for (; step <= mask; step++, s = (s + 1) & mask) {
            ramcrc_replay_table_host::Slot& sl = t->slots[s];
            if (!sl.claim) {
                sl.claim = (bno << 32) | (i + 1);
                sl.table_id = p.table_id;
                sl.key = key;
                sl.key_len = p.key_len;
                sl.version = version;
                sl.rank = rank;
                t->keys++;
                break;
            }
            if (sl.table_id != p.table_id || sl.key_len != p.key_len ||
                (p.key_len && memcmp(sl.key, key, p.key_len)))
                continue;
            if (rr::beats(version, rank, sl.version, sl.rank)) {
                sl.version = version;
                sl.rank = rank;
            }
            break;
        }
        if (step > mask) {   // no slot: the table is full
            t->spoiled = true;
            return RAMCRC_EINVAL;
        }
        work[i] = s;
    }
    if (t->keys > t->key_cap) {
        t->spoiled = true;
        return RAMCRC_EINVAL;
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_live_host(ramcrc_replay_table_host* t, uint32_t batch,
                                  ramcrc_replay_ref* winner, ramcrc_placement* live,
                                  uint64_t live_cap, uint64_t* n_live, ramcrc_resolve_counts* counts)
{
    if (!t || !n_live || !counts || live_cap >= 0xFFFFFFFFull || (live_cap && !live) ||
        batch >= t->batches.size() || t->batches[batch].retired)
        return RAMCRC_EINVAL;
    *n_live = 0;
    *counts = ramcrc_resolve_counts{0, 0, 0, 0, 0, 0};
    if (t->spoiled)
        return RAMCRC_OK;
    const ramcrc_replay_table_host::Batch& bt = t->batches[batch];
    ramcrc_resolve_counts ct{bt.objects, bt.tombstones, 0, 0, bt.malformed, t->safe_version};
    uint64_t nl = 0;
    for (uint64_t i = 0; i < bt.n; i++) {
        ramcrc_replay_ref w{0xFFFFFFFFu, 0xFFFFFFFFu};
        bool obj = false;
        if (bt.work[i] != ~0ull) {
            const uint64_t rank = t->slots[bt.work[i]].rank;
            w = ramcrc_replay_ref{uint32_t(rank >> 32) & 0xFFFFu, uint32_t(rank)};
            obj = (rank >> 48) & 1;
        }
        if (winner)
            winner[i] = w;
        if (w.batch != batch || w.record != i)
            continue;
        (obj ? ct.live_objects : ct.live_tombstones)++;
        if (nl < live_cap)
            live[nl] = ramcrc_placement{uint32_t(i), 0u};
        nl++;
    }
    *n_live = nl;
    *counts = ct;
    return RAMCRC_OK;
}

int ramcrc_replay_table_stats_host(ramcrc_replay_table_host* t, ramcrc_replay_table_stats* stats)
{
    if (!t || !stats)
        return RAMCRC_EINVAL;
    *stats = ramcrc_replay_table_stats{0, 0, 0, 0, 0, 0};
    if (t->spoiled) {
        stats->spoiled = 1;
        return RAMCRC_OK;
    }
    for (const ramcrc_replay_table_host::Slot& sl : t->slots) {
        if (!sl.claim)
            continue;
        stats->keys++;
        ((sl.rank >> 48) & 1 ? stats->live_objects : stats->live_tombstones)++;
    }
    stats->safe_version = t->safe_version;
    stats->batches = t->batches.size();
    return RAMCRC_OK;
}

// What the table holds for a key (the rules of lookup_rules.h): the add's
// probe without the writes, then the winner's record for the version and the
// value's place.  *pay and *pay_len: the winning object's payload.
namespace {
struct LookRd {
    const uint8_t* pay;
    uint32_t u8(uint32_t o) const { return pay[o]; }
    uint32_t u16(uint32_t o) const { return ld16(pay + o); }
    uint32_t u32(uint32_t o) const { return ld32(pay + o); }
    uint64_t u64(uint32_t o) const { return ld64(pay + o); }
};

ramcrc_lookup_result look_one(const ramcrc_replay_table_host* t, const uint8_t* kb, uint64_t keys_bytes,
                              const ramcrc_lookup_key& q, const uint64_t* hash_given,
                              const uint8_t** pay, uint32_t* pay_len, ramcrc_look::Value* value)
{
    namespace rl = ramcrc_look;
    if (rl::bad_query(q.key_off, q.key_len, q.reserved, keys_bytes))
        return rl::no_result(RAMCRC_LOOKUP_BAD_KEY);
    ramcrc_lookup_result res = rl::no_result(RAMCRC_LOOKUP_ABSENT);
    const uint64_t mask = t->slots.size() - 1;
    const uint8_t* const key = q.key_len ? kb + q.key_off : nullptr;
    const uint64_t hash = hash_given ? *hash_given : ramcrc::key_hash(q.table_id, key, q.key_len);
    uint64_t s = hash & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const ramcrc_replay_table_host::Slot& sl = t->slots[s];
        if (!sl.claim)
            break;
        if (sl.table_id != q.table_id || sl.key_len != q.key_len ||
            (q.key_len && memcmp(sl.key, key, q.key_len)))
            continue;
        const uint32_t wb = uint32_t(sl.rank >> 32) & 0xFFFFu, wr = uint32_t(sl.rank);
        const ramcrc_replay_table_host::Batch& bt = t->batches[wb];
        const ramcrc_seg_entry& r = bt.entries[wr];
        const uint32_t po = r.offset + 1 + ((r.header >> 6) & 3) + 1;
        res.ref = ramcrc_replay_ref{wb, wr};
        res.version = sl.version;
        if ((sl.rank >> 48) & 1) {
            const LookRd rd{bt.base + r.segment * bt.stride + po};
            const rl::Value v = rl::object_value(r.length, rd);
            res.kind = RAMCRC_LOOKUP_OBJECT;
            res.segment = r.segment;
            res.value_off = po + v.off;
            res.value_len = v.len;
            if (pay) {
                *pay = rd.pay;
                *pay_len = r.length;
                *value = v;
            }
        } else {
            res.kind = RAMCRC_LOOKUP_TOMBSTONE;
        }
        break;
    }
    return res;
}
}  // namespace

int ramcrc_replay_table_lookup_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* queries, uint64_t n_queries,
                                    const uint64_t* key_hash, ramcrc_lookup_result* results,
                                    ramcrc_lookup_counts* counts)
{
    if (!t || n_queries >= 0xFFFFFFFFull || (n_queries && (!queries || !results)) ||
        (keys_bytes && !keys))
        return RAMCRC_EINVAL;
    if (t->spoiled) {
        if (counts)
            *counts = ramcrc_lookup_counts{0, 0, 0, 0, 1};
        return RAMCRC_OK;
    }
    ramcrc_lookup_counts ct{0, 0, 0, 0, 0};
    const uint8_t* const kb = static_cast<const uint8_t*>(keys);
    for (uint64_t i = 0; i < n_queries; i++) {
        ramcrc_lookup_key q;   // (no alignment rule)
        memcpy(&q, reinterpret_cast<const uint8_t*>(queries) + i * sizeof(q), sizeof(q));
        const ramcrc_lookup_result res =
            look_one(t, kb, keys_bytes, q, key_hash ? key_hash + i : nullptr, nullptr, nullptr, nullptr);
        (res.kind == RAMCRC_LOOKUP_OBJECT ? ct.objects
         : res.kind == RAMCRC_LOOKUP_TOMBSTONE ? ct.tombstones
         : res.kind == RAMCRC_LOOKUP_ABSENT ? ct.absent : ct.bad)++;
        memcpy(reinterpret_cast<uint8_t*>(results) + i * sizeof(res), &res, sizeof(res));
    }
    if (counts)
        *counts = ct;
    return RAMCRC_OK;
}

// A multi-read's reply (the rules of read_rules.h): per query the lookup, the
// status, the part; the loop ends at the first part that does not fit.
int ramcrc_replay_table_read_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                  const ramcrc_lookup_key* queries, uint64_t n_queries,
                                  const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                  uint32_t flags, void* reply, uint64_t reply_cap,
                                  uint64_t* part_off, ramcrc_lookup_result* results,
                                  ramcrc_read_summary* summary)
{
    namespace rr = ramcrc_read;
    if (!t || n_queries >= 0xFFFFFFFFull || (flags & ~RAMCRC_READ_VALUE_ONLY) ||
        (n_queries && (!queries || !summary)) || (keys_bytes && !keys) || (reply_cap && !reply))
        return RAMCRC_EINVAL;
    if (!summary)
        return RAMCRC_OK;
    ramcrc_read_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        *summary = sm;
        return RAMCRC_OK;
    }
    const uint8_t* const kb = static_cast<const uint8_t*>(keys);
    uint8_t* const out = static_cast<uint8_t*>(reply);
    bool open = true;   // no part has failed to fit yet
    for (uint64_t i = 0; i < n_queries; i++) {
        ramcrc_lookup_key q;   // (no alignment rule)
        memcpy(&q, reinterpret_cast<const uint8_t*>(queries) + i * sizeof(q), sizeof(q));
        rr::Rules ru = rr::no_rules();
        if (rules) {
            const uint8_t* const p = reinterpret_cast<const uint8_t*>(rules) + i * sizeof(*rules);
            ru = rr::Rules{ld64(p), ld64(p + 8)};
        }
        const uint8_t* pay = nullptr;
        uint32_t pay_len = 0;
        ramcrc_look::Value v{0u, 0u};
        const ramcrc_lookup_result res =
            look_one(t, kb, keys_bytes, q, key_hash ? key_hash + i : nullptr, &pay, &pay_len, &v);
        if (results)
            memcpy(reinterpret_cast<uint8_t*>(results) + i * sizeof(res), &res, sizeof(res));
        uint64_t version = res.version;
        const uint32_t st = rr::status(rr::bad_rules(ru), res.kind, ru, &version);
        rr::Data d{0u, 0u};
        if (st == rr::kStatusOk)
            d = rr::data_range(flags, pay_len, v);
        const uint64_t size = rr::part_size(st, d.len);
        uint64_t at = RAMCRC_READ_NONE;
        if (open && size <= reply_cap - sm.reply_bytes) {
            at = sm.reply_bytes;
            uint64_t w[2];
            rr::header_words(st, version, d.len, &w[0], &w[1]);
            for (int b = 0; b < 16; b++)
                out[at + b] = uint8_t(w[b >> 3] >> (8 * (b & 7)));
            if (d.len)
                memcpy(out + at + rr::kPartHeader, pay + d.off, d.len);
            sm.returned++;
            sm.reply_bytes += size;
            if (st == rr::kStatusOk) {
                sm.ok++;
                sm.value_bytes += v.len;
                sm.key_bytes += rr::key_bytes(pay_len, v);
            } else {
                (st == rr::kStatusDoesntExist ? sm.doesnt_exist
                 : st == rr::kStatusExists ? sm.object_exists
                 : st == rr::kStatusWrongVersion ? sm.wrong_version : sm.bad)++;
            }
        } else {
            open = false;
        }
        if (part_off)
            memcpy(reinterpret_cast<uint8_t*>(part_off) + i * 8, &at, 8);
    }
    *summary = sm;
    return RAMCRC_OK;
}

// An indexed read's reply (the rules of read_hashes_rules.h): per asked hash
// the chain from its home slot, the matching keys' object winners in the order
// of their {batch, record}, the parts; the loop ends at the first hash that is
// not returned.
int ramcrc_replay_table_read_hashes_host(ramcrc_replay_table_host* t, uint64_t table_id,
                                         const uint64_t* hashes, uint64_t n_hashes, uint32_t flags,
                                         void* reply, uint64_t reply_capacity, uint64_t max_length,
                                         ramcrc_hash_part* parts, ramcrc_read_hashes_summary* summary)
{
    namespace rh = ramcrc_rh;
    if (!t || flags != 0 || !summary || n_hashes >= 0xFFFFFFFFull || (n_hashes && !hashes) ||
        (reply_capacity && !reply))
        return RAMCRC_EINVAL;
    ramcrc_read_hashes_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
        return RAMCRC_OK;
    }
    struct Obj {
        uint64_t order, version;
        const uint8_t* data;
        uint32_t len;
    };
    std::vector<Obj> objs;
    const uint64_t mask = t->slots.size() - 1;
    uint8_t* const out = static_cast<uint8_t*>(reply);
    bool open = true;   // every hash so far was returned
    try {
        for (uint64_t q = 0; q < n_hashes; q++) {
            uint64_t h;   // (no alignment rule)
            memcpy(&h, reinterpret_cast<const uint8_t*>(hashes) + q * 8, 8);
            rh::Found f = rh::nothing();
            objs.clear();
            uint64_t s = h & mask;
            for (uint64_t step = 0; open && step <= mask; step++, s = (s + 1) & mask) {
                const ramcrc_replay_table_host::Slot& sl = t->slots[s];
                if (!sl.claim)
                    break;
                if (sl.table_id != table_id)
                    continue;
                const ramcrc_replay_table_host::Batch& cb = t->batches[sl.claim >> 32];
                uint64_t rec_hash;   // the claimant's record hash
                if (cb.key_hash)
                    memcpy(&rec_hash, reinterpret_cast<const uint8_t*>(cb.key_hash) +
                                          ((sl.claim & 0xFFFFFFFFull) - 1) * 8, 8);
                else
                    rec_hash = ramcrc::key_hash(sl.table_id, sl.key, sl.key_len);
                if (rec_hash != h)
                    continue;
                if (!((sl.rank >> 48) & 1)) {
                    f.tombstones++;
                    continue;
                }
                const uint32_t wb = uint32_t(sl.rank >> 32) & 0xFFFFu, wr = uint32_t(sl.rank);
                const ramcrc_replay_table_host::Batch& bt = t->batches[wb];
                ramcrc_seg_entry r;   // (a survivor's table has no alignment rule)
                memcpy(&r, reinterpret_cast<const uint8_t*>(bt.entries) + uint64_t(wr) * sizeof(r), sizeof(r));
                const uint32_t po = r.offset + 1 + ((r.header >> 6) & 3) + 1;
                const LookRd rd{bt.base + r.segment * bt.stride + po};
                rh::add_object(&f, r.length, ramcrc_look::object_value(r.length, rd));
                objs.push_back(Obj{rh::order_of(wb, wr), sl.version, rd.pay + rh::kObjHeader,
                                   rh::data_len(r.length)});
            }
            ramcrc_hash_part part{RAMCRC_READ_NONE, 0u, 0u};
            if (open && rh::returned(sm.reply_bytes, sm.reply_bytes + f.bytes, max_length, reply_capacity)) {
                // one hash's objects: ascending {batch, record} (insertion sort:
                // more than one needs equal 64-bit hashes)
                for (size_t i = 1; i < objs.size(); i++)
                    for (size_t j = i; j > 0 && objs[j].order < objs[j - 1].order; j--)
                        std::swap(objs[j], objs[j - 1]);
                part.off = sm.reply_bytes;
                part.objects = uint32_t(f.objects);
                uint64_t at = sm.reply_bytes;
                for (const Obj& o : objs) {
                    for (uint32_t b = 0; b < rh::kPartHeader; b++)
                        out[at + b] = rh::header_byte(o.version, o.len, b);
                    if (o.len)
                        memcpy(out + at + rh::kPartHeader, o.data, o.len);
                    at += rh::kPartHeader + o.len;
                }
                rh::count_returned(&sm, f);
            } else if (open) {
                // the first hash that is not returned: its objects stay counted
                // in the reference's numObjects (:242 is not undone at :260)
                sm.objects_counted = f.objects;
                open = false;
            }
            if (parts)
                memcpy(reinterpret_cast<uint8_t*>(parts) + q * sizeof(part), &part, sizeof(part));
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.objects_counted += sm.objects;
    memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
    return RAMCRC_OK;
}

// One reply of an enumeration (the rules of enumerate_rules.h): bucket by
// bucket from the cursor the chain from the bucket's slot, the selected keys
// whose home the bucket is, their object winners in the order of {hash, batch,
// record}; the loop ends at the first bucket that is not kept whole.
int ramcrc_replay_table_enumerate_host(ramcrc_replay_table_host* t, uint64_t table_id,
                                       uint64_t first_hash, uint64_t last_hash, uint64_t bucket_index,
                                       uint64_t bucket_next_hash, uint64_t bucket_limit,
                                       const ramcrc_enum_frame* stale, uint32_t n_stale, uint32_t flags,
                                       void* payload, uint64_t payload_capacity, uint64_t max_bytes,
                                       ramcrc_enumerate_summary* summary)
{
    namespace en = ramcrc_en;
    if (!t || (flags & ~RAMCRC_ENUM_KEYS_ONLY) || !summary || (payload_capacity && !payload) ||
        n_stale > RAMCRC_ENUM_MAX_STALE || (n_stale && !stale))
        return RAMCRC_EINVAL;
    const uint64_t S = t->slots.size();
    if (bucket_index > S || (bucket_limit && (bucket_limit < bucket_index || bucket_limit > S)))
        return RAMCRC_EINVAL;
    en::Select sel{};
    sel.first_hash = first_hash;
    sel.last_hash = last_hash;
    sel.bucket_index = bucket_index;
    sel.bucket_next_hash = bucket_next_hash;
    sel.n_stale = n_stale;
    for (uint32_t k = 0; k < n_stale; k++) {
        memcpy(&sel.stale[k], reinterpret_cast<const uint8_t*>(stale) + k * sizeof(*stale), sizeof(*stale));
        if (en::bad_frame(sel.stale[k]))
            return RAMCRC_EINVAL;
    }
    ramcrc_enumerate_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
        return RAMCRC_OK;
    }
    struct Ent {
        uint64_t hash, order;
        const uint8_t* pay;
        uint32_t len;
        ramcrc_look::Value v;
    };
    std::vector<Ent> ents;
    const uint64_t mask = S - 1, lim = en::limit(max_bytes, payload_capacity);
    const uint64_t end = bucket_limit ? bucket_limit : S;
    uint8_t* const out = static_cast<uint8_t*>(payload);
    en::Found all = en::nothing();   // what is sent
    const auto send = [&](const Ent& e) {
        const uint32_t length = en::entry_length(flags, e.len, e.v);
        for (uint32_t b = 0; b < en::kLengthBytes; b++)
            out[all.bytes + b] = en::length_byte(length, b);
        memcpy(out + all.bytes + en::kLengthBytes, e.pay, length);
        en::add_object(&all, flags, e.len, e.v);
    };
    sm.num_buckets = S;
    sm.next_bucket = end;
    try {
        for (uint64_t b = bucket_index; b < end; b++) {
            ents.clear();
            en::Found f = en::nothing();
            uint64_t s = b;
            for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                const ramcrc_replay_table_host::Slot& sl = t->slots[s];
                if (!sl.claim)
                    break;
                if (sl.table_id != table_id)
                    continue;
                const ramcrc_replay_table_host::Batch& cb = t->batches[sl.claim >> 32];
                uint64_t h;   // the claimant's record hash
                if (cb.key_hash)
                    memcpy(&h, reinterpret_cast<const uint8_t*>(cb.key_hash) +
                                   ((sl.claim & 0xFFFFFFFFull) - 1) * 8, 8);
                else
                    h = ramcrc::key_hash(sl.table_id, sl.key, sl.key_len);
                if ((h & mask) != b || !en::selected(sel, b, h))
                    continue;
                if (!((sl.rank >> 48) & 1)) {
                    f.tombstones++;
                    continue;
                }
                const uint32_t wb = uint32_t(sl.rank >> 32) & 0xFFFFu, wr = uint32_t(sl.rank);
                const ramcrc_replay_table_host::Batch& bt = t->batches[wb];
                ramcrc_seg_entry r;   // (a survivor's table has no alignment rule)
                memcpy(&r, reinterpret_cast<const uint8_t*>(bt.entries) + uint64_t(wr) * sizeof(r), sizeof(r));
                const uint32_t po = r.offset + 1 + ((r.header >> 6) & 3) + 1;
                const LookRd rd{bt.base + r.segment * bt.stride + po};
                const ramcrc_look::Value v = ramcrc_look::object_value(r.length, rd);
                en::add_object(&f, flags, r.length, v);
                ents.push_back(Ent{h, en::order_of(wb, wr), rd.pay, r.length, v});
            }
            std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) {
                return en::below(x.hash, x.order, y.hash, y.order);
            });
            if (all.bytes + f.bytes <= lim) {   // kept whole
                for (const Ent& e : ents)
                    send(e);
                sm.tombstones += f.tombstones;
                continue;
            }
            sm.full = 1;
            sm.next_bucket = b;
            if (b == bucket_index) {   // (nothing was sent before it)
                en::Cut c = en::cut_begin();
                for (const Ent& e : ents)
                    if (!en::cut_entry(&c, lim, e.hash, flags, e.len, e.v))
                        break;
                sm.next_hash = c.next_hash;
                for (uint64_t k = 0; k < c.sent.objects; k++)
                    send(ents[k]);
                sm.stuck = c.sent.objects == 0;
            }
            break;
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.objects = all.objects;
    sm.payload_bytes = all.bytes;
    sm.value_bytes = all.value_bytes;
    sm.key_bytes = all.key_bytes;
    memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
    return RAMCRC_OK;
}

// A secondary index (the rules of index_rules.h): slot by slot the object
// winners of the table id, the key of the asked index, its copy; then
// std::stable_sort under the shared comparator.
extern "C++" {
namespace {
struct IxBytes {
    const uint8_t* p;
    uint32_t operator[](uint32_t i) const { return p[i]; }
};

ramcrc_ix::KeyRef<IxBytes> ix_ref(const ramcrc_index_entry& e, const uint8_t* keys)
{
    return ramcrc_ix::KeyRef<IxBytes>{e.prefix, e.key_len, IxBytes{keys + e.key_off + ramcrc_ix::kPrefixBytes}};
}

ramcrc_ix::KeyRef<IxBytes> ix_query_ref(const uint8_t* key, uint32_t len)
{
    return ramcrc_ix::KeyRef<IxBytes>{ramcrc_ix::prefix_of(IxBytes{key}, len), len,
                                      IxBytes{key + ramcrc_ix::kPrefixBytes}};
}
}  // namespace
}

int ramcrc_replay_table_index_build_host(ramcrc_replay_table_host* t, uint64_t table_id, uint32_t index_id,
                                         ramcrc_index_entry* entries, uint64_t entry_capacity,
                                         uint64_t* hashes, void* index_keys, uint64_t keys_capacity,
                                         ramcrc_index_build_summary* summary)
{
    namespace ix = ramcrc_ix;
    if (!t || !summary || index_id == 0 || entry_capacity >= 0xFFFFFFFFull ||
        (entry_capacity && (!entries || !hashes)) || (keys_capacity && !index_keys))
        return RAMCRC_EINVAL;
    ramcrc_index_build_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
        return RAMCRC_OK;
    }
    struct Found {
        const uint8_t* key;
        uint32_t len;
        uint64_t hash;
    };
    try {
        std::vector<Found> found;
        for (const ramcrc_replay_table_host::Slot& sl : t->slots) {
            if (!sl.claim || sl.table_id != table_id || !((sl.rank >> 48) & 1))
                continue;
            sm.objects_seen++;
            const uint32_t wb = uint32_t(sl.rank >> 32) & 0xFFFFu, wr = uint32_t(sl.rank);
            const ramcrc_replay_table_host::Batch& bt = t->batches[wb];
            ramcrc_seg_entry r;   // (a survivor's table has no alignment rule)
            memcpy(&r, reinterpret_cast<const uint8_t*>(bt.entries) + uint64_t(wr) * sizeof(r), sizeof(r));
            const uint32_t po = r.offset + 1 + ((r.header >> 6) & 3) + 1;
            const LookRd rd{bt.base + r.segment * bt.stride + po};
            const ix::KeyAt k = ix::key_at(r.length, rd, index_id);
            if (k.len == 0)
                continue;
            const ramcrc_replay_table_host::Batch& cb = t->batches[sl.claim >> 32];
            uint64_t h;   // the claimant's record hash
            if (cb.key_hash)
                memcpy(&h, reinterpret_cast<const uint8_t*>(cb.key_hash) + ((sl.claim & 0xFFFFFFFFull) - 1) * 8,
                       8);
            else
                h = ramcrc::key_hash(sl.table_id, sl.key, sl.key_len);
            found.push_back(Found{rd.pay + k.off, k.len, h});
            sm.key_bytes_needed += k.len;
        }
        sm.entries_needed = found.size();
        if (ix::overflow(sm.entries_needed, sm.key_bytes_needed, entry_capacity, keys_capacity)) {
            sm.overflow = 1;
            memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));
            return RAMCRC_OK;
        }
        uint8_t* const kb = static_cast<uint8_t*>(index_keys);
        std::vector<ramcrc_index_entry> es;
        es.reserve(found.size());
        uint64_t off = 0;
        for (const Found& f : found) {
            memcpy(kb + off, f.key, f.len);
            es.push_back(ix::make_entry(ix::prefix_of(IxBytes{f.key}, f.len), f.hash, off, f.len));
            off += f.len;
        }
        std::stable_sort(es.begin(), es.end(), [kb](const ramcrc_index_entry& x, const ramcrc_index_entry& y) {
            return ix::entry_less(ix_ref(x, kb), x.pk_hash, ix_ref(y, kb), y.pk_hash);
        });
        for (size_t i = 0; i < es.size(); i++) {
            memcpy(reinterpret_cast<uint8_t*>(entries) + i * sizeof(es[i]), &es[i], sizeof(es[i]));
            memcpy(reinterpret_cast<uint8_t*>(hashes) + i * 8, &es[i].pk_hash, 8);
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.n_entries = sm.entries_needed;
    sm.key_bytes = sm.key_bytes_needed;
    memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));
    return RAMCRC_OK;
}

// A batch of lookupIndexKeys (the rules of index_rules.h): per query the two
// binary searches; the loop stops serving at the first query whose hashes do
// not fit.
int ramcrc_index_lookup_host(const ramcrc_index_entry* entries, const uint64_t* hashes, const void* index_keys,
                             const ramcrc_index_build_summary* build_summary, const void* qkeys,
                             uint64_t qkeys_bytes, const ramcrc_index_query* queries, uint64_t n_queries,
                             uint64_t* out_hashes, uint64_t out_capacity, ramcrc_index_result* results,
                             ramcrc_index_lookup_summary* summary)
{
    namespace ix = ramcrc_ix;
    if (!build_summary || !summary || n_queries >= 0xFFFFFFFFull || (n_queries && (!queries || !results)) ||
        (qkeys_bytes && !qkeys) || (out_capacity && !out_hashes))
        return RAMCRC_EINVAL;
    ramcrc_index_build_summary bs;   // (no alignment rule)
    memcpy(&bs, reinterpret_cast<const uint8_t*>(build_summary), sizeof(bs));
    const bool dead = bs.overflow || bs.spoiled;
    const uint64_t n = dead ? 0 : bs.n_entries;
    const uint8_t* const kb = static_cast<const uint8_t*>(index_keys);
    const uint8_t* const qb = static_cast<const uint8_t*>(qkeys);
    const auto entry = [entries](uint64_t i) {
        ramcrc_index_entry e;
        memcpy(&e, reinterpret_cast<const uint8_t*>(entries) + i * sizeof(e), sizeof(e));
        return e;
    };
    ramcrc_index_lookup_summary sm{};
    sm.overflow_index = dead;
    sm.n_entries = n;
    bool open = !dead;   // every query so far was served
    for (uint64_t i = 0; i < n_queries; i++) {
        ramcrc_index_query q;
        memcpy(&q, reinterpret_cast<const uint8_t*>(queries) + i * sizeof(q), sizeof(q));
        ramcrc_index_result res = ix::no_result(RAMCRC_INDEX_NOT_SERVED);
        if (open && ix::bad_query(q, qkeys_bytes)) {
            res = ix::no_result(RAMCRC_INDEX_BAD_QUERY);
            sm.served++;
            sm.bad++;
        } else if (open) {
            const ix::KeyRef<IxBytes> first = ix_query_ref(qb + q.first_off, q.first_len);
            const ix::KeyRef<IxBytes> last = ix_query_ref(qb + q.last_off, q.last_len);
            const uint64_t lo = ix::first_false(n, [&](uint64_t m) {
                const ramcrc_index_entry e = entry(m);
                return ix::entry_less(ix_ref(e, kb), e.pk_hash, first, q.first_allowed_hash);
            });
            uint64_t hi = n;
            if (q.last_len)
                hi = ix::first_false(n, [&](uint64_t m) { return ix::key_compare(ix_ref(entry(m), kb), last) <= 0; });
            const ix::Answer an = ix::answer(lo, hi, q.max_hashes);
            if (ix::served(sm.hashes, an.num, out_capacity)) {
                res = ramcrc_index_result{sm.hashes, 0ull, 0ull, 0ull, an.num, 0u, RAMCRC_INDEX_OK, 0u};
                if (an.more) {
                    const ramcrc_index_entry e = entry(lo + an.num);
                    res.next_entry = lo + an.num;
                    res.next_key_hash = e.pk_hash;
                    res.next_key_off = e.key_off;
                    res.next_key_len = e.key_len;
                }
                if (an.num)
                    memcpy(reinterpret_cast<uint8_t*>(out_hashes) + sm.hashes * 8,
                           reinterpret_cast<const uint8_t*>(hashes) + lo * 8, uint64_t(an.num) * 8);
                sm.served++;
                sm.hashes += an.num;
                sm.maxed_out += an.more;
            } else {
                open = false;
            }
        }
        memcpy(reinterpret_cast<uint8_t*>(results) + i * sizeof(res), &res, sizeof(res));
    }
    memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));
    return RAMCRC_OK;
}

// A multi-write (the rules of write_rules.h): per request the first key, the
// duplicate test, the lookup, rejectOperation, the version, then the object and
// the tombstone of the object it replaces, appended to the one output.
int ramcrc_replay_table_write_host(ramcrc_replay_table_host* t, const void* data, uint64_t data_bytes,
                                   const ramcrc_write_req* reqs, uint64_t n_reqs,
                                   const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                   uint64_t next_version, uint32_t timestamp,
                                   const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                   ramcrc_seg_cert* out_cert, void* parts, ramcrc_write_ref* refs,
                                   ramcrc_lookup_result* old, ramcrc_write_summary* summary)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !summary || !out_cert ||
        (n_reqs && (!reqs || !parts)) || (data_bytes && !data) || (out_capacity && !out))
        return RAMCRC_EINVAL;
    ramcrc_write_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        *summary = sm;
        return RAMCRC_OK;
    }
    struct DataRd {
        const uint8_t* p;
        uint32_t u8(uint32_t o) const { return p[o]; }
        uint32_t u16(uint32_t o) const { return ld16(p + o); }
    };
    const uint8_t* const db = static_cast<const uint8_t*>(data);
    uint8_t* const ob = static_cast<uint8_t*>(out);
    std::unordered_set<std::string> seen;   // table id, then the key
    uint32_t meta = 0xFFFFFFFFu;            // the output's running metadata checksum
    uint64_t top = 0;                       // one past the highest version the tombstone rule gave
    bool open = true;                       // no request has failed to fit yet
    try {
        for (uint64_t i = 0; i < n_reqs; i++) {
            ramcrc_write_req q;   // (no alignment rule)
            memcpy(&q, reinterpret_cast<const uint8_t*>(reqs) + i * sizeof(q), sizeof(q));
            rr::Rules ru = rr::no_rules();
            if (rules) {
                const uint8_t* const p = reinterpret_cast<const uint8_t*>(rules) + i * sizeof(*rules);
                ru = rr::Rules{ld64(p), ld64(p + 8)};
            }
            uint32_t status = rr::kStatusFormatError;
            uint64_t version = 0;
            ramcrc_write_ref ref{rw::kNone, rw::kNone};
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            rw::Key key{false, 0u, 0u};
            if (!rw::bad_request(q.data_off, q.data_len, q.reserved, rr::bad_rules(ru), data_bytes))
                key = rw::first_key(q.data_len, DataRd{db + q.data_off});
            if (key.ok) {
                const uint8_t* const d = db + q.data_off;
                ramcrc_lookup_key lk{q.table_id, q.data_off + key.off, key.len, 0u};
                res = look_one(t, db, data_bytes, lk, key_hash ? key_hash + i : nullptr, nullptr,
                               nullptr, nullptr);
                std::string id(reinterpret_cast<const char*>(&q.table_id), 8);
                id.append(reinterpret_cast<const char*>(d + key.off), key.len);
                if (!seen.insert(id).second) {
                    status = rw::kStatusRetry;   // a later request of a key of this call
                    sm.retry_duplicate++;
                } else {
                    const bool obj = res.kind == RAMCRC_LOOKUP_OBJECT;
                    const bool tomb = res.kind == RAMCRC_LOOKUP_TOMBSTONE;
                    const uint64_t cur = obj ? res.version : 0;
                    status = rr::reject(ru, cur);
                    version = cur;
                    if (status == rr::kStatusOk) {
                        const uint64_t a = next_version + sm.allocated;
                        const uint64_t v = rw::new_version(cur, tomb, res.version, a);
                        if (cur == 0) {
                            sm.allocated++;
                            if (v != a && v + 1 > top)
                                top = v + 1;
                        }
                        const bool with_tomb = cur != 0;
                        const uint64_t size = rw::request_size(q.data_len, with_tomb, key.len);
                        if (open && size <= out_capacity - sm.out_bytes) {
                            uint8_t* e = ob + sm.out_bytes;
                            const uint32_t olen = rw::kObjHeader + q.data_len;
                            uint32_t nm;
                            uint64_t m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJ, olen, &nm);
                            ref.object_off = uint32_t(sm.out_bytes);
                            for (uint32_t b = 0; b < nm; b++)
                                e[b] = uint8_t(m >> (8 * b));
                            meta = ramcrc_update(meta, e, nm);
                            e += nm;
                            for (uint32_t b = 4; b < rw::kObjHeader; b++)
                                e[b] = uint8_t(rw::obj_header_byte(b, timestamp, v, q.table_id));
                            memcpy(e + rw::kObjHeader, d, q.data_len);
                            const uint32_t ck = ~ramcrc_update(0xFFFFFFFFu, e + 4, olen - 4);
                            for (int b = 0; b < 4; b++)
                                e[b] = uint8_t(ck >> (8 * b));
                            e += olen;
                            if (with_tomb) {
                                const uint32_t tlen = rw::kTombHeader + key.len;
                                const uint64_t seg_id =
                                    batch_segment_id ? batch_segment_id[res.ref.batch] + res.segment : 0ull;
                                m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, tlen, &nm);
                                ref.tombstone_off = uint32_t(e - ob);
                                for (uint32_t b = 0; b < nm; b++)
                                    e[b] = uint8_t(m >> (8 * b));
                                meta = ramcrc_update(meta, e, nm);
                                e += nm;
                                for (uint32_t b = 0; b < 28; b++)
                                    e[b] = uint8_t(rw::tomb_header_byte(b, q.table_id, seg_id, cur, timestamp));
                                if (key.len)
                                    memcpy(e + rw::kTombHeader, d + key.off, key.len);
                                uint32_t tk = ramcrc_update(0xFFFFFFFFu, e, 28);
                                tk = ~ramcrc_update(tk, e + rw::kTombHeader, key.len);
                                for (int b = 0; b < 4; b++)
                                    e[28 + b] = uint8_t(tk >> (8 * b));
                                sm.tombstones++;
                                sm.tombstone_bytes += tlen;
                            }
                            const uint32_t vl = rw::value_len(q.data_len, DataRd{d});
                            sm.ok++;
                            sm.out_bytes += size;
                            sm.object_bytes += olen;
                            sm.value_bytes += vl;
                            sm.key_bytes += q.data_len - vl;
                            version = v;
                        } else {
                            open = false;
                            status = rw::kStatusRetry;   // "Must wait for cleaner"
                            sm.retry_full++;
                        }
                    } else {
                        (status == rr::kStatusDoesntExist ? sm.doesnt_exist
                         : status == rr::kStatusExists ? sm.object_exists : sm.wrong_version)++;
                    }
                }
            } else {
                sm.bad++;
            }
            uint8_t* const p = static_cast<uint8_t*>(parts) + i * rw::kPartBytes;
            memcpy(p, &status, 4);
            memcpy(p + 4, &version, 8);
            if (refs)
                memcpy(reinterpret_cast<uint8_t*>(refs) + i * sizeof(ref), &ref, sizeof(ref));
            if (old)
                memcpy(reinterpret_cast<uint8_t*>(old) + i * sizeof(res), &res, sizeof(res));
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.next_version = next_version + sm.allocated > top ? next_version + sm.allocated : top;
    const uint32_t head = uint32_t(sm.out_bytes);
    uint8_t lenle[4];
    for (int b = 0; b < 4; b++)
        lenle[b] = uint8_t(head >> (8 * b));
    *out_cert = ramcrc_seg_cert{head, ~ramcrc_update(meta, lenle, 4)};   // Segment::getAppendedLength
    *summary = sm;
    return RAMCRC_OK;
}

// A multi-remove (the rules of remove_rules.h): per request the duplicate
// test, the lookup, rejectOperation, then the tombstone of the object it
// removes, appended to the one output.
int ramcrc_replay_table_remove_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* reqs, uint64_t n_reqs,
                                    const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                    uint64_t next_version, uint32_t timestamp,
                                    const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                    ramcrc_seg_cert* out_cert, void* parts, uint32_t* refs,
                                    ramcrc_lookup_result* old, ramcrc_remove_summary* summary)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    namespace rm = ramcrc_remove;
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !summary || !out_cert ||
        (n_reqs && (!reqs || !parts)) || (keys_bytes && !keys) || (out_capacity && !out))
        return RAMCRC_EINVAL;
    ramcrc_remove_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        *summary = sm;
        return RAMCRC_OK;
    }
    const uint8_t* const kb = static_cast<const uint8_t*>(keys);
    uint8_t* const ob = static_cast<uint8_t*>(out);
    std::unordered_set<std::string> seen;   // table id, then the key
    uint32_t meta = 0xFFFFFFFFu;            // the output's running metadata checksum
    uint64_t top = 0;                       // the highest version among the written tombstones
    bool open = true;                       // no request has failed to fit yet
    try {
        for (uint64_t i = 0; i < n_reqs; i++) {
            ramcrc_lookup_key q;   // (no alignment rule)
            memcpy(&q, reinterpret_cast<const uint8_t*>(reqs) + i * sizeof(q), sizeof(q));
            rr::Rules ru = rr::no_rules();
            if (rules) {
                const uint8_t* const p = reinterpret_cast<const uint8_t*>(rules) + i * sizeof(*rules);
                ru = rr::Rules{ld64(p), ld64(p + 8)};
            }
            uint32_t status = rr::kStatusFormatError;
            uint64_t version = 0;
            uint32_t ref = rm::kNone;
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            if (!rm::bad_request(q.key_off, q.key_len, q.reserved, rr::bad_rules(ru), keys_bytes)) {
                const uint8_t* const key = kb + q.key_off;
                res = look_one(t, kb, keys_bytes, q, key_hash ? key_hash + i : nullptr, nullptr, nullptr,
                               nullptr);
                std::string id(reinterpret_cast<const char*>(&q.table_id), 8);
                if (q.key_len)
                    id.append(reinterpret_cast<const char*>(key), q.key_len);
                if (!seen.insert(id).second) {
                    status = rm::kStatusRetry;   // a later request of a key of this call
                    sm.retry_duplicate++;
                } else {
                    const rm::Outcome o = rm::outcome(res.kind, res.version, ru);
                    status = o.status;
                    version = o.version;
                    if (o.reach) {
                        const uint64_t size = rm::tomb_size(q.key_len);
                        if (open && size <= out_capacity - sm.out_bytes) {
                            uint8_t* e = ob + sm.out_bytes;
                            const uint32_t tlen = rm::tomb_len(q.key_len);
                            const uint64_t seg_id =
                                batch_segment_id ? batch_segment_id[res.ref.batch] + res.segment : 0ull;
                            uint32_t nm;
                            const uint64_t m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, tlen, &nm);
                            ref = uint32_t(sm.out_bytes);
                            for (uint32_t b = 0; b < nm; b++)
                                e[b] = uint8_t(m >> (8 * b));
                            meta = ramcrc_update(meta, e, nm);
                            e += nm;
                            for (uint32_t b = 0; b < 28; b++)
                                e[b] = uint8_t(rw::tomb_header_byte(b, q.table_id, seg_id, o.version, timestamp));
                            if (q.key_len)
                                memcpy(e + rm::kTombHeader, key, q.key_len);
                            uint32_t tk = ramcrc_update(0xFFFFFFFFu, e, 28);
                            tk = ~ramcrc_update(tk, e + rm::kTombHeader, q.key_len);
                            for (int b = 0; b < 4; b++)
                                e[28 + b] = uint8_t(tk >> (8 * b));
                            sm.removed++;
                            sm.out_bytes += size;
                            sm.tombstone_bytes += tlen;
                            if (o.version > top)
                                top = o.version;
                        } else {
                            open = false;
                            status = rm::kStatusRetry;   // "Must wait for cleaner"
                            sm.retry_full++;
                        }
                    } else {
                        (status == rr::kStatusDoesntExist ? sm.doesnt_exist
                         : status == rr::kStatusExists ? sm.object_exists
                         : status == rr::kStatusWrongVersion ? sm.wrong_version : sm.ok_absent)++;
                    }
                }
            } else {
                sm.bad++;
            }
            uint8_t* const p = static_cast<uint8_t*>(parts) + i * rm::kPartBytes;
            memcpy(p, &status, 4);
            memcpy(p + 4, &version, 8);
            if (refs)
                memcpy(reinterpret_cast<uint8_t*>(refs) + i * sizeof(ref), &ref, sizeof(ref));
            if (old)
                memcpy(reinterpret_cast<uint8_t*>(old) + i * sizeof(res), &res, sizeof(res));
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.next_version = rm::next_version(next_version, top);
    const uint32_t head = uint32_t(sm.out_bytes);
    uint8_t lenle[4];
    for (int b = 0; b < 4; b++)
        lenle[b] = uint8_t(head >> (8 * b));
    *out_cert = ramcrc_seg_cert{head, ~ramcrc_update(meta, lenle, 4)};   // Segment::getAppendedLength
    *summary = sm;
    return RAMCRC_OK;
}

// A multi-increment (the rules of increment_rules.h): per request the
// duplicate test, the lookup, rejectOperation, the length test and the sum;
// then the write's version, object and tombstone (write_rules.h) for the image
// of the new value, appended to the one output.
int ramcrc_replay_table_increment_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                       const ramcrc_lookup_key* reqs, uint64_t n_reqs,
                                       const ramcrc_increment_arg* args,
                                       const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                       uint64_t next_version, uint32_t timestamp,
                                       const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                       ramcrc_seg_cert* out_cert, void* parts, ramcrc_write_ref* refs,
                                       ramcrc_lookup_result* old, ramcrc_increment_summary* summary)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    namespace ri = ramcrc_increment;
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !summary || !out_cert ||
        (n_reqs && (!reqs || !args || !parts)) || (keys_bytes && !keys) || (out_capacity && !out))
        return RAMCRC_EINVAL;
    ramcrc_increment_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        *summary = sm;
        return RAMCRC_OK;
    }
    const uint8_t* const kb = static_cast<const uint8_t*>(keys);
    uint8_t* const ob = static_cast<uint8_t*>(out);
    std::unordered_set<std::string> seen;   // table id, then the key
    uint32_t meta = 0xFFFFFFFFu;            // the output's running metadata checksum
    uint64_t top = 0;                       // one past the highest version the tombstone rule gave
    bool open = true;                       // no request has failed to fit yet
    try {
        for (uint64_t i = 0; i < n_reqs; i++) {
            ramcrc_lookup_key q;   // (no alignment rule)
            memcpy(&q, reinterpret_cast<const uint8_t*>(reqs) + i * sizeof(q), sizeof(q));
            const uint8_t* const ap = reinterpret_cast<const uint8_t*>(args) + i * sizeof(*args);
            const uint64_t add_int = ld64(ap), add_dbl = ld64(ap + 8);
            rr::Rules ru = rr::no_rules();
            if (rules) {
                const uint8_t* const p = reinterpret_cast<const uint8_t*>(rules) + i * sizeof(*rules);
                ru = rr::Rules{ld64(p), ld64(p + 8)};
            }
            uint32_t status = rr::kStatusFormatError;
            uint64_t version = 0, bits = 0;
            ramcrc_write_ref ref{rw::kNone, rw::kNone};
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            if (!ri::bad_request(q.key_off, q.key_len, q.reserved, rr::bad_rules(ru), keys_bytes)) {
                const uint8_t* const key = kb + q.key_off;
                const uint8_t* pay = nullptr;
                uint32_t pay_len = 0;
                ramcrc_look::Value val{0u, 0u};
                res = look_one(t, kb, keys_bytes, q, key_hash ? key_hash + i : nullptr, &pay, &pay_len, &val);
                std::string id(reinterpret_cast<const char*>(&q.table_id), 8);
                if (q.key_len)
                    id.append(reinterpret_cast<const char*>(key), q.key_len);
                if (!seen.insert(id).second) {
                    status = ri::kStatusRetry;   // a later request of a key of this call
                    sm.retry_duplicate++;
                } else {
                    const bool obj = res.kind == RAMCRC_LOOKUP_OBJECT;
                    const ri::Outcome o = ri::outcome(res.kind, res.version, obj ? res.value_len : 0u, ru);
                    const uint64_t cur = o.cur;
                    status = o.status;
                    version = cur;
                    if (o.reach) {
                        bits = ri::sum(obj ? ld64(pay + val.off) : 0ull, add_int, add_dbl);
                        const uint32_t dl = ri::image_len(q.key_len);
                        const uint64_t a = next_version + sm.allocated;
                        const uint64_t v =
                            rw::new_version(cur, res.kind == RAMCRC_LOOKUP_TOMBSTONE, res.version, a);
                        if (cur == 0) {
                            sm.allocated++;
                            if (v != a && v + 1 > top)
                                top = v + 1;
                        }
                        const bool with_tomb = cur != 0;
                        const uint64_t size = rw::request_size(dl, with_tomb, q.key_len);
                        if (open && size <= out_capacity - sm.out_bytes) {
                            uint8_t* e = ob + sm.out_bytes;
                            const uint32_t olen = rw::kObjHeader + dl;
                            uint32_t nm;
                            uint64_t m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJ, olen, &nm);
                            ref.object_off = uint32_t(sm.out_bytes);
                            for (uint32_t b = 0; b < nm; b++)
                                e[b] = uint8_t(m >> (8 * b));
                            meta = ramcrc_update(meta, e, nm);
                            e += nm;
                            const auto key_byte = [key](uint32_t k) { return uint32_t(key[k]); };
                            for (uint32_t b = 4; b < olen; b++)
                                e[b] = uint8_t(ri::object_byte(b - 4, q.key_len, timestamp, v, q.table_id, bits,
                                                               key_byte));
                            const uint32_t ck = ~ramcrc_update(0xFFFFFFFFu, e + 4, olen - 4);
                            for (int b = 0; b < 4; b++)
                                e[b] = uint8_t(ck >> (8 * b));
                            e += olen;
                            if (with_tomb) {
                                const uint32_t tlen = rw::kTombHeader + q.key_len;
                                const uint64_t seg_id =
                                    batch_segment_id ? batch_segment_id[res.ref.batch] + res.segment : 0ull;
                                m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, tlen, &nm);
                                ref.tombstone_off = uint32_t(e - ob);
                                for (uint32_t b = 0; b < nm; b++)
                                    e[b] = uint8_t(m >> (8 * b));
                                meta = ramcrc_update(meta, e, nm);
                                e += nm;
                                for (uint32_t b = 0; b < 28; b++)
                                    e[b] = uint8_t(rw::tomb_header_byte(b, q.table_id, seg_id, cur, timestamp));
                                if (q.key_len)
                                    memcpy(e + rw::kTombHeader, key, q.key_len);
                                uint32_t tk = ramcrc_update(0xFFFFFFFFu, e, 28);
                                tk = ~ramcrc_update(tk, e + rw::kTombHeader, q.key_len);
                                for (int b = 0; b < 4; b++)
                                    e[28 + b] = uint8_t(tk >> (8 * b));
                                sm.tombstones++;
                                sm.tombstone_bytes += tlen;
                            } else {
                                sm.created++;
                            }
                            sm.ok++;
                            sm.out_bytes += size;
                            sm.object_bytes += olen;
                            sm.value_bytes += ri::kValueBytes;
                            sm.key_bytes += dl - ri::kValueBytes;
                            version = v;
                        } else {
                            open = false;
                            status = ri::kStatusRetry;   // "Must wait for cleaner"
                            sm.retry_full++;
                        }
                    } else {
                        (status == rr::kStatusDoesntExist ? sm.doesnt_exist
                         : status == rr::kStatusExists ? sm.object_exists
                         : status == rr::kStatusWrongVersion ? sm.wrong_version : sm.invalid_object)++;
                    }
                }
            } else {
                sm.bad++;
            }
            const uint64_t third = ri::part_value(status, bits, add_dbl);
            uint8_t* const p = static_cast<uint8_t*>(parts) + i * ri::kPartBytes;
            memcpy(p, &status, 4);
            memcpy(p + 4, &version, 8);
            memcpy(p + 12, &third, 8);
            if (refs)
                memcpy(reinterpret_cast<uint8_t*>(refs) + i * sizeof(ref), &ref, sizeof(ref));
            if (old)
                memcpy(reinterpret_cast<uint8_t*>(old) + i * sizeof(res), &res, sizeof(res));
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    sm.next_version = next_version + sm.allocated > top ? next_version + sm.allocated : top;
    const uint32_t head = uint32_t(sm.out_bytes);
    uint8_t lenle[4];
    for (int b = 0; b < 4; b++)
        lenle[b] = uint8_t(head >> (8 * b));
    *out_cert = ramcrc_seg_cert{head, ~ramcrc_update(meta, lenle, 4)};   // Segment::getAppendedLength
    *summary = sm;
    return RAMCRC_OK;
}

// Cleaning (the rules of clean_rules.h): a pass over the victims' records for
// the usage and the summary; then, for clean, the copy of the live entries
// with their rows, the winners' new ranks, and the claims that named a victim.
namespace {
int clean_host(ramcrc_replay_table_host* t, const uint32_t* victims, uint32_t n_victims, bool size_only,
               void* out, uint32_t out_capacity, ramcrc_seg_cert* out_cert, ramcrc_seg_status* out_status,
               ramcrc_seg_entry* out_entries, uint64_t out_entries_cap, uint64_t* out_n_entries,
               uint64_t* out_work, ramcrc_replay_ref* moved, ramcrc_clean_usage* usage,
               ramcrc_clean_summary* summary, uint32_t* batch)
{
    namespace cl = ramcrc_clean;
    typedef ramcrc_replay_table_host::Batch Batch;
    if (!t || !victims || !summary || n_victims == 0)
        return RAMCRC_EINVAL;
    if (!size_only &&
        (!out_cert || !out_status || !out_n_entries || (out_entries_cap && (!out_entries || !out_work)) ||
         (out_capacity && !out) || (out_capacity & 15) || out_entries_cap >= 0x100000000ull ||
         t->batches.size() >= t->max_batches))
        return RAMCRC_EINVAL;
    try {
        std::vector<uint8_t> seen(t->batches.size(), 0);
        for (uint32_t v = 0; v < n_victims; v++) {
            const uint32_t b = victims[v];
            if (b >= t->batches.size() || t->batches[b].retired || seen[b])
                return RAMCRC_EINVAL;
            seen[b] = 1;
        }
        if (!size_only)
            t->batches.reserve(t->batches.size() + 1);
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    ramcrc_clean_summary sm{};
    const uint32_t N = uint32_t(t->batches.size());
    if (!size_only) {
        // the number is taken and the victims are retired whatever follows
        for (uint32_t v = 0; v < n_victims; v++)
            t->batches[victims[v]].retired = true;
        t->batches.push_back(Batch{out_work, 0, 0, 0, 0, static_cast<const uint8_t*>(out), out_capacity,
                                   out_entries, false});
        if (batch)
            *batch = N;
    }
    if (t->spoiled) {
        sm.spoiled = 1;
        *summary = sm;
        return RAMCRC_OK;
    }
    for (uint32_t v = 0; v < n_victims; v++) {
        const uint32_t b = victims[v];
        const Batch& bt = t->batches[b];
        ramcrc_clean_usage u{bt.n, 0, 0, 0};
        for (uint64_t i = 0; i < bt.n; i++) {
            const ramcrc_seg_entry& r = bt.entries[i];
            const uint64_t w = bt.work[i];
            const uint64_t rank = w != cl::kNoSlot ? t->slots[w].rank : 0ull;
            switch (cl::classify(w, rank, b, i, r.header)) {
            case cl::kLiveObject:
                u.live_objects++;
                u.live_bytes += cl::entry_bytes(r.header, r.length);
                sm.object_bytes += r.length;
                break;
            case cl::kLiveTombstone:
                u.live_tombstones++;
                u.live_bytes += cl::entry_bytes(r.header, r.length);
                sm.tombstone_bytes += r.length;
                break;
            case cl::kDroppedObject:
                sm.dropped_objects++;
                break;
            case cl::kDroppedTombstone:
                sm.dropped_tombstones++;
                break;
            default:
                sm.dropped_other++;
            }
        }
        sm.records += u.records;
        sm.moved_objects += u.live_objects;
        sm.moved_tombstones += u.live_tombstones;
        sm.needed_bytes += u.live_bytes;
        if (usage)
            memcpy(reinterpret_cast<uint8_t*>(usage) + v * sizeof(u), &u, sizeof(u));
    }
    sm.victims = n_victims;
    sm.needed_records = sm.moved_objects + sm.moved_tombstones;
    sm.out_bytes = sm.needed_bytes;
    if (size_only) {
        *summary = sm;
        return RAMCRC_OK;
    }
    if (!cl::fits(sm.needed_bytes, sm.needed_records, out_capacity, out_entries_cap)) {
        ramcrc_clean_summary no{};
        no.needed_bytes = sm.needed_bytes;
        no.needed_records = sm.needed_records;
        no.spoiled = 1;
        *summary = no;
        t->spoiled = true;
        return RAMCRC_EINVAL;
    }
    sm.batch = N;
    uint8_t* const ob = static_cast<uint8_t*>(out);
    uint32_t meta = 0xFFFFFFFFu;   // the survivor's running metadata checksum
    uint64_t head = 0, j = 0;
    for (uint32_t v = 0; v < n_victims; v++) {
        const uint32_t b = victims[v];
        const Batch& bt = t->batches[b];
        for (uint64_t i = 0; i < bt.n; i++) {
            const ramcrc_seg_entry& r = bt.entries[i];
            const uint64_t w = bt.work[i];
            if (w == cl::kNoSlot || !cl::live(w, t->slots[w].rank, b, i))
                continue;
            const uint64_t size = cl::entry_bytes(r.header, r.length);
            const uint8_t* const src = bt.base + r.segment * bt.stride + r.offset;
            memcpy(ob + head, src, size);
            meta = ramcrc_update(meta, src, cl::meta_bytes(r.header));
            const ramcrc_seg_entry row{0u, uint32_t(head), r.length, r.header};
            memcpy(reinterpret_cast<uint8_t*>(out_entries) + j * sizeof(row), &row, sizeof(row));
            memcpy(reinterpret_cast<uint8_t*>(out_work) + j * sizeof(w), &w, sizeof(w));
            if (moved) {
                const ramcrc_replay_ref old{b, uint32_t(i)};
                memcpy(reinterpret_cast<uint8_t*>(moved) + j * sizeof(old), &old, sizeof(old));
            }
            t->slots[w].rank =
                cl::rank_of((r.header & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ, N, j);
            head += size;
            j++;
        }
    }
    Batch& nb = t->batches[N];
    nb.n = j;
    nb.objects = sm.moved_objects;
    nb.tombstones = sm.moved_tombstones;
    // every winner names a batch that stays: the claims that named a victim
    for (uint32_t v = 0; v < n_victims; v++) {
        const uint32_t b = victims[v];
        const Batch& bt = t->batches[b];
        for (uint64_t i = 0; i < bt.n; i++) {
            const uint64_t w = bt.work[i];
            if (w == cl::kNoSlot || t->slots[w].claim != cl::claim_of(b, i))
                continue;
            ramcrc_replay_table_host::Slot& sl = t->slots[w];
            sl.claim = cl::claim_after(sl.rank);
            const Batch& wb = t->batches[cl::claim_batch(sl.claim)];
            ramcrc_seg_entry r;   // (the survivor's table has no alignment rule)
            memcpy(&r, reinterpret_cast<const uint8_t*>(wb.entries) + cl::claim_record(sl.claim) * sizeof(r),
                   sizeof(r));
            const uint64_t pay = uint64_t(r.offset) + 1 + ((r.header >> 6) & 3) + 1;
            const LookRd rd{wb.base + r.segment * wb.stride + pay};
            const ramcrc_part::Parsed p = ramcrc_part::parse(r.header & 0x3f, r.length, true, rd);
            sl.key = rd.pay + p.key_off;   // the same key, in a batch that stays
        }
    }
    uint8_t lenle[4];
    for (int k = 0; k < 4; k++)
        lenle[k] = uint8_t(uint32_t(head) >> (8 * k));
    const ramcrc_seg_cert cert{uint32_t(head), ~ramcrc_update(meta, lenle, 4)};   // Segment::getAppendedLength
    const ramcrc_seg_status st{RAMCRC_SEG_OK, cert.checksum, uint32_t(j), 0u};
    memcpy(out_cert, &cert, sizeof(cert));
    memcpy(out_status, &st, sizeof(st));
    memcpy(out_n_entries, &j, sizeof(j));
    *summary = sm;
    return RAMCRC_OK;
}
}  // namespace

int ramcrc_replay_table_clean_size_host(ramcrc_replay_table_host* t, const uint32_t* victims,
                                        uint32_t n_victims, ramcrc_clean_usage* usage,
                                        ramcrc_clean_summary* summary)
{
    return clean_host(t, victims, n_victims, true, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr,
                      nullptr, nullptr, usage, summary, nullptr);
}

int ramcrc_replay_table_clean_host(ramcrc_replay_table_host* t, const uint32_t* victims,
                                   uint32_t n_victims, void* out, uint32_t out_capacity,
                                   ramcrc_seg_cert* out_cert, ramcrc_seg_status* out_status,
                                   ramcrc_seg_entry* out_entries, uint64_t out_entries_cap,
                                   uint64_t* out_n_entries, uint64_t* out_work,
                                   ramcrc_replay_ref* moved, ramcrc_clean_usage* usage,
                                   ramcrc_clean_summary* summary, uint32_t* batch)
{
    return clean_host(t, victims, n_victims, false, out, out_capacity, out_cert, out_status, out_entries,
                      out_entries_cap, out_n_entries, out_work, moved, usage, summary, batch);
}

// A tablet migration (the rules of migrate_rules.h): the listed batches'
// records in order from the cursor, each classified, the sent ones appended to
// the current output until one closes it.
int ramcrc_replay_table_migrate_host(ramcrc_replay_table_host* t, const uint32_t* batches,
                                     uint32_t n_batches, uint64_t table_id, uint64_t first_hash,
                                     uint64_t last_hash, uint32_t flags, uint32_t start_index,
                                     uint32_t start_record, void* out, uint32_t out_capacity,
                                     uint64_t out_stride, uint32_t max_segments,
                                     ramcrc_seg_cert* out_certs, ramcrc_migrate_count* out_counts,
                                     ramcrc_replay_ref* sent, uint64_t sent_cap, uint64_t* seg_first,
                                     ramcrc_migrate_summary* summary)
{
    namespace mg = ramcrc_mig;
    namespace cl = ramcrc_clean;
    typedef ramcrc_replay_table_host::Batch Batch;
    if (!t || !batches || !summary || n_batches == 0 || (flags & ~mg::kKnownFlags))
        return RAMCRC_EINVAL;
    if ((out_capacity & 15) || (out_stride & 15) || out_stride < out_capacity ||
        out_capacity > RAMCRC_MIGRATE_MAX_CAPACITY || max_segments > RAMCRC_MIGRATE_MAX_SEGMENTS ||
        (max_segments && (!out_certs || !out_counts || (out_capacity && !out))) || (sent_cap && !sent) ||
        start_index > n_batches || (start_index == n_batches && start_record))
        return RAMCRC_EINVAL;
    try {
        std::vector<uint8_t> seen(t->batches.size(), 0);
        for (uint32_t v = 0; v < n_batches; v++) {
            const uint32_t b = batches[v];
            if (b >= t->batches.size() || t->batches[b].retired || seen[b])
                return RAMCRC_EINVAL;
            seen[b] = 1;
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    if (start_index < n_batches && start_record > t->batches[batches[start_index]].n)
        return RAMCRC_EINVAL;
    ramcrc_migrate_summary sm{};
    if (t->spoiled) {
        sm.spoiled = 1;
        memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
        return RAMCRC_OK;
    }
    uint8_t* const ob = static_cast<uint8_t*>(out);
    bool open = false;           // output segments_used - 1 takes entries
    uint64_t head = 0;
    uint32_t meta = 0;           // its running header checksum
    ramcrc_migrate_count cnt{};
    const auto seal = [&]() {
        uint8_t lenle[4];
        for (int k = 0; k < 4; k++)
            lenle[k] = uint8_t(uint32_t(head) >> (8 * k));
        const ramcrc_seg_cert cert{uint32_t(head), ~ramcrc_update(meta, lenle, 4)};   // Segment::getAppendedLength
        const uint64_t k = sm.segments_used - 1;
        memcpy(reinterpret_cast<uint8_t*>(out_certs) + k * sizeof(cert), &cert, sizeof(cert));
        memcpy(reinterpret_cast<uint8_t*>(out_counts) + k * sizeof(cnt), &cnt, sizeof(cnt));
    };
    sm.next_index = n_batches;
    sm.done = 1;
    for (uint32_t v = start_index; v < n_batches && sm.done; v++) {
        const uint32_t b = batches[v];
        const Batch& bt = t->batches[b];
        for (uint64_t i = v == start_index ? start_record : 0; i < bt.n; i++) {
            ramcrc_seg_entry r;   // (a survivor's table has no alignment rule)
            memcpy(&r, reinterpret_cast<const uint8_t*>(bt.entries) + i * sizeof(r), sizeof(r));
            uint64_t w;
            memcpy(&w, reinterpret_cast<const uint8_t*>(bt.work) + i * sizeof(w), sizeof(w));
            const bool part = w != cl::kNoSlot;
            const uint32_t po = r.offset + 1 + ((r.header >> 6) & 3) + 1;
            const LookRd rd{bt.base + r.segment * bt.stride + po};
            uint64_t table = 0, hash = 0;
            bool winner = false;
            if (part) {
                const ramcrc_part::Parsed p = ramcrc_part::parse(r.header & 0x3f, r.length, true, rd);
                table = p.table_id;
                if (table == table_id) {
                    if (bt.key_hash)
                        memcpy(&hash, reinterpret_cast<const uint8_t*>(bt.key_hash) + i * 8, 8);
                    else
                        hash = ramcrc::key_hash(p.table_id, rd.pay + p.key_off, p.key_len);
                    winner = cl::live(w, t->slots[w].rank, b, i);
                }
            }
            const uint32_t k = mg::classify(part, r.header, table, table_id, hash, first_hash, last_hash, flags, winner);
            if (mg::sent(k)) {
                const uint64_t size = mg::entry_bytes(r.length);
                const bool stop = mg::too_large(size, out_capacity) || (sent && sm.sent_objects + sm.sent_tombstones == sent_cap) ||
                                  ((!open || mg::closes(head, size, out_capacity)) && sm.segments_used == max_segments);
                if (stop) {
                    sm.too_large = mg::too_large(size, out_capacity);
                    sm.next_index = v;
                    sm.next_record = i;
                    sm.done = 0;
                    break;
                }
                if (!open || mg::closes(head, size, out_capacity)) {
                    if (open)
                        seal();
                    if (seg_first) {
                        const uint64_t f = sm.sent_objects + sm.sent_tombstones;
                        memcpy(reinterpret_cast<uint8_t*>(seg_first) + sm.segments_used * 8, &f, 8);
                    }
                    sm.segments_used++;
                    open = true;
                    head = 0;
                    meta = 0xFFFFFFFFu;
                    cnt = ramcrc_migrate_count{};
                }
                uint8_t* const at = ob + (sm.segments_used - 1) * out_stride + head;
                const uint32_t nm = mg::meta_bytes(r.length);
                for (uint32_t q = 0; q < nm; q++)
                    at[q] = uint8_t(mg::meta_byte(r.header, r.length, q));
                meta = ramcrc_update(meta, at, nm);
                memcpy(at + nm, rd.pay, r.length);
                if (sent) {
                    const ramcrc_replay_ref ref{b, uint32_t(i)};
                    memcpy(reinterpret_cast<uint8_t*>(sent) + (sm.sent_objects + sm.sent_tombstones) * sizeof(ref),
                           &ref, sizeof(ref));
                }
                head += size;
                cnt.entries++;
                (k == mg::kSentObject ? cnt.objects : cnt.tombstones)++;
                (k == mg::kSentObject ? sm.sent_objects : sm.sent_tombstones)++;
                sm.sent_bytes += size;
                sm.payload_bytes += r.length;
            }
            sm.records_read++;
            sm.skipped_other += k == mg::kSkippedOther;
            sm.skipped_table += k == mg::kSkippedTable;
            sm.skipped_range += k == mg::kSkippedRange;
            sm.skipped_dead += k == mg::kSkippedDead;
        }
    }
    if (open)
        seal();
    memcpy(reinterpret_cast<uint8_t*>(summary), &sm, sizeof(sm));   // (no alignment rule)
    return RAMCRC_OK;
}

}  // extern "C"
