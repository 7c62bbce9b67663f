// ramcrc_replay_table_enumerate_host driven from a host-only program (no GPU,
// no Python): buckets of 1, 2, 3 and 40 keys, the cut at every entry's start
// and end, and the cursor walk of tests/enumerate_cases.py, restated in C++
// with their own bookkeeping.  It is what a sanitizer build
// (-fsanitize=address,undefined) of ramcrc_host.cc runs.
//
// Every record is a one-key object or a tombstone of table 1 whose caller hash
// the test chooses; the version of an object is 1000 * batch + record, so the
// order of a bucket's entries can be read off the payload.  Payloads, frames
// and summaries lie in exactly sized heap blocks at odd addresses: a byte
// written past an end, or a misaligned typed access, is the sanitizer's to find.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ramcrc.h"

static int bad = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            bad++;                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
        }                                                               \
    } while (0)

static const uint32_t kCap = 64 * 1024;
static const uint64_t kSlots = 128;   // of a table for 64 keys

struct Batch {
    std::vector<uint8_t> seg;
    std::vector<ramcrc_seg_entry> table;
    std::vector<uint64_t> hashes, work;
    ramcrc_seg_status status;
    uint32_t pos;
    Batch() : seg(kCap, 0), pos(0) {}
    void append(uint8_t type, const std::vector<uint8_t>& payload, uint64_t hash)
    {
        const uint32_t len = uint32_t(payload.size());   // < 256 here
        ramcrc_seg_entry e = {0u, pos, len, type};
        seg[pos] = type;
        seg[pos + 1] = uint8_t(len);
        memcpy(&seg[pos + 2], payload.data(), len);
        pos += 2 + len;
        table.push_back(e);
        hashes.push_back(hash);
    }
    void object(const std::string& key, uint64_t version, uint32_t valueLen, uint64_t hash)
    {
        // Object::Header {checksum, timestamp, version, tableId}, KeyCount,
        // CumulativeKeyLength, key, value
        std::vector<uint8_t> o(24 + 1 + 2 + key.size() + valueLen, uint8_t(version));
        memset(&o[0], 0, 24);
        memcpy(&o[8], &version, 8);
        o[16] = 1;
        o[24] = 1;
        o[25] = uint8_t(key.size());
        o[26] = 0;
        memcpy(&o[27], key.data(), key.size());
        append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o, hash);
    }
    void tombstone(const std::string& key, uint64_t version, uint64_t hash)
    {
        // ObjectTombstone::Header {tableId, segmentId, objectVersion, timestamp, checksum}, key
        std::vector<uint8_t> t(32 + key.size(), 0);
        t[0] = 1;
        memcpy(&t[16], &version, 8);
        memcpy(&t[32], key.data(), key.size());
        append(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, t, hash);
    }
    bool add(ramcrc_replay_table_host* t, uint32_t want)
    {
        ramcrc_seg_status st = {RAMCRC_SEG_OK, 0u, uint32_t(table.size()), 0u};
        status = st;
        work.assign(table.size() + 1, 0);
        uint32_t number = ~0u;
        return ramcrc_replay_table_add_host(t, &seg[0], kCap, 1, &status, table.empty() ? NULL : &table[0],
                                            table.size(), hashes.empty() ? NULL : &hashes[0], &work[0],
                                            &number) == RAMCRC_OK && number == want;
    }
};

// What the test itself knows of an object that must come back.
struct Known {
    uint64_t hash, version;   // version: 1000 * batch + record, the order within a hash
    uint32_t length;          // of the log entry
    uint32_t keysLength;      // of the entry with keys only
    bool operator<(const Known& o) const
    {
        const uint64_t b = hash & (kSlots - 1), ob = o.hash & (kSlots - 1);
        return b != ob ? b < ob : hash != o.hash ? hash < o.hash : version < o.version;
    }
};

// One call on exactly sized blocks at odd addresses.
struct Reply {
    std::vector<uint8_t> bytes;
    ramcrc_enumerate_summary sm;
};

static Reply ask(ramcrc_replay_table_host* t, uint64_t bucket, uint64_t nextHash, uint64_t limit, bool keysOnly,
                 uint64_t capacity, uint64_t maxBytes, const std::vector<ramcrc_enum_frame>& stale)
{
    uint8_t* const out = static_cast<uint8_t*>(malloc(capacity + 1));
    uint8_t* const sm = static_cast<uint8_t*>(malloc(sizeof(ramcrc_enumerate_summary) + 1));
    uint8_t* const fr = static_cast<uint8_t*>(malloc(sizeof(ramcrc_enum_frame) * stale.size() + 1));
    if (!stale.empty())
        memcpy(fr + 1, &stale[0], sizeof(ramcrc_enum_frame) * stale.size());
    memset(out, 0xA5, capacity + 1);
    const int rc = ramcrc_replay_table_enumerate_host(
        t, 1, 0, ~0ull, bucket, nextHash, limit, stale.empty() ? NULL : reinterpret_cast<ramcrc_enum_frame*>(fr + 1),
        uint32_t(stale.size()), keysOnly ? RAMCRC_ENUM_KEYS_ONLY : 0u, capacity ? out + 1 : NULL, capacity, maxBytes,
        reinterpret_cast<ramcrc_enumerate_summary*>(sm + 1));
    CHECK(rc == RAMCRC_OK);
    Reply r;
    memcpy(&r.sm, sm + 1, sizeof r.sm);
    CHECK(r.sm.payload_bytes <= capacity && r.sm.payload_bytes <= maxBytes && r.sm.num_buckets == kSlots);
    r.bytes.assign(out + 1, out + 1 + (r.sm.payload_bytes <= capacity ? r.sm.payload_bytes : 0));
    for (uint64_t b = r.sm.payload_bytes; b < capacity; b++)
        CHECK(out[1 + b] == 0xA5);   // nothing at or past payload_bytes
    free(out);
    free(sm);
    free(fr);
    return r;
}

// The versions of the objects in a payload, in order; its entries must tile it.
static std::vector<uint64_t> versions(const Reply& r, bool keysOnly)
{
    std::vector<uint64_t> v;
    uint64_t at = 0;
    for (uint64_t k = 0; k < r.sm.objects; k++) {
        if (at + 4 > r.bytes.size()) {
            bad++;
            break;
        }
        uint32_t length;
        memcpy(&length, &r.bytes[at], 4);
        at += 4;
        CHECK(at + length <= r.bytes.size() && length >= 28);
        if (at + length > r.bytes.size() || length < 28)
            break;
        uint64_t version;
        memcpy(&version, &r.bytes[at + 8], 8);
        CHECK(r.bytes[at + 16] == 1 && r.bytes[at + 24] == 1);   // table id, key count
        CHECK(length == 27u + r.bytes[at + 25] + (keysOnly ? 0u : uint32_t(version % 7) + 1));
        v.push_back(version);
        at += length;
    }
    CHECK(at == r.bytes.size());
    return v;
}

static const std::vector<ramcrc_enum_frame> kNone;

static void buckets(uint32_t n, uint32_t adds)
{
    ramcrc_replay_table_host* t = NULL;
    CHECK(ramcrc_replay_table_create_host(64, adds, &t) == RAMCRC_OK);
    std::vector<Batch> bs(adds);
    std::vector<Known> known;
    // bucket 7: n keys of hash 7, two of 7 + slots, one of 7 + 5 * slots; bucket 8 on
    // the same chain; bucket 127, whose keys wrap to slot 0; a tombstone winner
    std::vector<uint64_t> hs(n, 7);
    const uint64_t others[7] = {8, 7 + kSlots, 8, 7 + kSlots, 7 + 5 * kSlots, 127, 127};
    hs.insert(hs.end(), others, others + 7);
    for (size_t i = 0; i < hs.size(); i++) {
        Batch& b = bs[i % adds];
        const uint64_t version = 1000 * (i % adds) + b.table.size();
        const std::string key = "key " + std::to_string(i);
        b.object(key, version, uint32_t(version % 7) + 1, hs[i]);
        const Known k = {hs[i], version, uint32_t(27 + key.size() + version % 7 + 1), uint32_t(27 + key.size())};
        known.push_back(k);
    }
    bs[adds - 1].object("dead", 1, 3, 7);
    bs[adds - 1].tombstone("dead", 1, 7);
    for (uint32_t j = 0; j < adds; j++)
        CHECK(bs[j].add(t, j));
    std::sort(known.begin(), known.end());
    for (int keysOnly = 0; keysOnly < 2; keysOnly++) {
        std::vector<uint64_t> want, start, end;
        uint64_t at = 0;
        for (size_t k = 0; k < known.size(); k++) {
            want.push_back(known[k].version);
            start.push_back(at);
            at += 4 + (keysOnly ? known[k].keysLength : known[k].length);
            end.push_back(at);
        }
        const Reply whole = ask(t, 0, 0, 0, keysOnly, at, at, kNone);
        CHECK(versions(whole, keysOnly) == want && whole.sm.payload_bytes == at && whole.sm.full == 0);
        CHECK(whole.sm.next_bucket == kSlots && whole.sm.next_hash == 0 && whole.sm.tombstones == 1);
        // the cut at every entry's start and end, +- 1, from bucket 0 (a later
        // bucket is left out whole) and from bucket 7 (the cut inside it)
        for (size_t k = 0; k < known.size(); k++)
            for (int d = -1; d <= 2; d++) {
                const uint64_t mb = d == 2 ? start[k] : end[k] + d;
                const Reply r = ask(t, 0, 0, 0, keysOnly, mb, mb, kNone);
                // whole buckets only
                size_t m = 0;
                while (m < known.size()) {
                    size_t e = m;
                    while (e < known.size() && (known[e].hash & (kSlots - 1)) == (known[m].hash & (kSlots - 1)))
                        e++;
                    if (end[e - 1] > mb)
                        break;
                    m = e;
                }
                CHECK(r.sm.objects == m && r.sm.payload_bytes == (m ? end[m - 1] : 0));
                CHECK(r.sm.full == (m < known.size()) && r.sm.stuck == 0 && r.sm.next_hash == 0);
                CHECK(r.sm.next_bucket == (m < known.size() ? (known[m].hash & (kSlots - 1)) : kSlots));
                CHECK(r.bytes.empty() || memcmp(&r.bytes[0], &whole.bytes[0], r.bytes.size()) == 0);
                versions(r, keysOnly);
                if (mb < start[0])
                    continue;
                const uint64_t room = mb - start[0];   // bucket 7 is the first with entries
                const Reply c = ask(t, 7, 0, 0, keysOnly, room, room, kNone);
                size_t f = 0;   // whole hashes of bucket 7 only, unless the bucket fits
                while (f < known.size() && (known[f].hash & (kSlots - 1)) == 7)
                    f++;
                if (end[f - 1] - start[0] > room) {
                    size_t s = 0;
                    while (end[s] - start[0] <= room)
                        s++;
                    const uint64_t nh = known[s].hash;
                    while (s && known[s - 1].hash == nh)
                        s--;
                    CHECK(c.sm.objects == s && c.sm.next_bucket == 7 && c.sm.next_hash == nh && c.sm.full == 1);
                    CHECK(c.sm.stuck == (s == 0));
                    // the resume sends the rest of the bucket, nothing twice
                    const Reply rest = ask(t, 7, nh, 8, keysOnly, at, at, kNone);
                    std::vector<uint64_t> both = versions(c, keysOnly), more = versions(rest, keysOnly);
                    both.insert(both.end(), more.begin(), more.end());
                    CHECK(both == std::vector<uint64_t>(want.begin(), want.begin() + f));
                } else {
                    CHECK(c.sm.objects >= f && c.sm.next_bucket > 7 && c.sm.next_hash == 0);
                }
            }
        // the walk: small replies, three buckets a call
        std::vector<uint64_t> got;
        uint64_t bucket = 0, nextHash = 0, calls = 0;
        while (bucket < kSlots && calls < 10000) {
            uint64_t mb = 70;
            Reply r = ask(t, bucket, nextHash, std::min(bucket + 3, kSlots), keysOnly, mb, mb, kNone);
            while (r.sm.stuck && mb < (1u << 20)) {
                mb *= 2;
                r = ask(t, bucket, nextHash, std::min(bucket + 3, kSlots), keysOnly, mb, mb, kNone);
            }
            const std::vector<uint64_t> v = versions(r, keysOnly);
            got.insert(got.end(), v.begin(), v.end());
            bucket = r.sm.next_bucket;
            nextHash = r.sm.next_hash;
            calls++;
        }
        CHECK(got == want && calls >= kSlots / 3);
        // a stale frame over everything, of four buckets, that stands at bucket 3: hashes 7 + k * slots are
        // in its bucket 3 and not below hash 0, so nothing of them is hidden; at bucket 4 they all are
        ramcrc_enum_frame f = {0, ~0ull, 4, 3, 0};
        Reply r = ask(t, 0, 0, 0, keysOnly, at, at, std::vector<ramcrc_enum_frame>(1, f));
        std::vector<uint64_t> open;
        for (size_t k = 0; k < known.size(); k++)
            if ((known[k].hash & 3) >= 3)
                open.push_back(known[k].version);
        CHECK(versions(r, keysOnly) == open && r.sm.tombstones == 1);
        f.bucket_index = 4;
        r = ask(t, 0, 0, 0, keysOnly, at, at, std::vector<ramcrc_enum_frame>(8, f));
        CHECK(r.sm.objects == 0 && r.sm.payload_bytes == 0 && r.sm.tombstones == 0 && r.sm.next_bucket == kSlots);
    }
    ramcrc_replay_table_destroy_host(t);
}

int main()
{
    static const uint32_t counts[4] = {1, 2, 3, 40};
    for (int k = 0; k < 4; k++) {
        buckets(counts[k], 1);
        buckets(counts[k], 3);
    }
    printf("enumerate_host: buckets of 1, 2, 3 and 40 keys in one and three adds, the cut at every entry's "
           "start and end, the cursor walk, stale frames; %d mismatches\n", bad);
    return bad ? 1 : 0;
}
