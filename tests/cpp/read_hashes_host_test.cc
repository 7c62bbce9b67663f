// ramcrc_replay_table_read_hashes_host driven from a host-only program (no GPU,
// no Python): the fan-out and truncation cases of tests/read_hashes_cases.py,
// restated in C++ with their own bookkeeping.  It is what a sanitizer build
// (-fsanitize=address,undefined) of ramcrc_host.cc runs.
//
// Every record is a one-key object or a tombstone of table 1 whose caller hash
// the test chooses; the version of an object is 1000 * batch + record, so the
// order of one hash's objects can be read off the reply.  Replies, parts and
// summaries lie in exactly sized heap blocks at odd addresses: a byte written
// past an end, or a misaligned typed access, is the sanitizer's to find.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

// One call on exactly sized blocks at odd addresses.
struct Reply {
    std::vector<uint8_t> bytes;
    std::vector<ramcrc_hash_part> parts;
    ramcrc_read_hashes_summary sm;
};

static Reply ask(ramcrc_replay_table_host* t, const std::vector<uint64_t>& asked, uint64_t capacity,
                 uint64_t maxLength)
{
    const size_t n = asked.size();
    uint8_t* const h = static_cast<uint8_t*>(malloc(8 * n + 1));
    uint8_t* const out = static_cast<uint8_t*>(malloc(capacity + 1));
    uint8_t* const parts = static_cast<uint8_t*>(malloc(sizeof(ramcrc_hash_part) * n + 1));
    uint8_t* const sm = static_cast<uint8_t*>(malloc(sizeof(ramcrc_read_hashes_summary) + 1));
    if (n)
        memcpy(h + 1, &asked[0], 8 * n);
    memset(out, 0xA5, capacity + 1);
    const int rc = ramcrc_replay_table_read_hashes_host(
        t, 1, n ? reinterpret_cast<const uint64_t*>(h + 1) : NULL, n, 0u, capacity ? out + 1 : NULL, capacity,
        maxLength, reinterpret_cast<ramcrc_hash_part*>(parts + 1),
        reinterpret_cast<ramcrc_read_hashes_summary*>(sm + 1));
    CHECK(rc == RAMCRC_OK);
    Reply r;
    memcpy(&r.sm, sm + 1, sizeof r.sm);
    CHECK(r.sm.reply_bytes <= capacity);
    r.bytes.assign(out + 1, out + 1 + (r.sm.reply_bytes <= capacity ? r.sm.reply_bytes : 0));
    for (uint64_t b = r.sm.reply_bytes; b < capacity; b++)
        CHECK(out[1 + b] == 0xA5);   // nothing at or past reply_bytes
    r.parts.resize(n);
    if (n)
        memcpy(&r.parts[0], parts + 1, sizeof(ramcrc_hash_part) * n);
    free(h);
    free(out);
    free(parts);
    free(sm);
    return r;
}

// The versions of the objects in a reply, in order; their parts must tile it.
static std::vector<uint64_t> versions(const Reply& r)
{
    std::vector<uint64_t> v;
    uint64_t at = 0;
    for (uint64_t k = 0; k < r.sm.objects; k++) {
        if (at + 12 > r.bytes.size()) {
            bad++;
            break;
        }
        uint64_t version;
        uint32_t length;
        memcpy(&version, &r.bytes[at], 8);
        memcpy(&length, &r.bytes[at + 8], 4);
        at += 12 + length;
        CHECK(at <= r.bytes.size() && length >= 4);
        if (at <= r.bytes.size() && length >= 4)
            CHECK(r.bytes[at - length] == 1 && r.bytes[at - 1] == uint8_t(version));   // key count, value
        v.push_back(version);
    }
    CHECK(at == r.bytes.size());
    return v;
}

static void fanOut(uint32_t n, uint32_t adds)
{
    ramcrc_replay_table_host* t = NULL;
    CHECK(ramcrc_replay_table_create_host(64, adds + 1, &t) == RAMCRC_OK);
    const uint64_t nslots = 128;   // of a table for 64 keys
    std::vector<Batch> bs(adds + 1);
    std::vector<uint64_t> want;
    for (uint32_t i = 0; i < n; i++) {
        Batch& b = bs[i % adds];
        const uint64_t version = 1000 * (i % adds) + b.table.size();
        b.object("fan " + std::to_string(i), version, i % 7 + 1, 7);
    }
    if (adds > 1) {   // a tombstone over key 0, in the last of the adds
        Batch& b = bs[adds - 1];
        b.tombstone("fan 0", 5000, 7);
    }
    for (uint32_t j = 0; j < adds; j++) {
        for (size_t r = 0; r < bs[j].table.size(); r++)
            if (bs[j].table[r].header == RAMCRC_LOG_ENTRY_TYPE_OBJ && !(adds > 1 && j == 0 && r == 0))
                want.push_back(1000 * j + r);
        CHECK(bs[j].add(t, j));
    }
    const uint64_t seven[1] = {7};
    Reply r = ask(t, std::vector<uint64_t>(seven, seven + 1), 1 << 16, 1 << 16);
    CHECK(versions(r) == want);   // ascending {batch, record}
    CHECK(r.sm.hashes == 1 && r.sm.objects == want.size() && r.sm.tombstones == (adds > 1 ? 1u : 0u));
    CHECK(r.parts[0].off == 0 && r.parts[0].objects == want.size() && r.parts[0].reserved == 0);
    const uint64_t others[4] = {8, 7 + nslots, 7, 6};
    r = ask(t, std::vector<uint64_t>(others, others + 4), 1 << 16, 1 << 16);
    CHECK(versions(r) == want && r.sm.hashes == 4 && r.sm.empty == 3 + (want.empty() ? 1u : 0u));
    CHECK(r.parts[0].objects == 0 && r.parts[1].objects == 0 && r.parts[3].objects == 0);
    CHECK(r.parts[0].off == 0 && r.parts[2].off == 0 && r.parts[3].off == r.sm.reply_bytes);
    // a second group, hash 8, on the same chain
    Batch& more = bs[adds];
    std::vector<uint64_t> want8;
    for (uint32_t i = 0; i < 5; i++) {
        want8.push_back(1000 * adds + i);
        more.object("eight " + std::to_string(i), 1000 * adds + i, i + 1, 8);
    }
    CHECK(more.add(t, adds));
    const uint64_t both[3] = {8, 7, 8};
    r = ask(t, std::vector<uint64_t>(both, both + 3), 1 << 16, 1 << 16);
    std::vector<uint64_t> all(want8);
    all.insert(all.end(), want.begin(), want.end());
    all.insert(all.end(), want8.begin(), want8.end());
    CHECK(versions(r) == all && r.sm.objects == all.size());
    ramcrc_replay_table_destroy_host(t);
}

static void truncation()
{
    ramcrc_replay_table_host* t = NULL;
    CHECK(ramcrc_replay_table_create_host(64, 1, &t) == RAMCRC_OK);
    Batch b;
    uint64_t bytesOf[200] = {0}, objectsOf[200] = {0};
    for (uint32_t i = 0; i < 8; i++) {   // hash 100 + i: one object of 7 i + 1 value bytes
        b.object("t" + std::to_string(i), b.table.size(), 7 * i + 1, 100 + i);
        bytesOf[100 + i] = 12 + 3 + 2 + 7 * i + 1;
        objectsOf[100 + i] = 1;
    }
    b.tombstone("dead", 9, 50);   // hash 50: nothing
    for (uint32_t i = 0; i < 3; i++) {   // hash 60: three objects
        b.object("three " + std::to_string(i), b.table.size(), 10 + i, 60);
        bytesOf[60] += 12 + 3 + 7 + 10 + i;
        objectsOf[60]++;
    }
    CHECK(b.add(t, 0));
    const uint64_t list[13] = {101, 60, 103, 50, 199, 60, 107, 100, 102, 50, 105, 60, 104};
    const std::vector<uint64_t> asked(list, list + 13);
    std::vector<uint64_t> start(13), end(13);
    uint64_t at = 0, longest = 0;
    for (int q = 0; q < 13; q++) {
        start[q] = at;
        at += bytesOf[asked[q]];
        end[q] = at;
        if (bytesOf[asked[q]] > longest)
            longest = bytesOf[asked[q]];
    }
    const Reply whole = ask(t, asked, at, at);
    CHECK(whole.sm.hashes == 13 && whole.sm.reply_bytes == at && whole.sm.objects == 16);
    CHECK(whole.sm.objects_counted == 16 && whole.sm.empty == 3 && whole.sm.tombstones == 2);
    for (int q = 0; q < 13; q++)
        CHECK(whole.parts[q].off == start[q] && whole.parts[q].objects == objectsOf[asked[q]]);
    // max_length one byte around every start, with room for the overshoot;
    // then the capacity alone around every end
    for (int pass = 0; pass < 2; pass++)
        for (int q = 0; q < 13; q++)
            for (int d = -1; d <= 1; d++) {
                const uint64_t edge = pass == 0 ? start[q] : end[q];
                if (edge == 0 && d < 0)
                    continue;
                const uint64_t ml = pass == 0 ? edge + d : at;
                const uint64_t cap = pass == 0 ? (ml < at ? ml : at) + longest : edge + d;
                const Reply r = ask(t, asked, cap, ml);
                uint64_t n = 0, objects = 0;
                while (n < 13 && start[n] <= ml && end[n] <= cap)
                    objects += objectsOf[asked[n++]];
                CHECK(r.sm.hashes == n && r.sm.objects == objects);
                CHECK(r.sm.reply_bytes == (n ? end[n - 1] : 0));
                CHECK(r.sm.objects_counted == objects + (n < 13 ? objectsOf[asked[n]] : 0));
                CHECK(r.bytes.size() == r.sm.reply_bytes &&
                      (r.bytes.empty() || memcmp(&r.bytes[0], &whole.bytes[0], r.bytes.size()) == 0));
                for (uint64_t q2 = 0; q2 < 13; q2++)
                    CHECK(r.parts[q2].off == (q2 < n ? start[q2] : RAMCRC_READ_NONE) &&
                          r.parts[q2].objects == (q2 < n ? objectsOf[asked[q2]] : 0));
                versions(r);
            }
    // no hashes, and no room at all
    Reply r = ask(t, std::vector<uint64_t>(), 0, 0);
    CHECK(r.sm.hashes == 0 && r.sm.reply_bytes == 0 && r.sm.spoiled == 0);
    r = ask(t, asked, 0, 0);
    CHECK(r.sm.hashes == 0 && r.sm.objects_counted == 1);
    ramcrc_replay_table_destroy_host(t);
}

int main()
{
    static const uint32_t counts[4] = {1, 2, 3, 40};
    for (int k = 0; k < 4; k++) {
        fanOut(counts[k], 1);
        fanOut(counts[k], 3);
    }
    truncation();
    printf("read_hashes_host: fan-out of 1, 2, 3 and 40 keys in one and three adds, truncation at every "
           "start and end; %d mismatches\n", bad);
    return bad ? 1 : 0;
}
