// ramcrc_replay_table_index_build_host and ramcrc_index_lookup_host driven from
// a host-only program (no GPU, no Python): two batches of two- and three-key
// objects, overwrites, tombstones and another table id; the entries against
// std::sort over std::string keys (whose order is memcmp, then the shorter
// first); every point query, ranges with max_hashes and first_allowed_hash, an
// output that ends inside the batch, a bad query.  It is what a sanitizer build
// (-fsanitize=address,undefined) of ramcrc_host.cc and index_rules.h runs:
// entries, hashes, keys, queries, results and summaries lie in exactly sized
// heap blocks at odd addresses, so a byte past an end or a misaligned typed
// access is the sanitizer's to find.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
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
    // Object::Header {checksum, timestamp, version, tableId}, KeyCount,
    // CumulativeKeyLength per key, the keys, a one-byte value
    void object(uint64_t tableId, const std::vector<std::string>& keys, uint64_t version, uint64_t hash)
    {
        std::vector<uint8_t> o(24, 0);
        memcpy(&o[8], &version, 8);
        memcpy(&o[16], &tableId, 8);
        o.push_back(uint8_t(keys.size()));
        uint16_t cum = 0;
        for (size_t k = 0; k < keys.size(); k++) {
            cum = uint16_t(cum + keys[k].size());
            o.push_back(uint8_t(cum));
            o.push_back(uint8_t(cum >> 8));
        }
        for (size_t k = 0; k < keys.size(); k++)
            o.insert(o.end(), keys[k].begin(), keys[k].end());
        o.push_back('v');
        append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o, hash);
    }
    void tombstone(uint64_t tableId, const std::string& key, uint64_t version, uint64_t hash)
    {
        // ObjectTombstone::Header {tableId, segmentId, objectVersion, timestamp, checksum}, key
        std::vector<uint8_t> t(32 + key.size(), 0);
        memcpy(&t[0], &tableId, 8);
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
        return ramcrc_replay_table_add_host(t, &seg[0], kCap, 1, &status, &table[0], table.size(), &hashes[0],
                                            &work[0], &number) == RAMCRC_OK && number == want;
    }
};

// A block of n bytes at an odd address.
struct Odd {
    uint8_t* base;
    explicit Odd(size_t n) : base(static_cast<uint8_t*>(malloc(n + 1))) { memset(base, 0xA5, n + 1); }
    ~Odd() { free(base); }
    uint8_t* p() { return base + 1; }
    Odd(const Odd&);
    Odd& operator=(const Odd&);
};

typedef std::pair<std::string, uint64_t> Pair;   // {secondary key, pk hash}

struct Index {
    Odd entries, hashes, keys, summary;
    ramcrc_index_build_summary sm;
    Index(uint64_t ecap, uint64_t kcap)
        : entries(32 * ecap), hashes(8 * ecap), keys(kcap), summary(sizeof(ramcrc_index_build_summary))
    {
    }
    ramcrc_index_entry entry(uint64_t i)
    {
        ramcrc_index_entry e;
        memcpy(&e, entries.p() + 32 * i, 32);
        return e;
    }
};

static void build(ramcrc_replay_table_host* t, uint64_t tableId, uint32_t indexId, Index* ix, uint64_t ecap,
                  uint64_t kcap)
{
    const int rc = ramcrc_replay_table_index_build_host(
        t, tableId, indexId, reinterpret_cast<ramcrc_index_entry*>(ix->entries.p()), ecap,
        reinterpret_cast<uint64_t*>(ix->hashes.p()), ix->keys.p(), kcap,
        reinterpret_cast<ramcrc_index_build_summary*>(ix->summary.p()));
    CHECK(rc == RAMCRC_OK);
    memcpy(&ix->sm, ix->summary.p(), sizeof ix->sm);
}

static void checkIndex(Index* ix, std::vector<Pair> want, uint64_t seen)
{
    std::sort(want.begin(), want.end());
    uint64_t kb = 0;
    for (size_t i = 0; i < want.size(); i++)
        kb += want[i].first.size();
    CHECK(ix->sm.n_entries == want.size() && ix->sm.entries_needed == want.size() && ix->sm.key_bytes == kb &&
          ix->sm.key_bytes_needed == kb && ix->sm.objects_seen == seen && !ix->sm.overflow && !ix->sm.spoiled);
    for (size_t i = 0; i < want.size() && i < ix->sm.n_entries; i++) {
        const ramcrc_index_entry e = ix->entry(i);
        uint64_t h;
        memcpy(&h, ix->hashes.p() + 8 * i, 8);
        CHECK(e.key_off + e.key_len <= kb && e.reserved == 0 && h == e.pk_hash && e.pk_hash == want[i].second);
        if (e.key_off + e.key_len > kb)
            continue;
        CHECK(std::string(reinterpret_cast<char*>(ix->keys.p() + e.key_off), e.key_len) == want[i].first);
        uint64_t prefix = 0;
        for (uint32_t b = 0; b < 8; b++)
            prefix = (prefix << 8) | (b < want[i].first.size() ? uint8_t(want[i].first[b]) : 0u);
        CHECK(e.prefix == prefix);
    }
}

struct Range {
    std::string first, last;
    uint64_t firstAllowed;
    uint32_t maxHashes;
};

// The lookup on exactly sized blocks; checked against a scan of the sorted pairs.
static void lookup(Index* ix, std::vector<Pair> all, const std::vector<Range>& ranges, uint64_t ocap, int badQuery)
{
    std::sort(all.begin(), all.end());
    std::string qk;
    Odd queries(40 * ranges.size()), results(48 * ranges.size()), out(8 * ocap), summary(48);
    for (size_t i = 0; i < ranges.size(); i++) {
        ramcrc_index_query q = {qk.size(), qk.size() + ranges[i].first.size(), ranges[i].firstAllowed,
                                uint32_t(ranges[i].first.size()), uint32_t(ranges[i].last.size()),
                                ranges[i].maxHashes, 0u};
        qk += ranges[i].first + ranges[i].last;
        if (int(i) == badQuery)
            q.last_off = ~0ull;
        memcpy(queries.p() + 40 * i, &q, 40);
    }
    Odd qkeys(qk.size());
    memcpy(qkeys.p(), qk.data(), qk.size());
    const int rc = ramcrc_index_lookup_host(
        reinterpret_cast<ramcrc_index_entry*>(ix->entries.p()), reinterpret_cast<uint64_t*>(ix->hashes.p()),
        ix->keys.p(), reinterpret_cast<ramcrc_index_build_summary*>(ix->summary.p()), qkeys.p(), qk.size(),
        reinterpret_cast<ramcrc_index_query*>(queries.p()), ranges.size(), reinterpret_cast<uint64_t*>(out.p()), ocap,
        reinterpret_cast<ramcrc_index_result*>(results.p()), reinterpret_cast<ramcrc_index_lookup_summary*>(summary.p()));
    CHECK(rc == RAMCRC_OK);
    ramcrc_index_lookup_summary sm;
    memcpy(&sm, summary.p(), sizeof sm);
    uint64_t at = 0, served = 0, maxed = 0;
    bool open = true;
    for (size_t i = 0; i < ranges.size(); i++) {
        ramcrc_index_result r;
        memcpy(&r, results.p() + 48 * i, 48);
        if (open && int(i) == badQuery) {
            CHECK(r.status == RAMCRC_INDEX_BAD_QUERY && r.out_off == RAMCRC_READ_NONE && r.num_hashes == 0);
            served++;
            continue;
        }
        std::vector<uint64_t> want;
        bool more = false;
        Pair next;
        for (size_t k = 0; k < all.size() && open; k++) {
            const Pair& p = all[k];
            if (p < Pair(ranges[i].first, ranges[i].firstAllowed) || (!ranges[i].last.empty() && p.first > ranges[i].last))
                continue;
            if (want.size() == ranges[i].maxHashes) {
                more = true;
                next = p;
                break;
            }
            want.push_back(p.second);
        }
        if (open && at + want.size() > ocap)
            open = false;
        if (!open) {
            CHECK(r.status == RAMCRC_INDEX_NOT_SERVED && r.out_off == RAMCRC_READ_NONE && r.num_hashes == 0);
            continue;
        }
        CHECK(r.status == RAMCRC_INDEX_OK && r.out_off == at && r.num_hashes == want.size() && r.reserved == 0);
        for (size_t k = 0; k < want.size() && r.num_hashes == want.size(); k++) {
            uint64_t h;
            memcpy(&h, out.p() + 8 * (at + k), 8);
            CHECK(h == want[k]);
        }
        if (more) {
            CHECK(r.next_key_len == next.first.size() && r.next_key_hash == next.second &&
                  r.next_key_off + r.next_key_len <= ix->sm.key_bytes);
            if (r.next_key_off + r.next_key_len <= ix->sm.key_bytes)
                CHECK(std::string(reinterpret_cast<char*>(ix->keys.p() + r.next_key_off), r.next_key_len) == next.first);
        } else {
            CHECK(r.next_key_len == 0 && r.next_key_hash == 0 && r.next_entry == 0 && r.next_key_off == 0);
        }
        at += want.size();
        served++;
        maxed += more;
    }
    CHECK(sm.served == served && sm.hashes == at && sm.maxed_out == maxed && sm.n_entries == ix->sm.n_entries &&
          sm.overflow_index == 0 && sm.bad == uint64_t(badQuery >= 0 && uint64_t(badQuery) < served));
    for (uint64_t b = 8 * at; b < 8 * ocap; b++)
        CHECK(out.p()[b] == 0xA5);   // nothing at or past `hashes`
}

int main()
{
    ramcrc_replay_table_host* t = NULL;
    if (ramcrc_replay_table_create_host(256, 4, &t))
        return 1;
    Batch a, b;
    std::vector<Pair> want1, want2;
    uint64_t seen = 0;
    // batch 0: 60 objects of table 1; keys of 1 .. 12 bytes that share 8-byte
    // prefixes, runs of equal keys, every third with a third key
    for (uint32_t i = 0; i < 60; i++) {
        std::vector<std::string> keys;
        keys.push_back("pk" + std::to_string(i));
        keys.push_back(std::string("samepref", 1 + i % 8) + std::string(i % 5, char('a' + i % 3)));
        if (i % 3 == 0)
            keys.push_back("third" + std::to_string(i % 4));
        a.object(1, keys, 1, 1000 + 37 * i % 64);
    }
    a.object(2, std::vector<std::string>{"other table", "samepref"}, 1, 5);
    a.object(1, std::vector<std::string>{"no second key"}, 1, 6);
    a.object(1, std::vector<std::string>{"empty second", ""}, 1, 7);
    CHECK(a.add(t, 0));
    // batch 1: every fourth is removed, every fifth gets a newer version with another key
    for (uint32_t i = 0; i < 60; i++) {
        if (i % 4 == 0)
            b.tombstone(1, "pk" + std::to_string(i), 1, 1000 + 37 * i % 64);
        else if (i % 5 == 0)
            b.object(1, std::vector<std::string>{"pk" + std::to_string(i), "moved" + std::to_string(i)}, 2,
                     1000 + 37 * i % 64);
    }
    CHECK(b.add(t, 1));
    for (uint32_t i = 0; i < 60; i++) {
        if (i % 4 == 0)
            continue;
        seen++;
        const uint64_t h = 1000 + 37 * i % 64;
        if (i % 5 == 0) {
            want1.push_back(Pair("moved" + std::to_string(i), h));
            continue;
        }
        want1.push_back(Pair(std::string("samepref", 1 + i % 8) + std::string(i % 5, char('a' + i % 3)), h));
        if (i % 3 == 0)
            want2.push_back(Pair("third" + std::to_string(i % 4), h));
    }
    seen += 2;   // the objects of table 1 without an index key
    uint64_t kb1 = 0;
    for (size_t i = 0; i < want1.size(); i++)
        kb1 += want1[i].first.size();
    {
        Index sizing(0, 0);
        const int rc = ramcrc_replay_table_index_build_host(
            t, 1, 1, NULL, 0, NULL, NULL, 0, reinterpret_cast<ramcrc_index_build_summary*>(sizing.summary.p()));
        memcpy(&sizing.sm, sizing.summary.p(), sizeof sizing.sm);
        CHECK(rc == RAMCRC_OK && sizing.sm.overflow == 1 && sizing.sm.entries_needed == want1.size() &&
              sizing.sm.key_bytes_needed == kb1 && sizing.sm.n_entries == 0);
        Index shortE(want1.size() - 1, kb1), shortK(want1.size(), kb1 - 1);
        build(t, 1, 1, &shortE, want1.size() - 1, kb1);
        build(t, 1, 1, &shortK, want1.size(), kb1 - 1);
        CHECK(shortE.sm.overflow == 1 && shortK.sm.overflow == 1);
        for (uint64_t k = 0; k < kb1; k++)
            CHECK(shortE.keys.p()[k] == 0xA5);
    }
    Index ix1(want1.size(), kb1), ix2(want2.size() + 2, 128), ix3(4, 4), other(1, 8);
    build(t, 1, 1, &ix1, want1.size(), kb1);
    checkIndex(&ix1, want1, seen);
    build(t, 1, 2, &ix2, want2.size() + 2, 128);
    checkIndex(&ix2, want2, seen);
    build(t, 1, 3, &ix3, 4, 4);
    checkIndex(&ix3, std::vector<Pair>(), seen);
    build(t, 2, 1, &other, 1, 8);
    checkIndex(&other, std::vector<Pair>(1, Pair("samepref", 5)), 1);
    CHECK(ramcrc_replay_table_index_build_host(t, 1, 0, NULL, 0, NULL, NULL, 0, &ix1.sm) == RAMCRC_EINVAL);

    std::vector<Range> ranges;
    for (size_t i = 0; i < want1.size(); i++)
        ranges.push_back(Range{want1[i].first, want1[i].first, 0, 100});
    lookup(&ix1, want1, ranges, 8 * want1.size(), -1);
    ranges.clear();
    ranges.push_back(Range{"", "", 0, 1000});
    ranges.push_back(Range{"s", "samepre", 0, 3});
    ranges.push_back(Range{"samepref", "samepref", 1020, 2});
    ranges.push_back(Range{"samepref", "", ~0ull, 5});
    ranges.push_back(Range{"t", "s", 0, 5});
    ranges.push_back(Range{"", "moved9", 0, 0});
    ranges.push_back(Range{"samepref", "sameprefzz", 0, 1000});
    for (uint64_t ocap = 0; ocap < 2 * want1.size() + 20; ocap += 7)
        lookup(&ix1, want1, ranges, ocap, -1);
    lookup(&ix1, want1, ranges, 4 * want1.size(), 2);
    lookup(&ix2, want2, ranges, 64, -1);
    ramcrc_replay_table_destroy_host(t);
    printf("index: %zu and %zu entries; %d mismatches\n", want1.size(), want2.size(), bad);
    return bad ? 1 : 0;
}
