// ramcrc_replay_table_migrate_host driven from a host-only program (no GPU, no
// Python): three batches of objects and tombstones over two table ids with
// overwrites, an RPCRESULT record and caller hashes; both modes, hash ranges,
// output capacities from 64 bytes up, every max_segments, every start cursor
// and a short d_sent, each held against this file's own bookkeeping: a
// sequential pass over its record list that packs greedily and takes the
// certificate from ramcrc_update.  It is what a sanitizer build
// (-fsanitize=address,undefined) of ramcrc_host.cc and migrate_rules.h runs:
// outputs, certificates, counts, references, first indices and the summary lie
// in exactly sized heap blocks at odd addresses, so a byte past an end or a
// misaligned typed access is the sanitizer's to find.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
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

static const uint32_t kCap = 16 * 1024;

struct Rec {
    uint8_t type;
    uint64_t table, hash, version;
    std::string key;
    std::vector<uint8_t> payload;
    bool participant;
};

struct Batch {
    std::vector<uint8_t> seg;
    std::vector<ramcrc_seg_entry> table;
    std::vector<uint64_t> hashes, work;
    std::vector<Rec> recs;
    ramcrc_seg_status status;
    uint32_t pos;
    Batch() : seg(kCap, 0), pos(0) {}
    void append(const Rec& r)
    {
        const uint32_t len = uint32_t(r.payload.size());   // < 256 here
        ramcrc_seg_entry e = {0u, pos, len, r.type};
        seg[pos] = r.type;
        seg[pos + 1] = uint8_t(len);
        memcpy(&seg[pos + 2], r.payload.data(), len);
        pos += 2 + len;
        table.push_back(e);
        hashes.push_back(r.hash);
        recs.push_back(r);
    }
    void object(uint64_t tableId, const std::string& key, uint64_t version, uint64_t hash, size_t valueLen)
    {
        Rec r = {RAMCRC_LOG_ENTRY_TYPE_OBJ, tableId, hash, version, key, std::vector<uint8_t>(24, 0), true};
        memcpy(&r.payload[8], &version, 8);
        memcpy(&r.payload[16], &tableId, 8);
        r.payload.push_back(1);
        r.payload.push_back(uint8_t(key.size()));
        r.payload.push_back(0);
        r.payload.insert(r.payload.end(), key.begin(), key.end());
        r.payload.insert(r.payload.end(), valueLen, uint8_t('a' + version));
        append(r);
    }
    void tombstone(uint64_t tableId, const std::string& key, uint64_t version, uint64_t hash)
    {
        Rec r = {RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, tableId, hash, version, key,
                 std::vector<uint8_t>(32 + key.size(), 0), true};
        memcpy(&r.payload[0], &tableId, 8);
        memcpy(&r.payload[16], &version, 8);
        memcpy(&r.payload[32], key.data(), key.size());
        append(r);
    }
    void rpcResult(uint64_t tableId, uint64_t hash)
    {
        Rec r = {RAMCRC_LOG_ENTRY_TYPE_RPCRESULT, tableId, hash, 0, "", std::vector<uint8_t>(56, 0), false};
        memcpy(&r.payload[0], &tableId, 8);
        memcpy(&r.payload[8], &hash, 8);
        append(r);
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
    size_t n;
    explicit Odd(size_t n_) : base(static_cast<uint8_t*>(malloc(n_ + 1))), n(n_) { memset(base, 0xA5, n + 1); }
    ~Odd() { free(base); }
    uint8_t* p() { return base + 1; }
    bool untouched(size_t from) const
    {
        for (size_t i = from; i < n; i++)
            if (base[1 + i] != 0xA5)
                return false;
        return true;
    }
    Odd(const Odd&);
    Odd& operator=(const Odd&);
};

struct Want {
    std::vector<std::string> segs;
    std::vector<std::pair<uint32_t, uint32_t> > sent;
    std::vector<uint64_t> first;
    std::vector<uint32_t> objects, tombstones;
    ramcrc_migrate_summary sm;
};

typedef std::pair<uint64_t, std::string> Key;

// The winners by this file's own rule: the highest version; a tombstone before
// an object; then the first record.
static std::map<Key, std::pair<uint32_t, uint32_t> > winners(const std::vector<Batch*>& bs)
{
    std::map<Key, std::pair<uint32_t, uint32_t> > win;
    for (uint32_t b = 0; b < bs.size(); b++)
        for (uint32_t i = 0; i < bs[b]->recs.size(); i++) {
            const Rec& r = bs[b]->recs[i];
            if (!r.participant)
                continue;
            const Key k(r.table, r.key);
            if (!win.count(k)) {
                win[k] = std::make_pair(b, i);
                continue;
            }
            const Rec& w = bs[win[k].first]->recs[win[k].second];
            if (r.version > w.version || (r.version == w.version && r.type == RAMCRC_LOG_ENTRY_TYPE_OBJTOMB &&
                                          w.type == RAMCRC_LOG_ENTRY_TYPE_OBJ))
                win[k] = std::make_pair(b, i);
        }
    return win;
}

static Want expect(const std::vector<Batch*>& bs, uint64_t tableId, uint64_t first, uint64_t last, bool liveOnly,
                   uint32_t startIndex, uint32_t startRecord, uint32_t cap, uint32_t maxSegments, bool haveSent,
                   uint64_t sentCap)
{
    const std::map<Key, std::pair<uint32_t, uint32_t> > win = winners(bs);
    Want w;
    memset(&w.sm, 0, sizeof w.sm);
    w.sm.next_index = bs.size();
    w.sm.done = 1;
    for (uint32_t b = startIndex; b < bs.size() && w.sm.done; b++)
        for (uint32_t i = b == startIndex ? startRecord : 0; i < bs[b]->recs.size(); i++) {
            const Rec& r = bs[b]->recs[i];
            w.sm.records_read++;
            if (!r.participant) {
                w.sm.skipped_other++;
                continue;
            }
            if (r.table != tableId) {
                w.sm.skipped_table++;
                continue;
            }
            if (r.hash < first || r.hash > last) {
                w.sm.skipped_range++;
                continue;
            }
            if (liveOnly && win.find(Key(r.table, r.key))->second != std::make_pair(b, i)) {
                w.sm.skipped_dead++;
                continue;
            }
            const size_t size = 2 + r.payload.size();
            const bool opens = w.segs.empty() || w.segs.back().size() + size > cap;
            if (size > cap || (haveSent && w.sent.size() == sentCap) || (opens && w.segs.size() == maxSegments)) {
                w.sm.records_read--;
                w.sm.next_index = b;
                w.sm.next_record = i;
                w.sm.done = 0;
                w.sm.too_large = size > cap;
                break;
            }
            if (opens) {
                w.first.push_back(w.sent.size());
                w.segs.push_back(std::string());
                w.objects.push_back(0);
                w.tombstones.push_back(0);
            }
            w.segs.back().push_back(char(r.type));
            w.segs.back().push_back(char(r.payload.size()));
            w.segs.back().append(reinterpret_cast<const char*>(r.payload.data()), r.payload.size());
            w.sent.push_back(std::make_pair(b, i));
            if (r.type == RAMCRC_LOG_ENTRY_TYPE_OBJ) {
                w.objects.back()++;
                w.sm.sent_objects++;
            } else {
                w.tombstones.back()++;
                w.sm.sent_tombstones++;
            }
            w.sm.sent_bytes += size;
            w.sm.payload_bytes += r.payload.size();
        }
    w.sm.segments_used = w.segs.size();
    return w;
}

// Segment::getAppendedLength's certificate of a segment holding `seg`, whose
// entries all have one length byte.
static ramcrc_seg_cert certOf(const std::string& seg)
{
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t at = 0; at < seg.size(); at += 2 + uint8_t(seg[at + 1]))
        crc = ramcrc_update(crc, seg.data() + at, 2);
    const uint32_t head = uint32_t(seg.size());
    uint8_t le[4];
    for (int k = 0; k < 4; k++)
        le[k] = uint8_t(head >> (8 * k));
    const ramcrc_seg_cert c = {head, ~ramcrc_update(crc, le, 4)};
    return c;
}

static int calls = 0;

static void run(ramcrc_replay_table_host* t, const std::vector<Batch*>& bs, uint64_t tableId, uint64_t first,
                uint64_t last, bool liveOnly, uint32_t startIndex, uint32_t startRecord, uint32_t cap,
                uint32_t maxSegments, bool haveSent, uint64_t sentCap)
{
    calls++;
    const Want w = expect(bs, tableId, first, last, liveOnly, startIndex, startRecord, cap, maxSegments, haveSent,
                          sentCap);
    std::vector<uint32_t> list;
    for (uint32_t b = 0; b < bs.size(); b++)
        list.push_back(b);
    Odd out(size_t(cap) * maxSegments), certs(8 * maxSegments), counts(16 * maxSegments), sent(8 * sentCap),
        segFirst(8 * maxSegments), summary(sizeof(ramcrc_migrate_summary));
    const int rc = ramcrc_replay_table_migrate_host(
        t, &list[0], uint32_t(list.size()), tableId, first, last, liveOnly ? RAMCRC_MIGRATE_LIVE_ONLY : 0u,
        startIndex, startRecord, out.p(), cap, cap, maxSegments, reinterpret_cast<ramcrc_seg_cert*>(certs.p()),
        reinterpret_cast<ramcrc_migrate_count*>(counts.p()),
        haveSent ? reinterpret_cast<ramcrc_replay_ref*>(sent.p()) : NULL, haveSent ? sentCap : 0,
        reinterpret_cast<uint64_t*>(segFirst.p()), reinterpret_cast<ramcrc_migrate_summary*>(summary.p()));
    CHECK(rc == RAMCRC_OK);
    ramcrc_migrate_summary sm;
    memcpy(&sm, summary.p(), sizeof sm);
    CHECK(memcmp(&sm, &w.sm, sizeof sm) == 0);
    if (sm.segments_used != w.segs.size())
        return;
    const size_t used = w.segs.size();
    for (size_t k = 0; k < used; k++) {
        ramcrc_seg_cert c;
        ramcrc_migrate_count n;
        uint64_t f;
        memcpy(&c, certs.p() + 8 * k, 8);
        memcpy(&n, counts.p() + 16 * k, 16);
        memcpy(&f, segFirst.p() + 8 * k, 8);
        const ramcrc_seg_cert e = certOf(w.segs[k]);
        CHECK(c.segment_length == e.segment_length && c.checksum == e.checksum);
        CHECK(n.objects == w.objects[k] && n.tombstones == w.tombstones[k] && n.entries == n.objects + n.tombstones &&
              n.reserved == 0 && f == w.first[k]);
        CHECK(memcmp(out.p() + k * cap, w.segs[k].data(), w.segs[k].size()) == 0);
        bool pastHeadUntouched = true;
        for (size_t i = w.segs[k].size(); i < cap; i++)
            pastHeadUntouched = pastHeadUntouched && out.p()[k * cap + i] == 0xA5;
        CHECK(pastHeadUntouched);
    }
    CHECK(out.untouched(used * cap) && certs.untouched(8 * used) && counts.untouched(16 * used) &&
          segFirst.untouched(8 * used));
    if (haveSent) {
        for (size_t j = 0; j < w.sent.size(); j++) {
            ramcrc_replay_ref r;
            memcpy(&r, sent.p() + 8 * j, 8);
            CHECK(r.batch == w.sent[j].first && r.record == w.sent[j].second);
        }
        CHECK(sent.untouched(8 * w.sent.size()));
    } else {
        CHECK(sent.untouched(0));
    }
}

int main()
{
    ramcrc_replay_table_host* t = NULL;
    CHECK(ramcrc_replay_table_create_host(256, 4, &t) == RAMCRC_OK);
    Batch b0, b1, b2;
    // hashes are the caller's: 1000 * key number
    for (int i = 0; i < 12; i++) {
        char key[16];
        snprintf(key, sizeof key, "key %d", i);
        b0.object(i % 4 == 3 ? 8 : 7, key, 1, 1000 * i, 5 + 7 * i);
    }
    b0.rpcResult(7, 3000);
    b1.object(7, "key 2", 2, 2000, 30);          // an overwrite
    b1.tombstone(7, "key 4", 1, 4000);           // a tombstone of the object's version: it wins
    b1.tombstone(7, "key 5", 0, 5000);           // a stale tombstone
    b1.object(8, "key 3", 3, 3000, 9);
    b2.object(7, "key 12", 1, 12000, 200);       // the largest entry: 2 + 27 + 6 + 200 = 235 bytes
    b2.object(7, "key 2", 1, 2000, 1);           // a stale object
    CHECK(b0.add(t, 0) && b1.add(t, 1) && b2.add(t, 2));
    std::vector<Batch*> bs;
    bs.push_back(&b0);
    bs.push_back(&b1);
    bs.push_back(&b2);
    const uint64_t all = ~0ull;
    for (int live = 0; live < 2; live++) {
        // capacities from 64 bytes (several entries are too large) up; every max_segments
        const uint32_t caps[] = {64, 80, 128, 240, 256, 4096};
        for (size_t c = 0; c < sizeof caps / sizeof caps[0]; c++)
            for (uint32_t nseg = 0; nseg <= 12; nseg++)
                run(t, bs, 7, 0, all, live, 0, 0, caps[c], nseg, true, 32);
        // hash ranges: the ends included, one above and one below, first > last
        const uint64_t ranges[][2] = {{2000, 5000}, {2001, 5000}, {2000, 4999}, {2001, 4999}, {5000, 2000},
                                      {12000, 12000}, {12001, all}, {0, 0}};
        for (size_t r = 0; r < sizeof ranges / sizeof ranges[0]; r++)
            for (uint64_t tid = 7; tid <= 9; tid++)
                run(t, bs, tid, ranges[r][0], ranges[r][1], live, 0, 0, 256, 8, true, 32);
        // every start cursor, the end's included
        for (uint32_t b = 0; b < 3; b++)
            for (uint32_t i = 0; i <= bs[b]->recs.size(); i++)
                run(t, bs, 7, 0, all, live, b, i, 128, 3, true, 32);
        run(t, bs, 7, 0, all, live, 3, 0, 128, 3, true, 32);
        // d_sent: none, empty, short by one
        run(t, bs, 7, 0, all, live, 0, 0, 256, 12, false, 0);
        for (uint64_t cap = 0; cap <= 14; cap++)
            run(t, bs, 7, 0, all, live, 0, 0, 256, 12, true, cap);
    }
    // the EINVAL list
    const uint32_t list[] = {0, 1, 2, 1, 5};
    Odd out(512), certs(16), counts(32), summary(sizeof(ramcrc_migrate_summary));
    ramcrc_seg_cert* pc = reinterpret_cast<ramcrc_seg_cert*>(certs.p());
    ramcrc_migrate_count* pn = reinterpret_cast<ramcrc_migrate_count*>(counts.p());
    ramcrc_migrate_summary* ps = reinterpret_cast<ramcrc_migrate_summary*>(summary.p());
#define EINVAL_CALL(T, L, N, FL, SI, SR, CAP, STR, NS, PS)                                                  \
    CHECK(ramcrc_replay_table_migrate_host(T, L, N, 7, 0, all, FL, SI, SR, out.p(), CAP, STR, NS, pc, pn,   \
                                           NULL, 0, NULL, PS) == RAMCRC_EINVAL)
    EINVAL_CALL(NULL, list, 3, 0, 0, 0, 256, 256, 2, ps);
    EINVAL_CALL(t, NULL, 3, 0, 0, 0, 256, 256, 2, ps);
    EINVAL_CALL(t, list, 0, 0, 0, 0, 256, 256, 2, ps);
    EINVAL_CALL(t, list, 4, 0, 0, 0, 256, 256, 2, ps);       // batch 1 twice
    EINVAL_CALL(t, list + 4, 1, 0, 0, 0, 256, 256, 2, ps);   // never added
    EINVAL_CALL(t, list, 3, 2, 0, 0, 256, 256, 2, ps);       // an unknown flag
    EINVAL_CALL(t, list, 3, 0, 4, 0, 256, 256, 2, ps);
    EINVAL_CALL(t, list, 3, 0, 3, 1, 256, 256, 2, ps);
    EINVAL_CALL(t, list, 3, 0, 1, 5, 256, 256, 2, ps);       // batch 1 has 4 records
    EINVAL_CALL(t, list, 3, 0, 0, 0, 250, 256, 2, ps);
    EINVAL_CALL(t, list, 3, 0, 0, 0, 256, 264, 2, ps);
    EINVAL_CALL(t, list, 3, 0, 0, 0, 256, 240, 2, ps);
    EINVAL_CALL(t, list, 3, 0, 0, 0, 256, 256, 2, NULL);
    CHECK(out.untouched(0) && certs.untouched(0) && counts.untouched(0) && summary.untouched(0));
    CHECK(ramcrc_replay_table_destroy_host(t) == RAMCRC_OK);
    printf("%d calls, %d mismatches\n", calls, bad);
    return bad ? 1 : 0;
}
