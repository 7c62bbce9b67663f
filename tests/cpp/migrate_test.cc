// RAMCloud::ReplayTable::migrateTablet as a master migrates a tablet out of the
// table it serves from: log segments arrive in three batches (two segments,
// one, one), each is verified and added as it arrives, and after each add the
// tablet [0, 2^63) of table 1 is migrated from the batches so far -- first in
// one call, then chained by the cursor one transfer segment a call -- in both
// modes, into 256-byte transfer segments.  Outputs, certificates, counts, the
// sent references, first indices and summaries are compared with the host form
// (ramcrc_replay_table_migrate_host) over a host table fed the same batches;
// then the transfer segments are verified under their certificates and added
// to a second table, as the receiving master does.  Built with hipcc for
// hipMalloc.
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "Crc32C.h"
#include "Crc32CBatch.h"

using namespace RAMCloud;

static const uint32_t kCap = 64 * 1024;
static const uint32_t kRecords = 150, kKeys = 50;
static const uint32_t kBatches = 3;
static const uint32_t kSegs[kBatches] = {2, 1, 1};
static const uint32_t kOutCap = 256, kMaxSegs = 128;
static const uint64_t kEcap = 512, kSentCap = 1024;

struct Builder {
    uint8_t* seg;
    uint32_t pos;
    Crc32C meta;
    void append(uint8_t type, const std::vector<uint8_t>& payload)
    {
        const uint32_t len = uint32_t(payload.size());   // < 256 here
        seg[pos] = type;
        seg[pos + 1] = uint8_t(len);
        meta.update(&seg[pos], 2);
        memcpy(&seg[pos + 2], payload.data(), len);
        pos += 2 + len;
    }
    ramcrc_seg_cert cert()
    {
        ramcrc_seg_cert c;
        c.segment_length = pos;
        meta.update(&pos, 4);
        c.checksum = meta.getResult();
        return c;
    }
};

static void put64(std::vector<uint8_t>& v, size_t at, uint64_t x) { memcpy(&v[at], &x, 8); }

// SEGHEADER, safe version 1 + s, then objects and tombstones of tables 1 and 2
static ramcrc_seg_cert fill(uint8_t* seg, uint32_t s)
{
    Builder b = {seg, 0, Crc32C()};
    std::vector<uint8_t> h(24, 0);
    put64(h, 8, 10 + s);
    b.append(RAMCRC_LOG_ENTRY_TYPE_SEGHEADER, h);
    std::vector<uint8_t> sv(12, 0);
    sv[0] = uint8_t(1 + s);
    b.append(RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION, sv);
    for (uint32_t k = 0; k < kRecords; k++) {
        const std::string key = std::to_string(k % kKeys);
        const uint64_t version = (k * 7 + s * 3) % 5, tableId = 1 + k % 3 / 2;
        if ((k + s) % 7) {
            std::vector<uint8_t> o(24 + 1 + 2 + key.size() + k % 40, uint8_t(k));
            memset(&o[0], 0, 24);
            put64(o, 8, version);
            put64(o, 16, tableId);
            o[24] = 1;
            o[25] = uint8_t(key.size());
            o[26] = 0;
            memcpy(&o[27], key.data(), key.size());
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o);
        } else {
            std::vector<uint8_t> t(32 + key.size(), 0);
            put64(t, 0, tableId);
            put64(t, 8, 3);
            put64(t, 16, version);
            memcpy(&t[32], key.data(), key.size());
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, t);
        }
    }
    return b.cert();
}

#define HIP(expr)                                                \
    do {                                                         \
        if ((expr) != hipSuccess) {                              \
            fprintf(stderr, "%s failed\n", #expr);               \
            return 1;                                            \
        }                                                        \
    } while (0)

template <typename T>
static T* dalloc(size_t n)
{
    void* p = NULL;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess)
        throw std::runtime_error("hipMalloc failed");
    return static_cast<T*>(p);
}

struct Arrived {
    uint32_t nseg;
    std::vector<uint8_t> host;
    std::vector<ramcrc_seg_cert> certs;
    std::vector<ramcrc_seg_status> status;
    std::vector<ramcrc_seg_entry> table;
    std::vector<uint64_t> hostWork;
    uint8_t* d_base;
    ramcrc_seg_cert* d_certs;
    ramcrc_seg_status* d_status;
    ramcrc_seg_entry* d_entries;
    uint64_t *d_n, *d_work;
    uint32_t* d_crc;
};

// One migration's outputs on the host.
struct Outs {
    std::vector<uint8_t> out;
    std::vector<ramcrc_seg_cert> certs;
    std::vector<ramcrc_migrate_count> counts;
    std::vector<ramcrc_replay_ref> sent;
    std::vector<uint64_t> first;
    ramcrc_migrate_summary sm;
    Outs() : out(size_t(kOutCap) * kMaxSegs, 0xA5), certs(kMaxSegs), counts(kMaxSegs), sent(kSentCap), first(kMaxSegs)
    {
        memset(&certs[0], 0xA5, kMaxSegs * sizeof certs[0]);
        memset(&counts[0], 0xA5, kMaxSegs * sizeof counts[0]);
        memset(&sent[0], 0xA5, kSentCap * sizeof sent[0]);
        memset(&first[0], 0xA5, kMaxSegs * 8);
        memset(&sm, 0xA5, sizeof sm);
    }
    bool same(const Outs& o) const
    {
        return out == o.out && memcmp(&certs[0], &o.certs[0], kMaxSegs * sizeof certs[0]) == 0 &&
               memcmp(&counts[0], &o.counts[0], kMaxSegs * sizeof counts[0]) == 0 &&
               memcmp(&sent[0], &o.sent[0], kSentCap * sizeof sent[0]) == 0 && first == o.first &&
               memcmp(&sm, &o.sm, sizeof sm) == 0;
    }
};

static int run();

int main()
{
    try {
        return run();
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
}

static int run()
{
    Crc32CBatch batch(0);
    ReplayTable table(batch, 4 * kKeys, kBatches);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(4 * kKeys, kBatches, &hostTable))
        return 1;
    uint8_t* d_out = dalloc<uint8_t>(size_t(kOutCap) * kMaxSegs);
    ramcrc_seg_cert* d_certs = dalloc<ramcrc_seg_cert>(kMaxSegs);
    ramcrc_migrate_count* d_counts = dalloc<ramcrc_migrate_count>(kMaxSegs);
    ramcrc_replay_ref* d_sent = dalloc<ramcrc_replay_ref>(kSentCap);
    uint64_t* d_first = dalloc<uint64_t>(kMaxSegs);
    ramcrc_migrate_summary* d_sm = dalloc<ramcrc_migrate_summary>(1);
    const uint64_t lastHash = (1ull << 63) - 1;

    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0, list[kBatches];
    uint64_t sentAtEnd = 0, segsAtEnd = 0;
    for (uint32_t j = 0; j < kBatches; j++) {
        Arrived& a = arrived[j];
        list[j] = j;
        a.nseg = kSegs[j];
        a.host.assign(a.nseg * kCap, 0);
        a.certs.resize(a.nseg);
        a.status.resize(a.nseg);
        for (uint32_t s = 0; s < a.nseg; s++)
            a.certs[s] = fill(&a.host[s * kCap], seg++);
        a.d_base = dalloc<uint8_t>(a.host.size());
        a.d_certs = dalloc<ramcrc_seg_cert>(a.nseg);
        a.d_status = dalloc<ramcrc_seg_status>(a.nseg);
        a.d_entries = dalloc<ramcrc_seg_entry>(kEcap);
        a.d_n = dalloc<uint64_t>(1);
        a.d_work = dalloc<uint64_t>(kEcap);
        a.d_crc = dalloc<uint32_t>(kEcap);
        HIP(hipMemcpy(a.d_base, &a.host[0], a.host.size(), hipMemcpyHostToDevice));
        HIP(hipMemcpy(a.d_certs, &a.certs[0], a.nseg * sizeof(ramcrc_seg_cert), hipMemcpyHostToDevice));
        batch.deviceReplayVerify(a.d_base, kCap, kCap, a.nseg, a.d_certs, a.d_status, a.d_entries,
                                 kEcap, a.d_n, a.d_crc);
        bad += table.add(a.d_base, kCap, a.nseg, a.d_status, a.d_entries, kEcap, a.d_n, NULL,
                         a.d_work) != j;
        batch.sync();
        uint64_t n = 0;
        HIP(hipMemcpy(&n, a.d_n, 8, hipMemcpyDeviceToHost));
        if (n != a.nseg * (kRecords + 2)) {
            fprintf(stderr, "walk found %llu records\n", static_cast<unsigned long long>(n));
            return 1;
        }
        a.table.resize(n);
        a.hostWork.resize(n);
        HIP(hipMemcpy(&a.table[0], a.d_entries, n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&a.status[0], a.d_status, a.nseg * sizeof(ramcrc_seg_status),
                      hipMemcpyDeviceToHost));
        uint32_t hostNumber = ~0u;
        if (ramcrc_replay_table_add_host(hostTable, &a.host[0], kCap, a.nseg, &a.status[0],
                                         &a.table[0], n, NULL, &a.hostWork[0], &hostNumber) ||
            hostNumber != j)
            return 1;

        for (uint32_t flags = 0; flags <= RAMCRC_MIGRATE_LIVE_ONLY; flags++) {
            // one call, then the same chained one transfer segment a call
            Outs whole;
            for (int chained = 0; chained < 2; chained++) {
                Outs got, want;
                HIP(hipMemset(d_out, 0xA5, size_t(kOutCap) * kMaxSegs));
                HIP(hipMemset(d_certs, 0xA5, kMaxSegs * sizeof *d_certs));
                HIP(hipMemset(d_counts, 0xA5, kMaxSegs * sizeof *d_counts));
                HIP(hipMemset(d_sent, 0xA5, kSentCap * sizeof *d_sent));
                HIP(hipMemset(d_first, 0xA5, kMaxSegs * 8));
                uint32_t at[2] = {0, 0};
                uint64_t segs = 0, sent = 0;
                for (uint32_t call = 0; call <= kMaxSegs; call++) {
                    const uint32_t nseg = chained ? 1 : kMaxSegs;
                    table.migrateTablet(list, j + 1, 1, 0, lastHash, flags, at[0], at[1], d_out + segs * kOutCap,
                                        kOutCap, kOutCap, nseg, d_certs + segs, d_counts + segs, d_sent + sent,
                                        kSentCap - sent, d_first + segs, d_sm);
                    batch.sync();
                    HIP(hipMemcpy(&got.sm, d_sm, sizeof got.sm, hipMemcpyDeviceToHost));
                    if (ramcrc_replay_table_migrate_host(hostTable, list, j + 1, 1, 0, lastHash, flags, at[0], at[1],
                                                         &want.out[segs * kOutCap], kOutCap, kOutCap, nseg,
                                                         &want.certs[segs], &want.counts[segs], &want.sent[sent],
                                                         kSentCap - sent, &want.first[segs], &want.sm))
                        return 1;
                    bad += memcmp(&got.sm, &want.sm, sizeof got.sm) != 0 || got.sm.too_large || got.sm.spoiled;
                    segs += got.sm.segments_used;
                    sent += got.sm.sent_objects + got.sm.sent_tombstones;
                    at[0] = uint32_t(got.sm.next_index);
                    at[1] = uint32_t(got.sm.next_record);
                    if (got.sm.done || segs >= kMaxSegs)
                        break;
                }
                bad += !got.sm.done || segs < 3 || sent == 0;
                HIP(hipMemcpy(&got.out[0], d_out, got.out.size(), hipMemcpyDeviceToHost));
                HIP(hipMemcpy(&got.certs[0], d_certs, kMaxSegs * sizeof got.certs[0], hipMemcpyDeviceToHost));
                HIP(hipMemcpy(&got.counts[0], d_counts, kMaxSegs * sizeof got.counts[0], hipMemcpyDeviceToHost));
                HIP(hipMemcpy(&got.sent[0], d_sent, kSentCap * sizeof got.sent[0], hipMemcpyDeviceToHost));
                HIP(hipMemcpy(&got.first[0], d_first, kMaxSegs * 8, hipMemcpyDeviceToHost));
                bad += !got.same(want);
                if (!chained) {
                    whole = got;
                    sentAtEnd = sent;
                    segsAtEnd = segs;
                } else {
                    // K calls of one segment write what one call with K writes
                    bad += got.out != whole.out || segs != segsAtEnd || sent != sentAtEnd ||
                           memcmp(&got.certs[0], &whole.certs[0], kMaxSegs * sizeof got.certs[0]) != 0 ||
                           memcmp(&got.sent[0], &whole.sent[0], kSentCap * sizeof got.sent[0]) != 0;
                }
            }
        }
    }
    // the receiving master: the last migration's transfer segments (live-only,
    // chained), verified under their certificates and added to its own table
    {
        ReplayTable dest(batch, 4 * kKeys, 1);
        ramcrc_seg_status* d_status = dalloc<ramcrc_seg_status>(kMaxSegs);
        ramcrc_seg_entry* d_entries = dalloc<ramcrc_seg_entry>(kSentCap);
        uint64_t* d_n = dalloc<uint64_t>(1);
        uint64_t* d_work = dalloc<uint64_t>(kSentCap);
        uint32_t* d_crc = dalloc<uint32_t>(kSentCap);
        ramcrc_replay_table_stats* d_stats = dalloc<ramcrc_replay_table_stats>(1);
        batch.deviceReplayVerify(d_out, kOutCap, kOutCap, segsAtEnd, d_certs, d_status, d_entries, kSentCap, d_n,
                                 d_crc);
        bad += dest.add(d_out, kOutCap, segsAtEnd, d_status, d_entries, kSentCap, d_n, NULL, d_work) != 0;
        dest.stats(d_stats);
        batch.sync();
        std::vector<ramcrc_seg_status> st(segsAtEnd);
        ramcrc_replay_table_stats stats;
        uint64_t n = 0;
        HIP(hipMemcpy(&st[0], d_status, segsAtEnd * sizeof st[0], hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&stats, d_stats, sizeof stats, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&n, d_n, 8, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < segsAtEnd; k++)
            bad += st[k].flags != RAMCRC_SEG_OK;
        // live-only sends one record a key: every one is a winner there too
        bad += n != sentAtEnd || stats.keys != sentAtEnd || stats.spoiled;
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("migrate: %llu entries in %llu transfer segments at the end; %d mismatches\n",
           static_cast<unsigned long long>(sentAtEnd), static_cast<unsigned long long>(segsAtEnd), bad);
    return bad ? 1 : 0;
}
