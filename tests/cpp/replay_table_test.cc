// RAMCloud::ReplayTable as a recovery master would drive it: recovery segments
// arrive in two batches (two segments, then one), each is verified and added
// as it arrives, and at the end every batch's live list goes through
// deviceRecoveryAppend with one partition.  The segments open with a SEGHEADER
// and a safe version and hold objects and tombstones of table 1 under keys
// "0" .. "49" with versions 0 .. 4, so most keys of batch 0 meet a newer or an
// equal record in batch 1.  Winners, live lists, counters and stats are
// compared with the host form (ramcrc_replay_table_*_host) after each add; the
// appended entry counts are the lists'.  Built with hipcc for hipMalloc.
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
static const uint32_t kBatches = 2;
static const uint32_t kSegs[kBatches] = {2, 1};

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

// SEGHEADER, safe version 1 + s, then objects and tombstones
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
        const uint64_t version = (k * 7 + s * 3) % 5;
        if ((k + s) % 3) {
            // Object::Header {checksum, timestamp, version, tableId}, KeyCount,
            // CumulativeKeyLength, key, value
            std::vector<uint8_t> o(24 + 1 + 2 + key.size() + k % 40, uint8_t(k));
            put64(o, 8, version);
            put64(o, 16, 1);
            o[24] = 1;
            o[25] = uint8_t(key.size());
            o[26] = 0;
            memcpy(&o[27], key.data(), key.size());
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o);
        } else {
            // ObjectTombstone::Header {tableId, segmentId, objectVersion, timestamp, checksum}, key
            std::vector<uint8_t> t(32 + key.size(), 0);
            put64(t, 0, 1);
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

// One arriving batch: its segments and everything the table keeps reading.
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
    uint64_t *d_n, *d_work, *d_nl;
    uint32_t* d_crc;
    ramcrc_replay_ref* d_winner;
    ramcrc_placement* d_live;
    ramcrc_resolve_counts* d_counts;
};

static const uint64_t kEcap = 512, kLcap = 512;

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

// live() of batch j on the device against the host table's; returns mismatches.
static int compare(ReplayTable& table, Crc32CBatch& batch, ramcrc_replay_table_host* hostTable,
                   Arrived& a, uint32_t j, uint64_t* kept)
{
    int bad = 0;
    const uint64_t n = a.table.size();
    std::vector<ramcrc_replay_ref> wantWinner(n);
    std::vector<ramcrc_placement> wantLive(kLcap);
    uint64_t wantNl = 0;
    ramcrc_resolve_counts wantCounts;
    if (ramcrc_replay_table_live_host(hostTable, j, &wantWinner[0], &wantLive[0], kLcap, &wantNl,
                                      &wantCounts))
        return 1000;
    if (hipMemset(a.d_live, 0xA5, kLcap * sizeof(ramcrc_placement)) != hipSuccess ||
        hipMemset(a.d_winner, 0xA5, kEcap * sizeof(ramcrc_replay_ref)) != hipSuccess)
        return 1000;
    table.live(j, a.d_winner, a.d_live, kLcap, a.d_nl, a.d_counts);
    batch.sync();
    std::vector<ramcrc_replay_ref> winner(kEcap);
    std::vector<ramcrc_placement> live(kLcap);
    uint64_t nl = 0;
    ramcrc_resolve_counts counts;
    if (hipMemcpy(&winner[0], a.d_winner, kEcap * sizeof(ramcrc_replay_ref), hipMemcpyDeviceToHost) !=
            hipSuccess ||
        hipMemcpy(&live[0], a.d_live, kLcap * sizeof(ramcrc_placement), hipMemcpyDeviceToHost) !=
            hipSuccess ||
        hipMemcpy(&nl, a.d_nl, 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&counts, a.d_counts, sizeof counts, hipMemcpyDeviceToHost) != hipSuccess)
        return 1000;
    bad += nl != wantNl || nl > kLcap ||
           memcmp(&live[0], &wantLive[0], nl * sizeof(ramcrc_placement)) != 0;
    bad += memcmp(&winner[0], &wantWinner[0], n * sizeof(ramcrc_replay_ref)) != 0;
    bad += memcmp(&counts, &wantCounts, sizeof counts) != 0;
    for (uint64_t i = nl; i < kLcap; i++)
        bad += live[i].record != 0xA5A5A5A5u;   // slots past the list keep their fill
    for (uint64_t i = n; i < kEcap; i++)
        bad += winner[i].batch != 0xA5A5A5A5u;
    bad += counts.objects + counts.tombstones != a.nseg * kRecords || counts.malformed != 0;
    *kept = nl;
    return bad;
}

static int run()
{
    Crc32CBatch batch(0);
    ReplayTable table(batch, 2 * kKeys, kBatches);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(2 * kKeys, kBatches, &hostTable))
        return 1;
    ramcrc_replay_table_stats* d_stats = dalloc<ramcrc_replay_table_stats>(1);
    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    for (uint32_t j = 0; j < kBatches; j++) {
        // the batch arrives: device buffers (freed with the process), walk, verify
        Arrived& a = arrived[j];
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
        a.d_nl = dalloc<uint64_t>(1);
        a.d_work = dalloc<uint64_t>(kEcap);
        a.d_crc = dalloc<uint32_t>(kEcap);
        a.d_winner = dalloc<ramcrc_replay_ref>(kEcap);
        a.d_live = dalloc<ramcrc_placement>(kLcap);
        a.d_counts = dalloc<ramcrc_resolve_counts>(1);
        HIP(hipMemcpy(a.d_base, &a.host[0], a.host.size(), hipMemcpyHostToDevice));
        HIP(hipMemcpy(a.d_certs, &a.certs[0], a.nseg * sizeof(ramcrc_seg_cert), hipMemcpyHostToDevice));
        batch.deviceReplayVerify(a.d_base, kCap, kCap, a.nseg, a.d_certs, a.d_status, a.d_entries,
                                 kEcap, a.d_n, a.d_crc);
        // ... and is resolved into the table at once
        const uint32_t number = table.add(a.d_base, kCap, a.nseg, a.d_status, a.d_entries, kEcap,
                                          a.d_n, NULL, a.d_work);
        batch.sync();
        bad += number != j;
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
        // the verdict on every batch so far, as the table stands now
        for (uint32_t q = 0; q <= j; q++) {
            uint64_t kept = 0;
            bad += compare(table, batch, hostTable, arrived[q], q, &kept);
        }
    }
    // every key is in every segment: one winner per key over the two batches
    ramcrc_replay_table_stats stats, wantStats;
    table.stats(d_stats);
    batch.sync();
    HIP(hipMemcpy(&stats, d_stats, sizeof stats, hipMemcpyDeviceToHost));
    if (ramcrc_replay_table_stats_host(hostTable, &wantStats))
        return 1;
    bad += memcmp(&stats, &wantStats, sizeof stats) != 0;
    bad += stats.keys != kKeys || stats.live_objects + stats.live_tombstones != kKeys ||
           stats.safe_version != 3 || stats.batches != kBatches || stats.spoiled != 0;
    // the end of the recovery: live -> append with one partition, per batch
    uint64_t total = 0;
    for (uint32_t j = 0; j < kBatches; j++) {
        Arrived& a = arrived[j];
        uint64_t kept = 0;
        bad += compare(table, batch, hostTable, a, j, &kept);
        total += kept;
        uint8_t* d_out = dalloc<uint8_t>(a.host.size());
        ramcrc_seg_cert* d_oc = dalloc<ramcrc_seg_cert>(a.nseg);
        ramcrc_append_status* d_os = dalloc<ramcrc_append_status>(a.nseg);
        batch.deviceRecoveryAppend(a.d_base, kCap, a.nseg, a.d_status, a.d_entries, kEcap, a.d_n,
                                   a.d_live, kLcap, a.d_nl, 1, d_out, kCap, kCap, d_oc, d_os);
        std::vector<ramcrc_append_status> os(a.nseg);
        std::vector<ramcrc_placement> live(kLcap);
        HIP(hipMemcpy(&os[0], d_os, a.nseg * sizeof(ramcrc_append_status), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&live[0], a.d_live, kLcap * sizeof(ramcrc_placement), hipMemcpyDeviceToHost));
        std::vector<uint32_t> perSeg(a.nseg, 0);
        for (uint64_t i = 0; i < kept; i++)
            perSeg[a.table[live[i].record].segment]++;
        for (uint32_t s = 0; s < a.nseg; s++)
            bad += os[s].entries != perSeg[s] || os[s].flags != RAMCRC_SEG_OK;
    }
    bad += total != kKeys;
    // reset: the table is empty and takes batch 1's segments as its batch 0
    table.reset();
    bad += table.add(arrived[1].d_base, kCap, arrived[1].nseg, arrived[1].d_status,
                     arrived[1].d_entries, kEcap, arrived[1].d_n, NULL, arrived[1].d_work) != 0;
    table.stats(d_stats);
    batch.sync();
    HIP(hipMemcpy(&stats, d_stats, sizeof stats, hipMemcpyDeviceToHost));
    bad += stats.keys != kKeys || stats.batches != 1 || stats.safe_version != 3;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("replay table: %llu live records over %u batches; %d mismatches\n",
           static_cast<unsigned long long>(total), kBatches, bad);
    return bad ? 1 : 0;
}
