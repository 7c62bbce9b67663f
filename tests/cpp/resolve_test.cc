// Crc32CBatch::deviceReplayResolve as a recovery master would call it after
// deviceReplayVerify: three recovery segments that open with a SEGHEADER and a
// safe version and hold objects and tombstones of table 1 under keys "0" ..
// "49" with versions 0 .. 4 (one segment with a wrong certificate in the
// second round).  The winners, the live list and the counters are compared
// with ramcrc_replay_resolve_host, with the partition call's hashes and with
// computed ones; the list then goes through deviceRecoveryAppend unchanged
// with one partition.  Built with hipcc for hipMalloc.
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
static const uint32_t kSeg = 3, kRecords = 150, kKeys = 50;

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
    std::vector<uint8_t> host(kSeg * kCap, 0);
    ramcrc_seg_cert certs[kSeg];
    for (uint32_t s = 0; s < kSeg; s++)
        certs[s] = fill(&host[s * kCap], s);
    const ramcrc_tablet tablets[1] = {{1, 0, ~0ull, 0, 0, 0}};
    const uint64_t cap = 512, lcap = 512;
    // device buffers (freed with the process)
    uint8_t* d_base = dalloc<uint8_t>(host.size());
    ramcrc_seg_cert* d_certs = dalloc<ramcrc_seg_cert>(kSeg);
    ramcrc_seg_status* d_status = dalloc<ramcrc_seg_status>(kSeg);
    ramcrc_seg_entry* d_entries = dalloc<ramcrc_seg_entry>(cap);
    uint64_t *d_n = dalloc<uint64_t>(1), *d_np = dalloc<uint64_t>(1), *d_nl = dalloc<uint64_t>(1);
    uint64_t* d_hash = dalloc<uint64_t>(cap);
    uint32_t *d_crc = dalloc<uint32_t>(cap), *d_winner = dalloc<uint32_t>(cap);
    ramcrc_tablet* d_tab = dalloc<ramcrc_tablet>(1);
    ramcrc_placement *d_place = dalloc<ramcrc_placement>(cap), *d_live = dalloc<ramcrc_placement>(lcap);
    ramcrc_partition_status* d_ps = dalloc<ramcrc_partition_status>(kSeg);
    ramcrc_resolve_counts* d_counts = dalloc<ramcrc_resolve_counts>(1);
    uint8_t* d_out = dalloc<uint8_t>(host.size());
    ramcrc_seg_cert* d_oc = dalloc<ramcrc_seg_cert>(kSeg);
    ramcrc_append_status* d_os = dalloc<ramcrc_append_status>(kSeg);
    HIP(hipMemcpy(d_base, &host[0], host.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_tab, tablets, sizeof tablets, hipMemcpyHostToDevice));
    Crc32CBatch batch(0);
    int bad = 0;
    uint64_t kept = 0;
    for (int round = 0; round < 2; round++) {
        // round 1: segment 2 fails its metadata check and takes no part
        if (round)
            certs[2].checksum ^= 1;
        HIP(hipMemcpy(d_certs, certs, sizeof certs, hipMemcpyHostToDevice));
        batch.deviceReplayVerify(d_base, kCap, kCap, kSeg, d_certs, d_status, d_entries, cap, d_n,
                                 d_crc);
        batch.deviceRecoveryPartition(d_base, kCap, kSeg, d_status, d_entries, cap, d_n, d_tab, 1, 1,
                                      d_place, cap, d_np, d_hash, d_ps);
        uint64_t n = 0;
        HIP(hipMemcpy(&n, d_n, 8, hipMemcpyDeviceToHost));
        if (n != kSeg * (kRecords + 2)) {
            fprintf(stderr, "walk found %llu records\n", static_cast<unsigned long long>(n));
            return 1;
        }
        std::vector<ramcrc_seg_entry> table(n);
        ramcrc_seg_status st[kSeg];
        HIP(hipMemcpy(&table[0], d_entries, n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(st, d_status, sizeof st, hipMemcpyDeviceToHost));
        std::vector<uint32_t> wantWinner(n);
        std::vector<ramcrc_placement> wantLive(lcap);
        uint64_t wantNl = 0;
        ramcrc_resolve_counts wantCounts;
        if (ramcrc_replay_resolve_host(&host[0], kCap, kSeg, st, &table[0], n, NULL, &wantWinner[0],
                                       &wantLive[0], lcap, &wantNl, &wantCounts))
            return 1;
        // with the partition call's hashes, then with computed ones
        for (int given = 1; given >= 0; given--) {
            HIP(hipMemset(d_live, 0xA5, lcap * sizeof(ramcrc_placement)));
            HIP(hipMemset(d_winner, 0xA5, cap * 4));
            batch.deviceReplayResolve(d_base, kCap, kSeg, d_status, d_entries, cap, d_n,
                                      given ? d_hash : NULL, d_winner, d_live, lcap, d_nl, d_counts);
            std::vector<uint32_t> winner(cap);
            std::vector<ramcrc_placement> live(lcap);
            uint64_t nl = 0;
            ramcrc_resolve_counts counts;
            HIP(hipMemcpy(&winner[0], d_winner, cap * 4, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&live[0], d_live, lcap * sizeof(ramcrc_placement), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&nl, d_nl, 8, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
            bad += nl != wantNl || nl > lcap ||
                   memcmp(&live[0], &wantLive[0], nl * sizeof(ramcrc_placement)) != 0;
            bad += memcmp(&winner[0], &wantWinner[0], n * 4) != 0;
            bad += memcmp(&counts, &wantCounts, sizeof counts) != 0;
            for (uint64_t i = nl; i < lcap; i++)
                bad += live[i].record != 0xA5A5A5A5u;   // slots past the list keep their fill
            for (uint64_t i = n; i < cap; i++)
                bad += winner[i] != 0xA5A5A5A5u;
            // every key is in every segment: one winner per key
            bad += nl != kKeys || counts.live_objects + counts.live_tombstones != kKeys;
            bad += counts.objects + counts.tombstones != (round ? 2u : 3u) * kRecords;
            bad += counts.safe_version != (round ? 2u : 3u) || counts.malformed != 0;
        }
        batch.deviceRecoveryAppend(d_base, kCap, kSeg, d_status, d_entries, cap, d_n, d_live, lcap, d_nl,
                                   1, d_out, kCap, kCap, d_oc, d_os);
        ramcrc_append_status os[kSeg];
        HIP(hipMemcpy(os, d_os, sizeof os, hipMemcpyDeviceToHost));
        uint32_t perSeg[kSeg] = {};
        for (uint64_t i = 0; i < wantNl; i++)
            perSeg[table[wantLive[i].record].segment]++;
        for (uint32_t s = 0; s < kSeg; s++)
            bad += os[s].entries != perSeg[s] ||
                   os[s].flags != ((round && s == 2) ? RAMCRC_SEG_SOURCE_BAD : RAMCRC_SEG_OK);
        kept += wantNl;
    }
    printf("replay resolve: %llu live records over 2 rounds; %d mismatches\n",
           static_cast<unsigned long long>(kept), bad);
    return bad ? 1 : 0;
}
