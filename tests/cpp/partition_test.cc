// Crc32CBatch::deviceRecoveryPartition as a backup would call it between
// deviceReplayVerify and deviceRecoveryAppend: two replicas that open with a
// SEGHEADER and a safe version and hold objects of tables 1 and 2 under keys
// "1", "2", ... (one replica with a wrong certificate), partitioned over the
// tablets of RecoverySegmentBuilderTest (src/RecoverySegmentBuilderTest.cc:56-60),
// whose boundary is the hash of (1, "1").  The list, the hashes and the
// counters are compared with ramcrc_recovery_partition_host and with the
// hashes that test prints; the list then goes through deviceRecoveryAppend
// unchanged.  Built with hipcc for hipMalloc.
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
static const uint32_t kSeg = 2, kPart = 2, kObjects = 200;
static const uint64_t kHashOneOne = 0xDD5D9F7F60D5B056ull;   // Key::getHash(1, "1", 1)
static const uint64_t kHashOneTwo = 0x3554F985FBED3C16ull;   // Key::getHash(1, "2", 1)

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

// SEGHEADER {logId, segmentId, capacity, checksum}, safe version 1, then the objects
static ramcrc_seg_cert fill(uint8_t* seg, uint64_t segmentId, uint32_t firstKey)
{
    Builder b = {seg, 0, Crc32C()};
    std::vector<uint8_t> h(24, 0);
    put64(h, 8, segmentId);
    b.append(RAMCRC_LOG_ENTRY_TYPE_SEGHEADER, h);
    std::vector<uint8_t> sv(12, 0);
    sv[0] = 1;
    b.append(RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION, sv);
    for (uint32_t k = 0; k < kObjects; k++) {
        const std::string key = std::to_string(firstKey + k / 2);
        // Object::Header (24 bytes, tableId last), KeyCount, CumulativeKeyLength, key, value
        std::vector<uint8_t> o(24 + 1 + 2 + key.size() + k % 40, uint8_t(k));
        put64(o, 16, 1 + k % 2);
        o[24] = 1;
        o[25] = uint8_t(key.size());
        o[26] = 0;
        memcpy(&o[27], key.data(), key.size());
        b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o);
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
    certs[0] = fill(&host[0], 1, 1);
    certs[1] = fill(&host[kCap], 1, 1000);
    const ramcrc_tablet tablets[4] = {
        {1, 0, kHashOneOne - 1, 0, 0, 0}, {1, kHashOneOne, ~0ull, 0, 0, 1},
        {2, 0, ~0ull, 2, 0, 0},           {3, 0, 1, 0, 0, 0}};
    const uint64_t cap = 512, pcap = 1024;
    const uint64_t outBytes = uint64_t(kSeg) * kPart * kCap;
    // device buffers (freed with the process)
    uint8_t* d_base = dalloc<uint8_t>(host.size());
    ramcrc_seg_cert* d_certs = dalloc<ramcrc_seg_cert>(kSeg);
    ramcrc_seg_status* d_status = dalloc<ramcrc_seg_status>(kSeg);
    ramcrc_seg_entry* d_entries = dalloc<ramcrc_seg_entry>(cap);
    uint64_t *d_n = dalloc<uint64_t>(1), *d_np = dalloc<uint64_t>(1), *d_hash = dalloc<uint64_t>(cap);
    uint32_t* d_crc = dalloc<uint32_t>(cap);
    ramcrc_tablet* d_tab = dalloc<ramcrc_tablet>(4);
    ramcrc_placement* d_place = dalloc<ramcrc_placement>(pcap);
    ramcrc_partition_status* d_ps = dalloc<ramcrc_partition_status>(kSeg);
    uint8_t* d_out = dalloc<uint8_t>(outBytes);
    ramcrc_seg_cert* d_oc = dalloc<ramcrc_seg_cert>(kSeg * kPart);
    ramcrc_append_status* d_os = dalloc<ramcrc_append_status>(kSeg * kPart);
    HIP(hipMemcpy(d_base, &host[0], host.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_tab, tablets, sizeof tablets, hipMemcpyHostToDevice));
    Crc32CBatch batch(0);
    int bad = 0;
    uint64_t placed = 0;
    for (int round = 0; round < 2; round++) {
        // round 1: replica 1 fails its metadata check and contributes nothing
        if (round)
            certs[1].checksum ^= 1;
        HIP(hipMemcpy(d_certs, certs, sizeof certs, hipMemcpyHostToDevice));
        HIP(hipMemset(d_place, 0xA5, pcap * sizeof(ramcrc_placement)));
        batch.deviceReplayVerify(d_base, kCap, kCap, kSeg, d_certs, d_status, d_entries, cap, d_n,
                                 d_crc);
        batch.deviceRecoveryPartition(d_base, kCap, kSeg, d_status, d_entries, cap, d_n, d_tab, 4,
                                      kPart, d_place, pcap, d_np, d_hash, d_ps);
        batch.deviceRecoveryAppend(d_base, kCap, kSeg, d_status, d_entries, cap, d_n, d_place, pcap,
                                   d_np, kPart, d_out, kCap, kCap, d_oc, d_os);
        uint64_t n = 0, np = 0;
        HIP(hipMemcpy(&n, d_n, 8, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&np, d_np, 8, hipMemcpyDeviceToHost));
        if (n != kSeg * (kObjects + 2) || np > pcap) {
            fprintf(stderr, "walk found %llu records, %llu placements\n",
                    static_cast<unsigned long long>(n), static_cast<unsigned long long>(np));
            return 1;
        }
        std::vector<ramcrc_seg_entry> table(n);
        std::vector<ramcrc_placement> place(pcap), wantPlace(pcap);
        std::vector<uint64_t> hash(n), wantHash(n);
        ramcrc_seg_status st[kSeg];
        ramcrc_partition_status ps[kSeg], wantPs[kSeg];
        ramcrc_append_status os[kSeg * kPart];
        HIP(hipMemcpy(&table[0], d_entries, n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&place[0], d_place, pcap * sizeof(ramcrc_placement), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&hash[0], d_hash, n * 8, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(st, d_status, sizeof st, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(ps, d_ps, sizeof ps, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(os, d_os, sizeof os, hipMemcpyDeviceToHost));
        uint64_t wantNp = 0;
        if (ramcrc_recovery_partition_host(&host[0], kCap, kSeg, st, &table[0], n, tablets, 4, kPart,
                                           &wantPlace[0], pcap, &wantNp, &wantHash[0], wantPs))
            return 1;
        bad += np != wantNp || memcmp(&place[0], &wantPlace[0], np * sizeof(ramcrc_placement)) != 0;
        bad += memcmp(&hash[0], &wantHash[0], n * 8) != 0 || memcmp(ps, wantPs, sizeof ps) != 0;
        // the first two objects of replica 0 are (1, "1") and (2, "1"); the third is (1, "2")
        uint32_t perOut[kSeg * kPart] = {};
        for (uint64_t i = 0; i < n; i++) {
            if (table[i].segment != 0 || (table[i].header & 0x3f) != RAMCRC_LOG_ENTRY_TYPE_OBJ)
                continue;
            bad += hash[i] != kHashOneOne || hash[i + 2] != kHashOneTwo;
            break;
        }
        for (uint64_t i = 0; i < np; i++) {
            bad += place[i].partition >= kPart || (i && place[i].record < place[i - 1].record);
            perOut[table[place[i].record].segment * kPart + place[i].partition]++;
        }
        for (uint64_t i = np; i < pcap; i++)
            bad += place[i].record != 0xA5A5A5A5u;   // slots past the list keep their fill
        for (uint32_t k = 0; k < kSeg * kPart; k++)
            bad += os[k].entries != perOut[k];
        // table 2's tablet was created at segment 2: its objects (segment 1) are dead
        bad += ps[0].flags != RAMCRC_SEG_OK || ps[0].dead != kObjects / 2 || ps[0].unplaced != 0 ||
               ps[0].placed != kPart + kObjects / 2;
        bad += round ? ps[1].flags != RAMCRC_SEG_SOURCE_BAD || ps[1].placed != 0
                     : ps[1].flags != RAMCRC_SEG_OK || ps[1].placed != kPart + kObjects / 2;
        placed += np;
    }
    printf("recovery partition: %llu placements over 2 rounds; %d mismatches\n",
           static_cast<unsigned long long>(placed), bad);
    return bad ? 1 : 0;
}
