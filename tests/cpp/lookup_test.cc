// RAMCloud::ReplayTable::lookup as a master serves a multi-read from the table
// it recovered into: recovery segments arrive in two batches (two segments,
// then one), each is verified and added as it arrives, and after each add a
// batch of keys is looked up: the keys "0" .. "49" of table 1 that the segments
// hold, the same keys under a table id no record has, and one unusable query.
// The results and counts are compared with the host form
// (ramcrc_replay_table_lookup_host) byte for byte, and every object's value is
// read at {batch, segment, value_off, value_len}: the builder fills the value
// of record k with value_len = k % 40 bytes of uint8_t(k).  Built with hipcc
// for hipMalloc.
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

static const uint64_t kEcap = 512;
static const uint32_t kQueries = 2 * kKeys + 1;

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
    ReplayTable table(batch, 2 * kKeys, kBatches);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(2 * kKeys, kBatches, &hostTable))
        return 1;
    // the multi-read: key k, then key k under table 2, then a query past the buffer
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> queries(kQueries);
    for (uint32_t q = 0; q < 2 * kKeys; q++) {
        const std::string key = std::to_string(q % kKeys);
        queries[q].table_id = q < kKeys ? 1 : 2;
        queries[q].key_off = keys.size();
        queries[q].key_len = uint32_t(key.size());
        queries[q].reserved = 0;
        keys.insert(keys.end(), key.begin(), key.end());
    }
    queries[2 * kKeys].table_id = 1;
    queries[2 * kKeys].key_off = keys.size();
    queries[2 * kKeys].key_len = 1;
    queries[2 * kKeys].reserved = 0;
    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_queries = dalloc<ramcrc_lookup_key>(kQueries);
    ramcrc_lookup_result* d_results = dalloc<ramcrc_lookup_result>(kQueries + 1);
    ramcrc_lookup_counts* d_counts = dalloc<ramcrc_lookup_counts>(1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_queries, &queries[0], kQueries * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    uint64_t objects = 0, tombstones = 0;
    for (uint32_t j = 0; j < kBatches; j++) {
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
        a.d_work = dalloc<uint64_t>(kEcap);
        a.d_crc = dalloc<uint32_t>(kEcap);
        HIP(hipMemcpy(a.d_base, &a.host[0], a.host.size(), hipMemcpyHostToDevice));
        HIP(hipMemcpy(a.d_certs, &a.certs[0], a.nseg * sizeof(ramcrc_seg_cert), hipMemcpyHostToDevice));
        batch.deviceReplayVerify(a.d_base, kCap, kCap, a.nseg, a.d_certs, a.d_status, a.d_entries,
                                 kEcap, a.d_n, a.d_crc);
        bad += table.add(a.d_base, kCap, a.nseg, a.d_status, a.d_entries, kEcap, a.d_n, NULL,
                         a.d_work) != j;
        // the reads the master serves while the next batch is on its way
        HIP(hipMemset(d_results, 0xA5, (kQueries + 1) * sizeof(ramcrc_lookup_result)));
        table.lookup(d_keys, keys.size(), d_queries, kQueries, NULL, d_results, d_counts);
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
        std::vector<ramcrc_lookup_result> got(kQueries + 1), want(kQueries);
        ramcrc_lookup_counts counts, wantCounts;
        HIP(hipMemcpy(&got[0], d_results, (kQueries + 1) * sizeof(ramcrc_lookup_result),
                      hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
        if (ramcrc_replay_table_lookup_host(hostTable, &keys[0], keys.size(), &queries[0], kQueries,
                                            NULL, &want[0], &wantCounts))
            return 1;
        bad += memcmp(&got[0], &want[0], kQueries * sizeof(ramcrc_lookup_result)) != 0;
        bad += memcmp(&counts, &wantCounts, sizeof counts) != 0;
        bad += got[kQueries].kind != 0xA5A5A5A5u;   // the slot past the results keeps its fill
        bad += counts.objects + counts.tombstones != kKeys || counts.absent != kKeys ||
               counts.bad != 1 || counts.spoiled != 0;
        for (uint32_t q = 0; q < kQueries; q++) {
            const ramcrc_lookup_result& r = got[q];
            if (q >= kKeys) {
                bad += r.kind != (q < 2 * kKeys ? RAMCRC_LOOKUP_ABSENT : RAMCRC_LOOKUP_BAD_KEY) ||
                       r.ref.batch != 0xFFFFFFFFu;
                continue;
            }
            if (r.ref.batch > j) {
                bad++;
                continue;
            }
            if (r.kind != RAMCRC_LOOKUP_OBJECT) {
                bad += r.kind != RAMCRC_LOOKUP_TOMBSTONE;
                continue;
            }
            // the value, where the answer says it lies
            const Arrived& w = arrived[r.ref.batch];
            const uint8_t* v = &w.host[uint64_t(r.segment) * kCap + r.value_off];
            for (uint32_t b = 0; b < r.value_len; b++)
                bad += v[b] != v[0];
            bad += r.value_len != 0 && (v[0] % 40 != r.value_len || v[0] % kKeys != q);
            bad += r.version > 4;
        }
        objects = counts.objects;
        tombstones = counts.tombstones;
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("lookup: %llu objects and %llu tombstones for %u keys; %d mismatches\n",
           static_cast<unsigned long long>(objects), static_cast<unsigned long long>(tombstones),
           kKeys, bad);
    return bad ? 1 : 0;
}
