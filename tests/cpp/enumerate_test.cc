// RAMCloud::ReplayTable::enumerate as a master answers ENUMERATE from the table
// it recovered into: recovery segments arrive in two batches (two segments,
// then one), each is verified and added as it arrives, and after each add the
// table is enumerated from cursor (0, 0) to its end in replies of at most 300
// bytes and 16 buckets a call, with full objects and with keys only, then once
// more in a single call under a stale frame.  Payload and summary of every
// call are compared with the host form (ramcrc_replay_table_enumerate_host)
// byte for byte; the entries are then read as TableEnumerator reads them: the
// builder fills the value of record k with k % 40 bytes of uint8_t(k), and
// every key "0" .. "49" of table 1 comes back at most once.  Built with hipcc
// for hipMalloc.
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <set>
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
        if ((k + s) % 7) {   // (a tombstone wins a tie: about two keys in five end as tombstones)
            // Object::Header {checksum, timestamp, version, tableId}, KeyCount,
            // CumulativeKeyLength, key, value
            std::vector<uint8_t> o(24 + 1 + 2 + key.size() + k % 40, uint8_t(k));
            memset(&o[0], 0, 24);
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
static const uint64_t kRoom = 16 * 1024;   // more than any payload here

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

// The entries of a payload as a client reads them: the keys into *keys (each
// at most once), the values checked against the builder's pattern.
static int readEntries(const std::vector<uint8_t>& got, const ramcrc_enumerate_summary& sm, bool keysOnly,
                       std::set<std::string>* keys)
{
    int bad = 0;
    uint64_t at = 0, objects = 0;
    while (at < sm.payload_bytes) {
        uint32_t length;
        memcpy(&length, &got[at], 4);
        at += 4;
        if (length < 28 || at + length > sm.payload_bytes)
            return bad + 1;
        const uint8_t* o = &got[at];
        uint64_t tableId;
        memcpy(&tableId, o + 16, 8);
        const uint32_t keyLen = o[25];
        bad += tableId != 1 || o[24] != 1 || o[26] != 0 || 27 + keyLen > length;
        const std::string key(reinterpret_cast<const char*>(o + 27), keyLen);
        bad += !keys->insert(key).second;   // a key twice
        const uint32_t vlen = length - 27 - keyLen;
        bad += keysOnly && vlen != 0;
        for (uint32_t b = 0; b < vlen; b++)
            bad += o[27 + keyLen + b] != o[27 + keyLen];
        bad += vlen != 0 && (o[27 + keyLen] % 40 != vlen || std::to_string(o[27 + keyLen] % kKeys) != key);
        at += length;
        objects++;
    }
    return bad + (at != sm.payload_bytes) + (objects != sm.objects);
}

static int run()
{
    Crc32CBatch batch(0);
    ReplayTable table(batch, 2 * kKeys, kBatches);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(2 * kKeys, kBatches, &hostTable))
        return 1;
    ramcrc_enumerate_summary* d_summary = dalloc<ramcrc_enumerate_summary>(1);
    uint8_t* d_payload = dalloc<uint8_t>(kRoom + 1);
    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    uint64_t calls = 0, allObjects = 0;
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
        // the enumerations the master serves while the next batch is on its
        // way: pass 0 and 1 walk the cursor, pass 2 is one call under a frame
        // of a table of 8 buckets that stands at its bucket 4
        for (int pass = 0; pass < 3; pass++) {
            const bool keysOnly = pass == 1;
            const ramcrc_enum_frame frame = {0, ~0ull, 8, 4, 0};
            std::set<std::string> keys;
            uint64_t bucket = 0, nextHash = 0, numBuckets = 1, objects = 0, tombstones = 0;
            while (bucket < numBuckets) {
                uint64_t maxBytes = pass == 2 ? kRoom : 300;
                ramcrc_enumerate_summary sm, wantSm;
                std::vector<uint8_t> got(kRoom + 1), want(kRoom + 1, 0xA5);
                for (;;) {
                    const uint64_t limit = pass == 2 ? 0 : (bucket + 16 < numBuckets ? bucket + 16 : 0);
                    HIP(hipMemset(d_payload, 0xA5, kRoom + 1));
                    table.enumerate(1, 0, ~0ull, bucket, nextHash, limit, pass == 2 ? &frame : NULL,
                                    pass == 2 ? 1 : 0, keysOnly, d_payload, kRoom, maxBytes, d_summary);
                    batch.sync();
                    HIP(hipMemcpy(&got[0], d_payload, kRoom + 1, hipMemcpyDeviceToHost));
                    HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
                    want.assign(kRoom + 1, 0xA5);
                    if (ramcrc_replay_table_enumerate_host(hostTable, 1, 0, ~0ull, bucket, nextHash, limit,
                                                           pass == 2 ? &frame : NULL, pass == 2 ? 1 : 0,
                                                           keysOnly ? RAMCRC_ENUM_KEYS_ONLY : 0u, &want[0], kRoom,
                                                           maxBytes, &wantSm))
                        return 1;
                    // (the bytes at and past payload_bytes keep their fill in both)
                    bad += memcmp(&got[0], &want[0], kRoom + 1) != 0;
                    bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
                    bad += sm.spoiled != 0 || sm.payload_bytes > maxBytes || sm.num_buckets != 256;
                    calls++;
                    if (!sm.stuck || maxBytes >= kRoom)
                        break;
                    maxBytes *= 2;   // the first object alone did not fit
                }
                numBuckets = sm.num_buckets;
                bad += readEntries(got, sm, keysOnly, &keys);
                bad += sm.next_bucket < bucket || (sm.next_bucket == bucket && sm.next_hash <= nextHash);
                objects += sm.objects;
                tombstones += sm.tombstones;
                bucket = sm.next_bucket;
                nextHash = sm.next_hash;
            }
            if (pass < 2) {
                // every key is there, as an object or as a tombstone
                bad += objects + tombstones != kKeys || objects == 0 || keys.size() != objects;
                allObjects = objects;
            } else {
                bad += objects >= allObjects || objects == 0;
            }
        }
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("enumerate: %llu calls, %llu objects in the table at the end; %d mismatches\n",
           static_cast<unsigned long long>(calls), static_cast<unsigned long long>(allObjects), bad);
    return bad ? 1 : 0;
}
