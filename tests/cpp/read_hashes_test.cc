// RAMCloud::ReplayTable::readHashes as a master answers READ_HASHES from the
// table it recovered into: recovery segments arrive in two batches (two
// segments, then one), each is verified and added as it arrives, and after each
// add one indexed read is answered twice, once under a max_length that cuts
// the reply short and once under none: the Key::getHash of the keys "0" ..
// "49" of table 1 that the segments hold, every fifth one twice, and between
// them hashes no key has.  Reply, parts and summary are compared with the host
// form (ramcrc_replay_table_read_hashes_host) byte for byte; the object parts
// are then walked as IndexLookup walks them: the builder fills the value of
// record k with k % 40 bytes of uint8_t(k).  Built with hipcc for hipMalloc.
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
        if ((k + s) % 7) {   // (a tombstone wins a tie: about two keys in five end as tombstones)
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

// Key::getHash (MurmurHash3_x64_128's low word, seeded with the table id) of a
// key of fewer than 16 bytes: the tail and the finish only.
static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

static uint64_t fmix(uint64_t k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

static uint64_t keyHash(uint32_t tableId, const std::string& key)
{
    uint64_t h1 = tableId, h2 = tableId, k1 = 0, k2 = 0;
    for (size_t b = 0; b < key.size() && b < 8; b++)
        k1 |= uint64_t(uint8_t(key[b])) << (8 * b);
    for (size_t b = 8; b < key.size(); b++)
        k2 |= uint64_t(uint8_t(key[b])) << (8 * (b - 8));
    if (key.size() > 8) {
        k2 *= 0x4cf5ad432745937full;
        k2 = rotl(k2, 33);
        k2 *= 0x87c37b91114253d5ull;
        h2 ^= k2;
    }
    if (!key.empty()) {
        k1 *= 0x87c37b91114253d5ull;
        k1 = rotl(k1, 31);
        k1 *= 0x4cf5ad432745937full;
        h1 ^= k1;
    }
    h1 ^= key.size();
    h2 ^= key.size();
    h1 += h2;
    h2 += h1;
    h1 = fmix(h1);
    h2 = fmix(h2);
    return h1 + h2;
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
static const uint64_t kRoom = 16 * 1024;   // more than any reply here

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
    // the request: per key its hash (every fifth one twice) and a hash no key has
    std::vector<uint64_t> hashes;
    std::vector<int> keyOf;   // -1: nobody's
    for (uint32_t q = 0; q < kKeys; q++) {
        for (uint32_t copy = 0; copy < (q % 5 == 0 ? 2u : 1u); copy++) {
            hashes.push_back(keyHash(1, std::to_string(q)));
            keyOf.push_back(int(q));
        }
        hashes.push_back(keyHash(2, std::to_string(q)));
        keyOf.push_back(-1);
    }
    const uint64_t nHashes = hashes.size();
    uint64_t* d_hashes = dalloc<uint64_t>(nHashes);
    ramcrc_hash_part* d_parts = dalloc<ramcrc_hash_part>(nHashes);
    ramcrc_read_hashes_summary* d_summary = dalloc<ramcrc_read_hashes_summary>(1);
    uint8_t* d_reply = dalloc<uint8_t>(kRoom + 1);
    HIP(hipMemcpy(d_hashes, &hashes[0], nHashes * 8, hipMemcpyHostToDevice));
    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    uint64_t allObjects = 0, shortHashes = 0;
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
        // the indexed reads the master serves while the next batch is on its
        // way: under a max_length of 600 bytes, then under none
        for (int pass = 0; pass < 2; pass++) {
            const uint64_t maxLength = pass == 0 ? 600 : kRoom;
            HIP(hipMemset(d_reply, 0xA5, kRoom + 1));
            table.readHashes(1, d_hashes, nHashes, d_reply, kRoom, maxLength, d_parts, d_summary);
            batch.sync();
            std::vector<uint8_t> got(kRoom + 1), want(kRoom + 1, 0xA5);
            std::vector<ramcrc_hash_part> parts(nHashes), wantParts(nHashes);
            ramcrc_read_hashes_summary sm, wantSm;
            HIP(hipMemcpy(&got[0], d_reply, kRoom + 1, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&parts[0], d_parts, nHashes * sizeof(ramcrc_hash_part), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
            if (ramcrc_replay_table_read_hashes_host(hostTable, 1, &hashes[0], nHashes, 0u, &want[0], kRoom,
                                                     maxLength, &wantParts[0], &wantSm))
                return 1;
            // (the bytes at and past reply_bytes keep their fill in both)
            bad += memcmp(&got[0], &want[0], kRoom + 1) != 0;
            bad += memcmp(&parts[0], &wantParts[0], nHashes * sizeof(ramcrc_hash_part)) != 0;
            bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
            bad += sm.spoiled != 0 || sm.reply_bytes > kRoom;
            if (pass == 0) {
                // the first hash left out begins past max_length, and it begins where the reply ends
                bad += sm.hashes == 0 || sm.hashes >= nHashes || sm.reply_bytes <= maxLength;
                shortHashes = sm.hashes;
            } else {
                bad += sm.hashes != nHashes || sm.objects_counted != sm.objects || sm.empty < kKeys;
                // every key is there, as an object or as a tombstone
                bad += sm.objects + sm.tombstones != kKeys + kKeys / 5 || sm.objects == 0;
                allObjects = sm.objects;
            }
            // the object parts, as a client walks them
            uint64_t at = 0, objects = 0;
            for (uint64_t q = 0; q < sm.hashes; q++) {
                bad += parts[q].off != at || parts[q].objects > 1 || parts[q].reserved != 0;
                bad += keyOf[q] < 0 && parts[q].objects != 0;
                for (uint32_t k = 0; k < parts[q].objects; k++) {
                    uint64_t version;
                    uint32_t length;
                    memcpy(&version, &got[at], 8);
                    memcpy(&length, &got[at + 8], 4);
                    at += 12;
                    objects++;
                    const std::string key = std::to_string(keyOf[q]);
                    const uint8_t* v = &got[at];
                    // key count, one cumulative length, the key
                    bad += version > 4 || length < 3 + key.size() || v[0] != 1 || v[1] != key.size() ||
                           v[2] != 0 || memcmp(v + 3, key.data(), key.size()) != 0;
                    v += 3 + key.size();
                    const uint32_t vlen = length - uint32_t(3 + key.size());
                    for (uint32_t b = 0; b < vlen; b++)
                        bad += v[b] != v[0];
                    bad += vlen != 0 && (v[0] % 40 != vlen || int(v[0] % kKeys) != keyOf[q]);
                    at += length;
                }
            }
            bad += at != sm.reply_bytes || objects != sm.objects;
            for (uint64_t q = sm.hashes; q < nHashes; q++)
                bad += parts[q].off != RAMCRC_READ_NONE || parts[q].objects != 0;
        }
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("readHashes: %llu of %llu hashes under the limit, %llu objects read without one; %d mismatches\n",
           static_cast<unsigned long long>(shortHashes), static_cast<unsigned long long>(nHashes),
           static_cast<unsigned long long>(allObjects), bad);
    return bad ? 1 : 0;
}
