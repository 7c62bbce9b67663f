// RAMCloud::ReplayTable::multiRead as a master answers a multi-read from the
// table it recovered into: recovery segments arrive in two batches (two
// segments, then one), each is verified and added as it arrives, and after each
// add one request is answered twice, once with keys and values under a limit
// that cuts the reply short and once with values only under no limit: the keys
// "0" .. "49" of table 1 that the segments hold, every fifth under a reject
// rule, the same keys under a table id no record has, and one unusable query.
// Reply, part offsets, results and summary are compared with the host form
// (ramcrc_replay_table_read_host) byte for byte; the parts are then walked as
// a client walks them: the builder fills the value of record k with value_len
// = k % 40 bytes of uint8_t(k).  Built with hipcc for hipMalloc.
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
    // the multi-read: key k, then key k under table 2, then a query past the buffer
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> queries(kQueries);
    std::vector<ramcrc_reject_rules> rules(kQueries);
    memset(&rules[0], 0, kQueries * sizeof(ramcrc_reject_rules));
    for (uint32_t q = 0; q < 2 * kKeys; q++) {
        const std::string key = std::to_string(q % kKeys);
        queries[q].table_id = q < kKeys ? 1 : 2;
        queries[q].key_off = keys.size();
        queries[q].key_len = uint32_t(key.size());
        queries[q].reserved = 0;
        keys.insert(keys.end(), key.begin(), key.end());
        if (q % 5 == 0) {   // only versions above 2 may be read
            rules[q].given_version = 2;
            rules[q].version_le_given = 1;
        }
    }
    queries[2 * kKeys].table_id = 1;
    queries[2 * kKeys].key_off = keys.size();
    queries[2 * kKeys].key_len = 1;
    queries[2 * kKeys].reserved = 0;
    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_queries = dalloc<ramcrc_lookup_key>(kQueries);
    ramcrc_reject_rules* d_rules = dalloc<ramcrc_reject_rules>(kQueries);
    ramcrc_lookup_result* d_results = dalloc<ramcrc_lookup_result>(kQueries);
    uint64_t* d_partOff = dalloc<uint64_t>(kQueries);
    ramcrc_read_summary* d_summary = dalloc<ramcrc_read_summary>(1);
    uint8_t* d_reply = dalloc<uint8_t>(kRoom + 1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_queries, &queries[0], kQueries * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rules, &rules[0], kQueries * sizeof(ramcrc_reject_rules), hipMemcpyHostToDevice));
    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    uint64_t okParts = 0, shortCount = 0;
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
        // the reads the master serves while the next batch is on its way:
        // keys and values under a limit of 1,000 bytes, then values under none
        for (int pass = 0; pass < 2; pass++) {
            const bool valueOnly = pass == 1;
            const uint64_t cap = pass == 0 ? 1000 : kRoom;
            HIP(hipMemset(d_reply, 0xA5, kRoom + 1));
            table.multiRead(d_keys, keys.size(), d_queries, kQueries, NULL, d_rules, valueOnly, d_reply,
                            cap, d_partOff, d_results, d_summary);
            batch.sync();
            std::vector<uint8_t> got(kRoom + 1), want(kRoom + 1, 0xA5);
            std::vector<uint64_t> off(kQueries), wantOff(kQueries);
            std::vector<ramcrc_lookup_result> res(kQueries), wantRes(kQueries);
            ramcrc_read_summary sm, wantSm;
            HIP(hipMemcpy(&got[0], d_reply, kRoom + 1, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&off[0], d_partOff, kQueries * 8, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&res[0], d_results, kQueries * sizeof(ramcrc_lookup_result), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
            if (ramcrc_replay_table_read_host(hostTable, &keys[0], keys.size(), &queries[0], kQueries, NULL,
                                              &rules[0], valueOnly ? RAMCRC_READ_VALUE_ONLY : 0u, &want[0],
                                              cap, &wantOff[0], &wantRes[0], &wantSm))
                return 1;
            // (the bytes at and past reply_bytes keep their fill in both)
            bad += memcmp(&got[0], &want[0], kRoom + 1) != 0;
            bad += memcmp(&off[0], &wantOff[0], kQueries * 8) != 0;
            bad += memcmp(&res[0], &wantRes[0], kQueries * sizeof(ramcrc_lookup_result)) != 0;
            bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
            bad += sm.spoiled != 0 || sm.reply_bytes > cap;
            if (pass == 0) {
                bad += sm.returned == 0 || sm.returned >= kQueries;
                shortCount = sm.returned;
            } else {
                bad += sm.returned != kQueries || sm.bad != 1 || sm.doesnt_exist < kKeys;
                okParts = sm.ok;
            }
            // the parts, as a client walks them
            uint64_t at = 0, ok = 0;
            for (uint64_t q = 0; q < sm.returned; q++) {
                uint32_t status, length;
                uint64_t version;
                bad += off[q] != at;
                memcpy(&status, &got[at], 4);
                memcpy(&version, &got[at + 4], 8);
                memcpy(&length, &got[at + 12], 4);
                at += 16;
                if (status != RAMCRC_STATUS_OK) {
                    bad += length != 0;
                    bad += q >= kKeys && status != (q < 2 * kKeys ? RAMCRC_STATUS_OBJECT_DOESNT_EXIST
                                                                 : RAMCRC_STATUS_REQUEST_FORMAT_ERROR);
                    bad += status == RAMCRC_STATUS_WRONG_VERSION && (q % 5 != 0 || version == 0 || version > 2);
                    continue;
                }
                ok++;
                // (version 0 is VERSION_NONEXISTENT: rejectOperation lets it pass)
                bad += q >= kKeys || version > 4 || (q % 5 == 0 && version != 0 && version <= 2);
                const std::string key = std::to_string(q);
                const uint8_t* v = &got[at];
                uint32_t vlen = length;
                if (!valueOnly) {   // key count, one cumulative length, the key
                    bad += length < 3 + key.size() || v[0] != 1 || v[1] != key.size() || v[2] != 0 ||
                           memcmp(v + 3, key.data(), key.size()) != 0;
                    v += 3 + key.size();
                    vlen -= uint32_t(3 + key.size());
                }
                for (uint32_t b = 0; b < vlen; b++)
                    bad += v[b] != v[0];
                bad += vlen != 0 && (v[0] % 40 != vlen || v[0] % kKeys != q);
                at += length;
            }
            bad += at != sm.reply_bytes || ok != sm.ok;
            for (uint64_t q = sm.returned; q < kQueries; q++)
                bad += off[q] != RAMCRC_READ_NONE;
        }
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("multiRead: %llu of %u parts under the limit, %llu objects read without one; %d mismatches\n",
           static_cast<unsigned long long>(shortCount), kQueries,
           static_cast<unsigned long long>(okParts), bad);
    return bad ? 1 : 0;
}
