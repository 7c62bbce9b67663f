// RAMCloud::ReplayTable::multiWrite as a master serves a multi-write from the
// table it recovered into: one recovery segment is verified and added; then one
// request writes the keys "0" .. "59" of table 1 -- the 50 the segment holds,
// objects and tombstones, and 10 new ones --, every seventh under a reject rule
// that refuses existing objects, plus one repeated key and one unusable
// request.  Output, certificate, parts, references, old results and summary are
// compared with the host form (ramcrc_replay_table_write_host) byte for byte.
// The output is then walked with the call's certificate (deviceReplayVerify
// finds no bad object), added as the next batch, and a multiRead of every key
// returns the version the write reported and the value it wrote: 30 bytes of
// uint8_t(100 + q).  Built with hipcc for hipMalloc.
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
static const uint32_t kRecords = 150, kKeys = 50, kNew = 10;
static const uint32_t kReqs = kKeys + kNew + 2;
static const uint32_t kValue = 30;
static const uint64_t kEcap = 1024;

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

// SEGHEADER, then objects and tombstones of versions 1 .. 5
static ramcrc_seg_cert fill(uint8_t* seg)
{
    Builder b = {seg, 0, Crc32C()};
    std::vector<uint8_t> h(24, 0);
    put64(h, 8, 10);
    b.append(RAMCRC_LOG_ENTRY_TYPE_SEGHEADER, h);
    for (uint32_t k = 0; k < kRecords; k++) {
        const std::string key = std::to_string(k % kKeys);
        const uint64_t version = 1 + (k * 7 + k / kKeys) % 5;
        if (k % 3) {
            std::vector<uint8_t> o(24 + 1 + 2 + key.size() + k % 40, uint8_t(k));
            put64(o, 8, version);
            put64(o, 16, 1);
            o[24] = 1;
            o[25] = uint8_t(key.size());
            o[26] = 0;
            memcpy(&o[27], key.data(), key.size());
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o);
        } else {
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

// One batch on the device and, read back, on the host.
struct Arrived {
    std::vector<uint8_t> host;
    ramcrc_seg_cert cert;
    ramcrc_seg_status status;
    std::vector<ramcrc_seg_entry> table;
    std::vector<uint64_t> hostWork;
    uint8_t* d_base;
    ramcrc_seg_cert* d_cert;
    ramcrc_seg_status* d_status;
    ramcrc_seg_entry* d_entries;
    uint64_t *d_n, *d_work;
    uint32_t* d_crc;
    uint64_t n;
};

// Verify the segment at a.d_base with a.d_cert and add it to both tables.
// checked: the segment's objects carry their checksums.
static int arrive(Crc32CBatch& batch, ReplayTable& table, ramcrc_replay_table_host* hostTable, Arrived& a,
                  uint32_t number, bool checked)
{
    a.d_status = dalloc<ramcrc_seg_status>(1);
    a.d_entries = dalloc<ramcrc_seg_entry>(kEcap);
    a.d_n = dalloc<uint64_t>(1);
    a.d_work = dalloc<uint64_t>(kEcap);
    a.d_crc = dalloc<uint32_t>(kEcap);
    batch.deviceReplayVerify(a.d_base, kCap, kCap, 1, a.d_cert, a.d_status, a.d_entries, kEcap, a.d_n,
                             a.d_crc);
    int bad = table.add(a.d_base, kCap, 1, a.d_status, a.d_entries, kEcap, a.d_n, NULL, a.d_work) != number;
    batch.sync();
    HIP(hipMemcpy(&a.n, a.d_n, 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&a.status, a.d_status, sizeof a.status, hipMemcpyDeviceToHost));
    a.host.resize(kCap);
    a.table.resize(a.n);
    a.hostWork.resize(a.n);
    HIP(hipMemcpy(&a.host[0], a.d_base, kCap, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&a.table[0], a.d_entries, a.n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    uint32_t hostNumber = ~0u;
    if (ramcrc_replay_table_add_host(hostTable, &a.host[0], kCap, 1, &a.status, &a.table[0], a.n, NULL,
                                     &a.hostWork[0], &hostNumber) ||
        hostNumber != number)
        return 1;
    bad += !(a.status.flags & RAMCRC_SEG_OK) || (checked && a.status.bad_objects != 0);
    return bad;
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
    Crc32CBatch batch(0);
    ReplayTable table(batch, 4 * kKeys, 2);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(4 * kKeys, 2, &hostTable))
        return 1;
    int bad = 0;
    // the recovered segment
    Arrived first;
    first.host.assign(kCap, 0);
    first.cert = fill(&first.host[0]);
    first.d_base = dalloc<uint8_t>(kCap);
    first.d_cert = dalloc<ramcrc_seg_cert>(1);
    HIP(hipMemcpy(first.d_base, &first.host[0], kCap, hipMemcpyHostToDevice));
    HIP(hipMemcpy(first.d_cert, &first.cert, sizeof first.cert, hipMemcpyHostToDevice));
    bad += arrive(batch, table, hostTable, first, 0, false);   // (the builder writes no checksums)
    bad += first.n != kRecords + 1;

    // the multi-write: key q, then key 7 again, then a request past the buffer
    std::vector<uint8_t> data;
    std::vector<ramcrc_write_req> reqs(kReqs);
    std::vector<ramcrc_reject_rules> rules(kReqs);
    memset(&rules[0], 0, kReqs * sizeof(ramcrc_reject_rules));
    for (uint32_t q = 0; q < kReqs - 1; q++) {
        const uint32_t k = q < kKeys + kNew ? q : 7;
        const std::string key = std::to_string(k);
        reqs[q].table_id = 1;
        reqs[q].data_off = data.size();
        reqs[q].data_len = uint32_t(3 + key.size() + kValue);
        reqs[q].reserved = 0;
        data.push_back(1);
        data.push_back(uint8_t(key.size()));
        data.push_back(0);
        data.insert(data.end(), key.begin(), key.end());
        data.insert(data.end(), kValue, uint8_t(100 + q));
        if (q % 7 == 0)
            rules[q].exists = 1;
    }
    reqs[kReqs - 1].table_id = 1;
    reqs[kReqs - 1].data_off = data.size();
    reqs[kReqs - 1].data_len = 4;
    reqs[kReqs - 1].reserved = 0;
    const uint64_t segmentIds[2] = {10, 77};
    const uint64_t nextVersion = 1000;
    const uint32_t timestamp = 0x12345678;

    uint8_t* d_data = dalloc<uint8_t>(data.size());
    ramcrc_write_req* d_reqs = dalloc<ramcrc_write_req>(kReqs);
    ramcrc_reject_rules* d_rules = dalloc<ramcrc_reject_rules>(kReqs);
    uint64_t* d_segmentIds = dalloc<uint64_t>(2);
    uint8_t* d_parts = dalloc<uint8_t>(12 * kReqs);
    ramcrc_write_ref* d_refs = dalloc<ramcrc_write_ref>(kReqs);
    ramcrc_lookup_result* d_old = dalloc<ramcrc_lookup_result>(kReqs);
    ramcrc_write_summary* d_summary = dalloc<ramcrc_write_summary>(1);
    Arrived second;
    second.d_base = dalloc<uint8_t>(kCap);
    second.d_cert = dalloc<ramcrc_seg_cert>(1);
    HIP(hipMemcpy(d_data, &data[0], data.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_reqs, &reqs[0], kReqs * sizeof(ramcrc_write_req), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rules, &rules[0], kReqs * sizeof(ramcrc_reject_rules), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_segmentIds, segmentIds, sizeof segmentIds, hipMemcpyHostToDevice));
    HIP(hipMemset(second.d_base, 0, kCap));
    table.multiWrite(d_data, data.size(), d_reqs, kReqs, NULL, d_rules, nextVersion, timestamp, d_segmentIds,
                     second.d_base, kCap, second.d_cert, d_parts, d_refs, d_old, d_summary);
    batch.sync();

    std::vector<uint8_t> out(kCap), wantOut(kCap, 0), parts(12 * kReqs), wantParts(12 * kReqs);
    std::vector<ramcrc_write_ref> refs(kReqs), wantRefs(kReqs);
    std::vector<ramcrc_lookup_result> old(kReqs), wantOld(kReqs);
    ramcrc_write_summary sm, wantSm;
    ramcrc_seg_cert cert, wantCert;
    HIP(hipMemcpy(&out[0], second.d_base, kCap, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&parts[0], d_parts, 12 * kReqs, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&refs[0], d_refs, kReqs * sizeof(ramcrc_write_ref), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&old[0], d_old, kReqs * sizeof(ramcrc_lookup_result), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&cert, second.d_cert, sizeof cert, hipMemcpyDeviceToHost));
    if (ramcrc_replay_table_write_host(hostTable, &data[0], data.size(), &reqs[0], kReqs, NULL, &rules[0],
                                       nextVersion, timestamp, segmentIds, &wantOut[0], kCap, &wantCert,
                                       &wantParts[0], &wantRefs[0], &wantOld[0], &wantSm))
        return 1;
    // (the bytes at and past the head keep their zeros in both)
    bad += memcmp(&out[0], &wantOut[0], kCap) != 0;
    bad += memcmp(&parts[0], &wantParts[0], 12 * kReqs) != 0;
    bad += memcmp(&refs[0], &wantRefs[0], kReqs * sizeof(ramcrc_write_ref)) != 0;
    bad += memcmp(&old[0], &wantOld[0], kReqs * sizeof(ramcrc_lookup_result)) != 0;
    bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
    bad += memcmp(&cert, &wantCert, sizeof cert) != 0;
    bad += sm.spoiled != 0 || sm.bad != 1 || sm.retry_duplicate != 1 || sm.retry_full != 0;
    bad += sm.ok + sm.object_exists != kKeys + kNew || sm.object_exists == 0 || sm.tombstones == 0;
    bad += sm.allocated < kNew || sm.next_version != nextVersion + sm.allocated;
    bad += cert.segment_length != sm.out_bytes;

    // walk the output with its certificate, add it, read every key back
    bad += arrive(batch, table, hostTable, second, 1, true);
    bad += second.n != sm.ok + sm.tombstones;
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> queries(kKeys + kNew);
    for (uint32_t q = 0; q < kKeys + kNew; q++) {
        const std::string key = std::to_string(q);
        queries[q].table_id = 1;
        queries[q].key_off = keys.size();
        queries[q].key_len = uint32_t(key.size());
        queries[q].reserved = 0;
        keys.insert(keys.end(), key.begin(), key.end());
    }
    const uint64_t room = uint64_t(kKeys + kNew) * (16 + 64);
    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_queries = dalloc<ramcrc_lookup_key>(kKeys + kNew);
    uint8_t* d_reply = dalloc<uint8_t>(room);
    ramcrc_read_summary* d_readSummary = dalloc<ramcrc_read_summary>(1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_queries, &queries[0], queries.size() * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    table.multiRead(d_keys, keys.size(), d_queries, kKeys + kNew, NULL, NULL, true, d_reply, room, NULL, NULL,
                    d_readSummary);
    batch.sync();
    std::vector<uint8_t> reply(room);
    ramcrc_read_summary rs;
    HIP(hipMemcpy(&reply[0], d_reply, room, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&rs, d_readSummary, sizeof rs, hipMemcpyDeviceToHost));
    bad += rs.returned != kKeys + kNew;
    uint64_t at = 0, readBack = 0;
    for (uint32_t q = 0; q < rs.returned; q++) {
        uint32_t status, length, wstatus;
        uint64_t version, wversion;
        memcpy(&status, &reply[at], 4);
        memcpy(&version, &reply[at + 4], 8);
        memcpy(&length, &reply[at + 12], 4);
        memcpy(&wstatus, &parts[12 * q], 4);
        memcpy(&wversion, &parts[12 * q + 4], 8);
        at += 16;
        if (wstatus == RAMCRC_STATUS_OK) {
            // the written object answers: its version, its value
            bad += status != RAMCRC_STATUS_OK || version != wversion || length != kValue;
            for (uint32_t b = 0; b < length && b < kValue; b++)
                bad += reply[at + b] != uint8_t(100 + q);
            readBack++;
        } else {
            // refused because the key holds an object: that object still answers
            bad += wstatus != RAMCRC_STATUS_OBJECT_EXISTS || q % 7 != 0 || status != RAMCRC_STATUS_OK ||
                   version != wversion;
        }
        if (status == RAMCRC_STATUS_OK)
            at += length;
    }
    bad += readBack != sm.ok;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("multiWrite: %llu objects and %llu tombstones written, %llu refused, %llu read back; %d mismatches\n",
           static_cast<unsigned long long>(sm.ok), static_cast<unsigned long long>(sm.tombstones),
           static_cast<unsigned long long>(sm.object_exists), static_cast<unsigned long long>(readBack), bad);
    return bad ? 1 : 0;
}
