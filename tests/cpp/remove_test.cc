// RAMCloud::ReplayTable::multiRemove as a master serves a multi-remove from the
// table it recovered into: one recovery segment is verified and added; then one
// request removes the keys "0" .. "59" of table 1 -- the 50 the segment holds,
// objects and tombstones, and 10 it does not --, every seventh under a reject
// rule that refuses existing objects, plus one repeated key and one unusable
// request.  Output, certificate, parts, references, old results and summary are
// compared with the host form (ramcrc_replay_table_remove_host) byte for byte.
// The output is then walked with the call's certificate (deviceReplayVerify
// finds no bad tombstone), added as the next batch, and a multiRead of every
// key answers STATUS_OBJECT_DOESNT_EXIST for the removed ones and the object
// for the refused ones.  With --cpu the program only validates arguments, on
// the host form and on the device form's checks that come before any launch.
// Built with hipcc for hipMalloc.
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
static int cpu();

int main(int argc, char** argv)
{
    try {
        return argc > 1 && !strcmp(argv[1], "--cpu") ? cpu() : run();
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
}

// The keys "0" .. n - 1 of table 1, packed.
static void pack(uint32_t n, std::vector<uint8_t>& keys, std::vector<ramcrc_lookup_key>& queries)
{
    queries.resize(n);
    for (uint32_t q = 0; q < n; q++) {
        const std::string key = std::to_string(q);
        queries[q].table_id = 1;
        queries[q].key_off = keys.size();
        queries[q].key_len = uint32_t(key.size());
        queries[q].reserved = 0;
        keys.insert(keys.end(), key.begin(), key.end());
    }
}

// No GPU: what both forms refuse, and the host form against an empty table.
static int cpu()
{
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(16, 2, &hostTable))
        return 1;
    int bad = 0;
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> reqs;
    pack(3, keys, reqs);
    ramcrc_reject_rules rules[3];
    memset(rules, 0, sizeof rules);
    rules[1].doesnt_exist = 1;
    rules[2].reserved = 1;
    uint8_t out[64], parts[36];
    uint32_t refs[3];
    ramcrc_lookup_result old[3];
    ramcrc_seg_cert cert;
    ramcrc_remove_summary sm;
    // refused
    bad += ramcrc_replay_table_remove_host(NULL, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           out, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 0, 0, NULL,
                                           out, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           out, 64, NULL, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           out, 64, &cert, parts, refs, old, NULL) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), NULL, 3, NULL, rules, 1, 0, NULL,
                                           out, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           out, 64, &cert, NULL, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, NULL, keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           out, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL,
                                           NULL, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 0xFFFFFFFFull, NULL, rules, 1,
                                           0, NULL, out, 64, &cert, parts, refs, old, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_remove_device(NULL, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 1, 0, NULL, out,
                                             64, &cert, parts, refs, old, &sm, NULL) != RAMCRC_EINVAL;
    // an empty table: nothing to remove, the rules as rejectOperation applies them, the empty certificate
    memset(out, 0xA5, sizeof out);
    if (ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], 3, NULL, rules, 9, 0, NULL, out,
                                        64, &cert, parts, refs, old, &sm))
        return 1;
    const uint32_t wantStatus[3] = {RAMCRC_STATUS_OK, RAMCRC_STATUS_OBJECT_DOESNT_EXIST,
                                    RAMCRC_STATUS_REQUEST_FORMAT_ERROR};
    for (uint32_t q = 0; q < 3; q++) {
        uint32_t status;
        uint64_t version;
        memcpy(&status, &parts[12 * q], 4);
        memcpy(&version, &parts[12 * q + 4], 8);
        bad += status != wantStatus[q] || version != 0 || refs[q] != 0xFFFFFFFFu;
    }
    Crc32C empty;
    const uint32_t zero = 0;
    empty.update(&zero, 4);
    bad += sm.ok_absent != 1 || sm.doesnt_exist != 1 || sm.bad != 1 || sm.removed != 0 || sm.next_version != 9;
    bad += sm.out_bytes != 0 || cert.segment_length != 0 || cert.checksum != empty.getResult() || out[0] != 0xA5;
    bad += old[0].kind != RAMCRC_LOOKUP_ABSENT || old[2].kind != RAMCRC_LOOKUP_BAD_KEY;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("multiRemove arguments: %d mismatches\n", bad);
    return bad ? 1 : 0;
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

    // the multi-remove: key q, then key 7 again, then a request past the buffer
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> reqs;
    pack(kKeys + kNew, keys, reqs);
    reqs.resize(kReqs);
    reqs[kReqs - 2] = reqs[7];
    reqs[kReqs - 1] = reqs[0];
    reqs[kReqs - 1].key_off = keys.size();
    std::vector<ramcrc_reject_rules> rules(kReqs);
    memset(&rules[0], 0, kReqs * sizeof(ramcrc_reject_rules));
    for (uint32_t q = 0; q < kReqs; q += 7)
        rules[q].exists = 1;
    const uint64_t segmentIds[2] = {10, 77};
    const uint64_t nextVersion = 3;
    const uint32_t timestamp = 0x12345678;

    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_reqs = dalloc<ramcrc_lookup_key>(kReqs);
    ramcrc_reject_rules* d_rules = dalloc<ramcrc_reject_rules>(kReqs);
    uint64_t* d_segmentIds = dalloc<uint64_t>(2);
    uint8_t* d_parts = dalloc<uint8_t>(12 * kReqs);
    uint32_t* d_refs = dalloc<uint32_t>(kReqs);
    ramcrc_lookup_result* d_old = dalloc<ramcrc_lookup_result>(kReqs);
    ramcrc_remove_summary* d_summary = dalloc<ramcrc_remove_summary>(1);
    Arrived second;
    second.d_base = dalloc<uint8_t>(kCap);
    second.d_cert = dalloc<ramcrc_seg_cert>(1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_reqs, &reqs[0], kReqs * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rules, &rules[0], kReqs * sizeof(ramcrc_reject_rules), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_segmentIds, segmentIds, sizeof segmentIds, hipMemcpyHostToDevice));
    HIP(hipMemset(second.d_base, 0, kCap));
    table.multiRemove(d_keys, keys.size(), d_reqs, kReqs, NULL, d_rules, nextVersion, timestamp, d_segmentIds,
                      second.d_base, kCap, second.d_cert, d_parts, d_refs, d_old, d_summary);
    batch.sync();

    std::vector<uint8_t> out(kCap), wantOut(kCap, 0), parts(12 * kReqs), wantParts(12 * kReqs);
    std::vector<uint32_t> refs(kReqs), wantRefs(kReqs);
    std::vector<ramcrc_lookup_result> old(kReqs), wantOld(kReqs);
    ramcrc_remove_summary sm, wantSm;
    ramcrc_seg_cert cert, wantCert;
    HIP(hipMemcpy(&out[0], second.d_base, kCap, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&parts[0], d_parts, 12 * kReqs, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&refs[0], d_refs, kReqs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&old[0], d_old, kReqs * sizeof(ramcrc_lookup_result), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&cert, second.d_cert, sizeof cert, hipMemcpyDeviceToHost));
    if (ramcrc_replay_table_remove_host(hostTable, &keys[0], keys.size(), &reqs[0], kReqs, NULL, &rules[0],
                                        nextVersion, timestamp, segmentIds, &wantOut[0], kCap, &wantCert,
                                        &wantParts[0], &wantRefs[0], &wantOld[0], &wantSm))
        return 1;
    // (the bytes at and past the head keep their zeros in both)
    bad += memcmp(&out[0], &wantOut[0], kCap) != 0;
    bad += memcmp(&parts[0], &wantParts[0], 12 * kReqs) != 0;
    bad += memcmp(&refs[0], &wantRefs[0], kReqs * sizeof(uint32_t)) != 0;
    bad += memcmp(&old[0], &wantOld[0], kReqs * sizeof(ramcrc_lookup_result)) != 0;
    bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
    bad += memcmp(&cert, &wantCert, sizeof cert) != 0;
    bad += sm.spoiled != 0 || sm.bad != 1 || sm.retry_duplicate != 1 || sm.retry_full != 0;
    bad += sm.removed + sm.object_exists + sm.ok_absent != kKeys + kNew || sm.object_exists == 0;
    // (the versions are 1 .. 5)
    bad += sm.removed == 0 || sm.ok_absent < kNew || sm.next_version < nextVersion || sm.next_version > 6;
    bad += cert.segment_length != sm.out_bytes;

    // walk the output with its certificate, add it, read every key
    bad += arrive(batch, table, hostTable, second, 1, true);
    bad += second.n != sm.removed;
    const uint64_t room = uint64_t(kKeys + kNew) * (16 + 64);
    uint8_t* d_reply = dalloc<uint8_t>(room);
    ramcrc_read_summary* d_readSummary = dalloc<ramcrc_read_summary>(1);
    table.multiRead(d_keys, keys.size(), d_reqs, kKeys + kNew, NULL, NULL, true, d_reply, room, NULL, NULL,
                    d_readSummary);
    batch.sync();
    std::vector<uint8_t> reply(room);
    ramcrc_read_summary rs;
    HIP(hipMemcpy(&reply[0], d_reply, room, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&rs, d_readSummary, sizeof rs, hipMemcpyDeviceToHost));
    bad += rs.returned != kKeys + kNew;
    uint64_t at = 0, gone = 0;
    for (uint32_t q = 0; q < rs.returned; q++) {
        uint32_t status, length, rstatus;
        uint64_t version, rversion;
        memcpy(&status, &reply[at], 4);
        memcpy(&version, &reply[at + 4], 8);
        memcpy(&length, &reply[at + 12], 4);
        memcpy(&rstatus, &parts[12 * q], 4);
        memcpy(&rversion, &parts[12 * q + 4], 8);
        at += 16;
        if (rstatus == RAMCRC_STATUS_OK) {
            // removed, or never there: no object answers
            bad += status != RAMCRC_STATUS_OBJECT_DOESNT_EXIST;
            gone += refs[q] != 0xFFFFFFFFu;
        } else {
            // refused because the key holds an object: that object still answers
            bad += rstatus != RAMCRC_STATUS_OBJECT_EXISTS || q % 7 != 0 || status != RAMCRC_STATUS_OK ||
                   version != rversion;
        }
        if (status == RAMCRC_STATUS_OK)
            at += length;
    }
    bad += gone != sm.removed;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("multiRemove: %llu tombstones written, %llu refused, %llu keys without an object; %d mismatches\n",
           static_cast<unsigned long long>(sm.removed), static_cast<unsigned long long>(sm.object_exists),
           static_cast<unsigned long long>(sm.ok_absent), bad);
    return bad ? 1 : 0;
}
