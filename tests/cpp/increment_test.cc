// RAMCloud::ReplayTable::multiIncrement as a master serves a multi-increment
// from the table it recovered into.
//
// With --cpu the program needs no GPU.  It takes the host form
// (ramcrc_replay_table_increment_host) through what the reference's own tests
// assert (tests/golden/multi_increment_ref.json has the same scenarios as data:
// increment_basic, increment_create, increment_rejectRules,
// increment_invalidObject, multiIncrement_basics, multiIncrement_rejectRules)
// and through the closed loop -- increment, walk the output, add it, read the
// new 8 bytes, increment again --, and checks what both forms refuse before
// any launch.
//
// Without it, one recovery segment is verified and added on the device; one
// request increments the keys "0" .. "59" of table 1 -- the 50 the segment
// holds (8-byte values, other lengths, tombstones) and 10 it does not --, every
// seventh under a reject rule that refuses existing objects, plus one repeated
// key and one unusable request.  Output, certificate, parts, references, old
// results and summary are compared with the host form byte for byte.  The
// output is then walked with the call's certificate (deviceReplayVerify finds
// no bad checksum), added as the next batch, and a multiRead of every key
// returns the new 8 bytes of every incremented one.  Built with hipcc for
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
    void header(uint64_t id)
    {
        std::vector<uint8_t> h(24, 0);
        memcpy(&h[8], &id, 8);
        append(RAMCRC_LOG_ENTRY_TYPE_SEGHEADER, h);
    }
    void object(uint64_t tableId, const std::string& key, uint64_t version, const void* value, uint32_t valueLen)
    {
        std::vector<uint8_t> o(24 + 1 + 2 + key.size() + valueLen, 0);
        memcpy(&o[8], &version, 8);
        memcpy(&o[16], &tableId, 8);
        o[24] = 1;
        o[25] = uint8_t(key.size());
        memcpy(&o[27], key.data(), key.size());
        if (valueLen)
            memcpy(&o[27 + key.size()], value, valueLen);
        append(RAMCRC_LOG_ENTRY_TYPE_OBJ, o);
    }
    void tombstone(uint64_t tableId, const std::string& key, uint64_t version)
    {
        std::vector<uint8_t> t(32 + key.size(), 0);
        const uint64_t segmentId = 3;
        memcpy(&t[0], &tableId, 8);
        memcpy(&t[8], &segmentId, 8);
        memcpy(&t[16], &version, 8);
        memcpy(&t[32], key.data(), key.size());
        append(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, t);
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

struct Part {
    uint32_t status;
    uint64_t version, value;
};

static Part partOf(const std::vector<uint8_t>& parts, uint32_t q)
{
    Part p;
    memcpy(&p.status, &parts[20 * q], 4);
    memcpy(&p.version, &parts[20 * q + 4], 8);
    memcpy(&p.value, &parts[20 * q + 12], 8);
    return p;
}

static uint64_t bitsOf(double d)
{
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

// ------------------------------------------------------------ the host form
// A host table with the segments it has added (the table keeps pointers into
// them) and one call's outputs.
struct HostSide {
    ramcrc_replay_table_host* table;
    std::vector<std::vector<uint8_t> > segments;
    std::vector<std::vector<ramcrc_seg_entry> > tables;
    std::vector<std::vector<uint64_t> > work;
    std::vector<uint8_t> out, parts;
    std::vector<ramcrc_write_ref> refs;
    ramcrc_seg_cert cert;
    ramcrc_increment_summary sm;

    // Walk `len` bytes of one-length-byte entries and add them as the next batch.
    int add(const std::vector<uint8_t>& seg, uint32_t len)
    {
        segments.push_back(seg);
        segments.back().resize(kCap, 0);
        tables.push_back(std::vector<ramcrc_seg_entry>());
        for (uint32_t at = 0; at < len;) {
            const ramcrc_seg_entry e = {0, at, seg[at + 1], seg[at]};
            tables.back().push_back(e);
            at += 2 + seg[at + 1];
        }
        work.push_back(std::vector<uint64_t>(tables.back().size() + 1));
        const ramcrc_seg_status st = {RAMCRC_SEG_OK, 0, uint32_t(tables.back().size()), 0};
        uint32_t number = ~0u;
        return ramcrc_replay_table_add_host(table, &segments.back()[0], kCap, 1, &st, &tables.back()[0],
                                            tables.back().size(), NULL, &work.back()[0], &number) ||
               number + 1 != segments.size();
    }

    int increment(const std::vector<std::string>& keys, const std::vector<ramcrc_increment_arg>& args,
                  const ramcrc_reject_rules* rules, uint64_t nextVersion)
    {
        std::vector<uint8_t> kb;
        std::vector<ramcrc_lookup_key> reqs(keys.size());
        for (size_t q = 0; q < keys.size(); q++) {
            const ramcrc_lookup_key k = {1, kb.size(), uint32_t(keys[q].size()), 0};
            reqs[q] = k;
            kb.insert(kb.end(), keys[q].begin(), keys[q].end());
        }
        out.assign(kCap, 0);
        parts.assign(20 * keys.size(), 0xA5);
        refs.resize(keys.size());
        return ramcrc_replay_table_increment_host(table, &kb[0], kb.size(), &reqs[0], keys.size(), &args[0], NULL,
                                                  rules, nextVersion, 7, NULL, &out[0], kCap, &cert, &parts[0],
                                                  &refs[0], NULL, &sm);
    }

    // The value-only read of one key: its status, version and first 8 value bytes.
    Part read(const std::string& key)
    {
        const ramcrc_lookup_key k = {1, 0, uint32_t(key.size()), 0};
        uint8_t reply[16 + 64];
        ramcrc_read_summary rs;
        Part p = {~0u, 0, 0};
        if (ramcrc_replay_table_read_host(table, key.data(), key.size(), &k, 1, NULL, NULL, RAMCRC_READ_VALUE_ONLY,
                                          reply, sizeof reply, NULL, NULL, &rs) || rs.returned != 1)
            return p;
        uint32_t length;
        memcpy(&p.status, reply, 4);
        memcpy(&p.version, reply + 4, 8);
        memcpy(&length, reply + 12, 4);
        if (p.status == RAMCRC_STATUS_OK && length == 8)
            memcpy(&p.value, reply + 16, 8);
        return p;
    }
};

static ramcrc_increment_arg arg(int64_t i, double d)
{
    const ramcrc_increment_arg a = {i, d};
    return a;
}

// One increment of one key, then walk and add; returns the mismatches.
static int step(HostSide& h, const std::string& key, int64_t addInt, double addDouble, const ramcrc_reject_rules* rules,
                uint64_t nextVersion, uint32_t wantStatus, uint64_t wantVersion, uint64_t wantValue,
                uint64_t wantNextVersion)
{
    if (h.increment(std::vector<std::string>(1, key), std::vector<ramcrc_increment_arg>(1, arg(addInt, addDouble)),
                    rules, nextVersion))
        return 1;
    const Part p = partOf(h.parts, 0);
    int bad = p.status != wantStatus || p.version != wantVersion || p.value != wantValue ||
              h.sm.next_version != wantNextVersion;
    if (wantStatus == RAMCRC_STATUS_OK) {
        bad += h.sm.ok != 1 || h.add(h.out, h.cert.segment_length);
        const Part r = h.read(key);
        bad += r.status != RAMCRC_STATUS_OK || r.version != wantVersion || r.value != wantValue;
    } else {
        bad += h.sm.ok != 0 || h.sm.out_bytes != 0;
    }
    if (bad)
        printf("step %s: status %u version %llu value %llx next %llu\n", key.c_str(), p.status,
               static_cast<unsigned long long>(p.version), static_cast<unsigned long long>(p.value),
               static_cast<unsigned long long>(h.sm.next_version));
    return bad;
}

static HostSide fresh()
{
    HostSide h;
    h.table = NULL;
    if (ramcrc_replay_table_create_host(64, 16, &h.table))
        throw std::runtime_error("ramcrc_replay_table_create_host failed");
    // (the vectors of added segments must not move: the table points into them)
    h.segments.reserve(16);
    h.tables.reserve(16);
    h.work.reserve(16);
    return h;
}

// A batch of one object.
static int store(HostSide& h, const std::string& key, uint64_t version, const void* value, uint32_t valueLen)
{
    std::vector<uint8_t> seg(kCap, 0);
    Builder b = {&seg[0], 0, Crc32C()};
    b.header(1);
    b.object(1, key, version, value, valueLen);
    return h.add(seg, b.pos);
}

static int goldens()
{
    int bad = 0;
    ramcrc_reject_rules rules;
    const int64_t one = 1, zero = 0;
    const double oneD = 1.0;
    const int32_t zero32 = 0;
    const float zeroF = 0;
    const uint32_t OK = RAMCRC_STATUS_OK;
    {   // increment_basic
        HostSide h = fresh();
        bad += store(h, "key0", 1, &one, 8);
        bad += step(h, "key0", 2, 0.0, NULL, 2, OK, 2, 3, 2);
        bad += store(h, "key1", 2, &oneD, 8);
        bad += step(h, "key1", 0, 2.0, NULL, 3, OK, 3, bitsOf(3.0), 3);
        ramcrc_replay_table_destroy_host(h.table);
    }
    {   // increment_create: versions 1, 2, 3, 4; a zero increment still writes
        HostSide h = fresh();
        bad += step(h, "key0", 1, 0.0, NULL, 1, OK, 1, 1, 2);
        bad += step(h, "key1", 0, 1.0, NULL, 2, OK, 2, bitsOf(1.0), 3);
        bad += step(h, "key2", 0, 0.0, NULL, 3, OK, 3, 0, 4);
        bad += h.sm.out_bytes != 41 || h.sm.created != 1;
        bad += step(h, "key2", 0, 0.0, NULL, 4, OK, 4, 0, 4);
        bad += h.sm.tombstones != 1 || h.sm.created != 0;
        ramcrc_replay_table_destroy_host(h.table);
    }
    {   // increment_rejectRules
        HostSide h = fresh();
        memset(&rules, 0, sizeof rules);
        rules.doesnt_exist = 1;
        bad += step(h, "key0", 1, 0.0, &rules, 1, RAMCRC_STATUS_OBJECT_DOESNT_EXIST, 0, 0, 1);
        memset(&rules, 0, sizeof rules);
        rules.exists = 1;
        bad += store(h, "key1", 1, &zero, 8);
        bad += step(h, "key1", 1, 0.0, &rules, 2, RAMCRC_STATUS_OBJECT_EXISTS, 1, 0, 2);
        bad += store(h, "key2", 2, &zero, 8);
        bad += step(h, "key2", 1, 0.0, NULL, 3, OK, 3, 1, 3);
        memset(&rules, 0, sizeof rules);
        rules.given_version = 2;
        rules.version_ne_given = 1;
        bad += step(h, "key2", 1, 0.0, &rules, 3, RAMCRC_STATUS_WRONG_VERSION, 3, 0, 3);
        ramcrc_replay_table_destroy_host(h.table);
    }
    {   // increment_invalidObject: 4-byte values
        HostSide h = fresh();
        bad += store(h, "key0", 1, &zero32, 4);
        bad += step(h, "key0", 1, 0.0, NULL, 2, RAMCRC_STATUS_INVALID_OBJECT, 1, 0, 2);
        bad += store(h, "key1", 2, &zeroF, 4);
        bad += step(h, "key1", 0, 1.0, NULL, 3, RAMCRC_STATUS_INVALID_OBJECT, 2, bitsOf(1.0), 3);
        bad += h.sm.invalid_object != 1;
        ramcrc_replay_table_destroy_host(h.table);
    }
    {   // multiIncrement_basics: one call, two requests
        HostSide h = fresh();
        std::vector<std::string> keys;
        keys.push_back("0");
        keys.push_back("1");
        std::vector<ramcrc_increment_arg> args;
        args.push_back(arg(1, 0.0));
        args.push_back(arg(0, 1.0));
        bad += h.increment(keys, args, NULL, 1);
        const Part a = partOf(h.parts, 0), b = partOf(h.parts, 1);
        bad += a.status != OK || a.value != 1 || b.status != OK || b.value != bitsOf(1.0);
        bad += a.version + b.version != 3 || h.sm.ok != 2 || h.sm.created != 2 || h.sm.next_version != 3;
        ramcrc_replay_table_destroy_host(h.table);
    }
    {   // multiIncrement_rejectRules
        HostSide h = fresh();
        memset(&rules, 0, sizeof rules);
        rules.doesnt_exist = 1;
        bad += step(h, "key0", 1, 0.0, &rules, 1, RAMCRC_STATUS_OBJECT_DOESNT_EXIST, 0, 0, 1);
        ramcrc_replay_table_destroy_host(h.table);
    }
    return bad;
}

// Increment, walk, add, read; again: the second accumulates on the first's
// output and takes version + 1, and its tombstone carries the first's version.
static int closedLoop()
{
    int bad = 0;
    HostSide h = fresh();
    const int64_t forty = 40;
    bad += store(h, "counter", 7, &forty, 8);
    bad += step(h, "counter", 2, 0.0, NULL, 9, RAMCRC_STATUS_OK, 8, 42, 9);
    bad += h.sm.tombstones != 1 || h.refs[0].object_off != 0 || h.refs[0].tombstone_off != 2 + 24 + 11 + 7;
    bad += step(h, "counter", -50, 0.0, NULL, 9, RAMCRC_STATUS_OK, 9, uint64_t(-8), 9);
    uint64_t tombVersion;
    memcpy(&tombVersion, &h.out[h.refs[0].tombstone_off + 2 + 16], 8);
    bad += tombVersion != 8;
    bad += step(h, "other", 0, 0.5, NULL, 9, RAMCRC_STATUS_OK, 9, bitsOf(0.5), 10);
    bad += step(h, "other", 0, 0.25, NULL, 10, RAMCRC_STATUS_OK, 10, bitsOf(0.75), 10);
    ramcrc_replay_table_destroy_host(h.table);
    return bad;
}

// No GPU: what both forms refuse, the goldens and the closed loop on the host form.
static int cpu()
{
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(16, 2, &hostTable))
        return 1;
    int bad = 0;
    const uint8_t keys[3] = {'0', '1', '2'};
    ramcrc_lookup_key reqs[3];
    ramcrc_increment_arg args[3];
    for (uint32_t q = 0; q < 3; q++) {
        const ramcrc_lookup_key k = {1, q, 1, 0};
        reqs[q] = k;
        args[q] = arg(1, 0.0);
    }
    uint8_t out[64], parts[60];
    ramcrc_write_ref refs[3];
    ramcrc_lookup_result old[3];
    ramcrc_seg_cert cert;
    ramcrc_increment_summary sm;
#define INC_HOST(t, k, r, a, nv, o, c, p, s, n) \
    ramcrc_replay_table_increment_host(t, k, 3, r, n, a, NULL, NULL, nv, 0, NULL, o, 64, c, p, refs, old, s)
    bad += INC_HOST(NULL, keys, reqs, args, 1, out, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 0, out, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 1, out, NULL, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 1, out, &cert, parts, NULL, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, NULL, args, 1, out, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, NULL, 1, out, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 1, out, &cert, NULL, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, NULL, reqs, args, 1, out, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 1, NULL, &cert, parts, &sm, 3) != RAMCRC_EINVAL;
    bad += INC_HOST(hostTable, keys, reqs, args, 1, out, &cert, parts, &sm, 0xFFFFFFFFull) != RAMCRC_EINVAL;
#undef INC_HOST
    bad += ramcrc_replay_table_increment_device(NULL, keys, 3, reqs, 3, args, NULL, NULL, 1, 0, NULL, out, 64, &cert,
                                                parts, refs, old, &sm, NULL) != RAMCRC_EINVAL;
    ramcrc_replay_table_destroy_host(hostTable);
    const int refused = bad;
    const int gold = goldens();
    const int loop = closedLoop();
    bad += gold + loop;
    printf("multiIncrement on the host: refusals %d, goldens %d, closed loop %d; %d mismatches\n", refused, gold, loop,
           bad);
    return bad ? 1 : 0;
}

// ------------------------------------------------------------ the device form
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

// SEGHEADER, then objects (8-byte values, every fifth another length) and
// tombstones of versions 1 .. 5
static ramcrc_seg_cert fill(uint8_t* seg)
{
    Builder b = {seg, 0, Crc32C()};
    b.header(10);
    for (uint32_t k = 0; k < kRecords; k++) {
        const std::string key = std::to_string(k % kKeys);
        const uint64_t version = 1 + (k * 7 + k / kKeys) % 5;
        const uint64_t value[2] = {1000ull * k + 1, k};
        if (k % 3)
            b.object(1, key, version, value, k % 5 ? 8 : 4 + k % 13);
        else
            b.tombstone(1, key, version);
    }
    return b.cert();
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

    // the multi-increment: key q, then key 7 again, then a request past the buffer
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> reqs(kKeys + kNew);
    for (uint32_t q = 0; q < kKeys + kNew; q++) {
        const std::string key = std::to_string(q);
        const ramcrc_lookup_key k = {1, keys.size(), uint32_t(key.size()), 0};
        reqs[q] = k;
        keys.insert(keys.end(), key.begin(), key.end());
    }
    reqs.resize(kReqs);
    reqs[kReqs - 2] = reqs[7];
    reqs[kReqs - 1] = reqs[0];
    reqs[kReqs - 1].key_off = keys.size();
    std::vector<ramcrc_reject_rules> rules(kReqs);
    memset(&rules[0], 0, kReqs * sizeof(ramcrc_reject_rules));
    for (uint32_t q = 0; q < kReqs; q += 7)
        rules[q].exists = 1;
    std::vector<ramcrc_increment_arg> args(kReqs);
    for (uint32_t q = 0; q < kReqs; q++)
        args[q] = arg(q % 2 ? int64_t(q) : 0, q % 2 ? 0.0 : 0.5 * q);
    const uint64_t segmentIds[2] = {10, 77};
    const uint64_t nextVersion = 3;
    const uint32_t timestamp = 0x12345678;

    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_reqs = dalloc<ramcrc_lookup_key>(kReqs);
    ramcrc_increment_arg* d_args = dalloc<ramcrc_increment_arg>(kReqs);
    ramcrc_reject_rules* d_rules = dalloc<ramcrc_reject_rules>(kReqs);
    uint64_t* d_segmentIds = dalloc<uint64_t>(2);
    uint8_t* d_parts = dalloc<uint8_t>(20 * kReqs);
    ramcrc_write_ref* d_refs = dalloc<ramcrc_write_ref>(kReqs);
    ramcrc_lookup_result* d_old = dalloc<ramcrc_lookup_result>(kReqs);
    ramcrc_increment_summary* d_summary = dalloc<ramcrc_increment_summary>(1);
    Arrived second;
    second.d_base = dalloc<uint8_t>(kCap);
    second.d_cert = dalloc<ramcrc_seg_cert>(1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_reqs, &reqs[0], kReqs * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_args, &args[0], kReqs * sizeof(ramcrc_increment_arg), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rules, &rules[0], kReqs * sizeof(ramcrc_reject_rules), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_segmentIds, segmentIds, sizeof segmentIds, hipMemcpyHostToDevice));
    HIP(hipMemset(second.d_base, 0, kCap));
    table.multiIncrement(d_keys, keys.size(), d_reqs, kReqs, d_args, NULL, d_rules, nextVersion, timestamp,
                         d_segmentIds, second.d_base, kCap, second.d_cert, d_parts, d_refs, d_old, d_summary);
    batch.sync();

    std::vector<uint8_t> out(kCap), wantOut(kCap, 0), parts(20 * kReqs), wantParts(20 * kReqs);
    std::vector<ramcrc_write_ref> refs(kReqs), wantRefs(kReqs);
    std::vector<ramcrc_lookup_result> old(kReqs), wantOld(kReqs);
    ramcrc_increment_summary sm, wantSm;
    ramcrc_seg_cert cert, wantCert;
    HIP(hipMemcpy(&out[0], second.d_base, kCap, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&parts[0], d_parts, 20 * kReqs, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&refs[0], d_refs, kReqs * sizeof(ramcrc_write_ref), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&old[0], d_old, kReqs * sizeof(ramcrc_lookup_result), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&sm, d_summary, sizeof sm, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&cert, second.d_cert, sizeof cert, hipMemcpyDeviceToHost));
    if (ramcrc_replay_table_increment_host(hostTable, &keys[0], keys.size(), &reqs[0], kReqs, &args[0], NULL,
                                           &rules[0], nextVersion, timestamp, segmentIds, &wantOut[0], kCap,
                                           &wantCert, &wantParts[0], &wantRefs[0], &wantOld[0], &wantSm))
        return 1;
    // (the bytes at and past the head keep their zeros in both)
    bad += memcmp(&out[0], &wantOut[0], kCap) != 0;
    bad += memcmp(&parts[0], &wantParts[0], 20 * kReqs) != 0;
    bad += memcmp(&refs[0], &wantRefs[0], kReqs * sizeof(ramcrc_write_ref)) != 0;
    bad += memcmp(&old[0], &wantOld[0], kReqs * sizeof(ramcrc_lookup_result)) != 0;
    bad += memcmp(&sm, &wantSm, sizeof sm) != 0;
    bad += memcmp(&cert, &wantCert, sizeof cert) != 0;
    bad += sm.spoiled != 0 || sm.bad != 1 || sm.retry_duplicate != 1 || sm.retry_full != 0;
    bad += sm.ok + sm.object_exists + sm.invalid_object != kKeys + kNew || sm.object_exists == 0;
    bad += sm.invalid_object == 0 || sm.tombstones == 0 || sm.created < kNew || sm.ok != sm.created + sm.tombstones;
    bad += sm.next_version < nextVersion + sm.allocated || cert.segment_length != sm.out_bytes;

    // walk the output with its certificate, add it, read every key
    bad += arrive(batch, table, hostTable, second, 1, true);
    bad += second.n != sm.ok + sm.tombstones;
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
    uint64_t at = 0, served = 0;
    for (uint32_t q = 0; q < rs.returned; q++) {
        uint32_t status, length;
        uint64_t version;
        memcpy(&status, &reply[at], 4);
        memcpy(&version, &reply[at + 4], 8);
        memcpy(&length, &reply[at + 12], 4);
        at += 16;
        const Part p = partOf(parts, q);
        if (p.status == RAMCRC_STATUS_OK) {
            // the new object answers with the part's version and value
            bad += status != RAMCRC_STATUS_OK || version != p.version || length != 8 ||
                   memcmp(&reply[at], &p.value, 8) != 0;
            served++;
        } else {
            // refused, or an invalid object: the old object still answers; the third field is add_double
            bad += status != RAMCRC_STATUS_OK || version != p.version || p.value != bitsOf(args[q].add_double);
            bad += p.status != RAMCRC_STATUS_OBJECT_EXISTS && p.status != RAMCRC_STATUS_INVALID_OBJECT;
        }
        if (status == RAMCRC_STATUS_OK)
            at += length;
    }
    bad += served != sm.ok;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("multiIncrement: %llu objects written (%llu created), %llu tombstones, %llu refused, %llu invalid; "
           "%d mismatches\n",
           static_cast<unsigned long long>(sm.ok), static_cast<unsigned long long>(sm.created),
           static_cast<unsigned long long>(sm.tombstones), static_cast<unsigned long long>(sm.object_exists),
           static_cast<unsigned long long>(sm.invalid_object), bad);
    return bad ? 1 : 0;
}
