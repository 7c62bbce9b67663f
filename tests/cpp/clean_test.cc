// RAMCloud::ReplayTable::clean and cleanSize as a master's cleaner uses them:
// two segments are added -- 150 objects and tombstones of the keys "0" .. "49"
// of table 1, then newer objects of the keys "0" .. "24" --, cleanSize sizes
// the survivor of the first batch, clean moves its 25 live records and retires
// it.  Usage, summary, survivor bytes, certificate, status, record table, count
// and old references are compared with the host form
// (ramcrc_replay_table_clean_host) byte for byte; the survivor is walked with
// the call's certificate by deviceReplayVerify, which must write the same
// status and record table; then the victim's arrays are overwritten and a
// multiRead of every key must return the host form's reply.  With --cpu the
// program validates arguments and runs the host form alone, against a lookup
// before and after.  Built with hipcc for hipMalloc.
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
static const uint32_t kRecords = 150, kKeys = 50, kNewer = 25;
static const uint64_t kEcap = 1024;

// One segment built on the host, with the record table its walk would write.
struct Built {
    std::vector<uint8_t> seg;
    std::vector<ramcrc_seg_entry> table;
    std::vector<uint64_t> work;
    ramcrc_seg_cert cert;
    ramcrc_seg_status status;
    uint32_t pos;
    Crc32C meta;
    Built() : seg(kCap, 0), pos(0) {}
    void append(uint8_t type, const std::vector<uint8_t>& payload)
    {
        const uint32_t len = uint32_t(payload.size());   // < 256 here
        seg[pos] = type;
        seg[pos + 1] = uint8_t(len);
        meta.update(&seg[pos], 2);
        memcpy(&seg[pos + 2], payload.data(), len);
        const ramcrc_seg_entry e = {0, pos, len, type};
        table.push_back(e);
        pos += 2 + len;
    }
    void seal()
    {
        cert.segment_length = pos;
        meta.update(&pos, 4);
        cert.checksum = meta.getResult();
        const ramcrc_seg_status s = {RAMCRC_SEG_OK, cert.checksum, uint32_t(table.size()), 0};
        status = s;
        work.assign(table.size(), 0);
    }
};

static void put64(std::vector<uint8_t>& v, size_t at, uint64_t x) { memcpy(&v[at], &x, 8); }

static std::vector<uint8_t> object(const std::string& key, uint64_t version, uint32_t value, uint8_t fill)
{
    std::vector<uint8_t> o(24 + 1 + 2 + key.size() + value, fill);
    put64(o, 0, 0);
    put64(o, 8, version);
    put64(o, 16, 1);
    o[24] = 1;
    o[25] = uint8_t(key.size());
    o[26] = 0;
    memcpy(&o[27], key.data(), key.size());
    return o;
}

// SEGHEADER, then objects and tombstones of versions 1 .. 5
static void fillFirst(Built& b)
{
    std::vector<uint8_t> h(24, 0);
    put64(h, 8, 10);
    b.append(RAMCRC_LOG_ENTRY_TYPE_SEGHEADER, h);
    for (uint32_t k = 0; k < kRecords; k++) {
        const std::string key = std::to_string(k % kKeys);
        const uint64_t version = 1 + (k * 7 + k / kKeys) % 5;
        if (k % 3) {
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, object(key, version, k % 40, uint8_t(k)));
        } else {
            std::vector<uint8_t> t(32 + key.size(), 0);
            put64(t, 0, 1);
            put64(t, 8, 3);
            put64(t, 16, version);
            memcpy(&t[32], key.data(), key.size());
            b.append(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, t);
        }
    }
    b.seal();
}

// newer objects of the keys "0" .. "24"
static void fillSecond(Built& b)
{
    for (uint32_t k = 0; k < kNewer; k++)
        b.append(RAMCRC_LOG_ENTRY_TYPE_OBJ, object(std::to_string(k), 9, 20 + k, uint8_t(0xC0 + k)));
    b.seal();
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

// What a clean writes, on the host.
struct Survivor {
    std::vector<uint8_t> out;
    std::vector<ramcrc_seg_entry> entries;
    std::vector<uint64_t> work;
    std::vector<ramcrc_replay_ref> moved;
    ramcrc_seg_cert cert;
    ramcrc_seg_status status;
    uint64_t n;
    ramcrc_clean_usage usage;
    ramcrc_clean_summary summary;
    Survivor() : out(kCap, 0xA5), entries(kEcap), work(kEcap, 0), moved(kEcap), n(0)
    {
        memset(&entries[0], 0xA5, kEcap * sizeof(ramcrc_seg_entry));
        memset(&moved[0], 0xA5, kEcap * sizeof(ramcrc_replay_ref));
        memset(&cert, 0xA5, sizeof cert);
        memset(&status, 0xA5, sizeof status);
    }
};

// Both batches into the host table, cleanSize and clean of batch 0 there.
static int hostClean(ramcrc_replay_table_host* t, Built& a, Built& b, Survivor& s, uint32_t cap, uint64_t ecap)
{
    uint32_t n0 = ~0u, n1 = ~0u, n2 = ~0u;
    if (ramcrc_replay_table_add_host(t, &a.seg[0], kCap, 1, &a.status, &a.table[0], a.table.size(), NULL,
                                     &a.work[0], &n0) ||
        ramcrc_replay_table_add_host(t, &b.seg[0], kCap, 1, &b.status, &b.table[0], b.table.size(), NULL,
                                     &b.work[0], &n1) ||
        n0 != 0 || n1 != 1)
        return 1;
    const uint32_t victim = 0;
    ramcrc_clean_usage usage;
    ramcrc_clean_summary size;
    if (ramcrc_replay_table_clean_size_host(t, &victim, 1, &usage, &size))
        return 1;
    int bad = 0;
    bad += size.records != kRecords + 1 || size.needed_records != kKeys - kNewer || size.dropped_other != 1;
    bad += size.moved_objects + size.moved_tombstones != kKeys - kNewer || size.batch != 0 || size.spoiled != 0;
    bad += size.out_bytes != size.needed_bytes || usage.live_bytes != size.needed_bytes;
    if (cap == 0)
        cap = uint32_t((size.needed_bytes + 15) / 16 * 16);
    if (ecap == 0)
        ecap = size.needed_records;
    if (ramcrc_replay_table_clean_host(t, &victim, 1, &s.out[0], cap, &s.cert, &s.status, &s.entries[0], ecap,
                                       &s.n, &s.work[0], &s.moved[0], &s.usage, &s.summary, &n2) ||
        n2 != 2)
        return 1;
    size.batch = 2;
    bad += memcmp(&size, &s.summary, sizeof size) != 0 || memcmp(&usage, &s.usage, sizeof usage) != 0;
    bad += s.n != size.needed_records || s.cert.segment_length != size.needed_bytes;
    bad += s.status.flags != RAMCRC_SEG_OK || s.status.checksum != s.cert.checksum || s.status.entries != s.n;
    bad += s.out[size.needed_bytes] != 0xA5 || s.entries[s.n].offset != 0xA5A5A5A5u;
    return bad;
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

// No GPU: what both forms refuse, and the host form with a lookup around it.
static int cpu()
{
    ramcrc_replay_table_host* t = NULL;
    if (ramcrc_replay_table_create_host(4 * kKeys, 4, &t))
        return 1;
    int bad = 0;
    Built a, b;
    fillFirst(a);
    fillSecond(b);
    Survivor s;
    const uint32_t victim = 0, twice[2] = {0, 0}, never = 7;
    ramcrc_clean_summary sm;
    // refused: before anything is added every number is unknown
    bad += ramcrc_replay_table_clean_size_host(t, &victim, 1, NULL, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_clean_size_host(NULL, &victim, 1, NULL, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_clean_size_device(NULL, &victim, 1, NULL, &sm, NULL) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_clean_device(NULL, &victim, 1, &s.out[0], kCap, &s.cert, &s.status, &s.entries[0],
                                            kEcap, &s.n, &s.work[0], NULL, NULL, &sm, NULL, NULL) != RAMCRC_EINVAL;
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> queries;
    pack(kKeys + 5, keys, queries);
    // the host form; the lookups around it
    std::vector<ramcrc_lookup_result> before(queries.size()), after(queries.size());
    {
        // (hostClean adds first: look up between the adds and the clean through a second table)
        ramcrc_replay_table_host* u = NULL;
        Built a2, b2;
        fillFirst(a2);
        fillSecond(b2);
        uint32_t n;
        if (ramcrc_replay_table_create_host(4 * kKeys, 4, &u) ||
            ramcrc_replay_table_add_host(u, &a2.seg[0], kCap, 1, &a2.status, &a2.table[0], a2.table.size(), NULL,
                                         &a2.work[0], &n) ||
            ramcrc_replay_table_add_host(u, &b2.seg[0], kCap, 1, &b2.status, &b2.table[0], b2.table.size(), NULL,
                                         &b2.work[0], &n) ||
            ramcrc_replay_table_lookup_host(u, &keys[0], keys.size(), &queries[0], queries.size(), NULL, &before[0],
                                            NULL))
            return 1;
        ramcrc_replay_table_destroy_host(u);
    }
    bad += hostClean(t, a, b, s, 0, 0);
    // rule 1 and rule 6 on the handle
    bad += ramcrc_replay_table_clean_size_host(t, &victim, 1, NULL, &sm) != RAMCRC_EINVAL;   // cleaned
    bad += ramcrc_replay_table_clean_size_host(t, twice, 2, NULL, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_clean_size_host(t, &never, 1, NULL, &sm) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_clean_size_host(t, &victim, 0, NULL, &sm) != RAMCRC_EINVAL;
    uint64_t nLive;
    ramcrc_resolve_counts counts;
    bad += ramcrc_replay_table_live_host(t, 0, NULL, NULL, 0, &nLive, &counts) != RAMCRC_EINVAL;
    bad += ramcrc_replay_table_live_host(t, 2, NULL, NULL, 0, &nLive, &counts) != RAMCRC_OK || nLive != s.n;
    // the victim's arrays are ours again
    memset(&a.seg[0], 0xA5, kCap);
    memset(&a.table[0], 0xA5, a.table.size() * sizeof(ramcrc_seg_entry));
    memset(&a.work[0], 0xA5, a.work.size() * 8);
    if (ramcrc_replay_table_lookup_host(t, &keys[0], keys.size(), &queries[0], queries.size(), NULL, &after[0],
                                        NULL))
        return 1;
    uint64_t movedKeys = 0;
    for (size_t q = 0; q < queries.size(); q++) {
        bad += after[q].kind != before[q].kind || after[q].version != before[q].version ||
               after[q].value_len != before[q].value_len;
        if (before[q].ref.batch == 0) {
            movedKeys++;
            bad += after[q].ref.batch != 2 || after[q].ref.record >= s.n ||
                   s.moved[after[q].ref.record].batch != 0 ||
                   s.moved[after[q].ref.record].record != before[q].ref.record;
        } else {
            bad += memcmp(&after[q], &before[q], sizeof after[q]) != 0;
        }
    }
    bad += movedKeys != s.n;
    ramcrc_replay_table_stats stats;
    bad += ramcrc_replay_table_stats_host(t, &stats) != RAMCRC_OK || stats.batches != 3 || stats.keys != kKeys;
    ramcrc_replay_table_destroy_host(t);
    printf("clean on the host: %llu records moved, %llu bytes; %d mismatches\n",
           static_cast<unsigned long long>(s.n), static_cast<unsigned long long>(s.summary.out_bytes), bad);
    return bad ? 1 : 0;
}

// One built segment on the device, verified and added to the device table.
struct Arrived {
    uint8_t* d_base;
    ramcrc_seg_cert* d_cert;
    ramcrc_seg_status* d_status;
    ramcrc_seg_entry* d_entries;
    uint64_t *d_n, *d_work;
    uint32_t* d_crc;
};

static int arrive(Crc32CBatch& batch, ReplayTable& table, const Built& b, Arrived& a, uint32_t number)
{
    a.d_base = dalloc<uint8_t>(kCap);
    a.d_cert = dalloc<ramcrc_seg_cert>(1);
    a.d_status = dalloc<ramcrc_seg_status>(1);
    a.d_entries = dalloc<ramcrc_seg_entry>(kEcap);
    a.d_n = dalloc<uint64_t>(1);
    a.d_work = dalloc<uint64_t>(kEcap);
    a.d_crc = dalloc<uint32_t>(kEcap);
    HIP(hipMemcpy(a.d_base, &b.seg[0], kCap, hipMemcpyHostToDevice));
    HIP(hipMemcpy(a.d_cert, &b.cert, sizeof b.cert, hipMemcpyHostToDevice));
    batch.deviceReplayVerify(a.d_base, kCap, kCap, 1, a.d_cert, a.d_status, a.d_entries, kEcap, a.d_n, a.d_crc);
    int bad = table.add(a.d_base, kCap, 1, a.d_status, a.d_entries, kEcap, a.d_n, NULL, a.d_work) != number;
    batch.sync();
    // the walk writes the table the builder wrote
    std::vector<ramcrc_seg_entry> got(b.table.size());
    uint64_t n = 0;
    HIP(hipMemcpy(&n, a.d_n, 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got[0], a.d_entries, got.size() * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    bad += n != b.table.size() || memcmp(&got[0], &b.table[0], got.size() * sizeof(ramcrc_seg_entry)) != 0;
    return bad;
}

static int run()
{
    Crc32CBatch batch(0);
    ReplayTable table(batch, 4 * kKeys, 4);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(4 * kKeys, 4, &hostTable))
        return 1;
    int bad = 0;
    Built a, b;
    fillFirst(a);
    fillSecond(b);
    Arrived first, second;
    bad += arrive(batch, table, a, first, 0);
    bad += arrive(batch, table, b, second, 1);

    // cleanSize, then the outputs at exactly that size
    const uint32_t victim = 0;
    ramcrc_clean_usage* d_usage = dalloc<ramcrc_clean_usage>(2);
    ramcrc_clean_summary* d_summary = dalloc<ramcrc_clean_summary>(2);
    table.cleanSize(&victim, 1, d_usage, d_summary);
    batch.sync();
    ramcrc_clean_summary size;
    ramcrc_clean_usage sizeUsage;
    HIP(hipMemcpy(&size, d_summary, sizeof size, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&sizeUsage, d_usage, sizeof sizeUsage, hipMemcpyDeviceToHost));
    const uint32_t cap = uint32_t((size.needed_bytes + 15) / 16 * 16);
    const uint64_t ecap = size.needed_records;
    bad += ecap != kKeys - kNewer || cap == 0 || cap > kCap;

    uint8_t* d_out = dalloc<uint8_t>(kCap);
    ramcrc_seg_cert* d_cert = dalloc<ramcrc_seg_cert>(1);
    ramcrc_seg_status* d_status = dalloc<ramcrc_seg_status>(1);
    ramcrc_seg_entry* d_entries = dalloc<ramcrc_seg_entry>(kEcap);
    uint64_t* d_n = dalloc<uint64_t>(1);
    uint64_t* d_work = dalloc<uint64_t>(kEcap);
    ramcrc_replay_ref* d_moved = dalloc<ramcrc_replay_ref>(kEcap);
    HIP(hipMemset(d_out, 0xA5, kCap));
    HIP(hipMemset(d_entries, 0xA5, kEcap * sizeof(ramcrc_seg_entry)));
    HIP(hipMemset(d_moved, 0xA5, kEcap * sizeof(ramcrc_replay_ref)));
    HIP(hipMemset(d_work, 0xA5, kEcap * 8));
    bad += table.clean(&victim, 1, d_out, cap, d_cert, d_status, d_entries, ecap, d_n, d_work, d_moved,
                       d_usage + 1, d_summary + 1) != 2;
    batch.sync();

    Survivor got, want;
    std::vector<uint64_t> oldWork(kEcap);
    HIP(hipMemcpy(&got.out[0], d_out, kCap, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.entries[0], d_entries, kEcap * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.moved[0], d_moved, kEcap * sizeof(ramcrc_replay_ref), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.work[0], d_work, kEcap * 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&oldWork[0], first.d_work, kEcap * 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.cert, d_cert, sizeof got.cert, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.status, d_status, sizeof got.status, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.n, d_n, 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.usage, d_usage + 1, sizeof got.usage, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&got.summary, d_summary + 1, sizeof got.summary, hipMemcpyDeviceToHost));
    bad += hostClean(hostTable, a, b, want, cap, ecap);
    // (the bytes at and past the head and the rows past the count keep their 0xA5 in both)
    bad += memcmp(&got.out[0], &want.out[0], kCap) != 0;
    bad += memcmp(&got.entries[0], &want.entries[0], kEcap * sizeof(ramcrc_seg_entry)) != 0;
    bad += memcmp(&got.moved[0], &want.moved[0], kEcap * sizeof(ramcrc_replay_ref)) != 0;
    bad += memcmp(&got.cert, &want.cert, sizeof got.cert) != 0;
    bad += memcmp(&got.status, &want.status, sizeof got.status) != 0;
    bad += got.n != want.n;
    bad += memcmp(&got.usage, &want.usage, sizeof got.usage) != 0 || memcmp(&sizeUsage, &want.usage, sizeof sizeUsage) != 0;
    bad += memcmp(&got.summary, &want.summary, sizeof got.summary) != 0;
    size.batch = 2;
    bad += memcmp(&size, &got.summary, sizeof size) != 0;
    for (uint64_t j = 0; j < got.n && j < kEcap; j++)
        bad += got.work[j] != oldWork[got.moved[j].record];   // the survivor's slot is its old one

    // the existing walk over the survivor, under the call's certificate
    ramcrc_seg_status* d_status2 = dalloc<ramcrc_seg_status>(1);
    ramcrc_seg_entry* d_entries2 = dalloc<ramcrc_seg_entry>(kEcap);
    uint64_t* d_n2 = dalloc<uint64_t>(1);
    uint32_t* d_crc2 = dalloc<uint32_t>(kEcap);
    batch.deviceReplayVerify(d_out, cap, cap, 1, d_cert, d_status2, d_entries2, kEcap, d_n2, d_crc2);
    batch.sync();
    ramcrc_seg_status walked;
    std::vector<ramcrc_seg_entry> walkedTable(kEcap);
    uint64_t walkedN = 0;
    HIP(hipMemcpy(&walked, d_status2, sizeof walked, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&walkedTable[0], d_entries2, kEcap * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&walkedN, d_n2, 8, hipMemcpyDeviceToHost));
    bad += walkedN != got.n || walked.flags != got.status.flags || walked.checksum != got.status.checksum ||
           walked.entries != got.status.entries;
    bad += memcmp(&walkedTable[0], &got.entries[0], got.n * sizeof(ramcrc_seg_entry)) != 0;

    // the victim's arrays are ours again: overwrite them, then read every key
    HIP(hipMemset(first.d_base, 0xA5, kCap));
    HIP(hipMemset(first.d_status, 0xA5, sizeof(ramcrc_seg_status)));
    HIP(hipMemset(first.d_entries, 0xA5, kEcap * sizeof(ramcrc_seg_entry)));
    HIP(hipMemset(first.d_n, 0xA5, 8));
    HIP(hipMemset(first.d_work, 0xA5, kEcap * 8));
    memset(&a.seg[0], 0xA5, kCap);
    memset(&a.table[0], 0xA5, a.table.size() * sizeof(ramcrc_seg_entry));
    memset(&a.work[0], 0xA5, a.work.size() * 8);
    std::vector<uint8_t> keys;
    std::vector<ramcrc_lookup_key> queries;
    pack(kKeys + 5, keys, queries);
    const uint64_t room = uint64_t(queries.size()) * (16 + 128);
    uint8_t* d_keys = dalloc<uint8_t>(keys.size());
    ramcrc_lookup_key* d_queries = dalloc<ramcrc_lookup_key>(queries.size());
    uint8_t* d_reply = dalloc<uint8_t>(room);
    ramcrc_read_summary* d_readSummary = dalloc<ramcrc_read_summary>(1);
    HIP(hipMemcpy(d_keys, &keys[0], keys.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_queries, &queries[0], queries.size() * sizeof(ramcrc_lookup_key), hipMemcpyHostToDevice));
    HIP(hipMemset(d_reply, 0, room));
    table.multiRead(d_keys, keys.size(), d_queries, queries.size(), NULL, NULL, false, d_reply, room, NULL, NULL,
                    d_readSummary);
    batch.sync();
    std::vector<uint8_t> reply(room), wantReply(room, 0);
    ramcrc_read_summary rs, wantRs;
    HIP(hipMemcpy(&reply[0], d_reply, room, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&rs, d_readSummary, sizeof rs, hipMemcpyDeviceToHost));
    if (ramcrc_replay_table_read_host(hostTable, &keys[0], keys.size(), &queries[0], queries.size(), NULL, NULL, 0,
                                      &wantReply[0], room, NULL, NULL, &wantRs))
        return 1;
    bad += memcmp(&rs, &wantRs, sizeof rs) != 0 || memcmp(&reply[0], &wantReply[0], room) != 0;
    bad += rs.returned != queries.size() || rs.ok == 0 || rs.doesnt_exist < 5;
    ramcrc_replay_table_destroy_host(hostTable);
    printf("clean: %llu records moved, %llu bytes, %llu dropped; %d mismatches\n",
           static_cast<unsigned long long>(got.n), static_cast<unsigned long long>(got.summary.out_bytes),
           static_cast<unsigned long long>(got.summary.dropped_objects + got.summary.dropped_tombstones), bad);
    return bad ? 1 : 0;
}
