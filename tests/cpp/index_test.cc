// RAMCloud::ReplayTable::buildIndex and lookupIndexKeys as a master serves an
// indexed read from the table it recovered into: recovery segments arrive in
// two batches (two segments, then one), each is verified and added as it
// arrives, and after each add the index over key 1 is rebuilt, a batch of range
// queries is answered from it, and the returned hashes go to readHashes where
// they lie, all on one stream.  Entries (key_off dereferenced), hashes, results
// and summaries are compared with the host forms
// (ramcrc_replay_table_index_build_host, ramcrc_index_lookup_host) over a host
// table fed the same batches; the objects readHashes returns carry a second
// key inside the asked range.  Built with hipcc for hipMalloc.
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

// The second key of the object record k of segment s writes: a city of 3 .. 14
// bytes; several primary keys share one, and a key's city changes from one
// version to the next.
static std::string city(uint32_t k, uint32_t s)
{
    return "city" + std::string((k + s) % 11, 'x') + std::to_string((k * 3 + s) % 7);
}

// SEGHEADER, safe version 1 + s, then two-key objects and tombstones
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
        if ((k + s) % 7) {
            // Object::Header {checksum, timestamp, version, tableId}, KeyCount,
            // two CumulativeKeyLengths, the keys, a value of k % 20 bytes
            const std::string second = city(k, s);
            std::vector<uint8_t> o(24 + 1 + 4 + key.size() + second.size() + k % 20, uint8_t(k));
            memset(&o[0], 0, 24);
            put64(o, 8, version);
            put64(o, 16, 1);
            o[24] = 2;
            o[25] = uint8_t(key.size());
            o[26] = 0;
            o[27] = uint8_t(key.size() + second.size());
            o[28] = 0;
            memcpy(&o[29], key.data(), key.size());
            memcpy(&o[29 + key.size()], second.data(), second.size());
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
static const uint64_t kIndexCap = 64, kKeysCap = 1024, kOutCap = 256, kReplyCap = 64 * 1024;

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

struct Range {
    std::string first, last;
    uint64_t firstAllowed;
    uint32_t maxHashes;
};

static int run()
{
    Crc32CBatch batch(0);
    ReplayTable table(batch, 2 * kKeys, kBatches);
    ramcrc_replay_table_host* hostTable = NULL;
    if (ramcrc_replay_table_create_host(2 * kKeys, kBatches, &hostTable))
        return 1;
    ramcrc_index_entry* d_ix = dalloc<ramcrc_index_entry>(kIndexCap + 1);
    uint64_t* d_ixHashes = dalloc<uint64_t>(kIndexCap + 1);
    uint8_t* d_ixKeys = dalloc<uint8_t>(kKeysCap);
    ramcrc_index_build_summary* d_bs = dalloc<ramcrc_index_build_summary>(1);
    uint8_t* d_qkeys = dalloc<uint8_t>(1024);
    ramcrc_index_query* d_q = dalloc<ramcrc_index_query>(16);
    ramcrc_index_result* d_res = dalloc<ramcrc_index_result>(16);
    uint64_t* d_out = dalloc<uint64_t>(kOutCap);
    ramcrc_index_lookup_summary* d_ls = dalloc<ramcrc_index_lookup_summary>(1);
    uint8_t* d_reply = dalloc<uint8_t>(kReplyCap);
    ramcrc_read_hashes_summary* d_rs = dalloc<ramcrc_read_hashes_summary>(1);

    const Range ranges[] = {{"", "", 0, 1000}, {"city0", "cityx9", 0, 1000}, {"cityxx", "cityxxxx", 0, 3},
                            {"cityxxxxxxxx", "", 0, 1000}, {"cityxxx3", "cityxxx3", 0, 1000}, {"d", "c", 0, 10}};
    const uint32_t nq = sizeof ranges / sizeof ranges[0];
    std::string qk;
    std::vector<ramcrc_index_query> queries;
    for (uint32_t i = 0; i < nq; i++) {
        const ramcrc_index_query q = {qk.size(), qk.size() + ranges[i].first.size(), ranges[i].firstAllowed,
                                      uint32_t(ranges[i].first.size()), uint32_t(ranges[i].last.size()),
                                      ranges[i].maxHashes, 0u};
        queries.push_back(q);
        qk += ranges[i].first + ranges[i].last;
    }
    HIP(hipMemcpy(d_qkeys, qk.data(), qk.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_q, &queries[0], nq * sizeof queries[0], hipMemcpyHostToDevice));

    Arrived arrived[kBatches];
    int bad = 0;
    uint32_t seg = 0;
    uint64_t entriesAtEnd = 0, objectsRead = 0;
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

        // the indexed read the master serves while the next batch is on its
        // way: build, lookup, read_hashes of the first query's hashes, no sync
        // in between
        HIP(hipMemset(d_ix, 0xA5, (kIndexCap + 1) * sizeof *d_ix));
        HIP(hipMemset(d_ixHashes, 0xA5, (kIndexCap + 1) * 8));
        HIP(hipMemset(d_out, 0xA5, kOutCap * 8));
        table.buildIndex(1, 1, d_ix, kIndexCap, d_ixHashes, d_ixKeys, kKeysCap, d_bs);
        table.lookupIndexKeys(d_ix, d_ixHashes, d_ixKeys, d_bs, d_qkeys, qk.size(), d_q, nq, d_out, kOutCap,
                              d_res, d_ls);
        batch.sync();
        ramcrc_index_build_summary bs, wantBs;
        ramcrc_index_lookup_summary ls, wantLs;
        std::vector<ramcrc_index_entry> ix(kIndexCap + 1), wantIx(kIndexCap);
        std::vector<uint64_t> ixHashes(kIndexCap + 1), wantHashes(kIndexCap), out(kOutCap), wantOut(kOutCap, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<uint8_t> ixKeys(kKeysCap), wantKeys(kKeysCap);
        std::vector<ramcrc_index_result> res(nq), wantRes(nq);
        HIP(hipMemcpy(&bs, d_bs, sizeof bs, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&ls, d_ls, sizeof ls, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&ix[0], d_ix, ix.size() * sizeof ix[0], hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&ixHashes[0], d_ixHashes, ixHashes.size() * 8, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&ixKeys[0], d_ixKeys, kKeysCap, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&res[0], d_res, nq * sizeof res[0], hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&out[0], d_out, kOutCap * 8, hipMemcpyDeviceToHost));
        if (ramcrc_replay_table_index_build_host(hostTable, 1, 1, &wantIx[0], kIndexCap, &wantHashes[0], &wantKeys[0],
                                                 kKeysCap, &wantBs))
            return 1;
        bad += memcmp(&bs, &wantBs, sizeof bs) != 0 || bs.overflow || bs.n_entries == 0 || bs.n_entries > kKeys;
        for (uint64_t i = 0; i < bs.n_entries && i < wantBs.n_entries; i++) {
            const ramcrc_index_entry &e = ix[i], &w = wantIx[i];
            bad += e.prefix != w.prefix || e.pk_hash != w.pk_hash || e.key_len != w.key_len || e.reserved != 0 ||
                   ixHashes[i] != e.pk_hash || e.key_off + e.key_len > bs.key_bytes ||
                   memcmp(&ixKeys[e.key_off], &wantKeys[w.key_off], e.key_len) != 0;
        }
        // nothing past the entries
        bad += ixHashes[bs.n_entries] != 0xA5A5A5A5A5A5A5A5ull || ix[bs.n_entries].key_len != 0xA5A5A5A5u;
        // the lookup of the host form over the device's index: byte for byte
        if (ramcrc_index_lookup_host(&ix[0], &ixHashes[0], &ixKeys[0], &bs, qk.data(), qk.size(), &queries[0], nq,
                                     &wantOut[0], kOutCap, &wantRes[0], &wantLs))
            return 1;
        bad += memcmp(&ls, &wantLs, sizeof ls) != 0 || memcmp(&res[0], &wantRes[0], nq * sizeof res[0]) != 0 ||
               memcmp(&out[0], &wantOut[0], kOutCap * 8) != 0;
        bad += ls.served != nq || res[0].num_hashes != bs.n_entries || res[5].num_hashes != 0 ||
               res[2].num_hashes > 3 || ls.n_entries != bs.n_entries;
        // the second half of the indexed read, for query 1: every object
        // returned carries a city within ["city0", "cityx9"]
        table.readHashes(1, d_out + res[1].out_off, res[1].num_hashes, d_reply, kReplyCap, kReplyCap, NULL, d_rs);
        batch.sync();
        ramcrc_read_hashes_summary rs;
        std::vector<uint8_t> reply(kReplyCap);
        HIP(hipMemcpy(&rs, d_rs, sizeof rs, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(&reply[0], d_reply, kReplyCap, hipMemcpyDeviceToHost));
        bad += rs.hashes != res[1].num_hashes || rs.objects != res[1].num_hashes;
        uint64_t at = 0;
        for (uint64_t o = 0; o < rs.objects && at + 12 <= rs.reply_bytes; o++) {
            uint32_t length;
            memcpy(&length, &reply[at + 8], 4);
            const uint8_t* d = &reply[at + 12];   // key count, cumulative lengths, keys, value
            const uint32_t k0 = d[1] | (d[2] << 8), k1 = d[3] | (d[4] << 8);
            const std::string second(reinterpret_cast<const char*>(d + 5 + k0), k1 - k0);
            bad += d[0] != 2 || second < "city0" || second > "cityx9";
            at += 12 + length;
            objectsRead++;
        }
        bad += at != rs.reply_bytes;
        entriesAtEnd = bs.n_entries;
    }
    ramcrc_replay_table_destroy_host(hostTable);
    printf("index: %llu entries at the end, %llu objects read by hash; %d mismatches\n",
           static_cast<unsigned long long>(entriesAtEnd), static_cast<unsigned long long>(objectsRead), bad);
    return bad ? 1 : 0;
}
