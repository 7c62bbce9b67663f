// Crc32CBatch::deviceReplaySideLog as a recovery master would call it after
// deviceReplayVerify: two replicas of objects, tombstones (one with a wrong
// stored checksum) and a safe version, every record but each seventh kept.
// The expected bytes are built here with the drop-in Crc32C: Segment::append
// per kept record (src/Segment.cc:197-228), every tombstone rewritten as
// ObjectManager::replaySegment rewrites it (src/ObjectManager.cc:845-851).
// Built with hipcc for hipMalloc.
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <vector>

#include "Crc32C.h"
#include "Crc32CBatch.h"

using namespace RAMCloud;

static const uint32_t kCap = 64 * 1024;
static const uint32_t kOutCap = 8 * 1024;   // the second replica's side log fills up
static const uint32_t kSeg = 2;
static const uint32_t kTime = 0x65A1B2C3u;

static uint32_t g_seed = 5;
static uint8_t rnd()
{
    g_seed = g_seed * 1103515245u + 12345u;
    return uint8_t(g_seed >> 16);
}

// ObjectTombstone::computeChecksum (src/Object.cc:1042-1057)
static uint32_t tombChecksum(const uint8_t* t, uint32_t len)
{
    return Crc32C().update(t, 28).update(t + 32, len - 32).getResult();
}

// Fills `seg` with n records: objects, tombstones of 0 .. 299 key bytes, one
// safe version; returns the certificate.
static ramcrc_seg_cert fill(uint8_t* seg, int n)
{
    Crc32C meta;
    uint32_t pos = 0;
    for (int k = 0; k < n; k++) {
        const uint32_t type = k == 3 ? 5 : (k % 2 ? 3 : 2);
        const uint32_t len = type == 5 ? 12 : type == 3 ? 32 + (k * 37) % 300 : 24 + (k * 53) % 400;
        const uint32_t lb = len < 256 ? 1 : 2;
        seg[pos] = uint8_t(type | ((lb - 1) << 6));
        seg[pos + 1] = uint8_t(len);
        if (lb == 2)
            seg[pos + 2] = uint8_t(len >> 8);
        meta.update(&seg[pos], 1 + lb);
        uint8_t* p = &seg[pos + 1 + lb];
        for (uint32_t i = 0; i < len; i++)
            p[i] = rnd();
        uint32_t c;
        if (type == 2) {
            c = Crc32C().update(p + 4, len - 4).getResult();
            memcpy(p, &c, 4);
        } else if (type == 3) {
            c = tombChecksum(p, len) ^ (k == 5 ? 0x10u : 0u);   // record 5: a wrong stored checksum
            memcpy(p + 28, &c, 4);
        } else {
            c = Crc32C().update(p, 8).getResult();
            memcpy(p + 8, &c, 4);
        }
        pos += 1 + lb + len;
    }
    ramcrc_seg_cert cert;
    cert.segment_length = pos;
    meta.update(&pos, 4);
    cert.checksum = meta.getResult();
    return cert;
}

#define HIP(expr)                                                \
    do {                                                         \
        if ((expr) != hipSuccess) {                              \
            fprintf(stderr, "%s failed\n", #expr);               \
            return 1;                                            \
        }                                                        \
    } while (0)

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
    certs[0] = fill(&host[0], 30);
    certs[1] = fill(&host[kCap], 70);
    const uint64_t cap = 128, lcap = 128;
    const uint64_t outBytes = uint64_t(kSeg) * kOutCap;
    void *d_base, *d_certs, *d_status, *d_entries, *d_n, *d_crc, *d_live, *d_nl, *d_out, *d_oc, *d_os,
        *d_refs, *d_counts;
    HIP(hipMalloc(&d_base, host.size()));
    HIP(hipMalloc(&d_certs, sizeof certs));
    HIP(hipMalloc(&d_status, kSeg * sizeof(ramcrc_seg_status)));
    HIP(hipMalloc(&d_entries, cap * sizeof(ramcrc_seg_entry)));
    HIP(hipMalloc(&d_n, 8));
    HIP(hipMalloc(&d_crc, cap * 4));
    HIP(hipMalloc(&d_live, lcap * sizeof(ramcrc_placement)));
    HIP(hipMalloc(&d_nl, 8));
    HIP(hipMalloc(&d_out, outBytes));
    HIP(hipMalloc(&d_oc, kSeg * sizeof(ramcrc_seg_cert)));
    HIP(hipMalloc(&d_os, kSeg * sizeof(ramcrc_append_status)));
    HIP(hipMalloc(&d_refs, lcap * sizeof(ramcrc_log_ref)));
    HIP(hipMalloc(&d_counts, sizeof(ramcrc_sidelog_counts)));
    HIP(hipMemcpy(d_base, &host[0], host.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_certs, certs, sizeof certs, hipMemcpyHostToDevice));
    HIP(hipMemset(d_out, 0xA5, outBytes));
    Crc32CBatch batch(0);
    batch.deviceReplayVerify(d_base, kCap, kCap, kSeg, static_cast<ramcrc_seg_cert*>(d_certs),
                             static_cast<ramcrc_seg_status*>(d_status),
                             static_cast<ramcrc_seg_entry*>(d_entries), cap,
                             static_cast<uint64_t*>(d_n), static_cast<uint32_t*>(d_crc));
    uint64_t n = 0;
    HIP(hipMemcpy(&n, d_n, 8, hipMemcpyDeviceToHost));
    if (n != 100 || n > cap) {
        fprintf(stderr, "walk found %llu records\n", static_cast<unsigned long long>(n));
        return 1;
    }
    std::vector<ramcrc_seg_entry> table(n);
    ramcrc_seg_status st[kSeg];
    HIP(hipMemcpy(&table[0], d_entries, n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(st, d_status, sizeof st, hipMemcpyDeviceToHost));
    if (st[0].bad_objects + st[1].bad_objects != 2) {   // record 5 of each replica
        fprintf(stderr, "replay verify: %u bad records\n", st[0].bad_objects + st[1].bad_objects);
        return 1;
    }

    std::vector<ramcrc_placement> live;
    for (uint32_t r = 0; r < n; r++) {
        if (r % 7 != 6) {
            ramcrc_placement p = {r, 0};
            live.push_back(p);
        }
    }
    const uint64_t nl = live.size();
    HIP(hipMemcpy(d_live, &live[0], nl * sizeof(ramcrc_placement), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_nl, &nl, 8, hipMemcpyHostToDevice));
    batch.deviceReplaySideLog(d_base, kCap, kSeg, static_cast<ramcrc_seg_status*>(d_status),
                              static_cast<ramcrc_seg_entry*>(d_entries), cap,
                              static_cast<uint64_t*>(d_n), static_cast<ramcrc_placement*>(d_live),
                              lcap, static_cast<uint64_t*>(d_nl), kTime, d_out, kOutCap, kOutCap,
                              static_cast<ramcrc_seg_cert*>(d_oc),
                              static_cast<ramcrc_append_status*>(d_os),
                              static_cast<ramcrc_log_ref*>(d_refs),
                              static_cast<ramcrc_sidelog_counts*>(d_counts));
    std::vector<uint8_t> out(outBytes);
    std::vector<ramcrc_log_ref> refs(nl);
    ramcrc_seg_cert oc[kSeg];
    ramcrc_append_status os[kSeg];
    ramcrc_sidelog_counts counts;
    HIP(hipMemcpy(&out[0], d_out, outBytes, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&refs[0], d_refs, nl * sizeof(ramcrc_log_ref), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(oc, d_oc, sizeof oc, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(os, d_os, sizeof os, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(&counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));

    // sideLog->append per kept record, on the host
    std::vector<std::vector<uint8_t> > want(kSeg);
    std::vector<Crc32C> meta(kSeg);
    uint32_t count[kSeg] = {};
    bool full[kSeg] = {};
    ramcrc_sidelog_counts wc;
    memset(&wc, 0, sizeof wc);
    int bad = 0;
    for (size_t i = 0; i < live.size(); i++) {
        const ramcrc_seg_entry& e = table[live[i].record];
        const uint32_t k = e.segment;
        const uint32_t lb = e.length < 256 ? 1 : 2;
        if (full[k] || want[k].size() + 1 + lb + e.length > kOutCap) {
            full[k] = true;
            wc.left_out++;
            bad += refs[i].segment != RAMCRC_LOG_REF_NONE || refs[i].offset != RAMCRC_LOG_REF_NONE;
            continue;
        }
        bad += refs[i].segment != k || refs[i].offset != want[k].size();
        uint8_t hdr[3] = {uint8_t((e.header & 0x3f) | ((lb - 1) << 6)), uint8_t(e.length),
                          uint8_t(e.length >> 8)};
        meta[k].update(hdr, 1 + lb);
        want[k].insert(want[k].end(), hdr, hdr + 1 + lb);
        const uint8_t* p = &host[e.segment * kCap + e.offset + 1 + ((e.header >> 6) & 3) + 1];
        const size_t at = want[k].size();
        want[k].insert(want[k].end(), p, p + e.length);
        count[k]++;
        const uint32_t type = e.header & 0x3f;
        if (type == 2) {
            wc.objects++;
            wc.object_bytes += e.length;
        } else if (type == 3) {
            wc.tombstones++;
            wc.tombstone_bytes += e.length;
            uint8_t* t = &want[k][at];
            memset(t + 8, 0, 8);                      // segmentId = 0
            memcpy(t + 24, &kTime, 4);                // timestamp
            const uint32_t c = tombChecksum(t, e.length);
            memcpy(t + 28, &c, 4);
        } else {
            wc.other++;
        }
    }
    for (uint32_t k = 0; k < kSeg; k++) {
        const uint32_t head = uint32_t(want[k].size());
        meta[k].update(&head, 4);
        const uint8_t* o = &out[uint64_t(k) * kOutCap];
        int b = 0;
        b += oc[k].segment_length != head || oc[k].checksum != meta[k].getResult();
        b += os[k].flags != (full[k] ? RAMCRC_SEG_APPEND_FULL : RAMCRC_SEG_OK);
        b += os[k].entries != count[k] || count[k] == 0;
        b += head && memcmp(o, &want[k][0], head) != 0;
        for (uint32_t j = head; j < kOutCap; j++)
            b += o[j] != 0xA5;
        if (b)
            printf("side log %u: head %u (want %u) flags %u entries %u (want %u)\n", k,
                   oc[k].segment_length, head, os[k].flags, os[k].entries, count[k]);
        bad += b != 0;
    }
    bad += memcmp(&counts, &wc, sizeof wc) != 0;
    bad += !full[1] || full[0] || wc.tombstones < 20 || wc.other != 2;
    printf("replay side log: %llu kept records, %llu tombstones rewritten, %llu left out; "
           "%d mismatches\n", static_cast<unsigned long long>(nl),
           static_cast<unsigned long long>(counts.tombstones),
           static_cast<unsigned long long>(counts.left_out), bad);
    return bad ? 1 : 0;
}
