// Crc32CBatch::deviceRecoveryAppend as a backup would call it after
// deviceReplayVerify: three replicas of object entries (one with a wrong
// certificate), every record placed in partition (index % 2) and every fifth
// one in both, appended into 3 x 2 recovery segments.  The expected bytes and
// certificates are built here with the drop-in Crc32C, the way
// Segment::append and Segment::getAppendedLength build them
// (src/Segment.cc:197-228, :672-684).  Built with hipcc for hipMalloc.
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <vector>

#include "Crc32C.h"
#include "Crc32CBatch.h"

using namespace RAMCloud;

static const uint32_t kCap = 64 * 1024;
static const uint32_t kOutCap = 48 * 1024;
static const uint32_t kSeg = 3, kPart = 2;

// Fills `seg` with n objects of valueLen bytes, every entry with 2 length
// bytes (not minimal for the short ones); returns the certificate.
static ramcrc_seg_cert fill(uint8_t* seg, int n, uint32_t valueLen, uint32_t seed)
{
    Crc32C meta;
    uint32_t pos = 0;
    for (int k = 0; k < n; k++) {
        const uint32_t len = 24 + valueLen + (k % 3 == 0 ? 0 : 300);
        seg[pos] = 2 | (1 << 6);                      // LOG_ENTRY_TYPE_OBJ, 2 length bytes
        seg[pos + 1] = uint8_t(len);
        seg[pos + 2] = uint8_t(len >> 8);
        meta.update(&seg[pos], 3);
        uint8_t* obj = &seg[pos + 3];
        for (uint32_t i = 4; i < len; i++) {
            seed = seed * 1103515245u + 12345u;
            obj[i] = uint8_t(seed >> 16);
        }
        const uint32_t c = Crc32C().update(obj + 4, len - 4).getResult();
        memcpy(obj, &c, 4);
        pos += 3 + len;
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
    certs[0] = fill(&host[0], 60, 100, 7);
    certs[1] = fill(&host[kCap], 45, 700, 9);
    certs[2] = fill(&host[2 * kCap], 50, 40, 11);
    certs[1].checksum ^= 1;        // replica 1 fails its metadata check
    const uint64_t cap = 256, pcap = 512;
    const uint64_t outBytes = uint64_t(kSeg) * kPart * kOutCap;
    void *d_base, *d_certs, *d_status, *d_entries, *d_n, *d_crc, *d_place, *d_np, *d_out, *d_oc,
        *d_os;
    HIP(hipMalloc(&d_base, host.size()));
    HIP(hipMalloc(&d_certs, sizeof certs));
    HIP(hipMalloc(&d_status, kSeg * sizeof(ramcrc_seg_status)));
    HIP(hipMalloc(&d_entries, cap * sizeof(ramcrc_seg_entry)));
    HIP(hipMalloc(&d_n, 8));
    HIP(hipMalloc(&d_crc, cap * 4));
    HIP(hipMalloc(&d_place, pcap * sizeof(ramcrc_placement)));
    HIP(hipMalloc(&d_np, 8));
    HIP(hipMalloc(&d_out, outBytes));
    HIP(hipMalloc(&d_oc, kSeg * kPart * sizeof(ramcrc_seg_cert)));
    HIP(hipMalloc(&d_os, kSeg * kPart * sizeof(ramcrc_append_status)));
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
    if (n != 155 || n > cap) {
        fprintf(stderr, "walk found %llu records\n", static_cast<unsigned long long>(n));
        return 1;
    }
    std::vector<ramcrc_seg_entry> table(n);
    ramcrc_seg_status st[kSeg];
    HIP(hipMemcpy(&table[0], d_entries, n * sizeof(ramcrc_seg_entry), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(st, d_status, sizeof st, hipMemcpyDeviceToHost));

    // the caller's partitioner
    std::vector<ramcrc_placement> place;
    for (uint32_t r = 0; r < n; r++) {
        ramcrc_placement p = {r, r % kPart};
        place.push_back(p);
        if (r % 5 == 0) {
            p.partition ^= 1;
            place.push_back(p);
        }
    }
    const uint64_t np = place.size();
    HIP(hipMemcpy(d_place, &place[0], np * sizeof(ramcrc_placement), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_np, &np, 8, hipMemcpyHostToDevice));
    batch.deviceRecoveryAppend(d_base, kCap, kSeg, static_cast<ramcrc_seg_status*>(d_status),
                               static_cast<ramcrc_seg_entry*>(d_entries), cap,
                               static_cast<uint64_t*>(d_n),
                               static_cast<ramcrc_placement*>(d_place), pcap,
                               static_cast<uint64_t*>(d_np), kPart, d_out, kOutCap, kOutCap,
                               static_cast<ramcrc_seg_cert*>(d_oc),
                               static_cast<ramcrc_append_status*>(d_os));
    std::vector<uint8_t> out(outBytes);
    ramcrc_seg_cert oc[kSeg * kPart];
    ramcrc_append_status os[kSeg * kPart];
    HIP(hipMemcpy(&out[0], d_out, outBytes, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(oc, d_oc, sizeof oc, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(os, d_os, sizeof os, hipMemcpyDeviceToHost));

    // Segment::append per placement, on the host
    std::vector<std::vector<uint8_t> > want(kSeg * kPart);
    std::vector<Crc32C> meta(kSeg * kPart);
    uint32_t count[kSeg * kPart] = {};
    for (size_t i = 0; i < place.size(); i++) {
        const ramcrc_seg_entry& e = table[place[i].record];
        if (!(st[e.segment].flags & RAMCRC_SEG_OK))
            continue;
        const uint32_t k = e.segment * kPart + place[i].partition;
        const uint32_t lb = e.length < 256 ? 1 : 2;
        uint8_t hdr[3] = {uint8_t((e.header & 0x3f) | ((lb - 1) << 6)), uint8_t(e.length),
                          uint8_t(e.length >> 8)};
        meta[k].update(hdr, 1 + lb);
        want[k].insert(want[k].end(), hdr, hdr + 1 + lb);
        const uint8_t* p = &host[e.segment * kCap + e.offset + 1 + ((e.header >> 6) & 3) + 1];
        want[k].insert(want[k].end(), p, p + e.length);
        count[k]++;
    }
    int bad = 0;
    for (uint32_t k = 0; k < kSeg * kPart; k++) {
        const uint32_t head = uint32_t(want[k].size());
        meta[k].update(&head, 4);
        const bool source_ok = (st[k / kPart].flags & RAMCRC_SEG_OK) != 0;
        const uint8_t* o = &out[uint64_t(k) * kOutCap];
        int b = 0;
        b += oc[k].segment_length != head || oc[k].checksum != meta[k].getResult();
        b += os[k].flags != (source_ok ? RAMCRC_SEG_OK : RAMCRC_SEG_SOURCE_BAD);
        b += os[k].entries != count[k] || (source_ok && count[k] == 0);
        b += head && memcmp(o, &want[k][0], head) != 0;
        for (uint32_t j = head; j < kOutCap; j++)
            b += o[j] != 0xA5;
        if (b)
            printf("output %u: head %u (want %u) flags %u entries %u (want %u)\n", k,
                   oc[k].segment_length, head, os[k].flags, os[k].entries, count[k]);
        bad += b != 0;
    }
    bad += (st[1].flags & RAMCRC_SEG_OK) != 0;   // the damaged replica
    printf("recovery append: %llu placements into %u segments; %d mismatches\n",
           static_cast<unsigned long long>(np), kSeg * kPart, bad);
    return bad ? 1 : 0;
}
