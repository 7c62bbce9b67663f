// Recovery-segment partitioning (ramcrc_recovery_partition_device): k_part_heads,
// k_part_classify, k_part_void, k_part_tiles, k_part_scan, k_part_emit
// (DESIGN.md 5.9).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.
//
// The placement decision of RecoverySegmentBuilder::build
// (src/RecoverySegmentBuilder.cc:74-201) for every walked record; the per-record
// rules are partition_rules.h's, shared with the host form.  Six launches, none
// of which waits for another workgroup:
//   k_part_heads     finds every segment's run of the table (the walk keeps a
//                    segment's records contiguous; anything else is refused),
//                    counts its SEGHEADER records and notes the first, and
//                    checks the tablet list;
//   k_part_classify  one thread per record: reads its fields, hashes the key,
//                    looks the tablet up, tests liveness; writes the record's
//                    placement count and first partition, its hash, and the
//                    segment's flags and counters;
//   k_part_void      zeroes the counts of a segment that turned out to have a
//                    placed record without a header (rare: exits at once);
//   k_part_tiles     sums the counts of every tile of 1,024 records;
//   k_part_scan      one workgroup: exclusive sum of the tile sums, *d_n_place,
//                    and the per-segment status;
//   k_part_emit      per tile, an exclusive sum of its counts behind the tile's
//                    offset, and the placements.

namespace {

constexpr uint32_t kPartLdsTablets = 256;   // tablets staged in LDS (40 B each)
constexpr int kPartThreads = 256;
constexpr uint32_t kPartPer = 4;            // records per thread of a scan tile
constexpr uint32_t kPartTile = kPartThreads * kPartPer;
constexpr uint32_t kPartNone = 0xFFFFFFFFu;

struct PartDesc {
    uint64_t base;              // source segments
    uint64_t stride;
    uint64_t nseg;
    const ramcrc_seg_status* status;
    const u32x4* entries;       // {segment, offset, length, header}
    uint64_t ecap;
    const uint64_t* n_entries;
    const ramcrc_tablet* tablets;
    uint32_t ntab;
    uint32_t npart;
    uint2* place;               // {record, partition}
    uint64_t pcap;
    uint64_t* n_place;
    uint64_t* key_hash;         // nullable
    ramcrc_partition_status* pstat;
    // scratch
    uint32_t* refuse;           // nonzero: the call writes only *n_place = 0
    uint32_t* run_lo;           // [nseg] first record of the segment's run
    uint32_t* run_hi;           // [nseg] one past its last
    uint32_t* run_cnt;          // [nseg] runs found (more than one: refused)
    uint32_t* hdr_cnt;          // [nseg] SEGHEADER records
    uint32_t* hdr_first;        // [nseg] ~(index of the first one), by atomicMax
    uint32_t* sflags;           // [nseg] RAMCRC_SEG_NO_HEADER | RAMCRC_SEG_MALFORMED
    uint32_t* counts;           // [3 * nseg] placed, unplaced, dead
    uint64_t* cls;              // [ecap] placements of the record | first partition << 32
    uint64_t* tile_sum;         // [tiles] sum of a tile's counts, then its exclusive offset
    uint32_t* ctx_status;
};

__device__ __forceinline__ void part_refuse(const PartDesc& a)
{
    *a.refuse = 1u;
    atomicOr(a.ctx_status, kStatusSticky);
}

__device__ __forceinline__ uint64_t part_n_records(const PartDesc& a)
{
    const uint64_t nw = *a.n_entries;
    return nw < a.ecap ? nw : a.ecap;
}

// The n (1..8) bytes at addr, little-endian: the aligned 16-byte word that
// holds the first byte, and the next one only when the field crosses into it
// (it then holds a byte of the field, so both lie inside the segment).
__device__ __forceinline__ uint64_t part_bytes(uint64_t addr, uint32_t n)
{
    const uint64_t a = addr & ~15ull;
    const uint32_t sh = uint32_t(addr) & 15u;
    const u32x4 w = load16(a);
    uint64_t x0 = w.x | (uint64_t(w.y) << 32), x1 = w.z | (uint64_t(w.w) << 32), y0 = 0;
    if (sh + n > 16) {
        const u32x4 v = load16(a + 16);
        y0 = v.x | (uint64_t(v.y) << 32);
    }
    if (sh & 8u) {
        x0 = x1;
        x1 = y0;
    }
    const uint32_t s = (sh & 7u) * 8;
    const uint64_t v = s ? (x0 >> s) | (x1 << (64 - s)) : x0;
    return ramcrc::murmur_low_bytes(v, n);
}

struct PartRd {
    uint64_t pay;   // address of payload byte 0
    __device__ __forceinline__ uint32_t u8(uint32_t o) const { return uint32_t(part_bytes(pay + o, 1)); }
    __device__ __forceinline__ uint32_t u16(uint32_t o) const { return uint32_t(part_bytes(pay + o, 2)); }
    __device__ __forceinline__ uint32_t u32(uint32_t o) const { return uint32_t(part_bytes(pay + o, 4)); }
    __device__ __forceinline__ uint64_t u64(uint32_t o) const { return part_bytes(pay + o, 8); }
};

// Key::getHash of the len bytes at addr (any byte residue): aligned 16-byte
// loads, each block of the hash taken from two neighbouring words by a byte
// funnel shift.  A word is loaded only when it holds a key byte.
__device__ __forceinline__ uint64_t part_key_hash(uint64_t table_id, uint64_t addr, uint32_t len)
{
    ramcrc::Murmur3 m{uint32_t(table_id)};
    if (len == 0)
        return m.finish(0, 0, 0, 0);
    const uint64_t end = addr + len;
    const uint32_t sh = uint32_t(addr) & 15u, s = (sh & 7u) * 8;
    uint64_t pos = addr & ~15ull;
    u32x4 w = load16(pos);
    uint64_t x0 = w.x | (uint64_t(w.y) << 32), x1 = w.z | (uint64_t(w.w) << 32);
    uint32_t left = len;
    while (true) {
        pos += 16;
        uint64_t y0 = 0, y1 = 0;
        if (pos < end) {
            w = load16(pos);
            y0 = w.x | (uint64_t(w.y) << 32);
            y1 = w.z | (uint64_t(w.w) << 32);
        }
        const uint64_t a0 = (sh & 8u) ? x1 : x0, a1 = (sh & 8u) ? y0 : x1, a2 = (sh & 8u) ? y1 : y0;
        const uint64_t k1 = s ? (a0 >> s) | (a1 << (64 - s)) : a0;
        const uint64_t k2 = s ? (a1 >> s) | (a2 << (64 - s)) : a1;
        if (left < 16)
            return m.finish(ramcrc::murmur_low_bytes(k1, left < 8 ? left : 8u),
                            left > 8 ? ramcrc::murmur_low_bytes(k2, left - 8) : 0ull, left, len);
        m.block(k1, k2);
        left -= 16;
        if (left == 0)
            return m.finish(0, 0, 0, len);
        x0 = y0;
        x1 = y1;
    }
}

// Exclusive sum of v over the workgroup (kPartThreads threads) and its total.
__device__ __forceinline__ uint64_t part_block_excl(uint64_t v, uint64_t* wsum, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & (kWaveSize - 1), wv = threadIdx.x / kWaveSize;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < kWaveSize; d <<= 1) {
        const uint64_t o = __shfl_up(static_cast<unsigned long long>(inc), d);
        if (lane >= uint32_t(d))
            inc += o;
    }
    if (lane == kWaveSize - 1)
        wsum[wv] = inc;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPartThreads / kWaveSize; w++) {
        pre += w < wv ? wsum[w] : 0ull;
        tot += wsum[w];
    }
    __syncthreads();   // wsum is free again
    *total = tot;
    return pre + inc - v;
}

// ------------------------------------------------------------ k_part_heads
__global__ __launch_bounds__(kPartThreads) void k_part_heads(PartDesc a)
{
    const uint64_t ne = part_n_records(a);
    const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    if (tid == 0 && a.npart == 0)
        part_refuse(a);
    for (uint64_t t = tid; t < a.ntab; t += nthr)
        if (a.tablets[t].partition >= a.npart)
            part_refuse(a);
    for (uint64_t i = tid; i < ne; i += nthr) {
        const u32x4 r = a.entries[i];
        const uint32_t seg = r.x;
        if (seg >= a.nseg) {
            part_refuse(a);
            continue;
        }
        const bool first = i == 0 || a.entries[i - 1].x != seg;
        const bool last = i + 1 == ne || a.entries[i + 1].x != seg;
        if (first) {
            if (atomicAdd(&a.run_cnt[seg], 1u) != 0)
                part_refuse(a);   // a second run of this segment: the table is not a walk's
            a.run_lo[seg] = uint32_t(i);
        }
        if (last)
            a.run_hi[seg] = uint32_t(i + 1);
        if ((r.w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_SEGHEADER) {
            atomicAdd(&a.hdr_cnt[seg], 1u);
            atomicMax(&a.hdr_first[seg], ~uint32_t(i));
        }
    }
}

// --------------------------------------------------------- k_part_classify
// The segmentId of the SEGHEADER record that governs record i of segment seg
// (the latest one before it), or false when there is none it can read.  With
// one SEGHEADER in the segment (every log segment: it is the first record) the
// answer is k_part_heads'; with more, this lane walks back through the run.
__device__ __forceinline__ bool part_segment_id(const PartDesc& a, uint32_t seg, uint64_t i,
                                                uint64_t* seg_id)
{
    const uint32_t hc = a.hdr_cnt[seg];
    uint64_t h = ~0ull;
    if (hc == 1) {
        const uint32_t hf = ~a.hdr_first[seg];
        if (hf < i)
            h = hf;
    } else if (hc > 1) {
        const uint64_t lo = a.run_lo[seg];
        for (uint64_t j = i; j-- > lo;) {
            if ((a.entries[j].w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_SEGHEADER) {
                h = j;
                break;
            }
        }
    }
    if (h == ~0ull)
        return false;
    const u32x4 hr = a.entries[h];
    const uint64_t pay = uint64_t(hr.y) + 1 + ((hr.w >> 6) & 3) + 1;
    if ((hr.w & kRecOverlong) || hr.z < ramcrc_part::kSegHeaderBytes || pay + hr.z > a.stride)
        return false;
    *seg_id = part_bytes(a.base + uint64_t(seg) * a.stride + pay + ramcrc_part::kSegIdAt, 8);
    return true;
}

template <bool kLds>
__global__ __launch_bounds__(kPartThreads) void k_part_classify(PartDesc a)
{
    __shared__ ramcrc_tablet lt[kLds ? kPartLdsTablets : 1];
    if (*a.refuse)
        return;
    if constexpr (kLds) {
        for (uint32_t t = threadIdx.x; t < a.ntab; t += kPartThreads)
            lt[t] = a.tablets[t];
        __syncthreads();
    }
    auto tab = [&](uint32_t t) -> ramcrc_tablet {
        if constexpr (kLds)
            return lt[t];
        else
            return a.tablets[t];
    };
    const uint64_t ne = part_n_records(a);
    for (uint64_t i0 = uint64_t(blockIdx.x) * kPartThreads; i0 < ne;
         i0 += uint64_t(gridDim.x) * kPartThreads) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t seg = kPartNone, n = 0, part = 0, fl = 0, unplaced = 0, dead = 0;
        uint64_t hash = 0;
        if (i < ne) {
            const u32x4 r = a.entries[i];
            seg = r.x;   // < nseg: k_part_heads checked
            const uint32_t type = r.w & 0x3f;
            if ((a.status[seg].flags & RAMCRC_SEG_OK) && ramcrc_part::placed_type(type)) {
                const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
                const bool readable = !(r.w & kRecOverlong) && pay + r.z <= a.stride;
                const PartRd rd{a.base + uint64_t(seg) * a.stride + pay};
                const ramcrc_part::Parsed p = ramcrc_part::parse(type, r.z, readable, rd);
                if (p.kind == ramcrc_part::kMalformed) {
                    fl = RAMCRC_SEG_MALFORMED;
                } else {
                    uint64_t seg_id = 0;
                    const bool have = part_segment_id(a, seg, i, &seg_id);
                    if (!have)
                        fl = RAMCRC_SEG_NO_HEADER;
                    if (p.kind == ramcrc_part::kSafeVersion) {
                        n = a.npart;
                    } else if (p.kind == ramcrc_part::kPlist) {
                        for (uint32_t k = 0; k < p.count; k++) {
                            const uint32_t o = ramcrc_part::kPlistHeader + ramcrc_part::kPartyBytes * k;
                            const uint32_t t = ramcrc_part::which_tablet(rd.u64(o), rd.u64(o + 8),
                                                                         a.ntab, tab);
                            if (t != ramcrc_part::kNoTablet) {
                                if (n == 0)
                                    part = tab(t).partition;
                                n++;
                            }
                        }
                    } else {
                        hash = p.kind == ramcrc_part::kKeyed
                                   ? part_key_hash(p.table_id, rd.pay + p.key_off, p.key_len)
                                   : p.hash;
                        const uint32_t t = ramcrc_part::which_tablet(p.table_id, hash, a.ntab, tab);
                        if (t == ramcrc_part::kNoTablet) {
                            unplaced = 1;
                        } else if (have) {
                            const ramcrc_tablet tb = tab(t);
                            if (ramcrc_part::alive(seg_id, r.y, tb)) {
                                n = 1;
                                part = tb.partition;
                            } else {
                                dead = 1;
                            }
                        }
                    }
                    if (!have)
                        n = 0;
                }
            }
            a.cls[i] = uint64_t(n) | (uint64_t(part) << 32);
            if (a.key_hash)
                a.key_hash[i] = hash;
            if (fl)
                atomicOr(&a.sflags[seg], fl);
        }
        // the segment's counters: the lanes of the wave's first segment add up
        // and issue one atomic each, the others (a wave across a segment
        // boundary) their own
        const uint32_t lead = uint32_t(__builtin_amdgcn_readfirstlane(seg));
        const bool same = seg == lead && lead != kPartNone;
        const uint32_t nu = uint32_t(__builtin_popcountll(__ballot(same && unplaced)));
        const uint32_t nd = uint32_t(__builtin_popcountll(__ballot(same && dead)));
        uint32_t np = same ? n : 0u;
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            np += __shfl_xor(np, d);
        if ((threadIdx.x & (kWaveSize - 1)) == 0 && lead != kPartNone) {
            if (np)
                atomicAdd(&a.counts[3 * uint64_t(lead)], np);
            if (nu)
                atomicAdd(&a.counts[3 * uint64_t(lead) + 1], nu);
            if (nd)
                atomicAdd(&a.counts[3 * uint64_t(lead) + 2], nd);
        }
        if (!same && seg != kPartNone) {
            if (n)
                atomicAdd(&a.counts[3 * uint64_t(seg)], n);
            if (unplaced)
                atomicAdd(&a.counts[3 * uint64_t(seg) + 1], 1u);
            if (dead)
                atomicAdd(&a.counts[3 * uint64_t(seg) + 2], 1u);
        }
    }
}

// ------------------------------------------------------------- k_part_void
// A wave per segment: a segment flagged RAMCRC_SEG_NO_HEADER places nothing.
__global__ __launch_bounds__(kWaveSize) void k_part_void(PartDesc a)
{
    if (*a.refuse)
        return;
    for (uint64_t s = blockIdx.x; s < a.nseg; s += gridDim.x) {
        if (!(a.sflags[s] & RAMCRC_SEG_NO_HEADER) || !a.run_cnt[s])
            continue;
        const uint64_t lo = a.run_lo[s], hi = a.run_hi[s];
        for (uint64_t i = lo + threadIdx.x; i < hi; i += kWaveSize)
            a.cls[i] = 0;
    }
}

// ------------------------------------------------------------ k_part_tiles
__global__ __launch_bounds__(kPartThreads) void k_part_tiles(PartDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse)
        return;
    const uint64_t ne = part_n_records(a);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        uint64_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++)
            v += i0 + k < ne ? uint32_t(a.cls[i0 + k]) : 0u;
        uint64_t tot;
        (void)part_block_excl(v, wsum, &tot);
        if (threadIdx.x == 0)
            a.tile_sum[tile] = tot;
    }
}

// ------------------------------------------------------------- k_part_scan
// One workgroup: the tile sums become exclusive offsets, kPartThreads tiles a
// step; then the list's length and the per-segment status.
__global__ __launch_bounds__(kPartThreads) void k_part_scan(PartDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse) {
        if (threadIdx.x == 0)
            *a.n_place = 0;
        return;
    }
    const uint64_t ne = part_n_records(a);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPartThreads) {
        const uint64_t t = t0 + threadIdx.x;
        const uint64_t v = t < ntiles ? a.tile_sum[t] : 0ull;
        uint64_t tot;
        const uint64_t ex = part_block_excl(v, wsum, &tot);
        if (t < ntiles)
            a.tile_sum[t] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0)
        *a.n_place = carry;
    for (uint64_t s = threadIdx.x; s < a.nseg; s += kPartThreads) {
        const uint32_t fl = a.sflags[s];
        ramcrc_partition_status st{RAMCRC_SEG_SOURCE_BAD, 0u, 0u, 0u};
        if (a.status[s].flags & RAMCRC_SEG_OK) {
            if (fl & RAMCRC_SEG_NO_HEADER)
                st.flags = RAMCRC_SEG_NO_HEADER | (fl & RAMCRC_SEG_MALFORMED);
            else
                st = ramcrc_partition_status{RAMCRC_SEG_OK | fl, a.counts[3 * s], a.counts[3 * s + 1],
                                             a.counts[3 * s + 2]};
        }
        a.pstat[s] = st;
    }
}

// ------------------------------------------------------------- k_part_emit
__global__ __launch_bounds__(kPartThreads) void k_part_emit(PartDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse)
        return;
    const uint64_t ne = part_n_records(a);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    auto tab = [&](uint32_t t) -> ramcrc_tablet { return a.tablets[t]; };
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        uint64_t c[kPartPer], v = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            c[k] = i0 + k < ne ? a.cls[i0 + k] : 0ull;
            v += uint32_t(c[k]);
        }
        uint64_t tot;
        uint64_t dst = a.tile_sum[tile] + part_block_excl(v, wsum, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            const uint32_t n = uint32_t(c[k]), rec = uint32_t(i0 + k);
            if (n == 1) {
                if (dst < a.pcap)
                    a.place[dst] = make_uint2(rec, uint32_t(c[k] >> 32));
            } else if (n > 1) {
                // a safe version (every partition) or a participant list (its
                // owned participants, looked up again)
                const u32x4 r = a.entries[rec];
                if ((r.w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION) {
                    for (uint32_t p = 0; p < n; p++)
                        if (dst + p < a.pcap)
                            a.place[dst + p] = make_uint2(rec, p);
                } else {
                    const PartRd rd{a.base + uint64_t(r.x) * a.stride + r.y + 1 + ((r.w >> 6) & 3) + 1};
                    const uint32_t count = rd.u32(ramcrc_part::kPlistCountAt);
                    uint32_t m = 0;
                    for (uint32_t q = 0; q < count && m < n; q++) {
                        const uint32_t o = ramcrc_part::kPlistHeader + ramcrc_part::kPartyBytes * q;
                        const uint32_t t = ramcrc_part::which_tablet(rd.u64(o), rd.u64(o + 8), a.ntab, tab);
                        if (t == ramcrc_part::kNoTablet)
                            continue;
                        if (dst + m < a.pcap)
                            a.place[dst + m] = make_uint2(rec, a.tablets[t].partition);
                        m++;
                    }
                }
            }
            dst += n;
        }
    }
}

}  // namespace
