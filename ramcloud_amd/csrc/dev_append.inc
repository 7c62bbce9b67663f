// Recovery-segment append (ramcrc_recovery_append_device): k_app_mark,
// k_app_scan, k_app_copy (DESIGN.md 5.8).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.
//
// A placement {record, partition} appends one walked record to output
// (source segment of the record, partition) as Segment::append writes it
// (src/Segment.cc:197-228).  Three launches:
//   k_app_mark  checks the list (the refusal word the other two test before
//               they write anything) and finds every source segment's run of
//               the list -- the walk keeps a segment's records contiguous, so
//               a non-decreasing list visits each segment once;
//   k_app_scan  up to 8 waves per source segment, each owning a share of
//               the partitions, step through its run 64 placements of their
//               partitions at a time: a stable exclusive sum of the appended
//               sizes keyed by partition gives every placement its offset in
//               its output (carried from step to step in a per-partition
//               state), the fit rule falls out of it, and the same step folds
//               the 2..5 metadata bytes of the entries that fit into the
//               output's running checksum with the X^n algebra of gf2.h.  At
//               the end of the run it seals the certificates;
//   k_app_copy  the payload bytes, read once and written once.

namespace {

constexpr uint32_t kAppLdsParts = 512;        // partitions whose scan state fits a wave's LDS
constexpr uint32_t kAppNone = 0xFFFFFFFFu;    // pdst: the placement is not appended
constexpr uint64_t kAppNoFit = 1ull << 33;    // size of a record that can never be appended
constexpr int kAppMetaShift = 44;             // scan value: size in bits 0..43, metadata bytes above
constexpr uint64_t kAppSizeMask = (1ull << kAppMetaShift) - 1;
constexpr uint32_t kAppFull = 0x80000000u;    // AppState::cnt: a placement did not fit
constexpr uint32_t kAppShortMax = 256;        // payload bytes up to which 8 lanes copy in one short pass
constexpr uint32_t kAppBigMin = 2048;         // payload bytes from which a whole wave copies
constexpr uint32_t kAppGroupMin = 64 * 1024;  // payload bytes from which the whole workgroup copies
constexpr int kAppCopyThreads = 256;

// Running state of one output while its source segment's run is scanned.
struct alignas(16) AppState {
    unsigned long long bytes;   // head: bytes appended so far
    uint32_t crc;               // running metadata checksum (raw, as Crc32C::result)
    uint32_t cnt;               // entries appended | kAppFull
};

struct AppDesc {
    uint64_t base;              // source segments
    uint64_t stride;
    uint64_t nseg;
    const ramcrc_seg_status* status;
    const u32x4* entries;       // {segment, offset, length, header}
    uint64_t ecap;
    const uint64_t* n_entries;
    const uint2* place;         // {record, partition}
    uint64_t pcap;
    const uint64_t* n_place;
    uint32_t npart;
    uint32_t ocap;
    uint64_t out;
    uint64_t ostride;
    ramcrc_seg_cert* certs;
    ramcrc_append_status* ostat;
    // scratch
    uint32_t* refuse;           // nonzero: the call writes nothing
    uint32_t* run_lo;           // [nseg] first placement of the segment's run
    uint32_t* run_hi;           // [nseg] one past its last
    uint32_t* run_cnt;          // [nseg] runs found (more than one: refused)
    uint32_t* pdst;             // [pcap] offset of the placement in its output, or kAppNone
    AppState* states;           // [nseg * npart] when npart > kAppLdsParts
    uint32_t nown;              // k_app_scan: waves per source segment (1, 2, 4 or 8)
    uint32_t* ctx_status;
};

__device__ __forceinline__ uint32_t app_len_bytes(uint32_t len)
{
    // the EntryHeader constructor's choice (src/Segment.h:134-149)
    return len < 0x100u ? 1u : len < 0x10000u ? 2u : len < 0x1000000u ? 3u : 4u;
}

__device__ __forceinline__ void app_refuse(const AppDesc& a)
{
    *a.refuse = 1u;
    atomicOr(a.ctx_status, kStatusSticky);
}

// ------------------------------------------------------------ k_app_mark
__global__ __launch_bounds__(256) void k_app_mark(AppDesc a)
{
    const uint64_t np = *a.n_place;
    const uint64_t nw = *a.n_entries;
    const uint64_t ne = nw < a.ecap ? nw : a.ecap;
    const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (np > a.pcap) {
        if (tid == 0)
            app_refuse(a);
        return;
    }
    for (uint64_t i = tid; i < np; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint2 pl = a.place[i];
        bool ok = pl.x < ne && pl.y < a.npart;
        uint32_t seg = 0;
        if (ok) {
            seg = a.entries[pl.x].x;
            ok = seg < a.nseg;
        }
        bool first = i == 0, last = i + 1 == np;
        if (ok && !first) {
            const uint32_t pr = a.place[i - 1].x;   // <= pl.x < ne when the list is in order
            ok = pr <= pl.x;
            if (ok)
                first = a.entries[pr].x != seg;
        }
        if (ok && !last) {
            const uint32_t nx = a.place[i + 1].x;
            last = nx >= ne || a.entries[nx].x != seg;   // (an index past the table: refused by its thread)
        }
        if (!ok) {
            app_refuse(a);
            continue;
        }
        if (first) {
            if (atomicAdd(&a.run_cnt[seg], 1u) != 0)
                app_refuse(a);   // a second run of this segment: the table is not a walk's
            a.run_lo[seg] = uint32_t(i);
        }
        if (last)
            a.run_hi[seg] = uint32_t(i + 1);
    }
}

// ------------------------------------------------------------ k_app_scan
// nown waves per source segment (1, 2, 4 or 8: enough to fill the device when
// the batch has few segments); wave w owns the partitions p with p % nown == w,
// reads the segment's whole run of the list and queues the placements of its
// partitions, so every output's state has one owner and no wave waits for
// another.  Every step takes 64 queued placements, one
// per lane, and exchanges them through LDS twice; each exchange is a loop over
// the 64 posted slots (broadcast reads), so a step costs the same for any
// number of partitions.
//   1. lane posts {partition, size | metadata bytes << 44}; the sum over the
//      lower lanes of its partition is its offset behind the output's head
//      (and its metadata offset).  A lane fits when the output is not full and
//      head + offset + size stays within the capacity; sizes only add up, so
//      the lanes that fit are a prefix of the partition's lanes.
//   2. a lane that fits posts its size, metadata bytes, a count of one, and
//      its metadata checksum moved back to the start of the step's metadata,
//          v_i = x^(-8 (metadata offset_i + m_i)) * raw(0, meta_i);
//      the sums and the XOR over its partition's slots are the step's totals.
//      The first lane of each partition moves the output's state on:
//          crc <- x^(8 M) * (crc ^ XOR_i v_i),    M = the step's metadata bytes
//      which is raw(s, A||B) = X^|B|(raw(s, A)) ^ raw(0, B) with every entry's
//      X^(bytes behind it) factored into x^(8 M) * x^(-8 (offset + m)).
// Two GF(2) multiplies per lane and step, none per partition.  The states live
// in LDS for up to kAppLdsParts partitions (kLds), else in the context's
// scratch.
constexpr int kAppCountShift = 54;   // exchange 2: entries that fit, above 10 bits of metadata bytes

template <bool kLds>
__global__ __launch_bounds__(kWaveSize) void k_app_scan(AppDesc a)
{
    __shared__ AppState lst[kLds ? kAppLdsParts : 1];
    __shared__ uint4 xs[kWaveSize];
    __shared__ uint4 q[2 * kWaveSize];        // queued placements: {index, partition, offset, length}
    __shared__ uint32_t qw[2 * kWaveSize];    // and their record headers
    __shared__ uint32_t t0[256];
    __shared__ uint32_t xm[5 * 64 + 1], xi[5 * 64 + 1];
    if (*a.refuse)
        return;
    const int lane = threadIdx.x;
    for (uint32_t t = lane; t < 256; t += kWaveSize)
        t0[t] = g_tab.t0.t[t];
    for (uint32_t t = lane; t <= 5 * 64; t += kWaveSize) {
        xm[t] = g_tab.xmeta[t];
        xi[t] = g_tab.xinv[t];
    }
    __syncthreads();
    // One wave: its LDS operations execute in program order, so a lane reads
    // what another lane stored by an earlier instruction.  This only keeps the
    // compiler from moving memory operations across the exchange; states in
    // global memory take a real fence.
    auto wsync = [&]() {
        if constexpr (kLds) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            __threadfence_block();
        }
    };

    const uint32_t W = a.nown;   // waves per source segment: a power of two
    for (uint64_t blk = blockIdx.x; blk < a.nseg * W; blk += gridDim.x) {
        const uint64_t s = blk / W;
        const uint32_t w = uint32_t(blk % W);   // this wave owns the partitions p with p % W == w
        AppState* const gst = kLds ? nullptr : a.states + s * a.npart;
        auto st_load = [&](uint32_t p) -> AppState {
            if constexpr (kLds)
                return lst[p];
            else
                return gst[p];
        };
        auto st_store = [&](uint32_t p, const AppState& v) {
            if constexpr (kLds)
                lst[p] = v;
            else
                gst[p] = v;
        };
        for (uint64_t p = w + uint64_t(W) * lane; p < a.npart; p += uint64_t(W) * kWaveSize)
            st_store(uint32_t(p), AppState{0ull, 0xFFFFFFFFu, 0u});   // head 0, a fresh Crc32C
        const bool good = (a.status[s].flags & RAMCRC_SEG_OK) != 0;
        uint64_t lo = 0, hi = 0;
        if (a.run_cnt[s]) {
            lo = a.run_lo[s];
            hi = a.run_hi[s];
        }
        if (hi < lo)
            hi = lo;
        if (!good) {
            // Segment::checkMetadataIntegrity failed: build throws before its loop
            if (w == 0)
                for (uint64_t i = lo + lane; i < hi; i += kWaveSize)
                    a.pdst[i] = kAppNone;
            lo = hi;
        }
        wsync();
        // The wave reads the whole run, 64 placements at a time, and queues
        // those of its partitions (with their records) in a ring of 128 slots;
        // a step takes the first 64 queued, or what is left at the end.
        uint32_t qh = 0, qn = 0;
        uint64_t i0 = lo;
        uint2 pl_n = make_uint2(0u, 0u);
        if (lo + lane < hi)
            pl_n = a.place[lo + lane];
        while (true) {
            while (i0 < hi && qn < kWaveSize) {
                const uint64_t i = i0 + lane;
                const uint2 cur = pl_n;
                if (i + kWaveSize < hi)
                    pl_n = a.place[i + kWaveSize];   // the next 64, in flight during these
                const bool own = i < hi && (cur.y & (W - 1)) == w;
                const uint64_t m = __ballot(own);
                if (own) {
                    const u32x4 r = a.entries[cur.x];
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi(
                        uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                    const uint32_t slot = (qh + qn + below) & (2 * kWaveSize - 1);
                    q[slot] = make_uint4(uint32_t(i), cur.y, r.y, r.z);
                    qw[slot] = r.w;
                }
                qn += uint32_t(__builtin_popcountll(m));
                i0 += kWaveSize;
            }
            if (qn == 0)
                break;
            wsync();
            const uint32_t nq = qn < uint32_t(kWaveSize) ? qn : uint32_t(kWaveSize);
            const bool valid = uint32_t(lane) < nq;
            const uint4 it = q[(qh + lane) & (2 * kWaveSize - 1)];
            const uint32_t hdr = qw[(qh + lane) & (2 * kWaveSize - 1)];
            qh = (qh + nq) & (2 * kWaveSize - 1);
            qn -= nq;
            const uint32_t part = valid ? it.y : 0xFFFFFFFFu;   // (no partition: npart <= 2^32 - 1)
            AppState S{0ull, 0u, 0u};
            if (valid)
                S = st_load(part);
            const uint32_t len = it.w, lb = app_len_bytes(len), mi = 1 + lb;
            const uint64_t srcoff = uint64_t(it.z) + 1 + ((hdr >> 6) & 3) + 1;
            const bool readable = !(hdr & kRecOverlong) && srcoff + len <= a.stride;
            const uint64_t size = readable ? uint64_t(mi) + len : kAppNoFit;
            const uint64_t packed = valid ? (size | (uint64_t(mi) << kAppMetaShift)) : 0ull;

            xs[lane] = make_uint4(part, 0u, uint32_t(packed), uint32_t(packed >> 32));
            wsync();
            uint64_t excl = 0;
            uint32_t nsame = 0;
#pragma unroll 16
            for (int j = 0; j < kWaveSize; j++) {
                const uint4 e = xs[j];
                const bool same = e.x == part;
                nsame += same ? 1u : 0u;
                excl += (same && j < lane) ? ((uint64_t(e.w) << 32) | e.z) : 0ull;
            }
            const uint64_t off = S.bytes + (excl & kAppSizeMask);
            const bool fit = valid && !(S.cnt & kAppFull) && off + size <= a.ocap;
            if (valid)
                a.pdst[it.x] = fit ? uint32_t(off) : kAppNone;
            uint32_t v = 0;
            uint64_t mine = 0;
            if (fit) {
                // raw(0, header byte || length bytes), moved back to the step's start
                uint32_t c = t0[(hdr & 0x3f) | ((lb - 1) << 6)];
                for (uint32_t b = 0; b < lb; b++)
                    c = t0[(c ^ (len >> (8 * b))) & 0xFF] ^ (c >> 8);
                v = mulmod_dev(c, xi[uint32_t(excl >> kAppMetaShift) + mi]);
                mine = packed | (1ull << kAppCountShift);
            }
            wsync();   // every lane has read exchange 1
            xs[lane] = make_uint4(part, v, uint32_t(mine), uint32_t(mine >> 32));
            wsync();
            uint64_t tot = 0;
            uint32_t pc = 0;
#pragma unroll 16
            for (int j = 0; j < kWaveSize; j++) {
                const uint4 e = xs[j];
                const bool same = e.x == part;
                tot += same ? ((uint64_t(e.w) << 32) | e.z) : 0ull;
                pc ^= same ? e.y : 0u;
            }
            if (valid && excl == 0) {   // the partition's first lane (every posted size is nonzero)
                const uint32_t mt = uint32_t(tot >> kAppMetaShift) & 0x3FFu;
                const uint32_t cnt = uint32_t(tot >> kAppCountShift);
                S.bytes += tot & kAppSizeMask;
                S.crc = mulmod_dev(S.crc ^ pc, xm[mt]);
                S.cnt = (S.cnt + cnt) | (cnt != nsame ? kAppFull : 0u);
                st_store(part, S);
            }
            wsync();   // the next step reads these states, and reuses xs and the ring
        }
        // Segment::getAppendedLength (src/Segment.cc:672-684): the running
        // checksum over the 4 head bytes, finalized
        for (uint64_t p = w + uint64_t(W) * lane; p < a.npart; p += uint64_t(W) * kWaveSize) {
            const AppState S = st_load(uint32_t(p));
            const uint64_t k = s * a.npart + p;
            const uint32_t head = uint32_t(S.bytes);
            uint32_t c = S.crc;
            for (int b = 0; b < 4; b++)
                c = t0[(c ^ (head >> (8 * b))) & 0xFF] ^ (c >> 8);
            a.certs[k] = ramcrc_seg_cert{head, ~c};
            const uint32_t fl = !good ? RAMCRC_SEG_SOURCE_BAD
                                      : (S.cnt & kAppFull) ? RAMCRC_SEG_APPEND_FULL : RAMCRC_SEG_OK;
            a.ostat[k] = ramcrc_append_status{fl, S.cnt & ~kAppFull};
        }
        wsync();   // lst is reused by this wave's next segment
    }
}

// ------------------------------------------------------------ k_app_copy
// `len` payload bytes from src to dst by kLanes lanes (this one is `sub`).
// Source and destination are arbitrary mod 16 and differ.  The destination's
// full 16-byte granules are written with aligned 16-byte stores, each taken
// from the two aligned 16-byte source words that hold its bytes, joined by a
// byte funnel shift; the bytes before the first and after the last full
// granule with byte stores, so two entries that share a granule never write
// each other's bytes and nothing past the end is written.  The second source
// word is read only when the shift is not zero: it then holds a payload byte,
// and as the source range is 16-byte aligned at both ends, lies inside it.
template <int kLanes, int kU>
__device__ __forceinline__ void app_copy(uint64_t src, uint64_t dst, uint32_t len, uint32_t sub)
{
    typedef __attribute__((address_space(1))) u32x4 gw32x4;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    const uint64_t end = dst + len;
    const uint64_t a0 = (dst + 15) & ~15ull, a1 = end & ~15ull;
    const uint64_t hend = a0 < end ? a0 : end;        // head bytes [dst, hend)
    const uint64_t tbeg = a1 > hend ? a1 : hend;      // tail bytes [tbeg, end)
    for (uint64_t p = dst + sub; p < hend; p += kLanes)
        *reinterpret_cast<gw8*>(p) = *reinterpret_cast<const gu8*>(src + (p - dst));
    for (uint64_t p = tbeg + sub; p < end; p += kLanes)
        *reinterpret_cast<gw8*>(p) = *reinterpret_cast<const gu8*>(src + (p - dst));
    if (a1 <= a0)
        return;
    const uint32_t ng = uint32_t((a1 - a0) >> 4);
    const uint64_t s0 = src + (a0 - dst);
    const uint32_t sh = uint32_t(s0) & 15u, dw = sh >> 2, by = sh & 3u;
    const uint64_t sa = s0 & ~15ull;
    for (uint32_t q0 = sub; q0 < ng; q0 += kLanes * kU) {
        u32x4 lo[kU], hi[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const uint32_t q = q0 + u * kLanes;
            if (q < ng) {
                lo[u] = *gptr16(sa + 16ull * q);
                hi[u] = sh ? *gptr16(sa + 16ull * q + 16) : lo[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const uint32_t q = q0 + u * kLanes;
            if (q < ng) {
                uint32_t w[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
                if (dw & 2u) {
#pragma unroll
                    for (int j = 0; j < 6; j++)
                        w[j] = w[j + 2];
                }
                if (dw & 1u) {
#pragma unroll
                    for (int j = 0; j < 5; j++)
                        w[j] = w[j + 1];
                }
                u32x4 o;
                o.x = __builtin_amdgcn_alignbyte(w[1], w[0], by);
                o.y = __builtin_amdgcn_alignbyte(w[2], w[1], by);
                o.z = __builtin_amdgcn_alignbyte(w[3], w[2], by);
                o.w = __builtin_amdgcn_alignbyte(w[4], w[3], by);
                *reinterpret_cast<gw32x4*>(a0 + 16ull * q) = o;
            }
        }
    }
}

// Tiles of 256 placements, one per thread: the thread writes its entry's
// header and length bytes and posts the payload in LDS.  Payloads below
// kAppBigMin are then copied by groups of 8 lanes (neighbouring groups take
// neighbouring entries, which are neighbours in the source too), 32 entries
// at a time, with all of a pass's loads in flight before its first store;
// payloads up to kAppGroupMin by a wave each, 4 KiB per pass, the workgroup's
// four waves on four entries; longer ones by the whole workgroup, 16 KiB per
// pass.
__global__ __launch_bounds__(kAppCopyThreads) void k_app_copy(AppDesc a)
{
    __shared__ uint64_t ssrc[kAppCopyThreads], sdst[kAppCopyThreads];
    __shared__ uint32_t slen[kAppCopyThreads], sbig[kAppCopyThreads];
    __shared__ uint32_t nbig[2];   // by tile parity: a slow wave may still read the previous tile's
    if (*a.refuse)
        return;
    const uint64_t np = *a.n_place;
    const uint64_t ntiles = (np + kAppCopyThreads - 1) / kAppCopyThreads;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
        __syncthreads();   // the previous tile's copies have read their descriptors and its count
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        const uint64_t i = tile * kAppCopyThreads + t;
        uint64_t src = 0, dst = 0;
        uint32_t len = 0;
        if (i < np) {
            const uint32_t off = a.pdst[i];
            if (off != kAppNone) {
                const uint2 pl = a.place[i];
                const u32x4 r = a.entries[pl.x];
                const uint32_t lb = app_len_bytes(r.z);
                // (k_app_scan placed only entries that fit; checked again as
                // the last thing between a stale word and a stray store)
                if (uint64_t(off) + 1 + lb + r.z <= a.ocap) {
                    typedef __attribute__((address_space(1))) uint8_t gw8;
                    len = r.z;
                    src = a.base + uint64_t(r.x) * a.stride + r.y + 1 + ((r.w >> 6) & 3) + 1;
                    const uint64_t e = a.out + (uint64_t(r.x) * a.npart + pl.y) * a.ostride + off;
                    *reinterpret_cast<gw8*>(e) = uint8_t((r.w & 0x3f) | ((lb - 1) << 6));
                    for (uint32_t b = 0; b < lb; b++)
                        *reinterpret_cast<gw8*>(e + 1 + b) = uint8_t(len >> (8 * b));
                    dst = e + 1 + lb;
                }
            }
        }
        ssrc[t] = src;
        sdst[t] = dst;
        slen[t] = len;
        if (len >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t j = g; j < kAppCopyThreads; j += kAppCopyThreads / 8) {
            const uint32_t L = slen[j];
            if (L && L <= kAppShortMax)
                app_copy<8, 2>(ssrc[j], sdst[j], L, sub);          // one pass of 2 granules per lane
            else if (L > kAppShortMax && L < kAppBigMin)
                app_copy<8, 8>(ssrc[j], sdst[j], L, sub);          // 1 KiB per pass
        }
        const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
        for (uint32_t b = wv; b < nb; b += kAppCopyThreads / kWaveSize) {
            const uint32_t j = sbig[b];
            if (slen[j] < kAppGroupMin)
                app_copy<kWaveSize, 4>(ssrc[j], sdst[j], slen[j], ln);   // a wave each, 4 KiB per pass
        }
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t j = sbig[b];
            if (slen[j] >= kAppGroupMin)
                app_copy<kAppCopyThreads, 4>(ssrc[j], sdst[j], slen[j], t);
        }
    }
}

}  // namespace
