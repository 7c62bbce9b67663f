// Side log of a replay (ramcrc_replay_sidelog_device): k_sl_stamp
// (DESIGN.md 5.12).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order, after dev_append.inc; not a standalone
// header.
//
// The call is the append at one partition (k_app_mark, k_app_scan, k_app_copy
// unchanged) followed by one pass over the list, behind the kernel boundary:
//   k_sl_stamp  reads every placement's destination (AppDesc::pdst), writes
//               its reference, counts it, and rewrites every appended
//               tombstone in its output as ObjectManager::replaySegment does
//               before it logs one (src/ObjectManager.cc:845-851): segmentId
//               0, the caller's timestamp, and ObjectTombstone::computeChecksum
//               (src/Object.cc:1042-1057) recomputed from the bytes that now
//               lie in the output.
// The segment certificate covers entry headers only (src/Segment.cc:672-684),
// so the rewrite leaves what k_app_scan sealed valid.

namespace {

constexpr int kSlThreads = 256;
constexpr int kSlLanes = 8;                  // lanes per tombstone
constexpr uint32_t kSlOneLaneMax = 68;       // payload bytes (keys up to 36) up to which one lane rewrites a tombstone
constexpr uint32_t kSlCountWords = 32;       // scratch: one 128-byte line of counters
constexpr int kSlCounters = 7;               // ramcrc_sidelog_counts, in its field order
constexpr int kSlTicket = 8;                 // counts[kSlTicket]: workgroups that have finished
static_assert(sizeof(ramcrc_sidelog_counts) == kSlCounters * sizeof(uint64_t), "sidelog counters");
static_assert(sizeof(ramcrc_log_ref) == sizeof(uint2), "log reference");
static_assert((kSlTicket + 1) * sizeof(uint64_t) <= kSlCountWords * sizeof(uint32_t), "counter line");

struct SlDesc {
    uint2* refs;                        // [pcap] {output, offset of the entry header}; nullable
    ramcrc_sidelog_counts* counts_out;
    unsigned long long* counts;         // scratch line, zeroed by the call: counters, ticket
    uint32_t timestamp;
};

// x^(8 d) for any 32-bit d (g_tab.xbyte: one factor per byte of d).
__device__ __forceinline__ uint32_t sl_xpow8(uint32_t d)
{
    uint32_t r = g_tab.xbyte[0][d & 0xFF];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const uint32_t b = (d >> (8 * j)) & 0xFF;
        if (b)
            r = mulmod_dev(r, g_tab.xbyte[j][b]);
    }
    return r;
}

// One appended tombstone of at most kSlOneLaneMax payload bytes, by one lane:
// the message is at most 64 bytes, loaded 32 at a time (every load in flight
// before the first table step; the rewritten fields are constants of the
// unrolled loop, not loads) and taken through the byte table.  A group's
// combine costs a GF(2) multiply per lane, more than these steps: over 102 M
// tombstones of 40 bytes the pass took 8.9 ms with a group each and 5.1 ms
// with a lane each (DESIGN.md 5.12).
__device__ __forceinline__ void sl_stamp_one(uint64_t pay, uint32_t len, uint32_t ts, const uint32_t* t0)
{
    typedef __attribute__((address_space(1))) uint8_t gw8;
    const uint32_t M = len - 4;   // 28 .. 64
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t h = 0; h < kSlOneLaneMax - 4; h += 32) {
        uint32_t v[32];
#pragma unroll
        for (uint32_t j = 0; j < 32; j++) {
            const uint32_t b = ramcrc_sl::at(h + j);
            uint32_t s = 0;
            if (!ramcrc_sl::stamped(b, ts, s) && h + j < M)
                s = *reinterpret_cast<const gu8*>(pay + b);
            v[j] = s;
        }
#pragma unroll
        for (uint32_t j = 0; j < 32; j++)
            if (h + j < M)
                c = t0[(c ^ v[j]) & 0xFF] ^ (c >> 8);
    }
    const uint32_t ck = ~c;
#pragma unroll
    for (uint32_t b = 0; b < ramcrc_sl::kSegmentIdBytes; b++)
        *reinterpret_cast<gw8*>(pay + ramcrc_sl::kSegmentIdAt + b) = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
        *reinterpret_cast<gw8*>(pay + ramcrc_sl::kTimestampAt + b) = uint8_t(ts >> (8 * b));
        *reinterpret_cast<gw8*>(pay + ramcrc_sl::kChecksumAt + b) = uint8_t(ck >> (8 * b));
    }
}
static_assert((kSlOneLaneMax - 4) % 32 == 0 && kSlOneLaneMax >= ramcrc_sl::kTombHeaderBytes, "two loads of 32");

// One longer appended tombstone, by the kSlLanes lanes of a group (this one is
// `sub`): payload at `pay` in its output (any alignment), `len` > kSlOneLaneMax.
// The checksummed message is the new bytes [0, 28) and the key [32, len); lane
// `sub` takes the sub-th eighth of it with the byte table, substituting the
// rewritten fields so that no lane reads a byte another lane writes, moves its
// part to the end of the message (raw(s, A||B) = X^|B|(raw(s, A)) ^ raw(0, B))
// and the group XORs the parts.  Every store is a byte store inside the
// payload.
__device__ __forceinline__ void sl_stamp(uint64_t pay, uint32_t len, uint32_t sub, uint32_t ts,
                                         const uint32_t* t0)
{
    typedef __attribute__((address_space(1))) uint8_t gw8;
    const uint32_t M = len - 4;
    const uint32_t C = (M + kSlLanes - 1) / kSlLanes;
    const uint32_t lo = sub * C < M ? sub * C : M;
    const uint32_t hi = lo + C < M ? lo + C : M;
    uint32_t c = sub == 0 ? 0xFFFFFFFFu : 0u;   // a fresh Crc32C in front of the first part
    for (uint32_t m = lo; m < hi; m++) {
        const uint32_t b = ramcrc_sl::at(m);
        uint32_t v;
        if (!ramcrc_sl::stamped(b, ts, v))
            v = *reinterpret_cast<const gu8*>(pay + b);
        c = t0[(c ^ v) & 0xFF] ^ (c >> 8);
    }
    if (hi < M)
        c = mulmod_dev(c, sl_xpow8(M - hi));
    c ^= __shfl_xor(c, 1);
    c ^= __shfl_xor(c, 2);
    c ^= __shfl_xor(c, 4);
    const uint32_t ck = ~c;
    *reinterpret_cast<gw8*>(pay + ramcrc_sl::kSegmentIdAt + sub) = 0;
    if (sub < 4) {
        *reinterpret_cast<gw8*>(pay + ramcrc_sl::kTimestampAt + sub) = uint8_t(ts >> (8 * sub));
        *reinterpret_cast<gw8*>(pay + ramcrc_sl::kChecksumAt + sub) = uint8_t(ck >> (8 * sub));
    }
}
static_assert(ramcrc_sl::kSegmentIdBytes == kSlLanes, "one lane per segmentId byte");

// Tiles of 256 placements, one per thread: the thread writes its placement's
// reference, counts it in registers, rewrites a short tombstone itself and
// posts a longer one in LDS; then the 32 groups of 8 lanes take the tile's
// longer tombstones.  At the end every workgroup adds its sums to the counter
// line with one atomic per nonzero counter, and the last workgroup to finish
// copies the line to d_counts.
__global__ __launch_bounds__(kSlThreads) void k_sl_stamp(AppDesc a, SlDesc sl)
{
    __shared__ unsigned long long spay[kSlThreads];   // a tile's payload addresses; at the end the waves' sums
    __shared__ uint32_t slen[kSlThreads];
    __shared__ uint32_t t0[256];
    __shared__ uint32_t is_last;
    if (*a.refuse)
        return;
    const uint32_t t = threadIdx.x;
    t0[t] = g_tab.t0.t[t];
    static_assert(kSlThreads == 256, "one byte-table entry per thread");
    const uint64_t np = *a.n_place;
    const uint64_t ntiles = (np + kSlThreads - 1) / kSlThreads;
    unsigned long long cnt[kSlCounters] = {};
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();   // the table is filled; the previous tile's groups have read their descriptors
        const uint64_t i = tile * kSlThreads + t;
        uint64_t pay = 0;
        uint32_t len = 0;
        if (i < np) {
            const uint32_t off = a.pdst[i];
            const u32x4 r = a.entries[a.place[i].x];
            const uint32_t lb = app_len_bytes(r.z);
            // (as k_app_copy checks it again: nothing is stamped past a head)
            const bool app = off != kAppNone && uint64_t(off) + 1 + lb + r.z <= a.ocap;
            if (sl.refs)
                sl.refs[i] = app ? make_uint2(r.x, off) : make_uint2(kAppNone, kAppNone);
            if (!app) {
                cnt[6]++;
            } else {
                switch (ramcrc_sl::kind(r.w & 0x3f, r.z)) {
                case ramcrc_sl::kObject:
                    cnt[0]++;
                    cnt[3] += r.z;
                    break;
                case ramcrc_sl::kTombstone:
                    cnt[1]++;
                    cnt[4] += r.z;
                    pay = a.out + uint64_t(r.x) * a.ostride + off + 1 + lb;
                    len = r.z;
                    break;
                case ramcrc_sl::kShortTombstone:
                    cnt[5]++;
                    break;
                default:
                    cnt[2]++;
                }
            }
        }
        if (len && len <= kSlOneLaneMax) {
            sl_stamp_one(pay, len, sl.timestamp, t0);
            len = 0;
        }
        spay[t] = pay;
        slen[t] = len;
        __syncthreads();
        const uint32_t g = t / kSlLanes, sub = t % kSlLanes;
        for (uint32_t j = g; j < kSlThreads; j += kSlThreads / kSlLanes) {
            const uint32_t L = slen[j];   // the same for the group's lanes
            if (L)
                sl_stamp(spay[j], L, sub, sl.timestamp, t0);
        }
    }
    // (one atomic per workgroup and nonzero counter: the counters share a
    // line, and 8 workgroups per CU of waves adding to it one after the other
    // took longer than the pass itself over a million records)
    __syncthreads();   // the last tile's groups are done with spay
    unsigned long long* const wsum = spay;
    static_assert(kSlCounters * (kSlThreads / kWaveSize) <= kSlThreads, "wave sums fit the tile's LDS");
#pragma unroll
    for (int k = 0; k < kSlCounters; k++) {
        unsigned long long v = cnt[k];
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            v += __shfl_xor(v, d);
        if ((t & (kWaveSize - 1)) == 0)
            wsum[k * (kSlThreads / kWaveSize) + t / kWaveSize] = v;
    }
    __syncthreads();
    if (t < kSlCounters) {
        unsigned long long v = 0;
        for (int w = 0; w < kSlThreads / kWaveSize; w++)
            v += wsum[t * (kSlThreads / kWaveSize) + w];
        if (v)
            atomicAdd(&sl.counts[t], v);
    }
    __syncthreads();   // this workgroup has issued its sums
    if (t == 0) {
        __threadfence();
        is_last = atomicAdd(&sl.counts[kSlTicket], 1ull) + 1 == gridDim.x;
    }
    __syncthreads();
    if (is_last && t < kSlCounters) {
        __threadfence();
        reinterpret_cast<unsigned long long*>(sl.counts_out)[t] = atomicAdd(&sl.counts[t], 0ull);
    }
}

}  // namespace
