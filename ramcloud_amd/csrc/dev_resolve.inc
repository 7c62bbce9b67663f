// Replay resolution (ramcrc_replay_resolve_device): k_res_zero, k_res_insert,
// k_res_pick, k_res_tiles, k_res_scan, k_res_emit (DESIGN.md 5.10).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.
//
// The decision ObjectManager::replaySegment makes after each checksum
// (src/ObjectManager.cc:671-734, :766-867) for every walked object and
// tombstone of a batch replayed into an empty table: per key the highest
// version survives, a tombstone before an object of the same version; the
// per-record rules are resolve_rules.h's, shared with the host form.  Six
// launches, none of which waits for another workgroup:
//   k_res_zero    clears the grouping table, sized from the walked count;
//   k_res_insert  one thread per record: parses it, reads its version, takes
//                 or computes its key hash, counts it; a participant probes
//                 the table from hash & mask, claims an empty slot with one
//                 CAS of its own index or compares its key with the slot's
//                 claimant (read from the segment bytes, which never change),
//                 then folds its version into the slot's maximum;
//   k_res_pick    participants at their slot's maximum version fold
//                 ~(is_object << 32 | index) into the slot's pick by maximum
//                 (the minimum of the rank: the table starts at zero);
//   k_res_tiles   the verdict: every record's winner, the live counters, and
//                 the live count of every tile of 1,024 records;
//   k_res_scan    one workgroup: exclusive sum of the tile sums, *d_n_live
//                 and the counters;
//   k_res_emit    per tile, the live records' slots of d_live.
// Inside k_res_insert and k_res_pick every access to a slot word is a relaxed
// agent-scope atomic, loads included (an XCD's L2 does not see another XCD's
// plain stores); the kernels after them read the words plainly.  A slot's
// only key material is its claimant's record index, published by the claiming
// CAS itself, so no lane ever waits for another lane's store.

namespace {

constexpr uint64_t kResNone = ~0ull;
constexpr uint32_t kResHeadWords = 16;   // the refusal word, then six 64-bit counters at word 4

struct ResDesc {
    uint64_t base;              // source segments
    uint64_t stride;
    uint64_t nseg;
    const ramcrc_seg_status* status;
    const u32x4* entries;       // {segment, offset, length, header}
    uint64_t ecap;
    const uint64_t* n_entries;
    const uint64_t* key_hash;   // nullable: the caller's hashes
    uint32_t* winner;           // nullable
    uint2* live;                // {record, 0}
    uint64_t lcap;
    uint64_t* n_live;
    ramcrc_resolve_counts* counts_out;
    // scratch
    uint32_t* refuse;           // nonzero: the call writes only *n_live = 0 and zeroed counts
    unsigned long long* counts; // objects, tombstones, live_objects, live_tombstones, malformed, safe_version
    unsigned long long* slots;  // [slots] three words each, so that a key's words share a cache line:
                                //   the key's highest version; ~(lowest rank at that version), 0:
                                //   none yet; low half 1 + the claiming record, 0: empty
    uint64_t* rec_ver;          // [ecap] a participant's version
    uint64_t* rec_slot;         // [ecap] its slot (kResNone: no participant); after k_res_tiles its winner
    uint64_t* tile_sum;         // [tiles] live records of a tile, then its exclusive offset
    uint32_t* ctx_status;
};

__device__ __forceinline__ void res_refuse(const ResDesc& a)
{
    *a.refuse = 1u;
    atomicOr(a.ctx_status, kStatusSticky);
}

__device__ __forceinline__ uint64_t res_n_records(const ResDesc& a)
{
    const uint64_t nw = *a.n_entries;
    return nw < a.ecap ? nw : a.ecap;
}

#define RES_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr uint64_t kResSlotWords = 3;
__device__ __forceinline__ unsigned long long* res_ver(const ResDesc& a, uint64_t s)
{
    return a.slots + kResSlotWords * s;
}
__device__ __forceinline__ unsigned long long* res_pick(const ResDesc& a, uint64_t s)
{
    return a.slots + kResSlotWords * s + 1;
}
__device__ __forceinline__ uint32_t* res_claim(const ResDesc& a, uint64_t s)
{
    return reinterpret_cast<uint32_t*>(a.slots + kResSlotWords * s + 2);
}

// The key fields of record r, a participant or a candidate for one.
struct ResKey {
    uint64_t table_id;
    uint64_t addr;   // of the key's first byte
    uint32_t len;
};

// Are the len bytes at a and at b (any residues) equal?  Eight bytes a step
// through part_bytes' aligned loads; every byte read is a key byte.
__device__ __forceinline__ bool res_bytes_equal(uint64_t a, uint64_t b, uint32_t len)
{
    for (uint32_t o = 0; o < len; o += 8) {
        const uint32_t n = len - o < 8 ? len - o : 8u;
        if (part_bytes(a + o, n) != part_bytes(b + o, n))
            return false;
    }
    return true;
}

// The key of record j, which claimed a slot and so is a participant.
__device__ __forceinline__ ResKey res_key_of(const ResDesc& a, uint64_t j)
{
    const u32x4 r = a.entries[j];
    const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
    const PartRd rd{a.base + uint64_t(r.x) * a.stride + pay};
    const ramcrc_part::Parsed p = ramcrc_part::parse(r.w & 0x3f, r.z, true, rd);
    return ResKey{p.table_id, rd.pay + p.key_off, p.key_len};
}

// -------------------------------------------------------------- k_res_zero
__global__ __launch_bounds__(kPartThreads) void k_res_zero(ResDesc a)
{
    const uint64_t nw = kResSlotWords * ramcrc_res::slots_for(res_n_records(a));
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < nw; w += nthr)
        a.slots[w] = 0;
}

// ------------------------------------------------------------ k_res_insert
template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_res_insert(ResDesc a)
{
    const uint64_t ne = res_n_records(a);
    const uint64_t mask = ramcrc_res::slots_for(ne) - 1;
    for (uint64_t i0 = uint64_t(blockIdx.x) * kPartThreads; i0 < ne;
         i0 += uint64_t(gridDim.x) * kPartThreads) {
        const uint64_t i = i0 + threadIdx.x;
        bool is_obj = false, is_tomb = false, mal = false;
        if (i < ne) {
            const u32x4 r = a.entries[i];
            const uint32_t seg = r.x, type = r.w & 0x3f;
            uint64_t slot = kResNone;
            if (seg >= a.nseg) {
                res_refuse(a);
            } else if (a.status[seg].flags & RAMCRC_SEG_OK) {
                const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
                const bool readable = !(r.w & kRecOverlong) && pay + r.z <= a.stride;
                const PartRd rd{a.base + uint64_t(seg) * a.stride + pay};
                if (ramcrc_res::resolved_type(type)) {
                    const ramcrc_part::Parsed p = ramcrc_part::parse(type, r.z, readable, rd);
                    if (p.kind == ramcrc_part::kMalformed) {
                        mal = true;
                    } else {
                        is_obj = type == RAMCRC_LOG_ENTRY_TYPE_OBJ;
                        is_tomb = !is_obj;
                        const ResKey me{p.table_id, rd.pay + p.key_off, p.key_len};
                        const uint64_t ver = ramcrc_res::version(type, rd);
                        uint64_t hash;
                        if constexpr (kGiven)
                            hash = a.key_hash[i];
                        else
                            hash = part_key_hash(me.table_id, me.addr, me.len);
                        // linear probing, bounded by the slot count (load <= 0.5:
                        // an empty slot ends every chain)
                        uint64_t s = hash & mask;
                        for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                            uint32_t c = __hip_atomic_load(res_claim(a, s), RES_RLX);
                            if (c == 0 && __hip_atomic_compare_exchange_strong(
                                              res_claim(a, s), &c, uint32_t(i) + 1, __ATOMIC_RELAXED,
                                              RES_RLX)) {
                                slot = s;
                                break;
                            }
                            // c: the claimant (the failed CAS stored it)
                            const uint64_t j = c - 1;
                            if (j == i) {   // (not reached: a record claims once)
                                slot = s;
                                break;
                            }
                            // equal hashes never make two keys equal; a caller's
                            // hashes that differ make them different
                            if constexpr (kGiven) {
                                if (a.key_hash[j] != hash)
                                    continue;
                            }
                            const ResKey k = res_key_of(a, j);
                            if (k.table_id == me.table_id && k.len == me.len &&
                                res_bytes_equal(k.addr, me.addr, me.len)) {
                                slot = s;
                                break;
                            }
                        }
                        if (slot != kResNone) {
                            __hip_atomic_fetch_max(res_ver(a, slot), static_cast<unsigned long long>(ver),
                                                   RES_RLX);
                            a.rec_ver[i] = ver;
                        }
                    }
                } else if (type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION && readable &&
                           r.z >= ramcrc_res::kSafeVersionBytes) {
                    __hip_atomic_fetch_max(&a.counts[5], static_cast<unsigned long long>(rd.u64(0)),
                                           RES_RLX);
                }
            }
            a.rec_slot[i] = slot;
        }
        // the counters: one atomic per wave and counter
        const unsigned long long no = __builtin_popcountll(__ballot(is_obj));
        const unsigned long long nt = __builtin_popcountll(__ballot(is_tomb));
        const unsigned long long nm = __builtin_popcountll(__ballot(mal));
        if ((threadIdx.x & (kWaveSize - 1)) == 0) {
            if (no)
                atomicAdd(&a.counts[0], no);
            if (nt)
                atomicAdd(&a.counts[1], nt);
            if (nm)
                atomicAdd(&a.counts[4], nm);
        }
    }
}

// -------------------------------------------------------------- k_res_pick
__global__ __launch_bounds__(kPartThreads) void k_res_pick(ResDesc a)
{
    if (*a.refuse)
        return;
    const uint64_t ne = res_n_records(a);
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < ne; i += nthr) {
        const uint64_t s = a.rec_slot[i];
        if (s == kResNone || a.rec_ver[i] != *res_ver(a, s))
            continue;
        const uint64_t rank = ramcrc_res::rank(a.entries[i].w & 0x3f, i);
        __hip_atomic_fetch_max(res_pick(a, s), static_cast<unsigned long long>(~rank), RES_RLX);
    }
}

// ------------------------------------------------------------- k_res_tiles
__global__ __launch_bounds__(kPartThreads) void k_res_tiles(ResDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse)
        return;
    const uint64_t ne = res_n_records(a);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        uint32_t lo = 0, lt = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            const uint64_t i = i0 + k;
            if (i >= ne)
                continue;
            const uint64_t s = a.rec_slot[i];
            // the low word of the pick's complement: the winner's index
            const uint32_t w = s == kResNone ? RAMCRC_RESOLVE_NONE : uint32_t(~*res_pick(a, s));
            a.rec_slot[i] = w;
            if (a.winner)
                a.winner[i] = w;
            if (w == uint32_t(i)) {
                if ((a.entries[i].w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ)
                    lo++;
                else
                    lt++;
            }
        }
        uint32_t so = lo, st = lt;
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1) {
            so += __shfl_xor(so, d);
            st += __shfl_xor(st, d);
        }
        if ((threadIdx.x & (kWaveSize - 1)) == 0) {
            if (so)
                atomicAdd(&a.counts[2], static_cast<unsigned long long>(so));
            if (st)
                atomicAdd(&a.counts[3], static_cast<unsigned long long>(st));
        }
        uint64_t tot;
        (void)part_block_excl(uint64_t(lo) + lt, wsum, &tot);
        if (threadIdx.x == 0)
            a.tile_sum[tile] = tot;
    }
}

// -------------------------------------------------------------- k_res_scan
// One workgroup: the tile sums become exclusive offsets, kPartThreads tiles a
// step; then the list's length and the counters.
__global__ __launch_bounds__(kPartThreads) void k_res_scan(ResDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse) {
        if (threadIdx.x == 0) {
            *a.n_live = 0;
            *a.counts_out = ramcrc_resolve_counts{0, 0, 0, 0, 0, 0};
        }
        return;
    }
    const uint64_t ne = res_n_records(a);
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
    if (threadIdx.x == 0) {
        *a.n_live = carry;
        *a.counts_out = ramcrc_resolve_counts{a.counts[0], a.counts[1], a.counts[2],
                                              a.counts[3], a.counts[4], a.counts[5]};
    }
}

// -------------------------------------------------------------- k_res_emit
__global__ __launch_bounds__(kPartThreads) void k_res_emit(ResDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (*a.refuse)
        return;
    const uint64_t ne = res_n_records(a);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        bool live[kPartPer];
        uint64_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            live[k] = i0 + k < ne && a.rec_slot[i0 + k] == i0 + k;
            v += live[k];
        }
        uint64_t tot;
        uint64_t dst = a.tile_sum[tile] + part_block_excl(v, wsum, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            if (!live[k])
                continue;
            if (dst < a.lcap)
                a.live[dst] = make_uint2(uint32_t(i0 + k), 0u);
            dst++;
        }
    }
}

#undef RES_RLX

}  // namespace
