// The persistent replay table (ramcrc_replay_table_*): k_rtab_zero,
// k_rtab_open, k_rtab_insert, k_rtab_pick (an add), k_rtab_tiles, k_rtab_scan,
// k_rtab_emit (a live query), k_rtab_stats (DESIGN.md 5.11), k_rtab_lookup
// (a lookup by key, DESIGN.md 5.13), k_rtab_read_size, k_rtab_read_scan,
// k_rtab_read_gather (a multi-read's reply, DESIGN.md 5.14).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, after dev_resolve.inc; not a standalone header.
//
// ramcrc_replay_resolve_device's decision, fed batch by batch: the grouping
// table outlives the call, and a key's winner is the winner over every batch
// added so far.  A record is named {batch, record}; a slot is four 64-bit
// words, so that it never straddles a 128-byte line:
//   [0] the key's highest version;
//   [1] ~(lowest rank at that version), the pick; 0: none;
//   [2] the claim, batch << 32 | record + 1 of the record whose key is the
//       slot's; 0: empty;
//   [3] spare.
// An add is three launches, none of which waits for another workgroup:
//   k_rtab_open    one thread writes the batch's descriptor (where its
//                  segments, tables and work array lie), so that later adds
//                  can read this batch's keys;
//   k_rtab_insert  one thread per record: k_res_insert's probe with a 64-bit
//                  claim, the claimant's key read through its batch's
//                  descriptor; folds the version into the slot's maximum,
//                  drops the slot's pick when that raised the maximum, and
//                  leaves the record's slot in d_work;
//   k_rtab_pick    the maxima are final: participants at their slot's maximum
//                  fold ~rank into the pick by maximum.
// The stale pick is the one hazard a table that stays adds.  Key K wins batch
// 0 with a tombstone of version 5; batch 1 brings an object of version 7.  The
// pick still holds the tombstone's ~rank, which is larger than the
// newcomer's, so a bare maximum would never replace it.  Between adds a pick
// is always one made at the slot's maximum version, and no launch but
// k_rtab_pick folds picks; so a lane of the insert whose version strictly
// raises the maximum (the fetch-max returns what it replaced) knows that the
// pick in the slot, if any, is of a lower version, and stores 0 (none) to it.
// Every such lane stores the same value, and the folds begin behind the
// kernel boundary.  A fresh slot's pick is 0 already, so version 0 needs no
// rule of its own.
// A live query reads one batch's d_work and the slots' picks as they stand:
// k_rtab_tiles (winners, live counts per tile of 1,024 records), k_rtab_scan
// (one workgroup: offsets, *d_n_live, the counters), k_rtab_emit (the list).
// Inside insert and pick every access to a slot word is a relaxed
// agent-scope atomic, loads included; words written by earlier launches lie
// behind kernel boundaries and are read plainly.  A slot's only key material
// is its claim, published by the claiming CAS itself, so no lane ever waits
// for another lane's store, in this batch or an earlier one.

namespace {

constexpr uint64_t kRtabSlotWords = 4;
constexpr uint64_t kRtabHeadWords = 16;   // 64-bit words before the descriptors

// The head of the table's allocation.
enum : uint32_t {
    kRtabRefuse = 0,   // nonzero: spoiled until the next reset
    kRtabKeys = 1,     // claimed slots
    kRtabSafe = 2,     // the highest SAFEVERSION seen
};

// One added batch: 16 words, written by k_rtab_open and only read afterwards
// (by every later add, for its claimants' keys).
struct RtabBatch {
    uint64_t base;              // source segments
    uint64_t stride;
    uint64_t nseg;
    const ramcrc_seg_status* status;
    const u32x4* entries;       // {segment, offset, length, header}
    const uint64_t* n_entries;
    uint64_t ecap;
    const uint64_t* key_hash;   // nullable: the caller's hashes
    uint64_t* work;             // [ecap] a participant's slot, kResNone: no participant
    uint64_t pad[7];
};
static_assert(sizeof(RtabBatch) == 128, "a descriptor is one 128-byte line");

// A batch's participants, counted by the insert with atomics: on a line of
// their own, away from the descriptor the probing lanes read.
struct RtabCount {
    unsigned long long objects, tombstones, malformed;
    uint64_t pad[13];
};
static_assert(sizeof(RtabCount) == 128, "a batch's counters are one 128-byte line");

struct RtabDesc {
    unsigned long long* head;   // [kRtabHeadWords]
    RtabBatch* batches;         // [max_batches]
    RtabCount* bcount;          // [max_batches]
    unsigned long long* slots;  // [nslots] four words each
    uint64_t nslots;            // a power of two
    uint64_t key_cap;
    uint32_t batch;             // the batch added or queried
    uint32_t n_batches;         // batches added so far (stats)
    RtabBatch open;             // k_rtab_open: the descriptor to write
    // a live query's outputs
    uint2* winner;              // nullable: {batch, record}
    uint2* live;                // {record, 0}
    uint64_t lcap;
    uint64_t* n_live;
    ramcrc_resolve_counts* counts_out;
    uint64_t* tile_sum;         // [tiles] live tombstones << 32 | live objects, then the exclusive sums
    ramcrc_replay_table_stats* stats_out;
    uint32_t* ctx_status;
};

#define RTAB_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ unsigned long long* rtab_word(const RtabDesc& a, uint64_t s, uint32_t w)
{
    return a.slots + kRtabSlotWords * s + w;
}

// Spoiled?  The word is only ever set, and a launch that sees it set late has
// only worked on a table nobody reads any more.
__device__ __forceinline__ bool rtab_refused(const RtabDesc& a)
{
    return __hip_atomic_load(&a.head[kRtabRefuse], RTAB_RLX) != 0;
}

__device__ __forceinline__ void rtab_refuse(const RtabDesc& a)
{
    __hip_atomic_store(&a.head[kRtabRefuse], 1ull, RTAB_RLX);
    atomicOr(a.ctx_status, kStatusSticky);
}

// After the insert: spoiled before this add, by it, or past the key capacity?
__device__ __forceinline__ bool rtab_spoiled_after_insert(const RtabDesc& a)
{
    return rtab_refused(a) || a.head[kRtabKeys] > a.key_cap;
}

__device__ __forceinline__ uint64_t rtab_n_records(const RtabBatch& b)
{
    const uint64_t nw = *b.n_entries;
    return nw < b.ecap ? nw : b.ecap;
}

// The rank of record {batch, record}: a tombstone before an object, then the
// lowest batch, then the lowest record.
__device__ __forceinline__ uint64_t rtab_rank(uint32_t type, uint32_t batch, uint64_t record)
{
    return (uint64_t(type == RAMCRC_LOG_ENTRY_TYPE_OBJ) << 48) | (uint64_t(batch) << 32) | record;
}

// The key of record j of batch b, which claimed a slot and so is a participant.
__device__ __forceinline__ ResKey rtab_key_of_row(const RtabBatch& b, const u32x4 r)
{
    const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
    const PartRd rd{b.base + uint64_t(r.x) * b.stride + pay};
    const ramcrc_part::Parsed p = ramcrc_part::parse(r.w & 0x3f, r.z, true, rd);
    return ResKey{p.table_id, rd.pay + p.key_off, p.key_len};
}

__device__ __forceinline__ ResKey rtab_key_of(const RtabBatch& b, uint64_t j)
{
    return rtab_key_of_row(b, b.entries[j]);
}

// The version of record i of batch b, a participant.
__device__ __forceinline__ uint64_t rtab_version_of(const RtabBatch& b, const u32x4 r)
{
    const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
    return ramcrc_res::version(r.w & 0x3f, PartRd{b.base + uint64_t(r.x) * b.stride + pay});
}

// ------------------------------------------------------------- k_rtab_zero
// Create and reset: the head and every slot.
__global__ __launch_bounds__(kPartThreads) void k_rtab_zero(RtabDesc a)
{
    const uint64_t nw = kRtabSlotWords * a.nslots;
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t < kRtabHeadWords)
        a.head[t] = 0;
    for (uint64_t w = t; w < nw; w += nthr)
        a.slots[w] = 0;
}

// ------------------------------------------------------------- k_rtab_open
__global__ void k_rtab_open(RtabDesc a)
{
    if (blockIdx.x || threadIdx.x || rtab_refused(a))
        return;
    a.batches[a.batch] = a.open;
    a.bcount[a.batch] = RtabCount{};
}

// ----------------------------------------------------------- k_rtab_insert
template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_rtab_insert(RtabDesc a)
{
    if (rtab_refused(a))
        return;
    const RtabBatch& b = a.batches[a.batch];
    RtabCount& cnt = a.bcount[a.batch];
    const uint64_t ne = rtab_n_records(b);
    const uint64_t base = b.base, stride = b.stride, nseg = b.nseg;
    const u32x4* const entries = b.entries;
    const ramcrc_seg_status* const status = b.status;
    const uint64_t* const key_hash = b.key_hash;
    uint64_t* const work = b.work;
    const uint64_t mask = a.nslots - 1;
    const uint64_t my_claim = uint64_t(a.batch) << 32;
    for (uint64_t i0 = uint64_t(blockIdx.x) * kPartThreads; i0 < ne;
         i0 += uint64_t(gridDim.x) * kPartThreads) {
        const uint64_t i = i0 + threadIdx.x;
        bool is_obj = false, is_tomb = false, mal = false, claimed = false;
        if (i < ne) {
            const u32x4 r = entries[i];
            const uint32_t seg = r.x, type = r.w & 0x3f;
            uint64_t slot = kResNone;
            if (seg >= nseg) {
                rtab_refuse(a);
            } else if (status[seg].flags & RAMCRC_SEG_OK) {
                const uint64_t pay = uint64_t(r.y) + 1 + ((r.w >> 6) & 3) + 1;
                const bool readable = !(r.w & kRecOverlong) && pay + r.z <= stride;
                const PartRd rd{base + uint64_t(seg) * stride + pay};
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
                            hash = key_hash[i];
                        else
                            hash = part_key_hash(me.table_id, me.addr, me.len);
                        // linear probing, bounded by the slot count: a table
                        // within its key capacity has load <= 0.5, and one
                        // past it is spoiled whether or not a slot was found
                        uint64_t s = hash & mask;
                        for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                            unsigned long long c = __hip_atomic_load(rtab_word(a, s, 2), RTAB_RLX);
                            if (c == 0 && __hip_atomic_compare_exchange_strong(
                                              rtab_word(a, s, 2), &c,
                                              static_cast<unsigned long long>(my_claim | (i + 1)),
                                              __ATOMIC_RELAXED, RTAB_RLX)) {
                                slot = s;
                                claimed = true;
                                break;
                            }
                            // c: the claimant (the failed CAS stored it), of
                            // this batch or an earlier one; its descriptor was
                            // written before this launch
                            const ResKey k = rtab_key_of(a.batches[c >> 32], (c & 0xFFFFFFFFull) - 1);
                            if (k.table_id == me.table_id && k.len == me.len &&
                                res_bytes_equal(k.addr, me.addr, me.len)) {
                                slot = s;
                                break;
                            }
                        }
                        if (slot != kResNone) {
                            // a pick made below a version that raises the
                            // maximum is stale: none, until k_rtab_pick
                            if (__hip_atomic_fetch_max(rtab_word(a, slot, 0),
                                                       static_cast<unsigned long long>(ver),
                                                       RTAB_RLX) < ver)
                                __hip_atomic_store(rtab_word(a, slot, 1), 0ull, RTAB_RLX);
                        } else {
                            rtab_refuse(a);   // no slot: the table is full
                        }
                    }
                } else if (type == RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION && readable &&
                           r.z >= ramcrc_res::kSafeVersionBytes) {
                    __hip_atomic_fetch_max(&a.head[kRtabSafe],
                                           static_cast<unsigned long long>(rd.u64(0)), RTAB_RLX);
                }
            }
            work[i] = slot;
        }
        // the counters: one atomic per wave and counter
        const unsigned long long no = __builtin_popcountll(__ballot(is_obj));
        const unsigned long long nt = __builtin_popcountll(__ballot(is_tomb));
        const unsigned long long nm = __builtin_popcountll(__ballot(mal));
        const unsigned long long nc = __builtin_popcountll(__ballot(claimed));
        if ((threadIdx.x & (kWaveSize - 1)) == 0) {
            if (no)
                atomicAdd(&cnt.objects, no);
            if (nt)
                atomicAdd(&cnt.tombstones, nt);
            if (nm)
                atomicAdd(&cnt.malformed, nm);
            if (nc)
                atomicAdd(&a.head[kRtabKeys], nc);
        }
    }
}

// ------------------------------------------------------------- k_rtab_pick
// The slots' version maxima are final for this add.
__global__ __launch_bounds__(kPartThreads) void k_rtab_pick(RtabDesc a)
{
    if (rtab_spoiled_after_insert(a)) {
        // past the key capacity: this add spoils the table
        if (blockIdx.x == 0 && threadIdx.x == 0 && !rtab_refused(a))
            rtab_refuse(a);
        return;
    }
    const RtabBatch& b = a.batches[a.batch];
    const uint64_t ne = rtab_n_records(b);
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < ne; i += nthr) {
        const uint64_t s = b.work[i];
        if (s == kResNone)
            continue;
        const u32x4 r = b.entries[i];
        const uint64_t ver = rtab_version_of(b, r);
        if (ver != __hip_atomic_load(rtab_word(a, s, 0), RTAB_RLX))
            continue;
        const uint64_t rank = rtab_rank(r.w & 0x3f, a.batch, i);
        __hip_atomic_fetch_max(rtab_word(a, s, 1), static_cast<unsigned long long>(~rank), RTAB_RLX);
    }
}

// The winner of record i's key as the table stands: the pick's complement is
// its rank.  *type_obj: is the winner an object?
__device__ __forceinline__ uint2 rtab_winner(const RtabDesc& a, uint64_t s, bool* type_obj)
{
    if (s == kResNone)
        return make_uint2(RAMCRC_RESOLVE_NONE, RAMCRC_RESOLVE_NONE);
    const uint64_t rank = ~*rtab_word(a, s, 1);
    *type_obj = (rank >> 48) & 1;
    return make_uint2(uint32_t(rank >> 32) & 0xFFFFu, uint32_t(rank));
}

// ------------------------------------------------------------ k_rtab_tiles
__global__ __launch_bounds__(kPartThreads) void k_rtab_tiles(RtabDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const RtabBatch& b = a.batches[a.batch];
    const uint64_t ne = rtab_n_records(b);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        uint64_t v = 0;   // live tombstones << 32 | live objects
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            const uint64_t i = i0 + k;
            if (i >= ne)
                continue;
            bool obj = false;
            const uint2 w = rtab_winner(a, b.work[i], &obj);
            if (a.winner)
                a.winner[i] = w;
            if (w.x == a.batch && w.y == uint32_t(i))
                v += obj ? 1ull : 1ull << 32;
        }
        uint64_t tot;
        (void)part_block_excl(v, wsum, &tot);
        if (threadIdx.x == 0)
            a.tile_sum[tile] = tot;
    }
}

// ------------------------------------------------------------- k_rtab_scan
// One workgroup: the tile sums become exclusive sums (both halves: neither
// reaches 2^32), kPartThreads tiles a step; then the list's length and the
// counters.
__global__ __launch_bounds__(kPartThreads) void k_rtab_scan(RtabDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a)) {
        if (threadIdx.x == 0) {
            *a.n_live = 0;
            *a.counts_out = ramcrc_resolve_counts{0, 0, 0, 0, 0, 0};
        }
        return;
    }
    const RtabBatch& b = a.batches[a.batch];
    const uint64_t ne = rtab_n_records(b);
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
        *a.n_live = (carry & 0xFFFFFFFFull) + (carry >> 32);
        const RtabCount& cnt = a.bcount[a.batch];
        *a.counts_out = ramcrc_resolve_counts{cnt.objects, cnt.tombstones, carry & 0xFFFFFFFFull,
                                              carry >> 32, cnt.malformed, a.head[kRtabSafe]};
    }
}

// ------------------------------------------------------------- k_rtab_emit
__global__ __launch_bounds__(kPartThreads) void k_rtab_emit(RtabDesc a)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const RtabBatch& b = a.batches[a.batch];
    const uint64_t ne = rtab_n_records(b);
    const uint64_t ntiles = (ne + kPartTile - 1) / kPartTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kPartTile + uint64_t(threadIdx.x) * kPartPer;
        bool live[kPartPer];
        uint64_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPartPer; k++) {
            live[k] = false;
            if (i0 + k < ne) {
                bool obj = false;
                const uint2 w = rtab_winner(a, b.work[i0 + k], &obj);
                live[k] = w.x == a.batch && w.y == uint32_t(i0 + k);
            }
            v += live[k];
        }
        uint64_t tot;
        const uint64_t before = a.tile_sum[tile];
        uint64_t dst = (before & 0xFFFFFFFFull) + (before >> 32) + part_block_excl(v, wsum, &tot);
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

// ------------------------------------------------------------ k_rtab_stats
// One pass over the slots into *stats_out, which the caller zeroed: a claimed
// slot is a key, and after an add every key has a pick.
__global__ __launch_bounds__(kPartThreads) void k_rtab_stats(RtabDesc a)
{
    ramcrc_replay_table_stats* const st = a.stats_out;
    if (rtab_refused(a)) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            st->spoiled = 1;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->safe_version = a.head[kRtabSafe];
        st->batches = a.n_batches;
    }
    for (uint64_t s0 = uint64_t(blockIdx.x) * kPartThreads; s0 < a.nslots;
         s0 += uint64_t(gridDim.x) * kPartThreads) {
        const uint64_t s = s0 + threadIdx.x;
        bool key = false, obj = false;
        if (s < a.nslots && *rtab_word(a, s, 2)) {
            key = true;
            obj = (~*rtab_word(a, s, 1) >> 48) & 1;
        }
        const unsigned long long nk = __builtin_popcountll(__ballot(key));
        const unsigned long long no = __builtin_popcountll(__ballot(key && obj));
        if ((threadIdx.x & (kWaveSize - 1)) == 0 && nk) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&st->keys), nk);
            if (no)
                atomicAdd(reinterpret_cast<unsigned long long*>(&st->live_objects), no);
            if (nk - no)
                atomicAdd(reinterpret_cast<unsigned long long*>(&st->live_tombstones), nk - no);
        }
    }
}

// ----------------------------------------------------------- k_rtab_lookup
// What the table holds for a key (ramcrc_replay_table_lookup_device, DESIGN.md
// 5.13): k_rtab_insert's probe with the writes taken out.  One query per lane
// in tiles of kPartThreads; from hash & mask the lane steps to the first slot
// whose claim is 0 (absent: the table never deletes) or whose claimant's key,
// read through its batch's descriptor, equals the query's; there the pick
// names the winner, whose record -- not necessarily the claimant's -- gives
// the version and the value's place.  Every table word lies behind a kernel
// boundary and is read plainly; nothing of the table is written.  A query is
// a chain of dependent loads (query, claim, descriptor, record, key, pick,
// winner's record, its key table): residency hides it, so the kernel keeps no
// LDS in the loop and few registers.
// The counters: every lane counts its kinds in registers; at the end one
// reduction per workgroup (wave shuffles, then LDS), one atomic per nonzero
// counter on the scratch line, and the last workgroup to finish copies the
// line out, as k_sl_stamp does.
constexpr uint32_t kLookCountWords = 32;   // scratch: one 128-byte line of counters
constexpr int kLookCounters = 4;           // objects, tombstones, absent, bad; spoiled is written as 0
constexpr int kLookTicket = 8;             // counts[kLookTicket]: workgroups that have finished
static_assert(sizeof(ramcrc_lookup_key) == 24 && sizeof(ramcrc_lookup_result) == 32, "lookup ABI");
static_assert(sizeof(ramcrc_lookup_counts) == (kLookCounters + 1) * sizeof(uint64_t), "lookup counters");
static_assert((kLookTicket + 1) * sizeof(uint64_t) <= kLookCountWords * sizeof(uint32_t), "counter line");

struct LookDesc {
    uint64_t keys;                      // the caller's key buffer
    uint64_t keys_bytes;
    const uint64_t* queries;            // three words each: table id, key_off, reserved << 32 | key_len
    uint64_t nq;
    const uint64_t* key_hash;           // nullable: the caller's hashes
    u32x4* results;                     // two each
    ramcrc_lookup_counts* counts_out;   // nullable
    unsigned long long* counts;         // scratch line, zeroed by the call: counters, ticket
};

// ramcrc_lookup_counts' field of a kind.
__device__ __forceinline__ int look_counter(uint32_t kind)
{
    return kind == RAMCRC_LOOKUP_OBJECT ? 0 : kind == RAMCRC_LOOKUP_TOMBSTONE ? 1
           : kind == RAMCRC_LOOKUP_ABSENT ? 2 : 3;
}

// The winning object's payload, for a caller that goes on to read it.
struct LookHit {
    uint64_t pay;            // its address
    uint32_t len;            // its length
    ramcrc_look::Value v;    // the value's place in it
};

// A slot's words decoded, for every walk over the table between adds (the
// probe below, dev_read_hashes.inc).  The claimant of claim word c:
__device__ __forceinline__ uint32_t rtab_claim_batch(uint64_t c)
{
    return uint32_t(c >> 32);
}

__device__ __forceinline__ uint64_t rtab_claim_record(uint64_t c)
{
    return (c & 0xFFFFFFFFull) - 1;
}

// The winner a nonzero pick word names, as rtab_winner decodes it.
__device__ __forceinline__ bool rtab_pick_object(uint64_t pick)
{
    return (~pick >> 48) & 1;
}

__device__ __forceinline__ uint32_t rtab_pick_batch(uint64_t pick)
{
    return uint32_t(~pick >> 32) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t rtab_pick_record(uint64_t pick)
{
    return uint32_t(~pick);
}

// The same with the winner's row and its payload.
struct RtabWin {
    uint32_t batch, record;
    bool obj;
    u32x4 row;      // {segment, offset, length, header}
    uint32_t pay;   // the payload's offset in its segment
    PartRd rd;
};

__device__ __forceinline__ RtabWin rtab_decode_pick(const RtabDesc& a, uint64_t pick)
{
    RtabWin w;
    w.batch = rtab_pick_batch(pick);
    w.record = rtab_pick_record(pick);
    w.obj = rtab_pick_object(pick);
    const RtabBatch& b = a.batches[w.batch];
    w.row = b.entries[w.record];
    w.pay = w.row.y + 1 + ((w.row.w >> 6) & 3) + 1;
    w.rd = PartRd{b.base + uint64_t(w.row.x) * b.stride + w.pay};
    return w;
}

// Query i's answer: the probe k_rtab_lookup and k_rtab_read_size share.
template <bool kGiven>
__device__ __forceinline__ ramcrc_lookup_result rtab_probe(const RtabDesc& a, const LookDesc& q,
                                                           uint64_t i, LookHit* hit)
{
    const uint64_t mask = a.nslots - 1;
    const uint64_t table_id = q.queries[3 * i], off = q.queries[3 * i + 1];
    const uint64_t lr = q.queries[3 * i + 2];
    const uint32_t len = uint32_t(lr);
    ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
    if (ramcrc_look::bad_query(off, len, uint32_t(lr >> 32), q.keys_bytes))
        return res;
    res.kind = RAMCRC_LOOKUP_ABSENT;
    const uint64_t addr = q.keys + off;
    uint64_t hash;
    if constexpr (kGiven)
        hash = q.key_hash[i];
    else
        hash = part_key_hash(table_id, addr, len);
    // bounded by the slot count, as the insert's probe is
    uint64_t s = hash & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        const ResKey k = rtab_key_of(a.batches[rtab_claim_batch(c)], rtab_claim_record(c));
        if (k.table_id != table_id || k.len != len || !res_bytes_equal(k.addr, addr, len))
            continue;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0)   // (between adds every claimed slot has one)
            break;
        const RtabWin w = rtab_decode_pick(a, pick);
        const u32x4 r = w.row;
        res.ref = ramcrc_replay_ref{w.batch, w.record};
        res.version = ramcrc_res::version(r.w & 0x3f, w.rd);
        if (w.obj) {
            const ramcrc_look::Value v = ramcrc_look::object_value(r.z, w.rd);
            res.kind = RAMCRC_LOOKUP_OBJECT;
            res.segment = r.x;
            res.value_off = w.pay + v.off;
            res.value_len = v.len;
            *hit = LookHit{w.rd.pay, r.z, v};
        } else {
            res.kind = RAMCRC_LOOKUP_TOMBSTONE;
        }
        break;
    }
    return res;
}

__device__ __forceinline__ void look_store(const LookDesc& q, uint64_t i, const ramcrc_lookup_result& res)
{
    u32x4 lo, hi;
    lo.x = res.ref.batch;
    lo.y = res.ref.record;
    lo.z = uint32_t(res.version);
    lo.w = uint32_t(res.version >> 32);
    hi.x = res.kind;
    hi.y = res.segment;
    hi.z = res.value_off;
    hi.w = res.value_len;
    q.results[2 * i] = lo;
    q.results[2 * i + 1] = hi;
}

template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_rtab_lookup(RtabDesc a, LookDesc q)
{
    __shared__ unsigned long long wsum[kLookCounters * (kPartThreads / kWaveSize)];
    __shared__ uint32_t is_last;
    if (rtab_refused(a)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && q.counts_out)
            *q.counts_out = ramcrc_lookup_counts{0, 0, 0, 0, 1};
        return;
    }
    uint32_t cnt[kLookCounters] = {};   // (a lane takes fewer than 2^32 queries)
    for (uint64_t i0 = uint64_t(blockIdx.x) * kPartThreads; i0 < q.nq;
         i0 += uint64_t(gridDim.x) * kPartThreads) {
        const uint64_t i = i0 + threadIdx.x;
        if (i >= q.nq)
            continue;
        LookHit hit;
        const ramcrc_lookup_result res = rtab_probe<kGiven>(a, q, i, &hit);
        look_store(q, i, res);
#pragma unroll
        for (int k = 0; k < kLookCounters; k++)
            cnt[k] += look_counter(res.kind) == k;
    }
    if (!q.counts_out)
        return;
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kLookCounters; k++) {
        unsigned long long v = cnt[k];
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            v += __shfl_xor(v, d);
        if ((t & (kWaveSize - 1)) == 0)
            wsum[k * (kPartThreads / kWaveSize) + t / kWaveSize] = v;
    }
    __syncthreads();
    if (t < kLookCounters) {
        unsigned long long v = 0;
        for (int w = 0; w < kPartThreads / kWaveSize; w++)
            v += wsum[t * (kPartThreads / kWaveSize) + w];
        if (v)
            atomicAdd(&q.counts[t], v);
    }
    __syncthreads();   // this workgroup has issued its sums
    if (t == 0) {
        __threadfence();
        is_last = atomicAdd(&q.counts[kLookTicket], 1ull) + 1 == gridDim.x;
    }
    __syncthreads();
    if (is_last && t <= kLookCounters) {
        __threadfence();
        reinterpret_cast<unsigned long long*>(q.counts_out)[t] =
            t < kLookCounters ? atomicAdd(&q.counts[t], 0ull) : 0ull;   // spoiled: 0
    }
}

// ------------------------------------------------------------- k_rtab_read_*
// A multi-read's reply (ramcrc_replay_table_read_device, DESIGN.md 5.14), in
// the three launches of the live query; no workgroup waits for another:
//   k_rtab_read_size    one query per lane in tiles of kPartThreads: the
//                       lookup's probe, the status and the part's data range
//                       (read_rules.h) into four scratch words per query, and
//                       per tile the sums of the part sizes, the statuses and
//                       the value and key bytes, by one atomic per wave and sum
//                       (the call zeroes them): no barrier, as in the lookup;
//   k_rtab_read_scan    one workgroup: the tile sums become exclusive offsets;
//                       the tiles whose end lies within reply_cap count whole,
//                       the first one that does not is scanned query by query
//                       for the truncation point; then the summary;
//   k_rtab_read_gather  per tile the offsets of its parts, d_part_off, the
//                       headers and the data of the returned parts.
// The gather is k_app_copy with the sources in random order: a part's data
// goes through app_copy (aligned 16-byte stores for the destination's full
// granules, byte stores around them), by 8 lanes below kAppBigMin, by a wave
// below kAppGroupMin, by the workgroup above; the 16 header bytes, which may
// start at any byte and share granules with both neighbours, are byte stores,
// two by each of the part's 8 lanes.
constexpr uint32_t kReadRecWords = 4;    // scratch per query: source, version, length | status << 32,
                                         // value bytes | key bytes << 32
constexpr uint32_t kReadTileWords = 4;   // scratch per tile: size (then the offset), statuses, value, key bytes
constexpr int kReadStatuses = 5;         // ok, doesnt_exist, object_exists, wrong_version, bad
constexpr uint32_t kReadScanPer = 2;     // tiles per lane and step of the scan
constexpr int kReadCountBits = 12;       // a tile's count of one status: at most kPartThreads
static_assert(kPartThreads < (1 << kReadCountBits) && kReadStatuses * kReadCountBits <= 64, "tile counts");
static_assert(kAppCopyThreads == kPartThreads, "the gather posts one part per lane of a tile");
static_assert(sizeof(ramcrc_reject_rules) == 16 && sizeof(ramcrc_read_summary) == 80, "read ABI");

struct ReadDesc {
    const uint64_t* rules;          // nullable: two words a query
    uint32_t flags;
    uint64_t reply;
    uint64_t cap;
    uint64_t* part_off;             // nullable
    ramcrc_read_summary* summary;
    uint64_t* rec;                  // scratch [kReadRecWords * nq]
    uint64_t* tile;                 // scratch [kReadTileWords * tiles]
    unsigned long long* head;       // scratch line: [0] the returned queries, written by the scan
};

// ramcrc_read_summary's field of a status, from `ok` on.
__device__ __forceinline__ int read_counter(uint32_t status)
{
    return status == ramcrc_read::kStatusOk ? 0 : status == ramcrc_read::kStatusDoesntExist ? 1
           : status == ramcrc_read::kStatusExists ? 2 : status == ramcrc_read::kStatusWrongVersion ? 3 : 4;
}

// The sum of v over the workgroup, in every lane; red: kPartThreads / kWaveSize words.
__device__ __forceinline__ uint64_t rtab_block_sum(uint64_t v, uint64_t* red)
{
    unsigned long long s = v;
#pragma unroll
    for (int d = 1; d < kWaveSize; d <<= 1)
        s += __shfl_xor(s, d);
    if ((threadIdx.x & (kWaveSize - 1)) == 0)
        red[threadIdx.x / kWaveSize] = s;
    __syncthreads();
    uint64_t tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPartThreads / kWaveSize; w++)
        tot += red[w];
    __syncthreads();   // red is free again
    return tot;
}

template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_rtab_read_size(RtabDesc a, LookDesc q, ReadDesc r)
{
    namespace rr = ramcrc_read;
    if (rtab_refused(a))
        return;
    const uint64_t ntiles = (q.nq + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        uint64_t size = 0, cnt = 0, vbytes = 0, kbytes = 0;
        if (i < q.nq) {
            LookHit hit{0ull, 0u, ramcrc_look::Value{0u, 0u}};
            const ramcrc_lookup_result res = rtab_probe<kGiven>(a, q, i, &hit);
            if (q.results)
                look_store(q, i, res);
            rr::Rules ru = rr::no_rules();
            if (r.rules)
                ru = rr::Rules{r.rules[2 * i], r.rules[2 * i + 1]};
            uint64_t version = res.version;
            const uint32_t st = rr::status(rr::bad_rules(ru), res.kind, ru, &version);
            rr::Data d{0u, 0u};
            uint64_t src = 0;
            if (st == rr::kStatusOk) {
                d = rr::data_range(r.flags, hit.len, hit.v);
                src = hit.pay + d.off;
                vbytes = hit.v.len;
                kbytes = rr::key_bytes(hit.len, hit.v);
            }
            size = rr::part_size(st, d.len);
            cnt = 1ull << (kReadCountBits * read_counter(st));
            uint64_t* const rec = r.rec + kReadRecWords * i;
            rec[0] = src;
            rec[1] = version;
            rec[2] = uint64_t(d.len) | (uint64_t(st) << 32);
            rec[3] = vbytes | (kbytes << 32);
        }
        // the tile's sums, which the call zeroed: one atomic per wave and sum,
        // so that no wave waits for another, as in the lookup
        uint64_t sums[kReadTileWords] = {size, cnt, vbytes, kbytes};
#pragma unroll
        for (uint32_t k = 0; k < kReadTileWords; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kReadTileWords * tile + k), v);
        }
    }
}

// One workgroup.  Part sizes are at least 16, so the ends of the parts grow
// strictly and the returned queries are a prefix: whole tiles, then a prefix
// of one tile.
__global__ __launch_bounds__(kPartThreads) void k_rtab_read_scan(RtabDesc a, LookDesc q, ReadDesc r)
{
    namespace rr = ramcrc_read;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s;
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_read_summary sm{};
            sm.spoiled = 1;
            *r.summary = sm;
        }
        return;
    }
    const uint64_t ntiles = (q.nq + kPartThreads - 1) / kPartThreads;
    if (t == 0)
        cut_s = ntiles;
    __syncthreads();
    uint64_t carry = 0, vbytes = 0, kbytes = 0, cut = ntiles;
    uint64_t cnt[kReadStatuses] = {};
    for (uint64_t t0 = 0; t0 < ntiles; t0 += uint64_t(kPartThreads) * kReadScanPer) {
        // kReadScanPer neighbouring tiles a lane, their loads in flight together
        const uint64_t tl0 = t0 + uint64_t(t) * kReadScanPer;
        uint64_t v[kReadScanPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kReadScanPer; k++) {
            v[k] = tl0 + k < ntiles ? r.tile[kReadTileWords * (tl0 + k)] : 0ull;
            sum += v[k];
        }
        uint64_t tot;
        uint64_t base = carry + part_block_excl(sum, wsum, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kReadScanPer; k++) {
            const uint64_t tl = tl0 + k;
            if (tl >= ntiles)
                break;
            uint64_t* const ts = r.tile + kReadTileWords * tl;
            ts[0] = base;
            if (base + v[k] <= r.cap) {
                const uint64_t c = ts[1];
#pragma unroll
                for (int j = 0; j < kReadStatuses; j++)
                    cnt[j] += (c >> (kReadCountBits * j)) & ((1u << kReadCountBits) - 1);
                vbytes += ts[2];
                kbytes += ts[3];
            } else if (tl < cut) {
                cut = tl;
            }
            base += v[k];
        }
        carry += tot;
    }
    if (cut < ntiles)
        atomicMin(&cut_s, static_cast<unsigned long long>(cut));
    __syncthreads();   // the cut, and every tile's offset
    cut = cut_s;
    uint64_t returned = q.nq, bytes = carry;
    if (cut < ntiles) {
        // the tile the reply ends in: its parts one by one
        const uint64_t i = cut * kPartThreads + t;
        uint64_t size = 0, w2 = 0, w3 = 0;
        if (i < q.nq) {
            w2 = r.rec[kReadRecWords * i + 2];
            w3 = r.rec[kReadRecWords * i + 3];
            size = rr::part_size(uint32_t(w2 >> 32), uint32_t(w2));
        }
        uint64_t tot;
        const uint64_t base = r.tile[kReadTileWords * cut];
        const uint64_t off = base + part_block_excl(size, wsum, &tot);
        const bool in = i < q.nq && off + size <= r.cap;
        if (in) {
            const uint32_t st = uint32_t(w2 >> 32);
#pragma unroll
            for (int k = 0; k < kReadStatuses; k++)
                cnt[k] += read_counter(st) == k;
            if (st == rr::kStatusOk) {
                vbytes += uint32_t(w3);
                kbytes += w3 >> 32;
            }
        }
        const uint64_t n_in = rtab_block_sum(in ? 1ull : 0ull, wsum);
        returned = cut * kPartThreads + n_in;
        bytes = base + rtab_block_sum(in ? size : 0ull, wsum);
    }
    uint64_t sums[kReadStatuses + 2];
#pragma unroll
    for (int k = 0; k < kReadStatuses; k++)
        sums[k] = rtab_block_sum(cnt[k], wsum);
    sums[kReadStatuses] = rtab_block_sum(vbytes, wsum);
    sums[kReadStatuses + 1] = rtab_block_sum(kbytes, wsum);
    if (t == 0) {
        ramcrc_read_summary sm{};
        sm.returned = returned;
        sm.reply_bytes = bytes;
        sm.ok = sums[0];
        sm.doesnt_exist = sums[1];
        sm.object_exists = sums[2];
        sm.wrong_version = sums[3];
        sm.bad = sums[4];
        sm.value_bytes = sums[5];
        sm.key_bytes = sums[6];
        *r.summary = sm;
        r.head[0] = returned;
    }
}

__global__ __launch_bounds__(kPartThreads) void k_rtab_read_gather(RtabDesc a, LookDesc q, ReadDesc r)
{
    namespace rr = ramcrc_read;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];   // sdst: behind the header; 0: not returned
    __shared__ uint64_t sh0[kPartThreads], sh1[kPartThreads];     // the header's words
    __shared__ uint32_t slen[kPartThreads], sbig[kPartThreads];
    __shared__ uint32_t nbig[2];   // by tile parity, as in k_app_copy
    if (rtab_refused(a))
        return;
    const uint64_t returned = r.head[0];
    const uint64_t ntiles = (q.nq + kPartThreads - 1) / kPartThreads;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
        const uint64_t i = tile * kPartThreads + t;
        if (tile * kPartThreads >= returned) {
            // nothing of this tile is in the reply (the same for every lane)
            if (r.part_off && i < q.nq)
                r.part_off[i] = RAMCRC_READ_NONE;
            par ^= 1u;   // (no tile was posted: the parity stays)
            continue;
        }
        __syncthreads();   // the previous tile's copies have read their descriptors and its count
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        uint64_t src = 0, dst = 0, size = 0, version = 0;
        uint32_t len = 0, st = 0;
        if (i < q.nq) {
            const uint64_t* const rec = r.rec + kReadRecWords * i;
            const uint64_t w2 = rec[2];
            src = rec[0];
            version = rec[1];
            len = uint32_t(w2);
            st = uint32_t(w2 >> 32);
            size = rr::part_size(st, len);
        }
        uint64_t tot;
        const uint64_t off = r.tile[kReadTileWords * tile] + part_block_excl(size, wsum, &tot);
        // (the scan returned only parts that fit; checked again as the last
        // thing between a stale word and a stray store)
        const bool in = i < returned && off + size <= r.cap;
        if (r.part_off && i < q.nq)
            r.part_off[i] = in ? off : RAMCRC_READ_NONE;
        uint64_t h0 = 0, h1 = 0;
        if (in) {
            rr::header_words(st, version, len, &h0, &h1);
            dst = r.reply + off + rr::kPartHeader;
        } else {
            len = 0;
        }
        ssrc[t] = src;
        sdst[t] = dst;
        sh0[t] = h0;
        sh1[t] = h1;
        slen[t] = len;
        if (len >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t j = g; j < kPartThreads; j += kPartThreads / 8) {
            const uint64_t d = sdst[j];
            if (!d)
                continue;
            const uint64_t hw = sub < 4 ? sh0[j] : sh1[j];
            const uint32_t two = uint32_t(hw >> (16 * (sub & 3)));
            *reinterpret_cast<gw8*>(d - rr::kPartHeader + 2 * sub) = uint8_t(two);
            *reinterpret_cast<gw8*>(d - rr::kPartHeader + 2 * sub + 1) = uint8_t(two >> 8);
            const uint32_t L = slen[j];
            if (L && L <= kAppShortMax)
                app_copy<8, 2>(ssrc[j], d, L, sub);
            else if (L > kAppShortMax && L < kAppBigMin)
                app_copy<8, 8>(ssrc[j], d, L, sub);
        }
        const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
        for (uint32_t b = wv; b < nb; b += kPartThreads / kWaveSize) {
            const uint32_t j = sbig[b];
            if (slen[j] < kAppGroupMin)
                app_copy<kWaveSize, 4>(ssrc[j], sdst[j], slen[j], ln);
        }
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t j = sbig[b];
            if (slen[j] >= kAppGroupMin)
                app_copy<kPartThreads, 4>(ssrc[j], sdst[j], slen[j], t);
        }
    }
}

#undef RTAB_RLX

}  // namespace
