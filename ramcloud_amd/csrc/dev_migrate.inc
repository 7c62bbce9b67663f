// Migrating a tablet out of the replay table into transfer segments
// (ramcrc_replay_table_migrate_device, DESIGN.md 5.22): k_mig_size, k_mig_cut,
// k_mig_emit, k_mig_seal.  Part of ramcrc_device.hip (one translation unit);
// included only from there, after dev_clean.inc, whose list kernel, tile
// bookkeeping and block helpers it uses; not a standalone header.
//
// The listed batches' records from the start cursor on are laid out as tiles
// of kPartThreads records, batch after batch in the order given, a batch's
// tiles in record order; a tile never spans two batches.  A record's position
// is tile * kPartThreads + lane, and positions grow in log order.  The
// launches, none of which waits for another workgroup:
//   k_clean_open  the list (batch << 48 | first tile) into scratch;
//   k_mig_size    one record per lane: its class (migrate_rules.h) from its
//                 work word, its key's table id, its record hash (the batch's,
//                 or Key::getHash of the key) and, in live-only mode, its
//                 slot's pick; class and payload length into the record's
//                 scratch word; per tile the sums of entry bytes, payload
//                 bytes and classes and the first entry that fits no output,
//                 stored by the one workgroup that has the tile: no atomics;
//   k_mig_cut     one workgroup: exclusive sums over the tiles; where the call
//                 ends (the first entry that fits no output, the entry at
//                 which d_sent is full, or the end of the list); then the
//                 greedy cuts, serial in the segments: the tile that holds a
//                 cut by bisection over the tiles' sums, the record inside it
//                 by a scan of the tile's scratch words with the whole
//                 workgroup; the boundaries, the cursor and the summary;
//   k_mig_emit    per tile the offsets again from the scratch words; a sent
//                 record's segment by bisection over the boundaries; its
//                 rebuilt header bytes as byte stores, its payload with the
//                 append's granule copy as k_clean_move posts it; d_sent; per
//                 tile and segment the Crc32C of the entries' header bytes
//                 moved to the end of the segment's, folded into the
//                 segment's word by one atomic XOR (XOR commutes: the word
//                 does not depend on the order);
//   k_mig_seal    per segment the certificate from that word, the counts and
//                 the index of its first entry.
// The table is only read.  Per-record scratch words are kept (4 bytes a
// record) so that neither the cut nor the emit repeats the selection, which
// costs a work word, a slot word, a row, a key parse and perhaps a hash.

namespace {

constexpr uint32_t kMgTileWords = 8;     // scratch per tile, one 64-byte line
constexpr uint32_t kMgBoundWords = 8;    // scratch per boundary, one 64-byte line
constexpr uint32_t kMgHeadWords = 16;
static_assert(sizeof(ramcrc_migrate_count) == 16 && sizeof(ramcrc_migrate_summary) == 120, "migrate ABI");
static_assert(kPartThreads == 256, "a lane number is a position's low byte");

// A tile's line.
enum : uint32_t {
    kMgBytes = 0,     // entry bytes of the selected records (cut: of those before the tile)
    kMgPayload = 1,   // their payload bytes (cut: before the tile)
    kMgObjs = 2,      // selected objects (cut: before the tile)
    kMgTombs = 3,     // selected tombstones (cut: before the tile)
    kMgSkips = 4,     // records read | skipped_other << 16 | skipped_table << 32 | skipped_range << 48
    kMgDead = 5,      // skipped_dead | the lane of the first entry that fits no output << 16 (256: none)
    kMgBatch = 6,     // the tile's list word
    kMgIndex = 7,     // its place in the list given to the call
};

// A boundary: the position of a segment's first entry and the sums before it.
enum : uint32_t { kMgPos = 0, kMgS = 1, kMgP = 2, kMgO = 3, kMgT = 4, kMgCrc = 5 };

// The head line.
enum : uint32_t { kMgUsed = 0 };

struct MgBound {
    uint64_t pos, s, p, o, t;
};

struct MgDesc {
    uint64_t nlist;                  // listed batches from the start cursor on
    uint64_t ntiles;
    const uint64_t* list;            // scratch [nlist + 1]: batch << 48 | first tile; the last: ntiles
    uint64_t* head;                  // scratch [kMgHeadWords]
    uint64_t* bound;                 // scratch [kMgBoundWords * (max_segments + 1)]
    uint64_t* tile;                  // scratch [kMgTileWords * ntiles]
    uint32_t* rec;                   // scratch [kPartThreads * ntiles]
    uint64_t table_id, first_hash, last_hash;
    uint32_t flags;
    uint32_t start_index, start_record;
    uint32_t n_batches;              // the whole list's length: the cursor of a finished migration
    uint64_t out;
    uint64_t cap, stride;
    uint32_t max_segments;
    ramcrc_seg_cert* certs;
    ramcrc_migrate_count* counts;
    uint2* sent;                     // nullable
    uint64_t sent_cap;
    uint64_t* seg_first;             // nullable
    ramcrc_migrate_summary* summary;
};

// The list entry that has `tile` (see clean_victim_of).
__device__ __forceinline__ uint64_t mig_entry_of(const MgDesc& m, uint64_t tile)
{
    uint64_t lo = 0, hi = m.nlist;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((m.list[mid] & kClFirstMask) <= tile)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The first record of list entry e's tiles: the start cursor's batch begins at
// the tile that holds the cursor.
__device__ __forceinline__ uint64_t mig_base(const MgDesc& m, uint64_t e)
{
    return e == 0 ? uint64_t(m.start_record) & ~uint64_t(kPartThreads - 1) : 0ull;
}

// Minimum of v over the workgroup, in every lane; red: kPartThreads / kWaveSize words.
__device__ __forceinline__ uint64_t mig_block_min(uint64_t v, uint64_t* red)
{
#pragma unroll
    for (int d = 1; d < kWaveSize; d <<= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), d);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & (kWaveSize - 1)) == 0)
        red[threadIdx.x / kWaveSize] = v;
    __syncthreads();
    uint64_t x = ~0ull;
#pragma unroll
    for (uint32_t w = 0; w < kPartThreads / kWaveSize; w++)
        x = red[w] < x ? red[w] : x;
    __syncthreads();   // red is free again
    return x;
}

// ---------------------------------------------------------------- k_mig_size
__global__ __launch_bounds__(kPartThreads) void k_mig_size(RtabDesc a, MgDesc m)
{
    namespace mg = ramcrc_mig;
    namespace cl = ramcrc_clean;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < m.ntiles; tile += gridDim.x) {
        const uint64_t e = mig_entry_of(m, tile);
        const uint64_t vw = m.list[e];
        const uint32_t b = uint32_t(vw >> 48);
        const RtabBatch& vb = a.batches[b];
        const uint64_t ne = rtab_n_records(vb);
        const uint64_t i = mig_base(m, e) + (tile - (vw & kClFirstMask)) * kPartThreads + t;
        uint32_t k = mg::kNotRead, len = 0;
        if (i < ne && !(e == 0 && i < m.start_record)) {
            const uint64_t s = vb.work[i];
            const u32x4 r = vb.entries[i];
            const bool part = s != kResNone;
            uint64_t table = 0, hash = 0;
            bool winner = false;
            if (part) {
                const ResKey key = rtab_key_of_row(vb, r);
                table = key.table_id;
                if (table == m.table_id) {
                    hash = vb.key_hash ? vb.key_hash[i] : part_key_hash(key.table_id, key.addr, key.len);
                    if (m.flags & RAMCRC_MIGRATE_LIVE_ONLY)
                        winner = cl::live(s, ~*rtab_word(a, s, 1), b, i);
                }
            }
            k = mg::classify(part, r.w, table, m.table_id, hash, m.first_hash, m.last_hash, m.flags, winner);
            len = r.z;
        }
        const uint32_t w = mg::pack(k, len);
        m.rec[tile * kPartThreads + t] = w;
        const bool sel = mg::sent(k);
        const uint32_t plen = mg::packed_length(w);
        const uint64_t size = sel ? mg::entry_bytes(plen) : 0ull;
        const uint64_t skips = uint64_t(k != mg::kNotRead) | (uint64_t(k == mg::kSkippedOther) << 16) |
                               (uint64_t(k == mg::kSkippedTable) << 32) | (uint64_t(k == mg::kSkippedRange) << 48);
        const uint64_t s_bytes = rtab_block_sum(size, wsum);
        const uint64_t s_pay = rtab_block_sum(sel ? plen : 0u, wsum);
        const uint64_t s_cnt = rtab_block_sum(uint64_t(k == mg::kSentObject) | (uint64_t(k == mg::kSentTombstone) << 32), wsum);
        const uint64_t s_skips = rtab_block_sum(skips, wsum);
        const uint64_t s_dead = rtab_block_sum(k == mg::kSkippedDead, wsum);
        const uint64_t big = mig_block_min(sel && mg::too_large(size, m.cap) ? t : kPartThreads, wsum);
        if (t == 0) {
            uint64_t* const ts = m.tile + kMgTileWords * tile;
            ts[kMgBytes] = s_bytes;
            ts[kMgPayload] = s_pay;
            ts[kMgObjs] = s_cnt & 0xFFFFFFFFull;
            ts[kMgTombs] = s_cnt >> 32;
            ts[kMgSkips] = s_skips;
            ts[kMgDead] = s_dead | (big << 16);
            ts[kMgBatch] = vw;
            ts[kMgIndex] = m.start_index + e;
        }
    }
}

// ----------------------------------------------------------------- k_mig_cut
// What the in-tile search looks for.
enum : uint32_t {
    kMgAtLane = 0,    // the record at lane `arg`
    kMgAtCount = 1,   // the selected record with `arg` selected records before it (from the start)
    kMgPastBytes = 2, // the first selected record that ends behind byte `arg` (from the start)
};

// The boundary at the record of `tile` that `mode` names, in every lane;
// false: the tile has none.  sb: 6 words of LDS.
__device__ __forceinline__ bool mig_in_tile(const MgDesc& m, uint64_t tile, uint32_t mode, uint64_t arg,
                                            uint64_t* wsum, uint64_t* sb, MgBound* out)
{
    namespace mg = ramcrc_mig;
    const uint32_t t = threadIdx.x;
    const uint64_t* const ts = m.tile + kMgTileWords * tile;
    const uint32_t w = m.rec[tile * kPartThreads + t];
    const uint32_t k = mg::packed_class(w);
    const bool sel = mg::sent(k);
    const uint64_t size = sel ? mg::entry_bytes(mg::packed_length(w)) : 0ull;
    // (a tile's bytes stay below 2^38, its counts below 2^9)
    uint64_t tot;
    const uint64_t exa = part_block_excl(size | (uint64_t(k == mg::kSentObject) << 40) |
                                             (uint64_t(k == mg::kSentTombstone) << 50), wsum, &tot);
    const uint64_t exp = part_block_excl(sel ? mg::packed_length(w) : 0u, wsum, &tot);
    MgBound me;
    me.pos = tile * kPartThreads + t;
    me.s = ts[kMgBytes] + (exa & ((1ull << 40) - 1));
    me.p = ts[kMgPayload] + exp;
    me.o = ts[kMgObjs] + ((exa >> 40) & 0x3FF);
    me.t = ts[kMgTombs] + (exa >> 50);
    bool hit;
    if (mode == kMgAtLane)
        hit = t == arg;
    else if (mode == kMgAtCount)
        hit = sel && me.o + me.t == arg;
    else
        hit = sel && me.s + size > arg;
    const uint64_t first = mig_block_min(hit ? t : kPartThreads, wsum);
    if (first == t) {
        sb[0] = me.pos;
        sb[1] = me.s;
        sb[2] = me.p;
        sb[3] = me.o;
        sb[4] = me.t;
    }
    __syncthreads();
    if (first < kPartThreads)
        *out = MgBound{sb[0], sb[1], sb[2], sb[3], sb[4]};
    __syncthreads();   // sb is free again
    return first < kPartThreads;
}

// The first tile at or behind `lo` whose sum `word`, the tile included, is
// above `limit`; ntiles: none.  tot: the sum over all tiles.  The same in
// every lane.
__device__ __forceinline__ uint64_t mig_tile_past(const MgDesc& m, uint32_t word, uint32_t word2, uint64_t limit,
                                                  uint64_t tot, uint64_t lo)
{
    uint64_t hi = m.ntiles;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        uint64_t inc = tot;
        if (mid + 1 < m.ntiles) {
            const uint64_t* const ts = m.tile + kMgTileWords * (mid + 1);
            inc = ts[word] + (word2 ? ts[word2] : 0ull);
        }
        if (inc > limit)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kPartThreads) void k_mig_cut(RtabDesc a, MgDesc m)
{
    namespace mg = ramcrc_mig;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t sb[6];
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_migrate_summary sm{};
            sm.spoiled = 1;
            *m.summary = sm;
            m.head[kMgUsed] = 0;
        }
        return;
    }
    // exclusive sums over the tiles; the first tile with an entry that fits no output
    uint64_t carry[4] = {};
    uint64_t bigtile = m.ntiles;
    for (uint64_t tl0 = 0; tl0 < m.ntiles; tl0 += kPartThreads) {
        const uint64_t tl = tl0 + t;
        uint64_t v[4] = {};
        uint64_t* const ts = m.tile + kMgTileWords * tl;
        if (tl < m.ntiles) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[k] = ts[k];
            if ((ts[kMgDead] >> 16) < kPartThreads && tl < bigtile)
                bigtile = tl;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint64_t tot;
            const uint64_t ex = carry[k] + part_block_excl(v[k], wsum, &tot);
            carry[k] += tot;
            if (tl < m.ntiles)
                ts[k] = ex;
        }
    }
    bigtile = mig_block_min(bigtile, wsum);
    __syncthreads();   // every tile's sums before it
    const uint64_t all_pos = m.ntiles * kPartThreads, all_cnt = carry[kMgObjs] + carry[kMgTombs];
    const MgBound all{all_pos, carry[kMgBytes], carry[kMgPayload], carry[kMgObjs], carry[kMgTombs]};
    // where the call ends at the latest
    MgBound big = all, full = all;
    if (bigtile < m.ntiles)
        (void)mig_in_tile(m, bigtile, kMgAtLane, m.tile[kMgTileWords * bigtile + kMgDead] >> 16, wsum, sb, &big);
    if (m.sent && m.sent_cap < all_cnt) {
        const uint64_t tl = mig_tile_past(m, kMgObjs, kMgTombs, m.sent_cap, all_cnt, 0);
        if (tl < m.ntiles)
            (void)mig_in_tile(m, tl, kMgAtCount, m.sent_cap, wsum, sb, &full);
    }
    const bool by_big = big.pos <= full.pos;
    const MgBound last = by_big ? big : full;
    // the first entry sent, then the greedy cuts
    MgBound cur = all;
    if (all_cnt) {
        const uint64_t tl = mig_tile_past(m, kMgObjs, kMgTombs, 0, all_cnt, 0);
        if (tl < m.ntiles)
            (void)mig_in_tile(m, tl, kMgAtCount, 0, wsum, sb, &cur);
    }
    if (cur.pos > last.pos)
        cur = last;
    uint32_t used = 0;
    if (t == 0) {
        uint64_t* const bd = m.bound;
        bd[kMgPos] = cur.pos;
        bd[kMgS] = cur.s;
        bd[kMgP] = cur.p;
        bd[kMgO] = cur.o;
        bd[kMgT] = cur.t;
        bd[kMgCrc] = 0;
    }
    while (used < m.max_segments && cur.o + cur.t < last.o + last.t) {
        // (the entry at cur fits an empty output: it lies before `last`)
        const uint64_t limit = cur.s + m.cap;
        MgBound nxt = all;
        const uint64_t tl = mig_tile_past(m, kMgBytes, 0, limit, carry[kMgBytes], cur.pos / kPartThreads);
        if (tl < m.ntiles)
            (void)mig_in_tile(m, tl, kMgPastBytes, limit, wsum, sb, &nxt);
        if (nxt.pos > last.pos)
            nxt = last;
        used++;
        if (t == 0) {
            uint64_t* const bd = m.bound + uint64_t(kMgBoundWords) * used;
            bd[kMgPos] = nxt.pos;
            bd[kMgS] = nxt.s;
            bd[kMgP] = nxt.p;
            bd[kMgO] = nxt.o;
            bd[kMgT] = nxt.t;
            bd[kMgCrc] = 0;
        }
        cur = nxt;
    }
    // the call ends at `last` when nothing is left to send before it; else the
    // outputs are full and it ends before the entry at cur
    const bool to_last = cur.o + cur.t == last.o + last.t;
    const MgBound end = to_last ? last : cur;
    // what was read before the end: whole tiles, then the records of its tile
    const uint64_t etile = end.pos / kPartThreads, elane = end.pos % kPartThreads;
    uint64_t skips[5] = {};   // read, other, table, range, dead
    for (uint64_t tl = t; tl < etile; tl += kPartThreads) {
        const uint64_t* const ts = m.tile + kMgTileWords * tl;
        const uint64_t s = ts[kMgSkips];
        skips[0] += s & 0xFFFF;
        skips[1] += (s >> 16) & 0xFFFF;
        skips[2] += (s >> 32) & 0xFFFF;
        skips[3] += s >> 48;
        skips[4] += ts[kMgDead] & 0xFFFF;
    }
    if (etile < m.ntiles && t < elane) {
        const uint32_t k = mg::packed_class(m.rec[etile * kPartThreads + t]);
        skips[0] += k != mg::kNotRead;
        skips[1] += k == mg::kSkippedOther;
        skips[2] += k == mg::kSkippedTable;
        skips[3] += k == mg::kSkippedRange;
        skips[4] += k == mg::kSkippedDead;
    }
    uint64_t sums[5];
#pragma unroll
    for (int k = 0; k < 5; k++)
        sums[k] = rtab_block_sum(skips[k], wsum);
    if (t != 0)
        return;
    ramcrc_migrate_summary sm{};
    if (end.pos >= all_pos) {
        sm.next_index = m.n_batches;
        sm.next_record = 0;
        sm.done = 1;
    } else {
        const uint64_t* const ts = m.tile + kMgTileWords * etile;
        const uint64_t e = ts[kMgIndex] - m.start_index;
        sm.next_index = ts[kMgIndex];
        sm.next_record = mig_base(m, e) + (etile - (ts[kMgBatch] & kClFirstMask)) * kPartThreads + elane;
        sm.too_large = to_last && by_big;
    }
    sm.segments_used = used;
    sm.sent_objects = end.o;
    sm.sent_tombstones = end.t;
    sm.sent_bytes = end.s;
    sm.payload_bytes = end.p;
    sm.records_read = sums[0];
    sm.skipped_other = sums[1];
    sm.skipped_table = sums[2];
    sm.skipped_range = sums[3];
    sm.skipped_dead = sums[4];
    *m.summary = sm;
    m.head[kMgUsed] = used;
}

// The segment of position pos: the last boundary at or before it; used > 0.
__device__ __forceinline__ uint32_t mig_segment_of(const MgDesc& m, uint32_t used, uint64_t pos)
{
    uint32_t lo = 0, hi = used;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (m.bound[uint64_t(kMgBoundWords) * mid + kMgPos] <= pos)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- k_mig_emit
__global__ __launch_bounds__(kPartThreads) void k_mig_emit(RtabDesc a, MgDesc m)
{
    namespace mg = ramcrc_mig;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint32_t t0[256];
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];
    __shared__ uint32_t slen[kPartThreads], sbig[kPartThreads];
    __shared__ uint32_t nbig[2];   // by tile parity, as in k_app_copy
    if (rtab_refused(a))
        return;
    const uint32_t used = uint32_t(m.head[kMgUsed]);
    if (used == 0 || used > m.max_segments)
        return;
    const uint32_t t = threadIdx.x;
    t0[t] = g_tab.t0.t[t];
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    const uint64_t pos0 = m.bound[kMgPos], pos1 = m.bound[uint64_t(kMgBoundWords) * used + kMgPos];
    const uint64_t cnt0 = m.bound[kMgO] + m.bound[kMgT];
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < m.ntiles; tile += gridDim.x) {
        // (the same for every lane) nothing of this tile is sent
        if ((tile + 1) * kPartThreads <= pos0 || tile * kPartThreads >= pos1)
            continue;
        __syncthreads();   // the previous tile's copies have read their descriptors and its count
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        const uint64_t* const ts = m.tile + kMgTileWords * tile;
        const uint64_t pos = tile * kPartThreads + t;
        const uint32_t w = m.rec[pos];
        const uint32_t k = mg::packed_class(w);
        const bool sel = mg::sent(k);
        const uint32_t len = mg::packed_length(w);
        const uint64_t size = sel ? mg::entry_bytes(len) : 0ull;
        uint64_t tot;
        const uint64_t exa = part_block_excl(size | (uint64_t(sel) << 40), wsum, &tot);
        const uint64_t exp = part_block_excl(sel ? len : 0u, wsum, &tot);
        const uint64_t s = ts[kMgBytes] + (exa & ((1ull << 40) - 1));
        const uint64_t meta = s - (ts[kMgPayload] + exp);          // header bytes sent before this entry
        const uint64_t j = ts[kMgObjs] + ts[kMgTombs] + (exa >> 40) - cnt0;
        const bool in = sel && pos >= pos0 && pos < pos1;
        // the tile's segments: those of its first and last sent position
        const uint64_t pa = tile * kPartThreads > pos0 ? tile * kPartThreads : pos0;
        const uint64_t pb = (tile + 1) * kPartThreads < pos1 ? (tile + 1) * kPartThreads - 1 : pos1 - 1;
        const uint32_t ka = mig_segment_of(m, used, pa), kb = mig_segment_of(m, used, pb);
        uint32_t seg = ka, piece = 0;
        uint64_t src = 0, dst = 0;
        uint32_t clen = 0;
        if (in) {
            seg = ka == kb ? ka : mig_segment_of(m, used, pos);
            const uint64_t* const b0 = m.bound + uint64_t(kMgBoundWords) * seg;
            const uint64_t* const b1 = b0 + kMgBoundWords;
            const uint64_t off = s - b0[kMgS];
            const uint32_t nm = mg::meta_bytes(len);
            // (the cut let the entry in only where it fits; checked again as
            // the last thing between a stale word and a stray store)
            if (off + size <= m.cap && seg < m.max_segments) {
                const uint64_t vw = ts[kMgBatch];
                const uint32_t b = uint32_t(vw >> 48);
                const RtabBatch& vb = a.batches[b];
                const uint64_t e = ts[kMgIndex] - m.start_index;
                const uint64_t i = mig_base(m, e) + (tile - (vw & kClFirstMask)) * kPartThreads + t;
                const u32x4 r = vb.entries[i];
                const uint32_t type = r.w & 0x3f;
                const uint64_t at = m.out + uint64_t(seg) * m.stride + off;
                uint32_t x = 0;
                for (uint32_t q = 0; q < nm; q++) {
                    const uint32_t byte = mg::meta_byte(type, len, q);
                    *reinterpret_cast<gw8*>(at + q) = uint8_t(byte);
                    x = t0[(x ^ byte) & 0xFF] ^ (x >> 8);
                }
                // the header's checksum, moved to the end of the segment's header bytes
                const uint64_t meta_end = b1[kMgS] - b1[kMgP];
                const uint32_t behind = uint32_t(meta_end - meta) - nm;
                piece = behind ? mulmod_dev(x, sl_xpow8(behind)) : x;
                src = vb.base + uint64_t(r.x) * vb.stride + r.y + 1 + ((r.w >> 6) & 3) + 1;
                dst = at + nm;
                clen = len;
                if (m.sent && j < m.sent_cap)
                    m.sent[j] = make_uint2(b, uint32_t(i));
            }
        }
        ssrc[t] = src;
        sdst[t] = dst;
        slen[t] = clen;
        if (clen >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        for (uint32_t q = ka; q <= kb; q++) {
            const uint32_t x = clean_block_xor(in && seg == q ? piece : 0u, wsum);
            if (t == 0 && x)
                atomicXor(reinterpret_cast<unsigned int*>(m.bound + uint64_t(kMgBoundWords) * q + kMgCrc), x);
        }
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t q = g; q < kPartThreads; q += kPartThreads / 8) {
            const uint32_t L = slen[q];
            if (L && L <= kAppShortMax)
                app_copy<8, 2>(ssrc[q], sdst[q], L, sub);
            else if (L > kAppShortMax && L < kAppBigMin)
                app_copy<8, 8>(ssrc[q], sdst[q], L, sub);
        }
        const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
        for (uint32_t q = wv; q < nb; q += kPartThreads / kWaveSize) {
            const uint32_t u = sbig[q];
            if (slen[u] < kAppGroupMin)
                app_copy<kWaveSize, 4>(ssrc[u], sdst[u], slen[u], ln);
        }
        for (uint32_t q = 0; q < nb; q++) {
            const uint32_t u = sbig[q];
            if (slen[u] >= kAppGroupMin)
                app_copy<kPartThreads, 4>(ssrc[u], sdst[u], slen[u], t);
        }
        par ^= 1u;
    }
}

// ---------------------------------------------------------------- k_mig_seal
// One lane per segment.
__global__ __launch_bounds__(kPartThreads) void k_mig_seal(RtabDesc a, MgDesc m)
{
    if (rtab_refused(a))
        return;
    const uint32_t used = uint32_t(m.head[kMgUsed]);
    if (used > m.max_segments)
        return;
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < used; k += nthr) {
        const uint64_t* const b0 = m.bound + uint64_t(kMgBoundWords) * k;
        const uint64_t* const b1 = b0 + kMgBoundWords;
        const uint32_t head = uint32_t(b1[kMgS] - b0[kMgS]);
        const uint32_t meta = uint32_t((b1[kMgS] - b1[kMgP]) - (b0[kMgS] - b0[kMgP]));
        // Segment::getAppendedLength: a fresh Crc32C moved behind the header
        // bytes, the entries' header bytes, the 4 head bytes, finalized
        uint32_t x = uint32_t(b0[kMgCrc]) ^ (meta ? mulmod_dev(0xFFFFFFFFu, sl_xpow8(meta)) : 0xFFFFFFFFu);
        for (int q = 0; q < 4; q++)
            x = g_tab.t0.t[(x ^ (head >> (8 * q))) & 0xFF] ^ (x >> 8);
        m.certs[k] = ramcrc_seg_cert{head, ~x};
        const uint32_t no = uint32_t(b1[kMgO] - b0[kMgO]), nt = uint32_t(b1[kMgT] - b0[kMgT]);
        m.counts[k] = ramcrc_migrate_count{no + nt, no, nt, 0u};
        if (m.seg_first)
            m.seg_first[k] = (b0[kMgO] + b0[kMgT]) - (m.bound[kMgO] + m.bound[kMgT]);
    }
}

}  // namespace
