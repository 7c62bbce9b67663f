// An indexed read's reply (ramcrc_replay_table_read_hashes_device, DESIGN.md
// 5.19): k_rh_size, k_rh_scan, k_rh_gather, k_rh_several.  Part of ramcrc_device.hip (one
// translation unit); included only from there, after dev_replay_table.inc,
// whose table, slot decoding and sums it uses; not a standalone header.
//
// The launch shape is the multi-read's, with a short fourth launch for the
// rare hash that has several objects; no workgroup waits for another:
//   k_rh_size    one asked hash per lane in tiles of kPartThreads: the chain
//                from the hash's home slot to the first unclaimed one; a
//                claimed slot matches when its claimant's table id and record
//                hash are the asked ones (the hash from the claimant's batch
//                where that was added with hashes, else Key::getHash of the
//                claimant's key); per hash into scratch the bytes of its
//                parts, its objects and tombstones, value and key bytes, and
//                the source and version of an only object; per tile their
//                sums, by one atomic per wave and sum (the call zeroes them),
//                and how many of its hashes have several objects;
//   k_rh_scan    one workgroup: the tile sums become exclusive offsets; the
//                tiles that end within both limits count whole, the first one
//                that does not is scanned hash by hash for the cut
//                (read_hashes_rules.h); then the summary;
//   k_rh_gather  per tile the offsets of its hashes, d_parts, and the parts
//                of the returned hashes: every lane posts its hash's only
//                object, and the tile copies what was posted as
//                k_rtab_read_gather does (app_copy and its size classes; the
//                12 header bytes, which may begin at any byte, as byte
//                stores).  A hash with one object -- the common case: more
//                need equal 64-bit hashes -- posts what k_rh_size left in
//                scratch and walks no chain here; a hash with several is
//                left out;
//   k_rh_several the hashes with several objects, tile by tile where k_rh_size
//                counted one: the hash's lane walks its chain once an object
//                for the smallest winner {batch, record} above the last one
//                it sent, so the order does not depend on the slots' and no
//                list is kept in registers, and copies the part itself.

namespace {

constexpr uint32_t kRhRecWords = 6;    // scratch per hash: bytes, objects | tombstones << 32, value
                                       // bytes, key bytes, an only object's source (with several
                                       // objects: the gather's offset for k_rh_several) and version
constexpr uint32_t kRhTileWords = 6;   // a tile's sums: bytes (then the offset), objects, tombstones,
                                       // empty hashes, value bytes, key bytes
constexpr uint32_t kRhTileSeveral = 6; // behind them: the tile's hashes with several objects
constexpr uint32_t kRhTileStride = 8;  // scratch words per tile: one 64-byte line, which no other tile's
                                       // atomics share
constexpr uint32_t kRhScanPer = 2;     // tiles per lane and step of the scan
static_assert(sizeof(ramcrc_hash_part) == 16 && sizeof(ramcrc_read_hashes_summary) == 72, "read-hashes ABI");
static_assert(kAppCopyThreads == kPartThreads, "the gather posts one part per lane of a tile");

struct RhDesc {
    uint64_t table_id;
    const uint64_t* hashes;
    uint64_t nq;
    uint64_t reply;
    uint64_t cap;                   // reply_capacity
    uint64_t max_length;
    uint64_t* parts;                // nullable: two words a hash
    ramcrc_read_hashes_summary* summary;
    uint64_t* rec;                  // scratch [kRhRecWords * nq]
    uint64_t* tile;                 // scratch [kRhTileStride * tiles]
    unsigned long long* head;       // scratch line: [0] the returned hashes, written by the scan
};

// Does the slot claimed by c hold a key of table_id whose record hash is
// wanted?  *hash: the record hash, where the answer is yes.  The decoding and
// the record-hash test of every walk that goes by hashes (the one below,
// dev_enumerate.inc); `wanted` is the walk's own test of the hash.
template <typename Wanted>
__device__ __forceinline__ bool rh_claimant(const RtabDesc& a, uint64_t table_id, uint64_t c,
                                            const Wanted& wanted, uint64_t* hash)
{
    const RtabBatch& b = a.batches[rtab_claim_batch(c)];
    const uint64_t j = rtab_claim_record(c);
    if (b.key_hash) {
        // The record's row and its hash are loaded together: a chain is short,
        // and the slot that matches needs both.  `row.z == 0` below is never
        // true (a claimant is a participant: its payload has at least 25
        // bytes) and guards nothing.  It is there for the schedule alone:
        // with the row in the test, the compiler cannot move the row's load
        // behind the branch on the hash, where it would wait for it.
        const u32x4 row = b.entries[j];
        const uint64_t kh = b.key_hash[j];
        if (!wanted(kh) | (row.z == 0))
            return false;
        *hash = kh;
        return rtab_key_of_row(b, row).table_id == table_id;
    }
    const ResKey k = rtab_key_of(b, j);
    if (k.table_id != table_id)
        return false;
    *hash = part_key_hash(k.table_id, k.addr, k.len);
    return wanted(*hash);
}

struct RhIs {
    uint64_t h;
    __device__ __forceinline__ bool operator()(uint64_t kh) const { return kh == h; }
};

// The same for one asked hash h.
__device__ __forceinline__ bool rh_matches(const RtabDesc& a, uint64_t table_id, uint64_t h, uint64_t c)
{
    uint64_t kh;
    return rh_claimant(a, table_id, c, RhIs{h}, &kh);
}

// What hash h finds on its chain; *src and *version: of the last object met
// (the only one when there is one).
__device__ __forceinline__ ramcrc_rh::Found rh_find(const RtabDesc& a, uint64_t table_id, uint64_t h,
                                                    uint64_t* src, uint64_t* version)
{
    namespace rh = ramcrc_rh;
    rh::Found f = rh::nothing();
    const uint64_t mask = a.nslots - 1;
    uint64_t s = h & mask;
    // bounded by the slot count, as the insert's probe is
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        if (!rh_matches(a, table_id, h, c))
            continue;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0)   // (between adds every claimed slot has one)
            continue;
        if (!rtab_pick_object(pick)) {
            f.tombstones++;
            continue;
        }
        const RtabWin w = rtab_decode_pick(a, pick);
        rh::add_object(&f, w.row.z, ramcrc_look::object_value(w.row.z, w.rd));
        *src = w.rd.pay + rh::kObjHeader;
        *version = ramcrc_res::version(w.row.w & 0x3f, w.rd);
    }
    return f;
}

// The object of hash h with the smallest order at or above `from`; false:
// there is none.  *len: its data bytes.
__device__ __forceinline__ bool rh_next(const RtabDesc& a, uint64_t table_id, uint64_t h, uint64_t from,
                                        uint64_t* order, uint64_t* src, uint64_t* version, uint32_t* len)
{
    namespace rh = ramcrc_rh;
    const uint64_t mask = a.nslots - 1;
    uint64_t s = h & mask, best = ~0ull, best_pick = 0;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0 || !rtab_pick_object(pick))
            continue;
        const uint64_t o = rh::order_of(rtab_pick_batch(pick), rtab_pick_record(pick));
        if (o < from || o >= best || !rh_matches(a, table_id, h, c))
            continue;
        best = o;
        best_pick = pick;
    }
    if (best_pick == 0)
        return false;
    const RtabWin w = rtab_decode_pick(a, best_pick);
    *order = best;
    *src = w.rd.pay + rh::kObjHeader;
    *version = ramcrc_res::version(w.row.w & 0x3f, w.rd);
    *len = rh::data_len(w.row.z);
    return true;
}

// ---------------------------------------------------------------- k_rh_size
__global__ __launch_bounds__(kPartThreads) void k_rh_size(RtabDesc a, RhDesc r)
{
    namespace rh = ramcrc_rh;
    if (rtab_refused(a))
        return;
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        rh::Found f = rh::nothing();
        uint64_t empty = 0;
        if (i < r.nq) {
            uint64_t src = 0, version = 0;
            f = rh_find(a, r.table_id, r.hashes[i], &src, &version);
            empty = f.objects == 0;
            uint64_t* const rec = r.rec + kRhRecWords * i;
            rec[0] = f.bytes;
            rec[1] = f.objects | (f.tombstones << 32);
            rec[2] = f.value_bytes;
            rec[3] = f.key_bytes;
            rec[4] = src;
            rec[5] = version;
        }
        // the tile's sums, which the call zeroed: one atomic per wave and sum,
        // so that no wave waits for another, as in the multi-read
        uint64_t sums[kRhTileWords] = {f.bytes, f.objects, f.tombstones, empty, f.value_bytes, f.key_bytes};
#pragma unroll
        for (uint32_t k = 0; k < kRhTileWords; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kRhTileStride * tile + k), v);
        }
        // (rare: equal 64-bit hashes) the tile has work for k_rh_several
        if (f.objects > 1)
            atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kRhTileStride * tile + kRhTileSeveral), 1ull);
    }
}

// ---------------------------------------------------------------- k_rh_scan
// One workgroup.  Starts and ends of the hashes' parts grow with the index, so
// the returned hashes are a prefix: whole tiles, then a prefix of one tile.
__global__ __launch_bounds__(kPartThreads) void k_rh_scan(RtabDesc a, RhDesc r)
{
    namespace rh = ramcrc_rh;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s;
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_read_hashes_summary sm{};
            sm.spoiled = 1;
            *r.summary = sm;
        }
        return;
    }
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    if (t == 0)
        cut_s = ntiles;
    __syncthreads();
    uint64_t carry = 0, cut = ntiles;
    uint64_t cnt[kRhTileWords - 1] = {};   // objects, tombstones, empty, value bytes, key bytes
    for (uint64_t t0 = 0; t0 < ntiles; t0 += uint64_t(kPartThreads) * kRhScanPer) {
        // kRhScanPer neighbouring tiles a lane, their loads in flight together
        const uint64_t tl0 = t0 + uint64_t(t) * kRhScanPer;
        uint64_t v[kRhScanPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRhScanPer; k++) {
            v[k] = tl0 + k < ntiles ? r.tile[kRhTileStride * (tl0 + k)] : 0ull;
            sum += v[k];
        }
        uint64_t tot;
        uint64_t base = carry + part_block_excl(sum, wsum, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kRhScanPer; k++) {
            const uint64_t tl = tl0 + k;
            if (tl >= ntiles)
                break;
            uint64_t* const ts = r.tile + kRhTileStride * tl;
            ts[0] = base;
            if (rh::run_returned(base + v[k], r.max_length, r.cap)) {
#pragma unroll
                for (uint32_t j = 1; j < kRhTileWords; j++)
                    cnt[j - 1] += ts[j];
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
    // (a tile behind the cut has counted nothing: the ends grow with the index)
    uint64_t returned = r.nq, bytes = carry;
    if (cut < ntiles) {
        // the tile the reply ends in: its hashes one by one
        const uint64_t i = cut * kPartThreads + t;
        uint64_t size = 0, w1 = 0, vb = 0, kb = 0;
        if (i < r.nq) {
            const uint64_t* const rec = r.rec + kRhRecWords * i;
            size = rec[0];
            w1 = rec[1];
            vb = rec[2];
            kb = rec[3];
        }
        uint64_t tot;
        const uint64_t base = r.tile[kRhTileStride * cut];
        const uint64_t off = base + part_block_excl(size, wsum, &tot);
        const bool in = i < r.nq && rh::returned(off, off + size, r.max_length, r.cap);
        if (in) {
            cnt[0] += uint32_t(w1);
            cnt[1] += w1 >> 32;
            cnt[2] += uint32_t(w1) == 0;
            cnt[3] += vb;
            cnt[4] += kb;
        }
        returned = cut * kPartThreads + rtab_block_sum(in ? 1ull : 0ull, wsum);
        bytes = base + rtab_block_sum(in ? size : 0ull, wsum);
    }
    uint64_t sums[kRhTileWords - 1];
#pragma unroll
    for (uint32_t k = 0; k < kRhTileWords - 1; k++)
        sums[k] = rtab_block_sum(cnt[k], wsum);
    if (t == 0) {
        ramcrc_read_hashes_summary sm{};
        sm.hashes = returned;
        sm.objects = sums[0];
        // the objects of the first hash that is not returned stay counted in
        // the reference's numObjects (:242 is not undone at :260)
        sm.objects_counted = sums[0] + (returned < r.nq ? uint32_t(r.rec[kRhRecWords * returned + 1]) : 0u);
        sm.reply_bytes = bytes;
        sm.value_bytes = sums[3];
        sm.key_bytes = sums[4];
        sm.empty = sums[2];
        sm.tombstones = sums[1];
        *r.summary = sm;
        r.head[0] = returned;
    }
}

// -------------------------------------------------------------- k_rh_gather
__global__ __launch_bounds__(kPartThreads) void k_rh_gather(RtabDesc a, RhDesc r)
{
    namespace rh = ramcrc_rh;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];   // sdst: behind the header; 0: nothing posted
    __shared__ uint64_t sver[kPartThreads];
    __shared__ uint32_t slen[kPartThreads], sbig[kPartThreads];
    __shared__ uint32_t nbig[2];   // by tile parity, as in k_app_copy
    if (rtab_refused(a))
        return;
    const uint64_t returned = r.head[0];
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
        const uint64_t i = tile * kPartThreads + t;
        if (tile * kPartThreads >= returned) {
            // nothing of this tile is in the reply (the same for every lane)
            if (r.parts && i < r.nq) {
                r.parts[2 * i] = RAMCRC_READ_NONE;
                r.parts[2 * i + 1] = 0;
            }
            par ^= 1u;   // (no tile was posted: the parity stays)
            continue;
        }
        __syncthreads();   // the previous tile's copies have read their descriptors and its count
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        uint64_t size = 0;
        uint32_t k = 0;
        if (i < r.nq) {
            size = r.rec[kRhRecWords * i];
            k = uint32_t(r.rec[kRhRecWords * i + 1]);
        }
        uint64_t tot;
        const uint64_t off = r.tile[kRhTileStride * tile] + part_block_excl(size, wsum, &tot);
        // (the scan returned only hashes whose parts fit; checked again as the
        // last thing between a stale word and a stray store)
        const bool in = i < returned && off + size <= r.cap;
        if (r.parts && i < r.nq) {
            r.parts[2 * i] = in ? off : RAMCRC_READ_NONE;
            r.parts[2 * i + 1] = in ? k : 0u;
        }
        // a lane whose hash has one object posts it as k_rh_size left it; a
        // hash with several is k_rh_several's, which finds its place (~0: it
        // is not returned) where an only object's source would stand
        if (k > 1)
            r.rec[kRhRecWords * i + 4] = in ? off : ~0ull;
        uint64_t dst = 0, src = 0, version = 0;
        uint32_t len = 0;
        if (in && k == 1) {
            src = r.rec[kRhRecWords * i + 4];
            version = r.rec[kRhRecWords * i + 5];
            len = uint32_t(size - rh::kPartHeader);
            dst = r.reply + off + rh::kPartHeader;
        }
        ssrc[t] = src;
        sdst[t] = dst;
        sver[t] = version;
        slen[t] = len;
        if (len >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t j = g; j < kPartThreads; j += kPartThreads / 8) {
            const uint64_t d = sdst[j];
            if (!d)
                continue;
            const uint32_t L = slen[j];
            if (sub < rh::kPartHeader / 2) {
                const uint64_t v = sver[j];
                *reinterpret_cast<gw8*>(d - rh::kPartHeader + 2 * sub) = rh::header_byte(v, L, 2 * sub);
                *reinterpret_cast<gw8*>(d - rh::kPartHeader + 2 * sub + 1) = rh::header_byte(v, L, 2 * sub + 1);
            }
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

// ------------------------------------------------------------- k_rh_several
// The parts of the hashes with several objects, which the gather left out: a
// kernel of its own, so that the gather's copy loops keep no register for this
// rare path.  A tile without such a hash (k_rh_size counted them) costs its
// workgroup one word; in a tile with one, the gather has left every such hash
// its place in the hash's scratch words, and the hash's lane writes its parts
// itself: one walk per object, then its 12 header bytes and its data.
__global__ __launch_bounds__(kPartThreads) void k_rh_several(RtabDesc a, RhDesc r)
{
    namespace rh = ramcrc_rh;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    if (rtab_refused(a))
        return;
    const uint64_t returned = r.head[0];
    // (n_hashes < 2^32 - 1: tile numbers fit 32 bits)
    const uint32_t ntiles = uint32_t((returned + kPartThreads - 1) / kPartThreads);   // with a returned hash
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (r.tile[uint64_t(kRhTileStride) * tile + kRhTileSeveral] == 0)   // (the same for every lane)
            continue;
        const uint64_t i = uint64_t(tile) * kPartThreads + threadIdx.x;
        if (i >= returned || uint32_t(r.rec[kRhRecWords * i + 1]) < 2)
            continue;
        uint64_t at = r.rec[kRhRecWords * i + 4];   // the gather's word: where the hash's parts begin
        if (at == ~0ull)
            continue;
        const uint64_t end = at + r.rec[kRhRecWords * i];
        const uint64_t h = r.hashes[i];
        uint64_t from = 0, order = 0, src = 0, version = 0;
        uint32_t len = 0;
        // (inside the hash's own range, whatever the walks find)
        while (rh_next(a, r.table_id, h, from, &order, &src, &version, &len) && at + rh::kPartHeader + len <= end) {
            const uint64_t d = r.reply + at + rh::kPartHeader;
            for (uint32_t b = 0; b < rh::kPartHeader; b++)
                *reinterpret_cast<gw8*>(d - rh::kPartHeader + b) = rh::header_byte(version, len, b);
            for (uint32_t b = 0; b < len; b++)   // (one lane, byte by byte: the path is rare and stays small)
                *reinterpret_cast<gw8*>(d + b) = *reinterpret_cast<gu8*>(src + b);
            at += rh::kPartHeader + len;
            from = order + 1;
        }
    }
}

}  // namespace
