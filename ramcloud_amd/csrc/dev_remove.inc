// A multi-remove against the replay table (ramcrc_replay_table_remove_device,
// DESIGN.md 5.16): k_rm_group, k_rm_size, k_rm_scan, k_rm_emit.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, after dev_write.inc; not a standalone header.
//
// The table is only read.  The write's four launches, none of which waits for
// another workgroup:
//   k_rm_group  one request per lane: the tests that read nothing
//               (remove_rules.h), the key's hash into a scratch word, and
//               k_res_insert's claim and key compare in a scratch table of
//               slots_for(n) one-word slots: a slot holds the complement of a
//               request index of its key -- any request of the key names the
//               key --, and an atomic maximum leaves the lowest one there;
//   k_rm_size   one request per lane in tiles of kPartThreads: rtab_probe over
//               the caller's own requests with the group pass's hash as the
//               given one (a key is hashed once a call), the first-of-its-key
//               test, the outcome, three scratch words per request; per tile
//               the sums the cut depends on, stored by the one workgroup that
//               has the tile; the counts the cut does not depend on by one
//               atomic per workgroup and count on the head line;
//   k_rm_scan   one workgroup: the tile sums become offsets and metadata
//               offsets; the tiles whose end lies within the capacity count
//               whole, the first one that does not is scanned request by
//               request; then the summary;
//   k_rm_emit   per tile the offsets again, the part, the reference; then the
//               tombstones.  Every output entry is a tombstone, so the class
//               that decides the time is the short key: up to kRmLaneKeyMax key
//               bytes a lane builds its whole entry in registers -- metadata,
//               the 28 header bytes, the checksum, the key -- and stores it as
//               aligned 32-bit words between at most three head and three tail
//               bytes.  Longer keys go to groups of 8 lanes (wr_tombstone).
//               The certificate is folded from the entries' metadata bytes as
//               k_wr_emit folds it and sealed by the last workgroup to finish.

namespace {

constexpr uint32_t kRmReqWords = 5;      // scratch per request: the hash, the group slot, the record (3)
constexpr uint32_t kRmTileWords = 5;     // scratch per tile: bytes (then the offset), counts, tombstone
                                         // bytes, highest version, metadata bytes before the tile
constexpr uint32_t kRmHeadWords = 16;    // the head line, 64-bit words
constexpr int kRmCountBits = 12;         // a tile's counts: requests, metadata bytes
constexpr uint32_t kRmLaneKeyMax = kSlOneLaneMax - ramcrc_remove::kTombHeader;   // 36: k_sl_stamp's class bound
constexpr int kRmMetaShift = 48;         // the emit's scan word: posted bytes | metadata bytes << 48
static_assert(4 * kPartThreads < (1 << kRmCountBits), "a tile's metadata bytes");
static_assert(sizeof(ramcrc_remove_summary) == 96 && ramcrc_remove::kPartBytes == 12, "remove ABI");
static_assert(ramcrc_remove::kTombHeader + kRmLaneKeyMax < 0x100, "a lane's entry has one length byte");

// The head line.
enum : uint32_t {
    kRmMeta = 0,      // metadata bytes of the written entries (scan)
    kRmBytes = 1,     // the output's head (scan)
    kRmCert = 2,      // the folded metadata checksums (emit)
    kRmTicket = 3,    // workgroups of the emit that have finished
    kRmCounts = 6,    // doesnt_exist, object_exists, wrong_version, bad, retry_duplicate, ok_absent (size)
};
constexpr uint32_t kRmKinds = 6;

// The record's flags word: the status in the low byte, the key length above.
constexpr uint64_t kRmReach = 1ull << 8;
constexpr int kRmKeyLenShift = 32;

struct RmDesc {
    uint64_t keys;                   // the caller's key buffer
    uint64_t keys_bytes;
    const uint64_t* reqs;            // three words each: table id, key_off, reserved << 32 | key_len
    uint64_t nq;
    const uint64_t* key_hash;        // nullable
    const uint64_t* rules;           // nullable: two words a request
    const uint64_t* batch_seg;       // nullable
    uint64_t next_version;
    uint32_t timestamp;
    uint32_t cap;
    uint64_t out;
    ramcrc_seg_cert* cert;
    uint32_t* parts;                 // three words each
    uint32_t* refs;                  // nullable
    ramcrc_remove_summary* summary;
    // scratch
    uint64_t* hash;                  // [nq] a usable request's key hash
    uint64_t* slot;                  // [nq] the request's slot of the grouping table; kResNone: not usable
    uint64_t* rec;                   // [3 nq] the part's version, segment id, flags
    unsigned long long* group;       // [gslots] 0: free; else ~(a request of the slot's key), at the end the lowest
    uint64_t gslots;
    uint64_t* tile;                  // [kRmTileWords * tiles]
    unsigned long long* head;        // [kRmHeadWords]
};

// Request i's key, or false: from the caller's arrays alone, so that a lane
// can read another request's key without waiting for its lane.
__device__ __forceinline__ bool rm_key_of(const RmDesc& w, uint64_t i, ResKey* k)
{
    const uint64_t off = w.reqs[3 * i + 1], lr = w.reqs[3 * i + 2];
    bool bad_rules = false;
    if (w.rules)
        bad_rules = ramcrc_read::bad_rules(ramcrc_read::Rules{0ull, w.rules[2 * i + 1]});
    if (ramcrc_remove::bad_request(off, uint32_t(lr), uint32_t(lr >> 32), bad_rules, w.keys_bytes))
        return false;
    *k = ResKey{w.reqs[3 * i], w.keys + off, uint32_t(lr)};
    return true;
}

// -------------------------------------------------------------- k_rm_group
#define RM_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_rm_group(RtabDesc a, RmDesc w)
{
    if (rtab_refused(a))
        return;
    const uint64_t mask = w.gslots - 1;
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < w.nq; i += nthr) {
        ResKey me;
        uint64_t slot = kResNone;
        if (rm_key_of(w, i, &me)) {
            uint64_t hash;
            if constexpr (kGiven)
                hash = w.key_hash[i];
            else
                hash = part_key_hash(me.table_id, me.addr, me.len);
            w.hash[i] = hash;   // the probe's
            // linear probing, bounded by the slot count (load <= 0.5: an
            // empty slot ends every chain)
            uint64_t s = hash & mask;
            for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                unsigned long long c = __hip_atomic_load(&w.group[s], RM_RLX);
                if (c == 0 && __hip_atomic_compare_exchange_strong(
                                  &w.group[s], &c, static_cast<unsigned long long>(~i),
                                  __ATOMIC_RELAXED, RM_RLX)) {
                    slot = s;
                    break;
                }
                // ~c: a usable request of the slot's key (the failed CAS stored
                // c); whichever request the word names later, its key is the same
                ResKey k;
                if (rm_key_of(w, ~c, &k) && k.table_id == me.table_id && k.len == me.len &&
                    res_bytes_equal(k.addr, me.addr, me.len)) {
                    slot = s;
                    if (~i > c)
                        __hip_atomic_fetch_max(&w.group[s], static_cast<unsigned long long>(~i), RM_RLX);
                    break;
                }
            }
        }
        w.slot[i] = slot;
    }
}

#undef RM_RLX

// The bytes of the tombstone a record's flags word stands for.  What a request
// posts to the scans is wr_posted of that: capacity + 1 for one that can never
// fit, so that the sums stay below 2^64.
__device__ __forceinline__ uint64_t rm_size_of(uint64_t flags)
{
    return ramcrc_remove::tomb_size(uint32_t(flags >> kRmKeyLenShift));
}

// --------------------------------------------------------------- k_rm_size
// q: the lookup over the caller's requests, its given hashes the group pass's.
__global__ __launch_bounds__(kPartThreads) void k_rm_size(RtabDesc a, LookDesc q, RmDesc w)
{
    namespace rr = ramcrc_read;
    namespace rm = ramcrc_remove;
    if (rtab_refused(a))
        return;
    __shared__ unsigned long long red[kPartThreads / kWaveSize][4];
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    const uint32_t lane = threadIdx.x & (kWaveSize - 1), wv = threadIdx.x / kWaveSize;
    uint32_t cnt[kRmKinds] = {};   // (a lane takes fewer than 2^32 requests)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        uint64_t sums[3] = {0, 0, 0};   // bytes, counts, tombstone bytes
        uint64_t top = 0;               // the highest version that reaches the tombstone
        uint32_t kind = kRmKinds;       // (counted by the scan, or no request)
        if (i < w.nq) {
            const uint64_t slot = w.slot[i];
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            uint64_t flags = rr::kStatusFormatError, pv = 0, seg = 0;
            kind = 3;
            if (slot != kResNone) {
                LookHit hit{0ull, 0u, ramcrc_look::Value{0u, 0u}};
                res = rtab_probe<true>(a, q, i, &hit);
                if (~w.group[slot] != i) {
                    flags = rm::kStatusRetry;
                    kind = 4;
                } else {
                    rr::Rules ru = rr::no_rules();
                    if (w.rules)
                        ru = rr::Rules{w.rules[2 * i], w.rules[2 * i + 1]};
                    const rm::Outcome o = rm::outcome(res.kind, res.version, ru);
                    flags = o.status;
                    pv = o.version;
                    kind = o.status == rr::kStatusDoesntExist ? 0u : o.status == rr::kStatusExists ? 1u
                           : o.status == rr::kStatusWrongVersion ? 2u : 5u;
                    if (o.reach) {
                        const uint32_t kl = uint32_t(w.reqs[3 * i + 2]);
                        flags |= kRmReach | (uint64_t(kl) << kRmKeyLenShift);
                        if (w.batch_seg)
                            seg = w.batch_seg[res.ref.batch] + res.segment;
                        sums[0] = wr_posted(rm::tomb_size(kl), w.cap);
                        sums[1] = 1ull | (uint64_t(rm::tomb_meta(kl)) << kRmCountBits);
                        sums[2] = rm::tomb_len(kl);
                        top = pv;
                        kind = kRmKinds;
                    }
                }
            }
            if (q.results)
                look_store(q, i, res);
            uint64_t* const rec = w.rec + 3 * i;
            rec[0] = pv;
            rec[1] = seg;
            rec[2] = flags;
        }
        // the tile's sums: this workgroup alone has the tile
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            unsigned long long v = k < 3 ? sums[k] : top;
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1) {
                const unsigned long long o = __shfl_xor(v, d);
                v = k < 3 ? v + o : (o > v ? o : v);
            }
            if (lane == 0)
                red[wv][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const uint32_t k = threadIdx.x;
            unsigned long long v = red[0][k];
#pragma unroll
            for (uint32_t x = 1; x < kPartThreads / kWaveSize; x++)
                v = k < 3 ? v + red[x][k] : (red[x][k] > v ? red[x][k] : v);
            w.tile[kRmTileWords * tile + k] = v;
        }
        __syncthreads();   // red is free again
        // the outcomes no cut changes
#pragma unroll
        for (uint32_t k = 0; k < kRmKinds; k++)
            cnt[k] += kind == k;
    }
#pragma unroll
    for (uint32_t k = 0; k < kRmKinds; k++) {
        const unsigned long long n = rtab_block_sum(cnt[k], reinterpret_cast<uint64_t*>(&red[0][0]));
        if (threadIdx.x == 0 && n)
            atomicAdd(&w.head[kRmCounts + k], n);
    }
}

// --------------------------------------------------------------- k_rm_scan
// One workgroup.  A tombstone takes at least 34 bytes, so the ends of the
// requests that reach it grow strictly and the written ones are a prefix of
// them: whole tiles, then a prefix of one tile.
__global__ __launch_bounds__(kPartThreads) void k_rm_scan(RtabDesc a, RmDesc w)
{
    namespace rm = ramcrc_remove;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s, top_s;
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_remove_summary sm{};
            sm.spoiled = 1;
            *w.summary = sm;
        }
        return;
    }
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    constexpr uint64_t kF = (1ull << kRmCountBits) - 1;
    if (t == 0) {
        cut_s = ntiles;
        top_s = 0;
    }
    __syncthreads();
    uint64_t carry = 0, carry2 = 0, cut = ntiles, top = 0;
    uint64_t acc[4] = {};   // written: requests, metadata, tombstone bytes; all that reached the tombstone
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPartThreads) {
        const uint64_t tl = t0 + t;
        uint64_t v = 0, c = 0;
        if (tl < ntiles) {
            v = w.tile[kRmTileWords * tl];
            c = w.tile[kRmTileWords * tl + 1];
        }
        uint64_t tot, tot2;
        const uint64_t base = carry + part_block_excl(v, wsum, &tot);
        const uint64_t base2 = carry2 + part_block_excl((c >> kRmCountBits) & kF, wsum, &tot2);
        if (tl < ntiles) {
            uint64_t* const ts = w.tile + kRmTileWords * tl;
            ts[0] = base;
            ts[4] = base2;
            acc[3] += c & kF;
            if (base + v <= w.cap) {
                acc[0] += c & kF;
                acc[1] += (c >> kRmCountBits) & kF;
                acc[2] += ts[2];
                top = ts[3] > top ? ts[3] : top;
            } else if (tl < cut) {
                cut = tl;
            }
        }
        carry += tot;
        carry2 += tot2;
    }
    if (cut < ntiles)
        atomicMin(&cut_s, static_cast<unsigned long long>(cut));
    __syncthreads();   // the cut, and every tile's offsets
    cut = cut_s;
    uint64_t bytes = carry;
    if (cut < ntiles) {
        // the tile the output ends in: its requests one by one
        const uint64_t i = cut * kPartThreads + t;
        uint64_t flags = 0, size = 0;
        if (i < w.nq) {
            flags = w.rec[3 * i + 2];
            if (flags & kRmReach)
                size = rm_size_of(flags);
        }
        uint64_t tot;
        const uint64_t base = w.tile[kRmTileWords * cut];
        const uint64_t off = base + part_block_excl(wr_posted(size, w.cap), wsum, &tot);
        const bool in = (flags & kRmReach) && off + size <= w.cap;
        if (in) {
            const uint32_t kl = uint32_t(flags >> kRmKeyLenShift);
            const uint64_t cur = w.rec[3 * i];
            acc[0]++;
            acc[1] += rm::tomb_meta(kl);
            acc[2] += rm::tomb_len(kl);
            top = cur > top ? cur : top;
        }
        bytes = base + rtab_block_sum(in ? size : 0ull, wsum);
    }
    if (top)
        atomicMax(&top_s, static_cast<unsigned long long>(top));
    uint64_t sums[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        sums[k] = rtab_block_sum(acc[k], wsum);
    __syncthreads();   // top_s
    if (t == 0) {
        ramcrc_remove_summary sm{};
        sm.removed = sums[0];
        sm.doesnt_exist = w.head[kRmCounts];
        sm.object_exists = w.head[kRmCounts + 1];
        sm.wrong_version = w.head[kRmCounts + 2];
        sm.bad = w.head[kRmCounts + 3];
        sm.retry_duplicate = w.head[kRmCounts + 4];
        sm.ok_absent = w.head[kRmCounts + 5];
        sm.retry_full = sums[3] - sums[0];
        sm.next_version = rm::next_version(w.next_version, top_s);
        sm.out_bytes = bytes;
        sm.tombstone_bytes = sums[2];
        *w.summary = sm;
        w.head[kRmMeta] = sums[1];
        w.head[kRmBytes] = bytes;
    }
}

// --------------------------------------------------------------- k_rm_emit
// One lane's entry from registers: the first `size` bytes (at least 4, at most
// 4 kWords - 3) of the little-endian words x[0 .. kWords / 2] to e (any
// residue), as aligned 32-bit words with byte stores only in front of the first
// and behind the last.  Every store lies inside [e, e + size).
template <uint32_t kWords>
__device__ __forceinline__ void lane_store_entry(uint64_t e, const uint64_t* x, uint32_t size)
{
    typedef __attribute__((address_space(1))) uint8_t gw8;
    typedef __attribute__((address_space(1))) uint32_t gw32;
    const uint32_t lead = (4u - uint32_t(e)) & 3u;
#pragma unroll
    for (uint32_t b = 0; b < 3; b++)
        if (b < lead)
            *reinterpret_cast<gw8*>(e + b) = uint8_t(x[0] >> (8 * b));
    const uint32_t nd = (size - lead) >> 2, rem = (size - lead) & 3u;
    const uint64_t at = e + lead;
#pragma unroll
    for (uint32_t k = 0; k < kWords; k++) {
        const uint32_t lo = uint32_t(x[k >> 1] >> (32 * (k & 1)));
        const uint32_t hi = uint32_t(x[(k + 1) >> 1] >> (32 * ((k + 1) & 1)));
        const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, lead);
        if (k < nd) {
            *reinterpret_cast<gw32*>(at + 4 * k) = v;
        } else if (k == nd) {
#pragma unroll
            for (uint32_t b = 0; b < 3; b++)
                if (b < rem)
                    *reinterpret_cast<gw8*>(at + 4 * k + b) = uint8_t(v >> (8 * b));
        }
    }
}

// One tombstone of a key of at most kRmLaneKeyMax bytes, by one lane: the
// whole entry at e (any residue) -- two metadata bytes, the header, the
// checksum, the key.  The key is read once, as aligned 16-byte words; the
// header bytes come from registers; the entry's 34 + klen bytes are stored as
// aligned 32-bit words with byte stores only in front of the first and behind
// the last.  Every store lies inside the entry.
__device__ __forceinline__ void rm_tombstone_lane(uint64_t e, uint64_t key, uint32_t klen, uint32_t meta,
                                                  uint64_t table_id, uint64_t segment_id, uint64_t version,
                                                  uint32_t ts, const uint32_t* t0)
{
    namespace rw = ramcrc_write;
    constexpr uint32_t kKw = (kRmLaneKeyMax + 7) / 8;
    constexpr uint32_t kWords = (2 + rw::kTombHeader + kRmLaneKeyMax + 3) / 4;   // 18
    static_assert(kRmLaneKeyMax % 8 != 0 && kRmLaneKeyMax % 8 <= 6, "the last key word's top two bytes are 0");
    uint64_t kw[kKw];
#pragma unroll
    for (uint32_t j = 0; j < kKw; j++) {
        kw[j] = 0;
        if (8 * j < klen)
            kw[j] = part_bytes(key + 8 * j, klen - 8 * j < 8 ? klen - 8 * j : 8u);
    }
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t b = 0; b < 28; b++)
        c = t0[(c ^ rw::tomb_header_byte(b, table_id, segment_id, version, ts)) & 0xFF] ^ (c >> 8);
#pragma unroll
    for (uint32_t j = 0; j < kRmLaneKeyMax; j++)
        if (j < klen)
            c = t0[(c ^ uint32_t(kw[j >> 3] >> (8 * (j & 7)))) & 0xFF] ^ (c >> 8);
    const uint64_t ck = ~c;
    // the entry as 64-bit words: everything lies two bytes past a word's start
    uint64_t x[kWords / 2 + 1];
    x[0] = meta | (table_id << 16);
    x[1] = (table_id >> 48) | (segment_id << 16);
    x[2] = (segment_id >> 48) | (version << 16);
    x[3] = (version >> 48) | (uint64_t(ts) << 16) | (ck << 48);
    x[4] = (ck >> 16) | (kw[0] << 16);
#pragma unroll
    for (uint32_t j = 1; j < kKw; j++)
        x[4 + j] = (kw[j - 1] >> 48) | (kw[j] << 16);
    x[4 + kKw] = 0;
    static_assert(4 + kKw == kWords / 2, "the words of the longest entry, and one of zeros");
    lane_store_entry<kWords>(e, x, 2 + rw::kTombHeader + klen);   // (34 bytes or more)
}

__global__ __launch_bounds__(kPartThreads) void k_rm_emit(RtabDesc a, RmDesc w)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    namespace rm = ramcrc_remove;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint32_t t0[256];
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t skey[kPartThreads], spay[kPartThreads];   // the long keys of a tile, as they come
    __shared__ uint64_t scur[kPartThreads], sseg[kPartThreads], stid[kPartThreads];
    __shared__ uint32_t slen[kPartThreads];
    __shared__ uint32_t nlong;
    __shared__ uint32_t red[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const uint32_t t = threadIdx.x;
    static_assert(kPartThreads == 256, "one byte-table entry per thread");
    t0[t] = g_tab.t0.t[t];
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    const uint64_t meta_all = w.head[kRmMeta];
    uint32_t cert = 0;   // thread 0: this workgroup's tiles, moved to the end of the metadata
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();   // the table is filled; the previous tile's groups have read their descriptors
        if (t == 0)
            nlong = 0;
        const uint64_t i = tile * kPartThreads + t;
        uint64_t flags = 0, pv = 0, seg = 0, size = 0;
        uint32_t klen = 0, meta = 0;
        if (i < w.nq) {
            const uint64_t* const rec = w.rec + 3 * i;
            pv = rec[0];
            seg = rec[1];
            flags = rec[2];
            if (flags & kRmReach) {
                klen = uint32_t(flags >> kRmKeyLenShift);
                size = rm::tomb_size(klen);
                meta = rm::tomb_meta(klen);
            }
        }
        const uint64_t* const ts = w.tile + kRmTileWords * tile;
        uint64_t tot;
        const uint64_t ex =
            part_block_excl(wr_posted(size, w.cap) | (uint64_t(meta) << kRmMetaShift), wsum, &tot);
        const uint64_t off = ts[0] + (ex & ((1ull << kRmMetaShift) - 1));
        // (the scan cut where the entries stop fitting; checked here from the
        // same sums, as the last thing between a stale word and a stray store)
        const bool reach = (flags & kRmReach) != 0, in = reach && off + size <= w.cap;
        // the written entries are a prefix of those that reach the tombstone,
        // so a written one's metadata lies behind that of all before it
        const uint64_t meta_at = ts[4] + (ex >> kRmMetaShift);
        const uint64_t tile_end = ts[4] + (tot >> kRmMetaShift);
        const uint64_t meta_end = tile_end < meta_all ? tile_end : meta_all;   // of the tile's written entries
        if (i < w.nq) {
            const uint32_t st = uint32_t(flags & 0xFF);
            const uint32_t status = !reach ? st : in ? rr::kStatusOk : rm::kStatusRetry;
            w.parts[3 * i] = status;
            w.parts[3 * i + 1] = uint32_t(pv);
            w.parts[3 * i + 2] = uint32_t(pv >> 32);
            if (w.refs)
                w.refs[i] = in ? uint32_t(off) : rm::kNone;
        }
        uint32_t piece = 0;
        if (in) {
            const uint64_t e = w.out + off;
            const uint64_t table_id = w.reqs[3 * i], key = w.keys + w.reqs[3 * i + 1];
            uint32_t nm;
            const uint64_t m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, rm::tomb_len(klen), &nm);
            uint32_t c = 0;
            for (uint32_t b = 0; b < nm; b++)
                c = t0[(c ^ uint32_t(m >> (8 * b))) & 0xFF] ^ (c >> 8);
            const uint32_t behind = uint32_t(meta_end - meta_at) - nm;
            piece = behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
            if (klen <= kRmLaneKeyMax) {
                rm_tombstone_lane(e, key, klen, uint32_t(m), table_id, seg, pv, w.timestamp, t0);
            } else {
                for (uint32_t b = 0; b < nm; b++)
                    *reinterpret_cast<gw8*>(e + b) = uint8_t(m >> (8 * b));
                const uint32_t k = atomicAdd(&nlong, 1u);
                skey[k] = key;
                spay[k] = e + nm;
                scur[k] = pv;
                sseg[k] = seg;
                stid[k] = table_id;
                slen[k] = klen;
            }
        }
        // the tile's metadata checksum, moved to the end of all metadata
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            piece ^= __shfl_xor(piece, d);
        if ((t & (kWaveSize - 1)) == 0)
            red[t / kWaveSize] = piece;
        __syncthreads();
        if (t == 0) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPartThreads / kWaveSize; k++)
                c ^= red[k];
            if (c) {
                const uint32_t behind = uint32_t(meta_all - meta_end);
                cert ^= behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
            }
        }
        const uint32_t nl = nlong, g = t / kSlLanes, sub = t % kSlLanes;
        for (uint32_t j = g; j < nl; j += kPartThreads / kSlLanes)
            wr_tombstone(skey[j], spay[j], slen[j], sub, stid[j], sseg[j], scur[j], w.timestamp, t0);
    }
    __syncthreads();   // the table is filled, for a workgroup without a tile too
    // the certificate: every workgroup folds its share, the last one seals it
    if (t == 0) {
        if (cert)
            atomicXor(reinterpret_cast<unsigned int*>(&w.head[kRmCert]), cert);
        __threadfence();
        if (atomicAdd(&w.head[kRmTicket], 1ull) + 1 == gridDim.x) {
            __threadfence();
            const uint32_t folded = atomicXor(reinterpret_cast<unsigned int*>(&w.head[kRmCert]), 0u);
            const uint32_t head = uint32_t(w.head[kRmBytes]);
            // Segment::getAppendedLength: a fresh Crc32C moved behind the
            // metadata, the entries' metadata, the 4 head bytes, finalized
            uint32_t c = folded ^ (meta_all ? mulmod_dev(0xFFFFFFFFu, sl_xpow8(uint32_t(meta_all))) : 0xFFFFFFFFu);
            for (int b = 0; b < 4; b++)
                c = t0[(c ^ (head >> (8 * b))) & 0xFF] ^ (c >> 8);
            *w.cert = ramcrc_seg_cert{head, ~c};
        }
    }
}

}  // namespace
