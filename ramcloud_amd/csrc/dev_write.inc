// A multi-write against the replay table (ramcrc_replay_table_write_device,
// DESIGN.md 5.15): k_wr_group, k_wr_size, k_wr_scan, k_wr_emit.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, after dev_replay_table.inc; not a standalone
// header.
//
// The table is only read.  Four launches, none of which waits for another
// workgroup:
//   k_wr_group  one request per lane: the tests that read nothing, the first
//               key (write_rules.h), the lookup's query for it (three scratch
//               words, so that the size pass runs rtab_probe unchanged), and
//               k_res_insert's claim and key compare in a scratch table of
//               slots_for(n) slots, where the lowest request index of a key is
//               kept by an atomic maximum of its complement;
//   k_wr_size   one request per lane in tiles of kPartThreads: the probe, the
//               first-of-its-key test, rejectOperation, the byte size and the
//               "allocates" flag into four scratch words per request; per tile
//               the sums the cut depends on by one atomic per wave and sum, the
//               counts it does not depend on by one atomic per wave on the head
//               line;
//   k_wr_scan   one workgroup: the tile sums become offsets, allocation ranks
//               and metadata offsets; the tiles whose end lies within the
//               capacity count whole, the first one that does not is scanned
//               request by request; then the summary;
//   k_wr_emit   per tile the offsets again, the version, the part, the
//               reference, the entry headers; then every written object by a
//               group of 8 lanes (a wave from kAppBigMin data bytes on): the
//               data is read once and written once, k_app_copy's way, and the
//               checksum of [4, end) comes from the words that are stored;
//               the tombstone by the same 8 lanes.  The certificate is folded
//               from the entries' metadata bytes with the X^n algebra of gf2.h
//               (k_app_scan's, per tile instead of per step) and sealed by the
//               last workgroup to finish.
//
// The object checksum.  The message is 20 header bytes, the data bytes before
// the destination's first full granule, the full granules, and the bytes
// behind the last one.  Lane 0 takes the first two through the byte table; its
// state enters the first granule's first word.  Lane `sub` takes the granules
// sub, sub + K, ...: with acc at the end of granule q,
//     acc' = X^(16 K)(acc) ^ X^16(w0) ^ X^12(w1) ^ X^8(w2) ^ X^4(w3)
// is the state at the end of granule q + K: twenty independent LDS lookups a
// granule.  Each lane then moves its state to the end of the last granule (one
// GF(2) multiply), the group XORs, and lane 0 takes the tail bytes.

namespace {

constexpr uint32_t kWrReqWords = 8;      // scratch per request: the query (3), the group slot, the record (4)
constexpr uint32_t kWrTileWords = 6;     // scratch per tile: bytes (then the offset), counts, value, key,
                                         // tombstone bytes, allocations | metadata bytes << 32 before the tile
constexpr uint32_t kWrHeadWords = 16;    // the head line, 64-bit words
constexpr int kWrCountBits = 12;         // a tile's counts: requests, tombstones, allocations, metadata bytes
static_assert(10 * kPartThreads < (1 << kWrCountBits), "a tile's metadata bytes");
static_assert(sizeof(ramcrc_write_req) == 24 && sizeof(ramcrc_write_ref) == 8 &&
                  sizeof(ramcrc_write_summary) == 128, "write ABI");

// The head line.
enum : uint32_t {
    kWrMeta = 0,      // metadata bytes of the written entries (scan)
    kWrBytes = 1,     // the output's head (scan)
    kWrCert = 2,      // the folded metadata checksums (emit)
    kWrTicket = 3,    // workgroups of the emit that have finished
    kWrTop = 4,       // one past the highest version the tombstone rule gave
    kWrCounts = 6,    // doesnt_exist, object_exists, wrong_version, bad, retry_duplicate (size)
};

// The record's flags word.
constexpr uint64_t kWrReach = 1ull << 8, kWrAlloc = 1ull << 9, kWrTomb = 1ull << 10, kWrOverTomb = 1ull << 11;
constexpr int kWrKeyOffShift = 12, kWrKeyLenShift = 32;

__device__ const ramcrc::OpTable g_wr_x12 = ramcrc::make_op(12);

struct WrDesc {
    uint64_t data;                   // the caller's data buffer
    uint64_t data_bytes;
    const uint64_t* reqs;            // three words each: table id, data_off, reserved << 32 | data_len
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
    uint2* refs;                     // nullable
    ramcrc_write_summary* summary;
    // scratch
    uint64_t* query;                 // [3 nq] the lookup's queries
    uint64_t* slot;                  // [nq] the request's slot of the grouping table; kResNone: not usable
    uint64_t* rec;                   // [4 nq] winner's version, value | data bytes << 32, segment id, flags
    unsigned long long* group;       // [2 gslots] claim, ~(lowest request)
    uint64_t gslots;
    uint64_t* tile;                  // [kWrTileWords * tiles]
    unsigned long long* head;        // [kWrHeadWords]
};

struct WrRd {
    uint64_t at;   // address of data byte 0
    __device__ __forceinline__ uint32_t u8(uint32_t o) const { return uint32_t(part_bytes(at + o, 1)); }
    __device__ __forceinline__ uint32_t u16(uint32_t o) const { return uint32_t(part_bytes(at + o, 2)); }
};

// Request i's key, or ok = false: from the caller's arrays alone, so that a
// lane can read another request's key without waiting for its lane.
__device__ __forceinline__ bool wr_key_of(const WrDesc& w, uint64_t i, ResKey* k)
{
    const uint64_t off = w.reqs[3 * i + 1], lr = w.reqs[3 * i + 2];
    const uint32_t len = uint32_t(lr);
    bool bad_rules = false;
    if (w.rules)
        bad_rules = ramcrc_read::bad_rules(ramcrc_read::Rules{0ull, w.rules[2 * i + 1]});
    if (ramcrc_write::bad_request(off, len, uint32_t(lr >> 32), bad_rules, w.data_bytes))
        return false;
    const ramcrc_write::Key key = ramcrc_write::first_key(len, WrRd{w.data + off});
    if (!key.ok)
        return false;
    *k = ResKey{w.reqs[3 * i], w.data + off + key.off, key.len};
    return true;
}

// -------------------------------------------------------------- k_wr_group
#define WR_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_wr_group(RtabDesc a, WrDesc w)
{
    if (rtab_refused(a))
        return;
    const uint64_t mask = w.gslots - 1;
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < w.nq; i += nthr) {
        ResKey me;
        uint64_t slot = kResNone;
        if (wr_key_of(w, i, &me)) {
            w.query[3 * i] = me.table_id;
            w.query[3 * i + 1] = me.addr - w.data;
            w.query[3 * i + 2] = me.len;
            uint64_t hash;
            if constexpr (kGiven)
                hash = w.key_hash[i];
            else
                hash = part_key_hash(me.table_id, me.addr, me.len);
            // linear probing, bounded by the slot count (load <= 0.5: an
            // empty slot ends every chain)
            uint64_t s = hash & mask;
            for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                unsigned long long c = __hip_atomic_load(&w.group[2 * s], WR_RLX);
                if (c == 0 && __hip_atomic_compare_exchange_strong(
                                  &w.group[2 * s], &c, static_cast<unsigned long long>(i + 1),
                                  __ATOMIC_RELAXED, WR_RLX)) {
                    slot = s;
                    break;
                }
                // c: the claimant (the failed CAS stored it), a usable request
                ResKey k;
                if (wr_key_of(w, c - 1, &k) && k.table_id == me.table_id && k.len == me.len &&
                    res_bytes_equal(k.addr, me.addr, me.len)) {
                    slot = s;
                    break;
                }
            }
            if (slot != kResNone)
                __hip_atomic_fetch_max(&w.group[2 * slot + 1], static_cast<unsigned long long>(~i), WR_RLX);
        }
        w.slot[i] = slot;
    }
}

#undef WR_RLX

// The bytes request i posts to the scan: its true size, or capacity + 1 for a
// request that can never fit, so that the sums of 2^32 requests stay below 2^64.
__device__ __forceinline__ uint64_t wr_posted(uint64_t size, uint32_t cap)
{
    return size > cap ? uint64_t(cap) + 1 : size;
}

__device__ __forceinline__ uint64_t wr_size_of(uint64_t flags, uint32_t data_len)
{
    return ramcrc_write::request_size(data_len, (flags & kWrTomb) != 0, uint32_t(flags >> kWrKeyLenShift) & 0xFFFFu);
}

__device__ __forceinline__ uint32_t wr_meta_of(uint64_t flags, uint32_t data_len)
{
    uint32_t m = 1 + ramcrc_write::len_bytes(ramcrc_write::kObjHeader + data_len);
    if (flags & kWrTomb)
        m += 1 + ramcrc_write::len_bytes(ramcrc_write::kTombHeader + (uint32_t(flags >> kWrKeyLenShift) & 0xFFFFu));
    return m;
}

// --------------------------------------------------------------- k_wr_size
template <bool kGiven>
__global__ __launch_bounds__(kPartThreads) void k_wr_size(RtabDesc a, LookDesc q, WrDesc w)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    if (rtab_refused(a))
        return;
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        uint64_t sums[5] = {0, 0, 0, 0, 0};   // bytes, counts, value, key, tombstone bytes
        uint32_t st = 0xFFFFFFFFu;            // (no request)
        bool dup = false;
        if (i < w.nq) {
            const uint64_t slot = w.slot[i];
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            uint64_t flags = 0, vd = 0, seg = 0;
            st = rr::kStatusFormatError;
            if (slot != kResNone) {
                LookHit hit{0ull, 0u, ramcrc_look::Value{0u, 0u}};
                res = rtab_probe<kGiven>(a, q, i, &hit);
                if (~w.group[2 * slot + 1] != i) {
                    st = rw::kStatusRetry;
                    dup = true;
                } else {
                    // (an object of version 0 is VERSION_NONEXISTENT: no tombstone)
                    const uint64_t cur = res.kind == RAMCRC_LOOKUP_OBJECT ? res.version : 0ull;
                    const bool obj = cur != 0;
                    rr::Rules ru = rr::no_rules();
                    if (w.rules)
                        ru = rr::Rules{w.rules[2 * i], w.rules[2 * i + 1]};
                    st = rr::reject(ru, cur);
                    if (obj)
                        flags |= kWrTomb;   // (the replaced object's version: the tombstone's, and a rejected part's)
                    if (st == rr::kStatusOk) {
                        const uint32_t dl = uint32_t(w.reqs[3 * i + 2]);
                        const uint32_t kl = uint32_t(w.query[3 * i + 2]);
                        const uint32_t ko = uint32_t(w.query[3 * i + 1] - w.reqs[3 * i + 1]);
                        flags |= kWrReach | (cur == 0 ? kWrAlloc : 0ull) |
                                 (res.kind == RAMCRC_LOOKUP_TOMBSTONE ? kWrOverTomb : 0ull) |
                                 (uint64_t(ko) << kWrKeyOffShift) | (uint64_t(kl) << kWrKeyLenShift);
                        const uint32_t vl = rw::value_len(dl, WrRd{w.data + w.reqs[3 * i + 1]});
                        vd = vl | (uint64_t(dl) << 32);
                        if (obj && w.batch_seg)
                            seg = w.batch_seg[res.ref.batch] + res.segment;
                        sums[0] = wr_posted(wr_size_of(flags, dl), w.cap);
                        sums[1] = 1ull | (obj ? 1ull << kWrCountBits : 0ull) |
                                  (cur == 0 ? 1ull << (2 * kWrCountBits) : 0ull) |
                                  (uint64_t(wr_meta_of(flags, dl)) << (3 * kWrCountBits));
                        sums[2] = vl;
                        sums[3] = dl - vl;
                        sums[4] = obj ? rw::kTombHeader + kl : 0u;
                    }
                }
            }
            if (q.results)
                look_store(q, i, res);
            uint64_t* const rec = w.rec + 4 * i;
            rec[0] = res.version;
            rec[1] = vd;
            rec[2] = seg;
            rec[3] = flags | st;
        }
        // the tile's sums, which the call zeroed: one atomic per wave and sum
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(w.tile + kWrTileWords * tile + k), v);
        }
        // the outcomes no cut changes
        const uint32_t kinds[5] = {rr::kStatusDoesntExist, rr::kStatusExists, rr::kStatusWrongVersion,
                                   rr::kStatusFormatError, rw::kStatusRetry};
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) {
            const unsigned long long n = __builtin_popcountll(__ballot(st == kinds[k] && (k < 4 || dup)));
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && n)
                atomicAdd(&w.head[kWrCounts + k], n);
        }
    }
}

// --------------------------------------------------------------- k_wr_scan
// One workgroup.  A served request takes at least 27 bytes, so the ends of the
// served requests grow strictly and the written ones are a prefix of them:
// whole tiles, then a prefix of one tile.
__global__ __launch_bounds__(kPartThreads) void k_wr_scan(RtabDesc a, WrDesc w)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s;
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_write_summary sm{};
            sm.spoiled = 1;
            *w.summary = sm;
        }
        return;
    }
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    constexpr uint64_t kF = (1ull << kWrCountBits) - 1;
    if (t == 0)
        cut_s = ntiles;
    __syncthreads();
    uint64_t carry = 0, carry2 = 0, cut = ntiles;
    // written: requests, tombstones, metadata, value, key, tombstone bytes; all: served
    uint64_t acc[7] = {};
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPartThreads) {
        const uint64_t tl = t0 + t;
        uint64_t v = 0, c = 0;
        if (tl < ntiles) {
            v = w.tile[kWrTileWords * tl];
            c = w.tile[kWrTileWords * tl + 1];
        }
        const uint64_t v2 = ((c >> (2 * kWrCountBits)) & kF) | (((c >> (3 * kWrCountBits)) & kF) << 32);
        uint64_t tot, tot2;
        const uint64_t base = carry + part_block_excl(v, wsum, &tot);
        const uint64_t base2 = carry2 + part_block_excl(v2, wsum, &tot2);
        if (tl < ntiles) {
            uint64_t* const ts = w.tile + kWrTileWords * tl;
            ts[0] = base;
            ts[5] = base2;
            acc[6] += c & kF;
            if (base + v <= w.cap) {
                acc[0] += c & kF;
                acc[1] += (c >> kWrCountBits) & kF;
                acc[2] += (c >> (3 * kWrCountBits)) & kF;
                acc[3] += ts[2];
                acc[4] += ts[3];
                acc[5] += ts[4];
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
        uint64_t flags = 0, vd = 0, size = 0;
        if (i < w.nq) {
            flags = w.rec[4 * i + 3];
            vd = w.rec[4 * i + 1];
            if (flags & kWrReach)
                size = wr_size_of(flags, uint32_t(vd >> 32));
        }
        uint64_t tot;
        const uint64_t base = w.tile[kWrTileWords * cut];
        const uint64_t off = base + part_block_excl(wr_posted(size, w.cap), wsum, &tot);
        const bool in = (flags & kWrReach) && off + size <= w.cap;
        if (in) {
            const uint32_t dl = uint32_t(vd >> 32), vl = uint32_t(vd);
            acc[0]++;
            acc[1] += (flags & kWrTomb) ? 1 : 0;
            acc[2] += wr_meta_of(flags, dl);
            acc[3] += vl;
            acc[4] += dl - vl;
            acc[5] += (flags & kWrTomb)
                          ? ramcrc_write::kTombHeader + (uint32_t(flags >> kWrKeyLenShift) & 0xFFFFu) : 0u;
        }
        bytes = base + rtab_block_sum(in ? size : 0ull, wsum);
    }
    uint64_t sums[7];
#pragma unroll
    for (int k = 0; k < 7; k++)
        sums[k] = rtab_block_sum(acc[k], wsum);
    if (t == 0) {
        const uint64_t allocated = carry2 & 0xFFFFFFFFull;
        ramcrc_write_summary sm{};
        sm.ok = sums[0];
        sm.doesnt_exist = w.head[kWrCounts];
        sm.object_exists = w.head[kWrCounts + 1];
        sm.wrong_version = w.head[kWrCounts + 2];
        sm.bad = w.head[kWrCounts + 3];
        sm.retry_duplicate = w.head[kWrCounts + 4];
        sm.retry_full = sums[6] - sums[0];
        sm.tombstones = sums[1];
        sm.allocated = allocated;
        sm.next_version = w.next_version + allocated;   // (k_wr_emit raises it for the tombstone rule)
        sm.out_bytes = bytes;
        sm.value_bytes = sums[3];
        sm.key_bytes = sums[4];
        sm.tombstone_bytes = sums[5];
        sm.object_bytes = bytes - sums[2] - sums[5];
        *w.summary = sm;
        w.head[kWrMeta] = sums[2];
        w.head[kWrBytes] = bytes;
    }
}

// --------------------------------------------------------------- k_wr_emit
constexpr uint32_t kWrTabWords = 1024;   // one X^d operator in LDS
enum : uint32_t { kWrX4 = 0, kWrX8, kWrX12, kWrX16, kWrX128, kWrX1024, kWrTabs };

__device__ __forceinline__ uint32_t wr_apply(const uint32_t* tabs, uint32_t which, uint32_t v)
{
    const uint32_t* const t = tabs + which * kWrTabWords;
    return t[v & 0xFF] ^ t[256 + ((v >> 8) & 0xFF)] ^ t[512 + ((v >> 16) & 0xFF)] ^ t[768 + (v >> 24)];
}

// One object by kLanes lanes (this one is `sub`): the data bytes from src (any
// residue) to pay + 24 (any residue), the header bytes [4, 24), and the
// checksum of [4, end) into [0, 4).  Every store lies inside the payload.
template <int kLanes, int kU>
__device__ __forceinline__ void wr_object(uint64_t src, uint64_t pay, uint32_t len, uint32_t sub,
                                          uint32_t ts, uint64_t version, uint64_t table_id,
                                          const uint32_t* tabs, const uint32_t* t0)
{
    namespace rw = ramcrc_write;
    typedef __attribute__((address_space(1))) u32x4 gw32x4;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    constexpr uint32_t kStep = kLanes == 8 ? kWrX128 : kWrX1024;
    static_assert(kLanes == 8 || kLanes == 64, "X^(16 kLanes) is X^128 or X^1024");
    const uint64_t dst = pay + rw::kObjHeader;
    const uint64_t end = dst + len;
    const uint64_t a0 = (dst + 15) & ~15ull, a1 = end & ~15ull;
    const uint64_t hend = a0 < end ? a0 : end;        // head bytes [dst, hend)
    const uint64_t tbeg = a1 > hend ? a1 : hend;      // tail bytes [tbeg, end)
    for (uint32_t b = 4 + sub; b < rw::kObjHeader; b += kLanes)
        *reinterpret_cast<gw8*>(pay + b) = uint8_t(rw::obj_header_byte(b, ts, version, table_id));
    // lane 0: the state behind the header and the head bytes
    uint32_t c = 0;
    if (sub == 0) {
        c = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t b = 4; b < rw::kObjHeader; b++)
            c = t0[(c ^ rw::obj_header_byte(b, ts, version, table_id)) & 0xFF] ^ (c >> 8);
        for (uint64_t p = dst; p < hend; p++) {
            const uint32_t v = *reinterpret_cast<const gu8*>(src + (p - dst));
            *reinterpret_cast<gw8*>(p) = uint8_t(v);
            c = t0[(c ^ v) & 0xFF] ^ (c >> 8);
        }
    }
    uint32_t acc = c;   // without granules: the state itself
    if (a1 > a0) {
        const uint32_t ng = uint32_t((a1 - a0) >> 4);
        const uint64_t s0 = src + (a0 - dst);
        const uint32_t sh = uint32_t(s0) & 15u, dw = sh >> 2, by = sh & 3u;
        const uint64_t sa = s0 & ~15ull;
        acc = 0;
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
                    uint32_t x[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
                    if (dw & 2u) {
#pragma unroll
                        for (int j = 0; j < 6; j++)
                            x[j] = x[j + 2];
                    }
                    if (dw & 1u) {
#pragma unroll
                        for (int j = 0; j < 5; j++)
                            x[j] = x[j + 1];
                    }
                    u32x4 o;
                    o.x = __builtin_amdgcn_alignbyte(x[1], x[0], by);
                    o.y = __builtin_amdgcn_alignbyte(x[2], x[1], by);
                    o.z = __builtin_amdgcn_alignbyte(x[3], x[2], by);
                    o.w = __builtin_amdgcn_alignbyte(x[4], x[3], by);
                    *reinterpret_cast<gw32x4*>(a0 + 16ull * q) = o;
                    // (granule 0 is lane 0's first: c is its state, 0 elsewhere)
                    const uint32_t w0 = o.x ^ (q == 0 ? c : 0u);
                    acc = wr_apply(tabs, kStep, acc) ^ wr_apply(tabs, kWrX16, w0) ^
                          wr_apply(tabs, kWrX12, o.y) ^ wr_apply(tabs, kWrX8, o.z) ^
                          wr_apply(tabs, kWrX4, o.w);
                }
            }
        }
        // to the end of the last granule: this lane's last one is d granules before it
        if (sub < ng) {
            const uint32_t d = (ng - 1 - sub) % kLanes;
            if (d)
                acc = mulmod_dev(acc, sl_xpow8(16 * d));
        }
    }
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1)
        acc ^= __shfl_xor(acc, d);
    if (sub == 0) {
        for (uint64_t p = tbeg; p < end; p++) {
            const uint32_t v = *reinterpret_cast<const gu8*>(src + (p - dst));
            *reinterpret_cast<gw8*>(p) = uint8_t(v);
            acc = t0[(acc ^ v) & 0xFF] ^ (acc >> 8);
        }
        const uint32_t ck = ~acc;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            *reinterpret_cast<gw8*>(pay + b) = uint8_t(ck >> (8 * b));
    }
}

// One tombstone by 8 lanes (this one is `sub`), k_sl_stamp's way: the message
// is the 28 header bytes and the key; lane `sub` takes the sub-th eighth of it
// through the byte table, stores what it takes, moves its part to the end of
// the message and the group XORs the parts.
__device__ __forceinline__ void wr_tombstone(uint64_t key, uint64_t pay, uint32_t klen, uint32_t sub,
                                             uint64_t table_id, uint64_t segment_id, uint64_t version,
                                             uint32_t ts, const uint32_t* t0)
{
    namespace rw = ramcrc_write;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    const uint32_t M = 28 + klen;
    const uint32_t C = (M + kSlLanes - 1) / kSlLanes;
    const uint32_t lo = sub * C < M ? sub * C : M;
    const uint32_t hi = lo + C < M ? lo + C : M;
    uint32_t c = sub == 0 ? 0xFFFFFFFFu : 0u;   // a fresh Crc32C in front of the first part
    for (uint32_t m = lo; m < hi; m++) {
        uint32_t v;
        if (m < 28) {
            v = rw::tomb_header_byte(m, table_id, segment_id, version, ts);
            *reinterpret_cast<gw8*>(pay + m) = uint8_t(v);
        } else {
            v = *reinterpret_cast<const gu8*>(key + (m - 28));
            *reinterpret_cast<gw8*>(pay + m + 4) = uint8_t(v);
        }
        c = t0[(c ^ v) & 0xFF] ^ (c >> 8);
    }
    if (hi < M)
        c = mulmod_dev(c, sl_xpow8(M - hi));
    c ^= __shfl_xor(c, 1);
    c ^= __shfl_xor(c, 2);
    c ^= __shfl_xor(c, 4);
    const uint32_t ck = ~c;
    if (sub < 4)
        *reinterpret_cast<gw8*>(pay + 28 + sub) = uint8_t(ck >> (8 * sub));
}

__global__ __launch_bounds__(kPartThreads) void k_wr_emit(RtabDesc a, WrDesc w)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint32_t tabs[kWrTabs * kWrTabWords];
    __shared__ uint32_t t0[256];
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sobj[kPartThreads], stomb[kPartThreads];   // sobj, stomb: payloads; 0: none
    __shared__ uint64_t sver[kPartThreads], scur[kPartThreads], sseg[kPartThreads], stid[kPartThreads];
    __shared__ uint32_t slen[kPartThreads], skey[kPartThreads], sbig[kPartThreads];
    __shared__ uint32_t nbig[2];   // by tile parity, as in k_app_copy
    __shared__ uint32_t red[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const uint32_t t = threadIdx.x;
    static_assert(kPartThreads == 256, "one byte-table entry per thread");
    t0[t] = g_tab.t0.t[t];
    {
        const ramcrc::OpTable* const ops[kWrTabs] = {&g_tab.comb[0], &g_tab.lt.x8, &g_wr_x12, &g_tab.comb[1],
                                                     &g_tab.stride_small, &g_tab.stride_large};
#pragma unroll
        for (uint32_t k = 0; k < kWrTabs; k++)
#pragma unroll
            for (uint32_t j = 0; j < kWrTabWords / kPartThreads; j++)
                tabs[k * kWrTabWords + j * kPartThreads + t] = ops[k]->t[j][t];
    }
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    const uint64_t meta_all = w.head[kWrMeta];
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    __syncthreads();   // the tables are filled, for a workgroup without a tile too
    uint32_t cert = 0;   // thread 0: this workgroup's tiles, moved to the end of the metadata
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
        __syncthreads();   // the tables are filled; the previous tile's copies have read their descriptors
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        const uint64_t i = tile * kPartThreads + t;
        uint64_t flags = 0, wver = 0, vd = 0, seg = 0, size = 0, table_id = 0, data_off = 0;
        uint32_t dl = 0;
        if (i < w.nq) {
            const uint64_t* const rec = w.rec + 4 * i;
            wver = rec[0];
            vd = rec[1];
            seg = rec[2];
            flags = rec[3];
            dl = uint32_t(vd >> 32);
            if (flags & kWrReach) {
                size = wr_size_of(flags, dl);
                table_id = w.reqs[3 * i];
                data_off = w.reqs[3 * i + 1];
            }
        }
        const uint64_t* const ts = w.tile + kWrTileWords * tile;
        uint64_t tot;
        const uint64_t off = ts[0] + part_block_excl(wr_posted(size, w.cap), wsum, &tot);
        // (the scan cut where the entries stop fitting; checked here from the
        // same sums, as the last thing between a stale word and a stray store)
        const bool reach = (flags & kWrReach) != 0, in = reach && off + size <= w.cap;
        const uint32_t meta = in ? wr_meta_of(flags, dl) : 0u;
        const uint64_t ex2 =
            ts[5] + part_block_excl(((flags & kWrAlloc) ? 1ull : 0ull) | (uint64_t(meta) << 32), wsum, &tot);
        const uint32_t tile_meta = uint32_t(tot >> 32);
        const bool tomb = (flags & kWrTomb) != 0;
        const uint64_t cur = tomb ? wver : 0ull;
        const uint32_t klen = uint32_t(flags >> kWrKeyLenShift) & 0xFFFFu;
        uint64_t version = 0, src = 0, obj = 0, tmb = 0;
        uint32_t piece = 0;
        if (reach) {
            const uint64_t an = w.next_version + (ex2 & 0xFFFFFFFFull);
            version = rw::new_version(cur, (flags & kWrOverTomb) != 0, wver, an);
            if (cur == 0 && version != an)
                atomicMax(&w.head[kWrTop], static_cast<unsigned long long>(version + 1));
        }
        if (i < w.nq) {
            const uint32_t st = uint32_t(flags & 0xFF);
            const uint32_t status = !reach ? st : in ? rr::kStatusOk : rw::kStatusRetry;
            const uint64_t pv = in ? version : (st == rr::kStatusFormatError || st == rw::kStatusRetry) ? 0ull : cur;
            w.parts[3 * i] = status;
            w.parts[3 * i + 1] = uint32_t(pv);
            w.parts[3 * i + 2] = uint32_t(pv >> 32);
        }
        uint2 ref = make_uint2(rw::kNone, rw::kNone);
        if (in) {
            // the entry headers, and their checksum moved to the end of the tile's metadata
            const uint32_t olen = rw::kObjHeader + dl;
            uint32_t nm;
            uint64_t m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJ, olen, &nm);
            uint64_t e = w.out + off;
            uint32_t c = 0;
            ref.x = uint32_t(off);
            for (uint32_t b = 0; b < nm; b++) {
                *reinterpret_cast<gw8*>(e + b) = uint8_t(m >> (8 * b));
                c = t0[(c ^ uint32_t(m >> (8 * b))) & 0xFF] ^ (c >> 8);
            }
            obj = e + nm;
            src = w.data + data_off;
            if (tomb) {
                e = obj + olen;
                m = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, rw::kTombHeader + klen, &nm);
                ref.y = uint32_t(e - w.out);
                for (uint32_t b = 0; b < nm; b++) {
                    *reinterpret_cast<gw8*>(e + b) = uint8_t(m >> (8 * b));
                    c = t0[(c ^ uint32_t(m >> (8 * b))) & 0xFF] ^ (c >> 8);
                }
                tmb = e + nm;
            }
            const uint32_t behind = tile_meta - uint32_t(ex2 >> 32) + uint32_t(ts[5] >> 32) - meta;
            piece = behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
        }
        if (w.refs && i < w.nq)
            w.refs[i] = ref;
        // the tile's metadata checksum, moved to the end of all metadata
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            piece ^= __shfl_xor(piece, d);
        if ((t & (kWaveSize - 1)) == 0)
            red[t / kWaveSize] = piece;
        ssrc[t] = src;
        sobj[t] = obj;
        stomb[t] = tmb;
        sver[t] = version;
        scur[t] = cur;
        sseg[t] = seg;
        stid[t] = table_id;
        slen[t] = dl;
        skey[t] = (uint32_t(flags >> kWrKeyOffShift) & 0x3FFu) | (klen << 16);
        if (obj && dl >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        __syncthreads();
        if (t == 0) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPartThreads / kWaveSize; k++)
                c ^= red[k];
            if (c) {
                const uint32_t behind = uint32_t(meta_all) - uint32_t(ts[5] >> 32) - tile_meta;
                cert ^= behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
            }
        }
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t j = g; j < kPartThreads; j += kPartThreads / 8) {
            const uint64_t p = sobj[j];
            if (!p)
                continue;
            if (slen[j] < kAppBigMin)
                wr_object<8, 2>(ssrc[j], p, slen[j], sub, w.timestamp, sver[j], stid[j], tabs, t0);
            if (stomb[j])
                wr_tombstone(ssrc[j] + (skey[j] & 0xFFFFu), stomb[j], skey[j] >> 16, sub, stid[j], sseg[j],
                             scur[j], w.timestamp, t0);
        }
        const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
        for (uint32_t b = wv; b < nb; b += kPartThreads / kWaveSize) {
            const uint32_t j = sbig[b];
            wr_object<kWaveSize, 2>(ssrc[j], sobj[j], slen[j], ln, w.timestamp, sver[j], stid[j], tabs, t0);
        }
    }
    // the certificate: every workgroup folds its share, the last one seals it
    if (t == 0) {
        if (cert)
            atomicXor(reinterpret_cast<unsigned int*>(&w.head[kWrCert]), cert);
        __threadfence();
        if (atomicAdd(&w.head[kWrTicket], 1ull) + 1 == gridDim.x) {
            __threadfence();
            const uint32_t folded = atomicXor(reinterpret_cast<unsigned int*>(&w.head[kWrCert]), 0u);
            const uint32_t head = uint32_t(w.head[kWrBytes]);
            // Segment::getAppendedLength: a fresh Crc32C moved behind the
            // metadata, the entries' metadata, the 4 head bytes, finalized
            uint32_t c = folded ^ (meta_all ? mulmod_dev(0xFFFFFFFFu, sl_xpow8(uint32_t(meta_all))) : 0xFFFFFFFFu);
            for (int b = 0; b < 4; b++)
                c = t0[(c ^ (head >> (8 * b))) & 0xFF] ^ (c >> 8);
            *w.cert = ramcrc_seg_cert{head, ~c};
            const unsigned long long top = atomicMax(&w.head[kWrTop], 0ull);
            if (top > w.summary->next_version)
                w.summary->next_version = top;
        }
    }
}

}  // namespace
