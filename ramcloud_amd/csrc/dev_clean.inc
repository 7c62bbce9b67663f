// Cleaning batches out of the replay table (ramcrc_replay_table_clean_device
// and ramcrc_replay_table_clean_size_device, DESIGN.md 5.17): k_clean_open,
// k_clean_mark, k_clean_scan, k_clean_move, k_clean_claims.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, after dev_remove.inc; not a standalone header.
//
// Every record of an added batch knows its slot (the batch's work array), so
// cleaning hashes nothing, probes nothing and compares no key.  The victims'
// records are laid out as tiles of kPartThreads records, victim after victim
// in the order given, a victim's tiles in record order; a tile never spans two
// victims, and the survivors' order is the tiles' order.  The launches, none
// of which waits for another workgroup:
//   k_clean_open    the victim list (batch << 48 | first tile, from the
//                   kernel's arguments, kClOpenMax victims a launch) into
//                   scratch; then k_rtab_open for the survivor batch;
//   k_clean_mark    one record per lane: work[i], the slot's pick, the record's
//                   class (clean_rules.h); per tile the sums of entry bytes,
//                   classes, metadata and payload bytes, the Crc32C of the live
//                   entries' metadata bytes moved to the end of the tile's, and
//                   the four waves' live masks, stored by the one workgroup
//                   that has the tile: no atomics; the tile's victim, found by
//                   bisection of the list, is noted in its line for the later
//                   passes;
//   k_clean_scan    one workgroup: exclusive sums of bytes, live objects, live
//                   tombstones and metadata bytes over the tiles; per-victim
//                   usage from their differences; the fit decision, which
//                   spoils the table when it fails; the certificate from the
//                   tiles' checksums moved to the end of all metadata; the
//                   survivor's status, count and batch counters; the summary;
//   k_clean_move    per tile the offsets again from the masks; each live entry
//                   copied whole (header byte, length bytes, payload) with the
//                   append's granule copy as k_rtab_read_gather posts it; the
//                   survivor's row, work word and old reference; the slot's
//                   pick re-pointed to {N, j};
//   k_clean_claims  every claim that names a victim record becomes the claim
//                   of the slot's pick, which is final by now.
// clean_size is open, mark and scan with no outputs but usage and summary.
//
// The hazard.  A claimant in a victim needs the new place of its key's winner,
// which may be another victim's record that another lane moves.  The move pass
// therefore reads no pick: liveness comes from the mark pass's masks, and a
// lane writes the pick of its own record's slot only (a slot has one winner).
// The claims are fixed one launch later, when every pick names a batch that
// stays: a slot's claim is written by the lane of the record it names and by
// no other.  No slot word is written by two lanes or read while it is written,
// so the passes use plain loads and stores.
// Move and claims leave at once when the table is refused, which is also how
// the scan's "does not fit" reaches them.

namespace {

constexpr uint32_t kClTileWords = 16;    // scratch per tile, one 128-byte line
constexpr uint32_t kClOpenMax = 384;     // victims per k_clean_open launch (3 KiB of arguments)
constexpr int kClSizeShift = 44;         // the move's scan word: entry bytes | records << 44
constexpr uint64_t kClFirstMask = (1ull << 48) - 1;
static_assert(sizeof(ramcrc_clean_usage) == 32 && sizeof(ramcrc_clean_summary) == 112, "clean ABI");
static_assert(kPartThreads == 4 * kWaveSize, "a tile's live masks are four words");

// A tile's line.
enum : uint32_t {
    kClBytes = 0,      // live entry bytes (scan: those before the tile)
    kClClasses = 1,    // live objects | live tombstones << 16 | dropped objects << 32 | dropped tombstones << 48
    kClOther = 2,      // dropped_other | metadata bytes of the live entries << 16
    kClObjBytes = 3,   // payload bytes of the live objects
    kClTombBytes = 4,  // and of the live tombstones
    kClCrc = 5,        // Crc32C (from 0) of the live entries' metadata, at the end of the tile's
    kClObjsBefore = 6, // scan: live objects before the tile
    kClTombsBefore = 7,
    kClMask = 8,       // [4] the waves' live masks
    kClMetaBefore = 12,// scan: metadata bytes before the tile
    kClVictim = 13,    // the tile's victim word (mark), so that move and claims do not search
};

struct ClDesc {
    uint64_t nvic;
    uint64_t ntiles;
    const uint64_t* vic;             // scratch [nvic + 1]: batch << 48 | first tile; the last: ntiles
    uint64_t* tile;                  // scratch [kClTileWords * ntiles]
    uint32_t survivor;               // N
    uint32_t size_only;
    uint64_t out;
    uint64_t cap;
    uint64_t ecap;
    ramcrc_seg_cert* cert;
    ramcrc_seg_status* status;
    u32x4* entries;
    uint64_t* n_entries;
    uint64_t* work;
    uint2* moved;                    // nullable
    ramcrc_clean_usage* usage;       // nullable
    ramcrc_clean_summary* summary;
};

struct ClOpen {
    uint64_t* vic;
    uint64_t first;
    uint32_t n;
    uint64_t w[kClOpenMax];
};

// ------------------------------------------------------------ k_clean_open
__global__ __launch_bounds__(kClOpenMax) void k_clean_open(ClOpen o)
{
    if (threadIdx.x < o.n)
        o.vic[o.first + threadIdx.x] = o.w[threadIdx.x];
}

// The victim that has `tile`: the last one whose first tile is not behind it
// (victims without records have no tile).  The same for every lane.
__device__ __forceinline__ uint64_t clean_victim_of(const ClDesc& c, uint64_t tile)
{
    uint64_t lo = 0, hi = c.nvic;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((c.vic[mid] & kClFirstMask) <= tile)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// XOR of v over the workgroup, in every lane; red: kPartThreads / kWaveSize words.
__device__ __forceinline__ uint32_t clean_block_xor(uint32_t v, uint64_t* red)
{
#pragma unroll
    for (int d = 1; d < kWaveSize; d <<= 1)
        v ^= __shfl_xor(v, d);
    if ((threadIdx.x & (kWaveSize - 1)) == 0)
        red[threadIdx.x / kWaveSize] = v;
    __syncthreads();
    uint32_t x = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPartThreads / kWaveSize; w++)
        x ^= uint32_t(red[w]);
    __syncthreads();   // red is free again
    return x;
}

// ------------------------------------------------------------ k_clean_mark
__global__ __launch_bounds__(kPartThreads) void k_clean_mark(RtabDesc a, ClDesc c)
{
    namespace cl = ramcrc_clean;
    __shared__ uint32_t t0[256];
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a))
        return;
    const uint32_t t = threadIdx.x;
    static_assert(kPartThreads == 256, "one byte-table entry per thread");
    t0[t] = g_tab.t0.t[t];
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < c.ntiles; tile += gridDim.x) {
        const uint64_t vw = c.vic[clean_victim_of(c, tile)];
        const uint32_t b = uint32_t(vw >> 48);
        const RtabBatch& vb = a.batches[b];
        const uint64_t ne = rtab_n_records(vb);
        const uint64_t i = (tile - (vw & kClFirstMask)) * kPartThreads + t;
        uint64_t bytes = 0, classes = 0, other = 0, obytes = 0, tbytes = 0;
        uint32_t hdr = 0, len = 0, nm = 0;
        bool live = false;
        if (i < ne) {
            const uint64_t s = vb.work[i];
            const u32x4 r = vb.entries[i];
            const uint64_t rank = s != kResNone ? ~*rtab_word(a, s, 1) : 0ull;
            const cl::Class k = cl::classify(s, rank, b, i, r.w);
            live = k == cl::kLiveObject || k == cl::kLiveTombstone;
            if (live) {
                hdr = r.w;
                len = r.z;
                nm = cl::meta_bytes(hdr);
                bytes = cl::entry_bytes(hdr, len);
                (k == cl::kLiveObject ? obytes : tbytes) = len;
            }
            if (k == cl::kDroppedOther)
                other = 1;
            else
                classes = 1ull << (16 * uint32_t(k));
        }
        other |= uint64_t(nm) << 16;
        // the entry's metadata checksum, moved to the end of the tile's metadata
        uint64_t mtot;
        const uint64_t mex = part_block_excl(nm, wsum, &mtot);
        uint32_t piece = 0;
        if (live) {
            uint32_t x = 0;
            for (uint32_t k = 0; k < nm; k++)
                x = t0[(x ^ cl::meta_byte(hdr, len, k)) & 0xFF] ^ (x >> 8);
            const uint32_t behind = uint32_t(mtot - mex) - nm;
            piece = behind ? mulmod_dev(x, sl_xpow8(behind)) : x;
        }
        const unsigned long long mask = __ballot(live);
        const uint64_t s_bytes = rtab_block_sum(bytes, wsum);
        const uint64_t s_classes = rtab_block_sum(classes, wsum);
        const uint64_t s_other = rtab_block_sum(other, wsum);
        const uint64_t s_obytes = rtab_block_sum(obytes, wsum);
        const uint64_t s_tbytes = rtab_block_sum(tbytes, wsum);
        const uint32_t crc = clean_block_xor(piece, wsum);
        uint64_t* const ts = c.tile + kClTileWords * tile;
        if ((t & (kWaveSize - 1)) == 0)
            ts[kClMask + t / kWaveSize] = mask;
        if (t == 0) {
            ts[kClBytes] = s_bytes;
            ts[kClClasses] = s_classes;
            ts[kClOther] = s_other;
            ts[kClObjBytes] = s_obytes;
            ts[kClTombBytes] = s_tbytes;
            ts[kClCrc] = crc;
            ts[kClVictim] = vw;
        }
    }
}

// ------------------------------------------------------------ k_clean_scan
// One workgroup, kPartThreads tiles a step.
__global__ __launch_bounds__(kPartThreads) void k_clean_scan(RtabDesc a, ClDesc c)
{
    namespace cl = ramcrc_clean;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_clean_summary sm{};
            sm.spoiled = 1;
            *c.summary = sm;
        }
        return;
    }
    uint64_t carry[4] = {};   // bytes, live objects, live tombstones, metadata bytes
    uint64_t acc[5] = {};     // dropped objects, dropped tombstones, dropped other, object bytes, tombstone bytes
    for (uint64_t tl0 = 0; tl0 < c.ntiles; tl0 += kPartThreads) {
        const uint64_t tl = tl0 + t;
        uint64_t v[4] = {};
        uint64_t* const ts = c.tile + kClTileWords * tl;
        if (tl < c.ntiles) {
            const uint64_t k = ts[kClClasses], o = ts[kClOther];
            v[0] = ts[kClBytes];
            v[1] = k & 0xFFFF;
            v[2] = (k >> 16) & 0xFFFF;
            v[3] = o >> 16;
            acc[0] += (k >> 32) & 0xFFFF;
            acc[1] += k >> 48;
            acc[2] += o & 0xFFFF;
            acc[3] += ts[kClObjBytes];
            acc[4] += ts[kClTombBytes];
        }
        uint64_t ex[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint64_t tot;
            ex[k] = carry[k] + part_block_excl(v[k], wsum, &tot);
            carry[k] += tot;
        }
        if (tl < c.ntiles) {
            ts[kClBytes] = ex[0];
            ts[kClObjsBefore] = ex[1];
            ts[kClTombsBefore] = ex[2];
            ts[kClMetaBefore] = ex[3];
        }
    }
    uint64_t sums[5];
#pragma unroll
    for (int k = 0; k < 5; k++)
        sums[k] = rtab_block_sum(acc[k], wsum);
    const uint64_t need_bytes = carry[0], need_recs = carry[1] + carry[2], meta_all = carry[3];
    const bool fit = c.size_only || cl::fits(need_bytes, need_recs, c.cap, c.ecap);
    __syncthreads();   // every tile's sums before it
    // per-victim usage: the differences of the sums before its first tile and
    // before the next victim's
    uint64_t recs = 0;
    for (uint64_t v = t; v < c.nvic; v += kPartThreads) {
        const uint64_t w0 = c.vic[v], f0 = w0 & kClFirstMask, f1 = c.vic[v + 1] & kClFirstMask;
        const uint64_t n = rtab_n_records(a.batches[w0 >> 48]);
        recs += n;
        if (!c.usage)
            continue;
        uint64_t lo[3] = {carry[0], carry[1], carry[2]}, hi[3] = {carry[0], carry[1], carry[2]};
        if (f0 < c.ntiles) {
            const uint64_t* const ts = c.tile + kClTileWords * f0;
            lo[0] = ts[kClBytes];
            lo[1] = ts[kClObjsBefore];
            lo[2] = ts[kClTombsBefore];
        }
        if (f1 < c.ntiles) {
            const uint64_t* const ts = c.tile + kClTileWords * f1;
            hi[0] = ts[kClBytes];
            hi[1] = ts[kClObjsBefore];
            hi[2] = ts[kClTombsBefore];
        }
        c.usage[v] = ramcrc_clean_usage{n, hi[1] - lo[1], hi[2] - lo[2], hi[0] - lo[0]};
    }
    const uint64_t records = rtab_block_sum(recs, wsum);
    // the certificate: the tiles' checksums moved to the end of all metadata
    uint32_t folded = 0;
    if (fit && !c.size_only) {
        for (uint64_t tl = t; tl < c.ntiles; tl += kPartThreads) {
            const uint64_t* const ts = c.tile + kClTileWords * tl;
            const uint32_t x = uint32_t(ts[kClCrc]);
            if (x) {
                const uint32_t behind = uint32_t(meta_all - ts[kClMetaBefore] - (ts[kClOther] >> 16));
                folded ^= behind ? mulmod_dev(x, sl_xpow8(behind)) : x;
            }
        }
    }
    folded = clean_block_xor(folded, wsum);
    if (t != 0)
        return;
    ramcrc_clean_summary sm{};
    sm.needed_bytes = need_bytes;
    sm.needed_records = need_recs;
    if (!fit) {
        // (the host has retired the victims already: the table cannot go on)
        rtab_refuse(a);
        sm.spoiled = 1;
        *c.summary = sm;
        return;
    }
    sm.victims = c.nvic;
    sm.records = records;
    sm.moved_objects = carry[1];
    sm.moved_tombstones = carry[2];
    sm.object_bytes = sums[3];
    sm.tombstone_bytes = sums[4];
    sm.dropped_objects = sums[0];
    sm.dropped_tombstones = sums[1];
    sm.dropped_other = sums[2];
    sm.out_bytes = need_bytes;
    sm.batch = c.size_only ? 0 : c.survivor;
    *c.summary = sm;
    if (c.size_only)
        return;
    // Segment::getAppendedLength: a fresh Crc32C moved behind the metadata, the
    // entries' metadata, the 4 head bytes, finalized
    const uint32_t head = uint32_t(need_bytes);
    uint32_t x = folded ^ (meta_all ? mulmod_dev(0xFFFFFFFFu, sl_xpow8(uint32_t(meta_all))) : 0xFFFFFFFFu);
    for (int k = 0; k < 4; k++)
        x = g_tab.t0.t[(x ^ (head >> (8 * k))) & 0xFF] ^ (x >> 8);
    *c.cert = ramcrc_seg_cert{head, ~x};
    *c.status = ramcrc_seg_status{RAMCRC_SEG_OK, ~x, uint32_t(need_recs), 0u};
    *c.n_entries = need_recs;
    RtabCount& cnt = a.bcount[c.survivor];
    cnt.objects = carry[1];
    cnt.tombstones = carry[2];
    cnt.malformed = 0;
}

// ------------------------------------------------------------ k_clean_move
__global__ __launch_bounds__(kPartThreads) void k_clean_move(RtabDesc a, ClDesc c)
{
    namespace cl = ramcrc_clean;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];
    __shared__ uint32_t slen[kPartThreads], sbig[kPartThreads];
    __shared__ uint32_t nbig[2];   // by tile parity, as in k_app_copy
    if (rtab_refused(a))
        return;   // spoiled before the call, or the scan found that the survivors do not fit
    const uint32_t t = threadIdx.x;
    if (t == 0)
        nbig[0] = nbig[1] = 0;
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < c.ntiles; tile += gridDim.x, par ^= 1u) {
        __syncthreads();   // the previous tile's copies have read their descriptors and its count
        if (t == 0)
            nbig[par ^ 1u] = 0;   // the next tile's
        const uint64_t* const ts = c.tile + kClTileWords * tile;
        const uint64_t vw = ts[kClVictim];
        const uint32_t b = uint32_t(vw >> 48);
        const RtabBatch& vb = a.batches[b];
        const uint64_t i = (tile - (vw & kClFirstMask)) * kPartThreads + t;
        const bool live = (ts[kClMask + t / kWaveSize] >> (t & (kWaveSize - 1))) & 1;
        u32x4 r{};
        uint64_t size = 0;
        if (live) {
            r = vb.entries[i];
            size = cl::entry_bytes(r.w, r.z);
        }
        uint64_t tot;
        const uint64_t ex = part_block_excl(size | (uint64_t(live) << kClSizeShift), wsum, &tot);
        const uint64_t off = ts[kClBytes] + (ex & ((1ull << kClSizeShift) - 1));
        const uint64_t j = ts[kClObjsBefore] + ts[kClTombsBefore] + (ex >> kClSizeShift);
        uint64_t src = 0, dst = 0;
        uint32_t len = 0;
        // (the scan let the move run only when everything fits; checked again
        // as the last thing between a stale word and a stray store)
        if (live && off + size <= c.cap && j < c.ecap) {
            const uint64_t s = vb.work[i];
            u32x4 row;
            row.x = 0;
            row.y = uint32_t(off);
            row.z = r.z;
            row.w = r.w;
            c.entries[j] = row;
            c.work[j] = s;
            if (c.moved)
                c.moved[j] = make_uint2(b, uint32_t(i));
            *rtab_word(a, s, 1) =
                ~cl::rank_of((r.w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ, c.survivor, j);
            src = vb.base + uint64_t(r.x) * vb.stride + r.y;
            dst = c.out + off;
            len = uint32_t(size);
        }
        ssrc[t] = src;
        sdst[t] = dst;
        slen[t] = len;
        if (len >= kAppBigMin)
            sbig[atomicAdd(&nbig[par], 1u)] = t;
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t k = g; k < kPartThreads; k += kPartThreads / 8) {
            const uint32_t L = slen[k];
            if (L && L <= kAppShortMax)
                app_copy<8, 2>(ssrc[k], sdst[k], L, sub);
            else if (L > kAppShortMax && L < kAppBigMin)
                app_copy<8, 8>(ssrc[k], sdst[k], L, sub);
        }
        const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
        for (uint32_t k = wv; k < nb; k += kPartThreads / kWaveSize) {
            const uint32_t q = sbig[k];
            if (slen[q] < kAppGroupMin)
                app_copy<kWaveSize, 4>(ssrc[q], sdst[q], slen[q], ln);
        }
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t q = sbig[k];
            if (slen[q] >= kAppGroupMin)
                app_copy<kPartThreads, 4>(ssrc[q], sdst[q], slen[q], t);
        }
    }
}

// ---------------------------------------------------------- k_clean_claims
// Every pick names a batch that stays.
__global__ __launch_bounds__(kPartThreads) void k_clean_claims(RtabDesc a, ClDesc c)
{
    namespace cl = ramcrc_clean;
    if (rtab_refused(a))
        return;
    for (uint64_t tile = blockIdx.x; tile < c.ntiles; tile += gridDim.x) {
        const uint64_t vw = c.tile[kClTileWords * tile + kClVictim];
        const uint32_t b = uint32_t(vw >> 48);
        const RtabBatch& vb = a.batches[b];
        const uint64_t ne = rtab_n_records(vb);
        const uint64_t i = (tile - (vw & kClFirstMask)) * kPartThreads + threadIdx.x;
        if (i >= ne)
            continue;
        const uint64_t s = vb.work[i];
        if (s == kResNone || *rtab_word(a, s, 2) != cl::claim_of(b, i))
            continue;
        *rtab_word(a, s, 2) = cl::claim_after(~*rtab_word(a, s, 1));
    }
}

}  // namespace
