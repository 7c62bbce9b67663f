// Segment walks: serial k_seg_walk and the parallel k_walk_* kernels.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {

// ------------------------------------------------------------ segment walk
// Segment::checkMetadataIntegrity (src/Segment.cc:758-800) on the device: one
// wavefront per segment.  The walk is a pointer chase through length-prefixed
// entries (|EntryHeader|length 1-4 B|payload|, src/Segment.h:99-112): latency,
// not bandwidth, bounds it, so everything is arranged to keep one hop short.
//  * The chase reads only LDS.  The segment is staged through 16 KiB windows
//    (coalesced 1 KiB wave loads); while one window is walked the next one is
//    already in flight in registers.  Consecutive windows overlap by 16 bytes,
//    so an entry header and its length bytes (<= 5 B, read as 8) never
//    straddle two windows.  An entry that jumps past the prefetched window
//    reloads at its header: payload bytes of large entries are never fetched.
//  * The metadata checksum is off the chase.  A hop only parks its entry in
//    one lane; every 64 hops the wave checksums the 64 parked header+length
//    byte strings in parallel -- lane j: raw(0, bytes_j) moved past the bytes
//    of the entries after it (x^(8d) from a table, one GF(2) multiply) --
//    XORs them across the wave and folds the batch into the running state:
//    raw(s, A||B) = X^|B|(raw(s, A)) ^ raw(0, B).
// Complete entries are appended to the record table 64 at a time (one atomic
// per 64 records).
constexpr uint32_t kWalkWin = 16384;                          // bytes per window
constexpr uint32_t kWalkStep = kWalkWin - 16;                 // window advance
constexpr int kWalkPer = int(kWalkWin / 16 / kWaveSize);      // 16-byte units per lane
constexpr uint32_t kWalkMeta = 5 * kWaveSize;                 // metadata bytes per batch, max

struct WalkDesc {
    const uint8_t* base;
    uint64_t stride;
    uint64_t capacity;
    uint64_t nseg;
    const ramcrc_seg_cert* certs;
    ramcrc_seg_status* status;
    u32x4* entries;
    uint64_t cap;
    unsigned long long* n_entries;
    const uint32_t* only;   // nullable: walk only the segments with only[seg] != 0
    uint64_t* seg_base;     // nullable: per segment, the first slot of its records
    uint32_t* sum;          // nullable: ORed with the written records' replay_hard bits
};

// CRC32C update by the m (1..4) bytes in the low end of v; t[j][b] = X^(j+1)(b).
__device__ __forceinline__ uint32_t crc_small(const uint32_t* t, uint32_t c, uint32_t v, uint32_t m)
{
    const uint32_t x = c ^ v;
    uint32_t r = m >= 4 ? 0u : (c >> (8 * m));
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (k < m)
            r ^= t[(m - 1 - k) * 256 + ((x >> (8 * k)) & 0xFF)];
    return r;
}

// Issue the loads of window [wbase, wbase + kWalkWin) of a segment (lane l:
// units l + 64 k) as buffer loads whose descriptor ends at the segment's
// capacity: units past it read as zero with no branch, as Segment::copyOut
// leaves bytes past the segment's end.
__device__ __forceinline__ void walk_issue(u32x4 (&r)[kWalkPer], uint64_t sb, uint64_t wbase,
                                           uint64_t capacity, int lane)
{
    const uint64_t base = rfl64(sb + wbase);
    const uint32_t nrec =
        __builtin_amdgcn_readfirstlane(uint32_t(wbase < capacity ? capacity - wbase : 0));
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(base), (short)0, int(nrec),
                                          0x00020000);
#pragma unroll
    for (int k = 0; k < kWalkPer; k++)
        r[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, uint32_t(lane + kWaveSize * k) * 16, 0, 0);
}

__device__ __forceinline__ void walk_store(uint8_t* win, const u32x4 (&r)[kWalkPer], int lane)
{
#pragma unroll
    for (int k = 0; k < kWalkPer; k++)
        *reinterpret_cast<u32x4*>(win + (lane + kWaveSize * k) * 16) = r[k];
}

__global__ __launch_bounds__(kWaveSize) void k_seg_walk(WalkDesc w)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[2][kWalkWin];
    __shared__ __attribute__((aligned(16))) uint32_t tab[4 * 256];
    __shared__ uint32_t xm[kWalkMeta + 1];
    fill_plain(reinterpret_cast<uint8_t*>(tab), 0, &g_tab.pos[1 + kTinyRow0][0], 4 * 256);
    for (uint32_t t = threadIdx.x; t <= kWalkMeta; t += blockDim.x)
        xm[t] = g_tab.xmeta[t];
    __syncthreads();
    const int lane = threadIdx.x;
    uint32_t hard = 0;   // replay_hard bits of the records this wave wrote (w.sum)

    for (uint64_t seg = blockIdx.x; seg < w.nseg; seg += gridDim.x) {
        if (w.only && !w.only[seg])
            continue;   // walked by the parallel walk (uniform per workgroup)
        const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
        const ramcrc_seg_cert cert = w.certs[seg];
        // Two passes: the first counts the records, one atomic allocates them,
        // the second writes them -- so every segment's records are contiguous
        // and in offset order (the parallel walk's are too).
        unsigned long long rbase = 0, rdone = 0, rtotal = 0;
        for (int pass = 0; pass < 2; pass++) {
        uint32_t pos = 0, crc = 0xFFFFFFFFu, count = 0, flags = 0;
        // Parked entries: lane j holds entry j of the current batch of 64 --
        // its offset and the 4 bytes from its header on.  Its length is
        // recovered at the flush from the offset of the entry after it
        // (len = next - pos - 1 - lengthBytes, mod 2^32), so a hop parks two
        // values, not four.
        uint32_t rpos = 0, rq = 0;
        uint32_t ns = 0;

        // Fold the parked entries' header + length bytes into crc and append
        // the first nrec of them to the record table.
        // tail: the offset after the last parked entry (its `next`).
        auto flush = [&](uint32_t nrec, uint32_t tail) {
            const uint32_t pn = __shfl_down(rpos, 1, kWaveSize);
            const uint32_t nxt = lane + 1 == int(ns) ? tail : pn;
            const uint32_t hdr = rq & 0xFF, lb = (hdr >> 6) + 1;
            const uint32_t rlen = nxt - rpos - 1 - lb;
            // a payload past 2^32 (carry out of the reference's uint32_t
            // offset) is unreadable: kRecOverlong
            const uint32_t rinfo = hdr | (rlen > ~(rpos + 1 + lb) ? kRecOverlong : 0u);
            uint32_t m = 0, r = 0;
            if (lane < int(ns)) {
                m = 1 + lb;
                r = crc_small(tab, 0u, hdr | (rlen << 8), m < 4 ? m : 4);
                if (m == 5)
                    r = crc_small(tab, r, rlen >> 24, 1);
            }
            uint32_t incl = m;   // inclusive prefix of the byte counts
#pragma unroll
            for (int s = 1; s < kWaveSize; s <<= 1) {
                const uint32_t y = __shfl_up(incl, s, kWaveSize);
                if (lane >= s)
                    incl += y;
            }
            const uint32_t total = __shfl(incl, kWaveSize - 1, kWaveSize);
            uint32_t c = lane < int(ns) ? mulmod_horner(r, xm[total - incl]) : 0u;
#pragma unroll
            for (int s = 1; s < kWaveSize; s <<= 1)
                c ^= __shfl_xor(c, s, kWaveSize);
            crc = mulmod_horner(crc, xm[total]) ^ c;
            if (nrec && pass == 0) {
                rtotal += nrec;
            } else if (nrec) {
                const unsigned long long b = rbase + rdone;
                if (lane < int(nrec) && b + lane < w.cap) {
                    w.entries[b + lane] = u32x4{uint32_t(seg), rpos, rlen, rinfo};
                    hard |= w.sum ? replay_hard(rpos, rlen, rinfo) | kHardFull : 0u;
                }
                rdone += nrec;
            }
            ns = 0;
        };

        // window state: win[cur] holds [wb, wb + kWalkWin); pf is loading
        // [wb + kWalkStep, ...)
        int cur = 0;
        uint32_t wb = 0;
        u32x4 pf[kWalkPer];
        __syncthreads();   // the previous segment's LDS reads are done
        walk_issue(pf, sb, 0, w.capacity, lane);
        walk_store(win[0], pf, lane);
        walk_issue(pf, sb, kWalkStep, w.capacity, lane);
        __syncthreads();

        // The chase: every value below is wave-uniform (scalar registers).
        // The outer loop moves windows, flushes full batches and stops the
        // walk; the inner loop is the hop itself -- one LDS read and a few
        // scalar operations -- and runs while the entry header stays inside
        // the window, the batch has room and the cycle bound is not reached.
        const uint32_t cap32 = uint32_t(w.capacity);
        const uint32_t limit = cert.segment_length < cap32 ? cert.segment_length : cap32;
        uint32_t steps = 0, tail = 0;
        bool overrun = false;
        while (pos < limit) {
            // deterministic walk below the capacity: more steps than bytes means
            // a repeated position, i.e. the reference's loop never ends
            if (steps >= cap32) {
                flags |= RAMCRC_SEG_CYCLE;
                break;
            }
            if (pos - wb > kWalkWin - 8) {   // (a position below wb wraps: reload)
                const uint64_t nb = uint64_t(wb) + kWalkStep;
                if (uint64_t(pos) >= nb && uint64_t(pos) - nb <= kWalkWin - 8) {
                    walk_store(win[cur ^ 1], pf, lane);   // the prefetched window
                    cur ^= 1;
                    wb = uint32_t(nb);
                } else {                                    // a jump: reload at the header
                    wb = pos & ~15u;
                    walk_issue(pf, sb, wb, w.capacity, lane);
                    walk_store(win[cur], pf, lane);
                }
                __syncthreads();
                walk_issue(pf, sb, uint64_t(wb) + kWalkStep, w.capacity, lane);
            }
            if (ns == uint32_t(kWaveSize))
                flush(ns, pos);
            const uint32_t* w32 = reinterpret_cast<const uint32_t*>(win[cur]);
            // hop while pos - wb <= span (header + 7 bytes inside the window, pos
            // below the limit) and the batch and the cycle bound have room
            const uint64_t wend = uint64_t(wb) + (kWalkWin - 8);
            const uint32_t last = limit - 1 < wend ? limit - 1 : uint32_t(wend);
            const uint32_t span = last - wb;
            // the batch and the cycle bound: at most nsmax - ns hops
            uint32_t nsmax = uint32_t(kWaveSize);
            if (cap32 - steps < nsmax - ns)
                nsmax = ns + (cap32 - steps);
            const uint32_t ns0 = ns;
            uint32_t next;
            for (;;) {
                const uint32_t o = pos - wb;
                const uint32_t d0 = __builtin_amdgcn_readfirstlane(w32[o >> 2]);
                const uint32_t d1 = __builtin_amdgcn_readfirstlane(w32[(o >> 2) + 1]);
                const uint64_t q = ((uint64_t(d1) << 32) | d0) >> (8 * (o & 3));
                const uint32_t t = (uint32_t(q) >> 6) & 3;   // getLengthBytes() - 1
                // len = the t + 1 bytes after the header: one s_bfe_u64, field
                // {offset 8, width 8 t + 8}
                uint32_t fld;
                uint64_t len64;
                asm("s_lshl_b32 %0, %2, 19\n\ts_add_u32 %0, %0, 0x80008\n\ts_bfe_u64 %1, %3, %0"
                    : "=&s"(fld), "=s"(len64) : "s"(t), "s"(q) : "scc");
                // uint32_t arithmetic, as the reference (a wrap is legal)
                next = pos + t + 2 + uint32_t(len64);
                const bool mine = lane == int(ns);   // park: one compare, two selects
                rpos = mine ? pos : rpos;
                rq = mine ? uint32_t(q) : rq;
                ns++;
                // the next header leaves the window or the limit (this also
                // covers next > capacity and a wrapped next)
                if (next - wb > span)
                    break;
                if (ns == nsmax)   // the batch is full, or the cycle bound
                    break;
                pos = next;
            }
            steps += ns - ns0;
            tail = next;
            if (next > cap32) {
                // the last hop's header and length were checksummed; that
                // entry is not a record
                flags |= RAMCRC_SEG_PAST_CAPACITY;
                overrun = true;
                break;
            }
            pos = next;
        }
        count = steps - (overrun ? 1u : 0u);
        if (ns)
            flush(overrun ? ns - 1 : ns, tail);
        if (pass == 0) {
            unsigned long long b = 0;
            if (lane == 0 && rtotal)
                b = atomicAdd(w.n_entries, rtotal);
            rbase = __shfl(b, 0, kWaveSize);
            if (lane == 0 && w.seg_base)
                w.seg_base[seg] = rbase;
            if (rtotal == 0)
                pass = 1;   // nothing to write: the second pass is this one
        }
        if (rbase + rtotal > w.cap)
            flags |= RAMCRC_SEG_TABLE_FULL;
        if (pass == 0)
            continue;
        const uint32_t fin = ~crc_small(tab, crc, cert.segment_length, 4);
        if (!(flags & (RAMCRC_SEG_PAST_CAPACITY | RAMCRC_SEG_CYCLE))) {
            if (pos > cert.segment_length)
                flags |= RAMCRC_SEG_PAST_LENGTH;
            else if (fin != cert.checksum)
                flags |= RAMCRC_SEG_BAD_CHECKSUM;
            else if (!(flags & RAMCRC_SEG_TABLE_FULL))
                flags |= RAMCRC_SEG_OK;   // records dropped: not verified, never OK
        }
        if (lane == 0) {
            ramcrc_seg_status st;
            st.flags = flags;
            st.checksum = fin;
            st.entries = count;
            st.bad_objects = 0;
            w.status[seg] = st;
        }
        }   // pass
    }
    {
        const uint32_t hw = (__ballot(hard & 1u) ? 1u : 0u) | (__ballot(hard & 2u) ? 2u : 0u) |
                           (__ballot(hard & 4u) ? 4u : 0u) | (__ballot(hard & kHardFull) ? kHardFull : 0u);
        if (w.sum && hw && lane == 0)
            atomicOr(w.sum, hw);
    }
}

// ------------------------------------------------- parallel segment walk
// The walk of Segment::checkMetadataIntegrity (src/Segment.cc:758-800) is a
// chain: entry i+1 starts where entry i's length says.  One wave chasing it
// through a whole 8 MiB segment (k_seg_walk) is latency-bound at ~160 ns a
// hop, and a 512-segment batch is only 512 chains.  Here every segment is cut
// into 64 KiB parts and the chain is found in every part at once:
//
//  A0 k_walk_sync   per part k >= 1 (one wave): the first offset in the part
//                   from which kSyncHops consecutive hops each land on a
//                   header of a valid LogEntryType (src/LogEntryTypes.h:29-68,
//                   type < 12) inside the segment -- a guess of where the
//                   chain enters the part.  Candidates are tested 512 at a
//                   time, all hops of all live candidates issued together.
//  A  k_walk_parts  per part (one lane): the reference's walk from the guess
//                   (part 0: from offset 0) until it leaves the part or
//                   reaches min(certificate length, capacity): entries,
//                   the raw CRC of their header + length bytes, exit offset.
//  B  k_walk_fix    per segment (one wave): the true chain, part by part in
//                   order.  A part is accepted when the chain arrives exactly
//                   at its guess (the walk is deterministic, so its result is
//                   then the reference's); a part the chain skips is ignored;
//                   otherwise the part is walked again from the true offset.
//                   The accepted parts' metadata CRCs are combined with
//                   raw(0, A||B) = X^|B|(raw(0, A)) ^ raw(0, B), the status is
//                   written and the segment's records are allocated.
//  C  k_walk_emit   per accepted part (one lane): walk again, writing the
//                   records in order at their final slots.
// A segment whose chain wraps the reference's uint32_t offset (it would then
// walk backwards, or forever) or needs too many re-walks is handed to the
// serial walker k_seg_walk, which implements those semantics.  The result of
// every segment -- flags, checksum, entry count, records -- equals the serial
// walk's (tests/test_gpu_segments.py runs both against the oracle).
#ifndef RAMCRC_PART_SHIFT
#define RAMCRC_PART_SHIFT 16
#endif
constexpr uint32_t kPartShift = RAMCRC_PART_SHIFT;  // default parts: 64 KiB
constexpr uint32_t kPartShiftMin = 13;               // smallest part (RAMCRC_OPT_WALK_PART_SHIFT)
constexpr uint32_t kNoStart = 0xFFFFFFFFu;
#ifndef RAMCRC_SYNC_HOPS
#define RAMCRC_SYNC_HOPS 6
#endif
#ifndef RAMCRC_SYNC_PER
#define RAMCRC_SYNC_PER 8
#endif
#ifndef RAMCRC_SYNC_STAGE_KIB
#define RAMCRC_SYNC_STAGE_KIB 7
#endif
constexpr int kSyncHops = RAMCRC_SYNC_HOPS;         // hops a guess must survive
constexpr int kSyncPer = RAMCRC_SYNC_PER;           // candidates per lane per round
constexpr uint32_t kSyncRound = kSyncPer * kWaveSize;   // 512 candidates
static_assert(kSyncPer % 4 == 0 && kSyncPer <= 32, "candidates per lane: whole dwords");
constexpr uint32_t kSyncSpan = 16384;               // candidate bytes searched per part
constexpr uint32_t kSyncStage = RAMCRC_SYNC_STAGE_KIB * 1024;   // staged bytes per wave (k_walk_sync)
constexpr uint32_t kMeetMax = 4;                    // B's fast path: meets within 4 records
constexpr uint32_t kMeetHops = 3;                   // ... after at most 3 entries walked
constexpr uint32_t kRewalkBudget = 1u << 15;        // hops B may re-walk before falling back
// part flags
constexpr uint32_t kPartWalked = 1u, kPartWrap = 2u, kPartOverrun = 4u, kPartEmit = 8u;
constexpr uint32_t kPartSpill = 16u;   // A: more records than its scratch holds
constexpr uint32_t kPartChase = 32u;   // B: walked again; C walks it once more
constexpr uint32_t kPartHuge = 64u;    // A: an entry of 16 MiB or more (records hold 24-bit lengths)
constexpr uint32_t kMaxBlocks = 15;    // pool blocks per part: records 64 .. 1023 of A's walk
constexpr uint32_t kPartRec = 64;      // records A keeps per part (C copies them)

struct PartRes {
    uint32_t start;    // A0: guess (kNoStart: none); B: the true start of an emitting part
    uint32_t exit;     // A: offset where the part's walk stopped
    uint32_t count;    // A: entries (records)
    uint32_t nmeta;    // A: header + length bytes checksummed
    uint32_t raw;      // A: raw(0, those bytes)
    uint32_t flags;    // kPart*
    uint64_t rec;      // B: first record slot of the part
    uint32_t pre;      // B: entries walked before meeting the guessed chain (C walks them)
    uint32_t cut;      // B: junk entries at the head of the guessed chain (C skips them)
};

struct PWalk {
    const uint8_t* base;
    uint64_t stride;
    uint32_t capacity;
    uint32_t nparts;
    uint64_t nseg;
    const ramcrc_seg_cert* certs;
    ramcrc_seg_status* status;
    u32x4* entries;
    uint64_t cap;
    unsigned long long* n_entries;
    PartRes* parts;
    uint32_t* fallback;   // per segment: nonzero = walked by k_seg_walk
    uint64_t* seg_base;   // per segment: first record slot (B)
    uint2* recs;          // per part: kPartRec records of A's walk {offset, length << 8 | header}
    uint32_t pshift;      // log2 part bytes of this launch (from *geo when geo is set)
    const uint32_t* geo;  // the part shift k_walk_probe chose for this batch
    // A's records past the first kPartRec of a part: blocks of kPartRec from a
    // pool (one atomic per block), up to kMaxBlocks per part
    uint2* pool;
    uint32_t* pool_owner;            // per pool block: part * 16 + block number (1 ..)
    uint32_t* blocks;                // per part: kMaxBlocks pool block indices
    unsigned long long* pool_used;   // blocks taken (zeroed per launch)
    uint64_t pool_cap;               // pool blocks
    uint32_t* sum;                   // nullable: as WalkDesc::sum
    // the fused replay call's verify-in-walk mode (kSumFast, k_walk_copyv):
    uint32_t* obj_crc;               // nullable: per record slot, Object::computeChecksum
    uint32_t* left;                  // record slots left to k_left (other types, emitted records)
    unsigned long long* nleft;       // their count (zeroed by k_walk_probe)
    uint64_t left_cap;
    uint32_t vmode;                  // RAMCRC_OPT_VERIFY_IN_WALK: 1 small entries (probe), 2 always
};

typedef const __attribute__((address_space(1))) uint32_t gu32;

// The bytes from pos on (at least 5: the header and up to 4 length bytes), as
// Segment::copyOut would give them: bytes at or past the capacity read 0.
// Two aligned dword loads (pos < capacity, capacity % 16 == 0).
__device__ __forceinline__ uint64_t seg_peek(uint64_t seg, uint32_t pos, uint32_t capacity)
{
    const uint32_t a = pos & ~3u;
    const bool two = a + 4 < capacity;
    const uint32_t w0 = *reinterpret_cast<gu32*>(seg + a);
    uint32_t w1 = *reinterpret_cast<gu32*>(seg + (two ? a + 4 : a));
    w1 = two ? w1 : 0u;
    return ((uint64_t(w1) << 32) | w0) >> (8 * (pos & 3));
}

// raw CRC update by an entry's header + length bytes (2..5 of them, from q).
__device__ __forceinline__ uint32_t meta_update(const uint32_t* tab, uint32_t c, uint64_t q,
                                                uint32_t mbytes)
{
    c = crc_small(tab, c, uint32_t(q), mbytes < 4 ? mbytes : 4);
    if (mbytes == 5)
        c = crc_small(tab, c, uint32_t(q >> 32), 1);
    return c;
}

// x^(8d) for any 32-bit d.
__device__ __forceinline__ uint32_t xpow8_dev(uint32_t d)
{
    uint32_t r = ramcrc::kOne;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = (d >> (8 * j)) & 0xFF;
        if (b)
            r = r == ramcrc::kOne ? g_tab.xbyte[j][b] : mulmod_dev(r, g_tab.xbyte[j][b]);
    }
    return r;
}

__device__ __forceinline__ uint32_t walk_limit(const PWalk& w, uint64_t seg)
{
    const uint32_t len = w.certs[seg].segment_length;
    return len < w.capacity ? len : w.capacity;
}

// The part geometry of this batch: every walk kernel takes it from the word
// k_walk_probe wrote (the host sizes its grids and scratch for the smallest
// part the probe may choose).
__device__ __forceinline__ PWalk walk_geo(PWalk w)
{
    if (w.geo) {
        w.pshift = *w.geo;
        w.nparts = uint32_t((uint64_t(w.capacity) + (1ull << w.pshift) - 1) >> w.pshift);
    }
    return w;
}

// Part size per batch from the entry density.  A part should hold about 64
// entries: much fewer and the sync search (which stages the first 7 KiB of
// a part and chases 6 hops) mostly finds no header or chases far through
// global memory, and k_walk_fix re-walks the part; much more and the one-lane
// part walks get long (profiles/r04/parts: 8 KiB values 1.90 TB/s with 64 KiB
// parts, 3.85 with 512 KiB; 64 B values 1.25 with 64 KiB, 0.78 with 128 KiB).
// One wave: lane l walks the first kProbeHops entries of one of up to 64
// segments spread over the batch; the mean entry size m gives the shift
// round(log2(64 m)) within [kPartShift, kPartShiftMax].  A forced shift
// (RAMCRC_OPT_WALK_PART_SHIFT) is written as is.
constexpr uint32_t kPartShiftMax = 20;
constexpr int kProbeHops = 8;
constexpr uint32_t kPartShiftLow = kPartShift;   // the smallest part the probe picks

// The replay summary word (PWalk::sum, replay_hard bits) only gains bits
// within a batch.  A wave reads it (coherently) and ORs only the bits it
// would add: with 1 KiB objects every wave has hard records, and 32K
// same-address atomics cost 175 us per batch when k_walk_copy made them
// (profiles/r05/replayfix).  No word: everything counts as seen.
__device__ __forceinline__ uint32_t walk_sum_seen(const uint32_t* sum)
{
    return sum ? __hip_atomic_load(sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kHardAll;
}

// Verify in the walk (round 6).  When the probe finds small entries (mean
// at most kFastMean bytes: the objects of 64- and 128-byte values) in a fused
// replay call, it sets kSumFast and the record copy becomes k_walk_copyv: it
// stages each block of 64 records' object bytes in LDS with coalesced loads
// and checksums every object there, one lane per object, as it writes the
// record -- so the object bytes are read once, by streaming loads, and the
// binned object scan (k_bin_* + k_entries) has nothing left to do.  Records
// it cannot check that way (other replayed types, records k_walk_emit writes)
// go to a list k_left checks one lane per record; any record neither can take
// (an object of 64 KiB or more, a segment the serial walker took, a full
// list) sets kHardFull, and then the usual verify runs over the whole table.
#ifndef RAMCRC_FAST_MEAN
#define RAMCRC_FAST_MEAN 176   // largest mean entry (bytes, probe) that takes it: 64 of
                               // them (a block of records) fit k_walk_copyv's 12 KiB stage
#endif
constexpr uint32_t kFastMean = RAMCRC_FAST_MEAN;
constexpr uint32_t kFastMean8 = 120;   // ... and k_walk_copyv's 8 KiB stage up to this mean

// A record written outside k_walk_copyv in verify-in-walk mode: to k_left's
// list, or the full path when the list cannot take it or the record is an
// object longer than kLeftMax (k_left's byte loop is one thread per record).
constexpr uint32_t kLeftMax = 1024;
__device__ __forceinline__ uint32_t left_append(const PWalk& w, uint64_t slot, uint32_t len, uint32_t hdr)
{
    const uint32_t type = hdr & 0x3f;
    if (replay_header_bytes(type) == 0)
        return 0u;   // nothing replay checks
    if (type == RAMCRC_LOG_ENTRY_TYPE_OBJ && !(hdr & kRecOverlong) && len >= kObjHeaderBytes &&
        len > kLeftMax)
        return kHardFull;   // a longer object (k_entries / k_chunks): the full path
    const unsigned long long k = atomicAdd(w.nleft, 1ull);
    if (k >= w.left_cap || slot > 0xFFFFFFFFull)
        return kHardFull;
    w.left[k] = uint32_t(slot);
    return 0u;
}

__global__ __launch_bounds__(kWaveSize) void k_walk_probe(PWalk w, uint32_t forced, uint32_t* geo)
{
    const int lane = threadIdx.x;
    const uint64_t ns = w.nseg < uint64_t(kWaveSize) ? w.nseg : uint64_t(kWaveSize);
    uint64_t dist = 0, hops = 0;
    if (!forced && uint64_t(lane) < ns) {
        const uint64_t seg = uint64_t(lane) * w.nseg / ns;
        const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
        const uint32_t limit = walk_limit(w, seg);
        uint32_t pos = 0;
        for (int hh = 0; hh < kProbeHops && pos < limit; hh++) {
            const uint64_t q = seg_peek(sb, pos, w.capacity);
            const Hop h = hop_of(q, pos);
            if (!plausible(q, h, w.capacity) || h.next > limit)
                break;
            dist += h.next - pos;
            hops++;
            pos = uint32_t(h.next);
        }
    }
#pragma unroll
    for (int o = 1; o < kWaveSize; o <<= 1) {
        dist += __shfl_xor(dist, o, kWaveSize);
        hops += __shfl_xor(hops, o, kWaveSize);
    }
    if (lane == 0) {
        // the batch's counters, zeroed here rather than by three memsets
        // ahead of this launch (each a few microseconds on the stream)
        *w.n_entries = 0;
        w.pool_used[0] = 0;
        if (w.nleft)
            *w.nleft = 0;
        uint32_t shift = kPartShift;
        if (forced) {
            shift = forced;
        } else if (hops) {
            const uint64_t t = 64 * (dist / hops);   // bytes of 64 entries
            uint32_t l = 63 - uint32_t(__builtin_clzll(t | 1));   // floor(log2 t)
            // round to nearest in log scale: up when t >= 2^l * sqrt(2)
            if (t * t >= (1ull << (2 * l)) * 2)
                l++;
            shift = l < kPartShift ? kPartShift : (l > kPartShiftMax ? kPartShiftMax : l);
            // 128 KiB parts never won (profiles/r06/shift: 1 KiB values
            // -0.5 % against 64 KiB, 2 KiB values -9 % against 256 KiB --
            // the sync search's six validation hops leave its 7 KiB stage
            // and chase through global memory -- and 4 KiB -12 %): the
            // entries that round to them (≈ 1.45 .. 2.9 KiB) take 256 KiB
            if (shift == 17)
                shift = 18;
        }
        *geo = shift;
        // the sync search's stage (k_walk_sync) is sized for 16 mean entries
        // (1 KiB .. kSyncStage; a forced shift keeps kSyncStage) -- a dense batch's six-hop
        // chains fit a few hundred bytes, and every staged byte is read again
        // by the part walk
        uint32_t sstage = kSyncStage;
        if (!forced && hops) {
            const uint64_t want = ((16 * (dist / hops)) + 1023) & ~uint64_t(1023);
            sstage = uint32_t(want < 1024 ? 1024 : (want > kSyncStage ? kSyncStage : want));
        }
        geo[1] = sstage;
        if (w.sum) {
            const bool fast = w.obj_crc && w.nleft &&
                              (w.vmode == 2 || (hops && dist <= uint64_t(kFastMean) * hops));
            const bool small = hops && dist <= uint64_t(kFastMean8) * hops;
            *w.sum = fast ? (kSumFast | (small ? kSumStage8 : 0u)) : 0u;
        }
    }
}

// A0: one wave per part k >= 1.  The part's first kSyncWin bytes are staged
// in LDS, so most candidate hops (the true chain's included, for entries of
// a few KiB) read LDS instead of waiting on global memory.
constexpr uint32_t kSyncWin = kSyncStage - 16;       // candidates / hops read from LDS below this
constexpr int kSyncWaves = 4;                        // waves per workgroup
constexpr uint64_t kSyncJunkKey = 1ull << 63;        // search key bit: a survivor of the other class

// Wave minimum through DPP (quad swaps, half-row and row mirrors, row
// broadcasts): the result is valid in lane 63 and returned uniform.
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0xB1, 0xF, 0xF, false)));   // quad_perm 1,0,3,2
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0x4E, 0xF, 0xF, false)));   // quad_perm 2,3,0,1
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0x141, 0xF, 0xF, false)));  // row_half_mirror
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0x140, 0xF, 0xF, false)));  // row_mirror
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0x142, 0xA, 0xF, false)));  // row_bcast:15
    v = min(v, uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), 0x143, 0xC, 0xF, false)));  // row_bcast:31
    return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

// One part of the sync search.  The certificate length is loaded with the
// stage and used a search later, so its latency is not exposed either.
struct SyncPart {
    uint64_t sb;       // segment base address
    uint32_t k;        // part number in the segment
    uint32_t B;        // first byte of the part
    uint32_t seglen;   // certificate segment length
};

__device__ __forceinline__ SyncPart sync_part(const PWalk& w, uint64_t i)
{
    SyncPart P;
    const uint64_t seg = i / w.nparts;
    P.k = uint32_t(i - seg * w.nparts);
    P.B = P.k << w.pshift;
    P.seglen = w.certs[seg].segment_length;
    P.sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
    return P;
}

__global__ __launch_bounds__(kSyncWaves * kWaveSize) void k_walk_sync(PWalk w0)
{
    const PWalk w = walk_geo(w0);
    __shared__ __attribute__((aligned(16))) uint8_t wins[kSyncWaves][kSyncStage];
    __shared__ uint16_t lists[kSyncWaves][kSyncRound];   // a round's first-hop survivors
    constexpr uint32_t kSU = kSyncStage / 1024;
    const int lane = threadIdx.x & (kWaveSize - 1);
    const int wv = threadIdx.x / kWaveSize;
    uint8_t* win = wins[wv];
    uint16_t* list = lists[wv];
    const uint64_t nwave = uint64_t(gridDim.x) * kSyncWaves;
    const uint64_t total = w.nseg * w.nparts;
    // stage [B, B + kSyncStage): bytes at or past the capacity are 0.  All
    // loads are issued before the first store (one memory latency, not one
    // per 1 KiB), and the loads of the wave's next part are
    // in flight while this part is searched.  The LDS is wave-private.
    u32x4 v[kSU];
    // staged bytes of this batch (a multiple of 1 KiB, at most kSyncStage)
    const uint32_t ss = w.geo ? __builtin_amdgcn_readfirstlane(w.geo[1]) : kSyncStage;
    auto stage_load = [&](const SyncPart& P) {
#pragma unroll
        for (uint32_t u = 0; u < kSU; u++) {
            const uint64_t a = uint64_t(P.B) + u * 1024 + uint32_t(lane) * 16;
            if (u * 1024 < ss)   // uniform
                v[u] = a + 16 <= w.capacity ? load16(P.sb + a) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    uint64_t i = uint64_t(blockIdx.x) * kSyncWaves + wv;
    SyncPart nxt{};
    if (i < total) {
        nxt = sync_part(w, i);
        if (nxt.k != 0)
            stage_load(nxt);
    }
    for (; i < total; i += nwave) {
        const SyncPart P = nxt;
        const uint32_t B = P.B;
        const uint64_t sb = P.sb;
        const uint32_t limit = P.seglen < w.capacity ? P.seglen : w.capacity;   // walk_limit
        uint64_t end64 = uint64_t(B) + kSyncSpan;
        end64 = end64 < uint64_t(B) + (1ull << w.pshift) ? end64 : uint64_t(B) + (1ull << w.pshift);
        end64 = end64 < w.capacity ? end64 : w.capacity;
        const uint32_t end = uint32_t(end64 < limit ? end64 : limit);
        const bool search_part = P.k != 0 && end > B;   // part 0 starts at offset 0
        if (search_part) {
#pragma unroll
            for (uint32_t u = 0; u < kSU; u++)
                if (u * 1024 < ss)
                    *reinterpret_cast<u32x4*>(win + u * 1024 + uint32_t(lane) * 16) = v[u];
        }
        if (i + nwave < total) {
            nxt = sync_part(w, i + nwave);
            if (nxt.k != 0)   // (also for a part past the segment length: not known yet)
                stage_load(nxt);
        }
        if (!search_part) {
            if (P.k != 0 && lane == 0)
                w.parts[i].start = kNoStart;
            continue;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // stores land before the reads
        auto peek_lds = [&](uint32_t p) -> uint64_t {   // the bytes from p (B <= p, p + 8 <= B + kSyncStage)
            const uint32_t o = p - B;
            const uint32_t* w32 = reinterpret_cast<const uint32_t*>(win + (o & ~3u));
            return ((uint64_t(w32[1]) << 32) | w32[0]) >> (8 * (o & 3));
        };
        auto peek = [&](uint32_t p) -> uint64_t {   // the bytes from p (>= B)
            return p - B + 8 <= ss ? peek_lds(p) : seg_peek(sb, p, w.capacity);
        };
        // Candidates in rounds of 512 from B.  A candidate survives when its
        // chain makes kSyncHops plausible hops (or reaches the limit).  A
        // junk header whose length happens to land on a real header survives
        // too, and then skips the real entries it jumps over.  The real first
        // entry h is two real entries ahead after two hops, while a junk chain
        // that lands on the real chain only after skipping some of it is
        // further ahead: the survivor whose second hop lands nearest is kept
        // (ties: the lower candidate; a junk chain that wins has met the real
        // chain within two entries, which k_walk_fix resolves in as many
        // hops).  The scan ends with the first round that holds a survivor
        // (a junk survivor from an earlier position is then
        // met by k_walk_fix or its part walked again), or else at the nearest
        // first hop seen.  The guess only decides how much k_walk_fix re-walks,
        // never a result.  Replay A/B (profiles/r03/walk): stopping early cut
        // this kernel from 217 to 157 us on 1 KiB objects, but with the
        // permissive hop test alone it doubled k_walk_fix (more junk guesses);
        // with the strict test (see the hop loop) the step is 4.8 % faster.
        // Per round: lane l filters candidates c0 + 8 l + j (j < 8) four at a
        // time with byte-parallel (SWAR) tests on the words it holds
        // (first_hop4); the ~10 % that pass are listed in LDS and chased one
        // per lane, level by level (level 0 is the exact plausible() test),
        // and the wave minima are DPP reductions.  LDS-only: a hop
        // that leaves the staged window ends the candidate (no global round
        // trip for any lane); otherwise beyond-window hops read global memory.
        const bool kill4 = w.capacity <= (1u << 24);   // a 4-byte length ends past it
        const bool kill3 = w.capacity <= (1u << 23);   // so does a 3-byte one >= 2^23
        // The LDS-only instance has no global load: the waits a global peek
        // brings would also wait for the next part's stage loads.
        auto search = [&](auto lds_only_c, uint32_t to) -> uint32_t {
            constexpr bool lds_only = decltype(lds_only_c)::value;
            auto peek_any = [&](uint32_t p) -> uint64_t {
                if constexpr (lds_only)
                    return peek_lds(p);
                else
                    return peek(p);
            };
            const uint32_t wend = B + ss - 16;   // peeks below wend stay in LDS
            uint64_t best = ~0ull;                // (position after two hops << 32) | candidate
            uint32_t bound = 0xFFFFFFFFu;         // nearest first hop of a survivor: h lies below it
            // (early stop: once a survivor of the preferred class is known)
            for (uint32_t c0 = B; c0 < to && c0 < bound && !(best < kSyncJunkKey);
                 c0 += kSyncRound) {
                const uint32_t cl = c0 + uint32_t(lane) * kSyncPer;
                constexpr int kWords = (kSyncPer / 4 + 3) & ~1;
                uint32_t d[kWords];   // bytes [cl, cl + kSyncPer + 8) and up to 4 more
#pragma unroll
                for (int u = 0; u < kWords; u += 2) {
                    // (LDS-only: words past the window belong to candidates >= to, masked below)
                    const uint32_t pc = cl + 4 * u;
                    const uint64_t v = peek_any(lds_only && pc - B > ss - 8 ? B + ss - 8 : pc);
                    d[u] = uint32_t(v);
                    d[u + 1] = uint32_t(v >> 32);
                }
                uint32_t alive = 0;
#pragma unroll
                for (int g = 0; g < kSyncPer / 4; g++)
                    alive |= first_hop4(d[g], __builtin_amdgcn_alignbyte(d[g + 1], d[g], 3), kill4,
                                        kill3)
                             << (4 * g);
                alive &= to > cl ? (to - cl >= kSyncPer ? ~0u : (1u << (to - cl)) - 1u) : 0u;
                // survivors listed slot-major in LDS (offsets from c0)
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < kSyncPer; j++) {
                    const uint64_t m = __ballot((alive >> j) & 1);
                    const uint32_t at = total + __builtin_amdgcn_mbcnt_hi(
                                                    uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                    if ((alive >> j) & 1)
                        list[at] = uint16_t(uint32_t(lane) * kSyncPer + j);
                    total += uint32_t(__popcll(m));
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                for (uint32_t t0 = 0; t0 < total; t0 += kWaveSize) {
                    const bool have = t0 + uint32_t(lane) < total;
                    const uint32_t c = c0 + (have ? list[t0 + uint32_t(lane)] : 0u);
                    bool live = have;
                    bool junk = false;   // a hop whose entry is neither an object nor a tombstone
                    uint32_t p = c, first = 0, second = 0;
                    for (int hh = 0; hh < kSyncHops && __ballot(live && p < limit); hh++) {
                        if (live && p < limit) {   // (at the limit the walk ends: keep)
                            if (hh > 0 && lds_only && p >= wend) {
                                live = false;
                            } else {
                                const uint64_t q = peek_any(p);
                                const Hop h = hop_of(q, p);
                                // (guess heuristics, beyond plausible(): a real chain
                                // neither crosses the segment length nor holds an
                                // empty entry -- junk chains through structured
                                // object headers do both)
                                if (plausible(q, h, w.capacity) && h.next <= limit && h.len != 0) {
                                    p = uint32_t(h.next);
                                    const uint32_t ty = uint32_t(q) & 0x3F;
                                    junk = junk || (ty != RAMCRC_LOG_ENTRY_TYPE_OBJ &&
                                                    ty != RAMCRC_LOG_ENTRY_TYPE_OBJTOMB);
                                } else {
                                    live = false;
                                }
                            }
                        }
                        if (hh == 0)
                            first = p;
                        if (hh == 1)
                            second = p;
                    }
                    if (second == 0)
                        second = p;
                    if (first == 0)
                        first = p;
                    const uint32_t fb = wave_min(live ? first : 0xFFFFFFFFu);
                    bound = fb < bound ? fb : bound;
                    // nearest second hop, ties to the lower candidate; chains of
                    // objects and tombstones first: a fixed
                    // object layout can hold a junk chain of another type that
                    // runs beside the real one at the same stride and never meets
                    // it, and then beats it on the second hop -- k_walk_fix then
                    // re-walks the whole part (128 B values: 0.37 ms per batch)
                    for (int cls = 0; cls < 2; cls++) {
                        const bool lc = live && (cls == 1 || !junk);
                        const uint32_t s2 = wave_min(lc ? second : 0xFFFFFFFFu);
                        if (s2 != 0xFFFFFFFFu) {
                            const uint64_t tie = __ballot(lc && second == s2);
                            const uint32_t lo = __popcll(tie) == 1
                                                    ? uint32_t(__builtin_amdgcn_readlane(int(c), __builtin_ctzll(tie)))
                                                    : wave_min(lc && second == s2 ? c : 0xFFFFFFFFu);
                            const uint64_t key = (cls ? kSyncJunkKey : 0ull) |
                                                 (uint64_t(s2) << 32) | lo;
                            best = key < best ? key : best;
                            break;
                        }
                    }
                }
            }
            return best == ~0ull ? kNoStart : uint32_t(best);   // (bit 63, the class, dropped)
        };
        // entries of up to ~2 KiB: found with LDS reads alone; longer ones
        // (their chain leaves the window) by the general search
        const uint32_t lds_to = B + ss - 24 < end ? B + ss - 24 : end;
        uint32_t guess = search(std::true_type{}, lds_to);
        if (guess == kNoStart)
            guess = search(std::false_type{}, end);
        if (lane == 0)
            w.parts[i].start = guess;
    }
}

// The reference walk from `pos` while pos < stop (at most `budget` hops), as
// one lane: fills the part result (count, metadata bytes and raw CRC, exit,
// wrap / overrun flags) and hands every record to sink(index, offset,
// length, header byte).
// seg_peek on one segment.
struct GlobalPeek {
    uint64_t sb;
    uint32_t capacity;
    __device__ uint64_t operator()(uint32_t p) const { return seg_peek(sb, p, capacity); }
};

template <class Sink, class Peek>
__device__ __forceinline__ void walk_lane(const PWalk& w, const uint32_t* tab, uint32_t pos,
                                          uint32_t stop, PartRes& r, Sink&& sink, uint32_t budget,
                                          Peek&& peek)
{
    uint32_t count = 0, nmeta = 0, raw = 0, flags = kPartWalked, hops = 0;
    // The next header's load is issued before this entry's record store:
    // vmcnt counts stores too, so a wait for a load issued after a store
    // would also wait for the store to complete.
    uint64_t q = pos < stop ? peek(pos) : 0ull;
    while (pos < stop) {
        if (hops++ >= budget) {
            flags |= kPartWrap;   // out of budget: the serial walker takes the segment
            break;
        }
        const Hop h = hop_of(q, pos);
        raw = meta_update(tab, raw, q, h.mbytes);
        nmeta += h.mbytes;
        if (h.next > 0xFFFFFFFFull) {
            flags |= kPartWrap;
            break;
        }
        if (h.next > w.capacity) {
            flags |= kPartOverrun;
            break;
        }
        const uint32_t next = uint32_t(h.next);
        const uint64_t qn = next < stop ? peek(next) : 0ull;
        sink(count, pos, h.len, uint32_t(q) & 0xFF);
        count++;
        pos = next;
        q = qn;
    }
    r.exit = pos;
    r.count = count;
    r.nmeta = nmeta;
    r.raw = raw;
    r.flags = flags;
}

template <class Sink>
__device__ __forceinline__ void walk_lane(const PWalk& w, const uint32_t* tab, uint64_t seg,
                                          uint64_t sb, uint32_t pos, uint32_t stop, PartRes& r,
                                          Sink&& sink, uint32_t budget)
{
    walk_lane(w, tab, pos, stop, r, sink, budget, GlobalPeek{sb, w.capacity});
}

// B's re-walks are wave-uniform (every lane chases the same chain), so the
// wave stages the segment bytes around the chain in LDS, kFixWin at a time,
// and each hop reads LDS instead of waiting a memory round trip.
#ifndef RAMCRC_FIX_WIN_KIB
#define RAMCRC_FIX_WIN_KIB 16
#endif
constexpr uint32_t kFixWin = RAMCRC_FIX_WIN_KIB * 1024;
struct WinPeek {
    uint8_t* lds;
    uint64_t sb;
    uint32_t capacity;
    uint32_t wb;   // staged [wb, wb + kFixWin); kNoStart: nothing staged
    __device__ uint64_t operator()(uint32_t p)
    {
        if (wb == kNoStart || p < wb || ((p - wb) & ~3u) + 8 > kFixWin) {
            const uint32_t b = p & ~15u;
            const uint32_t l16 = (threadIdx.x & (kWaveSize - 1)) * 16;
            u32x4 v[kFixWin / 1024];
#pragma unroll
            for (uint32_t u = 0; u < kFixWin / 1024; u++) {
                const uint64_t a = uint64_t(b) + u * 1024 + l16;
                v[u] = a + 16 <= capacity ? load16(sb + a) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (uint32_t u = 0; u < kFixWin / 1024; u++)
                *reinterpret_cast<u32x4*>(lds + u * 1024 + l16) = v[u];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            wb = b;
        }
        const uint32_t o = p - wb;
        const uint32_t* w32 = reinterpret_cast<const uint32_t*>(lds + (o & ~3u));
        return ((uint64_t(w32[1]) << 32) | w32[0]) >> (8 * (o & 3));
    }
};

struct NoSink {
    __device__ void operator()(uint32_t, uint32_t, uint32_t, uint32_t) const {}
};

// Records straight to the table (slots below the table's capacity).
struct TableSink {
    u32x4* out;
    uint64_t n;
    uint32_t seg;
    uint32_t* hard;   // nullable: ORed with the written records' replay_hard bits
    const PWalk* fast = nullptr;   // verify-in-walk mode: the records go to k_left's list
    uint64_t slot0 = 0;            // ... out's first slot in the table
    __device__ void operator()(uint32_t idx, uint32_t pos, uint32_t len, uint32_t hdr) const
    {
        if (idx < n) {
            out[idx] = u32x4{seg, pos, len, hdr};
            if (hard)
                *hard |= replay_hard(pos, len, hdr);
            if (fast)
                *hard |= left_append(*fast, slot0 + idx, len, hdr);
        }
    }
};

__device__ __forceinline__ void walk_tab_fill(uint32_t* tab)
{
    for (uint32_t t = threadIdx.x; t < 4 * 256; t += blockDim.x)
        tab[t] = g_tab.pos[1 + kTinyRow0 + t / 256][t % 256];
    __syncthreads();
}

// A: one lane per part.
// A keeps each lane's records (offset; length << 8 | header byte) in LDS
// while it chases, then the wave writes them part by part with coalesced
// stores: records stored by a lane one hop at a time would reach memory as
// partial lines.  A part with more than kPartRec records, or an entry of
// 16 MiB or more, is marked kPartSpill and walked again by C; its first
// kPartRec records still go to the scratch (B meets a misguessed chain within
// its first few entries), unless an entry's length does not fit a record.
// Records a lane keeps in LDS before writing them out: a whole block.  (Runs
// of 32 with twice the lanes in flight on 32 KiB parts measured 8-9 %
// slower on dense replay, profiles/r06/combo1/walkab: the sync search and
// fix-up work per part doubled while the part walks gained little.)
constexpr uint32_t kLRec = kPartRec;
// Lane t keeps record e of its run in slot (e + t) mod kLRec of its row: the
// rows are 512 bytes apart, so unrotated, the lanes of a wave storing their
// e-th records all hit one bank (the round-6 PMC pass counted 90 % of the
// kernel's LDS cycles as bank conflicts, profiles/r06/viw3/pmc_summary.txt;
// rotated, none -- at the same kernel time: A waits on its header loads).
__device__ __forceinline__ uint32_t lrec_slot(uint32_t e, uint32_t t)
{
    return (e + t) & (kLRec - 1);
}
__global__ __launch_bounds__(256) void k_walk_parts(PWalk w0)
{
    const PWalk w = walk_geo(w0);
    __shared__ uint32_t tab[4 * 256];
    __shared__ uint2 lrec[256][kLRec];
    walk_tab_fill(tab);
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool valid = i < w.nseg * w.nparts;
    PartRes r{};
    uint2* mine = lrec[threadIdx.x];
    bool huge = false, lost = false;
    uint32_t curk = 0;   // the pool block of the block being filled (kLRec < kPartRec)
    // a full run of kLRec of this lane's records to its place: block 0 to the
    // part's scratch, later ones to pool blocks (a lane's contiguous bytes;
    // the lines fill up in L2).  Run j holds records j kLRec ..; a pool block
    // is taken at the first run of its block.
    auto put_block = [&](uint32_t j, uint32_t n) {
        const uint32_t b = j * kLRec / kPartRec, off = (j * kLRec) % kPartRec;
        uint2* dst = nullptr;
        if (b == 0) {
            dst = w.recs + i * kPartRec + off;
        } else if (b <= kMaxBlocks && !lost) {
            if (off == 0) {
                const unsigned long long k = atomicAdd(w.pool_used, 1ull);
                curk = k < w.pool_cap ? uint32_t(k) : 0xFFFFFFFFu;
                if (curk != 0xFFFFFFFFu) {
                    w.blocks[i * kMaxBlocks + (b - 1)] = curk;
                    w.pool_owner[k] = uint32_t(i * 16 + b);
                }
            }
            if (curk != 0xFFFFFFFFu)
                dst = w.pool + uint64_t(curk) * kPartRec + off;
        }
        if (!dst) {
            lost = true;   // C walks the part again
            return;
        }
        for (uint32_t e = 0; e < n; e += 2) {
            const uint2 a0 = mine[lrec_slot(e, threadIdx.x)], a1 = mine[lrec_slot(e + 1, threadIdx.x)];
            if (e + 1 < n)
                *reinterpret_cast<uint4*>(dst + e) = make_uint4(a0.x, a0.y, a1.x, a1.y);
            else
                dst[e] = a0;
        }
    };
    if (valid) {
        const uint64_t seg = i / w.nparts;
        const uint32_t k = uint32_t(i - seg * w.nparts);
        const uint32_t B = k << w.pshift;
        const uint32_t limit = walk_limit(w, seg);
        r = w.parts[i];
        const uint32_t start = k == 0 ? 0u : r.start;
        r.start = start;
        if (start == kNoStart || B >= limit) {
            r.flags = 0;
            r.count = r.nmeta = r.raw = 0;
            r.exit = start;
        } else {
            const uint32_t pend = uint32_t(uint64_t(B) + (1ull << w.pshift) < w.capacity
                                               ? uint64_t(B) + (1ull << w.pshift) : w.capacity);
            const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
            // a part of at most kLRec records keeps them in LDS for the
            // wave's coalesced flush below; a denser part writes every full
            // run as it goes
            auto sink = [&](uint32_t idx, uint32_t pos, uint32_t len, uint32_t hdr) {
                if (idx == kLRec)
                    put_block(0, kLRec);
                mine[lrec_slot(idx, threadIdx.x)] = make_uint2(pos, (len << 8) | hdr);
                huge = huge || len >= (1u << 24);
                if (idx >= kLRec && (idx & (kLRec - 1)) == kLRec - 1)
                    put_block(idx / kLRec, kLRec);
            };
            const uint32_t stop = pend < limit ? pend : limit;
            walk_lane(w, tab, seg, sb, start, stop, r, sink, 1u << w.pshift);
            if (r.count > kLRec && (r.count & (kLRec - 1)))
                put_block(r.count / kLRec, r.count & (kLRec - 1));
            if (r.count > kPartRec * (1 + kMaxBlocks) || huge || lost)
                r.flags |= kPartSpill;
            if (huge)
                r.flags |= kPartHuge;
        }
        w.parts[i] = r;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS records
    const int lane = threadIdx.x & (kWaveSize - 1);
    const bool flush = valid && (r.flags & kPartWalked) && !(r.flags & kPartHuge) && r.count <= kLRec;
    uint64_t todo = __ballot(flush);
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t n = __shfl(r.count, j, kWaveSize);
        const uint64_t dst = (i - uint64_t(lane) + uint64_t(j)) * kPartRec;
        const uint32_t t = (threadIdx.x & ~63u) + uint32_t(j);
        const uint2* src = lrec[t];
        for (uint32_t e = uint32_t(lane); e < n; e += kWaveSize)
            w.recs[dst + e] = src[lrec_slot(e, t)];
    }
}


// B: one wave per segment, lane k deciding part k of a chunk of 64.  A part
// is accepted as A walked it when the true chain arrives at its guess, or
// meets the guessed chain within kMeetHops entries at one of its first
// kMeetMax records (a junk guess whose length lands on the true chain: the
// common misguess); the true arrival offset of part k is the exit of part
// k-1 as A walked it, so every part is checked at once.  The parts that
// fail -- a guess that never meets, a part the chain jumps over, a part left
// unwalked -- are resolved in order by the whole wave (re-walked from the
// true offset through an LDS window), each resolution re-checking the part
// after it.  The accepted parts' metadata CRCs fold into the segment's with
// one GF(2) multiply per part, then the status is written and the records
// are allocated (one atomic per segment).
__global__ __launch_bounds__(kWaveSize) void k_walk_fix(PWalk w0)
{
    const PWalk w = walk_geo(w0);
    __shared__ uint32_t tab[4 * 256];
    __shared__ __attribute__((aligned(16))) uint8_t win[kFixWin];
    walk_tab_fill(tab);
    const int lane = threadIdx.x;
    for (uint64_t seg = blockIdx.x; seg < w.nseg; seg += gridDim.x) {
        const uint32_t limit = walk_limit(w, seg);
        const ramcrc_seg_cert cert = w.certs[seg];
        const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
        WinPeek wpeek{win, sb, w.capacity, kNoStart};
        PartRes* parts = w.parts + seg * w.nparts;
        // The true chain (wave-uniform): pos, the metadata CRC so far (raw
        // state from 0xFFFFFFFF), the records before the current chunk.
        uint32_t pos = 0, crc = 0xFFFFFFFFu, count = 0, rewalk = 0;
        bool overrun = false, fallback = false;
        // Fold the accepted parts of a chunk (one per lane) into crc in one
        // step: crc <- X^n(crc) ^ sum_j X^(suffix_j)(raw_j), suffix_j = the
        // metadata bytes of the accepted parts after j, n = all of them.
        auto fold = [&](bool acc, uint32_t nmeta, uint32_t raw) {
            const uint32_t nm = acc ? nmeta : 0u;
            uint32_t incl = nm;   // inclusive suffix sum over higher lanes
#pragma unroll
            for (int s = 1; s < kWaveSize; s <<= 1) {
                const uint32_t y = __shfl_down(incl, s, kWaveSize);
                if (lane + s < kWaveSize)
                    incl += y;
            }
            const uint32_t n_all = __shfl(incl, 0, kWaveSize);
            uint32_t c = acc ? mulmod_horner(raw, xpow8_dev(incl - nm)) : 0u;
#pragma unroll
            for (int s = 1; s < kWaveSize; s <<= 1)
                c ^= __shfl_xor(c, s, kWaveSize);
            crc = mulmod_horner(crc, xpow8_dev(n_all)) ^ c;
        };
        // Where the chain arriving at pe meets part k's guessed chain: after
        // `hops` (<= kMeetHops) entries walked from pe, at the guess's record
        // `cut` (0: the guess itself, up to kMeetMax); -1 when it does not.
        // The walked entries' header + length bytes: raw CRC wr over wn bytes.
        auto meet_at = [&](uint32_t k, uint32_t st, uint32_t fl, uint32_t gc, uint32_t pe,
                           uint32_t& wr, uint32_t& wn) -> int {
            wr = wn = 0;
            const uint64_t Ek = (uint64_t(k) << w.pshift) + (1ull << w.pshift);
            if (!(fl & kPartWalked) || (fl & kPartWrap) || uint64_t(pe) >= Ek)
                return -1;
            // the scratch holds a part's first kPartRec records (none when an
            // entry's length does not fit a record): met at its start only then
            const uint32_t gn = (fl & kPartHuge) ? 0u : (gc < kPartRec ? gc : kPartRec);
            const uint64_t base = (uint64_t(seg) * w.nparts + k) * kPartRec;
            uint32_t p = pe;
            for (uint32_t hh = 0;; hh++) {
                if (p == st)
                    return int(hh << 8);
                for (uint32_t c = 1; c <= kMeetMax && c < gn; c++)
                    if (w.recs[base + c].x == p)
                        return int((hh << 8) | c);
                if (hh == kMeetHops || p >= limit || uint64_t(p) >= Ek)
                    return -1;
                const uint64_t q = seg_peek(sb, p, w.capacity);
                const Hop h = hop_of(q, p);
                if (h.next > w.capacity)
                    return -1;
                wr = meta_update(tab, wr, q, h.mbytes);
                wn += h.mbytes;
                p = uint32_t(h.next);
            }
        };
        const uint32_t nlive =
            limit == 0 ? 0u : uint32_t((uint64_t(limit) + (1ull << w.pshift) - 1) >> w.pshift);
        for (uint32_t k0 = 0; k0 < nlive && !overrun && !fallback; k0 += kWaveSize) {
            const uint32_t k = k0 + uint32_t(lane);
            const bool in = k < nlive;
            PartRes r{};
            if (in)
                r = parts[k];
            const uint32_t gst = r.start;   // A's guess
            // per lane: ok (decided), emit (accepted: walked or met), the
            // meet to apply (mt >= 0; kResolved: totals already final), and
            // the exit handed to the next part
            constexpr int kResolved = -2;
            uint32_t ex = r.exit, wr = 0, wn = 0;
            int mt = -1;
            {
                uint32_t pe = __shfl_up(ex, 1, kWaveSize);
                pe = lane == 0 ? pos : pe;
                if (in)
                    mt = meet_at(k, gst, r.flags, r.count, pe, wr, wn);
                if (mt > 0)
                    r.start = pe;
            }
            bool ok = !in || mt >= 0, emit = in && mt >= 0;
            while (true) {
                // the first undecided part; every part before it is decided
                const uint64_t bad = __ballot(!ok);
                if (!bad)
                    break;
                const int j = int(__builtin_ctzll(bad));
                // an accepted part below it that overran ends the chain
                const uint64_t ovr = __ballot(emit && (r.flags & kPartOverrun));
                if (ovr && int(__builtin_ctzll(ovr)) < j)
                    break;
                const uint32_t kj = k0 + uint32_t(j);
                const uint32_t pe = j == 0 ? pos : uint32_t(__builtin_amdgcn_readlane(int(ex), j - 1));
                const uint32_t st = uint32_t(__builtin_amdgcn_readlane(int(gst), j));
                const uint32_t fl = uint32_t(__builtin_amdgcn_readlane(int(r.flags), j));
                const uint64_t Ej64 = (uint64_t(kj) << w.pshift) + (1ull << w.pshift);
                const uint32_t Ej = uint32_t(Ej64 < w.capacity ? Ej64 : w.capacity);
                const uint32_t stop = Ej < limit ? Ej : limit;
                const uint32_t budget = rewalk < kRewalkBudget ? kRewalkBudget - rewalk : 0u;
                bool jemit = true;
                uint32_t jex = pe;
                if (uint64_t(pe) >= Ej64) {
                    jemit = false;   // the chain jumps over this part
                } else if (fl & kPartWalked) {
                    // Walk from pe until the chain meets the guessed one at any
                    // of the offsets A recorded for it (lane e holds its e-th
                    // entry; the first is the guess); its entries from there on
                    // are the true chain's.  Without a meeting the walk covers
                    // the part (a full re-walk).
                    const uint32_t gc = uint32_t(__builtin_amdgcn_readlane(int(r.count), j));
                    const uint32_t gn = (fl & kPartHuge) ? 0u : (gc < kPartRec ? gc : kPartRec);
                    const uint64_t pidx = uint64_t(seg) * w.nparts + kj;
                    uint2 g = make_uint2(0xFFFFFFFFu, 0u);
                    if (uint32_t(lane) < gn)
                        g = w.recs[pidx * kPartRec + uint32_t(lane)];
                    uint32_t p = pe, wc = 0, wnn = 0, wrr = 0, wflags = kPartWalked;
                    int cut = -1;
                    // the walk's records and header + length bytes, 64 at a time:
                    // record wc in lane wc % 64; each full block's metadata CRC is
                    // summed in parallel off the chase, and blocks 1.. go to pool
                    // blocks (unattached until the walk proves to be a re-walk)
                    uint2 mine = make_uint2(0u, 0u), mine0 = make_uint2(0u, 0u);
                    uint64_t mq = 0;
                    uint32_t myblk = 0xFFFFFFFFu;   // lane b: pool block of block b
                    bool huge = false, pool_ok = true;
                    auto fold_block = [&](uint32_t n) {   // lanes < n hold metadata
                        const bool inr = uint32_t(lane) < n;
                        const uint32_t mb = inr ? uint32_t((mq >> 6) & 3) + 2 : 0u;
                        const uint32_t re = inr ? meta_update(tab, 0u, mq, mb) : 0u;
                        uint32_t incl = mb;
#pragma unroll
                        for (int s2 = 1; s2 < kWaveSize; s2 <<= 1) {
                            const uint32_t y = __shfl_down(incl, s2, kWaveSize);
                            if (lane + s2 < kWaveSize)
                                incl += y;
                        }
                        const uint32_t hn = __shfl(incl, 0, kWaveSize);
                        uint32_t hr = inr ? mulmod_horner(re, xpow8_dev(incl - mb)) : 0u;
#pragma unroll
                        for (int s2 = 1; s2 < kWaveSize; s2 <<= 1)
                            hr ^= __shfl_xor(hr, s2, kWaveSize);
                        // raw(0, A||B) = X^|B|(raw(0, A)) ^ raw(0, B)
                        wrr = mulmod_horner(wrr, xpow8_dev(hn)) ^ hr;
                        wnn += hn;
                    };
                    auto store_block = [&](uint32_t b, uint32_t n) {   // lanes < n hold records
                        if (b == 0) {
                            mine0 = mine;
                            return;
                        }
                        if (!pool_ok || b > kMaxBlocks) {
                            pool_ok = false;
                            return;
                        }
                        unsigned long long k = 0;
                        if (lane == 0)
                            k = atomicAdd(w.pool_used, 1ull);
                        k = __shfl(k, 0, kWaveSize);
                        if (k >= w.pool_cap) {
                            pool_ok = false;
                            return;
                        }
                        if (uint32_t(lane) < n)
                            w.pool[k * kPartRec + uint32_t(lane)] = mine;
                        if (lane == 0)
                            w.pool_owner[k] = 0xFFFFFFFFu;   // unattached
                        if (uint32_t(lane) == b)
                            myblk = uint32_t(k);
                    };
                    while (true) {
                        const uint64_t hit = __ballot(uint32_t(lane) < gn && g.x == p);
                        if (hit || (!(fl & kPartWrap) && p == st)) {
                            cut = hit ? int(__builtin_ctzll(hit)) : 0;
                            break;
                        }
                        if (p >= stop)
                            break;
                        if (wc >= budget) {
                            wflags |= kPartWrap;   // out of budget: the serial walker
                            break;
                        }
                        const uint64_t q = wpeek(p);
                        const Hop h = hop_of(q, p);
                        if (uint32_t(lane) == (wc & (kWaveSize - 1)))
                            mq = q;
                        if (h.next > 0xFFFFFFFFull) {
                            wflags |= kPartWrap;
                            break;
                        }
                        if (h.next > w.capacity) {
                            wflags |= kPartOverrun;
                            break;
                        }
                        if (uint32_t(lane) == (wc & (kWaveSize - 1)))
                            mine = make_uint2(p, (h.len << 8) | (uint32_t(q) & 0xFF));
                        huge = huge || h.len >= (1u << 24);
                        wc++;
                        p = uint32_t(h.next);
                        if ((wc & (kWaveSize - 1)) == 0) {
                            fold_block(kWaveSize);
                            store_block(wc / kWaveSize - 1, kWaveSize);
                        }
                    }
                    rewalk += wc + 1;
                    {
                        // the last partial block's header + length bytes (with an
                        // entry that overran or wrapped: the reference checksums its
                        // header too)
                        const uint32_t rem = (wc & (kWaveSize - 1)) +
                                             ((wflags & (kPartWrap | kPartOverrun)) ? 1u : 0u);
                        if (rem)
                            fold_block(rem);
                    }
                    if (cut >= 0 && (fl & kPartWrap)) {
                        wflags |= kPartWrap;   // met a chain that wraps: the serial walker
                    } else if (cut >= 0) {
                        // the guess's totals minus its first `cut` entries, whose
                        // header + length bytes are folded from the records:
                        // raw(0, A||S) = X^|S|(raw(0, A)) ^ raw(0, S)
                        const bool inp = lane < cut;
                        const uint32_t mb = inp ? ((g.y >> 6) & 3) + 2 : 0u;
                        const uint64_t qe = uint64_t(g.y & 0xFF) | (uint64_t(g.y >> 8) << 8);
                        const uint32_t re = inp ? meta_update(tab, 0u, qe, mb) : 0u;
                        uint32_t incl = mb;   // suffix sums of the prefix's bytes
#pragma unroll
                        for (int s = 1; s < kWaveSize; s <<= 1) {
                            const uint32_t y = __shfl_down(incl, s, kWaveSize);
                            if (lane + s < kWaveSize)
                                incl += y;
                        }
                        const uint32_t pn = __shfl(incl, 0, kWaveSize);
                        uint32_t pr = inp ? mulmod_horner(re, xpow8_dev(incl - mb)) : 0u;
#pragma unroll
                        for (int s = 1; s < kWaveSize; s <<= 1)
                            pr ^= __shfl_xor(pr, s, kWaveSize);
                        const uint32_t tn = uint32_t(__builtin_amdgcn_readlane(int(r.nmeta), j));
                        const uint32_t tr = uint32_t(__builtin_amdgcn_readlane(int(r.raw), j));
                        const uint32_t sn = tn - pn;   // suffix metadata bytes
                        const uint32_t sr = tr ^ mulmod_horner(pr, xpow8_dev(sn));
                        jex = uint32_t(__builtin_amdgcn_readlane(int(r.exit), j));
                        const uint32_t nn = wnn + sn;
                        const uint32_t rr = mulmod_horner(wrr, xpow8_dev(sn)) ^ sr;
                        if (lane == j) {
                            r.start = pe;
                            r.count = wc + gc - uint32_t(cut);
                            r.nmeta = nn;
                            r.raw = rr;
                            r.pre = wc;
                            r.cut = uint32_t(cut);
                            mt = kResolved;
                        }
                    } else {
                        // walked the whole part: its records go to the scratch and
                        // pool blocks (C copies them), or, when they do not fit, C
                        // walks it again
                        jex = p;
                        if (wc > kPartRec && (wc & (kPartRec - 1)))
                            store_block(wc / kPartRec, wc & (kPartRec - 1));
                        const bool keep = !huge && pool_ok && wc <= kPartRec * (1 + kMaxBlocks);
                        if (keep) {
                            const uint2 first = wc <= kPartRec ? mine : mine0;
                            if (uint32_t(lane) < (wc < kPartRec ? wc : kPartRec))
                                w.recs[pidx * kPartRec + uint32_t(lane)] = first;
                            // replace A's blocks of this part by the walk's
                            const uint32_t nb = (wc + kPartRec - 1) / kPartRec;   // blocks incl. 0
                            if (lane >= 1 && uint32_t(lane) <= kMaxBlocks) {
                                const uint32_t own = uint32_t(pidx * 16 + uint32_t(lane));
                                const uint32_t old = w.blocks[pidx * kMaxBlocks + uint32_t(lane) - 1];
                                if (old < w.pool_cap && w.pool_owner[old] == own)
                                    w.pool_owner[old] = 0xFFFFFFFFu;
                                if (uint32_t(lane) < nb) {
                                    w.blocks[pidx * kMaxBlocks + uint32_t(lane) - 1] = myblk;
                                    w.pool_owner[myblk] = own;
                                }
                            }
                        }
                        if (lane == j) {
                            r.start = pe;
                            r.exit = p;
                            r.count = wc;
                            r.nmeta = wnn;
                            r.raw = wrr;
                            r.flags = keep ? wflags : (wflags | kPartChase);
                            r.pre = r.cut = 0;
                            mt = kResolved;
                        }
                    }
                    if (wflags & kPartWrap)
                        fallback = true;
                } else {
                    // no guess: walk this part from the true offset, its
                    // records to the scratch as above
                    PartRes x;
                    uint2 mine = make_uint2(0u, 0u);
                    bool huge = false;
                    walk_lane(w, tab, pe, stop, x,
                              [&](uint32_t idx, uint32_t rp, uint32_t len, uint32_t hdr) {
                                  if (uint32_t(lane) == idx)
                                      mine = make_uint2(rp, (len << 8) | hdr);
                                  huge = huge || len >= (1u << 24);
                              },
                              budget, wpeek);
                    rewalk += x.count + 1;
                    jex = x.exit;
                    const bool keep = x.count <= kPartRec && !huge;
                    if (keep && uint32_t(lane) < x.count)
                        w.recs[(uint64_t(seg) * w.nparts + kj) * kPartRec + uint32_t(lane)] = mine;
                    if (lane == j) {
                        r.start = pe;
                        r.exit = x.exit;
                        r.count = x.count;
                        r.nmeta = x.nmeta;
                        r.raw = x.raw;
                        r.flags = keep ? x.flags : (x.flags | kPartChase);
                        r.pre = r.cut = 0;
                        mt = kResolved;
                    }
                    if (x.flags & kPartWrap)
                        fallback = true;
                }
                if (fallback)
                    break;
                if (lane == j) {
                    ok = true;
                    emit = jemit;
                    ex = jex;
                    mt = kResolved;
                }
                // the part after j: its arrival offset is now known
                if (lane == j + 1 && in) {
                    mt = meet_at(k, gst, r.flags, r.count, jex, wr, wn);
                    r.start = mt > 0 ? jex : gst;
                    ok = mt >= 0;
                    emit = ok;
                }
            }
            if (fallback)
                break;
            // the chain ends at the first accepted part that overran
            const uint64_t ovr = __ballot(emit && (r.flags & kPartOverrun));
            const int olane = ovr ? int(__builtin_ctzll(ovr)) : kWaveSize;
            if (lane > olane)
                emit = false;
            if (emit && mt > 0) {
                // drop the guess's first `cut` entries (junk), whose header +
                // length bytes are rebuilt from the records, and put the
                // `hops` entries walked from the arrival offset in front
                const uint32_t hops = uint32_t(mt) >> 8, cut = uint32_t(mt) & 0xFF;
                const uint64_t base = (uint64_t(seg) * w.nparts + k) * kPartRec;
                uint32_t jr = 0, jn = 0;
                for (uint32_t e = 0; e < cut; e++) {
                    const uint2 g = w.recs[base + e];
                    const uint32_t mb = ((g.y >> 6) & 3) + 2;
                    const uint64_t qe = uint64_t(g.y & 0xFF) | (uint64_t(g.y >> 8) << 8);
                    jr = meta_update(tab, jr, qe, mb);
                    jn += mb;
                }
                const uint32_t tn = r.nmeta - jn;
                const uint32_t tr = r.raw ^ mulmod_horner(jr, xpow8_dev(tn));
                r.raw = mulmod_horner(wr, xpow8_dev(tn)) ^ tr;
                r.nmeta = wn + tn;
                r.count = hops + r.count - cut;
                r.pre = hops;   // walked again (and emitted) by C
                r.cut = cut;
            } else if (emit && mt == 0) {
                r.pre = r.cut = 0;   // accepted as walked
            }
            const uint32_t c = emit ? r.count : 0u;
            uint32_t incl = c;   // inclusive prefix of the record counts
#pragma unroll
            for (int s = 1; s < kWaveSize; s <<= 1) {
                const uint32_t y = __shfl_up(incl, s, kWaveSize);
                if (lane >= s)
                    incl += y;
            }
            fold(emit, r.nmeta, r.raw);
            if (emit) {
                r.rec = count + incl - c;
                r.flags |= kPartEmit;
                parts[k] = r;
            }
            count += uint32_t(__builtin_amdgcn_readlane(int(incl), kWaveSize - 1));
            // the chain's position after the chunk: the overrun part's exit,
            // else the last live part's
            const int last = olane < kWaveSize ? olane
                                               : int(nlive - 1 - k0 < uint32_t(kWaveSize - 1)
                                                         ? nlive - 1 - k0 : uint32_t(kWaveSize - 1));
            pos = uint32_t(__builtin_amdgcn_readlane(int(ex), last));
            overrun = olane < kWaveSize;
        }
        if (fallback) {
            if (lane == 0)
                w.fallback[seg] = 1;
            continue;
        }
        uint32_t flags = 0;
        const uint32_t fin = ~crc_small(tab, crc, cert.segment_length, 4);
        if (overrun)
            flags |= RAMCRC_SEG_PAST_CAPACITY;
        else if (pos > cert.segment_length)
            flags |= RAMCRC_SEG_PAST_LENGTH;
        else if (fin != cert.checksum)
            flags |= RAMCRC_SEG_BAD_CHECKSUM;
        unsigned long long b = 0;
        if (lane == 0 && count)
            b = atomicAdd(w.n_entries, (unsigned long long)count);
        b = __shfl(b, 0, kWaveSize);
        if (b + count > w.cap)
            flags |= RAMCRC_SEG_TABLE_FULL;
        if (!(flags & (RAMCRC_SEG_PAST_CAPACITY | RAMCRC_SEG_PAST_LENGTH | RAMCRC_SEG_BAD_CHECKSUM |
                       RAMCRC_SEG_TABLE_FULL)))
            flags |= RAMCRC_SEG_OK;   // records dropped (TABLE_FULL): not verified, never OK
        if (lane == 0) {
            w.fallback[seg] = 0;
            w.seg_base[seg] = b;
            ramcrc_seg_status st;
            st.flags = flags;
            st.checksum = fin;
            st.entries = count;
            st.bad_objects = 0;
            w.status[seg] = st;
        }
    }
}

// C: the records of every accepted part at their final slots.  A part
// accepted as walked (the common case) already has its records in the
// scratch A wrote: the wave copies them, part after part, 64 records per
// instruction.  Entries walked by k_walk_fix before it met the guessed chain
// are walked once more here; parts walked again in full, or with more
// records than the scratch holds, are walked again here in full.
__global__ __launch_bounds__(256) void k_walk_emit(PWalk w0)
{
    const PWalk w = walk_geo(w0);
    __shared__ uint32_t tab[4 * 256];
    walk_tab_fill(tab);
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool valid = i < w.nseg * w.nparts;
    const uint64_t seg = valid ? i / w.nparts : 0;
    PartRes r{};
    bool emit = false;
    uint64_t slot = 0;
    if (valid) {
        r = w.parts[i];
        emit = (r.flags & kPartEmit) && !w.fallback[seg];
        if (emit)
            slot = w.seg_base[seg] + r.rec;
    }
    const bool chase = emit && (r.flags & (kPartChase | kPartSpill));
    const uint32_t pre = emit && !chase ? r.pre : 0u;
    uint32_t hard = 0;
    if (chase || pre) {
        const uint32_t k = uint32_t(i - seg * w.nparts);
        const uint32_t B = k << w.pshift;
        const uint32_t limit = walk_limit(w, seg);
        const uint32_t pend = uint32_t(uint64_t(B) + (1ull << w.pshift) < w.capacity ? uint64_t(B) + (1ull << w.pshift)
                                                                             : w.capacity);
        const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
        PartRes x;
        const bool fast = w.sum && (walk_sum_seen(w.sum) & kSumFast);
        walk_lane(w, tab, seg, sb, r.start, pend < limit ? pend : limit, x,
                  TableSink{w.entries + slot, slot < w.cap ? w.cap - slot : 0, uint32_t(seg),
                            w.sum ? &hard : nullptr, fast ? &w : nullptr, slot},
                  chase ? (1u << w.pshift) : pre);
    }
    if (w.sum) {
        const uint32_t hw = (__ballot(hard & 1u) ? 1u : 0u) | (__ballot(hard & 2u) ? 2u : 0u) |
                           (__ballot(hard & 4u) ? 4u : 0u) | (__ballot(hard & kHardFull) ? kHardFull : 0u);
        if (hw && (threadIdx.x & (kWaveSize - 1)) == 0 && (hw & ~walk_sum_seen(w.sum)))
            atomicOr(w.sum, hw);
    }
}

// C': the scratch records of the parts accepted without a second walk.  One
// wave per block of kPartRec (= 64) records -- a part's first block in the
// scratch, then the pool blocks in use -- lane j copying record j.  The copy
// is a chain of dependent loads (block owner and records, the part's result,
// the segment's base), so a wave takes kCopyU blocks at a time and issues
// each level's loads for all of them together.
static_assert(kPartRec == kWaveSize, "k_walk_copy: one lane per record of a block");

#ifndef RAMCRC_COPY_U
#define RAMCRC_COPY_U 4
#endif
constexpr int kCopyU = RAMCRC_COPY_U;
__global__ __launch_bounds__(256) void k_walk_copy(PWalk w0)
{
    const PWalk w = walk_geo(w0);
    const uint64_t nfirst = w.nseg * w.nparts;
    const uint64_t used = *w.pool_used;
    const uint64_t nblk = nfirst + (used < w.pool_cap ? used : w.pool_cap);
    const uint64_t nwave = uint64_t(gridDim.x) * (blockDim.x / kWaveSize);
    const uint32_t lane = threadIdx.x & (kWaveSize - 1);
    // the fused replay's summary (w.sum) over every record copied; the
    // records C walks again set it in k_walk_emit.  (Taking it in A and the
    // fix-up instead -- the last hard index per part, counted from each
    // accepted part's cut -- measured 1 % slower: profiles/r05/replayfix.)
    const uint32_t seen = walk_sum_seen(w.sum);
    if (w.sum && (seen & kSumFast))
        return;   // k_walk_copyv copies and verifies (uniform)
    uint32_t hard = 0;
    for (uint64_t b0 = (uint64_t(blockIdx.x) * (blockDim.x / kWaveSize) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize)) * kCopyU;
         b0 < nblk; b0 += nwave * kCopyU) {
        uint64_t part[kCopyU];
        uint32_t blk[kCopyU];   // block number within the part; ~0u: nothing to copy
        uint2 v[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint64_t bi = b0 + u;
            blk[u] = ~0u;
            part[u] = 0;
            if (bi < nfirst) {
                part[u] = bi;
                blk[u] = 0;
                v[u] = w.recs[bi * kPartRec + lane];
            } else if (bi < nblk) {
                const uint32_t own = w.pool_owner[bi - nfirst];
                v[u] = w.pool[(bi - nfirst) * kPartRec + lane];
                if (own != 0xFFFFFFFFu) {   // else a block the fix-up wrote for a walk that met the guess
                    part[u] = own / 16;
                    blk[u] = own % 16;
                }
            }
        }
        PartRes r[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; u++)
            if (blk[u] != ~0u)
                r[u] = w.parts[part[u]];
        uint32_t fb[kCopyU];
        uint64_t sbase[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint32_t fl = r[u].flags;
            if (blk[u] != ~0u && (!(fl & kPartEmit) || (fl & (kPartChase | kPartSpill))))
                blk[u] = ~0u;
            if (blk[u] != ~0u) {
                const uint64_t seg = part[u] / w.nparts;
                fb[u] = w.fallback[seg];
                sbase[u] = w.seg_base[seg];
            }
        }
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            if (blk[u] == ~0u || fb[u])
                continue;
            const uint32_t n = r[u].count - r[u].pre;   // records ri = cut .. cut + n - 1
            const uint32_t ri = blk[u] * kPartRec + lane;
            if (ri < r[u].cut || ri - r[u].cut >= n)
                continue;
            const uint64_t dst = sbase[u] + r[u].rec + r[u].pre + (ri - r[u].cut);
            if (dst < w.cap) {
                const u32x4 rec = {uint32_t(part[u] / w.nparts), v[u].x, v[u].y >> 8, v[u].y & 0xFF};
                // streamed: not read back by this kernel (replay 64 B +1.7 %
                // over plain stores).  (The same for the part walk's scratch
                // stores was 8 % slower: k_walk_copy reads that scratch back
                // while it is still in the caches.)
                __builtin_nontemporal_store(rec, &w.entries[dst]);
                hard |= (seen & kHardAll) != kHardAll ? replay_hard(v[u].x, v[u].y >> 8, v[u].y & 0xFF) : 0u;
            }
        }
    }
    {
        const uint32_t hw = (__ballot(hard & 1u) ? 1u : 0u) | (__ballot(hard & 2u) ? 2u : 0u) |
                           (__ballot(hard & 4u) ? 4u : 0u);
        if ((hw & ~seen) && lane == 0)
            atomicOr(w.sum, hw);
    }
}


// C'' (verify-in-walk mode, kSumFast): k_walk_copy's record copy plus the
// replay check of every small object it copies.  One wave per part (parts
// accepted as A walked them), its records in blocks of 64, lane j taking
// record j of a block: the records are consecutive entries, so a block's
// objects lie back to back in the segment.  The wave stages the bytes a
// block spans (up to kVStage) in LDS with coalesced 16-byte loads and each
// lane runs the CRC of its object's bytes [4, len) over LDS -- a dword per
// step through the X^4 byte tables, the unaligned ends bytewise -- compares
// it with the stored checksum (the object's first 4 bytes,
// src/ObjectManager.cc:659-669), writes it to obj_crc and counts a mismatch
// in its segment's bad_objects, exactly as k_entries + k_obj_compare would.
// Software-pipelined over a part's blocks: block b+1's bytes and block b+2's
// records are in flight while block b is checksummed.  Objects that do not
// fit the stage, and records of other replayed types, go to k_left's list.
constexpr int kVWaves = 4;   // waves per workgroup
// Stage sizes: two instantiations, the probe picks one per batch (kSumStage8):
// 8 KiB holds a block of entries up to kFastMean8 bytes and lets four
// workgroups share a CU (16 waves), 12 KiB holds entries up to kFastMean
// (three workgroups).  A block spanning more than the stage sends its objects
// past it to k_left.
constexpr uint32_t kVStageS = 8192, kVStageL = 12288;

// raw CRC -> finalized Object::computeChecksum over LDS bytes [o, o + n): a
// dword per step through the X^4 byte tables (tx4: table k at 256 k), the
// unaligned ends through X^1 (tx1)
__device__ __forceinline__ uint32_t crc_lds(const uint8_t* st, const uint32_t* tx4, const uint32_t* tx1,
                                            uint32_t o, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    while (n && (o & 3)) {
        c = tx1[(c ^ st[o]) & 0xFF] ^ (c >> 8);
        o++;
        n--;
    }
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(st);
    auto step4 = [&](uint32_t v) {
        v ^= c;
        c = xor3(tx4[v & 0xFF], tx4[256 + ((v >> 8) & 0xFF)], tx4[512 + ((v >> 16) & 0xFF)]) ^
            tx4[768 + (v >> 24)];
    };
    for (; n >= 16; o += 16, n -= 16) {   // the data loads do not wait for c
        const uint32_t a = s32[o >> 2], b = s32[(o >> 2) + 1], e = s32[(o >> 2) + 2], f = s32[(o >> 2) + 3];
        step4(a);
        step4(b);
        step4(e);
        step4(f);
    }
    for (; n >= 4; o += 4, n -= 4)
        step4(s32[o >> 2]);
    while (n) {
        c = tx1[(c ^ st[o]) & 0xFF] ^ (c >> 8);
        o++;
        n--;
    }
    return ~c;
}

// Measured and dropped (round 6, profiles/r06/combo1, combo2, combo4): the
// byte tables in 8 copies so that a half-wave's lookups fall on fewer banks
// (one 8-wave workgroup per CU: 5-7 % slower); eight nibble tables in 32
// copies, conflict-free at twice the lookups (three workgroups per CU: 13 %
// slower); the X^4 step as a GF(2) bit-matrix on the VALU -- 64 v_bfe /
// v_bitop3 per dword, no LDS lookups, alone or for half of each object --
// 25-31 % slower.  44 % of the LDS
// cycles of the table form are bank conflicts, but the LDS is busy only
// 56 % of the kernel.

template <uint32_t kVStage>
__global__ __launch_bounds__(kVWaves * kWaveSize) void k_walk_copyv(PWalk w0)
{
    constexpr uint32_t kVLoads = kVStage / 1024;   // 16-byte loads per lane per block
    const PWalk w = walk_geo(w0);
    const uint32_t seen = walk_sum_seen(w.sum);
    if (!w.sum || !(seen & kSumFast))
        return;   // not verify-in-walk mode: k_walk_copy ran (uniform)
    if (bool(seen & kSumStage8) != (kVStage == kVStageS))
        return;   // the other stage size's batch (uniform)
    __shared__ uint32_t tx4[4 * 256];   // X^4: the dword step
    __shared__ uint32_t tx1[256];       // X^1: the byte step
    __shared__ __attribute__((aligned(16))) uint8_t stage[kVWaves][kVStage];
    for (uint32_t t = threadIdx.x; t < 4 * 256; t += blockDim.x)
        tx4[t] = g_tab.comb[0].t[t >> 8][t & 0xFF];
    for (uint32_t t = threadIdx.x; t < 256; t += blockDim.x)
        tx1[t] = g_tab.t0.t[t];
    __syncthreads();
    const uint32_t lane = threadIdx.x & (kWaveSize - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
    const uint64_t nwave = uint64_t(gridDim.x) * kVWaves;
    const uint64_t nall = w.nseg * w.nparts;
    uint8_t* st = stage[wv];
    uint32_t hard = 0;
    for (uint64_t p = uint64_t(blockIdx.x) * kVWaves + wv; p < nall; p += nwave) {
        const PartRes r = w.parts[p];
        if (!(r.flags & kPartEmit) || (r.flags & (kPartChase | kPartSpill)))
            continue;   // not accepted, or walked again by k_walk_emit (uniform)
        const uint64_t seg = p / w.nparts;
        if (w.fallback[seg])
            continue;   // the serial walker's segment
        const uint32_t n = r.count - r.pre;   // A's records cut .. cut + n - 1
        if (n == 0)
            continue;
        const uint64_t sbase = w.seg_base[seg] + r.rec + r.pre;   // slot of record cut
        const uint32_t sflags = w.status[seg].flags;
        const uint64_t sb = reinterpret_cast<uint64_t>(w.base) + seg * w.stride;
        const uint32_t b0 = r.cut / kPartRec, b1 = (r.cut + n - 1) / kPartRec;
        // lane j < kMaxBlocks: the pool block holding the part's block j + 1
        const uint32_t bidx = b1 > 0 && lane < kMaxBlocks ? w.blocks[p * kMaxBlocks + lane] : 0u;
        auto recs_of = [&](uint32_t b) -> uint2 {
            if (b > b1)
                return make_uint2(0u, 0u);
            if (b == 0)
                return w.recs[p * kPartRec + lane];
            const uint32_t k = uint32_t(__shfl(int(bidx), int(b - 1), kWaveSize));
            return w.pool[uint64_t(k) * kPartRec + lane];
        };
        // block b's lane: its record, whether its object is checked here, the
        // object's payload offset in the segment, the slot
        struct Lane {
            u32x4 rec;
            uint64_t dst;
            uint32_t pl;
            bool valid, todo;
        };
        auto lane_of = [&](uint32_t b, uint2 v) -> Lane {
            Lane L;
            const uint32_t ri = b * kPartRec + lane;
            L.rec = u32x4{uint32_t(seg), v.x, v.y >> 8, v.y & 0xFF};
            L.dst = sbase + (ri - r.cut);
            L.valid = b <= b1 && ri >= r.cut && ri - r.cut < n && L.dst < w.cap;
            L.todo = L.valid && !replay_other(L.rec) && (L.rec.w & 0x3f) == RAMCRC_LOG_ENTRY_TYPE_OBJ &&
                     L.rec.z >= kObjHeaderBytes && !(L.rec.w & kRecOverlong) && (sflags & RAMCRC_SEG_OK);
            L.pl = L.rec.y + 1 + ((L.rec.w >> 6) & 3) + 1;
            return L;
        };
        // the staged window of a block: from its first object, 16-byte
        // aligned, to its last object's end (at most kVStage); loads of 1 KiB
        // units past that end are not issued
        auto base_of = [&](const Lane& L, uint32_t& units) -> uint32_t {
            uint32_t lo = L.todo ? L.pl : 0xFFFFFFFFu, hi = L.todo ? L.pl + L.rec.z : 0u;
#pragma unroll
            for (int s2 = 1; s2 < kWaveSize; s2 <<= 1) {
                lo = min(lo, uint32_t(__shfl_xor(int(lo), s2, kWaveSize)));
                hi = max(hi, uint32_t(__shfl_xor(int(hi), s2, kWaveSize)));
            }
            const uint32_t base = lo & ~15u;   // 0xFFFFFFF0: nothing to check in this block
            units = hi > base ? min((hi - base + 1023) / 1024, kVLoads) : 0u;
            return base;
        };
        auto issue = [&](uint32_t base, uint32_t units, u32x4 (&t)[kVLoads]) {
#pragma unroll
            for (uint32_t u = 0; u < kVLoads; u++) {
                const uint64_t a = uint64_t(base) + u * 1024 + lane * 16;
                if (u < units)   // uniform
                    t[u] = a + 16 <= w.capacity ? load16(sb + a) : u32x4{0u, 0u, 0u, 0u};
            }
        };
        Lane cur = lane_of(b0, recs_of(b0));
        uint2 vn = recs_of(b0 + 1);
        uint32_t units = 0;
        uint32_t base = base_of(cur, units);
        u32x4 t[kVLoads];
        issue(base, units, t);
        for (uint32_t b = b0; b <= b1; b++) {
#pragma unroll
            for (uint32_t u = 0; u < kVLoads; u++)
                if (u < units)
                    *reinterpret_cast<u32x4*>(st + u * 1024 + lane * 16) = t[u];
            // the next block's bytes and the one after's records in flight
            const Lane nxt = lane_of(b + 1, vn);
            uint32_t nunits = 0;
            const uint32_t nbase = base_of(nxt, nunits);
            if (b + 1 <= b1)
                issue(nbase, nunits, t);
            vn = recs_of(b + 2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (cur.valid) {
                __builtin_nontemporal_store(cur.rec, &w.entries[cur.dst]);
                hard |= (seen & kHardAll) != kHardAll ? replay_hard(cur.rec.y, cur.rec.z, cur.rec.w) : 0u;
                if (replay_other(cur.rec))
                    hard |= left_append(w, cur.dst, cur.rec.z, cur.rec.w);
            }
            if (cur.todo) {
                if (uint64_t(cur.pl) + cur.rec.z <= uint64_t(base) + kVStage) {
                    const uint32_t o = cur.pl - base;
                    const uint32_t crc = crc_lds(st, tx4, tx1, o + 4, cur.rec.z - 4);
                    const uint32_t stored = uint32_t(st[o]) | (uint32_t(st[o + 1]) << 8) |
                                            (uint32_t(st[o + 2]) << 16) | (uint32_t(st[o + 3]) << 24);
                    w.obj_crc[cur.dst] = crc;
                    if (crc != stored)
                        atomicAdd(&w.status[seg].bad_objects, 1u);
                } else {
                    // past this block's window: one thread in k_left
                    hard |= left_append(w, cur.dst, cur.rec.z, cur.rec.w);
                }
            }
            cur = nxt;
            base = nbase;
            units = nunits;
            // (the next iteration's LDS writes follow these reads: in-order
            // LDS within the wave)
        }
    }
    const uint32_t hw = (__ballot(hard & 1u) ? 1u : 0u) | (__ballot(hard & 2u) ? 2u : 0u) |
                       (__ballot(hard & 4u) ? 4u : 0u) | (__ballot(hard & kHardFull) ? kHardFull : 0u);
    if ((hw & ~seen) && lane == 0)
        atomicOr(w.sum, hw);
}

}  // namespace
