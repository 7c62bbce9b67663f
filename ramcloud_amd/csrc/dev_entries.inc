// k_entries: the tiny, multi-window and long phases of the small-entry scan.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {


// Mask and init-inject the 16 bytes of lane piece `a` of entry [S, E): one
// 64-bit clamp per piece, then 32-bit arithmetic per word.
__device__ __forceinline__ int clamp32(int64_t x)
{
    return x < -32 ? -32 : (x > 32 ? 32 : int(x));
}

__device__ __forceinline__ uint32_t fix_word32(uint32_t w, int ds, int de, uint32_t init)
{
    const int lo = min(max(ds, 0), 4), hi = min(max(de, 0), 4);
    const uint32_t mhi = uint32_t((1ull << (8 * hi)) - 1);
    const uint32_t mlo = uint32_t((1ull << (8 * lo)) - 1);
    w &= mhi & ~mlo;
    const int dd = -ds;   // word address - S
    const uint32_t inj =
        uint32_t((uint64_t(init) << 24) >> (24 + 8 * min(max(dd, -3), 3)));
    return w ^ ((dd > -4 && dd < 4) ? inj : 0u);
}

__device__ __forceinline__ u32x4 fix_piece(u32x4 w, uint64_t a, uint64_t S, uint64_t E,
                                           uint32_t init)
{
    const int ds = clamp32(int64_t(S - a)), de = clamp32(int64_t(E - a));
    w.x = fix_word32(w.x, ds, de, init);
    w.y = fix_word32(w.y, ds - 4, de - 4, init);
    w.z = fix_word32(w.z, ds - 8, de - 8, init);
    w.w = fix_word32(w.w, ds - 12, de - 12, init);
    return w;
}

// Lane piece -> window end: fold the four word slots with X^4, then the
// group's eight lanes with X^16, X^32, X^64 (a shuffle butterfly).  Every lane
// of the group returns the entry's raw state relative to the end of its last
// 128-byte window; the caller removes the zero padding with x^(-8 pad).
__device__ __forceinline__ uint32_t group_fold(const uint8_t* lds, int gl, uint32_t u0,
                                               uint32_t u1, uint32_t u2, uint32_t u3)
{
    // X^12(u0) ^ X^8(u1) ^ X^4(u2) ^ u3 as a two-level tree (the two X^4
    // lookups are independent); the piece's final X^4 is left to the unpad
    // constant (xinv4), so the fold is three dependent lookups deep, not four.
    const uint32_t a = plain_apply(lds, kX4Off, u0) ^ u1;
    const uint32_t b = plain_apply(lds, kX4Off, u2) ^ u3;
    uint32_t z = plain_apply(lds, kX8Off, a) ^ b;
#pragma unroll
    for (int lvl = 0; lvl < 3; lvl++) {
        const uint32_t other = __shfl_xor(z, 1 << lvl, kWaveSize);
        const bool upper = (gl >> lvl) & 1;
        const uint32_t lower_v = upper ? other : z;
        const uint32_t upper_v = upper ? z : other;
        z = plain_apply(lds, kX4Off + (1 + lvl) * 4096, lower_v) ^ upper_v;
    }
    return z;
}

// Head word at distance ds = S - (word address): drop the bytes before S and
// inject the initial state into the four bytes at S.
__device__ __forceinline__ uint32_t keep_lo(int c);
__device__ __forceinline__ uint32_t head_word(uint32_t w, int ds, uint32_t init)
{
    const uint32_t inj = uint32_t((uint64_t(init) << 24) >> (24 - 8 * min(max(ds, -3), 3)));
    return (w & ~keep_lo(ds)) ^ ((ds > -4 && ds < 4) ? inj : 0u);
}

// Byte mask of a word whose first c bytes (clamped to 0..4) are kept.
__device__ __forceinline__ uint32_t keep_lo(int c)
{
    c = min(max(c, 0), 4);
    return c >= 4 ? 0xFFFFFFFFu : (1u << (8 * c)) - 1u;
}

// XOR of the 8 lanes of each lane group, valid in lanes 0-3 of the group
// (DPP: quad swaps, then the other quad of the 16-lane row; no LDS traffic).
__device__ __forceinline__ uint32_t group8_xor(uint32_t v)
{
    v ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, false));   // quad_perm 1,0,3,2
    v ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4E, 0xF, 0xF, false));   // quad_perm 2,3,0,1
    v ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x12C, 0xF, 0xF, false));  // row_ror:12 (lane + 4)
    return v;
}

// Entries of at most one 128-byte window (bins 0-1; 100-byte log entries are
// here): no Horner step and no per-entry multiply.  Byte b at distance m from
// the entry end contributes X^m(b), read from a 132 x 256 LDS table (rows for
// m <= 0 are zero), so a lane does 16 lookups for its 16 bytes and the group
// XORs its 8 lanes.  Round r of a wave covers 64 sorted
// slots; lane L owns slot 64 r + L: it loads that descriptor (one coalesced
// 1 KiB load per round instead of eight group-redundant ones), and at the end
// folds in the slot's initial state and stores its result.  Group g hashes
// the entries of lanes 8 g .. 8 g + 7 in turn, reading each owner's window
// (base, offset, length) by swizzle within the group.  Descriptors are loaded
// two rounds ahead and data one round ahead, so a wave's rounds overlap their
// memory latency with the previous round's lookups.
struct TinyOwn {
    uint64_t S, A;        // entry start; its 16-byte piece
    uint32_t geo;         // len (bits 0-7) | (S - A) << 8 for len >= 4 in bin 1; else 0
    uint32_t len, ix, init;
};

template <int q>
__device__ __forceinline__ uint32_t swz_from(uint32_t v)
{
    // lane (lane & 0x18) | q within each 32-lane half: lane q of this group
    return uint32_t(__builtin_amdgcn_ds_swizzle(int(v), 0x18 | (q << 5)));
}

template <int q = 0, class F>
__device__ __forceinline__ void static_for8(F&& f)
{
    if constexpr (q < 8) {
        f(std::integral_constant<int, q>{});
        static_for8<q + 1>(f);
    }
}

// Probe builds only (RAMCRC_STAMPS=1, tools/stamps.py): lane 0 of every wave
// records the 100 MHz real-time clock at k_entries' phase boundaries.
#ifndef RAMCRC_STAMPS
#define RAMCRC_STAMPS 0
#endif
#if RAMCRC_STAMPS
constexpr int kStampWaves = 8192, kStampSlots = 8;
__device__ unsigned long long g_stamps[kStampWaves * kStampSlots];
#define RAMCRC_STAMP(k)                                                                       \
    do {                                                                                      \
        const uint32_t sw_ = blockIdx.x * kEntWaves + threadIdx.x / kWaveSize;                \
        if ((threadIdx.x & (kWaveSize - 1)) == 0 && sw_ < uint32_t(kStampWaves))              \
            g_stamps[sw_ * kStampSlots + (k)] = __builtin_amdgcn_s_memrealtime();             \
    } while (0)
#define RAMCRC_STAMP_ONCE(k, flag) \
    do {                           \
        if (flag) {                \
            RAMCRC_STAMP(k);       \
            flag = false;          \
        }                          \
    } while (0)
#else
#define RAMCRC_STAMP_ONCE(k, flag) \
    do {                           \
        (void)(flag);              \
    } while (0)
#define RAMCRC_STAMP(k) \
    do {                \
    } while (0)
#endif

// The tiny phases with conflict-free table lookups: the
// window-relative table below puts a lookup's LDS bank on its window position,
// whatever the data byte.  Lane u of a group holds the window dwords u, u + 8,
// u + 16, u + 24 (window offsets 32 j + 4 u), so the 8 lanes of a group read
// rows 4 apart; each group takes the bytes of its dwords in a rotated order
// (byte (k + g) & 3 at instruction k, g the group's index in its 32-lane
// half), which puts the 4 groups of a half on the 4 residue classes: the 32
// lanes of a ds_read_b32 half hit 32 banks.  Bytes outside the entry are
// masked to 0, and X^m(0) = 0.
//
// tiny_run_cf: bins 0-1, entries of one 128-byte window (all 100-byte log
// entries).  tiny_multi: bins 2 .. kTinyK, entries of 2 .. kTinyK windows
// (objects of about 129 .. 500 B): window by window with Horner between them,
//   acc = X^e_w(acc) ^ R_w,
// R_w the group's sum over window w's bytes at their distance from the
// window's end e_w (128 for all but the last), X^e (e >= 4) four lookups in the
// same table by lanes gl & 3 and two quad swaps; an entry whose last window
// would hold only 1 .. 3 bytes stops a window early and its owner takes those
// bytes bytewise.  (The short-bin loop of entries_run spends an octet's head
// masks, fold and unpad multiply -- about 600 VALU per octet of 2-step entries
// -- where this spends the windows.)
//
// Round r of a wave covers 64 sorted slots; lane L owns slot 64 r + L: it loads
// that slot's descriptor two rounds ahead (one coalesced load per round instead
// of eight group-redundant ones; tiny_multi derives the entry geometry from it
// one round later), and at the end folds in the slot's initial state and
// stores the result.  Group g hashes the entries
// of lanes 8 g .. 8 g + 7 in turn, reading each owner's window (base, offset,
// length) by swizzle within the group; tiny_run_cf loads a round's windows one
// round ahead, tiny_multi an entry's windows one entry ahead.
struct TinyRaw {
    u32x4 dd;            // sorted descriptor {S, E}, or {off, len} on the direct path
    uint32_t ix, init;
};

struct TinyCf {
    uint64_t S;
    // E - A (bits 0-9; 0: nothing to hash, or bytewise), S - A (10-13), window
    // page-safe (14), E - S (16-25); A = S rounded down to 16
    uint32_t geo;
    uint32_t ix, init;
};

// windows hashed for an entry of geometry geo (tiny_multi: the last 1 .. 3
// bytes past a window go bytewise, as X^e needs e >= 4)
__device__ __forceinline__ uint32_t tk_tail(uint32_t geo)
{
    const uint32_t t = geo & 127u;
    return geo > 128 && t != 0 && t < 4 ? t : 0u;
}

__device__ __forceinline__ uint32_t tk_windows(uint32_t geo)
{
    return ((geo & 0x3FFu) - tk_tail(geo) + 127u) >> 7;
}

// The tiny phases' LDS holds X^(128 - q)(b) for window
// position q at ((q >> 6) << 16) | (b << 8) | ((q & 63) << 2) -- the data byte
// is address byte 1, so one v_perm forms an address from a per-lane constant
// -- and X^-128 (4 x 256 words) after it.  A window's bytes are summed at their
// distance from the window's end, whatever the entry; the owner lane moves its
// entry's sum to the entry end with X^e(X^-128(.)) (8 lookups per slot instead
// of per-window row arithmetic in every lane).  Masked bytes are 0, and
// X^m(0) = 0.
constexpr uint32_t kTwInvOff = 131072;
constexpr uint32_t kLdsTinyWr = kTwInvOff + 4096;
static_assert(kLdsTinyWr <= kLdsEntries, "k_entries' LDS holds the tiny phases' tables");

__device__ __forceinline__ uint32_t tw_addr(uint32_t q, uint32_t b)
{
    return ((q >> 6) << 16) | (b << 8) | ((q & 63) << 2);
}

// The tiny phases' tables built in place instead of copied: X^m is linear, so
// row q of X^(128 - q)(b) is the XOR of the basis words twb[q][k] over the set
// bits k of b.  Thread t takes row q = t % 128 and the 32 columns b0 .. b0 + 31,
// b0 = 32 (t / 128): T[b0] from bits 5-7, then T[b0 + i] = T[b0 + (i & (i - 1))]
// ^ twb[q][ctz i] -- 31 XORs -- and 32 stores at immediate offsets (a wave's
// 64 rows land on 32 banks).  Threads 0 .. 31 then build X^-128 the same way.
// The copy it replaces moved 132 KiB per CU through the L2 (33 MB per launch
// over the chip; 4.3 us of a 35 us 1M x 100 B launch, profiles/r04/ab).
// (split in two so that a caller can put loads of its own between them: the
// basis words' loads, then the build once they have landed)
struct TinyBasis {
    uint4 lo, hi, a, c;
};

__device__ __forceinline__ TinyBasis tiny_basis_load()
{
    TinyBasis t;
    const uint32_t q = threadIdx.x & 127;
    const uint4* bp = reinterpret_cast<const uint4*>(g_tab.twb[q]);
    t.lo = bp[0];
    t.hi = bp[1];
    t.a = t.c = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x < 32) {   // X^-128: table j = t / 8, columns 32 (t % 8) ..
        const uint4* ip = reinterpret_cast<const uint4*>(g_tab.twib[threadIdx.x >> 3]);
        t.a = ip[0];
        t.c = ip[1];
    }
    return t;
}

__device__ __forceinline__ void tiny_fill_build(uint8_t* lds, const TinyBasis& tb)
{
    static_assert(kEntWaves * kWaveSize == 1024, "one (row, column block) per thread");
    const uint32_t q = threadIdx.x & 127, b0 = 32 * (threadIdx.x >> 7);
    const uint32_t B[8] = {tb.lo.x, tb.lo.y, tb.lo.z, tb.lo.w, tb.hi.x, tb.hi.y, tb.hi.z, tb.hi.w};
    const uint32_t iv[8] = {tb.a.x, tb.a.y, tb.a.z, tb.a.w, tb.c.x, tb.c.y, tb.c.z, tb.c.w};
    const bool inv = threadIdx.x < 32;
    uint32_t T[32];
    T[0] = ((b0 >> 5) & 1 ? B[5] : 0u) ^ ((b0 >> 6) & 1 ? B[6] : 0u) ^ ((b0 >> 7) & 1 ? B[7] : 0u);
#pragma unroll
    for (int i = 1; i < 32; i++)
        T[i] = T[i & (i - 1)] ^ B[__builtin_ctz(i)];
    uint8_t* row = lds + (((q >> 6) << 16) | (b0 << 8) | ((q & 63) << 2));
#pragma unroll
    for (int i = 0; i < 32; i++)
        *reinterpret_cast<uint32_t*>(row + 256 * i) = T[i];
    if (inv) {
        const uint32_t c0 = 32 * (threadIdx.x & 7);
        uint32_t U[32];
        U[0] = ((c0 >> 5) & 1 ? iv[5] : 0u) ^ ((c0 >> 6) & 1 ? iv[6] : 0u) ^ ((c0 >> 7) & 1 ? iv[7] : 0u);
#pragma unroll
        for (int i = 1; i < 32; i++)
            U[i] = U[i & (i - 1)] ^ iv[__builtin_ctz(i)];
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds + kTwInvOff) + 256 * (threadIdx.x >> 3) + c0;
#pragma unroll
        for (int i = 0; i < 32; i++)
            dst[i] = U[i];
    }
}

__device__ __forceinline__ void tiny_fill(uint8_t* lds)
{
    tiny_fill_build(lds, tiny_basis_load());
}

// Per-lane address constants: byte k of a rotated dword (window position
// 32 j + 4 u + ((k + g4) & 3)) of dword pair j >> 1; + 128 for odd j.
struct TwRows {
    uint32_t lr[2][4];
    __device__ TwRows(uint32_t gl, uint32_t g4)
    {
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                lr[h][k] = (uint32_t(h) << 16) | (16 * gl + 4 * ((uint32_t(k) + g4) & 3));
    }
};

// Per-lane v_perm selectors for tiny_win_wr<true>: lookup k of a dword takes
// its byte (k + g4) & 3 straight into address bits 8-15, which replaces the
// v_alignbyte rotation per dword (4 VGPRs for 32 VALU per round).
struct TwSel {
    uint32_t sel[4];
    __device__ TwSel() {}
    __device__ explicit TwSel(uint32_t g4)
    {
#pragma unroll
        for (int k = 0; k < 4; k++)
            sel[k] = 0x0C020000u | ((4u + ((uint32_t(k) + g4) & 3)) << 8);
    }
};

// The group's sum over one window's bytes in [sa, e), byte b at position o
// as X^(128 - o)(b) (relative to the window's end; all 8 lanes get it).
// kTail3: the caller knows e >= 96 for every window of the wave, so dwords
// 0-2 (window offsets below 96) need no tail mask
template <bool kLsel = false, bool kTail3 = false>
__device__ __forceinline__ uint32_t tiny_win_wr(const uint8_t* lds, const u32x4& wv, uint32_t sa,
                                                uint32_t e, const TwRows& rw, uint32_t gl, uint32_t g4,
                                                const TwSel& ts = TwSel())
{
    // tail: dword j keeps its bytes before e, clamp(e - 32 j - 4 u, 0, 4)
    const int z = 32 - 8 * int(e) + 32 * int(gl);   // bits to drop from dword 0's top
    // head: window bytes before sa lie in dword 0 of lanes 0-3
    const uint32_t hd = uint32_t(min(max(8 * (int(sa) - 4 * int(gl)), 0), 32));
    const uint32_t ws[4] = {wv.x, wv.y, wv.z, wv.w};
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t keep = 0xFFFFFFFFu;
        if (!kTail3 || j == 3) {
            // one v_med3 after the add (the compiler's max/add/min is three ops)
            uint32_t sh;
            asm("v_med3_i32 %0, %1, 0, 32" : "=v"(sh) : "v"(z + 256 * j));
            keep = uint32_t(uint64_t(0xFFFFFFFFu) >> sh);
        }
        if (j == 0)
            keep &= uint32_t(~uint64_t(0) << hd);
        const uint32_t xb = ws[j] & keep;
        if constexpr (kLsel) {
            // lookup k takes byte (k + g4) & 3 (conflict-free banks) through
            // the lane's own selector instead of a rotated copy of the dword
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[4 * j + k] = *reinterpret_cast<const uint32_t*>(
                    lds + __builtin_amdgcn_perm(xb, rw.lr[j >> 1][k], ts.sel[k]) + 128 * (j & 1));
        } else {
            const uint32_t xr = __builtin_amdgcn_alignbyte(xb, xb, g4);   // conflict-free banks
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[4 * j + k] = *reinterpret_cast<const uint32_t*>(
                    lds + __builtin_amdgcn_perm(xr, rw.lr[j >> 1][k], 0x0C020000u | ((4u + uint32_t(k)) << 8)) +
                    128 * (j & 1));
        }
    }
    const uint32_t t0 = xor3(v[0], v[1], v[2]), t1 = xor3(v[3], v[4], v[5]);
    const uint32_t t2 = xor3(v[6], v[7], v[8]), t3 = xor3(v[9], v[10], v[11]);
    const uint32_t t4 = xor3(v[12], v[13], v[14]);
    uint32_t R = xor3(xor3(t0, t1, t2), xor3(t3, t4, v[15]), 0u);
    R = group8_xor_all(R);
    return R;
}

// X^m(v) for 4 <= m <= 128 (byte k at distance m - k), and X^-128(v)
__device__ __forceinline__ uint32_t tw_shift(const uint8_t* lds, uint32_t v, uint32_t m)
{
    auto t = [&](uint32_t q, uint32_t b) { return *reinterpret_cast<const uint32_t*>(lds + tw_addr(q, b)); };
    return xor3(t(128 - m, v & 0xFF), t(129 - m, (v >> 8) & 0xFF), t(130 - m, (v >> 16) & 0xFF)) ^
           t(131 - m, v >> 24);
}

__device__ __forceinline__ uint32_t tw_inv128(const uint8_t* lds, uint32_t v)
{
    auto t = [&](uint32_t k, uint32_t b) {
        return *reinterpret_cast<const uint32_t*>(lds + kTwInvOff + 4 * (256 * k + b));
    };
    return xor3(t(0, v & 0xFF), t(1, (v >> 8) & 0xFF), t(2, (v >> 16) & 0xFF)) ^ t(3, v >> 24);
}

template <bool kPF>
__device__ __forceinline__ bool tiny_run_cf(const BatchDesc& d, const Sorted& so, uint8_t* lds,
                                            bool bad, uint32_t blk, uint32_t nblk, bool need_table)
{
    const uint64_t direct_n = so.bt->direct_n;   // all tiny: the caller's table, in place
    if (!direct_n && so.bt->start[2] == so.bt->start[0]) {
        // no entry of at most one window (uniform: every wave exits); the
        // multi-window phase still needs the table
        if (need_table) {
            tiny_fill(lds);
            return !__syncthreads_or(bad);
        }
        return true;
    }
    const int lane = threadIdx.x & (kWaveSize - 1);
    const uint32_t gl = uint32_t(lane) & 7;
    const uint32_t g4 = (uint32_t(lane) >> 3) & 3;
    const uint64_t wave = uint64_t(blk) * kEntWaves +
                          __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
    const uint64_t nwaves = uint64_t(nblk) * kEntWaves;
    const uint64_t s0 = direct_n ? 0 : so.bt->start[0], s1 = direct_n ? direct_n : so.bt->start[2];
    const uint64_t rounds = (s1 - s0 + 63) / 64;
    const bool finalize = d.flags & RAMCRC_FINALIZE;
    const uint64_t dummy = reinterpret_cast<uint64_t>(so.bt);
    typedef const __attribute__((address_space(1))) uint32_t g32;

    auto load_own = [&](uint64_t r) -> TinyOwn {
        TinyOwn o;
        const uint64_t sl = s0 + r * 64 + uint32_t(lane);
        u32x4 dd = {0u, 0u, 0u, 0u};
        o.ix = kNoIdx;
        o.init = 0xFFFFFFFFu;
        if (r < rounds && sl < s1) {
            if (direct_n) {   // kTable: buffer sl = base + off[sl], len[sl]; records: record sl
                uint64_t S, E;
                bool act = true;
                if (d.rec) {
                    act = buffer_range<kRecords>(d, sl, S, E);
                } else {
                    S = reinterpret_cast<uint64_t>(d.base) + d.off[sl];
                    E = S + d.len[sl];
                }
                if (act)
                    dd = u32x4{uint32_t(S), uint32_t(S >> 32), uint32_t(E), uint32_t(E >> 32)};
                o.ix = act ? uint32_t(sl) : kNoIdx;
                if (d.init)
                    o.init = d.init[sl];
                if (act && E - S >= 4 && E - (S & ~uint64_t(15)) > kStep) {
                    // not tiny after all: the histogram lied; refuse, write nothing
                    atomicOr(so.status, kStatusSticky | kStatusBins);
                    o.ix = kNoIdx;
                }
            } else {
                dd = so.desc[sl];
                o.ix = so.idx[sl];
                if (d.init)
                    o.init = so.init[sl];
            }
        }
        o.S = (uint64_t(dd.y) << 32) | dd.x;
        const uint64_t E = (uint64_t(dd.w) << 32) | dd.z;
        const uint32_t len = uint32_t(E - o.S);   // <= 128 in bins 0-1
        const uint64_t A = o.S & ~uint64_t(15);   // the window; not kept (registers)
        o.geo = (o.ix != kNoIdx && len >= 4) ? (len | (uint32_t(o.S - A) << 8)) : 0u;
        // bit 12: the whole window [A, A + 128) lies in pages that hold entry
        // bytes (or, with nothing to hash, in the bin table), so its dwords
        // can be read unclamped
        const bool safe = !o.geo || ((A + 127) >> 12) == ((E - 1) >> 12);
        o.geo |= (safe ? (1u << 12) : 0u) | (len << 16);   // len again in bits 16-23
        return o;
    };
    // the group's eight windows: dwords gl + 8 j of each owner's window.
    // Bytes outside the entry are masked, so a dword past E may hold
    // anything: when all eight windows of a q stay inside pages that hold
    // entry bytes (bit 12 of geo), the dwords are read as they are; otherwise
    // a dword that starts at or past E loads the entry's last dword instead,
    // so no load leaves the entry's last dword.
    auto issue = [&](const TinyOwn& o, u32x4 (&w)[8], uint32_t (&geo)[8], uint32_t& st) {
        st = d.vstat && o.ix != kNoIdx ? load_u32_any(o.S - 4) : 0u;
        static_for8([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            geo[q] = swz_from<q>(o.geo);
            const uint64_t Sq = (uint64_t(swz_from<q>(uint32_t(o.S >> 32))) << 32) |
                                swz_from<q>(uint32_t(o.S));
            // nothing to hash: the window loads read valid memory (the bin table)
            const uint64_t A = (geo[q] & 0xFFF) ? (Sq & ~uint64_t(15)) : dummy;
            [[maybe_unused]] const uint64_t au = A + 4 * gl;
            u32x4 v;
            if (__builtin_amdgcn_ballot_w64(!((geo[q] >> 12) & 1)) == 0) {
                // every window of this q is page-safe: plain loads, immediate offsets
                v.x = *reinterpret_cast<g32*>(au);
                v.y = *reinterpret_cast<g32*>(au + 32);
                v.z = *reinterpret_cast<g32*>(au + 64);
                v.w = *reinterpret_cast<g32*>(au + 96);
            } else {
                const uint32_t e = ((geo[q] >> 8) & 0xF) + (geo[q] & 0xFF);   // E - A (0: empty)
                const int el = (max(int(e) - 1, 0) & ~3) - int(4 * gl);   // last dword, from 4 u
                v.x = *reinterpret_cast<g32*>(au + min(0, el));
                v.y = *reinterpret_cast<g32*>(au + min(32, el));
                v.z = *reinterpret_cast<g32*>(au + min(64, el));
                v.w = *reinterpret_cast<g32*>(au + min(96, el));
            }
            w[q] = v;
        });
    };

    // The table's basis words are loaded first, round 0's windows issued as
    // soon as its owners are known, and the table built while those loads are
    // in flight (the build waits for the basis alone)
    const TinyBasis tb = tiny_basis_load();
    uint64_t r = wave;
    TinyOwn o0 = load_own(r), o1 = load_own(r + nwaves);
    u32x4 wc[8];
    uint32_t gc[8], sc;
    issue(o0, wc, gc, sc);
    tiny_fill_build(lds, tb);
    const TwRows rw(gl, g4);
    // per-lane v_perm selectors instead of a v_alignbyte per dword: without
    // the register prefetch they fit; with the prefetch, the windows' geometry
    // is swizzled again from the owner in the compute so that the selectors
    // and the second window body fit in the registers
    const TwSel ts(g4);
    if (__syncthreads_or(bad))
        return false;
    RAMCRC_STAMP(5);
    bool first_round = true;
    for (; r < rounds; r += nwaves) {
        const TinyOwn o2 = load_own(r + 2 * nwaves);
        u32x4 wn[8];
        uint32_t gn[8], sn = 0;
        if constexpr (kPF) {
            if (r + nwaves < rounds)
                issue(o1, wn, gn, sn);
        }
        uint32_t mine = 0;
        static_for8([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const uint32_t g = kPF ? swz_from<q>(o0.geo) : gc[q];
            const uint32_t sa = (g >> 8) & 0xF;
            const uint32_t e = sa + (g & 0xFF);           // window-relative end, <= 128
            // (a wave-uniform branch: entries of 81 B or more skip most tail masks)
            const bool t3 = __builtin_amdgcn_ballot_w64(e < 96) == 0;
            const uint32_t R = t3 ? tiny_win_wr<true, true>(lds, wc[q], sa, e, rw, gl, g4, ts)
                                  : tiny_win_wr<true, false>(lds, wc[q], sa, e, rw, gl, g4, ts);
            mine = gl == uint32_t(q) ? R : mine;
        });
        // own slot: the initial state (byte k at distance len - k), or bytewise
        if (o0.ix != kNoIdx) {
            uint32_t R;
            const uint32_t n = (o0.geo >> 16) & 0xFF;   // the entry's length
            if (n >= 4) {
                // the window sum moved from the window's end to the entry's end,
                // e = S - A + n >= 4 bytes into the window
                const uint32_t e = ((o0.geo >> 8) & 0xF) + n;
                R = tw_shift(lds, tw_inv128(lds, mine), e) ^ tw_shift(lds, o0.init, n);
            } else {
                R = o0.init;
                for (uint32_t k = 0; k < n; k++)
                    R = *reinterpret_cast<const uint32_t*>(
                            lds + tw_addr(127, (R ^ *(const gu8*)(o0.S + k)) & 0xFF)) ^ (R >> 8);
            }
            const uint32_t Rf = finalize ? ~R : R;
            d.out[o0.ix] = Rf;
            if (d.vstat && Rf != sc)
                atomicAdd(&d.vstat[d.rec[o0.ix].x].bad_objects, 1u);
        }
        RAMCRC_STAMP_ONCE(6, first_round);
        o0 = o1;
        o1 = o2;
        if constexpr (kPF) {
            sc = sn;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                wc[q] = wn[q];
                gc[q] = gn[q];
            }
        } else {
            // the next round's windows straight into the spent buffer: the
            // other waves of the SIMD cover their latency
            if (r + nwaves < rounds)
                issue(o0, wc, gc, sc);
        }
    }
    return true;
}

// bins 2 .. kTinyK (see above): one entry per q as in tiny_run_cf, all K
// windows of a group's entry loaded while earlier ones are hashed: a ring of
// kDepth buffers of kK windows, the entry kDepth - 1 ahead loaded at each q.
// Bin 2 (entries of at most two windows: the objects of 128-byte values) runs
// with kK = 2 and a ring of 4 -- three entries in flight per group for the
// registers the general loop spends on two buffers of four windows; bins 3 ..
// kTinyK with kK = kTinyK and two buffers.
// kDirect: a records or table batch read in place (BinTable::direct_multi),
// entry i at slot i; an entry that is not one of 2 .. kK windows refuses the
// launch (the summary or histogram that chose this path was wrong), as the
// direct tiny path does.
template <int kK, int kDepth, bool kDirect = false>
__device__ __forceinline__ void tiny_multi_run(const BatchDesc& d, const Sorted& so, const uint8_t* lds,
                                               uint32_t blk, uint32_t nblk, uint64_t s0, uint64_t s1)
{
    static_assert(kDepth >= 2 && 8 % kDepth == 0, "tiny_multi: ring index q % kDepth must be static");
    if (s0 == s1)
        return;   // uniform
    const int lane = threadIdx.x & (kWaveSize - 1);
    const uint32_t gl = uint32_t(lane) & 7;
    const uint32_t g4 = (uint32_t(lane) >> 3) & 3;
    const uint64_t wave = uint64_t(blk) * kEntWaves +
                          __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
    const uint64_t nwaves = uint64_t(nblk) * kEntWaves;
    const uint64_t rounds = (s1 - s0 + 63) / 64;
    if (wave >= rounds)
        return;   // uniform
    const bool finalize = d.flags & RAMCRC_FINALIZE;
    const uint64_t dummy = reinterpret_cast<uint64_t>(so.bt);
    typedef const __attribute__((address_space(1))) uint32_t g32;

    auto load_raw = [&](uint64_t r) -> TinyRaw {
        TinyRaw w;
        const uint64_t sl = s0 + r * 64 + uint32_t(lane);
        const bool in = r < rounds && sl < s1;
        if constexpr (kDirect) {
            uint64_t S = 0, E = 0;
            bool act = in;
            if (act) {
                if (d.rec) {   // records: record sl
                    act = record_range(d, d.rec[sl], S, E);
                } else {       // kTable: buffer sl = base + off[sl], len[sl]
                    S = reinterpret_cast<uint64_t>(d.base) + d.off[sl];
                    E = S + d.len[sl];
                }
            }
            if (act) {
                const uint64_t k = entry_steps(S, E);
                // bounded by this instantiation's windows: the two-window ring
                // (kK = 2) refuses a record of three or more windows even if
                // the walk summary's "wide" bit missed it
                if (k < 2 || k > uint64_t(kK)) {
                    atomicOr(so.status, kStatusSticky | kStatusBins);   // refuse, write nothing
                    act = false;
                }
            }
            w.dd = u32x4{uint32_t(S), uint32_t(S >> 32), uint32_t(E), uint32_t(E >> 32)};
            w.ix = act ? uint32_t(sl) : kNoIdx;
            w.init = d.init && in ? d.init[sl] : 0xFFFFFFFFu;
        } else {
            const uint64_t sc = in ? sl : s0;
            w.dd = so.desc[sc];
            const uint32_t ix = so.idx[sc];
            w.ix = in ? ix : kNoIdx;
            w.init = d.init ? so.init[sc] : 0xFFFFFFFFu;
        }
        return w;
    };
    auto own_of = [&](const TinyRaw& w) -> TinyCf {
        TinyCf o;
        o.ix = w.ix;
        o.init = w.init;
        uint64_t S = (uint64_t(w.dd.y) << 32) | w.dd.x, E = (uint64_t(w.dd.w) << 32) | w.dd.z;
        if (o.ix == kNoIdx)
            S = E = dummy;
        o.S = S;
        const uint32_t len = uint32_t(E - S);
        const uint64_t A = S & ~uint64_t(15);
        o.geo = (len >= 4 ? uint32_t(E - A) : 0u) | (uint32_t(S - A) << 10) | (len << 16);
        return o;
    };
    // the owner's stored object checksum (records mode) and the word holding
    // the entry's last three bytes (its bytewise tail), a round ahead
    auto own_loads = [&](const TinyCf& o, uint32_t& st, uint32_t& tw) {
        st = d.vstat && o.ix != kNoIdx ? load_u32_any(o.S - 4) : 0u;
        const uint64_t E = o.S + ((o.geo >> 16) & 0x3FF);
        const uint64_t a = o.ix != kNoIdx ? E - 3 : dummy;   // entries here hold >= 113 bytes
        const uint64_t b = o.ix != kNoIdx ? E - 1 : dummy;
        const uint32_t w0 = *reinterpret_cast<g32*>(a & ~uint64_t(3));
        const uint32_t w1 = *reinterpret_cast<g32*>(b & ~uint64_t(3));
        tw = __builtin_amdgcn_alignbyte(w1, w0, uint32_t(a) & 3);   // bytes E - 3, E - 2, E - 1
    };
    const TwRows rw(gl, g4);
    // the windows of the entry (geo, S) into w: window k is [A + 128 k, + 128);
    // a dword at or past the window's last entry byte reads that byte's dword
    auto load_entry = [&](uint32_t geo, uint64_t S, u32x4 (&w)[kK]) {
        const uint32_t K = tk_windows(geo);
        const uint32_t el = (geo & 0x3FF) - tk_tail(geo) - 128 * (K - 1);   // last window's end
        const uint64_t au = (S & ~uint64_t(15)) + 4 * gl;
#pragma unroll
        for (int k = 0; k < kK; k++) {
            if (uint32_t(k) < K) {
                const uint32_t e = uint32_t(k) + 1 == K ? el : 128u;
                const int lim = (max(int(e) - 1, 0) & ~3) - int(4 * gl);
                const uint64_t aw = au + 128 * uint64_t(k);
                w[k].x = *reinterpret_cast<g32*>(aw + min(0, lim));
                w[k].y = *reinterpret_cast<g32*>(aw + min(32, lim));
                w[k].z = *reinterpret_cast<g32*>(aw + min(64, lim));
                w[k].w = *reinterpret_cast<g32*>(aw + min(96, lim));
            }
        }
    };
    // entry qe of the round whose owners are `on` (swizzled from lane 8g + qe)
    auto load_q = [&](auto qc, const TinyCf& on, bool valid, uint32_t& gq, u32x4 (&w)[kK]) {
        constexpr int qe = decltype(qc)::value;
        uint32_t g = swz_from<qe>(on.geo);
        g = valid ? g : 0u;
        const uint64_t Sn = (uint64_t(swz_from<qe>(uint32_t(on.S >> 32))) << 32) | swz_from<qe>(uint32_t(on.S));
        gq = g;
        load_entry(g, Sn, w);
    };

    uint64_t r = wave;
    TinyRaw w1 = load_raw(r + nwaves);
    TinyCf o0 = own_of(load_raw(r));
    uint32_t sc, tc;
    own_loads(o0, sc, tc);
    u32x4 buf[kDepth][kK];
    uint32_t gq[kDepth];
    // the ring's first kDepth - 1 entries
    static_for8([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j < kDepth - 1)
            load_q(jc, o0, true, gq[j], buf[j]);
    });
    for (; r < rounds; r += nwaves) {
        const TinyRaw w2 = load_raw(r + 2 * nwaves);
        const TinyCf o1 = own_of(w1);   // loaded a round ago
        const bool more = r + nwaves < rounds;
        uint32_t sn = 0, tn = 0;
        own_loads(o1, sn, tn);
        uint32_t mine = 0;
        static_for8([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            // the group's entry kDepth - 1 ahead: of this round, or of the next
            {
                constexpr int qn = q + kDepth - 1;
                constexpr int bn = qn % kDepth;
                if constexpr (qn < 8)
                    load_q(std::integral_constant<int, qn>{}, o0, true, gq[bn], buf[bn]);
                else
                    load_q(std::integral_constant<int, qn - 8>{}, o1, more, gq[bn], buf[bn]);
            }
            constexpr int bq = q % kDepth;
            const uint32_t geo = gq[bq];
            const uint32_t K = tk_windows(geo);
            const uint32_t el = (geo & 0x3FF) - tk_tail(geo) - 128 * (K - 1);
            // window sums at their distance from their window's end; Horner with
            // X^128 between windows: acc is relative to the last window's end
            uint32_t acc = tiny_win_wr(lds, buf[bq][0], (geo >> 10) & 0xF,
                                       K > 1 ? 128u : (K ? el : 0u), rw, gl, g4);
#pragma unroll
            for (int k = 1; k < kK; k++) {
                if (__builtin_amdgcn_ballot_w64(uint32_t(k) < K)) {   // uniform
                    const uint32_t e = uint32_t(k) + 1 == K ? el : 128u;
                    const uint32_t R = tiny_win_wr(lds, buf[bq][k], 0, uint32_t(k) < K ? e : 0u, rw, gl, g4);
                    // X^128(acc) by lanes gl & 3 (byte gl & 3 at distance 128 - (gl & 3))
                    const uint32_t kk = gl & 3;
                    uint32_t X = *reinterpret_cast<const uint32_t*>(lds + tw_addr(kk, (acc >> (8 * kk)) & 0xFF));
                    X ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(X), 0xB1, 0xF, 0xF, false));
                    X ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(X), 0x4E, 0xF, 0xF, false));
                    acc = uint32_t(k) < K ? (X ^ R) : acc;
                }
            }
            mine = gl == uint32_t(q) ? acc : mine;
        });
        // own slot: the initial state X^(n - tail)(init) in steps of at most 128,
        // then the tail bytewise
        if (o0.ix != kNoIdx) {
            const uint32_t n = (o0.geo >> 16) & 0x3FF, tail = tk_tail(o0.geo);
            const uint32_t K = tk_windows(o0.geo);
            const uint32_t el = (o0.geo & 0x3FF) - tail - 128 * (K - 1);   // >= 4
            uint32_t v = o0.init, m = n - tail;
            while (m > 128) {
                const uint32_t st = m - 128 >= 4 ? 128u : m - 4;
                v = tw_shift(lds, v, st);
                m -= st;
            }
            // the windows' sum moved from the last window's end to E - tail
            uint32_t R = tw_shift(lds, tw_inv128(lds, mine), el) ^ tw_shift(lds, v, m);
            for (uint32_t k = 3 - tail; k < 3; k++)   // bytes E - tail .. E - 1
                R = *reinterpret_cast<const uint32_t*>(lds + tw_addr(127, (R ^ (tc >> (8 * k))) & 0xFF)) ^
                    (R >> 8);
            const uint32_t Rf = finalize ? ~R : R;
            d.out[o0.ix] = Rf;
            if (d.vstat && Rf != sc)
                atomicAdd(&d.vstat[d.rec[o0.ix].x].bad_objects, 1u);
        }
        o0 = o1;
        w1 = w2;
        sc = sn;
        tc = tn;
    }
}

__device__ __forceinline__ void tiny_multi(const BatchDesc& d, const Sorted& so, const uint8_t* lds,
                                           uint32_t blk, uint32_t nblk)
{
    if constexpr (kTinyK >= 2) {
        if (so.bt->direct_multi) {
            if (kTinyK > 2 && so.bt->direct_multi_k2)
                tiny_multi_run<2, 4, true>(d, so, lds, blk, nblk, 0, so.bt->direct_multi);
            else
                tiny_multi_run<kTinyK, 2, true>(d, so, lds, blk, nblk, 0, so.bt->direct_multi);
            return;
        }
        const uint64_t s0 = so.bt->start[2], s1 = so.bt->start[kTinyK + 1];
        if (s0 == s1)
            return;   // uniform
        if constexpr (kTinyK > 2) {
            const uint64_t s2 = so.bt->start[3];
            tiny_multi_run<2, 4>(d, so, lds, blk, nblk, s0, s2);
            tiny_multi_run<kTinyK, 2>(d, so, lds, blk, nblk, s2, s1);
        } else {
            tiny_multi_run<kTinyK, 2>(d, so, lds, blk, nblk, s0, s1);
        }
    }
}

// Entries of two or more 128-byte steps (bins >= 2).  One octet (8 entries,
// one per lane group) at a time:
//   step 0 (head)          start mask and init injection, precomputed per octet;
//   steps 1 .. Kmin-2      interior for every entry of the octet: no masks,
//                          unconditional loads, kPU-deep ping-pong prefetch;
//   steps Kmin-1 .. Koct-1 tail: end mask, lanes past their entry frozen.
// The head and the first two tail loads are issued with the interior ones, the
// next octet's descriptor is prefetched, and the previous octet's fold runs
// after this octet's loads are in flight.  The unpad multiply x^(-8 pad) is
// batched: lane gl of a group keeps the fold of octet gl of the current eight,
// and one wave-wide multiply finishes 64 entries.  Waves split the bins by
// estimated work (steps + kOctetCost per octet).
//
// kSmall: bins 2 .. kSmallK (whole octets loaded one ahead); otherwise bins
// kSmallK+1 and up.  Two instantiations keep the register allocation of the
// long-entry loop free of the short-entry loop's state.
template <bool kSmall>
__device__ __forceinline__ void entries_run(const BatchDesc& d, const Sorted& so, const uint8_t* lds,
                                            uint32_t blk, uint32_t nblk)
{
    constexpr int kT = kTinyK > kSmallK ? kTinyK : kSmallK;
    constexpr int b0 = kSmall ? (kTinyK > 1 ? kTinyK + 1 : 2) : kT + 1, b1 = kSmall ? kSmallK + 1 : kNB;
    if (b0 >= b1)
        return;
    const uint64_t* s_items = reinterpret_cast<const uint64_t*>(lds + kBinOff);   // kNB + 1
    const uint64_t* s_start = s_items + (kNB + 1);                                // kNB
    const uint32_t* s_cost = reinterpret_cast<const uint32_t*>(s_start + kNB);    // kNB
    if (s_items[b0] == s_items[b1])
        return;   // no entry in this phase's bins (uniform)
    const uint32_t* xinv = reinterpret_cast<const uint32_t*>(lds + kXinvOff);

    const int lane = threadIdx.x & (kWaveSize - 1);
    const int g = lane >> 3, gl = lane & 7;
    const RepOp op(lane);
    const uint64_t wave = uint64_t(blk) * kEntWaves +
                          __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
    const uint64_t nwaves = uint64_t(nblk) * kEntWaves;
    const uint64_t I0 = s_items[b0], T = s_items[b1] - I0;
    const bool finalize = d.flags & RAMCRC_FINALIZE;
    const uint64_t dummy = reinterpret_cast<uint64_t>(so.bt);   // device memory, 16 B aligned

    // batched unpad: lane gl holds octet gl of the current batch of eight
    uint32_t bY = 0, bPad = 0, bIx = kNoIdx, bSt = 0;
    int nb = 0;
    auto flush_batch = [&]() {
        const uint32_t R = mulmod_horner(bY, xinv[bPad & 255]);
        if (bIx != kNoIdx) {
            const uint32_t Rf = finalize ? ~R : R;
            d.out[bIx] = Rf;
            if (d.vstat && Rf != bSt)   // ObjectManager::replaySegment's check (:659-663)
                atomicAdd(&d.vstat[d.rec[bIx].x].bad_objects, 1u);
        }
        bIx = kNoIdx;
        nb = 0;
    };
    // deferred fold of the previous octet
    bool pend = false;
    uint32_t pu0 = 0, pu1 = 0, pu2 = 0, pu3 = 0, ppad = 0, pix = kNoIdx, pst = 0;
    auto flush = [&]() {
        if (pend) {
            const uint32_t Y = group_fold(lds, gl, pu0, pu1, pu2, pu3);
            if (gl == nb) {
                bY = Y;
                bPad = ppad;
                bIx = pix;
                bSt = pst;
            }
            pend = false;
            if (++nb == kG)
                flush_batch();
        }
    };

    // the octets whose first work unit lies in [lo, hi)
    auto run = [&](const uint64_t lo, const uint64_t hi) {
        for (int b = b0; b < b1; b++) {
            const uint64_t ib = s_items[b], ie = s_items[b + 1];
            if (ie <= lo || ib == ie)
                continue;
            if (ib >= hi)
                break;
            const uint64_t cost = s_cost[b];
            const uint64_t oa = ((lo > ib ? lo : ib) - ib + cost - 1) / cost;
            const uint64_t ob = ((hi < ie ? hi : ie) - ib + cost - 1) / cost;
            const uint64_t sb = s_start[b];
            if (oa >= ob)
                continue;
            if constexpr (kSmall) {
                // Exact bins of at most kSmallK steps: the whole octet is loaded
                // one octet ahead, so the load latency hides behind the previous
                // octet's steps and fold instead of stalling every octet.
                const uint32_t K = uint32_t(b);
                struct Oct {
                    uint64_t S, E;
                    uint32_t init, ix, steps, st, st1;   // st, st1: dwords around the stored checksum
                    u32x4 w[kSmallK + 1];
                };
                auto load_oct = [&](uint64_t o, Oct& t) {
                    const uint64_t sl = sb + o * kG + g;
                    const u32x4 dd = so.desc[sl];
                    t.ix = so.idx[sl];
                    t.init = d.init ? so.init[sl] : 0xFFFFFFFFu;
                    t.S = (uint64_t(dd.y) << 32) | dd.x;
                    t.E = (uint64_t(dd.w) << 32) | dd.z;
                    t.steps = t.ix != kNoIdx ? uint32_t(entry_steps_line(t.S, t.E)) : 0u;   // K or K+1
                    const uint64_t A = line_base(t.S);
                    const uint64_t p0 = A + gl * 16;
                    const uint64_t safe = t.steps ? A : dummy;
                    t.st = t.st1 = 0u;   // joined at use: a join here would wait for them
                    if (d.vstat && t.steps) {
                        typedef const __attribute__((address_space(1))) uint32_t g32s;
                        const uint64_t sa = (t.S - 4) & ~uint64_t(3);
                        t.st = *reinterpret_cast<g32s*>(sa);
                        t.st1 = *reinterpret_cast<g32s*>(sa + 4);
                    }
    #pragma unroll
                    for (int k = 0; k <= kSmallK; k++) {
                        const uint64_t a = p0 + uint64_t(k) * kStep;
                        if (k <= int(K))
                            t.w[k] = load16(t.steps && a < t.E ? a : safe);
                    }
                };
                Oct cur, nxt;
                load_oct(oa, cur);
                for (uint64_t o = oa; o < ob; o++) {
                    if (o + 1 < ob)
                        load_oct(o + 1, nxt);
                    const uint64_t A = line_base(cur.S);
                    const uint64_t p0 = A + gl * 16;
                    uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0;
                    {
                        const int off = int(uint32_t(cur.S - A)) - 16 * gl;
                        u32x4 w = cur.w[0];
                        w.x = head_word(w.x, off, cur.init);
                        w.y = head_word(w.y, off - 4, cur.init);
                        w.z = head_word(w.z, off - 8, cur.init);
                        w.w = head_word(w.w, off - 12, cur.init);
                        op.apply4(lds, u0, u1, u2, u3, w);
                    }
                    const int64_t erel = int64_t(cur.E - p0);
    #pragma unroll
                    for (int k = 1; k <= kSmallK; k++) {
                        if (k <= int(K)) {
                            const int64_t de64 = erel - int64_t(k) * int64_t(kStep);
                            const int de = int(de64 < 0 ? 0 : (de64 > 16 ? 16 : de64));
                            u32x4 w = cur.w[k];
                            w.x &= keep_lo(de);
                            w.y &= keep_lo(de - 4);
                            w.z &= keep_lo(de - 8);
                            w.w &= keep_lo(de - 12);
                            const bool live = uint32_t(k) < cur.steps;
                            uint32_t v0 = u0, v1 = u1, v2 = u2, v3 = u3;
                            op.apply4(lds, v0, v1, v2, v3, w);
                            u0 = live ? v0 : u0;
                            u1 = live ? v1 : u1;
                            u2 = live ? v2 : u2;
                            u3 = live ? v3 : u3;
                        }
                    }
                    pend = true;
                    pu0 = u0;
                    pu1 = u1;
                    pu2 = u2;
                    pu3 = u3;
                    ppad = uint32_t((A + uint64_t(cur.steps) * kStep) - cur.E);
                    pix = cur.ix;
                    pst = __builtin_amdgcn_alignbyte(cur.st1, cur.st, uint32_t(cur.S - 4) & 3);
                    flush();
                    cur = nxt;
                }
            }
        }
    };
    // One octet of a long bin b: 8 entries, one per lane group.
    auto octet = [&](const u32x4 dd, const uint32_t ix, const uint32_t init, const int b) {
            const uint64_t S = (uint64_t(dd.y) << 32) | dd.x;
            const uint64_t E = (uint64_t(dd.w) << 32) | dd.z;
            const uint32_t steps = ix != kNoIdx ? uint32_t(entry_steps_line(S, E)) : 0u;
            const uint64_t A = line_base(S);   // windows on 128-byte lines
            const uint64_t p0 = A + gl * 16;
            // longest / shortest entry of the octet (padding slots excluded)
            uint32_t Koct, Kmin;
            if (b <= 32) {
                // exact bin b: a step count is b or b + 1 (line_base(S) lies
                // at most 112 bytes before the 16-byte piece of S)
                const bool hi = __ballot(steps == uint32_t(b) + 1) != 0;
                const bool lo1 = __ballot(steps == uint32_t(b)) != 0;
                Koct = hi ? uint32_t(b) + 1 : (lo1 ? uint32_t(b) : 0u);
                Kmin = lo1 ? uint32_t(b) : uint32_t(b) + 1;
            } else {
                uint32_t kmax32 = steps, kmin32 = steps ? steps : 0xFFFFFFFFu;
#pragma unroll
                for (int s = 8; s < 64; s <<= 1) {
                    kmax32 = max(kmax32, uint32_t(__shfl_xor(kmax32, s, kWaveSize)));
                    kmin32 = min(kmin32, uint32_t(__shfl_xor(kmin32, s, kWaveSize)));
                }
                Koct = __builtin_amdgcn_readfirstlane(kmax32);
                Kmin = __builtin_amdgcn_readfirstlane(kmin32);   // >= 2
            }
            if (Koct == 0)
                return;   // an octet of padding slots only: none in a consistent layout
                          // (each bin's last octet holds >= 1 entry), but Kmin - 1
                          // would bound the interior loop at 2^32 steps
            const uint32_t kt0 = Kmin - 1;   // first tail step (>= 1)
            const uint64_t safe = steps ? A : dummy;

            // loads: head, first two tail steps, first kPU interior steps
            const gu32x4* pb = gptr16(steps ? p0 : dummy);
            const uint64_t bstride = steps ? kStep / 16 : 0;
            auto ldf = [&](uint64_t k) -> u32x4 { return __builtin_nontemporal_load(pb + k * bstride); };
            auto ldt = [&](uint32_t k) -> u32x4 {   // tail step: lanes past E read a safe word
                const uint64_t a = p0 + uint64_t(k) * kStep;
                return load16(k < steps && a < E ? a : safe);
            };
            const u32x4 wh = ldf(0);
            const u32x4 wt0 = ldt(kt0);
            const u32x4 wt1 = ldt(kt0 + 1 < Koct ? kt0 + 1 : kt0);
            u32x4 Abuf[kPU], Bbuf[kPU];
#pragma unroll
            for (int j = 0; j < kPU; j++)
                Abuf[j] = ldf(1 + j < kt0 ? 1 + j : 0);
            // the stored checksum (records mode) behind the data loads; read at
            // the octet's end
            // (its two dwords are loaded here and joined at the octet's end:
            // joining them here would wait for every load above before the
            // previous octet's fold, exposing one memory latency per octet)
            typedef const __attribute__((address_space(1))) uint32_t g32s;
            uint32_t sw0 = 0u, sw1 = 0u;
            if (d.vstat && steps) {
                const uint64_t sa = (S - 4) & ~uint64_t(3);
                sw0 = *reinterpret_cast<g32s*>(sa);
                sw1 = *reinterpret_cast<g32s*>(sa + 4);
            }
            __builtin_amdgcn_sched_barrier(0);
            flush();

            uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0;
            auto stepf = [&](const u32x4& w) { op.apply4(lds, u0, u1, u2, u3, w); };
            // head: keep bytes >= S, inject init at S .. S+3 (masks and
            // v_perm selectors from the LDS table of the piece's offset)
            {
                const int off = int(uint32_t(S - A)) - 16 * gl;   // S - p0
                const int c = min(max(off, -4), 16) + 4;
                const u32x4* ht = reinterpret_cast<const u32x4*>(lds + kHeadOff) + 2 * c;
                const u32x4 m = ht[0], sl = ht[1];
                u32x4 w;
                w.x = (wh.x & m.x) ^ __builtin_amdgcn_perm(init, 0u, sl.x);
                w.y = (wh.y & m.y) ^ __builtin_amdgcn_perm(init, 0u, sl.y);
                w.z = (wh.z & m.z) ^ __builtin_amdgcn_perm(init, 0u, sl.z);
                w.w = (wh.w & m.w) ^ __builtin_amdgcn_perm(init, 0u, sl.w);
                stepf(w);
            }
            // interior
            uint32_t k = 1;
            for (; k + 2 * kPU <= kt0; k += 2 * kPU) {
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    Bbuf[j] = ldf(k + kPU + j);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    stepf(Abuf[j]);
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    Abuf[j] = ldf(k + 2 * kPU + j < kt0 ? k + 2 * kPU + j : 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    stepf(Bbuf[j]);
            }
#pragma unroll
            for (int j = 0; j < kPU; j++)
                if (k + j < kt0)
                    stepf(Abuf[j]);
            if (k + kPU < kt0) {
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    Bbuf[j] = ldf(k + kPU + j < kt0 ? k + kPU + j : 0);
#pragma unroll
                for (int j = 0; j < kPU; j++)
                    if (k + kPU + j < kt0)
                        stepf(Bbuf[j]);
            }
            // tail: keep bytes < E (masks from the LDS table of the bytes
            // left).  Every entry of the octet is live at step kt0; at
            // kt0 + 1 the ones that have ended take one more step of zeros
            // (no select: their padding grows by 128 bytes, < 256); the
            // ragged steps of log-scale bins freeze ended entries.
            const uint64_t trel64 = E - (p0 + uint64_t(kt0) * kStep);   // > 0 for live lanes
            const int trel = int(trel64 > 1024 && int64_t(trel64) > 0 ? 1024 : int64_t(trel64));
            const u32x4* tt = reinterpret_cast<const u32x4*>(lds + kTailOff);
            auto stepm = [&](u32x4 w, int de) {
                const u32x4 m = tt[min(max(de, 0), 16)];
                w.x &= m.x;
                w.y &= m.y;
                w.z &= m.z;
                w.w &= m.w;
                stepf(w);
            };
            stepm(wt0, trel);
            uint32_t eff = steps;   // steps the group ran for this entry
            if (kt0 + 1 < Koct) {
                stepm(wt1, trel - int(kStep));
                eff = steps > kt0 + 2 ? steps : kt0 + 2;
            }
            const int64_t erel = int64_t(E - p0);
            for (uint32_t kk = kt0 + 2; kk < Koct; kk++) {   // ragged octets (log-scale bins)
                const int64_t de64 = erel - int64_t(kk) * int64_t(kStep);
                const uint32_t p0v = u0, p1v = u1, p2v = u2, p3v = u3;
                stepm(ldt(kk), int(de64 < 0 ? 0 : (de64 > 16 ? 16 : de64)));
                const bool live = kk < steps;
                u0 = live ? u0 : p0v;
                u1 = live ? u1 : p1v;
                u2 = live ? u2 : p2v;
                u3 = live ? u3 : p3v;
            }

            pend = true;
            pu0 = u0;
            pu1 = u1;
            pu2 = u2;
            pu3 = u3;
            ppad = uint32_t((A + uint64_t(eff) * kStep) - E);
            pix = ix;
            pst = __builtin_amdgcn_alignbyte(sw1, sw0, uint32_t(S - 4) & 3);
    };

    // Work split.  Waves given equal shares of the long bins finish in the
    // order they were created (phase stamps, tools/stamps.py, 1M x 4 KiB:
    // the four oldest waves of a workgroup -- one per SIMD -- end at 564 us,
    // the next four at 588, then 617, the youngest four at 657: each SIMD
    // issues by age).  Each workgroup's share is therefore split among its
    // waves by age rank (slot / 4): older waves get age_weight(rank) / 2000 of
    // an equal share.  The octets of a wave's range form one stream: the next
    // octet's descriptor is always fetched one octet ahead, across bin
    // boundaries too.  (Taking part of the share from a counter instead -- one
    // LDS counter per workgroup or one device counter -- cost 1.6-2.7x, about
    // 1-2 us per chunk; DESIGN.md section 5.4, profiles/r03/long.)
    if constexpr (kSmall) {
        run(I0 + T * wave / nwaves, I0 + T * (wave + 1) / nwaves);
    } else {
        const uint64_t P0 = I0 + T * blk / nblk, PT = I0 + T * (blk + 1) / nblk - P0;
        const uint32_t slot = __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
        // cumulative weight of the slots before `slot` (4 slots per age rank)
        const int skew = d.vstat ? kAgeSkewRec : kAgeSkew;
        auto cum = [&](uint32_t sl) -> uint64_t {
            uint64_t c = 0;
#pragma unroll
            for (uint32_t r = 0; r < kEntWaves / 4; r++) {
                const uint32_t n = sl > 4 * r ? (sl - 4 * r < 4 ? sl - 4 * r : 4) : 0;
                c += uint64_t(n) * age_weight(r, skew);
            }
            return c;
        };
        const uint64_t tot = cum(kEntWaves);
        const uint64_t rlo = P0 + PT * cum(slot) / tot, rhi = P0 + PT * cum(slot + 1) / tot;
        struct Pos {
            int b;
            uint64_t o, ob, sb;
        };
        // first octet of [rlo, rhi) in bins >= bs
        auto seek = [&](int bs, Pos& p) -> bool {
            for (int b = bs; b < b1; b++) {
                const uint64_t ib = s_items[b], ie = s_items[b + 1];
                if (ie <= rlo || ib == ie)
                    continue;
                if (ib >= rhi)
                    return false;
                const uint64_t cost = s_cost[b];
                const uint64_t oa = ((rlo > ib ? rlo : ib) - ib + cost - 1) / cost;
                const uint64_t ob = ((rhi < ie ? rhi : ie) - ib + cost - 1) / cost;
                if (oa >= ob)
                    continue;
                p.b = b;
                p.o = oa;
                p.ob = ob;
                p.sb = s_start[b];
                return true;
            }
            return false;
        };
        // the octet after p: in its bin, else the first of the next bins
        auto advance = [&](Pos& p) -> bool {
            if (p.o + 1 < p.ob) {
                p.o++;
                return true;
            }
            return seek(p.b + 1, p);
        };
        Pos cur;
        bool have = seek(b0, cur);
        u32x4 nd = {0u, 0u, 0u, 0u};
        uint32_t nix = kNoIdx, ninit = 0xFFFFFFFFu;
        auto fetch = [&](const Pos& p) {
            const uint64_t sl = p.sb + p.o * kG + g;
            nd = so.desc[sl];
            nix = so.idx[sl];
            if (d.init)
                ninit = so.init[sl];
        };
        if (have)
            fetch(cur);
        while (have) {
            const u32x4 dd = nd;
            const uint32_t ix = nix, init = ninit;
            const int b = cur.b;
            Pos nxt = cur;
            have = advance(nxt);
            if (have)   // prefetch the next octet's descriptor
                fetch(nxt);
            octet(dd, ix, init, b);
            cur = nxt;
        }
    }
    flush();
    if (nb)
        flush_batch();
}

// The long-phase tables into the LDS, then the short and the long bins over
// workgroups blk of nblk.  Refuses (status bits) on an inconsistent layout.
__device__ __forceinline__ void long_phase(const BatchDesc& d, const Sorted& so, uint8_t* lds, bool bad,
                                           uint32_t blk, uint32_t nblk)
{
    fill_long(lds);
    uint64_t* s_items = reinterpret_cast<uint64_t*>(lds + kBinOff);   // kNB + 1
    uint64_t* s_start = s_items + (kNB + 1);                          // kNB
    uint32_t* s_cost = reinterpret_cast<uint32_t*>(s_start + kNB);    // kNB
    for (int t = threadIdx.x; t <= kNB; t += blockDim.x) {
        s_items[t] = so.bt->items[t];
        if (t < kNB) {
            s_start[t] = so.bt->start[t];
            s_cost[t] = uint32_t(so.bt->kcost[t]);
        }
    }
    if (__syncthreads_or(bad)) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicOr(so.status, kStatusSticky | kStatusBins);
        return;
    }
    RAMCRC_STAMP(2);
    entries_run<true>(d, so, lds, blk, nblk);
    RAMCRC_STAMP(3);
    entries_run<false>(d, so, lds, blk, nblk);
    RAMCRC_STAMP(4);
}

// Both phases in one launch (one LDS fill, one launch boundary): the exact
// short bins, then the pipelined long bins.  The phases are separate inlined
// loops, so the long-entry loop's registers are not shared with the short one.
__global__ __launch_bounds__(kEntWaves * kWaveSize, 1) void k_entries(BatchDesc d, Sorted so)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsEntries];
    // Every bin must hold exactly the entries the scatter placed in it
    // (cursor == count): then every sorted slot this launch reads was written
    // by this sequence.  Checked at the first barrier of each phase, before
    // any slot's contents are used; a mismatch refuses the launch (no output
    // written, status bits kStatusSticky | kStatusBins, RAMCRC_EINTERNAL from
    // ramcrc_ctx_check) instead of walking stale slots.
    const bool bad = threadIdx.x < kNB &&
                     so.bt->ctr[so.par].cursor[threadIdx.x] != so.bt->count[threadIdx.x];
    auto refuse = [&]() {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicOr(so.status, kStatusSticky | kStatusBins);
    };
    RAMCRC_STAMP(0);
    const bool have_tk = kTinyK >= 2 && !so.bt->direct_n &&
                         (so.bt->direct_multi || so.bt->start[kTinyK + 1] != so.bt->start[2]);
    // Role split: when a batch has both tiny and long
    // entries, workgroups < T run only the tiny phases (filling only their
    // table) and the others only the long phase, so the two overlap and no
    // workgroup waits for its slowest tiny wave before refilling its LDS.  T
    // follows the work: a tiny window costs kSplitKappa / 1024 long-phase work
    // units.  T = 0: both phases on every workgroup, in sequence -- also the
    // only choice for a grid of one workgroup (a context sized for one CU),
    // where a split of T = 1 left nobody for the long phase: its entries'
    // outputs were never written, with no error.
    uint32_t T = 0;
    constexpr int kT = kTinyK > kSmallK ? kTinyK : kSmallK;
    if (gridDim.x > 1 && !so.bt->direct_n && so.bt->start[kTinyK + 1] != so.bt->start[0] &&
        so.bt->items[kNB] != so.bt->items[kT + 1]) {
        uint64_t win = so.bt->start[2] - so.bt->start[0];   // one window each
        for (int b = 2; b <= kTinyK; b++)
            win += (so.bt->start[b + 1] - so.bt->start[b]) * uint64_t(b);
        const uint64_t ct = win * kSplitKappa / 1024, cl = so.bt->items[kNB] - so.bt->items[kT + 1];
        T = uint32_t((uint64_t(gridDim.x) * ct + (ct + cl) / 2) / (ct + cl));
        T = T < 1 ? 1 : (T > gridDim.x - 1 ? gridDim.x - 1 : T);
    }
    const bool do_tiny = T == 0 || blockIdx.x < T, do_long = T == 0 || blockIdx.x >= T;
    const uint32_t tn = T ? T : gridDim.x;
    bool tiny_ok = true;
    if (do_tiny) {
        // records (replay) keep the register prefetch: without it their
        // tiny phase measured 3-4 % slower; table batches 5-7 % faster
        tiny_ok = d.rec != nullptr
                      ? tiny_run_cf<true>(d, so, lds, bad, blockIdx.x, tn, have_tk)
                      : tiny_run_cf<false>(d, so, lds, bad, blockIdx.x, tn, have_tk);
        if (tiny_ok && have_tk)
            tiny_multi(d, so, lds, blockIdx.x, tn);
    }
    RAMCRC_STAMP(1);
    if (!tiny_ok) {
        refuse();
        return;
    }
    if (!do_long)
        return;
    if (so.bt->items[2] == so.bt->items[kNB]) {   // every entry is tiny (or large on the batch path)
        if (__syncthreads_or(bad))
            refuse();
        return;
    }
    // the position table is dead (when this workgroup ran the tiny phases)
    __syncthreads();
    long_phase(d, so, lds, bad, blockIdx.x - T, gridDim.x - T);
}


}  // namespace
