// Geometry, device tables, LDS layouts, table operators, batch descriptors.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {


constexpr int kWaveSize = 64;
constexpr int kWavesPerGroup = 16;                 // 1024-thread workgroups, 1 per CU
constexpr int kThreads = kWaveSize * kWavesPerGroup;
constexpr uint32_t kBlock = 1024;                  // bytes per wave step
#ifndef RAMCRC_CHUNK_SHIFT
#define RAMCRC_CHUNK_SHIFT 18
#endif
#ifndef RAMCRC_UNROLL
#define RAMCRC_UNROLL 4
#endif
constexpr int kChunkShift = RAMCRC_CHUNK_SHIFT;
constexpr uint64_t kChunk = 1ull << kChunkShift;   // 256 KiB per wave work item
constexpr uint64_t kLargeMin = 64 * 1024;          // batch API threshold
constexpr uint64_t kWideCombineMin = 16384;        // tables above: k_combine<kWide>
constexpr int kUnroll = RAMCRC_UNROLL;             // blocks per register group (x2 in flight)

// ------------------------------------------------------------------ tables
struct alignas(16) DeviceTables {
    OpTable stride_large;   // X^1024: Horner step of k_chunks
    OpTable stride_small;   // X^128:  Horner step of k_entries (8 lanes x 16 B)
    OpTable comb[7];        // X^4, X^16, X^32, X^64, X^128, X^256, X^512
    ramcrc::ByteTable t0;   // X^1 byte step
    uint32_t xblk[4][256];  // x^(8 * 1024 * b * 256^j)
    uint32_t xinv[1024];    // x^(-8 p)
    uint32_t pos[132][256]; // k_entries, tiny phase: row r = X^(r-3)(byte), rows 0..3 (m <= 0) zero
    uint32_t xmeta[5 * 64 + 1];   // k_seg_walk: x^(8d), d = 0 .. 320 (one batch of metadata)
    uint32_t xbyte[4][256];       // x^(8 * b * 256^j): x^(8d) for any 32-bit d in 4 factors
    // Bases the tiny phase builds its LDS tables from (tiny_fill_build):
    // twb[q][k] = X^(128 - q)(1 << k), twib[j][k] = X^-128(1 << (8 j + k))
    alignas(16) uint32_t twb[128][8];
    alignas(16) uint32_t twib[4][8];
    // k_entries' long phase (group_fold, flush_batch, head and tail steps),
    // laid out as in LDS from kX4Off on, so one fill copies them all:
    struct alignas(16) LongTabs {
        OpTable x4, x16, x32, x64;        // group_fold
        OpTable x8;                       // X^8, the in-lane fold's second level
        uint32_t xinv4[256];              // x^(-8 (p - 4)): unpad by p, the fold's X^4 folded in
        uint32_t headtab[21][8];          // c = S - piece + 4 (0..20): 4 keep masks, 4 init selectors
        uint32_t tailtab[17][4];          // bytes d (0..16) of the piece below E: 4 keep masks
    } lt;
};

constexpr DeviceTables make_device_tables()
{
    DeviceTables t{};
    t.stride_large = ramcrc::make_op(kBlock);
    t.stride_small = ramcrc::make_op(128);
    const uint64_t comb_d[7] = {4, 16, 32, 64, 128, 256, 512};
    for (int i = 0; i < 7; i++)
        t.comb[i] = ramcrc::make_op(comb_d[i]);
    t.t0 = ramcrc::make_byte_table();
    for (int j = 0; j < 4; j++) {
        const uint32_t base = ramcrc::xpow8(uint64_t(kBlock) << (8 * j));
        uint32_t acc = ramcrc::kOne;
        for (int b = 0; b < 256; b++) {
            t.xblk[j][b] = acc;
            acc = ramcrc::mulmod(acc, base);
        }
    }
    const uint32_t inv8 = ramcrc::xinv8pow(1);
    uint32_t acc = ramcrc::kOne;
    for (int p = 0; p < 1024; p++) {
        t.xinv[p] = acc;
        acc = ramcrc::mulmod(acc, inv8);
    }
    for (int m = 1; m <= 128; m++) {
        const uint32_t c = ramcrc::xpow8(uint64_t(m));
        for (uint32_t b = 0; b < 256; b++)
            t.pos[m + 3][b] = ramcrc::mulmod(b, c);
    }
    for (int d = 0; d <= 5 * 64; d++)
        t.xmeta[d] = ramcrc::xpow8(uint64_t(d));
    for (int j = 0; j < 4; j++) {
        const uint32_t base = ramcrc::xpow8(uint64_t(1) << (8 * j));
        uint32_t acc = ramcrc::kOne;
        for (int b = 0; b < 256; b++) {
            t.xbyte[j][b] = acc;
            acc = ramcrc::mulmod(acc, base);
        }
    }
    {
        // X^-128 (a window sum moved back from the window end): only its
        // basis words go to the device
        OpTable xinv128{};
        const uint32_t c = ramcrc::xinv8pow(128);
        for (int k = 0; k < 4; k++)
            for (uint32_t b = 0; b < 256; b++)
                xinv128.t[k][b] = ramcrc::mulmod(b << (8 * k), c);
        for (int k = 0; k < 4; k++)
            for (int j = 0; j < 8; j++)
                t.twib[k][j] = xinv128.t[k][1u << j];
    }
    for (int q = 0; q < 128; q++) {
        const uint32_t c = ramcrc::xpow8(uint64_t(128 - q));
        for (int j = 0; j < 8; j++)
            t.twb[q][j] = ramcrc::mulmod(1u << j, c);
    }
    t.lt.x4 = t.comb[0];
    t.lt.x16 = t.comb[1];
    t.lt.x32 = t.comb[2];
    t.lt.x64 = t.comb[3];
    t.lt.x8 = ramcrc::make_op(8);
    for (int p = 0; p < 256; p++)   // x^(-8 (p - 4)) = x^(-8 p) * x^32
        t.lt.xinv4[p] = ramcrc::mulmod(t.xinv[p], ramcrc::xpow8(4));
    for (int c = 0; c <= 20; c++) {   // c = clamp(S - piece, -4, 16) + 4
        const int off = c - 4;
        for (int j = 0; j < 4; j++) {
            uint32_t m = 0, sel = 0;
            for (int q = 0; q < 4; q++) {
                const int b = 4 * j + q, r = b - off;   // init byte r lands on piece byte b
                m |= uint32_t(b >= off ? 0xFF : 0) << (8 * q);
                // v_perm_b32(init, 0, sel): 4 + r picks init byte r, 0x0C yields 0
                sel |= uint32_t(r >= 0 && r < 4 ? 4 + r : 0x0C) << (8 * q);
            }
            t.lt.headtab[c][j] = m;
            t.lt.headtab[c][4 + j] = sel;
        }
    }
    for (int d = 0; d <= 16; d++)
        for (int j = 0; j < 4; j++) {
            const int k = d - 4 * j < 0 ? 0 : (d - 4 * j > 4 ? 4 : d - 4 * j);
            t.lt.tailtab[d][j] = k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u;
        }
    return t;
}

__device__ const DeviceTables g_tab = make_device_tables();

// Compile-time self-checks of the algebra the kernels rely on.
static_assert(ramcrc::mulmod(ramcrc::kXInv, 0x40000000u) == ramcrc::kOne, "x * x^-1 != 1");
static_assert(ramcrc::mulmod(ramcrc::xpow8(3), ramcrc::xinv8pow(3)) == ramcrc::kOne,
              "x^24 * x^-24 != 1");

// --------------------------------------------------------- LDS layouts
// Replicated stride tables (both kernels): 128 KiB.
//   byte address = region*65536 + b*256 + (k&1)*128 + (lane&31)*4
//   region = k>>1, b = byte value, k = which byte of u (0..3)
// so ds_read_b32 of lane l always lands in bank l%32.
constexpr uint32_t kRepBytes = 131072;
constexpr uint32_t kCombOff = kRepBytes;                  // k_chunks: 7 x 4 KiB
constexpr uint32_t kLdsChunks = kCombOff + 7 * 4096;      // 159744 B
constexpr uint32_t kX4Off = kRepBytes;                    // k_entries: X^4,16,32,64 (16 KiB)
constexpr uint32_t kX8Off = kX4Off + 4 * 4096;            // k_entries: X^8 (4 KiB)
constexpr uint32_t kXinvOff = kX8Off + 4096;              // k_entries: x^(-8 (pad - 4)) (1 KiB)
constexpr uint32_t kHeadOff = kXinvOff + 1024;            // k_entries: head masks/selectors (672 B)
constexpr uint32_t kTailOff = kHeadOff + 21 * 32;         // k_entries: tail masks (272 B)
constexpr uint32_t kBinOff = kTailOff + 17 * 16;          // k_entries: bin table (4 KiB)
constexpr uint32_t kLdsEntries = kBinOff + 4096;          // 157616 B
static_assert(kBinOff % 16 == 0, "LDS table alignment");
static_assert(kBinOff - kX4Off == sizeof(DeviceTables::LongTabs), "long-phase tables: LDS = g_tab.lt");
static_assert(kLdsEntries <= 160 * 1024, "LDS budget");
static_assert(kLdsChunks <= 160 * 1024, "LDS budget");
#define RAMCRC_LDS_CHUNKS 159744    // reported by ramcrc_build_info
#define RAMCRC_LDS_ENTRIES 157616
static_assert(kLdsChunks == RAMCRC_LDS_CHUNKS && kLdsEntries == RAMCRC_LDS_ENTRIES,
              "build_info LDS sizes");

// LDS table fills.  Every thread issues all of its global loads before its
// first LDS store, so a fill costs about one L2 round trip instead of one per
// loop iteration (a 129 KiB fill would otherwise serialise ~33 round trips).
__device__ __forceinline__ void fill_replicated(uint8_t* lds, const OpTable& op)
{
    // 4 tables x 256 entries x 32 replicas; each item writes 4 replicas (16
    // contiguous bytes): 8192 items.
    constexpr uint32_t kItems = 4 * 256 * 8;
    constexpr int kU = 8;
    for (uint32_t base = threadIdx.x; base < kItems; base += kU * blockDim.x) {
        uint32_t v[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const uint32_t idx = base + j * blockDim.x;
            const uint32_t ci = idx < kItems ? idx : 0;
            v[j] = op.t[ci >> 11][(ci >> 3) & 255];
        }
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const uint32_t idx = base + j * blockDim.x;
            if (idx < kItems) {
                const uint32_t k = idx >> 11, bv = (idx >> 3) & 255, q = idx & 7;
                const uint32_t off = (k >> 1) * 65536 + bv * 256 + (k & 1) * 128 + q * 16;
                *reinterpret_cast<uint4*>(lds + off) = make_uint4(v[j], v[j], v[j], v[j]);
            }
        }
    }
}

// k_entries' long-phase LDS: the replicated X^128 table and g_tab.lt, every
// global load issued before the first LDS store (one L2 round trip for the
// whole refill instead of one per table: 5.5 -> ~2 us per launch).
__device__ __forceinline__ void fill_long(uint8_t* lds);

// words % 4 == 0; src and lds + off 16-byte aligned.
__device__ __forceinline__ void fill_plain(uint8_t* lds, uint32_t off, const uint32_t* src,
                                           uint32_t words)
{
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* dst = reinterpret_cast<uint4*>(lds + off);
    const uint32_t n = words / 4;
    constexpr int kU = 9;
    for (uint32_t base = threadIdx.x; base < n; base += kU * blockDim.x) {
        uint4 v[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const uint32_t i = base + j * blockDim.x;
            v[j] = s[i < n ? i : 0];
        }
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const uint32_t i = base + j * blockDim.x;
            if (i < n)
                dst[i] = v[j];
        }
    }
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Per-lane constant for table k: [byte0 = bank offset (+128 for odd k),
// byte2 = region].
__device__ __forceinline__ uint32_t lane_reg(int k, int lane)
{
    return (uint32_t(k >> 1) << 16) | (uint32_t(k & 1) << 7) | (uint32_t(lane & 31) << 2);
}

// v_perm_b32 selector: dst.b0 = lanereg.b0, dst.b1 = u.byte(k), dst.b2 =
// lanereg.b2, dst.b3 = 0.  (sel 0-3 pick the 2nd operand's bytes, 4-7 the
// 1st operand's, 0x0C yields 0x00.)
template <int k>
__device__ __forceinline__ uint32_t rep_addr(uint32_t u, uint32_t lr)
{
    return __builtin_amdgcn_perm(u, lr, 0x0C020000u | ((4u + k) << 8));
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct RepOp {
    uint32_t lr0, lr1, lr2, lr3;
    __device__ explicit RepOp(int lane)
        : lr0(lane_reg(0, lane)), lr1(lane_reg(1, lane)), lr2(lane_reg(2, lane)),
          lr3(lane_reg(3, lane))
    {
    }
    // X^stride(u) ^ w through the replicated tables.  The four lookups are
    // consumed by two 3-input XORs, v_bitop3_b32 0x96 (inline asm so that hipcc waits once for all
    // four LDS reads instead of chaining 2-input XORs behind one wait each).
    __device__ __forceinline__ uint32_t apply(const uint8_t* lds, uint32_t u, uint32_t w) const
    {
        const uint32_t a = *reinterpret_cast<const uint32_t*>(lds + rep_addr<0>(u, lr0));
        const uint32_t b = *reinterpret_cast<const uint32_t*>(lds + rep_addr<1>(u, lr1));
        const uint32_t c = *reinterpret_cast<const uint32_t*>(lds + rep_addr<2>(u, lr2));
        const uint32_t d = *reinterpret_cast<const uint32_t*>(lds + rep_addr<3>(u, lr3));
        return xor3(xor3(a, b, w), c, d);
    }
    // One Horner step of the four word accumulators, issued as k_chunks' loop
    // runs it: the 16 table reads back to back, one wait, then the 8 XORs, so
    // a step costs one LDS round trip.  (Under k_entries' register pressure
    // hipcc otherwise interleaves the four lookup groups behind a wait each:
    // four round trips per step.)  The empty asm takes every read result at
    // once, so no XOR can be scheduled between the reads.
    __device__ __forceinline__ void apply4(const uint8_t* lds, uint32_t& u0, uint32_t& u1,
                                           uint32_t& u2, uint32_t& u3, const u32x4& w) const;
};

// X^d(v) through a plain (non-replicated) 4 KiB table at LDS byte offset off.
__device__ __forceinline__ uint32_t plain_apply(const uint8_t* lds, uint32_t off, uint32_t v)
{
    const uint32_t* t = reinterpret_cast<const uint32_t*>(lds + off);
    return t[v & 0xFF] ^ t[256 + ((v >> 8) & 0xFF)] ^ t[512 + ((v >> 16) & 0xFF)] ^
           t[768 + (v >> 24)];
}

__device__ __forceinline__ uint32_t mulmod_dev(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? ramcrc::kPoly : 0u);
    }
    return p;
}

// Same product, Horner over the bits of a (highest power first): one running
// register, for call sites where register pressure matters more than latency.
__device__ __forceinline__ uint32_t mulmod_horner(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const uint32_t ma = uint32_t(int32_t(a << (31 - j)) >> 31);   // coefficient of x^(31-j)
        const uint32_t mp = 0u - (p & 1u);
        p = (p >> 1) ^ (mp & ramcrc::kPoly) ^ (ma & b);
    }
    return p;
}

// x^(8 * 1024 * t) for t < 2^32 block units.
__device__ __forceinline__ uint32_t xpow_blocks(uint64_t t)
{
    uint32_t r = ramcrc::kOne;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = uint32_t(t >> (8 * j)) & 0xFF;
        if (b)
            r = (r == ramcrc::kOne) ? g_tab.xblk[j][b] : mulmod_dev(r, g_tab.xblk[j][b]);
    }
    return r;
}

// Mask a 4-byte word at absolute address a to the bytes inside [S, E) and XOR
// in the initial state at its byte position (bytes S..S+3).
__device__ __forceinline__ uint32_t fix_word(uint32_t w, uint64_t a, uint64_t S, uint64_t E,
                                             uint32_t init)
{
    // Branch-free.  ds/de: byte offsets of S and E from this word, clamped.
    const int64_t ds64 = int64_t(S - a), de64 = int64_t(E - a);
    const int ds = ds64 < -8 ? -8 : (ds64 > 8 ? 8 : int(ds64));
    const int de = de64 < -8 ? -8 : (de64 > 8 ? 8 : int(de64));
    const int lo = min(max(ds, 0), 4), hi = min(max(de, 0), 4);
    const uint32_t mhi = uint32_t((1ull << (8 * hi)) - 1);
    const uint32_t mlo = uint32_t((1ull << (8 * lo)) - 1);
    w &= mhi & ~mlo;
    // init occupies bytes S..S+3; word byte q holds init byte q - ds
    const int dd = -ds;   // a - S
    const uint32_t inj = uint32_t((uint64_t(init) << 24) >> (24 + 8 * (dd < -3 ? -3 : (dd > 3 ? 3 : dd))));
    return w ^ ((dd > -4 && dd < 4) ? inj : 0u);
}

// Wave-uniform 64-bit value into scalar registers.  (The builtin returns a
// signed int: each half goes through uint32_t, or the low half would
// sign-extend into the high one.)
__device__ __forceinline__ uint64_t rfl64(uint64_t v)
{
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(v)));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(v >> 32)));
    return (uint64_t(hi) << 32) | lo;
}

// Explicit global address space: generic (flat_*) loads would also count in
// lgkmcnt and serialise against the LDS table lookups.
typedef const __attribute__((address_space(1))) u32x4 gu32x4;
typedef const __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ const gu32x4* gptr16(uint64_t addr)
{
    return (const gu32x4*)addr;
}

__device__ __forceinline__ u32x4 load16(uint64_t addr) { return *gptr16(addr); }

// The 4 bytes at a (any alignment; a + 8 rounded down to 4 stays inside the
// buffer): two aligned dword loads and one byte funnel shift.
__device__ __forceinline__ uint32_t load_u32_any(uint64_t a)
{
    typedef const __attribute__((address_space(1))) uint32_t g32;
    const uint64_t b = a & ~uint64_t(3);
    const uint32_t w0 = *reinterpret_cast<g32*>(b), w1 = *reinterpret_cast<g32*>(b + 4);
    return __builtin_amdgcn_alignbyte(w1, w0, uint32_t(a) & 3);
}

__device__ __forceinline__ void RepOp::apply4(const uint8_t* lds, uint32_t& u0, uint32_t& u1,
                                              uint32_t& u2, uint32_t& u3, const u32x4& w) const
{
    auto rd = [&](uint32_t a) { return *reinterpret_cast<const uint32_t*>(lds + a); };
    uint32_t a0 = rd(rep_addr<0>(u0, lr0)), a1 = rd(rep_addr<1>(u0, lr1));
    uint32_t a2 = rd(rep_addr<2>(u0, lr2)), a3 = rd(rep_addr<3>(u0, lr3));
    uint32_t b0 = rd(rep_addr<0>(u1, lr0)), b1 = rd(rep_addr<1>(u1, lr1));
    uint32_t b2 = rd(rep_addr<2>(u1, lr2)), b3 = rd(rep_addr<3>(u1, lr3));
    uint32_t c0 = rd(rep_addr<0>(u2, lr0)), c1 = rd(rep_addr<1>(u2, lr1));
    uint32_t c2 = rd(rep_addr<2>(u2, lr2)), c3 = rd(rep_addr<3>(u2, lr3));
    uint32_t d0 = rd(rep_addr<0>(u3, lr0)), d1 = rd(rep_addr<1>(u3, lr1));
    uint32_t d2 = rd(rep_addr<2>(u3, lr2)), d3 = rd(rep_addr<3>(u3, lr3));
    asm volatile(""
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3),
                   "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));
    u0 = xor3(xor3(a0, a1, w.x), a2, a3);
    u1 = xor3(xor3(b0, b1, w.y), b2, b3);
    u2 = xor3(xor3(c0, c1, w.z), c2, c3);
    u3 = xor3(xor3(d0, d1, w.w), d2, d3);
}

// ------------------------------------------------------------ descriptors
struct BatchDesc {
    const uint8_t* base;     // d_base
    const uint64_t* off;     // general mode
    const uint64_t* len;     // general mode
    uint64_t seg_bytes;      // uniform mode; segment stride in record mode
    uint64_t n;              // buffers (record mode: table capacity)
    const uint32_t* init;    // nullable
    uint32_t* out;
    uint32_t flags;
    uint32_t cshift;         // log2 chunk bytes of this launch (k_chunks/k_combine)
    const u32x4* rec;        // record mode: ramcrc_seg_entry table
    const uint64_t* n_dev;   // record mode: live entry count (device), <= n
    const u32x4* seg_status; // record mode: ramcrc_seg_status per segment (walk result)
    ramcrc_seg_status* vstat; // record mode, nullable: k_entries compares each object's CRC
                              // with its stored checksum (the 4 bytes before S, loaded beside
                              // its head) and counts mismatches in vstat[segment].bad_objects
};

// Buffer addressing modes.
//   kSegAligned: segment i = base + i*seg_bytes, base and seg_bytes multiples
//                of the chunk size -> chunk g maps to (g / per, g % per).
//   kSegUniform: same geometry, any alignment -> goes through the plan.
//   kTable:      buffer i = base + off[i], len[i] -> goes through the plan.
//   kRecords:    buffer i = the object of segment-walk record i: bytes
//                [4, length) of its payload (Object::computeChecksum,
//                src/Object.cc:805-819).  Inactive: records that are not
//                objects, objects shorter than their header or running past
//                the segment (kRecOverlong), and every record of a segment
//                whose metadata check failed (RecoverySegmentBuilder::build
//                stops there, src/RecoverySegmentBuilder.cc:61-203).
//   kObjects:    buffer i = bytes [4, len[i]) of the serialized object at
//                base + off[i] (Object::computeChecksum on the write path,
//                Object::assembleForLog, src/Object.cc:213-238); objects
//                shorter than their 24-byte header are inactive.
enum Mode { kSegAligned = 0, kSegUniform = 1, kTable = 2, kRecords = 3, kObjects = 4 };

constexpr uint32_t kObjHeaderBytes = 24;     // Object::Header, src/Object.h:137-182
constexpr uint32_t kTombHeaderBytes = 32;    // ObjectTombstone::Header, src/Object.h:285-338
constexpr uint32_t kSafeVersionBytes = 12;   // ObjectSafeVersion::Header, src/Object.h:402-427
constexpr uint32_t kPrepHeaderBytes = 32;    // PreparedOp::Header, src/PreparedOp.h:63-100
constexpr uint32_t kPrepTombBytes = 44;      // PreparedOpTombstone::Header, src/PreparedOp.h:142-185
constexpr uint32_t kTxDecisionHeaderBytes = 48;  // TxDecisionRecord::Header, src/TxDecisionRecord.h:62-128
constexpr uint32_t kTxPlistHeaderBytes = 24;     // ParticipantList::Header, src/ParticipantList.h:81-113
constexpr uint32_t kRecOverlong = 0x100;   // record header bit: payload past the capacity

template <int kMode>
__device__ __forceinline__ uint64_t entry_count(const BatchDesc& d)
{
    if (kMode == kRecords) {
        const uint64_t live = *d.n_dev;
        return live < d.n ? live : d.n;
    }
    return d.n;
}

// Header bytes a record of `type` must hold to be checked; 0 = not checked.
// (a nibble per type of bytes / 4 in one 64-bit constant: branch-free, and
// it can never become a lookup table in memory on a per-record path)
constexpr uint64_t replay_header_nibbles()
{
    const uint32_t t[][2] = {{RAMCRC_LOG_ENTRY_TYPE_OBJ, kObjHeaderBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, kTombHeaderBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION, kSafeVersionBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_PREP, kPrepHeaderBytes + kObjHeaderBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_PREPTOMB, kPrepTombBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_TXDECISION, kTxDecisionHeaderBytes},
                             {RAMCRC_LOG_ENTRY_TYPE_TXPLIST, kTxPlistHeaderBytes}};
    uint64_t v = 0;
    for (const auto& e : t)
        v |= uint64_t(e[1] / 4) << (4 * e[0]);
    return v;
}
constexpr uint64_t kReplayHeaderNibbles = replay_header_nibbles();
static_assert(kObjHeaderBytes % 4 == 0 && kTombHeaderBytes % 4 == 0 && kSafeVersionBytes % 4 == 0 &&
                  kPrepTombBytes % 4 == 0 && kTxDecisionHeaderBytes % 4 == 0 && kTxPlistHeaderBytes % 4 == 0 &&
                  (kPrepHeaderBytes + kObjHeaderBytes) / 4 < 16 && kTxDecisionHeaderBytes / 4 < 16 &&
                  RAMCRC_LOG_ENTRY_TYPE_TXPLIST < 16,
              "replay header sizes: one nibble of bytes / 4 per type below 16");

__device__ __forceinline__ uint32_t replay_header_bytes(uint32_t type)
{
    return type < 16 ? 4 * uint32_t((kReplayHeaderNibbles >> (4 * type)) & 15) : 0u;
}

// The object bytes [S, E) of walk record r ({segment, offset, length,
// header}); false (S == E) unless it is an object of a segment that passed.
// (seg_st: the flags word of the record's segment status)
__device__ __forceinline__ bool record_range_st(const BatchDesc& d, const u32x4& r, uint32_t seg_st,
                                                uint64_t& S, uint64_t& E)
{
    const uint64_t payload = reinterpret_cast<uint64_t>(d.base) + uint64_t(r.x) * d.seg_bytes + r.y + 1 +
                             ((r.w >> 6) & 3) + 1;
    const bool obj = (r.w & (0x3f | kRecOverlong)) == RAMCRC_LOG_ENTRY_TYPE_OBJ && r.z >= kObjHeaderBytes &&
                     (seg_st & RAMCRC_SEG_OK);
    S = payload + 4;
    E = obj ? payload + r.z : S;
    return obj;
}

__device__ __forceinline__ bool record_range(const BatchDesc& d, const u32x4& r, uint64_t& S, uint64_t& E)
{
    return record_range_st(d, r, d.seg_status[r.x].x, S, E);
}

// [S, E) of buffer i; false for an inactive record (then S == E).
template <int kMode>
__device__ __forceinline__ bool buffer_range(const BatchDesc& d, uint64_t i, uint64_t& S,
                                             uint64_t& E)
{
    if (kMode == kRecords) {
        return record_range(d, d.rec[i], S, E);
    } else if (kMode == kObjects) {
        const uint64_t o = reinterpret_cast<uint64_t>(d.base) + d.off[i];
        const uint64_t L = d.len[i];
        S = o + 4;
        E = L >= kObjHeaderBytes ? o + L : S;
        return L >= kObjHeaderBytes;
    } else if (kMode != kTable) {
        S = reinterpret_cast<uint64_t>(d.base) + i * d.seg_bytes;
        E = S + d.seg_bytes;
    } else {
        S = reinterpret_cast<uint64_t>(d.base) + d.off[i];
        E = S + d.len[i];
    }
    return true;
}

__device__ __forceinline__ uint64_t chunk_count(uint64_t S, uint64_t E, uint32_t cshift)
{
    return ((E - 1) >> cshift) - (S >> cshift) + 1;
}

// Context status word (ramcrc_ctx_status / ramcrc_ctx_check).
constexpr uint32_t kStatusRefused = 1u;   // this launch's chunk plan overflowed (k_chunks)
constexpr uint32_t kStatusSticky = 2u;    // some launch wrote no outputs since the last check
constexpr uint32_t kStatusBins = 4u;      // a binned launch found its layout inconsistent

struct Plan {
    uint64_t* local;      // per entry: exclusive prefix of chunk counts within its group
    uint64_t* group_pref;  // per group of kThreads entries, exclusive prefix; [ngroups] = total
    uint64_t ngroups;
    uint32_t* partials;
    uint64_t partials_cap;
    uint32_t* status;      // bit 0: this launch's partials overflow; bit 1: sticky (ramcrc_ctx_check)
    const uint32_t* nlarge;       // nullable: large buffers counted by this sequence's
                                  // k_bin_count; 0 -> every plan kernel exits at once
};

__device__ __forceinline__ bool plan_empty(const Plan& pl) { return pl.nlarge && *pl.nlarge == 0; }

__device__ __forceinline__ bool is_large(uint64_t len) { return len >= kLargeMin; }


}  // namespace
