// MurmurHash3 x64-128 (Austin Appleby's public-domain definition), the hash
// behind RAMCloud's Key::getHash (src/Key.cc:140-151): the key bytes hashed
// with the low 32 bits of the table id as the seed, first 64-bit output word.
// Shared by host and device code, written from the definition; nothing is
// copied from the reference.
//
// The definition, for a message of n bytes and a 32-bit seed:
//     h1 = h2 = seed
//     for every full 16-byte block (k1, k2 little-endian 64-bit words):
//         h1 ^= rotl(k1 * c1, 31) * c2;  h1 = (rotl(h1, 27) + h2) * 5 + n1
//         h2 ^= rotl(k2 * c2, 33) * c1;  h2 = (rotl(h2, 31) + h1) * 5 + n2
//     the last n % 16 bytes, zero-extended to (k1, k2):
//         h2 ^= rotl(k2 * c2, 33) * c1   (only when more than 8 bytes are left)
//         h1 ^= rotl(k1 * c1, 31) * c2   (only when any byte is left)
//     h1 ^= n; h2 ^= n; h1 += h2; h2 += h1
//     h1 = fmix(h1); h2 = fmix(h2); h1 += h2            (h2 += h1: second word)
// The state is fed block by block (Murmur3::block, ::finish), so the device
// can hand it words it assembled from aligned loads.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RAMCRC_MM_HD __host__ __device__
#else
#define RAMCRC_MM_HD
#endif

namespace ramcrc {

constexpr uint64_t kMurmurC1 = 0x87c37b91114253d5ull;
constexpr uint64_t kMurmurC2 = 0x4cf5ad432745937full;
constexpr uint64_t kMurmurN1 = 0x52dce729ull;
constexpr uint64_t kMurmurN2 = 0x38495ab5ull;
constexpr uint64_t kMurmurF1 = 0xff51afd7ed558ccdull;
constexpr uint64_t kMurmurF2 = 0xc4ceb9fe1a85ec53ull;

RAMCRC_MM_HD constexpr uint64_t murmur_rotl(uint64_t v, int r)
{
    return (v << r) | (v >> (64 - r));
}

RAMCRC_MM_HD constexpr uint64_t murmur_fmix(uint64_t k)
{
    k ^= k >> 33;
    k *= kMurmurF1;
    k ^= k >> 33;
    k *= kMurmurF2;
    k ^= k >> 33;
    return k;
}

struct Murmur3 {
    uint64_t h1, h2;

    RAMCRC_MM_HD constexpr explicit Murmur3(uint32_t seed) : h1(seed), h2(seed) {}

    RAMCRC_MM_HD constexpr void mix1(uint64_t k1)
    {
        h1 ^= murmur_rotl(k1 * kMurmurC1, 31) * kMurmurC2;
    }
    RAMCRC_MM_HD constexpr void mix2(uint64_t k2)
    {
        h2 ^= murmur_rotl(k2 * kMurmurC2, 33) * kMurmurC1;
    }

    // one full 16-byte block
    RAMCRC_MM_HD constexpr void block(uint64_t k1, uint64_t k2)
    {
        mix1(k1);
        h1 = (murmur_rotl(h1, 27) + h2) * 5 + kMurmurN1;
        mix2(k2);
        h2 = (murmur_rotl(h2, 31) + h1) * 5 + kMurmurN2;
    }

    // The last `tail` (0..15) bytes in the low bytes of (k1, k2), every byte
    // past them zero, and the message length; returns the first output word.
    RAMCRC_MM_HD constexpr uint64_t finish(uint64_t k1, uint64_t k2, uint32_t tail, uint64_t len)
    {
        if (tail > 8)
            mix2(k2);
        if (tail > 0)
            mix1(k1);
        h1 ^= len;
        h2 ^= len;
        h1 += h2;
        h2 += h1;
        return murmur_fmix(h1) + murmur_fmix(h2);
    }
};

// The low `n` (0..8) bytes of w.
RAMCRC_MM_HD constexpr uint64_t murmur_low_bytes(uint64_t w, uint32_t n)
{
    return n >= 8 ? w : w & ((1ull << (8 * n)) - 1);
}

template <typename Byte>
RAMCRC_MM_HD constexpr uint64_t murmur_le64(const Byte* p, uint64_t n)
{
    uint64_t w = 0;
    for (uint64_t i = 0; i < n && i < 8; i++)
        w |= uint64_t(uint8_t(p[i])) << (8 * i);
    return w;
}

// Key::getHash over bytes in addressable memory (the host form; the
// compile-time known answers below).
template <typename Byte>
RAMCRC_MM_HD constexpr uint64_t key_hash(uint64_t table_id, const Byte* key, uint64_t len)
{
    Murmur3 m{uint32_t(table_id)};
    uint64_t i = 0;
    for (; i + 16 <= len; i += 16)
        m.block(murmur_le64(key + i, 8), murmur_le64(key + i + 8, 8));
    const uint32_t tail = uint32_t(len - i);
    const uint64_t k1 = murmur_le64(key + i, tail);
    const uint64_t k2 = tail > 8 ? murmur_le64(key + i + 8, tail - 8) : 0;
    return m.finish(k1, k2, tail, len);
}

// Known answers the reference's own tests hold: Key(82, "hey-hey-hey", 12)
// (src/KeyTest.cc:95-101; the 12th byte is the string's NUL) and the hashes of
// (1, "1") and (1, "2") that src/RecoverySegmentBuilderTest.cc:246-268 prints.
static_assert(key_hash(82, "hey-hey-hey", 12) == 0x889d47d556739eebull, "MurmurHash3 x64-128");
static_assert(key_hash(1, "1", 1) == 0xDD5D9F7F60D5B056ull, "MurmurHash3 x64-128");
static_assert(key_hash(1, "2", 1) == 0x3554F985FBED3C16ull, "MurmurHash3 x64-128");

}  // namespace ramcrc
