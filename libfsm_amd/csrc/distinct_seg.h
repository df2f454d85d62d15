/*
 * distinct_seg.h -- the arithmetic of the distinct records of a packed text (distinct.hip): no HIP header, so that
 * tests/c/test_distinct_seg.cpp checks it on the CPU against std::map.  Not part of the C ABI.
 *
 * The KEY of a record is its trimmed bytes and, where tags are given, its tag (include/fsm_hip.h, "distinct").
 *   Length.  With trim >= 0 a non-empty record whose last byte is the trim byte is one byte shorter; at most one byte goes.
 *   Chunks.  A key of len bytes is ceil(len / 16) chunks of two 64-bit words, little endian; the bytes of the last chunk behind
 *   the key read as 0 (dst_mask_lo / dst_mask_hi).
 *   Hash.  ONE definition: every chunk i gives dst_chunk_hash(lo, hi, i), the chunks' values are ADDED (mod 2^64), and
 *   dst_hash_finish mixes the sum with the length and the tag.  Addition commutes, so a lane that goes chunk by chunk and a
 *   wavefront whose lanes take strided chunks and add their partial sums get the same word, however the chunks are split.
 *   Table.  dst_table_slots(R) slots, a power of two >= 2 R and >= 16: open addressing, linear probing, never more than half full.
 *   A slot is one word, tag32(hash) << 32 | r; DST_EMPTY (all ones) is no record's, because r <= 2^32 - 2.  Words with one tag
 *   order as their r do, so the minimum of the words of equal keys is the word of the lowest r.
 *   Probe.  A chain starts at dst_probe_start(hash, slots) and goes on by dst_probe_next, which wraps.
 *   Weak hash (FSM_HIP_DISTINCT_WEAK_HASH, for tests): dst_weak_hash(len, slots) puts every chain's start into one of the LAST
 *   four slots, by len & 3, and gives all keys of one len & 3 one tag: chains, equal tags with different bytes, and the wrap happen
 *   on a handful of records.
 * Everything is unsigned and may wrap.
 */
#ifndef FSMHIP_CSRC_DISTINCT_SEG_H
#define FSMHIP_CSRC_DISTINCT_SEG_H

#include <cstdint>

#ifdef __HIPCC__
#define FSMHIP_DST_FN __host__ __device__ inline
#else
#define FSMHIP_DST_FN inline
#endif

namespace fsmhip {

constexpr uint64_t DST_EMPTY = ~(uint64_t)0;
constexpr uint64_t DST_MAX_RECORDS = 0xfffffffeull;       /* R <= 2^32 - 2: r <= 2^32 - 3, so no slot word is DST_EMPTY */
constexpr uint64_t DST_MIN_SLOTS = 16;
constexpr uint32_t DST_CHUNK = 16;
constexpr uint64_t DST_GOLD = 0x9e3779b97f4a7c15ull;

/* the bytes of the key of a record of `raw` bytes whose last byte is `last` (not looked at when raw == 0) */
FSMHIP_DST_FN uint64_t dst_trimmed(uint64_t raw, uint32_t last, int trim)
{
	return raw != 0u && trim >= 0 && last == ((uint32_t)trim & 0xffu) ? raw - 1u : raw;
}

/* the chunks of a key */
FSMHIP_DST_FN uint64_t dst_chunks(uint64_t len) { return len / DST_CHUNK + (len % DST_CHUNK != 0u ? 1u : 0u); }

/* the key's bytes in chunk i: 1 .. 16 for i < dst_chunks(len) */
FSMHIP_DST_FN uint32_t dst_chunk_bytes(uint64_t len, uint64_t i)
{
	const uint64_t left = len - i * DST_CHUNK;
	return left < DST_CHUNK ? (uint32_t)left : DST_CHUNK;
}

/* the masks of a chunk's two words of which n bytes (0 .. 16) belong to the key */
FSMHIP_DST_FN uint64_t dst_mask_lo(uint32_t n) { return n >= 8u ? ~(uint64_t)0 : ((uint64_t)1 << (8u * n)) - 1u; }
FSMHIP_DST_FN uint64_t dst_mask_hi(uint32_t n) { return n <= 8u ? 0u : dst_mask_lo(n - 8u); }

/* two chunks are equal in their first n bytes */
FSMHIP_DST_FN bool dst_chunk_equal(uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi, uint32_t n)
{
	return (((alo ^ blo) & dst_mask_lo(n)) | ((ahi ^ bhi) & dst_mask_hi(n))) == 0u;
}

FSMHIP_DST_FN uint64_t dst_mix(uint64_t x)
{
	x ^= x >> 30;
	x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27;
	x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return x;
}

/* what chunk i (its words masked) adds to the sum */
FSMHIP_DST_FN uint64_t dst_chunk_hash(uint64_t lo, uint64_t hi, uint64_t i)
{
	const uint64_t a = dst_mix(lo ^ ((2u * i + 1u) * DST_GOLD));
	const uint64_t b = dst_mix(hi ^ ((2u * i + 2u) * DST_GOLD));
	return a + ((b << 23) | (b >> 41));
}

/* the hash of a key from the sum over its chunks; tag 0 where no tags are given */
FSMHIP_DST_FN uint64_t dst_hash_finish(uint64_t sum, uint64_t len, uint32_t tag)
{
	return dst_mix(sum ^ dst_mix(len * DST_GOLD + tag));
}

FSMHIP_DST_FN uint64_t dst_table_slots(uint64_t R)
{
	uint64_t s = DST_MIN_SLOTS;
	while (s < 2u * R) s <<= 1;          /* R <= 2^32 - 2: at most 2^33 */
	return s;
}

/* (slots <= 2^33: the start is the low bits, len & 3 the top two, so the tag depends on len & 3 alone) */
FSMHIP_DST_FN uint64_t dst_weak_hash(uint64_t len, uint64_t slots) { return (len & 3u) << 62 | (slots - 4u + (len & 3u)); }

FSMHIP_DST_FN uint64_t dst_slot_word(uint64_t hash, uint64_t r) { return (hash >> 32) << 32 | (r & 0xffffffffu); }
FSMHIP_DST_FN uint32_t dst_slot_record(uint64_t word) { return (uint32_t)word; }
FSMHIP_DST_FN bool dst_same_tag(uint64_t a, uint64_t b) { return (a >> 32) == (b >> 32); }

FSMHIP_DST_FN uint64_t dst_probe_start(uint64_t hash, uint64_t slots) { return hash & (slots - 1u); }
FSMHIP_DST_FN uint64_t dst_probe_next(uint64_t i, uint64_t slots) { return (i + 1u) & (slots - 1u); }

}

#endif
