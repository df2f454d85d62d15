/*
 * sort_seg.h -- the arithmetic of the sort of a packed text's records (sort.hip): no HIP header, so that
 * tests/c/test_sort_seg.cpp runs the rounds sequentially on the CPU against std::stable_sort.  Not part of the C ABI.
 *
 * Keys order as memcmp does, a proper prefix before the longer key (include/fsm_hip.h, "sort").  A ROUND looks at eight key bytes
 * from a depth on:
 *   Word.  srt_word: the bytes depth .. depth + 7 of the key big endian, so that words order as the bytes do; the bytes behind
 *   the key read as 0 (srt_tail_mask on the little-endian load, then the swap).  srt_valid: how many of the eight exist, 0 .. 8.
 *   "ab" and "ab\0" have equal words and valid 2 and 3: the entry orders by (word, valid).
 *   Reverse.  Under FSM_HIP_SORT_REVERSE both are complemented (srt_sort_word, srt_sort_valid): the larger word first, and of
 *   equal words the longer key first.
 *   Prefix.  srt_common_chunk: the leading bytes two 16-byte chunks share, of the first n; a lane adds them up chunk by chunk
 *   and stops at the first chunk that is not shared whole.  srt_skip: the minimum over a bucket, rounded down to whole words.
 *   Digit.  An entry is sorted by (bucket, word, valid) with a least-significant-digit radix sort of SRT_DIGITS digits of eight
 *   bits: digit 0 is valid, 1 .. 8 the word from its low byte up, 9 .. 12 the bucket from its low byte up.
 *   Head.  A sorted entry opens a bucket when (bucket, word, valid) differs from its predecessor's.  A bucket goes on -- is ACTIVE
 *   -- while it has more than one member and its word was full (raw valid 8): srt_active, from the entry's and its successor's
 *   head flags.
 *   Rounds.  srt_rounds_bound(maxlen) = ceil(maxlen / 8) + 1: a round per word of the longest key and one for the word that
 *   shows that two keys of a whole number of words have ended.
 * Everything is unsigned.
 */
#ifndef FSMHIP_CSRC_SORT_SEG_H
#define FSMHIP_CSRC_SORT_SEG_H

#include <cstdint>

#ifdef __HIPCC__
#define FSMHIP_SRT_FN __host__ __device__ inline
#else
#define FSMHIP_SRT_FN inline
#endif

namespace fsmhip {

constexpr uint64_t SRT_MAX_RECORDS = 0xfffffffeull;       /* R <= 2^32 - 2, as the distinct records */
constexpr uint32_t SRT_WORD = 8;                          /* key bytes of a round */
constexpr uint32_t SRT_CHUNK = 16;                        /* key bytes of a step of the prefix comparison */
constexpr uint32_t SRT_DIGITS = 13;                       /* valid, eight of the word, four of the bucket */
constexpr uint32_t SRT_DIGIT_BUCKET = 9;                  /* the first digit of the bucket */
constexpr uint32_t SRT_BINS = 256;

/* the mask of the n (0 .. 8) low bytes of a little-endian word */
FSMHIP_SRT_FN uint64_t srt_tail_mask(uint32_t n) { return n >= 8u ? ~(uint64_t)0 : ((uint64_t)1 << (8u * n)) - 1u; }

FSMHIP_SRT_FN uint64_t srt_swap(uint64_t x)
{
	x = (x & 0x00ff00ff00ff00ffull) << 8 | (x >> 8 & 0x00ff00ff00ff00ffull);
	x = (x & 0x0000ffff0000ffffull) << 16 | (x >> 16 & 0x0000ffff0000ffffull);
	return x << 32 | x >> 32;
}

/* the key bytes that exist from `depth` on, at most eight */
FSMHIP_SRT_FN uint32_t srt_valid(uint64_t len, uint64_t depth)
{
	if (depth >= len) return 0u;
	return len - depth < SRT_WORD ? (uint32_t)(len - depth) : SRT_WORD;
}

/* the round's word from the eight bytes loaded little endian at the key's byte `depth`, of which `valid` are the key's */
FSMHIP_SRT_FN uint64_t srt_word(uint64_t le, uint32_t valid) { return srt_swap(le & srt_tail_mask(valid)); }

/* what is sorted by */
FSMHIP_SRT_FN uint64_t srt_sort_word(uint64_t word, bool reverse) { return reverse ? ~word : word; }
FSMHIP_SRT_FN uint32_t srt_sort_valid(uint32_t valid, bool reverse) { return reverse ? SRT_WORD - valid : valid; }
FSMHIP_SRT_FN uint32_t srt_raw_valid(uint32_t sort_valid, bool reverse) { return reverse ? SRT_WORD - sort_valid : sort_valid; }

/* the leading bytes that two chunks (two little-endian words each) share among their first n (0 .. 16) */
FSMHIP_SRT_FN uint32_t srt_common_chunk(uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi, uint32_t n)
{
	const uint64_t xl = alo ^ blo, xh = ahi ^ bhi;
	const uint32_t c = xl != 0u ? (uint32_t)__builtin_ctzll(xl) >> 3 : xh != 0u ? 8u + ((uint32_t)__builtin_ctzll(xh) >> 3) : SRT_CHUNK;
	return c < n ? c : n;
}

/* the bytes a bucket's depth advances by when its members share `common` bytes from the depth on: whole words */
FSMHIP_SRT_FN uint64_t srt_skip(uint64_t common) { return common & ~(uint64_t)(SRT_WORD - 1u); }

/* digit d (0 .. SRT_DIGITS - 1) of an entry */
FSMHIP_SRT_FN uint32_t srt_digit(uint64_t sort_word, uint32_t sort_valid, uint32_t bucket, uint32_t d)
{
	if (d == 0u) return sort_valid & 0xffu;
	if (d < SRT_DIGIT_BUCKET) return (uint32_t)(sort_word >> (8u * (d - 1u))) & 0xffu;
	return bucket >> (8u * (d - SRT_DIGIT_BUCKET)) & 0xffu;
}

/* the digits of the bucket that can differ among R records: the bytes of R - 1 */
FSMHIP_SRT_FN uint32_t srt_bucket_digits(uint64_t R)
{
	uint32_t n = 0;
	for (uint64_t top = R != 0u ? R - 1u : 0u; top != 0u; top >>= 8) n++;
	return n;
}

/* a sorted entry opens a bucket: the first one, or one that differs from its predecessor */
FSMHIP_SRT_FN bool srt_head(bool is_first, uint32_t bucket, uint64_t word, uint32_t valid, uint32_t pbucket, uint64_t pword, uint32_t pvalid)
{
	return is_first || bucket != pbucket || word != pword || valid != pvalid;
}

/* an entry's bucket goes on: more than one member (it is no head, or its successor is none) and a full word */
FSMHIP_SRT_FN bool srt_active(bool head, bool next_is_member, uint32_t raw_valid) { return raw_valid == SRT_WORD && (!head || next_is_member); }

FSMHIP_SRT_FN uint64_t srt_rounds_bound(uint64_t maxlen) { return maxlen / SRT_WORD + (maxlen % SRT_WORD != 0u ? 1u : 0u) + 1u; }

}

#endif
