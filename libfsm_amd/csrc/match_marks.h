/*
 * match_marks.h -- where the marks of the matches (match.hip, walk_mark / walk_match) lie: the index arithmetic alone, no HIP
 * header, so that tests/c/test_match_marks.cpp checks it on the CPU.  Not part of the C ABI.
 *
 * A mark is one bit per position of a walked line: bit (s & 15) of word (s >> 4) of the line's region says M(s), for s in
 * 0 .. len inclusive (include/fsm_hip.h, "matches").  The words are u16.  The region of line i begins at
 *     floor(beg / 16) + i
 * where beg is the line's first byte (the limit, for a line that begins behind it), and has floor(len / 16) + 1 words; the
 * array has floor(limit / 16) + n + 1.  With offsets that do not decrease the regions are disjoint: a line ends where the next
 * begins, and the + i keeps two lines of the same sixteen bytes apart.
 * No scan is needed, and no offsets can make a region leave the array: the clip gives beg + len <= limit, so
 *     floor(beg / 16) + floor(len / 16) <= floor((beg + len) / 16) <= floor(limit / 16)
 * and with i <= n - 1 the region's last word is at most floor(limit / 16) + n - 1.  Offsets that decrease can make regions
 * overlap: wrong answers, never a store outside the array.
 */
#ifndef FSMHIP_CSRC_MATCH_MARKS_H
#define FSMHIP_CSRC_MATCH_MARKS_H

#include <cstdint>

#ifdef __HIPCC__
#define FSMHIP_MARKS_FN __host__ __device__ inline
#else
#define FSMHIP_MARKS_FN inline
#endif

namespace fsmhip {

/* the line [o0, o1) of a text of which `limit` bytes may be read: its first byte and its length, clipped (walk_pos's rule) */
FSMHIP_MARKS_FN void marks_clip(uint64_t o0, uint64_t o1, uint64_t limit, uint64_t *beg, uint64_t *len)
{
	uint64_t l = o1 > o0 ? o1 - o0 : 0u;
	if (o0 > limit) l = 0u;
	else if (l > limit - o0) l = limit - o0;
	*beg = o0;
	*len = l;
}

/* the words of the whole array, for n lines */
FSMHIP_MARKS_FN uint64_t marks_words(uint64_t limit, uint64_t n) { return (limit >> 4) + n + 1u; }

/* the first word of line i's region; a line that begins behind the limit is empty and counts as beginning at the limit */
FSMHIP_MARKS_FN uint64_t marks_region(uint64_t beg, uint64_t limit, uint64_t i) { return ((beg < limit ? beg : limit) >> 4) + i; }

/* the words a line of (trimmed or not) length len uses: positions 0 .. len */
FSMHIP_MARKS_FN uint64_t marks_line_words(uint64_t len) { return (len >> 4) + 1u; }

/* the seek step of walk_match.  `word` is word p >> 4 of a line's region, p <= len: the lowest marked position in [p, len] that
 * it holds, or MARKS_NONE.  The bits of positions behind len are masked off, not trusted to be 0: where offsets decrease, regions
 * overlap and another line's bits can stand there, and a position behind len must never reach the walk (it would read behind
 * the line, and behind the limit). */
constexpr uint64_t MARKS_NONE = UINT64_MAX;
FSMHIP_MARKS_FN uint64_t marks_next_in_word(uint32_t word, uint64_t p, uint64_t len)
{
	uint32_t keep = (0xffffu << (uint32_t)(p & 15u)) & 0xffffu;
	if ((p >> 4) == (len >> 4)) keep &= (2u << (uint32_t)(len & 15u)) - 1u;
	word &= keep;
	if (word == 0u) return MARKS_NONE;
	return (p & ~(uint64_t)15u) + (uint32_t)__builtin_ctz(word);
}

}

#endif
