/*
 * test_match_marks.cpp -- libfsm_amd/csrc/match_marks.h on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_matches_abi.py builds and runs it): for random offsets -- increasing, decreasing, beyond the limit, huge --
 * clipped to a limit, every word a line may touch lies inside an array of marks_words(limit, n) words, and the marks of a line
 * written as walk_mark writes them (downward from the word of position len) are read back bit by bit.  With increasing offsets
 * inside the limit no two lines share a word.  And the seek step of walk_match (marks_next_in_word) against a bit-by-bit search:
 * whatever bits a word holds behind len -- another line's, where regions overlap -- it never gives a position behind len.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libfsm_amd/csrc/match_marks.h"

using namespace fsmhip;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

/* one text: n lines with offsets of `kind`, limit; trim: every line one byte shorter where it can be */
static void one(uint64_t n, uint64_t limit, int kind, bool trim)
{
	std::vector<uint64_t> off(n + 1);
	uint64_t at = rnd() % 7;
	for (uint64_t i = 0; i <= n; i++) {
		switch (kind) {
		case 0: off[i] = at; at += rnd() % 70; break;                                   /* increasing, may pass the limit */
		case 1: off[i] = rnd() % (limit + 40); break;                                   /* any order */
		case 2: off[i] = (i & 1) ? UINT64_MAX - rnd() % 5 : rnd() % (limit + 1); break; /* huge ones between */
		default: off[i] = limit > i ? limit - i : 0; break;                             /* decreasing */
		}
	}
	const uint64_t words = marks_words(limit, n);
	std::vector<uint16_t> marks(words, 0);
	std::vector<uint32_t> owner(words, UINT32_MAX);
	bool increasing = true;
	for (uint64_t i = 0; i < n; i++) increasing = increasing && off[i] <= off[i + 1];
	for (uint64_t i = 0; i < n; i++) {
		uint64_t beg = 0, len = 0;
		marks_clip(off[i], off[i + 1], limit, &beg, &len);
		CHECK(len == 0 || (beg <= limit && len <= limit - beg));
		const uint64_t region = marks_region(beg, limit, i);
		if (trim && len != 0) len--;
		const uint64_t nw = marks_line_words(len);
		CHECK(nw == (len >> 4) + 1);
		CHECK(region <= words && nw <= words - region);      /* every word of the line is below the array's size */
		/* as walk_mark stores them: a pattern of the position, from the top word down */
		for (uint64_t w = nw; w-- > 0;) {
			uint16_t v = 0;
			for (uint32_t b = 0; b < 16; b++) {
				const uint64_t s = (w << 4) + b;
				if (s <= len && (s * 2654435761u + i) % 3 == 0) v |= (uint16_t)(1u << b);
			}
			marks[region + w] = v;                           /* (the vector is the bound check under ASan, too) */
			if (increasing) {
				CHECK(owner[region + w] == UINT32_MAX);      /* no two lines share a word */
				owner[region + w] = (uint32_t)i;
			}
		}
		if (increasing)
			for (uint64_t s = 0; s <= len; s++)
				CHECK(((marks[region + (s >> 4)] >> (s & 15)) & 1u) == ((s * 2654435761u + i) % 3 == 0 ? 1u : 0u));
	}
}

/* the seek step: against a bit-by-bit search, with foreign bits standing behind len in the top word (overlapping regions) */
static void seek()
{
	for (int round = 0; round < 20000; round++) {
		const uint64_t len = round < 40 ? (uint64_t)round : rnd() % 700;
		const uint64_t p = rnd() % (len + 1);
		const uint32_t word = round % 3 == 0 ? 0xffffu : (uint32_t)(rnd() & 0xffffu);      /* any bits, behind len too */
		uint64_t want = MARKS_NONE;
		for (uint32_t b = 0; b < 16; b++) {
			const uint64_t s = (p & ~(uint64_t)15) + b;
			if (s >= p && s <= len && ((word >> b) & 1u) != 0u) { want = s; break; }
		}
		const uint64_t got = marks_next_in_word(word, p, len);
		CHECK(got == want);
		CHECK(got == MARKS_NONE || (got >= p && got <= len));           /* never a position behind len */
	}
	/* the reviewer's case: line 0 is empty (len 0), and a long line's word lies over its region: bits 1 .. 15 are foreign */
	CHECK(marks_next_in_word(0xfffeu, 0, 0) == MARKS_NONE);
	CHECK(marks_next_in_word(0xffffu, 0, 0) == 0);
	CHECK(marks_next_in_word(0xffffu, 17, 20) == 17 && marks_next_in_word(0xffe0u, 17, 20) == MARKS_NONE);
	CHECK(marks_next_in_word(0x8000u, 16, 31) == 31 && marks_next_in_word(0x8000u, 16, 30) == MARKS_NONE);
	CHECK(marks_next_in_word(0x8000u, 16, 100) == 31);
}

int main()
{
	seek();
	for (int round = 0; round < 400; round++) {
		const uint64_t n = 1 + rnd() % 200;
		const uint64_t limit = round % 10 == 0 ? rnd() % 20 : rnd() % 6000;
		for (int kind = 0; kind < 4; kind++) {
			one(n, limit, kind, false);
			one(n, limit, kind, true);
		}
	}
	one(1, 0, 0, false);
	one(5, 15, 3, true);
	one(5, 16, 0, false);
	/* the largest values do not wrap: a limit of 2^63 and lines at its end */
	{
		uint64_t beg = 0, len = 0;
		const uint64_t limit = (uint64_t)1 << 63;
		marks_clip(limit - 100, UINT64_MAX, limit, &beg, &len);
		CHECK(len == 100);
		CHECK(marks_region(beg, limit, 7) + marks_line_words(len) <= marks_words(limit, 8));
		marks_clip(UINT64_MAX, UINT64_MAX, limit, &beg, &len);
		CHECK(len == 0 && marks_region(beg, limit, 7) + marks_line_words(len) <= marks_words(limit, 8));
	}
	std::printf("test_match_marks: ok\n");
	return 0;
}
