/*
 * tally_seg.h -- the arithmetic of the tally (tally.hip, tally_spans) that can go wrong on its own: no HIP header, so that
 * tests/c/test_tally_seg.cpp checks it on the CPU against a brute-force count.  Not part of the C ABI.
 *
 * The definition is include/fsm_hip.h, "tally": input j owns entries off[j] .. off[j + 1] of id[total]; entry k falls into column
 * col(id[k]) of the group of its input; count[] counts entries, lines[] counts inputs that own at least one entry of the column.
 * Here are: the column of an id, the clamp of an offset to the total, the group of an input (as a position in group_off, so that
 * the two "counted nowhere" edges are values like any other), the 64-ary form of the search that a wavefront makes, and the rule
 * "first of its column in its input" over a window of (input, column) pairs with a bitmap carried from window to window for the
 * one input that may continue.  The search for the input of an entry is extract_seg.h's ext_last_le.
 * Everything is unsigned; nothing is trusted: whatever the arrays hold, every index these functions hand out lies inside the
 * bounds they were given -- arrays that do not ascend give wrong counts, never a wild access.  The arrays are read through []
 * alone, so the kernel passes pointers that name their address space and the CPU test plain ones.
 */
#ifndef FSMHIP_CSRC_TALLY_SEG_H
#define FSMHIP_CSRC_TALLY_SEG_H

#include <cstdint>

#include "extract_seg.h"

namespace fsmhip {

constexpr uint64_t TALLY_NONE = ~(uint64_t)0;    /* no input: no j is this large, since j < m <= SIZE_MAX / 8 */

/* the column of an id: itself below nrules, else the last column, "other" */
FSMHIP_EXT_FN uint64_t tally_col(uint32_t id, uint64_t nrules) { return (uint64_t)id < nrules ? (uint64_t)id : nrules; }

/* an entry of off above the total is the total */
FSMHIP_EXT_FN uint64_t tally_clamp(uint64_t x, uint64_t total) { return x < total ? x : total; }

/* The position of input j in group_off[0 .. G]: the number of entries at or below j, looked for in [lo, hi] with lo <= hi <=
 * G + 1 (the position of an input before j bounds it from below, of one behind j from above).  Position p means group p - 1;
 * 0 is "below group_off[0]" and G + 1 "at or above group_off[G]": counted nowhere.  Equal entries -- empty groups -- are stepped
 * over by the search itself: the group of j is the LAST g with group_off[g] <= j.  Reads group_off[lo .. hi - 1] at most. */
template <typename U64A>
FSMHIP_EXT_FN uint64_t tally_group_pos(U64A group_off, uint64_t j, uint64_t lo, uint64_t hi)
{
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2u;
		if ((uint64_t)group_off[mid] <= j) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

/* ext_last_le by a wavefront: the last index i in [lo, hi] with a[i] <= p, lo when there is none.  A round probes TALLY_KARY
 * indices -- lane t looks at tally_kary_probe(lo, hi, t) -- counts the lanes c whose entry is <= p, and narrows [lo, hi] to the
 * stretch between probe c - 1 (or lo) and probe c: a span of 38 000 inputs is 3 dependent loads, not 15.  The probes lie in
 * [lo + 1, hi], the range shrinks in every round whatever c is, and c of entries that do not ascend names some stretch of it. */
constexpr uint32_t TALLY_KARY = 64;
FSMHIP_EXT_FN uint64_t tally_kary_step(uint64_t lo, uint64_t hi) { return (hi - lo + (TALLY_KARY - 1u)) / TALLY_KARY; }
FSMHIP_EXT_FN uint64_t tally_kary_probe(uint64_t lo, uint64_t hi, uint32_t lane)
{
	const uint64_t idx = lo + (uint64_t)(lane + 1u) * tally_kary_step(lo, hi);
	return idx < hi ? idx : hi;
}
/* lo < hi, c in 0 .. TALLY_KARY */
FSMHIP_EXT_FN void tally_kary_narrow(uint64_t *lo, uint64_t *hi, uint32_t c)
{
	const uint64_t step = tally_kary_step(*lo, *hi);
	const uint64_t nlo = *lo + (uint64_t)c * step, nhi = *lo + (uint64_t)(c + 1u) * step - 1u;
	*lo = nlo < *hi ? nlo : *hi;
	*hi = nhi < *hi ? nhi : *hi;
}

/* a position that names a group of [0, G) */
FSMHIP_EXT_FN bool tally_pos_counts(uint64_t pos, uint64_t G) { return pos >= 1u && pos <= G; }

/* entry t of a window of (input, column) pairs is the first of its column in its input AS FAR AS THE WINDOW SHOWS: the look goes
 * backwards and stops at the first other input, so it takes at most t steps whatever the line holds */
template <typename U64A, typename U32A>
FSMHIP_EXT_FN bool tally_window_first(U64A win_j, U32A win_c, uint32_t t)
{
	const uint64_t j = win_j[t];
	const uint32_t c = win_c[t];
	for (uint32_t s = t; s-- > 0u;) {
		if ((uint64_t)win_j[s] != j) break;
		if ((uint32_t)win_c[s] == c) return false;
	}
	return true;
}

/* What a window does with the bitmap of the columns seen in ONE input.  jf and jl are the inputs of the window's first and last
 * entry, `carried` the input the bitmap belongs to (the last input of the window before; TALLY_NONE at the start of a span).
 *   carry_in  the bitmap holds the columns input jf has shown in earlier windows
 *   clear     the bitmap is cleared in mid-window: behind the tests of jf's entries, before the entries of jl set their bits --
 *             always when jf's line closes in this window, and when the bitmap belongs to an input that has closed already
 * An entry that is first of its column in the window counts, except:
 *   of input jf != jl:  only if carry_in does not hold or its bit is clear (a test: the line closes here, nothing is set)
 *   of input jl:        only if the bit was clear when it set it (behind the clear, if there is one)
 * Afterwards the bitmap belongs to jl. */
struct TallyCarry {
	bool carry_in, clear;
};
FSMHIP_EXT_FN TallyCarry tally_carry(uint64_t jf, uint64_t jl, uint64_t carried)
{
	TallyCarry r;
	r.carry_in = jf == carried;
	r.clear = jf != jl || !r.carry_in;
	return r;
}

FSMHIP_EXT_FN uint32_t tally_bit_word(uint32_t c) { return c >> 5; }
FSMHIP_EXT_FN uint32_t tally_bit_mask(uint32_t c) { return 1u << (c & 31u); }
/* the words of a bitmap of C columns */
FSMHIP_EXT_FN uint32_t tally_bit_words(uint64_t C) { return (uint32_t)((C + 31u) / 32u); }

}

#endif
