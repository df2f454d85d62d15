/*
 * extract_seg.h -- the arithmetic of one lookup of the extraction (extract.hip, ext_lengths / ext_offsets / ext_write): no HIP
 * header, so that tests/c/test_extract_seg.cpp checks it on the CPU against a brute-force extraction.  Not part of the C ABI.
 *
 * A kept match (start, end) of a line of `raw` bytes that begins at text byte beg is a RECORD (include/fsm_hip.h, "extract"):
 * the text bytes [beg + st, beg + en) with en = min(end, raw), st = min(start, en), followed by one separator byte when there is
 * one.  The records are packed, off[R + 1]; src[r] = beg + st of record r.  Output byte p belongs to the LAST r with off[r] <= p:
 * records without bytes (an empty match and no separator) share their offset with their successor, and only the last of such a
 * run can hold a byte.
 * Everything is unsigned and may wrap; nothing is trusted: whatever the arrays hold, ext_at() gives a text index that the caller
 * still holds against the limit, the separator, or no source at all, and a run of at least one byte -- wrong arrays give wrong
 * bytes, never a wild access and never a loop that does not advance.  The arrays are read through [] alone, so the kernel passes
 * pointers that name their address space and the CPU test plain ones.
 */
#ifndef FSMHIP_CSRC_EXTRACT_SEG_H
#define FSMHIP_CSRC_EXTRACT_SEG_H

#include <cstdint>

#ifdef __HIPCC__
#define FSMHIP_EXT_FN __host__ __device__ inline
#else
#define FSMHIP_EXT_FN inline
#endif

namespace fsmhip {

constexpr uint32_t EXT_FROM_NONE = 0;    /* no source: the byte is 0 (arrays gone wrong only) */
constexpr uint32_t EXT_FROM_TEXT = 1;    /* at: bytes from the text's first byte */
constexpr uint32_t EXT_FROM_SEP = 2;     /* the separator byte */

/* a match as the extraction takes it, on its own: inside [0, raw], start not behind end */
FSMHIP_EXT_FN void ext_clamp_match(uint64_t raw, uint64_t *start, uint64_t *end)
{
	const uint64_t e = *end < raw ? *end : raw;
	*start = *start < e ? *start : e;
	*end = e;
}

/* the bytes of the record of a clamped match */
FSMHIP_EXT_FN uint64_t ext_record_len(uint64_t st, uint64_t en, bool has_sep) { return (en - st) + (has_sep ? 1u : 0u); }

/* the match of rule `id` is kept: bits = the set's words of 32 rules, read only for id < nrules; no set keeps every match */
template <typename U32A>
FSMHIP_EXT_FN bool ext_kept(U32A bits, bool has_set, uint64_t nrules, bool keep_other, uint32_t id)
{
	if (!has_set) return true;
	if ((uint64_t)id >= nrules) return keep_other;
	return ((uint32_t)bits[id >> 5] >> (id & 31u) & 1u) != 0u;
}

/* the last index i in [lo, hi] with a[i] <= p; lo when there is none (or when hi < lo).  Entries that repeat -- inputs without
 * matches, records without bytes -- are stepped over by the search itself, so a run of a million of them costs 20 steps. */
template <typename U64A>
FSMHIP_EXT_FN uint64_t ext_last_le(U64A a, uint64_t lo, uint64_t hi, uint64_t p)
{
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1u) / 2u;
		if ((uint64_t)a[mid] <= p) lo = mid; else hi = mid - 1u;
	}
	return lo;
}

struct ExtAt {
	uint32_t from;   /* EXT_FROM_* */
	uint64_t at;     /* EXT_FROM_TEXT: the text index of output byte p */
	uint64_t run;    /* >= 1: output bytes p .. p + run - 1 come from at .. at + run - 1 (one byte for the separator) */
};

/* the source of output byte p in the record [o0, o1) whose text begins at src */
FSMHIP_EXT_FN ExtAt ext_at(uint64_t o0, uint64_t o1, uint64_t src, bool has_sep, uint64_t p)
{
	ExtAt r;
	r.from = EXT_FROM_NONE;
	r.at = 0;
	r.run = 1u;
	if (p < o0 || p >= o1) return r;
	const uint64_t q = p - o0, tlen = (o1 - o0) - (has_sep ? 1u : 0u);
	if (q < tlen) {
		r.from = EXT_FROM_TEXT;
		r.at = src + q;
		r.run = tlen - q;
		if (r.at < src) r.from = EXT_FROM_NONE, r.run = 1u;   /* (wrapped) */
	} else {
		r.from = EXT_FROM_SEP;
	}
	return r;
}

/* sixteen bytes may be loaded at text index `at`: all of them below the limit */
FSMHIP_EXT_FN bool ext_window_below(uint64_t at, uint64_t limit) { return limit >= 16u && at <= limit - 16u; }

/* the window whose byte t (0 .. 15) is text byte `at` may be loaded whole: it begins inside the text and ends below the limit */
FSMHIP_EXT_FN bool ext_window_ok(uint64_t at, uint32_t t, uint64_t limit) { return at >= t && ext_window_below(at - t, limit); }

/* the whole chunk of sixteen output bytes from p on lies in the text part of the record [o0, o1) and may be loaded at once */
FSMHIP_EXT_FN bool ext_chunk_in_text(const ExtAt &s, uint64_t limit) { return s.from == EXT_FROM_TEXT && s.run >= 16u && ext_window_below(s.at, limit); }

}

#endif
