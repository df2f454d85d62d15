/*
 * replace_seg.h -- where byte q of a replaced line comes from (replace.hip, repl_lengths / repl_write): the arithmetic alone, no
 * HIP header, so that tests/c/test_replace_seg.cpp checks it on the CPU against a brute-force splice.  Not part of the C ABI.
 *
 * A line of `raw` bytes (its trimmed delimiter included) has nm matches (start_k, end_k, id_k) in order.  Match k is replaced by
 * X_k (include/fsm_hip.h, "replace"): R[id_k] under the default rule, R[id_k] repeated to the match's own length under MASK, the
 * match's own bytes where the table has nothing for it ("stays").  The lengths pass leaves, per match,
 *     xlen[k] = |X_k|,   mpos[k] = start_k + sum over i < k of (xlen[i] - (end_i - start_i))
 * mpos[k] is where X_k begins in the OUTPUT line, so the output line is
 *     [0, mpos[0])  the text from 0;  [mpos[k], mpos[k] + xlen[k])  X_k;  [mpos[k] + xlen[k], mpos[k + 1])  the text from end_k
 * and byte q belongs to the LAST k with mpos[k] <= q: matches whose X is empty and that are followed by no text share their mpos
 * with the next one, and only the last of such a run can hold a byte.
 * Everything is unsigned and may wrap; nothing is trusted: whatever the arrays hold, repl_at() gives an index below `raw` (text),
 * below `rbytes` (table) or no source at all, and a run of at least one byte -- wrong arrays give wrong bytes, never a wild access
 * and never a loop that does not advance.  The arrays are read through [] alone, so the kernel passes pointers that name their
 * address space (global or LDS) and the CPU test plain ones.
 * A template table (the match itself inside its replacement) has a repl_at() and a repl_xlen() of its own at the end of this file,
 * with the same promises; tests/c/test_replace_tmpl.cpp checks them.
 */
#ifndef FSMHIP_CSRC_REPLACE_SEG_H
#define FSMHIP_CSRC_REPLACE_SEG_H

#include <cstdint>

#ifdef __HIPCC__
#define FSMHIP_REPL_FN __host__ __device__ inline
#else
#define FSMHIP_REPL_FN inline
#endif

namespace fsmhip {

constexpr uint32_t REPL_FROM_NONE = 0;   /* no source: the byte is 0 (arrays gone wrong only) */
constexpr uint32_t REPL_FROM_TEXT = 1;   /* at: bytes from the line's first byte, < raw */
constexpr uint32_t REPL_FROM_TABLE = 2;  /* at: bytes from the table's first byte, < rbytes */

/* the table has bytes for a match of rule `id`: else the match stays.  rlen = |R[id]| (read only when id < nrepl) */
FSMHIP_REPL_FN bool repl_uses_table(uint64_t id, uint64_t nrepl, uint64_t rlen, bool mask) { return id < nrepl && !(mask && rlen == 0u); }

/* |X| of a match of mlen bytes */
FSMHIP_REPL_FN uint64_t repl_xlen(uint64_t mlen, bool uses_table, uint64_t rlen, bool mask) { return uses_table && !mask ? rlen : mlen; }

/* a match as the lengths pass takes it: inside [at_least, len], end not before start (matches that are in order and inside the line
 * are left as they are); with it the sum of the matches' lengths never exceeds len and no output length wraps */
FSMHIP_REPL_FN void repl_clamp_match(uint64_t at_least, uint64_t len, uint64_t *start, uint64_t *end)
{
	uint64_t s = *start, e = *end;
	if (s < at_least) s = at_least;
	if (s > len) s = len;
	if (e < s) e = s;
	if (e > len) e = len;
	*start = s;
	*end = e;
}

struct ReplAt {
	uint32_t from;   /* REPL_FROM_* */
	uint64_t at;     /* the source index of output byte q */
	uint64_t run;    /* >= 1: output bytes q .. q + run - 1 come from at .. at + run - 1 and lie in the same output line */
	uint64_t k;      /* the match q belongs to, nm if none: always <= nm */
};

/* the source of byte q of an output line of outlen bytes.  mpos, xlen, start, end, id: the line's nm matches; roff: the table's
 * nrepl + 1 offsets, rbytes its bytes */
template <typename U64A, typename U64B, typename U32A, typename ROFF>
FSMHIP_REPL_FN ReplAt repl_at(U64A mpos, U64A xlen, U64B start, U64B end, U32A id, uint64_t nm, ROFF roff, uint64_t nrepl, uint64_t rbytes,
                              bool mask, uint64_t q, uint64_t outlen, uint64_t raw)
{
	uint64_t lo = 0, hi = nm;                        /* the first match with mpos > q */
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2u;
		if ((uint64_t)mpos[mid] <= q) lo = mid + 1u; else hi = mid;
	}
	const uint64_t next = lo < nm ? (uint64_t)mpos[lo] : outlen;   /* where the stretch q lies in ends at the latest */
	ReplAt r;
	r.from = REPL_FROM_TEXT;
	r.k = nm;
	r.at = q;
	r.run = next > q ? next - q : 1u;
	if (lo != 0u) {
		const uint64_t k = lo - 1u, d = q - (uint64_t)mpos[k], xl = (uint64_t)xlen[k];
		r.k = k;
		if (d < xl) {                                /* inside X_k */
			const uint64_t i = (uint64_t)id[k];
			const uint64_t r0 = i < nrepl ? (uint64_t)roff[i] : 0u, r1 = i < nrepl ? (uint64_t)roff[i + 1u] : 0u;
			const uint64_t rlen = r1 > r0 ? r1 - r0 : 0u;
			if (xl - d < r.run) r.run = xl - d;
			if (repl_uses_table(i, nrepl, rlen, mask)) {
				const uint64_t t = mask ? d % rlen : d;
				r.from = REPL_FROM_TABLE;
				r.at = r0 + t;
				if (r.at >= rbytes || t >= rlen) {
					r.from = REPL_FROM_NONE;
					r.run = 1u;
				} else if (rlen - t < r.run) {
					r.run = rlen - t;                /* MASK: the table's bytes begin again */
				}
				return r;
			}
			r.at = (uint64_t)start[k] + d;           /* the match stays */
		} else {
			r.at = (uint64_t)end[k] + (d - xl);
		}
	}
	if (r.at >= raw) {
		r.from = REPL_FROM_NONE;
		r.run = 1u;
	} else if (raw - r.at < r.run) {
		r.run = raw - r.at;
	}
	return r;
}

/* ---- templates: the match itself inside its replacement (include/fsm_hip.h, "replace", templates) --------------------------------
 * Rule i has c inserts at the ascending positions a_0 <= ... <= a_{c-1} of R[i], each at most |R[i]|, and a match of L bytes gives
 *     X = R[i][0:a_0]  M  R[i][a_0:a_1]  M ... M  R[i][a_{c-1}:|R[i]|],      |X| = |R[i]| + c * L
 * The s-th copy of M begins at byte a_s + s * L of X, which does not decrease in s: byte d of X lies behind the LAST s with
 * a_s + s * L <= d, in that copy when d - (a_s + s * L) < L and in the literal behind it otherwise.  A table without MASK only. */

constexpr uint64_t REPL_MAX_INSERTS = 255;   /* per rule: an interface condition (fsm_hip_repl_max_inserts) */

/* the inserts of rule `id`: [*i0, *i0 + c) of the nins positions, whatever ioff holds; c <= REPL_MAX_INSERTS; none beyond the table */
template <typename IOFF>
FSMHIP_REPL_FN uint64_t repl_inserts_of(IOFF ioff, uint64_t id, uint64_t nrepl, uint64_t nins, uint64_t *i0)
{
	*i0 = 0;
	if (id >= nrepl) return 0u;
	uint64_t a = (uint64_t)ioff[id], b = (uint64_t)ioff[id + 1u];
	if (a > nins) a = nins;
	if (b > nins) b = nins;
	*i0 = a;
	const uint64_t c = b > a ? b - a : 0u;
	return c < REPL_MAX_INSERTS ? c : REPL_MAX_INSERTS;
}

/* |X| of a match of mlen bytes whose rule is in the table (id < nrepl) and has c inserts: mlen <= the line's bytes and
 * c <= REPL_MAX_INSERTS, so nothing wraps */
FSMHIP_REPL_FN uint64_t repl_xlen(uint64_t mlen, uint64_t rlen, uint64_t c) { return rlen + c * mlen; }

/* repl_at() for a template table: ioff, the table's nrepl + 1 insert offsets, ins its nins positions.  Where no rule of the line
 * has an insert the answer is repl_at()'s for mask = false.  The match's length is taken from xlen, as the lengths pass left it:
 * L = (xlen - |R|) / c. */
template <typename U64A, typename U64B, typename U32A, typename ROFF, typename IOFF, typename INS>
FSMHIP_REPL_FN ReplAt repl_at(U64A mpos, U64A xlen, U64B start, U64B end, U32A id, uint64_t nm, ROFF roff, IOFF ioff, INS ins, uint64_t nrepl,
                              uint64_t rbytes, uint64_t nins, uint64_t q, uint64_t outlen, uint64_t raw)
{
	uint64_t lo = 0, hi = nm;                        /* the first match with mpos > q */
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2u;
		if ((uint64_t)mpos[mid] <= q) lo = mid + 1u; else hi = mid;
	}
	const uint64_t next = lo < nm ? (uint64_t)mpos[lo] : outlen;
	ReplAt r;
	r.from = REPL_FROM_TEXT;
	r.k = nm;
	r.at = q;
	r.run = next > q ? next - q : 1u;
	if (lo != 0u) {
		const uint64_t k = lo - 1u, d = q - (uint64_t)mpos[k], xl = (uint64_t)xlen[k];
		r.k = k;
		if (d < xl) {                                /* inside X_k */
			const uint64_t i = (uint64_t)id[k];
			if (xl - d < r.run) r.run = xl - d;
			if (i < nrepl) {
				const uint64_t r0 = (uint64_t)roff[i], r1 = (uint64_t)roff[i + 1u];
				const uint64_t rlen = r1 > r0 ? r1 - r0 : 0u;
				uint64_t i0;
				const uint64_t c = repl_inserts_of(ioff, i, nrepl, nins, &i0);
				const uint64_t L = c != 0u && xl > rlen ? (xl - rlen) / c : 0u;
				uint64_t t = d, upto = rlen;         /* the literal's byte and where its stretch ends: L == 0 is X = R[i] */
				if (L != 0u) {
					uint64_t slo = 0, shi = c;       /* the first insert whose copy begins behind d (s * L <= xl: no wrap) */
					while (slo < shi) {
						const uint64_t mid = slo + (shi - slo) / 2u;
						uint64_t a = (uint64_t)ins[i0 + mid];
						if (a > rlen) a = rlen;
						if (a + mid * L <= d) slo = mid + 1u; else shi = mid;
					}
					if (slo < c) {
						upto = (uint64_t)ins[i0 + slo];
						if (upto > rlen) upto = rlen;
					}
					if (slo != 0u) {
						uint64_t a = (uint64_t)ins[i0 + slo - 1u];
						if (a > rlen) a = rlen;
						const uint64_t e = d - (a + (slo - 1u) * L);
						if (e < L) {                 /* in the copy of the match: text again */
							if (L - e < r.run) r.run = L - e;
							r.at = (uint64_t)start[k] + e;
							if (r.at >= raw) {
								r.from = REPL_FROM_NONE;
								r.run = 1u;
							} else if (raw - r.at < r.run) {
								r.run = raw - r.at;
							}
							return r;
						}
						t = a + (e - L);
					}
				}
				r.from = REPL_FROM_TABLE;
				r.at = r0 + t;
				if (r.at >= rbytes || t >= rlen) {
					r.from = REPL_FROM_NONE;
					r.run = 1u;
				} else {
					const uint64_t left = upto > t ? upto - t : 1u;
					if (left < r.run) r.run = left;
					if (rbytes - r.at < r.run) r.run = rbytes - r.at;
				}
				return r;
			}
			r.at = (uint64_t)start[k] + d;           /* the match stays */
		} else {
			r.at = (uint64_t)end[k] + (d - xl);
		}
	}
	if (r.at >= raw) {
		r.from = REPL_FROM_NONE;
		r.run = 1u;
	} else if (raw - r.at < r.run) {
		r.run = raw - r.at;
	}
	return r;
}

}

#endif
