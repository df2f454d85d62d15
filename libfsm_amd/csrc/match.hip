/*
 * match.hip -- matches: every match of every line -- start, end, the end-id of the state it ended in -- in ONE call.
 *
 * The spans of text.hip deliver one match per hit per round: two walk_pos launches a round, `starts` walked backward over
 * [p, len) again in every round, the host driving.  Here `starts` walks every line ONCE and leaves a bit per position, and a
 * lane with a cursor of its own (walk_tok's loop) goes from mark to mark.  include/fsm_hip.h, section "matches", is the
 * definition.
 *
 * walk_mark is walk_pos<true> with from = 0 that keeps its accept masks: one workgroup = 256 consecutive inputs, one input per
 * lane, the table copied to LDS once, the line taken in 16-byte chunks from its end, the sixteen class lookups issued together,
 * then the chain of sixteen dependent table lookups.  The chunks are the sixteens of the LINE (chunk w = bytes 16 w .. 16 w +
 * 15, the short one first, at the line's end), so the mask of a chunk is word w of the line's marks as it stands: bit b is
 * M(16 w + b).  The bit of position len comes from the start state.  After DEAD or an absorbing state a lane looks nothing up:
 * the words it still owes are all 0 or all 1 and are stored after the loop.  Where the words lie: match_marks.h.
 *
 * walk_match<EMIT> is walk_tok's loop with another restart: at its cursor p a lane takes the next marked position from its
 * marks, sixteen positions a load, and walks `ends` forward from there with the last accept (bytes, state) kept beside the
 * chain, from the start state's own bit on.  After the chunk in which the walk stopped -- DEAD, an absorbing state, the line's
 * end -- it closes the attempt (a match, or the input is done) and moves p.  The turn ends when no lane is live.  EMIT = false
 * counts; the front scans the counts; EMIT = true walks again and stores start / end / id at match_off[j] + t, never more than
 * match_off[j + 1] - match_off[j] of them.  Nothing outside [base, base + limit) is read (walk_pos's clipping rule), no mark
 * outside the array is touched.  Every pointer names its address space (no FLAT instruction: tests/test_abi.py).
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <optional>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "image.h"
#include "match.h"
#include "match_marks.h"
#include "span.h"
#include "text_objects.h"
#include "tok.h"

namespace fsmhip {

constexpr uint32_t MATCH_THREADS = 256;      /* inputs per workgroup, one per lane */

/* m inputs fit one launch's grid */
static bool match_grid_fits(uint64_t m) { return (m + MATCH_THREADS - 1u) / MATCH_THREADS <= 0x7fffffffu; }

/* one pass over m inputs; every pointer is device memory */
struct MatchRun {
	LineBatch in;                            /* its limit always given (the marks are sized by it); flags: FSM_HIP_MATCHES_* */
	uint16_t *marks = nullptr;               /* marks_words(limit, n) words (match_marks.h): walk_mark writes, walk_match reads */
	uint64_t nwords = 0;
	uint64_t *count = nullptr;               /* the count pass writes it: m */
	const uint64_t *match_off = nullptr;     /* the emit pass reads it: m + 1 */
	uint64_t *start_out = nullptr, *end_out = nullptr;   /* ... and stores at match_off[j] + t */
	uint32_t *id_out = nullptr;
};

}

using namespace fsmhip;

namespace {

static_assert(MATCH_THREADS == 256, "one thread per byte value copies the class map");
static_assert(POS_LDS_ENTRIES == TOK_LDS_ENTRIES, "both images have the same LDS form");
constexpr uint32_t MATCH_LDS_ENTRIES = POS_LDS_ENTRIES;

typedef uint32_t u32x4m __attribute__((ext_vector_type(4)));

/* the launch's arguments, by value: every pointer is device memory */
struct MatchArgs {
	const void *tab;         /* [entries]: u16 (LDS form) or u32, the end-state bit of the target folded in */
	const uint16_t *col;     /* [256] */
	const uint32_t *ids;     /* walk_match: by TokImage::id_index() */
	const uint8_t *base;
	const uint64_t *off, *pick;
	uint16_t *marks;
	uint64_t *count;
	const uint64_t *match_off;
	uint64_t *start_out, *end_out;
	uint32_t *id_out;
	uint64_t n, m, limit, nwords;
	uint32_t entries, C;
	uint32_t start, abs_min;     /* in the walk's unit */
	uint32_t in_lds, flags;
	int32_t trim;
};

__device__ __forceinline__ uint32_t match_byte_at(const u32x4m &w, int k)
{
	const uint32_t d = (k < 4) ? w.x : (k < 8) ? w.y : (k < 12) ? w.z : w.w;
	return (d >> (8 * (k & 3))) & 0xffu;
}

__global__ void __launch_bounds__(MATCH_THREADS)
walk_mark(const MatchArgs a)
{
	typedef const uint16_t __attribute__((address_space(1))) *g_u16p;
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef uint16_t __attribute__((address_space(1))) *g_u16w;
	typedef u32x4m __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	__shared__ uint16_t col[256];
	__shared__ uint16_t tab[MATCH_LDS_ENTRIES];
	const uint32_t tid = threadIdx.x;
	const bool in_lds = a.in_lds != 0u;
	const uint32_t C = a.C;
	col[tid] = ((g_u16p)(uintptr_t)a.col)[tid];
	if (in_lds)
		for (uint32_t e = tid; e < a.entries; e += MATCH_THREADS) tab[e] = ((g_u16p)(uintptr_t)a.tab)[e];
	__syncthreads();

	const g_u64p off = (g_u64p)(uintptr_t)a.off;
	const g_u32p dense = (g_u32p)(uintptr_t)a.tab;
	const g_u16w marks = (g_u16w)(uintptr_t)a.marks;
	const uint64_t base = reinterpret_cast<uint64_t>(a.base);
	const uint64_t j = (uint64_t)blockIdx.x * MATCH_THREADS + tid;
	const bool valid = j < a.m;
	uint64_t i = j;
	if (valid && a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	const bool have = valid && i < a.n;              /* a pick beyond the lines: no mark, nothing read */
	const uint64_t limit = a.limit;
	uint64_t beg = 0, len = 0;
	if (have) marks_clip(off[i], off[i + 1], limit, &beg, &len);   /* every load below stays inside the readable bytes */
	const uint64_t region = marks_region(beg, limit, have ? i : 0u);  /* (before the trim: the same in both kernels) */
	if (a.trim >= 0 && len != 0u && (uint32_t)((g_u8p)(base + beg))[len - 1u] == (uint32_t)a.trim) len--;

	const uint32_t end_bit = in_lds ? 1u : 0x80000000u;
	const uint32_t absorbing = a.abs_min;            /* (even in the LDS form: comparing the state with its bit still on is the same) */
	const uint32_t col_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)col;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;
	uint32_t s = a.start;
	const int64_t top = (int64_t)(len >> 4);         /* the word of position len */
	int64_t w = have ? top : -1;                     /* the word this lane owes next, downward; -1: none */
	uint32_t at_len = (s & end_bit) != 0u ? 1u << (uint32_t)(len & 15u) : 0u;   /* M(len): the start state, before any byte */

	for (;;) {
		const bool live = w >= 0 && (s & ~end_bit) < absorbing;
		if (!__any(live)) break;
		/* the bytes of the line in chunk w: 16, but len & 15 (0 .. 15) in the first */
		const uint32_t cnt = !live ? 0u : w == top ? (uint32_t)(len & 15u) : 16u;
		u32x4m v = {0u, 0u, 0u, 0u};
		if (live) {
			const uint64_t at = beg + ((uint64_t)w << 4);    /* the chunk's first byte, from base */
			if (at + 16u <= limit) {
				v = *(g_chunkp)(base + at);
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(base + at))[k] << ((k & 3u) * 8u);
				v = u32x4m{d[0], d[1], d[2], d[3]};
			}
		}
		/* walk step k takes byte 15 - k of the chunk; the state after it is the one of position 16 w + 15 - k */
		uint32_t mask = 0u;
		uint32_t c2[16];
#pragma unroll
		for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(col_at + match_byte_at(v, 15 - k) * 2u);
		if (in_lds) {
			if (__all(cnt == 16u || !live)) {            /* whole chunks everywhere */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					sn = *(l_u16p)(uintptr_t)(tab_at + (sn & 0xfffeu) + c2[k]);
					mask |= (sn & 1u) << (15 - k);
				}
				s = live ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + (s & 0xfffeu) + c2[k]);
					const bool in = (uint32_t)(15 - k) < cnt;    /* the bytes behind the line's end are not walked */
					s = in ? sn : s;
					mask |= (in ? sn & 1u : 0u) << (15 - k);
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)(15 - k) < cnt) {
					s = dense[(uint64_t)(s & 0x7fffffffu) * C + c2[k]];
					mask |= (s >> 31) << (15 - k);
				}
			}
		}
		if (live) {
			const uint64_t at = region + (uint64_t)w;
			if (at < a.nwords) marks[at] = (uint16_t)(mask | at_len);
			at_len = 0u;
			w--;
		}
	}
	/* DEAD accepts nothing more, an absorbing end state accepts at every smaller position: nothing is looked up for them */
	const uint32_t fill = (s & end_bit) != 0u ? 0xffffu : 0u;
	if (w == top && w >= 0) {                        /* the start state itself is absorbing: positions 16 top .. len */
		const uint64_t at = region + (uint64_t)w;
		if (at < a.nwords) marks[at] = (uint16_t)(fill & ((2u << (uint32_t)(len & 15u)) - 1u));
		w--;
	}
	for (; w >= 0; w--) {
		const uint64_t at = region + (uint64_t)w;
		if (at < a.nwords) marks[at] = (uint16_t)fill;
	}
}

template <bool EMIT>
__global__ void __launch_bounds__(MATCH_THREADS)
walk_match(const MatchArgs a)
{
	typedef const uint16_t __attribute__((address_space(1))) *g_u16p;
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;
	typedef uint32_t __attribute__((address_space(1))) *g_u32w;
	typedef u32x4m __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	__shared__ uint16_t col[256];
	__shared__ uint16_t tab[MATCH_LDS_ENTRIES];
	const uint32_t tid = threadIdx.x;
	const bool in_lds = a.in_lds != 0u;
	const uint32_t C = a.C;
	col[tid] = ((g_u16p)(uintptr_t)a.col)[tid];
	if (in_lds)
		for (uint32_t e = tid; e < a.entries; e += MATCH_THREADS) tab[e] = ((g_u16p)(uintptr_t)a.tab)[e];
	__syncthreads();

	const g_u64p off = (g_u64p)(uintptr_t)a.off;
	const g_u32p dense = (g_u32p)(uintptr_t)a.tab;
	const g_u32p ids = (g_u32p)(uintptr_t)a.ids;
	const g_u16p marks = (g_u16p)(uintptr_t)a.marks;
	const uint64_t base = reinterpret_cast<uint64_t>(a.base);
	const uint64_t j = (uint64_t)blockIdx.x * MATCH_THREADS + tid;
	const bool valid = j < a.m;
	uint64_t i = j;
	if (valid && a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	const bool have = valid && i < a.n;              /* a pick beyond the lines: no match, nothing read */
	const uint64_t limit = a.limit;
	uint64_t beg = 0, len = 0;
	if (have) marks_clip(off[i], off[i + 1], limit, &beg, &len);   /* every load below stays inside the readable bytes */
	const uint64_t region = marks_region(beg, limit, have ? i : 0u);
	if (a.trim >= 0 && len != 0u && (uint32_t)((g_u8p)(base + beg))[len - 1u] == (uint32_t)a.trim) len--;
	uint64_t cap = 0, out_at = 0;                    /* EMIT: the lane's slots */
	if (EMIT && valid) {
		out_at = ((g_u64p)(uintptr_t)a.match_off)[j];
		const uint64_t nx = ((g_u64p)(uintptr_t)a.match_off)[j + 1u];
		cap = nx > out_at ? nx - out_at : 0u;
	}
	const g_u64w start_out = (g_u64w)(uintptr_t)a.start_out, end_out = (g_u64w)(uintptr_t)a.end_out;
	const g_u32w id_out = (g_u32w)(uintptr_t)a.id_out;

	const uint32_t end_bit = in_lds ? 1u : 0x80000000u;
	const uint32_t absorbing = a.abs_min;            /* (even in the LDS form: comparing the state with its bit still on is the same) */
	const bool drop_empty = (a.flags & FSM_HIP_MATCHES_DROP_EMPTY) != 0u;
	const uint32_t col_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)col;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;

	bool done = !have;                               /* no further match in this input */
	bool seek = true;                                /* the lane looks for the next mark at or after p; else it is in an attempt */
	uint64_t p = 0;                                  /* the cursor; in an attempt: its start */
	uint64_t t = 0;                                  /* bytes of the attempt walked in earlier chunks */
	uint64_t acc = FSM_HIP_NO_POS;                   /* the attempt's last accept: bytes from p (0: the start state's own) */
	uint32_t accs = 0;                               /* ... and the state there */
	uint32_t s = a.start;
	uint64_t nmatch = 0;

	for (;;) {
		if (!__any(!done)) break;
		if (!done && seek) {                         /* the next marked position at or after p: sixteen positions a load */
			for (;;) {
				if (p > len) { done = true; break; }
				const uint64_t at = region + (p >> 4);
				const uint32_t word = at < a.nwords ? (uint32_t)marks[at] : 0u;
				const uint64_t nx = marks_next_in_word(word, p, len);       /* in [p, len]: a bit behind len is not taken */
				if (nx != MARKS_NONE) {
					p = nx;
					break;
				}
				p = (p & ~(uint64_t)15u) + 16u;
			}
			seek = false;
			t = 0;
			s = a.start;
			const bool ends0 = (s & end_bit) != 0u;  /* e = start counts: an empty match */
			acc = ends0 ? 0u : FSM_HIP_NO_POS;
			accs = s;
		}
		const bool live = !done;
		const uint64_t left = live && p + t < len ? len - p - t : 0u;   /* (p + t <= len in an attempt; it never wraps) */
		const bool sunk = (s & ~end_bit) >= absorbing;   /* (only a start state can be: an attempt that sank was closed) */
		const uint32_t cnt = !live || sunk ? 0u : left < 16u ? (uint32_t)left : 16u;
		u32x4m v = {0u, 0u, 0u, 0u};
		if (cnt != 0u) {
			const uint64_t at = beg + p + t;             /* the chunk's first byte, from base */
			if (at + 16u <= limit) {
				v = *(g_chunkp)(base + at);
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(base + at))[k] << ((k & 3u) * 8u);
				v = u32x4m{d[0], d[1], d[2], d[3]};
			}
		}
		uint32_t c2[16];
#pragma unroll
		for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(col_at + match_byte_at(v, k) * 2u);
		uint32_t acck = 0;                           /* bytes of this chunk at the last accept in it (0: none) */
		uint32_t as = accs;
		if (in_lds) {
			if (__all(cnt == 16u || !live)) {        /* whole chunks everywhere */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					sn = *(l_u16p)(uintptr_t)(tab_at + (sn & 0xfffeu) + c2[k]);
					const bool hit = (sn & 1u) != 0u;
					as = hit ? sn : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
				}
				s = live ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + (s & 0xfffeu) + c2[k]);
					const bool in = (uint32_t)k < cnt;
					const bool hit = in && (sn & 1u) != 0u;
					s = in ? sn : s;
					as = hit ? sn : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)k < cnt) {
					s = dense[(uint64_t)(s & 0x7fffffffu) * C + c2[k]];
					const bool hit = (s >> 31) != 0u;
					as = hit ? s : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
				}
			}
		}
		if (live) {
			if (acck != 0u) { acc = t + acck; accs = as; }
			const bool absorbed = (s & ~end_bit) >= absorbing, s_ends = (s & end_bit) != 0u;
			if (absorbed || cnt == left) {           /* the walk stopped: close the attempt */
				uint64_t e = acc;                        /* the match's bytes; NO_POS: none */
				uint32_t q = accs;
				if (absorbed && s_ends) {                /* an absorbing end state accepts at every later position */
					q = s;
					e = len - p;
				}
				if (e == FSM_HIP_NO_POS) {
					done = true;                         /* a hit without a span stays without one */
				} else {
					if (!(drop_empty && e == 0u)) {
						if (EMIT && nmatch < cap) {
							start_out[out_at + nmatch] = p;
							end_out[out_at + nmatch] = p + e;
							id_out[out_at + nmatch] = ids[in_lds ? q >> 1 : q & 0x7fffffffu];
						}
						nmatch++;
					}
					p += e != 0u ? e : 1u;               /* behind the match; an empty one: a byte on */
					seek = true;
				}
			} else {
				t += 16u;
			}
		}
	}
	if (!EMIT && valid) ((g_u64w)(uintptr_t)a.count)[j] = nmatch;
}

MatchArgs args_of(const MatchRun &r)
{
	MatchArgs a;
	a.tab = nullptr;
	a.col = nullptr;
	a.ids = nullptr;
	a.base = static_cast<const uint8_t *>(r.in.base);
	a.off = r.in.off;
	a.pick = r.in.pick;
	a.marks = r.marks;
	a.count = r.count;
	a.match_off = r.match_off;
	a.start_out = r.start_out;
	a.end_out = r.end_out;
	a.id_out = r.id_out;
	a.n = r.in.n;
	a.m = r.in.m;
	a.limit = r.in.limit;
	a.nwords = r.nwords;
	a.entries = a.C = a.start = a.abs_min = a.in_lds = 0;
	a.flags = r.in.flags;
	a.trim = r.in.trim;
	return a;
}

}   // namespace

namespace fsmhip {

/* walk_mark on stream s, the image's device current; 0, or -1 + errno */
static int match_launch_mark(const fsm_hip_pos_dfa *starts, const MatchRun &r, hipStream_t s)
{
	if (r.in.m == 0) return 0;
	if (!match_grid_fits(r.in.m)) { errno = ENOMEM; return -1; }
	const PosView v = pos_dfa_view(starts);
	if (v.in_lds != 0u && v.entries > MATCH_LDS_ENTRIES) { errno = EINVAL; return -1; }
	MatchArgs a = args_of(r);
	a.tab = v.tab;
	a.col = v.col;
	a.entries = v.entries;
	a.C = v.C;
	a.start = v.start;
	a.abs_min = v.abs_min;
	a.in_lds = v.in_lds;
	const dim3 grid((unsigned)((r.in.m + MATCH_THREADS - 1u) / MATCH_THREADS)), block(MATCH_THREADS);
	hipLaunchKernelGGL(walk_mark, grid, block, 0, s, a);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

/* walk_match<emit> */
static int match_launch(const fsm_hip_tok_dfa *ends, const MatchRun &r, bool emit, hipStream_t s)
{
	if (r.in.m == 0) return 0;
	if (!match_grid_fits(r.in.m)) { errno = ENOMEM; return -1; }
	const TokView v = tok_dfa_view(ends);
	if (v.in_lds != 0u && v.entries > MATCH_LDS_ENTRIES) { errno = EINVAL; return -1; }
	MatchArgs a = args_of(r);
	a.tab = v.tab;
	a.col = v.col;
	a.ids = v.ids;
	a.entries = v.entries;
	a.C = v.C;
	a.start = v.start;
	a.abs_min = v.abs_min;
	a.in_lds = v.in_lds;
	const dim3 grid((unsigned)((r.in.m + MATCH_THREADS - 1u) / MATCH_THREADS)), block(MATCH_THREADS);
	if (emit) hipLaunchKernelGGL(walk_match<true>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(walk_match<false>, grid, block, 0, s, a);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

}   // namespace fsmhip

/* ---- the matches object (match.h): marks pass -> count pass -> scan -> ONE wait for the total -> allocation -> emit pass --------- */
extern "C" void fsm_hip_matches_free(struct fsm_hip_matches *mt) { run_free(mt); }

/* the passes on stream s into *mt, the images' device current; r: the inputs, their limit given (its outputs are set here) */
static int matches_passes(struct fsm_hip_matches *mt, const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends, fsmhip::MatchRun r,
	hipStream_t s)
{
	const uint64_t m = r.in.m;
	uint64_t total = 0;
	if (!HIP_OK(mt->d_off.alloc(m + 1u))) return -1;
	r.nwords = fsmhip::marks_words(r.in.limit, r.in.n);
	if (m != 0 && !HIP_OK(mt->d_marks.alloc(r.nwords))) return -1;
	r.marks = mt->d_marks;
	r.count = mt->d_off;
	if (!mt->begin(0, s)) return -1;
	if (m != 0 && fsmhip::match_launch_mark(starts, r, s) != 0) return -1;
	if (!mt->end(0, s) || !mt->begin(1, s)) return -1;
	if (m != 0 && fsmhip::match_launch(ends, r, false, s) != 0) return -1;
	if (!mt->end(1, s) || !mt->begin(2, s)) return -1;
	if (scan_total(mt->d_off, m, mt->ev[5], s, &total) != 0) return -1;   /* the total sizes the arrays */
	mt->total = (size_t)total;
	if (total != 0 && (!HIP_OK(mt->d_start.alloc(total)) || !HIP_OK(mt->d_end.alloc(total)) || !HIP_OK(mt->d_id.alloc(total)))) return -1;
	if (!mt->begin(3, s)) return -1;
	if (total != 0) {
		r.match_off = mt->d_off;
		r.start_out = mt->d_start;
		r.end_out = mt->d_end;
		r.id_out = mt->d_id;
		if (fsmhip::match_launch(ends, r, true, s) != 0) return -1;
	}
	return mt->end(3, s) ? 0 : -1;
}

static struct fsm_hip_matches *matches_new(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends, const fsmhip::LineBatch &in,
	hipStream_t s)
{
	fsmhip::MatchRun r;
	r.in = in;
	return run_new<struct fsm_hip_matches>(fsmhip::tok_dfa_device(ends), in.m, fsmhip::match_grid_fits(in.m), s,
	                                       [&](struct fsm_hip_matches *mt) { return matches_passes(mt, starts, ends, r, s); });
}

/* the arguments both forms refuse alike; *in: the batch as given */
static bool matches_check(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends, const struct fsm_hip_match_batch *b,
	fsmhip::LineBatch *in)
{
	if (!have_device()) { errno = ENODEV; return false; }
	if (starts == nullptr || ends == nullptr || fsmhip::pos_dfa_device(starts) != fsmhip::tok_dfa_device(ends)) { errno = EINVAL; return false; }
	return fsmhip::batch_shape(b, FSM_HIP_MATCHES_DROP_EMPTY, in);
}

extern "C" struct fsm_hip_matches *fsm_hip_matches_run_device(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_match_batch *b, void *hip_stream)
{
	fsmhip::LineBatch in;
	if (!matches_check(starts, ends, b, &in) || !fsmhip::batch_device_ok(in)) return nullptr;
	DevGuard dg(fsmhip::tok_dfa_device(ends));
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (!fsmhip::batch_read_limit(&in, s)) return nullptr;   /* the marks are sized by the limit */
	return matches_new(starts, ends, in, s);
}

extern "C" struct fsm_hip_matches *fsm_hip_matches_run(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_match_batch *b)
{
	fsmhip::LineBatch host;
	if (!matches_check(starts, ends, b, &host) || !fsmhip::batch_host_arrays_ok(host)) return nullptr;
	return run_host(fsmhip::tok_dfa_device(ends), host, [&](const fsmhip::LineBatch &in, hipStream_t s) { return matches_new(starts, ends, in, s); });
}

extern "C" struct fsm_hip_matches *fsm_hip_text_matches(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_text *t, const struct fsm_hip_text_hits *h, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (starts == nullptr || ends == nullptr || t == nullptr || (flags & ~FSM_HIP_MATCHES_DROP_EMPTY) != 0u) { errno = EINVAL; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	std::optional<DevGuard> dg;
	fsmhip::LineBatch in;
	if (!text_batch(t, h, {fsmhip::pos_dfa_device(starts), fsmhip::tok_dfa_device(ends)}, s, &dg, &in)) return nullptr;
	in.flags = flags;
	return matches_new(starts, ends, in, s);
}

extern "C" size_t fsm_hip_matches_count(const struct fsm_hip_matches *mt) { return mt == nullptr ? 0 : mt->m; }
extern "C" size_t fsm_hip_matches_total(const struct fsm_hip_matches *mt) { return mt == nullptr ? 0 : mt->total; }
extern "C" const uint64_t *fsm_hip_matches_off_device(const struct fsm_hip_matches *mt) { return mt == nullptr ? nullptr : mt->d_off.p; }
extern "C" const uint64_t *fsm_hip_matches_start_device(const struct fsm_hip_matches *mt) { return mt == nullptr ? nullptr : mt->d_start.p; }
extern "C" const uint64_t *fsm_hip_matches_end_device(const struct fsm_hip_matches *mt) { return mt == nullptr ? nullptr : mt->d_end.p; }
extern "C" const uint32_t *fsm_hip_matches_id_device(const struct fsm_hip_matches *mt) { return mt == nullptr ? nullptr : mt->d_id.p; }

extern "C" int fsm_hip_matches_copy(const struct fsm_hip_matches *mt, uint64_t *off, uint64_t *start, uint64_t *end, uint32_t *id)
{
	if (mt == nullptr) { errno = EINVAL; return -1; }
	return copy_out(mt->device, mt->done(), {{off, mt->d_off, (mt->m + 1u) * sizeof(uint64_t)}, {start, mt->d_start, mt->total * sizeof(uint64_t)},
	                                         {end, mt->d_end, mt->total * sizeof(uint64_t)}, {id, mt->d_id, mt->total * sizeof(uint32_t)}});
}

extern "C" double fsm_hip_matches_ms(const struct fsm_hip_matches *mt) { return run_ms(mt, 0, 3); }
extern "C" double fsm_hip_matches_pass_ms(const struct fsm_hip_matches *mt, int pass) { return run_ms(mt, pass, pass); }
