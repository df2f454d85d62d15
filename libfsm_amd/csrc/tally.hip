/*
 * tally.hip -- counts of entries and of inputs per group and per column, on the device: a histogram over the id[total] and the
 * off[m + 1] that a matches or a tokens object owns.  include/fsm_hip.h, section "tally", is the definition; tally_seg.h holds
 * the arithmetic, shared with tests/c/test_tally_seg.cpp.
 *
 * One kernel, tally_spans.  A workgroup takes a contiguous span of INPUTS -- `per` granules of TALLY_SPAN -- so every input lies
 * inside one workgroup, and goes through the span's entries [off[j0], off[j1]) in windows of TALLY_WINDOW, one lane per entry:
 *     two wavefronts find the inputs of the window's first and last entry in off, each by a 64-ary search -- 64 probes a round, a
 *     ballot, three dependent loads for a span of 38 000 inputs where two lanes' binary searches took fifteen -- and their first
 *     lanes the positions of those two inputs in group_off;
 *     the offsets between the two inputs are staged in LDS when they are at most TALLY_STAGE, and every lane finds its own input
 *     among them (the last j with off[j] <= k: inputs without entries, which share their offset with their successor, are
 *     stepped over), and, only where the window spans a group boundary, its own group;
 *     count: +1 at (group, col(id[k]));
 *     lines: +1 at (group, column) iff no earlier entry of the same input has the column.  Inside the window that is a look
 *     backwards through the window's (input, column) pairs in LDS, which stops at the first other input.  Only the window's first
 *     input can have begun before the window: for it there is a bitmap of the columns it has shown, kept in LDS by the entries
 *     of each window's LAST input with an atomic OR that returns the old word (tally_seg.h, tally_carry).
 * Where the adds go: while the columns fit (C <= TALLY_LDS_COLS) and the whole window lies in ONE group, into u32 counters in LDS,
 * which are flushed into the u64 tables -- one device-scope atomic add per non-zero bin -- when the group changes, at the end of
 * the span and before a counter could wrap.  Above the cap only the LAST column, "other", has such a counter -- the one column that
 * is hot whatever the rules are: states without an id, rules beyond nrules, the bad bytes of SKIP_BAD -- and every other entry, like
 * every entry of a window that spans a group boundary, adds straight to the tables.  Either way a wavefront first combines equal
 * destinations: the destination of the first lane that is left is broadcast, the lanes that share it are counted by a ballot and
 * one of them adds the count; two such rounds before LDS adds and eight before adds to the tables, where 64 adds to one address
 * cost most, then every lane that is left adds for itself.  One rule with 64 M matches is then one LDS add per wavefront and
 * window, not 64 to one bank; a bin that a third of the entries hit is met by one of eight first lanes in 97 of 100 wavefronts.
 * Every global access names its address space (no FLAT instruction), integer adds only: the result is exact and the same on
 * every run.  Loads stay inside off[0 .. m], id[0 .. total), group_off[0 .. G]; a store goes to (g, c) with g < G and c < C only.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "hip_host.h"
#include "tally.h"
#include "tally_seg.h"

using namespace fsmhip;

namespace {

typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
typedef uint64_t __attribute__((address_space(1))) *g_u64w;

constexpr uint32_t TALLY_STAGE = 2u * TALLY_THREADS;                /* offsets of a window's inputs held in LDS: two a lane */
constexpr uint32_t ROUNDS_LDS = 2, ROUNDS_TABLE = 8;                /* rounds of wave_add before every lane adds for itself */
constexpr uint32_t TALLY_WRAP_GUARD = 0xffffffffu - TALLY_WINDOW;   /* entries a counter may have seen before the next window */

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

/* ext_last_le by the whole wavefront (tally_seg.h, tally_kary_*): lo and hi are the same in every lane */
__device__ __forceinline__ uint64_t wave_last_le(g_u64p a, uint64_t lo, uint64_t hi, uint64_t p)
{
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
	while (lo < hi) {
		const uint32_t c = (uint32_t)__builtin_popcountll(__ballot(a[tally_kary_probe(lo, hi, lane)] <= p));
		tally_kary_narrow(&lo, &hi, c);
	}
	return lo;
}

/* +1 at `key` for every lane that is `on`, equal keys of the wavefront combined: ROUNDS rounds of "the first lane left names its
 * key, a ballot counts the lanes that share it, that lane adds the count", then one add per lane that is left */
template <uint32_t ROUNDS, typename Add>
__device__ __forceinline__ void wave_add(bool on, uint64_t key, Add add)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t rem = __ballot(on);
#pragma unroll 1
	for (uint32_t r = 0; r < ROUNDS && rem != 0u; r++) {
		const uint32_t src = (uint32_t)__builtin_ctzll(rem);
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, (int)src);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), (int)src);
		const bool mine = on && key == ((uint64_t)hi << 32 | lo);
		const uint64_t same = __ballot(mine);
		if (lane == src) add(key, (uint32_t)__builtin_popcountll(same));
		on = on && !mine;
		rem &= ~same;
	}
	if (on) add(key, 1u);
}

__device__ __forceinline__ void table_add(uint64_t *table, uint64_t at, uint64_t v)
{
	(void)__hip_atomic_fetch_add((g_u64w)(uintptr_t)table + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TALLY_THREADS)
tally_spans(const TallyRun a)
{
	__shared__ uint32_t cnt[TALLY_LDS_COLS];         /* the partial counts of group `gcur`: of every column, or ([0]) of the last */
	__shared__ uint32_t lin[TALLY_LDS_COLS];
	__shared__ uint32_t seen[TALLY_LINE_COLS / 32u]; /* the columns the carried input has shown */
	__shared__ uint64_t win_j[TALLY_WINDOW];
	__shared__ uint32_t win_c[TALLY_WINDOW];
	__shared__ uint64_t stage[TALLY_STAGE];          /* off[jf .. jl] of the window */
	__shared__ uint64_t ends[2][4];                  /* by the window's parity: the inputs of its two ends, their positions */

	const uint32_t tid = threadIdx.x;
	const g_u64p off = (g_u64p)(uintptr_t)a.off, goff = (g_u64p)(uintptr_t)a.group_off;
	const g_u32p id = (g_u32p)(uintptr_t)a.id;
	const uint64_t G = a.ngroups, C = a.nrules + 1u;
	const bool want_count = a.count != nullptr, want_lines = a.lines != nullptr;
	const bool in_lds = C <= TALLY_LDS_COLS;
	const uint32_t nwords = want_lines ? tally_bit_words(C) : 0u;     /* (the front has held C to TALLY_LINE_COLS) */

	const uint64_t j0 = (uint64_t)blockIdx.x * a.per * TALLY_SPAN;    /* below m: the launch's grid */
	const uint64_t j1 = min64(j0 + a.per * TALLY_SPAN, a.m);
	const uint64_t k0 = tally_clamp(off[j0], a.total);
	uint64_t k1 = tally_clamp(off[j1], a.total);
	if (k1 < k0) k1 = k0;

	const uint32_t nslots = in_lds ? (uint32_t)C : 1u;                /* counters in LDS; slot s is column s, or the last column */
	for (uint32_t c = tid; c < nslots; c += TALLY_THREADS) cnt[c] = lin[c] = 0u;
	for (uint32_t w = tid; w < nwords; w += TALLY_THREADS) seen[w] = 0u;
	__syncthreads();

	/* the partial counts into the tables' row g, and cleared; between two barriers */
	auto flush = [&](uint64_t g) {
		__syncthreads();
		if (g != TALLY_NONE) {
			for (uint32_t c = tid; c < nslots; c += TALLY_THREADS) {
				const uint32_t x = cnt[c], y = lin[c];
				const uint64_t at = g * C + (in_lds ? (uint64_t)c : a.nrules);
				if (x != 0u) { table_add(a.count, at, x); cnt[c] = 0u; }
				if (y != 0u) { table_add(a.lines, at, y); lin[c] = 0u; }
			}
		}
		__syncthreads();
	};

	uint64_t gcur = TALLY_NONE, carried = TALLY_NONE, since = 0;      /* all the same in every lane */
	uint64_t jlo = j0, plo = 0;
	uint32_t par = 0;
#pragma unroll 1
	for (uint64_t w = k0; w < k1; w += TALLY_WINDOW, par ^= 1u) {
		const uint64_t wend = min64(w + TALLY_WINDOW, k1);
		if (tid < 128u) {                            /* wavefront 0: the first entry's input, wavefront 1: the last entry's */
			const uint32_t which = tid >> 6;
			const uint64_t j = wave_last_le(off, jlo, j1 - 1u, which == 0u ? w : wend - 1u);
			if ((tid & 63u) == 0u) {
				ends[par][which] = j;
				ends[par][2u + which] = a.group_off != nullptr ? tally_group_pos(goff, j, plo, G + 1u) : 1u;
			}
		}
		__syncthreads();
		const uint64_t jf = ends[par][0], jl = ends[par][1], pf = ends[par][2], pl = ends[par][3];
		const bool staged = jl >= jf && jl - jf < TALLY_STAGE;
		if (staged) {                                /* (the barrier behind it is the one before `stage` is written again, too) */
			for (uint64_t x = tid; x <= jl - jf; x += TALLY_THREADS) stage[x] = off[jf + x];
			__syncthreads();
		}
		const uint64_t k = w + tid;
		const bool active = k < wend;
		uint64_t j = jf, c = 0, pos = pf;
		if (active) {
			j = staged ? jf + ext_last_le(stage, 0u, jl - jf, k) : ext_last_le(off, jf, jl, k);
			c = tally_col(id[k], a.nrules);
			if (pf != pl) pos = tally_group_pos(goff, j, pf, pl);     /* pl <= G + 1: reads group_off[pf .. pl - 1] */
		}
		const bool valid = active && tally_pos_counts(pos, G);
		const uint64_t g = pos - 1u;
		const bool one_group = pf == pl;             /* the whole window in one group, or counted nowhere */
		const bool to_lds = one_group && (in_lds || c == a.nrules);
		const uint64_t slot = in_lds ? c : 0u;
		if (one_group && tally_pos_counts(pf, G)) {
			if (pf - 1u != gcur || since > TALLY_WRAP_GUARD) {
				flush(gcur);
				gcur = pf - 1u;
				since = 0;
			}
			since += TALLY_WINDOW;
		}
		if (want_count) {
			wave_add<ROUNDS_LDS>(valid && to_lds, slot, [&](uint64_t key, uint32_t v) { atomicAdd(&cnt[(uint32_t)key], v); });
			wave_add<ROUNDS_TABLE>(valid && !to_lds, g * C + c, [&](uint64_t key, uint32_t v) { table_add(a.count, key, v); });
		}
		if (want_lines) {
			win_j[tid] = active ? j : TALLY_NONE;
			win_c[tid] = (uint32_t)c;
			__syncthreads();
			const bool first = active && tally_window_first(win_j, win_c, tid);
			const TallyCarry cy = tally_carry(jf, jl, carried);
			const uint32_t word = tally_bit_word((uint32_t)c), bit = tally_bit_mask((uint32_t)c);
			bool counts = first;
			if (first && j == jf && jf != jl) counts = !cy.carry_in || (seen[word] & bit) == 0u;
			if (cy.clear) {
				__syncthreads();
				for (uint32_t x = tid; x < nwords; x += TALLY_THREADS) seen[x] = 0u;
				__syncthreads();
			}
			if (first && j == jl) counts = (atomicOr(&seen[word], bit) & bit) == 0u;
			carried = jl;
			counts = counts && valid;
			wave_add<ROUNDS_LDS>(counts && to_lds, slot, [&](uint64_t key, uint32_t v) { atomicAdd(&lin[(uint32_t)key], v); });
			wave_add<ROUNDS_TABLE>(counts && !to_lds, g * C + c, [&](uint64_t key, uint32_t v) { table_add(a.lines, key, v); });
		}
		jlo = jl;
		plo = pl;
	}
	flush(gcur);
}

}   // namespace

namespace fsmhip {

int tally_launch(TallyRun r, int device, hipStream_t s)
{
	if (r.m == 0 || r.total == 0) return 0;
	int ncu = 0;
	if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
	const uint64_t granules = (r.m + TALLY_SPAN - 1u) / TALLY_SPAN;
	uint64_t wgs = (uint64_t)ncu * TALLY_WG_PER_CU;
	if (wgs > granules) wgs = granules;
	r.per = (granules + wgs - 1u) / wgs;
	wgs = (granules + r.per - 1u) / r.per;           /* none without an input */
	hipLaunchKernelGGL(tally_spans, dim3((unsigned)wgs), dim3(TALLY_THREADS), 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

}   // namespace fsmhip
