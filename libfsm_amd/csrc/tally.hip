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

#include "../../include/fsm_hip.h"
#include "front.h"
#include "match.h"
#include "tally_seg.h"
#include "text_objects.h"
#include "tok.h"

namespace fsmhip {

constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_WINDOW = TALLY_THREADS;            /* entries a workgroup takes a step, one per lane */
constexpr uint32_t TALLY_SPAN = 64;                         /* inputs of a granule: a workgroup takes whole granules */
constexpr uint32_t TALLY_LDS_COLS = 4096;                   /* columns counted in LDS: 2 x 16 KiB of u32, count and lines */
constexpr uint32_t TALLY_LINE_COLS = 65536;                 /* columns of the bitmap of one input: 8 KiB of LDS */
constexpr uint32_t TALLY_WG_PER_CU = 3;                     /* 47 KiB of LDS a workgroup: three fit a CU's 160 KiB */

/* the kernel's arguments; every pointer is device memory.  count or lines may be null, not both; group_off null: one group. */
struct TallyRun {
	const uint64_t *off = nullptr;           /* m + 1 */
	const uint32_t *id = nullptr;            /* total */
	uint64_t m = 0, total = 0;
	const uint64_t *group_off = nullptr;     /* ngroups + 1, or null */
	uint64_t ngroups = 1;
	uint64_t nrules = 0;                     /* nrules + 1 columns */
	uint64_t *count = nullptr, *lines = nullptr;   /* ngroups * (nrules + 1) each */
	uint64_t per = 1;                        /* granules of a workgroup; set by the launch */
};

}

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

/* on stream s, `device` current; m >= 1 and total >= 1.  0, or -1 + errno */
static int tally_launch(TallyRun r, int device, hipStream_t s)
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

/* ---- the fronts ---------------------------------------------------------------------------------------------------------------
 * Nothing is owned and nothing waits in the device forms: the tables are the caller's, cleared on the stream unless
 * FSM_HIP_TALLY_ADD is given, then ONE launch.  The host forms stage group_off and the tables on a stream of their own and wait. */
extern "C" size_t fsm_hip_tally_span_inputs(void) { return fsmhip::TALLY_SPAN; }
extern "C" size_t fsm_hip_tally_window(void) { return fsmhip::TALLY_WINDOW; }
extern "C" size_t fsm_hip_tally_lds_columns(void) { return fsmhip::TALLY_LDS_COLS; }
extern "C" size_t fsm_hip_tally_max_line_columns(void) { return fsmhip::TALLY_LINE_COLS; }

/* what every form refuses about the shape alike, behind ENODEV and the form's own EINVALs; *cells = G * C */
static bool tally_shape(const void *group_off, size_t *ngroups, size_t nrules, unsigned flags, const void *count, const void *lines, size_t *cells)
{
	if ((count == nullptr && lines == nullptr) || (flags & ~FSM_HIP_TALLY_ADD) != 0u || (group_off != nullptr && *ngroups == 0)) { errno = EINVAL; return false; }
	if (group_off == nullptr) *ngroups = 1;
	if (nrules == SIZE_MAX || *ngroups > SIZE_MAX / sizeof(uint64_t) / (nrules + 1u)) { errno = EOVERFLOW; return false; }
	if (lines != nullptr && nrules + 1u > fsmhip::TALLY_LINE_COLS) { errno = ENOTSUP; return false; }
	*cells = *ngroups * (nrules + 1u);
	return true;
}

/* the reduction on stream s, `device` current, behind tally_shape: the tables cleared unless they are added to, then the launch */
static int tally_run(int device, const uint64_t *d_off, const uint32_t *d_id, size_t m, size_t total, const uint64_t *d_group_off, size_t ngroups,
	size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, size_t cells, hipStream_t s)
{
	if ((flags & FSM_HIP_TALLY_ADD) == 0u)
		for (uint64_t *tab : {d_count, d_lines})
			if (tab != nullptr && !HIP_OK(hipMemsetAsync(tab, 0, cells * sizeof(uint64_t), s))) return -1;
	fsmhip::TallyRun r;
	r.off = d_off;
	r.id = d_id;
	r.m = m;
	r.total = total;
	r.group_off = d_group_off;
	r.ngroups = ngroups;
	r.nrules = nrules;
	r.count = d_count;
	r.lines = d_lines;
	return fsmhip::tally_launch(r, device, s);
}

extern "C" int fsm_hip_tally_ids_device(const uint64_t *d_off, const uint32_t *d_id, size_t m, size_t total, const uint64_t *d_group_off,
	size_t ngroups, size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	int dev = 0;
	size_t cells = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return -1; }
	if ((d_off == nullptr && m != 0) || (d_id == nullptr && m != 0 && total != 0)) { errno = EINVAL; return -1; }
	if (!tally_shape(d_group_off, &ngroups, nrules, flags, d_count, d_lines, &cells)) return -1;
	return tally_run(dev, d_off, d_id, m, total, d_group_off, ngroups, nrules, flags, d_count, d_lines, cells, static_cast<hipStream_t>(hip_stream));
}

/* the device form of an object's own arrays (a matches or a tokens object: both have device, m, total, d_off, d_id, done()) */
template <typename T>
static int tally_object_device(const T *o, const uint64_t *d_group_off, size_t ngroups, size_t nrules, unsigned flags, uint64_t *d_count,
	uint64_t *d_lines, void *hip_stream)
{
	size_t cells = 0;
	if (!have_device()) { errno = ENODEV; return -1; }
	if (o == nullptr) { errno = EINVAL; return -1; }
	if (!tally_shape(d_group_off, &ngroups, nrules, flags, d_count, d_lines, &cells)) return -1;
	DevGuard dg(o->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (!HIP_OK(hipStreamWaitEvent(s, o->done(), 0))) return -1;      /* behind the object's emit pass */
	return tally_run(o->device, o->d_off, o->d_id, o->m, o->total, d_group_off, ngroups, nrules, flags, d_count, d_lines, cells, s);
}

/* the host form: group_off checked and staged, the tables made on the device (uploaded when they are added to), the device form
 * on a stream of its own, the tables read back, ONE wait */
template <typename T>
static int tally_object_host(const T *o, const uint64_t *group_off, size_t ngroups, size_t nrules, unsigned flags, uint64_t *count, uint64_t *lines)
{
	size_t cells = 0;
	if (!have_device()) { errno = ENODEV; return -1; }
	if (o == nullptr) { errno = EINVAL; return -1; }
	if (!tally_shape(group_off, &ngroups, nrules, flags, count, lines, &cells)) return -1;
	if (group_off != nullptr) {
		for (size_t g = 0; g < ngroups; g++)
			if (group_off[g] > group_off[g + 1u]) { errno = EINVAL; return -1; }
		if (group_off[ngroups] > o->m) { errno = EINVAL; return -1; }
	}
	DevGuard dg(o->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	DevStream own;
	if (!HIP_OK(own.create(hipStreamNonBlocking))) return -1;
	DevBuf<uint64_t> d_goff, d_tab[2];
	uint64_t *host[2] = {count, lines};
	int rc = 0;
	if (group_off != nullptr && (!HIP_OK(d_goff.alloc(ngroups + 1u)) ||
	                             !HIP_OK(hipMemcpyAsync(d_goff.p, group_off, (ngroups + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, own))))
		rc = -1;
	for (int i = 0; i < 2 && rc == 0; i++) {
		if (host[i] == nullptr) continue;
		if (!HIP_OK(d_tab[i].alloc(cells))) rc = -1;
		else if ((flags & FSM_HIP_TALLY_ADD) != 0u && !HIP_OK(hipMemcpyAsync(d_tab[i].p, host[i], cells * sizeof(uint64_t), hipMemcpyHostToDevice, own))) rc = -1;
	}
	if (rc == 0 && !HIP_OK(hipStreamWaitEvent(own, o->done(), 0))) rc = -1;
	if (rc == 0) rc = tally_run(o->device, o->d_off, o->d_id, o->m, o->total, d_goff.p, ngroups, nrules, flags, d_tab[0].p, d_tab[1].p, cells, own);
	for (int i = 0; i < 2 && rc == 0; i++)
		if (host[i] != nullptr && !HIP_OK(hipMemcpyAsync(host[i], d_tab[i].p, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, own))) rc = -1;
	const int e = errno;
	const bool idle = HIP_OK(hipStreamSynchronize(own));                /* also when a step failed: the staged arrays go at return */
	if (rc != 0) { errno = e; return -1; }
	return idle ? 0 : -1;
}

/* the text form: the groups are the text's files -- file_lines, or the hits' file_first -- and a plain text is one group */
template <typename T>
static int tally_object_text(const T *o, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *h, size_t nrules, unsigned flags,
	uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	size_t cells = 0;
	if (!have_device()) { errno = ENODEV; return -1; }
	if (o == nullptr || t == nullptr || o->m != (h != nullptr ? h->m : t->n) || o->device != t->device || (h != nullptr && h->device != t->device)) {
		errno = EINVAL;
		return -1;
	}
	const uint64_t *d_goff = t->nfiles == 0 ? nullptr : h != nullptr ? h->d_file_first.p : t->d_file_lines.p;
	size_t ngroups = t->nfiles;
	if (t->nfiles != 0 && d_goff == nullptr) { errno = EINVAL; return -1; }   /* hits of another, plain text */
	if (!tally_shape(d_goff, &ngroups, nrules, flags, d_count, d_lines, &cells)) return -1;
	DevGuard dg(t->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (!HIP_OK(hipStreamWaitEvent(s, h != nullptr ? h->ev[5] : t->ev[3], 0)) || !HIP_OK(hipStreamWaitEvent(s, o->done(), 0))) return -1;
	return tally_run(o->device, o->d_off, o->d_id, o->m, o->total, d_goff, ngroups, nrules, flags, d_count, d_lines, cells, s);
}

extern "C" int fsm_hip_matches_tally_device(const struct fsm_hip_matches *mt, const uint64_t *d_group_off, size_t ngroups, size_t nrules,
	unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	return tally_object_device(mt, d_group_off, ngroups, nrules, flags, d_count, d_lines, hip_stream);
}

extern "C" int fsm_hip_tokens_tally_device(const struct fsm_hip_tokens *tk, const uint64_t *d_group_off, size_t ngroups, size_t nrules,
	unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	return tally_object_device(tk, d_group_off, ngroups, nrules, flags, d_count, d_lines, hip_stream);
}

extern "C" int fsm_hip_matches_tally(const struct fsm_hip_matches *mt, const uint64_t *group_off, size_t ngroups, size_t nrules, unsigned flags,
	uint64_t *count, uint64_t *lines)
{
	return tally_object_host(mt, group_off, ngroups, nrules, flags, count, lines);
}

extern "C" int fsm_hip_tokens_tally(const struct fsm_hip_tokens *tk, const uint64_t *group_off, size_t ngroups, size_t nrules, unsigned flags,
	uint64_t *count, uint64_t *lines)
{
	return tally_object_host(tk, group_off, ngroups, nrules, flags, count, lines);
}

extern "C" int fsm_hip_text_matches_tally(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits,
	size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	return tally_object_text(mt, t, hits, nrules, flags, d_count, d_lines, hip_stream);
}

extern "C" int fsm_hip_text_tokens_tally(const struct fsm_hip_tokens *tk, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits,
	size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream)
{
	return tally_object_text(tk, t, hits, nrules, flags, d_count, d_lines, hip_stream);
}
