/*
 * multi.hip -- the many-DFA front: K automata, each with its own packed lines and outputs, ONE submission.
 *
 * The reference's batched driver compiles a DFA per record and runs a handful of lines through it
 * (src/retest/main.c:1056-1058 fsm_runner_initialize + fsm_free, :1114 fsm_runner_run; tests/retest/ *.tst:
 * 37 DFAs x ~3 lines).  One table upload + one launch per DFA is 37 x (a dozen synchronous copies + >= 23 us
 * of launch latency) for microseconds of walking.  Here every job that is small rides in ONE host-to-device
 * copy -- descriptors, the automata's plain tables (Plan::dense, the dfa_table form of src/libfsm/vm/ir.c:649-750:
 * next state per byte class, missing edge = DEAD), offsets and lines -- ONE kernel whose workgroups map to
 * (dfa, tile of 64 lines), and ONE copy back.  A job too big for that (more than MULTI_FUSE_LINES lines or
 * MULTI_FUSE_BYTES bytes) goes through its dfa's own walk kernels, enqueued beside the fused launch.
 *
 * The walk is fsm_exec's (src/libfsm/exec.c:132-151): state = table[state][class(byte)] from the start state;
 * a lane stops at an absorbing state (DEAD = the missing edge, exec.c:133-138, or an accept-everything state),
 * end_out = fin[state] (the caller's state id, or NO_MATCH when the final state is not an end state, :153-155).
 *
 * Eager-output sets (exec.c:126-144: the ids of the start state and of every state entered) are delivered by the same
 * submission to the jobs that ask for them (fsm_hip_exec_multi_eager*): the automata's eager masks ride in the one copy, and
 * the fused launch is then walk_multi_eager -- a submission in which no job asks launches walk_multi, as before.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/fsm_hip.h"
#include "dfa_access.h"
#include "image.h"
#include "hip_host.h"

using namespace fsmhip;

namespace {

constexpr uint32_t MULTI_LDS_ENTRIES = 16384;          /* a table of up to this many (state, class) entries is walked from LDS (u16 row offsets) */
constexpr size_t MULTI_FUSE_LINES = 65536, MULTI_FUSE_BYTES = (size_t)1 << 20, MULTI_FUSE_TABLE = (size_t)1 << 20;
constexpr uint32_t MULTI_EAGER_WORDS = 16;                /* eager-output sets of up to this many 64-bit words (1 024 ids) are collected by the fused kernel */
constexpr size_t MULTI_STAGE_CAP = (size_t)64 << 20;   /* one submission's staging; what does not fit goes the per-dfa way */

struct MultiJob {
	const uint32_t *dense;   /* [S1][C] next (renumbered) state */
	const uint32_t *cls4;    /* [64] byte -> class, four to a word */
	const uint32_t *fin;     /* [S1] caller's end state id or NO_MATCH */
	const uint32_t *fid;     /* [S1] what fsm_hip_exec_batch_ids writes for an input ending there, or null */
	const uint8_t  *base;
	const uint64_t *off;     /* n + 1 */
	uint32_t *end_out;       /* or null */
	uint32_t *id_out;        /* or null */
	uint64_t *bitmap;        /* or null */
	uint64_t n;
	uint64_t limit;          /* bytes of this job's text that may be read (>= off[n]); 0: off[n] */
	uint32_t C, S1, start, abs_min;
	uint32_t tile0;          /* first workgroup of this job */
	uint32_t lds_table;
	uint32_t pad[4];
};
static_assert(sizeof(MultiJob) % 16 == 0, "descriptors are read as aligned records");

typedef uint32_t u32x4m __attribute__((ext_vector_type(4)));
constexpr uint32_t MULTI_WAVES = 4;                    /* wavefronts per workgroup: MULTI_WAVES * 64 consecutive lines of ONE job share a table copy */

__device__ __forceinline__ uint32_t byte_at(const u32x4m &w, int k)
{
	const uint32_t d = (k < 4) ? w.x : (k < 8) ? w.y : (k < 12) ? w.z : w.w;
	return (d >> (8 * (k & 3))) & 0xffu;
}

/* one workgroup = MULTI_WAVES wavefronts = 256 consecutive lines of ONE job.  (Round 5: one wavefront per workgroup -- sized for
 * retest's three lines a record; a job of 1e5 lines then copied its table into LDS once per 64 of them.)  Every pointer of the
 * descriptor is device memory: the loads name that address space (no FLAT instruction: tests/test_abi.py). */
__global__ void __launch_bounds__(MULTI_WAVES * 64)
walk_multi(const MultiJob *jobs, const uint32_t *tile_job)
{
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef u32x4m __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	__shared__ uint32_t cls4[64];
	__shared__ uint16_t cls2[256];                  /* LDS tables: 2 * class of a byte -- the byte offset of its column in a row of u16 */
	__shared__ uint16_t tab[MULTI_LDS_ENTRIES];     /* ... and per (state, class) the BYTE offset of the next state's row */
	const uint32_t ji = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_job[blockIdx.x]);
	const MultiJob &j = jobs[ji];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t C = j.C, S1 = j.S1;
	const bool in_lds = j.lds_table != 0u;
	const g_u32p dense = (g_u32p)(uintptr_t)j.dense, fin = (g_u32p)(uintptr_t)j.fin, fid = (g_u32p)(uintptr_t)j.fid;
	const g_u64p off = (g_u64p)(uintptr_t)j.off;
	if (tid < 64u) {
		const uint32_t w4 = ((g_u32p)(uintptr_t)j.cls4)[tid];
		cls4[tid] = w4;
#pragma unroll
		for (int q = 0; q < 4; q++) cls2[tid * 4u + (uint32_t)q] = (uint16_t)(((w4 >> (8 * q)) & 0xffu) * 2u);
	}
	if (in_lds)
		for (uint32_t e = tid; e < S1 * C; e += MULTI_WAVES * 64u) tab[e] = (uint16_t)(dense[e] * C * 2u);   /* (S1 * C <= 16 384 entries: < 2^16 bytes) */
	__syncthreads();

	const uint64_t tile = blockIdx.x - j.tile0, i = tile * (MULTI_WAVES * 64u) + tid;
	const bool valid = i < j.n;
	uint64_t beg = 0, len = 0;
	if (valid) { beg = off[i]; len = off[i + 1] - beg; }
	const uint64_t limit = j.limit != 0u ? j.limit : off[j.n];
	const uint32_t unit = in_lds ? C * 2u : 1u;       /* the walk's state: byte offset of its row (LDS) or state index (global table) */
	const uint32_t absorbing = j.abs_min * unit;
	uint32_t s = j.start * unit;
	const uint64_t p = reinterpret_cast<uint64_t>(j.base) + beg;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	const uint32_t cls2_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)cls2;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;

	for (uint64_t t = 0;; t += 16u) {
		const bool live = t < len && s < absorbing;
		if (!__any(live)) break;
		const uint32_t cnt = !live ? 0u : len - t < 16u ? (uint32_t)(len - t) : 16u;
		u32x4m w = {0u, 0u, 0u, 0u};
		if (live) {
			if (beg + t + 16u <= limit) {
				w = *(g_chunkp)(p + t);
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(p + t))[k] << ((k & 3u) * 8u);
				w = u32x4m{d[0], d[1], d[2], d[3]};
			}
		}
		if (in_lds) {
			/* two LDS reads per byte: the byte's column offset (state-independent: all sixteen asked for at once), then the row */
			uint32_t c2[16];
#pragma unroll
			for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(cls2_at + byte_at(w, k) * 2u);
			if (__all(cnt == 16u || cnt == 0u)) {          /* whole chunks everywhere (lines of one length, the middle of long ones) */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) sn = *(l_u16p)(uintptr_t)(tab_at + sn + c2[k]);
				s = cnt != 0u ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + s + c2[k]);
					s = (uint32_t)k < cnt ? sn : s;
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)k < cnt) {
					const uint32_t b = byte_at(w, k);
					const uint32_t c = (cls4[b >> 2] >> ((b & 3u) * 8u)) & 0xffu;
					s = dense[(uint64_t)s * C + c];
				}
			}
		}
	}
	const uint32_t fs = in_lds ? s / (C * 2u) : s;
	uint32_t end = FSM_HIP_NO_MATCH;
	if (valid) end = fin[fs];
	typedef uint32_t __attribute__((address_space(1))) *g_u32w;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;
	if (valid && j.end_out != nullptr) ((g_u32w)(uintptr_t)j.end_out)[i] = end;
	if (valid && j.id_out != nullptr) ((g_u32w)(uintptr_t)j.id_out)[i] = fid[fs];
	const uint64_t m = __ballot(valid && end != FSM_HIP_NO_MATCH);
	if (j.bitmap != nullptr && lane == 0u && (tile * MULTI_WAVES + (tid >> 6)) * 64u < j.n) ((g_u64w)(uintptr_t)j.bitmap)[tile * MULTI_WAVES + (tid >> 6)] = m;
}

/* What a job with eager outputs adds to its descriptor (entry f belongs to jobs[f]).  Only walk_multi_eager reads it: the plain
 * kernel and its descriptor are what they were.  lo / hi are Plan::eager_lo_end / eager_hi_begin in the walk's own unit (the
 * byte offset of a row in the LDS form, the state index otherwise): a state emits iff state < lo || state >= hi.  A job
 * without eager_out, and one whose automaton emits nothing, has lo = 0, hi = 0xFFFFFFFF: no state emits. */
struct MultiEager {
	const uint64_t *emask;   /* [S1] the ids a state emits (W == 1) */
	const uint32_t *ew_off;  /* W > 1: state n ORs ew_mask[k] into word ew_word[k], k in [ew_off[n], ew_off[n + 1]) (Plan::ew_*) */
	const uint32_t *ew_word;
	const uint64_t *ew_mask;
	uint64_t *eager_out;     /* n * W words, or null: the job takes the plain path */
	uint32_t lo, hi;
	uint32_t W;
	uint32_t pad[3];
};
static_assert(sizeof(MultiEager) % 16 == 0, "descriptors are read as aligned records");

/* OR the outputs of the state at row index idx into the lane's set: a register pair (W == 1) or the lane's own row in memory */
__device__ __forceinline__ void multi_emit(const MultiEager &e, uint32_t idx, uint64_t &acc, uint64_t i)
{
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;
	if (e.W == 1u) {
		acc |= ((g_u64p)(uintptr_t)e.emask)[idx];
	} else {
		const g_u64w row = (g_u64w)(uintptr_t)e.eager_out + i * e.W;
		const g_u32p eo = (g_u32p)(uintptr_t)e.ew_off, ew = (g_u32p)(uintptr_t)e.ew_word;
		for (uint32_t k = eo[idx]; k < eo[idx + 1u]; k++) row[ew[k]] |= ((g_u64p)(uintptr_t)e.ew_mask)[k];
	}
}

/* walk_multi for a submission in which some job asks for eager-output sets (exec.c:126-144): the same walk, still ONE launch.
 * The job is wave-uniform; one that does not ask (or whose automaton emits nothing) has thresholds that no state meets and takes
 * the plain path.  As EagerPol::walk16 (walk_kernels.h): a chunk is walked as a plain chunk while a running minimum of the
 * states entered notes whether one of them lies below lo; the states from hi up are absorbing, so one of those was entered iff
 * the chunk ends there.  Only the lanes that did enter one walk the chunk again byte by byte, from the state it began in, and
 * collect.  Sets of up to 64 ids live in a register pair and are stored once (zero included: the result is overwritten, never
 * OR-ed into); wider ones in the lane's own row of eager_out, which the lane zeroes first.  A submission without eager outputs
 * launches walk_multi above, which is kept as it was: the two walks are to stay line for line the same. */
__global__ void __launch_bounds__(MULTI_WAVES * 64)
walk_multi_eager(const MultiJob *jobs, const uint32_t *tile_job, const MultiEager *ejobs)
{
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef u32x4m __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	__shared__ uint32_t cls4[64];
	__shared__ uint16_t cls2[256];                  /* LDS tables: 2 * class of a byte -- the byte offset of its column in a row of u16 */
	__shared__ uint16_t tab[MULTI_LDS_ENTRIES];     /* ... and per (state, class) the BYTE offset of the next state's row */
	const uint32_t ji = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_job[blockIdx.x]);
	const MultiJob &j = jobs[ji];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t C = j.C, S1 = j.S1;
	const bool in_lds = j.lds_table != 0u;
	const g_u32p dense = (g_u32p)(uintptr_t)j.dense, fin = (g_u32p)(uintptr_t)j.fin, fid = (g_u32p)(uintptr_t)j.fid;
	const g_u64p off = (g_u64p)(uintptr_t)j.off;
	if (tid < 64u) {
		const uint32_t w4 = ((g_u32p)(uintptr_t)j.cls4)[tid];
		cls4[tid] = w4;
#pragma unroll
		for (int q = 0; q < 4; q++) cls2[tid * 4u + (uint32_t)q] = (uint16_t)(((w4 >> (8 * q)) & 0xffu) * 2u);
	}
	if (in_lds)
		for (uint32_t e = tid; e < S1 * C; e += MULTI_WAVES * 64u) tab[e] = (uint16_t)(dense[e] * C * 2u);   /* (S1 * C <= 16 384 entries: < 2^16 bytes) */
	__syncthreads();

	const uint64_t tile = blockIdx.x - j.tile0, i = tile * (MULTI_WAVES * 64u) + tid;
	const bool valid = i < j.n;
	uint64_t beg = 0, len = 0;
	if (valid) { beg = off[i]; len = off[i + 1] - beg; }
	const uint64_t limit = j.limit != 0u ? j.limit : off[j.n];
	const uint32_t unit = in_lds ? C * 2u : 1u;       /* the walk's state: byte offset of its row (LDS) or state index (global table) */
	const uint32_t absorbing = j.abs_min * unit;
	uint32_t s = j.start * unit;
	const uint64_t p = reinterpret_cast<uint64_t>(j.base) + beg;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	const uint32_t cls2_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)cls2;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;

	const MultiEager *const ej = ejobs + ji;
	const uint32_t e_lo = ej->lo, e_hi = ej->hi;
	const bool collect = valid && ej->eager_out != nullptr;   /* this lane has a set to deliver */
	uint64_t acc = 0;
	if (collect) {
		if (ej->W != 1u)
			for (uint32_t k = 0; k < ej->W; k++) ((g_u64w)(uintptr_t)ej->eager_out)[i * ej->W + k] = 0u;
		if (s < e_lo || s >= e_hi) multi_emit(*ej, j.start, acc, i);   /* the start state emits before any input (exec.c:126-130) */
	}

	for (uint64_t t = 0;; t += 16u) {
		const bool live = t < len && s < absorbing;
		if (!__any(live)) break;
		const uint32_t cnt = !live ? 0u : len - t < 16u ? (uint32_t)(len - t) : 16u;
		u32x4m w = {0u, 0u, 0u, 0u};
		if (live) {
			if (beg + t + 16u <= limit) {
				w = *(g_chunkp)(p + t);
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(p + t))[k] << ((k & 3u) * 8u);
				w = u32x4m{d[0], d[1], d[2], d[3]};
			}
		}
		const uint32_t s0 = s;                        /* the state this chunk begins in */
		uint32_t mn = 0xFFFFFFFFu;                    /* the lowest state entered in this chunk */
		if (in_lds) {
			/* two LDS reads per byte: the byte's column offset (state-independent: all sixteen asked for at once), then the row */
			uint32_t c2[16];
#pragma unroll
			for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(cls2_at + byte_at(w, k) * 2u);
			if (__all(cnt == 16u || cnt == 0u)) {          /* whole chunks everywhere (lines of one length, the middle of long ones) */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					sn = *(l_u16p)(uintptr_t)(tab_at + sn + c2[k]);
					mn = sn < mn ? sn : mn;
				}
				s = cnt != 0u ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + s + c2[k]);
					s = (uint32_t)k < cnt ? sn : s;
					mn = s < mn ? s : mn;     /* (beyond cnt: the last state entered, again) */
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)k < cnt) {
					const uint32_t b = byte_at(w, k);
					const uint32_t c = (cls4[b >> 2] >> ((b & 3u) * 8u)) & 0xffu;
					s = dense[(uint64_t)s * C + c];
					mn = s < mn ? s : mn;
				}
			}
		}
		/* (cnt != 0: the lane was live, so s0 is not absorbing and a chunk that ends at or above hi entered that state) */
		if (collect && cnt != 0u && (mn < e_lo || s >= e_hi)) {
			uint32_t r = s0;
			for (uint32_t k = 0; k < cnt; k++) {
				const uint32_t b = byte_at(w, (int)k);
				uint32_t rn;
				if (in_lds) {
					rn = *(l_u16p)(uintptr_t)(tab_at + r + *(l_u16p)(uintptr_t)(cls2_at + b * 2u));
				} else {
					const uint32_t c = (cls4[b >> 2] >> ((b & 3u) * 8u)) & 0xffu;
					rn = dense[(uint64_t)r * C + c];
				}
				/* OR is idempotent: staying in the same state emits nothing new */
				if (rn != r && (rn < e_lo || rn >= e_hi)) multi_emit(*ej, in_lds ? rn / (C * 2u) : rn, acc, i);
				r = rn;
			}
		}
	}
	const uint32_t fs = in_lds ? s / (C * 2u) : s;
	uint32_t end = FSM_HIP_NO_MATCH;
	if (valid) end = fin[fs];
	typedef uint32_t __attribute__((address_space(1))) *g_u32w;
	if (valid && j.end_out != nullptr) ((g_u32w)(uintptr_t)j.end_out)[i] = end;
	if (valid && j.id_out != nullptr) ((g_u32w)(uintptr_t)j.id_out)[i] = fid[fs];
	if (collect && ej->W == 1u) ((g_u64w)(uintptr_t)ej->eager_out)[i] = acc;
	const uint64_t m = __ballot(valid && end != FSM_HIP_NO_MATCH);
	if (j.bitmap != nullptr && lane == 0u && (tile * MULTI_WAVES + (tid >> 6)) * 64u < j.n) ((g_u64w)(uintptr_t)j.bitmap)[tile * MULTI_WAVES + (tid >> 6)] = m;
}

struct MultiCtx {
	std::mutex mu;
	DevStream s;
	PinBuf<unsigned char> pin;
	DevBuf<unsigned char> dev;
	size_t pin_bytes = 0, dev_bytes = 0;
	DevEvent ev;
	bool busy = false;           /* a device-pointer call's launch may still read the blocks */
};
constexpr int MAXDEV = 64;
MultiCtx *const g_ctx = new MultiCtx[MAXDEV];   /* never deleted: nothing of HIP is called while the process unloads */
std::atomic<unsigned> g_last_launches{0}, g_last_fused_jobs{0};

size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }

int ctx_reserve(MultiCtx &cx, size_t bytes)
{
	if (cx.s == nullptr && !HIP_OK(cx.s.create(hipStreamNonBlocking))) return -1;
	if (cx.ev == nullptr && !HIP_OK(cx.ev.create(hipEventDisableTiming))) return -1;
	if (cx.busy) {
		if (!HIP_OK(hipEventSynchronize(cx.ev))) return -1;
		cx.busy = false;
	}
	if (bytes > cx.pin_bytes) {
		size_t want = (size_t)1 << 16;
		while (want < bytes) want *= 2;
		cx.pin.reset();
		cx.dev.reset();
		cx.pin_bytes = cx.dev_bytes = 0;
		if (!HIP_OK(cx.pin.alloc(want))) return -1;
		if (!HIP_OK(cx.dev.alloc(want))) return -1;
		cx.pin_bytes = cx.dev_bytes = want;
	}
	return 0;
}

/* where everything of a fused submission lies in the staging block (the same offsets on both sides) */
struct Lay {
	/* per fused job; (size_t)-1: not staged */
	std::vector<size_t> dense, cls, fin, fid, emask, ewoff, ewword, ewmask, off, text, end, bm, ids, sets;
	size_t jobs = 0, tiles = 0, ejobs = (size_t)-1, in_end = 0, total = 0;
	uint32_t ntiles = 0;
};

/* the head of the block: descriptors, tile map and -- when some job asks for eager outputs -- the eager descriptors; returns
 * the offset behind them */
size_t lay_head(Lay &L, size_t kf, uint64_t tiles, bool eager)
{
	for (std::vector<size_t> *v : {&L.dense, &L.cls, &L.fin, &L.fid, &L.emask, &L.ewoff, &L.ewword, &L.ewmask, &L.off, &L.text, &L.end, &L.bm, &L.ids, &L.sets})
		v->assign(kf, (size_t)-1);
	size_t o = 0;
	L.ntiles = (uint32_t)tiles;
	L.jobs = o; o += up16(kf * sizeof(MultiJob));
	L.tiles = o; o += up16((size_t)tiles * 4u);
	if (eager) { L.ejobs = o; o += up16(kf * sizeof(MultiEager)); }
	return o;
}

/* bytes of the automaton's side of a fused job: plain table, byte classes, end states, ids, eager masks */
size_t table_bytes(const Plan *p, bool ids, bool eager)
{
	size_t o = up16(p->dense.size() * 4u) + 256u + up16((size_t)p->S1 * 4u) * (ids ? 2u : 1u);
	if (eager && !p->emask.empty())
		o += p->eager_words <= 1 ? up16((size_t)p->S1 * 8u) : up16(p->ew_off.size() * 4u) + up16(p->ew_word.size() * 4u) + up16(p->ew_mask.size() * 8u);
	return o;
}

/* ... and where they lie, from offset o on; returns the offset behind them (o + table_bytes) */
size_t lay_tables(Lay &L, size_t f, const Plan *p, bool ids, bool eager, size_t o)
{
	L.dense[f] = o; o += up16(p->dense.size() * 4u);
	L.cls[f] = o; o += 256u;
	L.fin[f] = o; o += up16((size_t)p->S1 * 4u);
	if (ids) { L.fid[f] = o; o += up16((size_t)p->S1 * 4u); }
	if (eager && !p->emask.empty()) {
		if (p->eager_words <= 1) {
			L.emask[f] = o; o += up16((size_t)p->S1 * 8u);
		} else {    /* wide sets: the (word, mask) pairs per state; Plan::emask only flags the emitting states there */
			L.ewoff[f] = o; o += up16(p->ew_off.size() * 4u);
			L.ewword[f] = o; o += up16(p->ew_word.size() * 4u);
			L.ewmask[f] = o; o += up16(p->ew_mask.size() * 8u);
		}
	}
	return o;
}

/* host front: a job small enough to stage (its lines ride in the one copy); device front: any job whose plain table fits the
 * kernel's LDS copy -- nothing of it is staged but the table, and MULTI_WAVES * 64 lines share each copy (round 5 fused on the
 * line count alone there and sent 1e5-line jobs, one launch each, through their dfa's own walk; a job with a bigger table
 * still goes that way: its planned layout beats a plain table in L2).  eager: the job asks for eager-output sets -- wider
 * than MULTI_EAGER_WORDS words, it goes its dfa's own way too. */
bool fusable(const Plan *p, size_t n, uint64_t bytes, bool host, bool eager)
{
	if (n == 0 || p->S1 == 0 || p->dense.size() != (size_t)p->S1 * p->C || p->dense.size() * 4u > MULTI_FUSE_TABLE) return false;
	if (eager && p->eager_words > MULTI_EAGER_WORDS) return false;
	if (host) return n <= MULTI_FUSE_LINES && bytes <= MULTI_FUSE_BYTES;
	return p->dense.size() <= MULTI_LDS_ENTRIES && n < ((size_t)1 << 31);
}

/* the automaton's side of fused job f: its plain table, byte classes, end states, (asked for) ids and eager masks into the host
 * block `pin` at the layout's offsets, the descriptors pointing at the same offsets of the device block `dev`.  ej: the job's
 * eager descriptor (null: a submission without eager outputs); its eager_out is the caller's to set. */
void fill_tables(unsigned char *pin, unsigned char *dev, const Lay &L, size_t f, const Plan *p, const std::vector<uint32_t> &fid, MultiJob &j, MultiEager *ej)
{
	const size_t none = (size_t)-1;
	memcpy(pin + L.dense[f], p->dense.data(), p->dense.size() * 4u);
	pack_cls4(p->cls, reinterpret_cast<uint32_t *>(pin + L.cls[f]));
	memcpy(pin + L.fin[f], p->fin.data(), (size_t)p->S1 * 4u);
	if (L.fid[f] != none) memcpy(pin + L.fid[f], fid.data(), (size_t)p->S1 * 4u);
	memset(&j, 0, sizeof j);
	j.fid = L.fid[f] != none ? reinterpret_cast<const uint32_t *>(dev + L.fid[f]) : nullptr;
	j.dense = reinterpret_cast<const uint32_t *>(dev + L.dense[f]);
	j.cls4 = reinterpret_cast<const uint32_t *>(dev + L.cls[f]);
	j.fin = reinterpret_cast<const uint32_t *>(dev + L.fin[f]);
	j.C = p->C; j.S1 = p->S1; j.start = p->start; j.abs_min = p->abs_min;
	j.lds_table = p->dense.size() <= MULTI_LDS_ENTRIES ? 1u : 0u;
	if (ej == nullptr) return;
	memset(ej, 0, sizeof *ej);
	ej->lo = 0u; ej->hi = 0xFFFFFFFFu; ej->W = 1u;       /* no state emits: an all-zero word per line */
	if (L.emask[f] == none && L.ewoff[f] == none) return;
	/* Plan::eager_lo_end / eager_hi_begin count in the renumbered index of Plan::dense (plan.h:37-46); the walk's state is that
	 * index (global table) or the byte offset of its row (LDS form).  hi_begin <= S1 - 1 (DEAD is last): no overflow. */
	const uint32_t unit = j.lds_table ? p->C * 2u : 1u;
	ej->lo = p->eager_lo_end * unit;
	ej->hi = p->eager_hi_begin * unit;
	ej->W = p->eager_words;
	if (L.emask[f] != none) {
		memcpy(pin + L.emask[f], p->emask.data(), (size_t)p->S1 * 8u);
		ej->emask = reinterpret_cast<const uint64_t *>(dev + L.emask[f]);
	} else {
		memcpy(pin + L.ewoff[f], p->ew_off.data(), p->ew_off.size() * 4u);
		memcpy(pin + L.ewword[f], p->ew_word.data(), p->ew_word.size() * 4u);
		memcpy(pin + L.ewmask[f], p->ew_mask.data(), p->ew_mask.size() * 8u);
		ej->ew_off = reinterpret_cast<const uint32_t *>(dev + L.ewoff[f]);
		ej->ew_word = reinterpret_cast<const uint32_t *>(dev + L.ewword[f]);
		ej->ew_mask = reinterpret_cast<const uint64_t *>(dev + L.ewmask[f]);
	}
}

/* the fused launch over a block laid out as above: today's kernel, or its eager form when the block has eager descriptors */
void launch_fused(const unsigned char *dev, size_t jobs_off, size_t tiles_off, size_t ejobs_off, uint32_t ntiles, hipStream_t s)
{
	const MultiJob *jobs = reinterpret_cast<const MultiJob *>(dev + jobs_off);
	const uint32_t *tile_job = reinterpret_cast<const uint32_t *>(dev + tiles_off);
	if (ejobs_off == (size_t)-1)
		hipLaunchKernelGGL(walk_multi, dim3(ntiles), dim3(MULTI_WAVES * 64u), 0, s, jobs, tile_job);
	else
		hipLaunchKernelGGL(walk_multi_eager, dim3(ntiles), dim3(MULTI_WAVES * 64u), 0, s, jobs, tile_job, reinterpret_cast<const MultiEager *>(dev + ejobs_off));
}

/* one job as the entry points hand it over (ids, eager sets: optional) */
struct JobView {
	const unsigned char *base;
	const uint64_t *off;
	size_t n;
	uint32_t *end_out;
	uint64_t *accept_bitmap;
	uint32_t *id_out;
	uint64_t *eager_out;
};

/* a job that does not ride in the fused launch: its dfa's own walk, every output it asks for from ONE walk (host: the
 * synchronous front; device: enqueued on the stream) */
int run_single(const struct fsm_hip_dfa *dfa, const JobView &j, int ids_mode, bool host, hipStream_t stream)
{
	if (j.id_out == nullptr && j.eager_out == nullptr)
		return host ? fsm_hip_exec_batch_offsets(dfa, j.base, j.off, j.n, j.end_out, j.accept_bitmap)
		            : fsm_hip_exec_batch_offsets_device(dfa, j.base, j.off, j.n, j.end_out, j.accept_bitmap, stream);
	return host ? fsm_hip_exec_batch_packed_all(dfa, j.base, FSM_HIP_META_OFF64, j.off, j.n, j.end_out, j.accept_bitmap, ids_mode, j.id_out, j.eager_out)
	            : fsm_hip_exec_batch_packed_all_device(dfa, j.base, FSM_HIP_META_OFF64, j.off, j.n, j.end_out, j.accept_bitmap, ids_mode, j.id_out, j.eager_out, stream);
}

/* Run the jobs idx[] (all on device `device`) of a submission.  host = true: b[] holds host pointers (lines and results are
 * staged); false: device pointers, launched on `stream` and not waited for. */
int run_device_group(int device, const struct fsm_hip_dfa *const *dfa, const JobView *b, int ids_mode, const std::vector<size_t> &idx,
	bool host, hipStream_t stream, unsigned *launches, unsigned *fused_jobs)
{
	if (device < 0 || device >= MAXDEV) { errno = ENODEV; return -1; }
	DevGuard dg(device);
	if (!dg.ok()) { errno = ENODEV; return -1; }

	MultiCtx &cx = g_ctx[device];
	std::lock_guard<std::mutex> lk(cx.mu);

	/* which jobs ride in the fused launch */
	std::vector<size_t> fj, single;
	std::vector<std::vector<uint32_t>> fids;      /* per fused job: ids by renumbered state (empty: none asked for) */
	Lay L;
	bool eager = false;                           /* some fused job asks for eager-output sets */
	{
		size_t staged = 0;
		for (size_t q : idx) {
			const Plan *p = dfa_plan(dfa[q]);
			const size_t n = b[q].n;
			const uint64_t bytes = n ? (host ? b[q].off[n] : 0) : 0;
			if (n == 0) continue;
			const bool eg = b[q].eager_out != nullptr;
			const size_t W = p->eager_words ? p->eager_words : 1u;
			const size_t need = table_bytes(p, true, eg) +
				(host ? up16((n + 1) * 8u) + up16((size_t)bytes + 16u) + 2u * up16(n * 4u) + up16(((n + 63u) / 64u) * 8u) + (eg ? up16(n * W * 8u) : 0u) : 0u);
			if (fusable(p, n, bytes, host, eg) && staged + need <= MULTI_STAGE_CAP) { fj.push_back(q); staged += need; eager = eager || eg; }
			else single.push_back(q);
		}
	}
	if (!fj.empty()) {
		const size_t kf = fj.size();
		uint64_t tiles = 0;
		for (size_t q : fj) tiles += (b[q].n + MULTI_WAVES * 64u - 1u) / (MULTI_WAVES * 64u);
		if (tiles > 0x7FFFFFFFu) { errno = EINVAL; return -1; }
		fids.resize(kf);
		for (size_t f = 0; f < kf; f++)
			if (b[fj[f]].id_out != nullptr) ids_by_state(*dfa_plan(dfa[fj[f]]), ids_mode, fids[f], nullptr);
		size_t o = lay_head(L, kf, tiles, eager);
		for (size_t f = 0; f < kf; f++) {
			const size_t q = fj[f];
			o = lay_tables(L, f, dfa_plan(dfa[q]), !fids[f].empty(), b[q].eager_out != nullptr, o);
			if (host) {
				const size_t n = b[q].n;
				L.off[f] = o; o += up16((n + 1) * 8u);
				L.text[f] = o; o += up16((size_t)b[q].off[n] + 16u);
			}
		}
		L.in_end = o;
		if (host)
			for (size_t f = 0; f < kf; f++) {
				const size_t q = fj[f], n = b[q].n;
				if (b[q].end_out) { L.end[f] = o; o += up16(n * 4u); }
				if (b[q].id_out) { L.ids[f] = o; o += up16(n * 4u); }
				if (b[q].accept_bitmap) { L.bm[f] = o; o += up16(((n + 63u) / 64u) * 8u); }
				if (b[q].eager_out) { L.sets[f] = o; o += up16(n * fsm_hip_eager_words(dfa[q]) * 8u); }
			}
		L.total = o;
		if (ctx_reserve(cx, L.total) != 0) return -1;

		/* fill the pinned block */
		MultiJob *jobs = reinterpret_cast<MultiJob *>(cx.pin + L.jobs);
		MultiEager *ejobs = eager ? reinterpret_cast<MultiEager *>(cx.pin + L.ejobs) : nullptr;
		uint32_t *tile_job = reinterpret_cast<uint32_t *>(cx.pin + L.tiles);
		uint32_t t0 = 0;
		const size_t none = (size_t)-1;
		for (size_t f = 0; f < kf; f++) {
			const size_t q = fj[f];
			const Plan *p = dfa_plan(dfa[q]);
			const size_t n = b[q].n;
			MultiJob &j = jobs[f];
			fill_tables(cx.pin, cx.dev, L, f, p, fids[f], j, eager ? ejobs + f : nullptr);
			if (host) {
				const size_t bytes = (size_t)b[q].off[n];
				memcpy(cx.pin + L.off[f], b[q].off, (n + 1) * 8u);
				if (bytes) memcpy(cx.pin + L.text[f], b[q].base, bytes);
				memset(cx.pin + L.text[f] + bytes, 0, 16);
				j.base = cx.dev + L.text[f];
				j.off = reinterpret_cast<const uint64_t *>(cx.dev + L.off[f]);
				j.end_out = L.end[f] != none ? reinterpret_cast<uint32_t *>(cx.dev + L.end[f]) : nullptr;
				j.id_out = L.ids[f] != none ? reinterpret_cast<uint32_t *>(cx.dev + L.ids[f]) : nullptr;
				j.bitmap = L.bm[f] != none ? reinterpret_cast<uint64_t *>(cx.dev + L.bm[f]) : nullptr;
				if (eager) ejobs[f].eager_out = L.sets[f] != none ? reinterpret_cast<uint64_t *>(cx.dev + L.sets[f]) : nullptr;
				j.limit = bytes + 16u;    /* the staged text is padded: whole 16-byte loads everywhere */
			} else {
				j.base = b[q].base;
				j.off = b[q].off;
				j.end_out = b[q].end_out;
				j.id_out = b[q].id_out;
				j.bitmap = b[q].accept_bitmap;
				if (eager) ejobs[f].eager_out = b[q].eager_out;
				j.limit = 0;              /* the kernel reads off[n] */
			}
			j.n = n;
			j.tile0 = t0;
			const uint32_t nt = (uint32_t)((n + MULTI_WAVES * 64u - 1u) / (MULTI_WAVES * 64u));
			for (uint32_t t = 0; t < nt; t++) tile_job[t0 + t] = (uint32_t)f;
			t0 += nt;
		}
		hipStream_t s = host ? cx.s : stream;
		if (!HIP_OK(hipMemcpyAsync(cx.dev, cx.pin, L.in_end, hipMemcpyHostToDevice, s))) return -1;
		launch_fused(cx.dev, L.jobs, L.tiles, L.ejobs, L.ntiles, s);
		if (!HIP_OK(hipGetLastError())) return -1;
		(*launches)++;
		*fused_jobs += (unsigned)kf;
		if (host) {
			if (L.total > L.in_end && !HIP_OK(hipMemcpyAsync(cx.pin + L.in_end, cx.dev + L.in_end, L.total - L.in_end, hipMemcpyDeviceToHost, s))) return -1;
		} else {
			if (!HIP_OK(hipEventRecord(cx.ev, s))) return -1;
			cx.busy = true;
		}
	}
	/* the big ones: each dfa's own walk, beside the fused launch */
	for (size_t q : single) {
		if (run_single(dfa[q], b[q], ids_mode, host, stream) != 0) { if (host && !fj.empty()) (void)hipStreamSynchronize(cx.s); return -1; }
		(*launches)++;
	}
	if (host && !fj.empty()) {
		if (!HIP_OK(hipStreamSynchronize(cx.s))) return -1;
		for (size_t f = 0; f < fj.size(); f++) {
			const size_t q = fj[f], n = b[q].n;
			if (L.end[f] != (size_t)-1) memcpy(b[q].end_out, cx.pin + L.end[f], n * 4u);
			if (L.ids[f] != (size_t)-1) memcpy(b[q].id_out, cx.pin + L.ids[f], n * 4u);
			if (L.bm[f] != (size_t)-1) memcpy(b[q].accept_bitmap, cx.pin + L.bm[f], ((n + 63u) / 64u) * 8u);
			if (L.sets[f] != (size_t)-1) memcpy(b[q].eager_out, cx.pin + L.sets[f], n * fsm_hip_eager_words(dfa[q]) * 8u);
		}
	}
	return 0;
}

/* what every form of a submission checks before anything is launched; *ids_mode: ERROR -> EARLIEST once no job is ambiguous */
int check_jobs(const struct fsm_hip_dfa *const *dfa, const JobView *b, int *ids_mode_io, size_t k, bool host)
{
	int ids_mode = *ids_mode_io;
	if (dfa == nullptr || b == nullptr) { errno = EINVAL; return -1; }
	bool want_ids = false;
	for (size_t q = 0; q < k; q++) want_ids = want_ids || b[q].id_out != nullptr;
	if (want_ids) {
		if (ids_mode != FSM_HIP_IDS_EARLIEST && ids_mode != FSM_HIP_IDS_RET && ids_mode != FSM_HIP_IDS_ERROR) { errno = EINVAL; return -1; }
		if (ids_mode == FSM_HIP_IDS_ERROR) {
			/* AMBIG_ERROR: an end state with more than one id is refused before anything is launched (as fsm_hip_exec_batch_ids) */
			std::vector<uint32_t> tmp;
			for (size_t q = 0; q < k; q++) {
				uint32_t cf = FSM_HIP_NO_MATCH;
				if (dfa[q] == nullptr) { errno = EINVAL; return -1; }
				if (b[q].id_out != nullptr) ids_by_state(*dfa_plan(dfa[q]), FSM_HIP_IDS_EARLIEST, tmp, &cf);
				if (cf != FSM_HIP_NO_MATCH) { errno = EINVAL; return -1; }
			}
			ids_mode = FSM_HIP_IDS_EARLIEST;
		}
	}
	for (size_t q = 0; q < k; q++) {
		if (dfa[q] == nullptr || (b[q].n != 0 && b[q].off == nullptr)) { errno = EINVAL; return -1; }
		if (host && b[q].n != 0) {
			for (size_t i = 0; i < b[q].n; i++)
				if (b[q].off[i + 1] < b[q].off[i]) { errno = EINVAL; return -1; }
			if (b[q].off[b[q].n] != 0 && b[q].base == nullptr) { errno = EINVAL; return -1; }
		}
	}
	*ids_mode_io = ids_mode;
	return 0;
}

int exec_multi(const struct fsm_hip_dfa *const *dfa, const JobView *b, int ids_mode, size_t k, bool host, hipStream_t stream)
{
	if (k == 0) { g_last_launches = 0; g_last_fused_jobs = 0; return 0; }
	if (check_jobs(dfa, b, &ids_mode, k, host) != 0) return -1;
	/* jobs by device (a submission usually has one) */
	std::vector<int> devs;
	for (size_t q = 0; q < k; q++) {
		const int dv = dfa_device(dfa[q]);
		if (std::find(devs.begin(), devs.end(), dv) == devs.end()) devs.push_back(dv);
	}
	unsigned launches = 0, fused = 0;
	for (int dv : devs) {
		std::vector<size_t> idx;
		for (size_t q = 0; q < k; q++) if (dfa_device(dfa[q]) == dv) idx.push_back(q);
		if (run_device_group(dv, dfa, b, ids_mode, idx, host, stream, &launches, &fused) != 0) return -1;
	}
	g_last_launches = launches;
	g_last_fused_jobs = fused;
	return 0;
}

} // namespace

static std::vector<JobView> views(const struct fsm_hip_multi_batch *b, size_t k)
{
	std::vector<JobView> v(b ? k : 0);
	for (size_t q = 0; q < v.size(); q++) v[q] = JobView{b[q].base, b[q].off, b[q].n, b[q].end_out, b[q].accept_bitmap, nullptr, nullptr};
	return v;
}
static std::vector<JobView> views(const struct fsm_hip_multi_batch_ids *b, size_t k)
{
	std::vector<JobView> v(b ? k : 0);
	for (size_t q = 0; q < v.size(); q++) v[q] = JobView{b[q].base, b[q].off, b[q].n, b[q].end_out, b[q].accept_bitmap, b[q].id_out, nullptr};
	return v;
}
static std::vector<JobView> views(const struct fsm_hip_multi_batch_eager *b, size_t k)
{
	std::vector<JobView> v(b ? k : 0);
	for (size_t q = 0; q < v.size(); q++) v[q] = JobView{b[q].base, b[q].off, b[q].n, b[q].end_out, b[q].accept_bitmap, b[q].id_out, b[q].eager_out};
	return v;
}

extern "C" int fsm_hip_exec_multi(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch *b, size_t k)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, 0, k, true, nullptr);
}

extern "C" int fsm_hip_exec_multi_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch *b, size_t k, void *hip_stream)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, 0, k, false, static_cast<hipStream_t>(hip_stream));
}

extern "C" int fsm_hip_exec_multi_ids(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, ids_mode, k, true, nullptr);
}

extern "C" int fsm_hip_exec_multi_ids_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode, void *hip_stream)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, ids_mode, k, false, static_cast<hipStream_t>(hip_stream));
}

extern "C" int fsm_hip_exec_multi_eager(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, ids_mode, k, true, nullptr);
}

extern "C" int fsm_hip_exec_multi_eager_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode, void *hip_stream)
{
	const std::vector<JobView> v = views(b, k);
	return exec_multi(dfa, k && b ? v.data() : nullptr, ids_mode, k, false, static_cast<hipStream_t>(hip_stream));
}

/*
 * The PREPARED form: a submission of device-resident jobs whose descriptors, tile map and tables are put on the device ONCE.
 * fsm_hip_multi_launch is then one kernel launch (plus one per job whose table is too big to fuse: its dfa's own device front)
 * on the caller's stream -- no copy, no allocation, no wait: it can be captured into a HIP graph and replayed on whatever the
 * jobs' buffers hold by then (reperf's loop over the same matcher, src/retest/reperf.c:772-784, for K matchers at once).
 */
struct __attribute__((visibility("hidden"))) fsm_hip_multi_prepared {      /* (the type: its members' C++ symbols stay out of the ABI) */
	int device = 0, ids_mode = FSM_HIP_IDS_EARLIEST;
	DevBuf<unsigned char> dev;
	size_t jobs_off = 0, tiles_off = 0, ejobs_off = (size_t)-1;
	uint32_t ntiles = 0;
	unsigned fused = 0;
	struct Single { const struct fsm_hip_dfa *dfa; JobView v; };
	std::vector<Single> singles;
};

/* what fsm_hip_multi_prepare and fsm_hip_multi_prepare_eager share: everything behind their job structs */
static int multi_prepare(const struct fsm_hip_dfa *const *dfa, const std::vector<JobView> &v, bool have_b, size_t k, int ids_mode, struct fsm_hip_multi_prepared **out)
{
	if (out == nullptr) { errno = EINVAL; return -1; }
	*out = nullptr;
	if (k != 0 && check_jobs(dfa, have_b ? v.data() : nullptr, &ids_mode, k, false) != 0) return -1;
	for (size_t q = 1; q < k; q++)
		if (dfa_device(dfa[q]) != dfa_device(dfa[0])) { errno = EINVAL; return -1; }      /* one stream, one device (fsm_hip_node_exec_multi shards) */
	std::unique_ptr<fsm_hip_multi_prepared> pp(new (std::nothrow) fsm_hip_multi_prepared);
	if (pp == nullptr) { errno = ENOMEM; return -1; }
	pp->ids_mode = ids_mode;
	pp->device = k != 0 ? dfa_device(dfa[0]) : 0;
	std::vector<size_t> fj;
	bool eager = false;
	for (size_t q = 0; q < k; q++) {
		if (v[q].n == 0) continue;
		if (fusable(dfa_plan(dfa[q]), v[q].n, 0, false, v[q].eager_out != nullptr)) { fj.push_back(q); eager = eager || v[q].eager_out != nullptr; }
		else pp->singles.push_back({dfa[q], v[q]});
	}
	if (!fj.empty()) {
		const size_t kf = fj.size();
		uint64_t tiles = 0;
		for (size_t q : fj) tiles += (v[q].n + MULTI_WAVES * 64u - 1u) / (MULTI_WAVES * 64u);
		if (tiles > 0x7FFFFFFFu) { errno = EINVAL; return -1; }
		std::vector<std::vector<uint32_t>> fids(kf);
		for (size_t f = 0; f < kf; f++)
			if (v[fj[f]].id_out != nullptr) ids_by_state(*dfa_plan(dfa[fj[f]]), ids_mode, fids[f], nullptr);
		Lay L;
		size_t o = lay_head(L, kf, tiles, eager);
		for (size_t f = 0; f < kf; f++) o = lay_tables(L, f, dfa_plan(dfa[fj[f]]), !fids[f].empty(), v[fj[f]].eager_out != nullptr, o);
		DevGuard dg(pp->device);
		if (!dg.ok()) { errno = ENODEV; return -1; }
		std::vector<unsigned char> host(o);
		DevBuf<unsigned char> dev;      /* (goes, if the copy fails, while its device is still current) */
		if (!HIP_OK(dev.alloc(o))) return -1;
		MultiJob *jobs = reinterpret_cast<MultiJob *>(host.data() + L.jobs);
		MultiEager *ejobs = eager ? reinterpret_cast<MultiEager *>(host.data() + L.ejobs) : nullptr;
		uint32_t *tile_job = reinterpret_cast<uint32_t *>(host.data() + L.tiles);
		uint32_t t0 = 0;
		for (size_t f = 0; f < kf; f++) {
			const size_t q = fj[f];
			MultiJob &j = jobs[f];
			fill_tables(host.data(), dev, L, f, dfa_plan(dfa[q]), fids[f], j, eager ? ejobs + f : nullptr);
			j.base = v[q].base; j.off = v[q].off;
			j.end_out = v[q].end_out; j.id_out = v[q].id_out; j.bitmap = v[q].accept_bitmap;
			if (eager) ejobs[f].eager_out = v[q].eager_out;
			j.limit = 0;
			j.n = v[q].n;
			j.tile0 = t0;
			const uint32_t nt = (uint32_t)((v[q].n + MULTI_WAVES * 64u - 1u) / (MULTI_WAVES * 64u));
			for (uint32_t t = 0; t < nt; t++) tile_job[t0 + t] = (uint32_t)f;
			t0 += nt;
		}
		if (!HIP_OK(hipMemcpy(dev, host.data(), o, hipMemcpyHostToDevice))) return -1;
		pp->dev = std::move(dev);
		pp->jobs_off = L.jobs; pp->tiles_off = L.tiles; pp->ejobs_off = L.ejobs; pp->ntiles = (uint32_t)tiles; pp->fused = (unsigned)kf;
	}
	*out = pp.release();
	return 0;
}

extern "C" int fsm_hip_multi_prepare(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode,
	struct fsm_hip_multi_prepared **out)
{
	return multi_prepare(dfa, views(b, k), b != nullptr, k, ids_mode, out);
}

extern "C" int fsm_hip_multi_prepare_eager(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode,
	struct fsm_hip_multi_prepared **out)
{
	return multi_prepare(dfa, views(b, k), b != nullptr, k, ids_mode, out);
}

extern "C" int fsm_hip_multi_launch(const struct fsm_hip_multi_prepared *pp, void *hip_stream)
{
	if (pp == nullptr) { errno = EINVAL; return -1; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	DevGuard dg(pp->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	unsigned launches = 0;
	if (pp->ntiles != 0) {
		launch_fused(pp->dev, pp->jobs_off, pp->tiles_off, pp->ejobs_off, pp->ntiles, s);
		if (!HIP_OK(hipGetLastError())) return -1;
		launches++;
	}
	for (const auto &sg : pp->singles) {
		if (run_single(sg.dfa, sg.v, pp->ids_mode, false, s) != 0) return -1;
		launches++;
	}
	g_last_launches = launches;
	g_last_fused_jobs = pp->fused;
	return 0;
}

extern "C" void fsm_hip_multi_prepared_free(struct fsm_hip_multi_prepared *pp)
{
	if (pp == nullptr) return;
	DevGuard dg(pp->device);
	delete pp;           /* (releasing the block waits for the device: a launch still reading it ends first) */
}

extern "C" unsigned fsm_hip_multi_last_launches(void) { return g_last_launches.load(); }
extern "C" unsigned fsm_hip_multi_last_fused_jobs(void) { return g_last_fused_jobs.load(); }

/* Which device runs which job of a many-DFA submission ("multi-DFA batches shard by DFA"): largest first,
 * each to the device with the least work so far; ties go to the lower device, equal costs keep their order.  Pure host
 * arithmetic: every rank of a multi-process run computes the same split. */
extern "C" int fsm_hip_multi_assign(const uint64_t *cost, size_t k, int ndev, int *dev_of)
{
	if (ndev <= 0 || (k != 0 && (cost == nullptr || dev_of == nullptr))) { errno = EINVAL; return -1; }
	std::vector<size_t> order(k);
	std::iota(order.begin(), order.end(), (size_t)0);
	std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cost[x] > cost[y]; });
	std::vector<uint64_t> load((size_t)ndev, 0);
	for (size_t q : order) {
		int best = 0;
		for (int g = 1; g < ndev; g++) if (load[(size_t)g] < load[(size_t)best]) best = g;
		dev_of[q] = best;
		load[(size_t)best] += cost[q] ? cost[q] : 1u;
	}
	return 0;
}
