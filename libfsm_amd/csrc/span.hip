/*
 * span.hip -- accept positions: for each input, the first and the last position at which the walk's state is an end state.
 *
 * Every other front answers with the state a walk ENDS in (src/libfsm/exec.c:153-155).  The walk of exec.c:132-151 visits every
 * state on the way, and whether each of them is an end state is what a caller needs to know where in a line a match begins or
 * ends: grep -o, a lexer's longest match, the offset of the first hit in a record.  Here that bit rides with the state: the device
 * image folds "the TARGET state is an end state" into every table entry, so the walk makes no second lookup:
 *     S1 * C <= 16 384 entries   u16 in LDS: the byte offset of the next state's row (always even) | the bit in bit 0
 *     otherwise                  u32 in device memory: the next state's index | the bit in bit 31
 * and the per-byte chain of walk_multi (multi.hip) gains an `and` and a shift-or into a 16-bit accept mask of the chunk; first and
 * last are taken from the mask's lowest and highest set bit once per chunk.  No per-byte branch.
 *
 * walk_pos<BACK> walks a sub-range [from', to'] of line pick[j] of a packed text forward, or backward from to' (the chunk that
 * ENDS at the cursor, its bytes taken from the top).  Positions are byte boundaries relative to the line's first byte; position
 * from' (backward: to') is the start state, before any byte.  A lane stops at an absorbing state: DEAD (the missing edge,
 * exec.c:133-138) accepts nothing more, an absorbing end state accepts at every later position, so last is the range's far end.
 * Nothing outside [base, base + limit) is read: a line is clipped to the limit before it is walked, a chunk that would cross
 * either end of the readable bytes is assembled from byte loads.  Every pointer names its address space (no FLAT instruction:
 * tests/test_abi.py).
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/fsm_hip.h"
#include "dfa_access.h"
#include "hip_host.h"
#include "line_batch.h"
#include "span.h"

using namespace fsmhip;

namespace {

constexpr uint32_t POS_WAVES = 4;                      /* wavefronts per workgroup: POS_WAVES * 64 consecutive inputs share a table copy */
constexpr uint32_t POS_THREADS = POS_WAVES * 64u;
static_assert(POS_THREADS == 256, "one thread per byte value copies the class map");

typedef uint32_t u32x4p __attribute__((ext_vector_type(4)));

/* the launch's arguments, by value: every pointer is device memory */
struct PosArgs {
	const void *tab;         /* [entries]: u16 (LDS form) or u32, the end-state bit of the target folded in */
	const uint16_t *col;     /* [256]: LDS form 2 * class of a byte (the byte offset of its column), else its class */
	const uint8_t *base;
	const uint64_t *off;     /* n + 1 */
	const uint64_t *pick;    /* m, or null: input j is line j */
	const uint64_t *from;    /* m, or null: 0 */
	const uint64_t *to;      /* m, or null: the line's length */
	uint64_t *first_out;     /* m, or null */
	uint64_t *last_out;      /* m, or null */
	uint64_t n, m;
	uint64_t limit;          /* has_limit: the bytes of base that may be read; else off[n] is */
	uint32_t entries, C;
	uint32_t start;          /* the start state in the walk's unit, its end-state bit folded in */
	uint32_t abs_min;        /* in the walk's unit: states from here up are absorbing */
	uint32_t in_lds, has_limit;
	int32_t trim;            /* -1: none */
};

__device__ __forceinline__ uint32_t pos_byte_at(const u32x4p &w, int k)
{
	const uint32_t d = (k < 4) ? w.x : (k < 8) ? w.y : (k < 12) ? w.z : w.w;
	return (d >> (8 * (k & 3))) & 0xffu;
}

/* one workgroup = POS_WAVES wavefronts = 256 consecutive inputs, one input per lane, the table copied to LDS once */
template <bool BACK>
__global__ void __launch_bounds__(POS_THREADS)
walk_pos(const PosArgs a)
{
	typedef const uint16_t __attribute__((address_space(1))) *g_u16p;
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;
	typedef u32x4p __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	__shared__ uint16_t col[256];
	__shared__ uint16_t tab[POS_LDS_ENTRIES];
	const uint32_t tid = threadIdx.x;
	const bool in_lds = a.in_lds != 0u;
	const uint32_t C = a.C;
	col[tid] = ((g_u16p)(uintptr_t)a.col)[tid];
	if (in_lds)
		for (uint32_t e = tid; e < a.entries; e += POS_THREADS) tab[e] = ((g_u16p)(uintptr_t)a.tab)[e];
	__syncthreads();

	const g_u64p off = (g_u64p)(uintptr_t)a.off;
	const g_u32p dense = (g_u32p)(uintptr_t)a.tab;
	const uint64_t base = reinterpret_cast<uint64_t>(a.base);
	const uint64_t j = (uint64_t)blockIdx.x * POS_THREADS + tid;
	const bool valid = j < a.m;
	uint64_t i = j;
	if (valid && a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	const bool have = valid && i < a.n;              /* a pick beyond the lines: NO_POS, nothing read */
	const uint64_t limit = a.has_limit != 0u ? a.limit : off[a.n];
	uint64_t beg = 0, len = 0;
	if (have) {
		beg = off[i];
		const uint64_t e = off[i + 1];
		len = e > beg ? e - beg : 0u;
		if (beg > limit) len = 0u;                   /* the line clipped to the readable bytes: every load below stays inside */
		else if (len > limit - beg) len = limit - beg;
	}
	if (a.trim >= 0 && len != 0u && (uint32_t)((g_u8p)(base + beg))[len - 1u] == (uint32_t)a.trim) len--;
	uint64_t lo = 0, hi = len;
	if (have && a.from != nullptr) lo = ((g_u64p)(uintptr_t)a.from)[j];
	if (have && a.to != nullptr) {
		const uint64_t t = ((g_u64p)(uintptr_t)a.to)[j];
		hi = t < len ? t : len;
	}
	const bool walked = have && lo <= hi;
	const uint64_t total = walked ? hi - lo : 0u;    /* bytes of the range */

	const uint32_t end_bit = in_lds ? 1u : 0x80000000u;
	const uint32_t absorbing = a.abs_min;            /* (even in the LDS form: comparing the state with its bit still on is the same) */
	uint32_t s = a.start;
	uint64_t first = FSM_HIP_NO_POS, last = FSM_HIP_NO_POS;
	if (walked && (s & end_bit) != 0u) first = last = BACK ? hi : lo;   /* k = 0: the start state, before any byte */
	const uint32_t col_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)col;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;

	for (uint64_t t = 0;; t += 16u) {
		const bool live = t < total && (s & ~end_bit) < absorbing;
		if (!__any(live)) break;
		const uint32_t cnt = !live ? 0u : total - t < 16u ? (uint32_t)(total - t) : 16u;
		/* the chunk: walk byte k is byte k of w forward, byte 15 - k backward */
		u32x4p w = {0u, 0u, 0u, 0u};
		if (live) {
			if (!BACK) {
				const uint64_t at = beg + lo + t;        /* the chunk's first byte, from base */
				if (at + 16u <= limit) {
					w = *(g_chunkp)(base + at);
				} else {
					uint32_t d[4] = {0u, 0u, 0u, 0u};
					for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(base + at))[k] << ((k & 3u) * 8u);
					w = u32x4p{d[0], d[1], d[2], d[3]};
				}
			} else {
				const uint64_t e = beg + hi - t;         /* one past the chunk's last byte, from base: <= limit */
				if (e >= 16u) {
					w = *(g_chunkp)(base + e - 16u);
				} else {                                 /* the head of the text: nothing before base is read */
					uint32_t d[4] = {0u, 0u, 0u, 0u};
					for (uint32_t k = 0; k < cnt; k++) {
						const uint32_t q = 15u - k;
						d[q >> 2] |= (uint32_t)((g_u8p)(base + e - 1u))[-(int64_t)k] << ((q & 3u) * 8u);
					}
					w = u32x4p{d[0], d[1], d[2], d[3]};
				}
			}
		}
		uint32_t mask = 0u;                              /* bit k: the state after walk byte k is an end state */
		uint32_t c2[16];
#pragma unroll
		for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(col_at + pos_byte_at(w, BACK ? 15 - k : k) * 2u);
		if (in_lds) {
			if (__all(cnt == 16u || cnt == 0u)) {        /* whole chunks everywhere */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					sn = *(l_u16p)(uintptr_t)(tab_at + (sn & 0xfffeu) + c2[k]);
					mask |= (sn & 1u) << k;
				}
				s = cnt != 0u ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + (s & 0xfffeu) + c2[k]);
					s = (uint32_t)k < cnt ? sn : s;
					mask |= (sn & 1u) << k;
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)k < cnt) {
					s = dense[(uint64_t)(s & 0x7fffffffu) * C + c2[k]];
					mask |= (s >> 31) << k;
				}
			}
		}
		mask &= (1u << cnt) - 1u;                        /* bytes beyond cnt set no bit */
		if (mask != 0u) {
			const uint64_t c_lo = t + (uint32_t)__builtin_ctz(mask) + 1u, c_hi = t + (31u - (uint32_t)__builtin_clz(mask)) + 1u;   /* bytes walked */
			if (first == FSM_HIP_NO_POS) first = BACK ? hi - c_lo : lo + c_lo;
			last = BACK ? hi - c_hi : lo + c_hi;
		}
	}
	/* an absorbing end state: every later position accepts */
	if (walked && (s & ~end_bit) >= absorbing && (s & end_bit) != 0u) last = BACK ? lo : hi;
	if (valid && a.first_out != nullptr) ((g_u64w)(uintptr_t)a.first_out)[j] = first;
	if (valid && a.last_out != nullptr) ((g_u64w)(uintptr_t)a.last_out)[j] = last;
}

bool pos_have_device()
{
	int ndev = 0;
	return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

}   // namespace

/* the type is the library's own: its destructor is no exported symbol */
struct __attribute__((visibility("hidden"))) fsm_hip_pos_dfa {
	int device = 0;
	uint32_t entries = 0, C = 0, start = 0, abs_min = 0, in_lds = 0;
	DevBuf<unsigned char> d_tab;
	DevBuf<uint16_t> d_col;
	mutable std::mutex mu;                           /* one host-pointer call at a time on `own` */
	DevStream own;                                   /* the host-pointer form runs here, never on the NULL stream (last: it goes first) */
};

namespace fsmhip {
int pos_dfa_device(const fsm_hip_pos_dfa *pd) { return pd->device; }

PosView pos_dfa_view(const fsm_hip_pos_dfa *pd)
{
	PosView v;
	v.tab = pd->d_tab.p;
	v.col = pd->d_col.p;
	v.entries = pd->entries;
	v.C = pd->C;
	v.start = pd->start;
	v.abs_min = pd->abs_min;
	v.in_lds = pd->in_lds;
	return v;
}
}

extern "C" struct fsm_hip_pos_dfa *fsm_hip_pos_dfa_create(const struct fsm_hip_dfa *dfa)
{
	if (!pos_have_device()) { errno = ENODEV; return nullptr; }   /* no CPU path, as everywhere in this library */
	if (dfa == nullptr) { errno = EINVAL; return nullptr; }
	const Plan &p = *dfa_plan(dfa);
	const uint64_t entries = (uint64_t)p.S1 * p.C;
	if (entries == 0 || p.S1 > 0x7fffffffu || entries > 0xffffffffu) { errno = EINVAL; return nullptr; }
	struct fsm_hip_pos_dfa *pd = new (std::nothrow) fsm_hip_pos_dfa;
	if (pd == nullptr) { errno = ENOMEM; return nullptr; }
	pd->device = dfa_device(dfa);
	pd->entries = (uint32_t)entries;
	pd->C = p.C;
	pd->in_lds = entries <= POS_LDS_ENTRIES ? 1u : 0u;
	auto is_end = [&](uint32_t st) { return p.fin[st] != FSM_HIP_NO_MATCH ? 1u : 0u; };
	std::vector<uint16_t> col(256);
	bool ok = true;
	DevGuard dg(pd->device);
	if (!dg.ok()) { errno = ENODEV; ok = false; }
	if (pd->in_lds != 0u) {
		const uint32_t unit = p.C * 2u;              /* a row's bytes: (S1 - 1) * unit < 2^15, bit 0 is free */
		std::vector<uint16_t> img(entries);
		for (uint64_t e = 0; e < entries; e++) img[e] = (uint16_t)(p.dense[e] * unit | is_end(p.dense[e]));
		for (uint32_t b = 0; b < 256u; b++) col[b] = (uint16_t)(p.cls[b] * 2u);
		pd->start = p.start * unit | is_end(p.start);
		pd->abs_min = p.abs_min * unit;
		ok = ok && HIP_OK(pd->d_tab.upload_bytes(img.data(), entries * sizeof(uint16_t), 16));
	} else {
		std::vector<uint32_t> img(entries);
		for (uint64_t e = 0; e < entries; e++) img[e] = p.dense[e] | is_end(p.dense[e]) << 31;
		for (uint32_t b = 0; b < 256u; b++) col[b] = p.cls[b];
		pd->start = p.start | is_end(p.start) << 31;
		pd->abs_min = p.abs_min;
		ok = ok && HIP_OK(pd->d_tab.upload_bytes(img.data(), entries * sizeof(uint32_t), 16));
	}
	ok = ok && HIP_OK(pd->d_col.upload(col)) && HIP_OK(pd->own.create(hipStreamNonBlocking));
	if (ok) return pd;
	const int e = errno;
	delete pd;
	errno = e;
	return nullptr;
}

extern "C" void fsm_hip_pos_dfa_free(struct fsm_hip_pos_dfa *pd)
{
	if (pd == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(pd->device);
		delete pd;                                   /* (hipFree waits for the device: no walk still reads the image) */
	}
	errno = e;
}

extern "C" int fsm_hip_pos_dfa_in_lds(const struct fsm_hip_pos_dfa *pd) { return pd != nullptr && pd->in_lds != 0u ? 1 : 0; }

/* the arguments both forms refuse alike; *in: the batch as given */
static int pos_check(const struct fsm_hip_pos_dfa *pd, const struct fsm_hip_pos_batch *b, fsmhip::LineBatch *in)
{
	if (!pos_have_device()) { errno = ENODEV; return -1; }
	if (pd == nullptr) { errno = EINVAL; return -1; }
	if (!fsmhip::batch_shape(b, FSM_HIP_POS_BACKWARD, in)) return -1;
	if ((in->m + POS_THREADS - 1u) / POS_THREADS > 0x7fffffffu) { errno = ENOMEM; return -1; }
	return 0;
}

extern "C" int fsm_hip_exec_accept_pos_device(const struct fsm_hip_pos_dfa *pd, const struct fsm_hip_pos_batch *b, void *hip_stream)
{
	fsmhip::LineBatch in;
	if (pos_check(pd, b, &in) != 0 || !fsmhip::batch_device_ok(in)) return -1;
	if (in.m == 0 || (b->first_out == nullptr && b->last_out == nullptr)) return 0;
	DevGuard dg(pd->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	PosArgs a;
	a.tab = pd->d_tab.p;
	a.col = pd->d_col.p;
	a.base = static_cast<const uint8_t *>(in.base);
	a.off = in.off;
	a.pick = in.pick;
	a.from = b->from;
	a.to = b->to;
	a.first_out = b->first_out;
	a.last_out = b->last_out;
	a.n = in.n;
	a.m = in.m;
	a.limit = in.limit;
	a.has_limit = in.has_limit ? 1u : 0u;
	a.entries = pd->entries;
	a.C = pd->C;
	a.start = pd->start;
	a.abs_min = pd->abs_min;
	a.in_lds = pd->in_lds;
	a.trim = in.trim;
	const dim3 grid((unsigned)((in.m + POS_THREADS - 1u) / POS_THREADS)), block(POS_THREADS);
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if ((in.flags & FSM_HIP_POS_BACKWARD) != 0u) hipLaunchKernelGGL(walk_pos<true>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(walk_pos<false>, grid, block, 0, s, a);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

extern "C" int fsm_hip_exec_accept_pos(const struct fsm_hip_pos_dfa *pd, const struct fsm_hip_pos_batch *b)
{
	fsmhip::LineBatch host, in;
	if (pos_check(pd, b, &host) != 0 || !fsmhip::batch_host_arrays_ok(host)) return -1;
	if (host.m == 0 || (b->first_out == nullptr && b->last_out == nullptr)) return 0;
	DevGuard dg(pd->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	std::lock_guard<std::mutex> lock(pd->mu);
	hipStream_t s = pd->own;
	/* the batch staged in one allocation, from / to and room for the two outputs behind it */
	fsmhip::StagedBatch staged;
	if (!staged.stage(host, s, &in, {{b->from}, {b->to}, {b->first_out, false}, {b->last_out, false}})) return -1;
	auto fail = [&] {   /* the stream idle before the staging memory goes */
		const int e = errno;
		(void)hipStreamSynchronize(s);
		errno = e;
		return -1;
	};
	struct fsm_hip_pos_batch db = *b;
	db.base = in.base;
	db.limit = in.limit;
	db.off = in.off;
	db.pick = in.pick;
	db.from = staged.extra(0);
	db.to = staged.extra(1);
	db.first_out = staged.extra(2);
	db.last_out = staged.extra(3);
	const uint64_t n_m = host.m * 8u;
	if (fsm_hip_exec_accept_pos_device(pd, &db, s) != 0) return fail();
	if (b->first_out && !HIP_OK(hipMemcpyAsync(b->first_out, db.first_out, n_m, hipMemcpyDeviceToHost, s))) return fail();
	if (b->last_out && !HIP_OK(hipMemcpyAsync(b->last_out, db.last_out, n_m, hipMemcpyDeviceToHost, s))) return fail();
	if (!HIP_OK(hipStreamSynchronize(s))) return fail();
	return 0;
}
