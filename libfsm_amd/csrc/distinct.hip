/*
 * distinct.hip -- the distinct records of a packed text with their counts, on the device: sort | uniq -c without the sort.
 * include/fsm_hip.h, section "distinct", is the definition; distinct_seg.h holds the arithmetic (the trimmed length, the hash, the
 * slot word, the probe sequence, the chunk comparison), shared with tests/c/test_distinct_seg.cpp.
 *
 * A block of every pass is DST_RECORDS records, one per lane.
 *     dst_hash       the trimmed length of every record and, for keys up to DST_LONG_BYTES, its hash, chunk by chunk.  Longer
 *                    records are appended to a list (one atomic add per wavefront; the list lives in the class array, which is
 *                    written only later) and hashed by
 *     dst_hash_long  a wavefront per listed record, lane l the chunks l, l + 64, ...; the partial sums are added, which gives the
 *                    word the lane-by-lane sum gives.  Equal keys have equal lengths and take the same path.
 *     dst_insert     the table: open addressing, linear probing, a slot one u64 tag32(hash) << 32 | r, empty all ones.  A wavefront
 *                    first combines: the lowest lane that is left names its (hash, length, tag), the lanes that share them compare
 *                    their bytes with ITS bytes, and those that are equal become its followers; after DST_ROUNDS rounds every lane
 *                    that is no follower inserts -- the named lanes for their group, with its lowest r and its size, the others for
 *                    themselves -- all in one divergent call, and the followers take their slot from their lane.  Between the two, the
 *                    first lanes of wavefronts 1 .. 3 join thread 0 through LDS where their keys are equal.  An insert claims
 *                    the first empty slot of its chain by a compare-and-swap; on a slot with its tag it compares its key with the
 *                    key of the record the slot names, byte for byte, always, and where they are equal it lowers the slot by an
 *                    atomic min unless the slot holds a lower r already; otherwise the next slot.  Slots are never emptied, so a
 *                    key lives in one slot and the slot ends with the LOWEST r of its key.  One add per group to the slot's counter.
 *     dst_mark       first(r) = the slot of r names r; per block the pair (firsts, key bytes with the separator)
 *     (scan)         the exclusive scan of the block pairs by one workgroup (text.hip), the totals for the host
 *     dst_number     the block's own scan redone: the first of rank d writes first[d], count[d] from its slot's counter, doff[d],
 *                    src[d], the index of the output blocks it covers -- and its rank into the counter's place
 *     dst_class      class[r] = the rank its slot now holds
 * The write pass is the extraction's (extract.hip, ext_write) over doff / src.
 * Coherence: a slot is read and written inside dst_insert by agent-scope atomics alone (a returning compare-and-swap, a min, a
 * relaxed atomic load) -- the XCDs do not see each other's L2, a plain load could keep an old word for ever.  The counters are
 * only added to.  Everything else a kernel reads was written by an EARLIER kernel or is the caller's read-only input.
 * Every global access names its address space (no FLAT instruction); no byte outside [bytes, bytes + min(off[R], nbytes)) is read;
 * every index read from an array is clamped to the array it is used on; every store goes below the sizes the host counted.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "hip_host.h"
#include "match_marks.h"
#include "extract.h"
#include "distinct.h"
#include "distinct_seg.h"

using namespace fsmhip;

namespace {

constexpr uint32_t DST_WAVES = DST_THREADS / 64u;
constexpr uint32_t DST_ROUNDS = 4;                          /* rounds of the wavefront's combine before every lane inserts */
constexpr uint32_t DST_LONG_BLOCKS = 1024;                  /* the grid of dst_hash_long, at most */

typedef uint32_t u32x4d __attribute__((ext_vector_type(4)));
typedef u32x4d __attribute__((aligned(1))) u32x4d_any;
typedef uint64_t u64x2d __attribute__((ext_vector_type(2)));
typedef const u32x4d_any __attribute__((address_space(1))) *g_chunkp;
typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
typedef uint32_t __attribute__((address_space(1))) *g_u32w;
typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
typedef uint64_t __attribute__((address_space(1))) *g_u64w;
typedef u64x2d __attribute__((address_space(1))) *g_u64x2w;
typedef const u64x2d __attribute__((address_space(1))) *g_u64x2p;

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

/* the bytes that may be read: off[R] and nbytes, whichever is less */
__device__ __forceinline__ uint64_t read_limit(const DstRun &a) { return min64(((g_u64p)(uintptr_t)a.off)[a.R], a.nbytes); }

/* record r: its first byte and its clipped bytes (the extraction's clip) */
__device__ __forceinline__ void record_of(const DstRun &a, uint64_t r, uint64_t limit, uint64_t *beg, uint64_t *raw)
{
	marks_clip(((g_u64p)(uintptr_t)a.off)[r], ((g_u64p)(uintptr_t)a.off)[r + 1u], limit, beg, raw);
}

/* the chunk of n bytes (1 .. 16) at byte `at`, all below the limit, masked: one load where sixteen bytes may be read, byte loads
 * at the end of the text */
__device__ __forceinline__ void load_chunk(uint64_t bx, uint64_t at, uint32_t n, uint64_t limit, uint64_t *lo, uint64_t *hi)
{
	uint64_t x0 = 0, x1 = 0;
	if (limit >= 16u && at <= limit - 16u) {
		const u32x4d v = *(g_chunkp)(bx + at);
		x0 = v.x | (uint64_t)v.y << 32;
		x1 = v.z | (uint64_t)v.w << 32;
	} else {
		for (uint32_t k = 0; k < n; k++) {
			if (at + k >= limit) break;
			const uint64_t b = (uint64_t)((g_u8p)bx)[at + k] << ((k & 7u) * 8u);
			x0 |= k < 8u ? b : 0u;
			x1 |= k < 8u ? 0u : b;
		}
	}
	*lo = x0 & dst_mask_lo(n);
	*hi = x1 & dst_mask_hi(n);
}

/* the keys of len bytes at ba and at bb are equal, byte for byte */
__device__ __forceinline__ bool key_equal(uint64_t bx, uint64_t ba, uint64_t bb, uint64_t len, uint64_t limit)
{
	if (ba == bb) return true;
	const uint64_t nch = dst_chunks(len);
#pragma unroll 1
	for (uint64_t i = 0; i < nch; i++) {
		const uint32_t n = dst_chunk_bytes(len, i);
		uint64_t alo, ahi, blo, bhi;
		load_chunk(bx, ba + i * DST_CHUNK, n, limit, &alo, &ahi);
		load_chunk(bx, bb + i * DST_CHUNK, n, limit, &blo, &bhi);
		if (!dst_chunk_equal(alo, ahi, blo, bhi, n)) return false;
	}
	return true;
}

__device__ __forceinline__ uint32_t tag_of(const DstRun &a, uint64_t r) { return a.tag != nullptr ? ((g_u32p)(uintptr_t)a.tag)[r] : 0u; }

/* pass 1a (grid: dst_blocks(R)) */
__global__ void __launch_bounds__(DST_THREADS)
dst_hash(const DstRun a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
	bool is_long = false;
	if (r < a.R) {
		uint64_t beg, raw;
		record_of(a, r, limit, &beg, &raw);
		const uint32_t last = raw != 0u ? ((g_u8p)bx)[beg + raw - 1u] : 0u;
		const uint64_t len = dst_trimmed(raw, last, a.trim);
		((g_u64w)(uintptr_t)a.len)[r] = len;
		if (a.weak) {
			((g_u64w)(uintptr_t)a.hash)[r] = dst_weak_hash(len, a.slots);
		} else if (len <= DST_LONG_BYTES) {
			const uint64_t nch = dst_chunks(len);
			uint64_t sum = 0;
#pragma unroll 1
			for (uint64_t i = 0; i < nch; i++) {
				uint64_t lo, hi;
				load_chunk(bx, beg + i * DST_CHUNK, dst_chunk_bytes(len, i), limit, &lo, &hi);
				sum += dst_chunk_hash(lo, hi, i);
			}
			((g_u64w)(uintptr_t)a.hash)[r] = dst_hash_finish(sum, len, tag_of(a, r));
		} else {
			is_long = true;
		}
	}
	const uint64_t m = __ballot(is_long);
	if (m != 0u) {                                   /* one add per wavefront; the order of the list decides nothing */
		const uint32_t lead = (uint32_t)__builtin_ctzll(m);
		uint64_t at = 0;
		if (lane == lead)
			at = __hip_atomic_fetch_add((g_u64w)(uintptr_t)(a.pairs + 2u * dst_blocks(a.R) + 3u), (uint64_t)__builtin_popcountll(m), __ATOMIC_RELAXED,
			                            __HIP_MEMORY_SCOPE_AGENT);
		at = __shfl(at, (int)lead, 64) + (uint64_t)__builtin_popcountll(m & (((uint64_t)1 << lane) - 1u));
		if (is_long && at < a.R) ((g_u32w)(uintptr_t)a.cls)[at] = (uint32_t)r;
	}
}

/* pass 1b: a wavefront per long record; every lane of a wavefront runs the same number of steps */
__global__ void __launch_bounds__(DST_THREADS)
dst_hash_long(const DstRun a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t nlong = min64(((g_u64p)(uintptr_t)a.pairs)[2u * dst_blocks(a.R) + 3u], a.R);
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
#pragma unroll 1
	for (uint64_t w = (uint64_t)blockIdx.x * DST_WAVES + (threadIdx.x >> 6); w < nlong; w += (uint64_t)gridDim.x * DST_WAVES) {
		const uint64_t r = min64(((g_u32p)(uintptr_t)a.cls)[w], a.R - 1u);
		uint64_t beg, raw;
		record_of(a, r, limit, &beg, &raw);
		const uint64_t len = min64(((g_u64p)(uintptr_t)a.len)[r], raw), nch = dst_chunks(len);
		uint64_t sum = 0;
#pragma unroll 1
		for (uint64_t i = lane; i < nch; i += 64u) {
			uint64_t lo, hi;
			load_chunk(bx, beg + i * DST_CHUNK, dst_chunk_bytes(len, i), limit, &lo, &hi);
			sum += dst_chunk_hash(lo, hi, i);
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
		if (lane == 0u) ((g_u64w)(uintptr_t)a.hash)[r] = dst_hash_finish(sum, len, tag_of(a, r));
	}
}

/* record r (key at beg, len bytes, tag) into the table: the slot of its key.  The chain is at most `slots` long: at most half the
 * slots are ever taken. */
__device__ __forceinline__ uint64_t insert(const DstRun &a, uint64_t hash, uint64_t r, uint64_t beg, uint64_t len, uint32_t tag, uint64_t limit)
{
	const g_u64w tab = (g_u64w)(uintptr_t)a.table;
	const uint64_t bx = (uint64_t)(uintptr_t)a.bytes, mine = dst_slot_word(hash, r);
	uint64_t i = dst_probe_start(hash, a.slots);
#pragma unroll 1
	for (uint64_t step = 0; step < a.slots; step++, i = dst_probe_next(i, a.slots)) {
		uint64_t cur = __hip_atomic_load(tab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == DST_EMPTY) {
			uint64_t expect = DST_EMPTY;
			if (__hip_atomic_compare_exchange_strong(tab + i, &expect, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return i;
			cur = expect;                            /* another record took it meanwhile: is it of this key? */
		}
		if (!dst_same_tag(cur, mine)) continue;
		const uint64_t q = dst_slot_record(cur);
		if (q >= a.R) continue;
		if (q != r) {
			if (((g_u64p)(uintptr_t)a.len)[q] != len || tag_of(a, q) != tag) continue;
			if (!key_equal(bx, beg, ((g_u64p)(uintptr_t)a.off)[q], len, limit)) continue;
			if (q > r) (void)__hip_atomic_fetch_min(tab + i, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		return i;
	}
	return i;
}

/* pass 2 (grid: dst_blocks(R)); lanes of a wavefront hold ascending r, so the lowest lane of a group holds its lowest r */
__global__ void __launch_bounds__(DST_THREADS)
dst_insert(const DstRun a)
{
	__shared__ uint64_t post[4];                     /* thread 0's hash, length and first byte; its slot */
	__shared__ uint32_t post_tag, extra;             /* its tag; the records of the wavefronts that joined it */
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
	const bool valid = r < a.R;
	uint64_t hash = 0, len = 0, beg = 0;
	uint32_t tag = 0;
	if (valid) {
		uint64_t raw;
		record_of(a, r, limit, &beg, &raw);
		len = min64(((g_u64p)(uintptr_t)a.len)[r], raw);
		hash = ((g_u64p)(uintptr_t)a.hash)[r];
		tag = tag_of(a, r);
	}
	bool follower = false;
	uint32_t leader = lane, group = 1u;
	uint64_t rem = __ballot(valid);
#pragma unroll 1
	for (uint32_t round = 0; round < DST_ROUNDS && rem != 0u; round++) {
		const int src = (int)__builtin_ctzll(rem);
		const uint64_t shash = __shfl(hash, src, 64), slen = __shfl(len, src, 64), sbeg = __shfl(beg, src, 64);
		const uint32_t stag = (uint32_t)__shfl((int)tag, src, 64);
		bool mine = valid && !follower && (rem >> lane & 1u) != 0u && hash == shash && len == slen && tag == stag;
		if (mine) mine = key_equal(bx, beg, sbeg, len, limit);
		const uint64_t same = __ballot(mine);        /* the named lane is among them */
		if (mine && lane != (uint32_t)src) { follower = true; leader = (uint32_t)src; }
		if (lane == (uint32_t)src) group = (uint32_t)__builtin_popcountll(same);
		rem &= ~same;
	}
	/* ... and the workgroup, for the one key that can be hot: the first lane of wavefronts 1 .. 3 -- the lane its first round named --
	 * compares its key with that of thread 0, which holds the block's lowest r, and where they are equal hands it its group through
	 * LDS and takes its slot from there.  64 M equal records are then R / 256 inserts and adds, not R / 64. */
	const uint64_t vmask = __ballot(valid);
	const bool first_lane = valid && lane == (uint32_t)__builtin_ctzll(vmask | ((uint64_t)1 << 63));
	if (threadIdx.x == 0u) {
		post[0] = hash;
		post[1] = len;
		post[2] = beg;
		post_tag = tag;
		extra = 0u;
	}
	__syncthreads();
	bool joins = false;
	if (first_lane && threadIdx.x >= 64u && hash == post[0] && len == post[1] && tag == post_tag && key_equal(bx, beg, post[2], len, limit)) {
		joins = true;
		atomicAdd(&extra, group);
	}
	__syncthreads();
	if (threadIdx.x == 0u) group += extra;
	const bool inserts = valid && !follower && !joins;
	uint64_t slot = 0;
	if (inserts) {
		slot = insert(a, hash, r, beg, len, tag, limit);
		(void)__hip_atomic_fetch_add((g_u64w)(uintptr_t)a.cnt + slot, (uint64_t)group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	if (threadIdx.x == 0u) post[3] = slot;
	__syncthreads();
	if (joins) slot = post[3];
	slot = __shfl(slot, (int)leader, 64);
	if (valid) ((g_u64w)(uintptr_t)a.hash)[r] = slot;
}

/* the slot of record r as the insert pass left it, inside the table whatever the array holds */
__device__ __forceinline__ uint64_t slot_of(const DstRun &a, uint64_t r) { return ((g_u64p)(uintptr_t)a.hash)[r] & (a.slots - 1u); }

/* r is the first of its key, and the bytes its key takes in the text of the keys */
__device__ __forceinline__ void first_of(const DstRun &a, uint64_t r, uint64_t *cnt, uint64_t *len)
{
	*cnt = *len = 0;
	if (r >= a.R) return;
	const uint64_t w = __hip_atomic_load((g_u64w)(uintptr_t)a.table + slot_of(a, r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (w == DST_EMPTY || dst_slot_record(w) != r) return;
	*cnt = 1u;
	*len = ((g_u64p)(uintptr_t)a.len)[r] + (a.sep >= 0 ? 1u : 0u);
}

/* pass 3a (grid: dst_blocks(R)) */
__global__ void __launch_bounds__(DST_THREADS)
dst_mark(const DstRun a)
{
	__shared__ uint64_t wtot[DST_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t cnt, len;
	first_of(a, (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x, &cnt, &len);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		cnt += __shfl_xor(cnt, d, 64);
		len += __shfl_xor(len, d, 64);
	}
	if (lane == 0u) { wtot[wave][0] = cnt; wtot[wave][1] = len; }
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint64_t sc = 0, sb = 0;
#pragma unroll
		for (uint32_t w = 0; w < DST_WAVES; w++) { sc += wtot[w][0]; sb += wtot[w][1]; }
		*(g_u64x2w)(uintptr_t)(a.pairs + 2u * blockIdx.x) = u64x2d{sc, sb};
		if (blockIdx.x == 0u) ((g_u64w)(uintptr_t)a.pairs)[2u * dst_blocks(a.R) + 2u] = read_limit(a);   /* rides along to the host */
	}
}

/* pass 3b (grid: dst_blocks(R); D >= 1): the rank of a first = pairs[b] (scanned) + the firsts of the block before it */
__global__ void __launch_bounds__(DST_THREADS)
dst_number(const DstRun a)
{
	__shared__ uint64_t wtot[DST_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	uint64_t cnt, len;
	first_of(a, r, &cnt, &len);
	uint64_t xc = cnt, xl = len;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t yc = __shfl_up(xc, d, 64), yl = __shfl_up(xl, d, 64);
		if (lane >= (uint32_t)d) { xc += yc; xl += yl; }
	}
	if (lane == 63u) { wtot[wave][0] = xc; wtot[wave][1] = xl; }
	__syncthreads();
	const u64x2d base = *(g_u64x2p)(uintptr_t)(a.pairs + 2u * blockIdx.x);
	uint64_t d = base.x + (xc - cnt), p = base.y + (xl - len);
#pragma unroll
	for (uint32_t w = 0; w < DST_WAVES; w++) {
		d += w < wave ? wtot[w][0] : 0u;
		p += w < wave ? wtot[w][1] : 0u;
	}
	if (cnt != 0u && d < a.D) {
		const g_u64w ct = (g_u64w)(uintptr_t)a.cnt + slot_of(a, r);
		((g_u64w)(uintptr_t)a.first)[d] = r;
		((g_u64w)(uintptr_t)a.count)[d] = *ct;
		*ct = d;                                     /* the slot's dense number, for dst_class */
		if (a.doff != nullptr) {
			((g_u64w)(uintptr_t)a.doff)[d] = p;
			((g_u64w)(uintptr_t)a.src)[d] = ((g_u64p)(uintptr_t)a.off)[r];
			if (a.bfirst != nullptr && len != 0u)        /* keys with bytes tile the output: one covers each block boundary */
				for (uint64_t g = (p + EXT_BLOCK - 1u) / EXT_BLOCK; g < a.ngb && g * EXT_BLOCK < p + len; g++) ((g_u64w)(uintptr_t)a.bfirst)[g] = d;
		}
	}
	if (blockIdx.x == 0u && threadIdx.x == 0u && a.doff != nullptr) {
		((g_u64w)(uintptr_t)a.doff)[a.D] = a.total;
		if (a.bfirst != nullptr) ((g_u64w)(uintptr_t)a.bfirst)[a.ngb] = a.D;
	}
}

/* pass 3c (grid: dst_blocks(R); D >= 1) */
__global__ void __launch_bounds__(DST_THREADS)
dst_class(const DstRun a)
{
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	if (r < a.R) ((g_u32w)(uintptr_t)a.cls)[r] = (uint32_t)min64(((g_u64p)(uintptr_t)a.cnt)[slot_of(a, r)], a.D - 1u);
}

int launched() { return HIP_OK(hipGetLastError()) ? 0 : -1; }

}   // namespace

namespace fsmhip {

int dst_launch_hash(const DstRun &r, hipStream_t s)
{
	const uint64_t nb = dst_blocks(r.R);
	hipLaunchKernelGGL(dst_hash, dim3((unsigned)nb), dim3(DST_THREADS), 0, s, r);
	if (launched() != 0) return -1;
	if (r.weak) return 0;                            /* no record is listed */
	hipLaunchKernelGGL(dst_hash_long, dim3((unsigned)(nb < DST_LONG_BLOCKS ? nb : DST_LONG_BLOCKS)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

int dst_launch_insert(const DstRun &r, hipStream_t s)
{
	hipLaunchKernelGGL(dst_insert, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

int dst_launch_mark(const DstRun &r, hipStream_t s)
{
	hipLaunchKernelGGL(dst_mark, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

int dst_launch_number(const DstRun &r, hipStream_t s)
{
	if (r.D == 0) return 0;
	hipLaunchKernelGGL(dst_number, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	if (launched() != 0) return -1;
	hipLaunchKernelGGL(dst_class, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

}   // namespace fsmhip
