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
 * The lookup (include/fsm_hip.h, "find"; find_seg.h) reads the table a finished object keeps: dst_hash and dst_hash_long over the
 * PROBE text with the dictionary's slots, then
 *     fnd_probe      a lane per probe record of at most DST_LONG_BYTES: its chain walked without a claim, the keys compared between
 *                    the two texts, the class from the slot's dense number
 *     fnd_probe_long a wavefront per listed record: the chain walked by all lanes alike, a candidate's chunks compared 64 at a time,
 *                    a ballot ends the comparison at the first round with a difference
 *     fnd_mark       a wavefront's ballot of class != NONE is one word of the bitmap; per block the pair (present, absent)
 *     (scan)         the same scan of the block pairs; P stays on the device
 *     fnd_pick       the block's scan redone: the present records first, the absent behind them, both ascending
 * They write nothing of the dictionary and hold no read-modify-write: any number of lookups may read one table at once.
 * Coherence: a slot is read and written inside dst_insert by agent-scope atomics alone (a returning compare-and-swap, a min, a
 * relaxed atomic load) -- the XCDs do not see each other's L2, a plain load could keep an old word for ever.  The counters are
 * only added to.  Everything else a kernel reads was written by an EARLIER kernel or is the caller's read-only input.
 * Every global access names its address space (no FLAT instruction); no byte outside [bytes, bytes + min(off[R], nbytes)) is read;
 * every index read from an array is clamped to the array it is used on; every store goes below the sizes the host counted.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "match_marks.h"
#include "extract.h"
#include "distinct_seg.h"
#include "find_seg.h"
#include "sort.h"
#include "text_objects.h"

namespace fsmhip {

constexpr uint32_t DST_THREADS = 256;
constexpr uint32_t DST_RECORDS = DST_THREADS;               /* records of a block of every pass, one per lane */
constexpr uint32_t DST_LONG_BYTES = 256;                    /* keys above it are hashed by a wavefront each */
constexpr uint32_t DST_PAIRS_EXTRA = 4;                     /* behind the block pairs: the two totals, the limit, the long records */

constexpr uint64_t dst_blocks(uint64_t R) { return (R + DST_RECORDS - 1u) / DST_RECORDS; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself. */
struct DstRun {
	/* the packed text */
	const uint64_t *off = nullptr;           /* R + 1 */
	const unsigned char *bytes = nullptr;
	const uint32_t *tag = nullptr;           /* R, or null */
	uint64_t R = 0, nbytes = 0;
	int trim = -1, sep = -1;
	bool weak = false;
	/* internal, sized by R */
	uint64_t slots = 0;
	uint64_t *len = nullptr;                 /* R: the trimmed lengths */
	uint64_t *hash = nullptr;                /* R: the hashes; from the insert pass on, the slot of each record */
	uint32_t *cls = nullptr;                 /* R: class; until the insert pass, the list of the long records */
	uint64_t *table = nullptr, *cnt = nullptr;   /* slots each: the slot words; the records of a slot, then its dense number */
	uint64_t *pairs = nullptr;               /* per block (firsts, key bytes), then (scanned) those before it; + DST_PAIRS_EXTRA */
	/* the object's arrays, sized after the scan */
	uint64_t *first = nullptr, *count = nullptr;   /* D each */
	uint64_t *doff = nullptr;                /* D + 1, or null (NO_TEXT) */
	uint64_t *src = nullptr;                 /* D: where each key's bytes begin in `bytes`; with doff */
	uint64_t *bfirst = nullptr;              /* ngb + 1: the key that covers the first byte of each output block; with doff */
	uint64_t D = 0, total = 0, ngb = 0;      /* known after the scan */
};

/* the lookup's arguments: the probe text as a run of the hash passes, the dictionary read-only, the outputs */
struct FndRun {
	DstRun p;                                /* off, bytes, tag, R, nbytes, trim of the probe; weak and slots the DICTIONARY's; len, hash,
	                                            pairs its own; cls the list of its long records */
	const uint64_t *k_off = nullptr;         /* the dictionary's source text: R_dict + 1 */
	const unsigned char *k_bytes = nullptr;
	const uint32_t *k_tag = nullptr;         /* R_dict, or null */
	const uint64_t *k_len = nullptr;         /* R_dict: the trimmed lengths */
	const uint64_t *table = nullptr, *cnt = nullptr;   /* slots each: the slot words, the dense numbers */
	uint64_t k_R = 0, k_limit = 0, D = 0;    /* its records, the bytes of its source that may be read, its keys */
	uint32_t *out = nullptr;                 /* R: class */
	uint64_t *bitmap = nullptr;              /* ceil(R / 64) */
	uint64_t *pick = nullptr;                /* R, or null (NO_PICK) */
};

}

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

/* ---- the lookup: the records of a probe text among the keys of a finished table (find_seg.h) ---- */

/* the keys of len bytes at ba of one text and at bb of another are equal, byte for byte */
__device__ __forceinline__ bool key_equal2(uint64_t ax, uint64_t ba, uint64_t alimit, uint64_t bx, uint64_t bb, uint64_t blimit, uint64_t len)
{
	const uint64_t nch = dst_chunks(len);
#pragma unroll 1
	for (uint64_t i = 0; i < nch; i++) {
		const uint32_t n = dst_chunk_bytes(len, i);
		uint64_t alo, ahi, blo, bhi;
		load_chunk(ax, ba + i * DST_CHUNK, n, alimit, &alo, &ahi);
		load_chunk(bx, bb + i * DST_CHUNK, n, blimit, &blo, &bhi);
		if (!dst_chunk_equal(alo, ahi, blo, bhi, n)) return false;
	}
	return true;
}

/* the table as another kernel, perhaps on another XCD, left it: agent-scope loads, as first_of reads it */
__device__ __forceinline__ uint64_t slot_word_of(const FndRun &f, uint64_t i)
{
	return __hip_atomic_load((g_u64w)(uintptr_t)f.table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t dense_of(const FndRun &f, uint64_t i)
{
	return (uint32_t)min64(__hip_atomic_load((g_u64w)(uintptr_t)f.cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), f.D - 1u);
}
__device__ __forceinline__ uint32_t key_tag_of(const FndRun &f, uint64_t q) { return f.k_tag != nullptr ? ((g_u32p)(uintptr_t)f.k_tag)[q] : 0u; }

/* a probe record goes to fnd_probe_long exactly when dst_hash listed it */
__device__ __forceinline__ bool probe_is_long(const FndRun &f, uint64_t len) { return !f.p.weak && len > DST_LONG_BYTES; }

/* pass 2a (grid: dst_blocks(R); D >= 1): a lane per record */
__global__ void __launch_bounds__(DST_THREADS)
fnd_probe(const FndRun f)
{
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	if (r >= f.p.R) return;
	const uint64_t limit = read_limit(f.p), bx = (uint64_t)(uintptr_t)f.p.bytes, kx = (uint64_t)(uintptr_t)f.k_bytes;
	uint64_t beg, raw;
	record_of(f.p, r, limit, &beg, &raw);
	const uint64_t len = min64(((g_u64p)(uintptr_t)f.p.len)[r], raw);
	if (probe_is_long(f, len)) return;
	const uint32_t tag = tag_of(f.p, r);
	((g_u32w)(uintptr_t)f.out)[r] = fnd_lookup(
		((g_u64p)(uintptr_t)f.p.hash)[r], f.p.slots, f.k_R, [&](uint64_t i) { return slot_word_of(f, i); },
		[&](uint64_t q) {
			if (((g_u64p)(uintptr_t)f.k_len)[q] != len || key_tag_of(f, q) != tag) return false;
			return key_equal2(bx, beg, limit, kx, ((g_u64p)(uintptr_t)f.k_off)[q], f.k_limit, len);
		},
		[&](uint64_t i) { return dense_of(f, i); });
}

/* pass 2b (D >= 1, not under the weak hash): a wavefront per listed record.  What the lanes branch on -- the list, the record, the
 * slot words, the ballots -- is the same in all of them: the wavefront walks the chain as one. */
__global__ void __launch_bounds__(DST_THREADS)
fnd_probe_long(const FndRun f)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t nlong = min64(((g_u64p)(uintptr_t)f.p.pairs)[2u * dst_blocks(f.p.R) + 3u], f.p.R);
	const uint64_t limit = read_limit(f.p), bx = (uint64_t)(uintptr_t)f.p.bytes, kx = (uint64_t)(uintptr_t)f.k_bytes;
#pragma unroll 1
	for (uint64_t w = (uint64_t)blockIdx.x * DST_WAVES + (threadIdx.x >> 6); w < nlong; w += (uint64_t)gridDim.x * DST_WAVES) {
		const uint64_t r = min64(((g_u32p)(uintptr_t)f.p.cls)[w], f.p.R - 1u);
		uint64_t beg, raw;
		record_of(f.p, r, limit, &beg, &raw);
		const uint64_t len = min64(((g_u64p)(uintptr_t)f.p.len)[r], raw), nch = dst_chunks(len);
		const uint32_t tag = tag_of(f.p, r);
		const uint32_t cls = fnd_lookup(
			((g_u64p)(uintptr_t)f.p.hash)[r], f.p.slots, f.k_R, [&](uint64_t i) { return slot_word_of(f, i); },
			[&](uint64_t q) {
				if (((g_u64p)(uintptr_t)f.k_len)[q] != len || key_tag_of(f, q) != tag) return false;
				const uint64_t kbeg = ((g_u64p)(uintptr_t)f.k_off)[q];
#pragma unroll 1
				for (uint64_t base = 0; base < nch; base += 64u) {       /* ceil(nch / 64) rounds at the most */
					const uint64_t i = base + lane;
					bool differs = false;
					if (i < nch) {
						const uint32_t n = dst_chunk_bytes(len, i);
						uint64_t alo, ahi, blo, bhi;
						load_chunk(bx, beg + i * DST_CHUNK, n, limit, &alo, &ahi);
						load_chunk(kx, kbeg + i * DST_CHUNK, n, f.k_limit, &blo, &bhi);
						differs = !dst_chunk_equal(alo, ahi, blo, bhi, n);
					}
					if (__ballot(differs) != 0u) return false;
				}
				return true;
			},
			[&](uint64_t i) { return dense_of(f, i); });
		if (lane == 0u) ((g_u32w)(uintptr_t)f.out)[r] = cls;
	}
}

__device__ __forceinline__ bool is_present(const FndRun &f, uint64_t r) { return r < f.p.R && ((g_u32p)(uintptr_t)f.out)[r] != FND_NONE; }

/* pass 3 (grid: dst_blocks(R)): the bitmap word of a wavefront is 4 * block + wave; the block's pair (present, absent) */
__global__ void __launch_bounds__(DST_THREADS)
fnd_mark(const FndRun f)
{
	__shared__ uint32_t wtot[DST_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	const uint64_t m = __ballot(is_present(f, r));
	if (lane == 0u) {
		if (fnd_bitmap_word(r) < fnd_bitmap_words(f.p.R)) ((g_u64w)(uintptr_t)f.bitmap)[fnd_bitmap_word(r)] = m;
		wtot[wave] = (uint32_t)__builtin_popcountll(m);
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint64_t present = 0;
#pragma unroll
		for (uint32_t w = 0; w < DST_WAVES; w++) present += wtot[w];
		const uint64_t records = min64(f.p.R - r, DST_RECORDS);
		*(g_u64x2w)(uintptr_t)(f.p.pairs + 2u * blockIdx.x) = u64x2d{present, records - present};
	}
}

/* pass 4 (grid: dst_blocks(R)): before(r) = pairs[b] (scanned) + the present records of the block below r */
__global__ void __launch_bounds__(DST_THREADS)
fnd_pick(const FndRun f)
{
	__shared__ uint32_t wtot[DST_WAVES];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t r = (uint64_t)blockIdx.x * DST_RECORDS + threadIdx.x;
	const bool present = is_present(f, r);
	const uint64_t m = __ballot(present);
	if (lane == 0u) wtot[wave] = (uint32_t)__builtin_popcountll(m);
	__syncthreads();
	uint64_t before = ((g_u64p)(uintptr_t)f.p.pairs)[2u * blockIdx.x] + (uint64_t)__builtin_popcountll(m & (((uint64_t)1 << lane) - 1u));
#pragma unroll
	for (uint32_t w = 0; w < DST_WAVES; w++) before += w < wave ? wtot[w] : 0u;
	const uint64_t P = ((g_u64p)(uintptr_t)f.p.pairs)[2u * dst_blocks(f.p.R)];
	if (r >= f.p.R || before > r) return;
	const uint64_t at = present ? fnd_pick_present(before) : fnd_pick_absent(r, before, P);
	if (at < f.p.R) ((g_u64w)(uintptr_t)f.pick)[at] = r;
}

int launched() { return HIP_OK(hipGetLastError()) ? 0 : -1; }

}   // namespace

namespace fsmhip {

/* each on stream s, the object's device current, R >= 1; 0, or -1 + errno */
static int dst_launch_hash(const DstRun &r, hipStream_t s)
{
	const uint64_t nb = dst_blocks(r.R);
	hipLaunchKernelGGL(dst_hash, dim3((unsigned)nb), dim3(DST_THREADS), 0, s, r);
	if (launched() != 0) return -1;
	if (r.weak) return 0;                            /* no record is listed */
	hipLaunchKernelGGL(dst_hash_long, dim3((unsigned)(nb < DST_LONG_BLOCKS ? nb : DST_LONG_BLOCKS)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

static int dst_launch_insert(const DstRun &r, hipStream_t s)
{
	hipLaunchKernelGGL(dst_insert, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

static int dst_launch_mark(const DstRun &r, hipStream_t s)
{
	hipLaunchKernelGGL(dst_mark, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

static int dst_launch_number(const DstRun &r, hipStream_t s)
{
	if (r.D == 0) return 0;
	hipLaunchKernelGGL(dst_number, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	if (launched() != 0) return -1;
	hipLaunchKernelGGL(dst_class, dim3((unsigned)dst_blocks(r.R)), dim3(DST_THREADS), 0, s, r);
	return launched();
}

/* the lookup's three launches, D >= 1 for the first */
static int fnd_launch_probe(const FndRun &f, hipStream_t s)
{
	const uint64_t nb = dst_blocks(f.p.R);
	hipLaunchKernelGGL(fnd_probe, dim3((unsigned)nb), dim3(DST_THREADS), 0, s, f);
	if (launched() != 0) return -1;
	if (f.p.weak) return 0;                          /* no record is listed */
	hipLaunchKernelGGL(fnd_probe_long, dim3((unsigned)(nb < DST_LONG_BLOCKS ? nb : DST_LONG_BLOCKS)), dim3(DST_THREADS), 0, s, f);
	return launched();
}

static int fnd_launch_mark(const FndRun &f, hipStream_t s)
{
	hipLaunchKernelGGL(fnd_mark, dim3((unsigned)dst_blocks(f.p.R)), dim3(DST_THREADS), 0, s, f);
	return launched();
}

static int fnd_launch_pick(const FndRun &f, hipStream_t s)
{
	hipLaunchKernelGGL(fnd_pick, dim3((unsigned)dst_blocks(f.p.R)), dim3(DST_THREADS), 0, s, f);
	return launched();
}

}   // namespace fsmhip

/* ---- the fronts: the distinct records as an object of five event pairs (front.h) -------------------------------------------------
 * hash -> insert -> mark -> the scan of the block pairs by one workgroup -> ONE wait for D, the key bytes and the read limit -> the
 * allocation -> number -> write, which is the extraction's write pass over doff / src.  Five event pairs: mark + scan and number
 * are reported together, so the wait and the allocation lie in neither. */
extern "C" size_t fsm_hip_distinct_long_bytes(void) { return fsmhip::DST_LONG_BYTES; }

extern "C" size_t fsm_hip_distinct_table_slots(size_t R)
{
	if ((uint64_t)R > fsmhip::DST_MAX_RECORDS) { errno = EOVERFLOW; return 0; }
	return (size_t)fsmhip::dst_table_slots(R);
}

struct __attribute__((visibility("hidden"))) fsm_hip_distinct : RunObject<5> {   /* hash, insert, mark + scan, number, write */
	size_t D = 0;                            /* (m is R) */
	uint64_t nbytes = 0;
	int sep = -1;                            /* the separator the keys were written with */
	DevBuf<uint64_t> d_len, d_hash;          /* R each: internal */
	DevBuf<uint32_t> d_class;                /* R */
	DevBuf<uint64_t> d_table, d_cnt;         /* one per slot: internal */
	DevBuf<uint64_t> d_pairs;                /* per block of records, + DST_PAIRS_EXTRA: internal */
	DevBuf<uint64_t> d_first, d_count;       /* D */
	DevBuf<uint64_t> d_doff;                 /* D + 1; NULL under NO_TEXT */
	DevBuf<uint64_t> d_src;                  /* D: internal */
	DevBuf<uint64_t> d_bfirst;               /* per block of the output, + 1: internal */
	DevBuf<unsigned char> d_dbytes;          /* nbytes, in whole blocks */
	DevBuf<uint64_t> own_off;                /* the host form's staged input */
	DevBuf<unsigned char> own_bytes;
	DevBuf<uint32_t> own_tag;
	fsmhip::DstRun src;                      /* what a lookup needs: the source off, bytes, tag, R, nbytes, trim, weak and slots */
	uint64_t limit = 0;                      /* ... and the bytes of the source that may be read */
};

extern "C" void fsm_hip_distinct_free(struct fsm_hip_distinct *dx) { run_free(dx); }

/* the passes on stream s into *dx, its device current; r: the packed text, the bytes and the flag (the rest is set here) */
static int distinct_passes(struct fsm_hip_distinct *dx, fsmhip::DstRun r, bool text, hipStream_t s)
{
	dx->src = r;
	if (r.R == 0) {                                  /* no record: doff[0] alone, and nothing is launched */
		if (text && (!HIP_OK(dx->d_doff.alloc(1)) || !HIP_OK(hipMemsetAsync(dx->d_doff.p, 0, sizeof(uint64_t), s)))) return -1;
		for (DevEvent &ev : dx->ev)
			if (!HIP_OK(hipEventRecord(ev, s))) return -1;
		return 0;
	}
	const uint64_t nblocks = fsmhip::dst_blocks(r.R);
	uint64_t tot[3] = {0, 0, 0};                     /* the firsts, the key bytes, the bytes that may be read */
	r.slots = dx->src.slots = fsmhip::dst_table_slots(r.R);
	if (!HIP_OK(dx->d_len.alloc(r.R)) || !HIP_OK(dx->d_hash.alloc(r.R)) || !HIP_OK(dx->d_class.alloc(r.R)) || !HIP_OK(dx->d_table.alloc(r.slots)) ||
	    !HIP_OK(dx->d_cnt.alloc(r.slots)) || !HIP_OK(dx->d_pairs.alloc(2u * nblocks + fsmhip::DST_PAIRS_EXTRA)))
		return -1;
	r.len = dx->d_len;
	r.hash = dx->d_hash;
	r.cls = dx->d_class;
	r.table = dx->d_table;
	r.cnt = dx->d_cnt;
	r.pairs = dx->d_pairs;
	if (!dx->begin(0, s)) return -1;
	if (!HIP_OK(hipMemsetAsync(r.pairs + 2u * nblocks, 0, fsmhip::DST_PAIRS_EXTRA * sizeof(uint64_t), s))) return -1;   /* the long records' count */
	if (fsmhip::dst_launch_hash(r, s) != 0) return -1;
	if (!dx->end(0, s) || !dx->begin(1, s)) return -1;
	if (!HIP_OK(hipMemsetAsync(r.table, 0xff, r.slots * sizeof(uint64_t), s)) || !HIP_OK(hipMemsetAsync(r.cnt, 0, r.slots * sizeof(uint64_t), s))) return -1;
	if (fsmhip::dst_launch_insert(r, s) != 0) return -1;
	if (!dx->end(1, s) || !dx->begin(2, s)) return -1;
	if (fsmhip::dst_launch_mark(r, s) != 0) return -1;
	if (pairs_scan_launch(r.pairs, nblocks, s) != 0) return -1;
	if (!dx->end(2, s)) return -1;
	/* the ONE wait: D sizes first and count, the bytes the text of the keys */
	if (!HIP_OK(hipMemcpyAsync(tot, r.pairs + 2u * nblocks, sizeof tot, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return -1;
	dx->D = (size_t)tot[0];
	dx->limit = tot[2];
	dx->nbytes = text ? tot[1] : 0u;
	r.D = tot[0];
	r.total = dx->nbytes;
	r.ngb = (r.total + fsmhip::EXT_BLOCK - 1u) / fsmhip::EXT_BLOCK;
	if (r.D != 0 && (!HIP_OK(dx->d_first.alloc(r.D)) || !HIP_OK(dx->d_count.alloc(r.D)))) return -1;
	if (text && (!HIP_OK(dx->d_doff.alloc(r.D + 1u)) || (r.D != 0 && !HIP_OK(dx->d_src.alloc(r.D))))) return -1;
	if (r.total != 0 && (!HIP_OK(dx->d_dbytes.alloc(r.ngb * fsmhip::EXT_BLOCK)) || !HIP_OK(dx->d_bfirst.alloc(r.ngb + 1u)))) return -1;
	r.first = dx->d_first;
	r.count = dx->d_count;
	r.doff = dx->d_doff;
	r.src = dx->d_src;
	r.bfirst = dx->d_bfirst;
	if (!dx->begin(3, s)) return -1;
	if (r.D == 0) {                                  /* (not with R >= 1; the arrays changed under the passes) */
		if (text && !HIP_OK(hipMemsetAsync(dx->d_doff.p, 0, sizeof(uint64_t), s))) return -1;
	} else if (fsmhip::dst_launch_number(r, s) != 0) {
		return -1;
	}
	if (!dx->end(3, s) || !dx->begin(4, s)) return -1;
	if (r.D != 0 && r.total != 0) {                  /* the extraction's write pass: record d is the key of first[d] */
		fsmhip::ExtRun w;
		w.base = r.bytes;
		w.limit = tot[2];
		w.sep = r.sep;
		w.out_off = r.doff;
		w.src = r.src;
		w.first = r.bfirst;
		w.out = dx->d_dbytes;
		w.nrec = r.D;
		w.total = r.total;
		w.ngb = r.ngb;
		const Grid g = grid_of(r.ngb, dx->device);
		w.wgs = g.wgs;
		w.per = g.per;
		if (fsmhip::ext_launch_write(w, s) != 0) return -1;
	}
	return dx->end(4, s) ? 0 : -1;
}

/* what every form refuses alike, behind ENODEV and the form's own NULLs */
static bool distinct_args(size_t R, int trim_byte, int sep_byte, unsigned flags)
{
	if (trim_byte < -1 || trim_byte > 255 || sep_byte < -1 || sep_byte > 255 || (flags & ~(FSM_HIP_DISTINCT_NO_TEXT | FSM_HIP_DISTINCT_WEAK_HASH)) != 0u) {
		errno = EINVAL;
		return false;
	}
	if ((uint64_t)R > fsmhip::DST_MAX_RECORDS) { errno = EOVERFLOW; return false; }
	return true;
}

/* the object over device arrays on stream s, `device` current, behind `after` (or nothing) */
static struct fsm_hip_distinct *distinct_new(int device, const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint32_t *d_tag, int sep_byte, unsigned flags, hipEvent_t after, hipStream_t s)
{
	fsmhip::DstRun r;
	r.off = d_off;
	r.bytes = static_cast<const unsigned char *>(d_bytes);
	r.tag = d_tag;
	r.R = R;
	r.nbytes = nbytes;
	r.trim = trim_byte;
	r.sep = sep_byte;
	r.weak = (flags & FSM_HIP_DISTINCT_WEAK_HASH) != 0u;
	return run_new<struct fsm_hip_distinct>(device, R, true, s, [&](struct fsm_hip_distinct *dx) {
		dx->sep = sep_byte;
		if (after != nullptr && !HIP_OK(hipStreamWaitEvent(s, after, 0))) return -1;
		return distinct_passes(dx, r, (flags & FSM_HIP_DISTINCT_NO_TEXT) == 0u, s);
	});
}

extern "C" struct fsm_hip_distinct *fsm_hip_distinct_device(const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint32_t *d_tag, int sep_byte, unsigned flags, void *hip_stream)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (d_off == nullptr || (d_bytes == nullptr && nbytes != 0)) { errno = EINVAL; return nullptr; }
	if (!distinct_args(R, trim_byte, sep_byte, flags)) return nullptr;
	return distinct_new(dev, d_off, d_bytes, R, nbytes, trim_byte, d_tag, sep_byte, flags, nullptr, static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_distinct *fsm_hip_distinct(const uint64_t *off, const void *bytes, size_t R, int trim_byte, const uint32_t *tag, int sep_byte,
	unsigned flags)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (off == nullptr) { errno = EINVAL; return nullptr; }
	if (!distinct_args(R, trim_byte, sep_byte, flags)) return nullptr;
	for (size_t r = 0; r < R; r++)
		if (off[r] > off[r + 1u]) { errno = EINVAL; return nullptr; }
	const uint64_t nbytes = R != 0 ? off[R] : 0u;
	if (bytes == nullptr && nbytes != 0) { errno = EINVAL; return nullptr; }
	DevStream own;
	if (!HIP_OK(own.create(hipStreamNonBlocking))) return nullptr;
	const hipStream_t s = own;
	fsmhip::DstRun r;
	r.R = R;
	r.nbytes = nbytes;
	r.trim = trim_byte;
	r.sep = sep_byte;
	r.weak = (flags & FSM_HIP_DISTINCT_WEAK_HASH) != 0u;
	struct fsm_hip_distinct *dx = run_new<struct fsm_hip_distinct>(dev, R, true, s, [&](struct fsm_hip_distinct *o) {
		o->sep = sep_byte;
		if (!HIP_OK(o->own_off.alloc(R + 1u)) || !HIP_OK(hipMemcpyAsync(o->own_off.p, off, (R + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, s))) return -1;
		if (nbytes != 0 && (!HIP_OK(o->own_bytes.alloc(nbytes)) || !HIP_OK(hipMemcpyAsync(o->own_bytes.p, bytes, nbytes, hipMemcpyHostToDevice, s)))) return -1;
		if (tag != nullptr && R != 0 &&
		    (!HIP_OK(o->own_tag.alloc(R)) || !HIP_OK(hipMemcpyAsync(o->own_tag.p, tag, R * sizeof(uint32_t), hipMemcpyHostToDevice, s))))
			return -1;
		r.off = o->own_off;
		r.bytes = o->own_bytes;
		r.tag = o->own_tag;
		return distinct_passes(o, r, (flags & FSM_HIP_DISTINCT_NO_TEXT) == 0u, s);
	});
	if (dx == nullptr || HIP_OK(hipStreamSynchronize(s))) return dx;   /* (null: run_new left the stream idle) the stream goes at return */
	const int e = errno;
	run_free(dx);
	errno = e;
	return nullptr;
}

extern "C" struct fsm_hip_distinct *fsm_hip_extracted_distinct(const struct fsm_hip_extracted *x, int sep_byte, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (x == nullptr) { errno = EINVAL; return nullptr; }
	if (!distinct_args(x->nrec, x->sep, sep_byte, flags)) return nullptr;
	DevGuard dg(x->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return distinct_new(x->device, x->d_off, x->d_bytes, x->nrec, x->nbytes, x->sep, nullptr, sep_byte, flags, x->done(), static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_distinct *fsm_hip_text_hits_distinct(const struct fsm_hip_text_hits *h, int sep_byte, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (h == nullptr || h->d_off.p == nullptr) { errno = EINVAL; return nullptr; }   /* (no offsets: FSM_HIP_HITS_NO_BYTES) */
	if (!distinct_args(h->m, h->delim, sep_byte, flags)) return nullptr;
	DevGuard dg(h->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return distinct_new(h->device, h->d_off, h->d_bytes, h->m, h->nbytes, h->delim, nullptr, sep_byte, flags, h->ev[5], static_cast<hipStream_t>(hip_stream));
}

/* the D keys in byte order (sort.hip), or by count[D] descending first: the keys are the object's own packed text */
extern "C" struct fsm_hip_sorted *fsm_hip_keys_sort(const struct fsm_hip_distinct *dx, int sep_byte, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (dx == nullptr || dx->d_doff.p == nullptr) { errno = EINVAL; return nullptr; }   /* (no keys: FSM_HIP_DISTINCT_NO_TEXT) */
	const bool by_count = (flags & FSM_HIP_SORT_BY_COUNT) != 0u;
	if (!fsmhip::sort_args(dx->D, dx->sep, sep_byte, flags, FSM_HIP_SORT_NO_TEXT | FSM_HIP_SORT_REVERSE | FSM_HIP_SORT_MAJOR_DESC | FSM_HIP_SORT_BY_COUNT, by_count))
		return nullptr;
	if (by_count) flags = (flags & ~FSM_HIP_SORT_BY_COUNT) | FSM_HIP_SORT_MAJOR_DESC;
	DevGuard dg(dx->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return fsmhip::sorted_new(dx->device, dx->d_doff, dx->d_dbytes, dx->D, dx->nbytes, dx->sep, by_count ? dx->d_count.p : nullptr, sep_byte, flags, dx->done(),
	                          static_cast<hipStream_t>(hip_stream));
}

extern "C" size_t fsm_hip_distinct_count(const struct fsm_hip_distinct *dx) { return dx == nullptr ? 0 : dx->D; }
extern "C" size_t fsm_hip_distinct_records(const struct fsm_hip_distinct *dx) { return dx == nullptr ? 0 : dx->m; }
extern "C" uint64_t fsm_hip_distinct_nbytes(const struct fsm_hip_distinct *dx) { return dx == nullptr ? 0 : dx->nbytes; }
extern "C" const uint64_t *fsm_hip_distinct_first_device(const struct fsm_hip_distinct *dx) { return dx == nullptr ? nullptr : dx->d_first.p; }
extern "C" const uint64_t *fsm_hip_distinct_count_device(const struct fsm_hip_distinct *dx) { return dx == nullptr ? nullptr : dx->d_count.p; }
extern "C" const uint32_t *fsm_hip_distinct_class_device(const struct fsm_hip_distinct *dx) { return dx == nullptr ? nullptr : dx->d_class.p; }
extern "C" const uint64_t *fsm_hip_distinct_off_device(const struct fsm_hip_distinct *dx) { return dx == nullptr ? nullptr : dx->d_doff.p; }
extern "C" const unsigned char *fsm_hip_distinct_bytes_device(const struct fsm_hip_distinct *dx) { return dx == nullptr ? nullptr : dx->d_dbytes.p; }

extern "C" int fsm_hip_distinct_copy(const struct fsm_hip_distinct *dx, uint64_t *first, uint64_t *count, uint32_t *cls, uint64_t *doff, void *dbytes)
{
	if (dx == nullptr || (doff != nullptr && dx->d_doff.p == nullptr)) { errno = EINVAL; return -1; }
	return copy_out(dx->device, dx->done(), {{first, dx->d_first, dx->D * sizeof(uint64_t)}, {count, dx->d_count, dx->D * sizeof(uint64_t)},
	                                         {cls, dx->d_class, dx->m * sizeof(uint32_t)}, {doff, dx->d_doff, (dx->D + 1u) * sizeof(uint64_t)},
	                                         {dbytes, dx->d_dbytes, (size_t)dx->nbytes}});
}

extern "C" double fsm_hip_distinct_ms(const struct fsm_hip_distinct *dx) { return run_ms(dx, 0, 4); }

extern "C" double fsm_hip_distinct_pass_ms(const struct fsm_hip_distinct *dx, int pass)
{
	if (pass < 0 || pass > 3) { errno = EINVAL; return -1.0; }
	return pass < 2 ? run_ms(dx, pass, pass) : pass == 2 ? run_ms(dx, 2, 3) : run_ms(dx, 4, 4);
}


/* ---- the lookup's fronts: the found object of four event pairs -- hash, probe, mark + scan, pick.  Every array is sized by R, so no
 * count has to reach the host: nothing waits, and everything may be in flight at return. ---------------------------------------- */
struct __attribute__((visibility("hidden"))) fsm_hip_found : RunObject<4> {
	bool has_pick = false;                   /* (m is R) */
	DevBuf<uint64_t> d_len, d_hash;          /* R each: internal */
	DevBuf<uint32_t> d_list;                 /* R: the long records, where there is no pick to lend its memory: internal */
	DevBuf<uint64_t> d_pairs;                /* per block of records, + DST_PAIRS_EXTRA: internal; P behind the block pairs */
	DevBuf<uint32_t> d_class;                /* R */
	DevBuf<uint64_t> d_bitmap;               /* ceil(R / 64) */
	DevBuf<uint64_t> d_pick;                 /* R; NULL under NO_PICK */
	DevBuf<uint64_t> own_off;                /* the host form's staged input */
	DevBuf<unsigned char> own_bytes;
	DevBuf<uint32_t> own_tag;
};

extern "C" void fsm_hip_found_free(struct fsm_hip_found *fx) { run_free(fx); }

/* the passes on stream s into *fx, its device current, behind the dictionary's last event; p: the probe text and its trim */
static int found_passes(struct fsm_hip_found *fx, const struct fsm_hip_distinct *keys, fsmhip::DstRun p, hipStream_t s)
{
	if (!HIP_OK(hipStreamWaitEvent(s, keys->done(), 0))) return -1;
	if (p.R == 0) {                                  /* no record: no array, and nothing is launched */
		for (DevEvent &ev : fx->ev)
			if (!HIP_OK(hipEventRecord(ev, s))) return -1;
		return 0;
	}
	const uint64_t nblocks = fsmhip::dst_blocks(p.R);
	const bool table = keys->D != 0;                 /* no key: no table is read, every record is absent */
	if (!HIP_OK(fx->d_class.alloc(p.R)) || !HIP_OK(fx->d_bitmap.alloc(fsmhip::fnd_bitmap_words(p.R))) ||
	    !HIP_OK(fx->d_pairs.alloc(2u * nblocks + fsmhip::DST_PAIRS_EXTRA)) || (fx->has_pick && !HIP_OK(fx->d_pick.alloc(p.R))))
		return -1;
	if (table && (!HIP_OK(fx->d_len.alloc(p.R)) || !HIP_OK(fx->d_hash.alloc(p.R)) || (!fx->has_pick && !HIP_OK(fx->d_list.alloc(p.R))))) return -1;
	fsmhip::FndRun f;
	p.sep = -1;
	p.weak = keys->src.weak;                         /* the weak hash depends on the slots: both are the dictionary's */
	p.slots = keys->src.slots;
	p.len = fx->d_len;
	p.hash = fx->d_hash;
	p.cls = fx->has_pick ? reinterpret_cast<uint32_t *>(fx->d_pick.p) : fx->d_list.p;   /* pick is written last, behind fnd_probe_long */
	p.pairs = fx->d_pairs;
	f.p = p;
	f.k_off = keys->src.off;
	f.k_bytes = keys->src.bytes;
	f.k_tag = keys->src.tag;
	f.k_len = keys->d_len;
	f.table = keys->d_table;
	f.cnt = keys->d_cnt;
	f.k_R = keys->m;
	f.k_limit = keys->limit;
	f.D = keys->D;
	f.out = fx->d_class;
	f.bitmap = fx->d_bitmap;
	f.pick = fx->d_pick;
	if (!fx->begin(0, s)) return -1;
	if (!HIP_OK(hipMemsetAsync(p.pairs + 2u * nblocks, 0, fsmhip::DST_PAIRS_EXTRA * sizeof(uint64_t), s))) return -1;   /* the long records' count */
	if (table && fsmhip::dst_launch_hash(p, s) != 0) return -1;
	if (!fx->end(0, s) || !fx->begin(1, s)) return -1;
	if (table) {
		if (fsmhip::fnd_launch_probe(f, s) != 0) return -1;
	} else if (!HIP_OK(hipMemsetAsync(f.out, 0xff, p.R * sizeof(uint32_t), s))) {
		return -1;
	}
	if (!fx->end(1, s) || !fx->begin(2, s)) return -1;
	if (fsmhip::fnd_launch_mark(f, s) != 0) return -1;
	if (pairs_scan_launch(p.pairs, nblocks, s) != 0) return -1;
	if (!fx->end(2, s) || !fx->begin(3, s)) return -1;
	if (fx->has_pick && fsmhip::fnd_launch_pick(f, s) != 0) return -1;
	return fx->end(3, s) ? 0 : -1;
}

/* what every form refuses alike, behind ENODEV and the form's own NULLs */
static bool found_args(size_t R, int trim_byte, unsigned flags)
{
	if (trim_byte < -1 || trim_byte > 255 || (flags & ~FSM_HIP_FIND_NO_PICK) != 0u) { errno = EINVAL; return false; }
	if ((uint64_t)R > fsmhip::DST_MAX_RECORDS) { errno = EOVERFLOW; return false; }
	return true;
}

/* the object over device arrays on stream s, the dictionary's device current, behind `after` (or nothing) and the dictionary */
static struct fsm_hip_found *found_new(const struct fsm_hip_distinct *keys, const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint32_t *d_tag, unsigned flags, hipEvent_t after, hipStream_t s)
{
	fsmhip::DstRun p;
	p.off = d_off;
	p.bytes = static_cast<const unsigned char *>(d_bytes);
	p.tag = d_tag;
	p.R = R;
	p.nbytes = nbytes;
	p.trim = trim_byte;
	return run_new<struct fsm_hip_found>(keys->device, R, true, s, [&](struct fsm_hip_found *fx) {
		fx->has_pick = (flags & FSM_HIP_FIND_NO_PICK) == 0u;
		if (after != nullptr && !HIP_OK(hipStreamWaitEvent(s, after, 0))) return -1;
		return found_passes(fx, keys, p, s);
	});
}

extern "C" struct fsm_hip_found *fsm_hip_keys_find_device(const struct fsm_hip_distinct *keys, const uint64_t *d_off, const void *d_bytes, size_t R,
	uint64_t nbytes, int trim_byte, const uint32_t *d_tag, unsigned flags, void *hip_stream)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (keys == nullptr || d_off == nullptr || (d_bytes == nullptr && nbytes != 0) || keys->device != dev) { errno = EINVAL; return nullptr; }
	if (!found_args(R, trim_byte, flags)) return nullptr;
	return found_new(keys, d_off, d_bytes, R, nbytes, trim_byte, d_tag, flags, nullptr, static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_found *fsm_hip_keys_find(const struct fsm_hip_distinct *keys, const uint64_t *off, const void *bytes, size_t R, int trim_byte,
	const uint32_t *tag, unsigned flags)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (keys == nullptr || off == nullptr) { errno = EINVAL; return nullptr; }
	if (!found_args(R, trim_byte, flags)) return nullptr;
	for (size_t r = 0; r < R; r++)
		if (off[r] > off[r + 1u]) { errno = EINVAL; return nullptr; }
	const uint64_t nbytes = R != 0 ? off[R] : 0u;
	if (bytes == nullptr && nbytes != 0) { errno = EINVAL; return nullptr; }
	DevGuard dg(keys->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	DevStream own;
	if (!HIP_OK(own.create(hipStreamNonBlocking))) return nullptr;
	const hipStream_t s = own;
	fsmhip::DstRun p;
	p.R = R;
	p.nbytes = nbytes;
	p.trim = trim_byte;
	struct fsm_hip_found *fx = run_new<struct fsm_hip_found>(keys->device, R, true, s, [&](struct fsm_hip_found *o) {
		o->has_pick = (flags & FSM_HIP_FIND_NO_PICK) == 0u;
		if (!HIP_OK(o->own_off.alloc(R + 1u)) || !HIP_OK(hipMemcpyAsync(o->own_off.p, off, (R + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, s))) return -1;
		if (nbytes != 0 && (!HIP_OK(o->own_bytes.alloc(nbytes)) || !HIP_OK(hipMemcpyAsync(o->own_bytes.p, bytes, nbytes, hipMemcpyHostToDevice, s)))) return -1;
		if (tag != nullptr && R != 0 &&
		    (!HIP_OK(o->own_tag.alloc(R)) || !HIP_OK(hipMemcpyAsync(o->own_tag.p, tag, R * sizeof(uint32_t), hipMemcpyHostToDevice, s))))
			return -1;
		p.off = o->own_off;
		p.bytes = o->own_bytes;
		p.tag = o->own_tag;
		return found_passes(o, keys, p, s);
	});
	if (fx == nullptr || HIP_OK(hipStreamSynchronize(s))) return fx;   /* (null: run_new left the stream idle) the stream goes at return */
	const int e = errno;
	run_free(fx);
	errno = e;
	return nullptr;
}

extern "C" struct fsm_hip_found *fsm_hip_keys_find_extracted(const struct fsm_hip_distinct *keys, const struct fsm_hip_extracted *x, unsigned flags,
	void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (keys == nullptr || x == nullptr || x->device != keys->device) { errno = EINVAL; return nullptr; }
	if (!found_args(x->nrec, x->sep, flags)) return nullptr;
	DevGuard dg(keys->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return found_new(keys, x->d_off, x->d_bytes, x->nrec, x->nbytes, x->sep, nullptr, flags, x->done(), static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_found *fsm_hip_keys_find_hits(const struct fsm_hip_distinct *keys, const struct fsm_hip_text_hits *h, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (keys == nullptr || h == nullptr || h->d_off.p == nullptr || h->device != keys->device) { errno = EINVAL; return nullptr; }   /* (no offsets: NO_BYTES) */
	if (!found_args(h->m, h->delim, flags)) return nullptr;
	DevGuard dg(keys->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return found_new(keys, h->d_off, h->d_bytes, h->m, h->nbytes, h->delim, nullptr, flags, h->ev[5], static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_found *fsm_hip_keys_find_text(const struct fsm_hip_distinct *keys, const struct fsm_hip_text *t, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (keys == nullptr || t == nullptr || t->device != keys->device) { errno = EINVAL; return nullptr; }
	if (!found_args(t->n, t->delim, flags)) return nullptr;
	DevGuard dg(keys->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return found_new(keys, t->d_off, t->d_text, t->n, t->nbytes, t->delim, nullptr, flags, t->ev[3], static_cast<hipStream_t>(hip_stream));
}

extern "C" size_t fsm_hip_found_records(const struct fsm_hip_found *fx) { return fx == nullptr ? 0 : fx->m; }

/* P; it waits for the object's last event */
extern "C" size_t fsm_hip_found_present(const struct fsm_hip_found *fx)
{
	uint64_t present = 0;
	if (fx == nullptr || fx->m == 0) return 0;
	if (copy_out(fx->device, fx->done(), {{&present, fx->d_pairs.p + 2u * fsmhip::dst_blocks(fx->m), sizeof present}}) != 0) return 0;
	return (size_t)present;
}

extern "C" const uint32_t *fsm_hip_found_class_device(const struct fsm_hip_found *fx) { return fx == nullptr ? nullptr : fx->d_class.p; }
extern "C" const uint64_t *fsm_hip_found_bitmap_device(const struct fsm_hip_found *fx) { return fx == nullptr ? nullptr : fx->d_bitmap.p; }
extern "C" const uint64_t *fsm_hip_found_pick_device(const struct fsm_hip_found *fx) { return fx == nullptr ? nullptr : fx->d_pick.p; }

extern "C" int fsm_hip_found_copy(const struct fsm_hip_found *fx, uint32_t *cls, uint64_t *bitmap, uint64_t *pick)
{
	if (fx == nullptr || (pick != nullptr && !fx->has_pick && fx->m != 0)) { errno = EINVAL; return -1; }   /* (no record: no array either way) */
	return copy_out(fx->device, fx->done(), {{cls, fx->d_class, fx->m * sizeof(uint32_t)}, {bitmap, fx->d_bitmap, (size_t)fsmhip::fnd_bitmap_words(fx->m) * sizeof(uint64_t)},
	                                         {pick, fx->d_pick, fx->m * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_found_ms(const struct fsm_hip_found *fx) { return run_ms(fx, 0, 3); }

extern "C" double fsm_hip_found_pass_ms(const struct fsm_hip_found *fx, int pass)
{
	if (pass < 0 || pass > 3) { errno = EINVAL; return -1.0; }
	return run_ms(fx, pass, pass);
}
