/*
 * sort.hip -- the records of a packed text in byte order, on the device: order, ranks and the sorted text.  include/fsm_hip.h,
 * section "sort", is the definition; sort_seg.h holds the arithmetic (the word and its valid bytes, the REVERSE complement, the
 * chunked common prefix, the digits, the head and active predicates, the rounds bound), shared with tests/c/test_sort_seg.cpp.
 *
 * Most-significant-word-first rounds over a stable least-significant-digit radix sort; the bookkeeping is positional.
 *   order[p]   the record at position p; starts as p, and every pass is stable, so equal records keep ascending r
 *   bucket[p]  the first position of the run of records equal on everything examined so far; buckets are contiguous
 *   dep[p]     the key bytes examined so far; one value for all of a bucket, kept per position so that no lane writes what
 *              another reads
 *   skip[h]    per bucket head: the minimum of the prefix skip, taken by atomics
 *   apos[i]    the positions of the ACTIVE buckets (more than one member, the last word full), ascending: the round's entries
 * A round (entries: the A active positions, a lane each, blocks of SRT_THREADS):
 *     srt_prefix     the entry's key against its bucket head's from dep on, in 16-byte chunks; the common bytes by an agent-scope
 *                    atomic min into skip[head] (one per wavefront where the wavefront is in one bucket)
 *     srt_fetch      dep += skip rounded down to 8; the next eight key bytes big endian, zero-padded, and how many exist; under
 *                    REVERSE both complemented.  The entry: (bucket, word, valid, record); perm[i] = i.  srt_major: the same from
 *                    major[r] for the round before the first, complemented under MAJOR_DESC
 *     srt_digits     all digit histograms at once, in LDS, then one atomic add per non-zero bin
 *     per digit      srt_tile_hist, srt_hist_scan (one workgroup), srt_scatter: a stable pass over perm, a tile SRT_TILE entries.  A
 *                    digit with one occupied bin is skipped by all three: the scan says so in par[digit + 1], which buffer of perm
 *                    is current.  Rank inside a tile: the wave64 match-by-ballot rank, per-wavefront counts in LDS, a prefix
 *                    across the wavefronts.  The bucket's digits above the bytes of R - 1 are not launched
 *     srt_mark       sorted entry i goes to active position i: order; head(i) = (bucket, word, valid) differs from i - 1's;
 *                    active(i); per block (active entries, last head position + 1)
 *     srt_blocks     the exclusive scan of the block pairs, a sum and a maximum, by one workgroup; the active entries for the host
 *     srt_assign     the block's scans redone: bucket = the last head at or before i, the active positions compacted
 *   then the round's ONE wait: 8 bytes, the active entries (the first wait also reads the text's bytes and the read limit).
 * Finish: srt_ranks (head(p) = bucket[p] == p; per block (heads, text bytes)), text.hip's scan of the block pairs, srt_finish
 * (rank, order widened, soff, src, the output-block index), and the extraction's write pass (extract.hip, ext_write).
 * Coherence: skip[] and the digit histograms are touched by several workgroups in one kernel, by agent-scope atomics alone -- the
 * XCDs do not share an L2.  Everything else a kernel reads was written by an EARLIER kernel or is the caller's read-only input.
 * Every global access names its address space (no FLAT instruction); no byte outside [bytes, bytes + min(off[R], nbytes)) is read;
 * every index read from an array is clamped to the array it is used on; every store goes below the sizes the host counted.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <utility>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "match_marks.h"
#include "extract.h"
#include "distinct_seg.h"
#include "sort_seg.h"
#include "sort.h"
#include "text_objects.h"

namespace fsmhip {

constexpr uint32_t SRT_THREADS = 256;
constexpr uint32_t SRT_WAVES = SRT_THREADS / 64u;
constexpr uint32_t SRT_ITEMS = 8;                           /* entries of a lane in a radix pass */
constexpr uint32_t SRT_TILE = SRT_THREADS * SRT_ITEMS;      /* entries a workgroup ranks in a radix pass */
constexpr uint32_t SRT_SCAN_THREADS = 1024;
constexpr uint32_t SRT_SCAN_PER = 4;
constexpr uint32_t SRT_PAR = 16;                            /* behind the digit histograms: which buffer of perm is current */
constexpr uint32_t SRT_META = 8;                            /* active entries, text bytes, read limit, -, passes run, passes skipped */

constexpr uint64_t srt_blocks(uint64_t n) { return (n + SRT_THREADS - 1u) / SRT_THREADS; }
constexpr uint64_t srt_tiles(uint64_t n) { return (n + SRT_TILE - 1u) / SRT_TILE; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself. */
struct SrtRun {
	/* the packed text */
	const uint64_t *off = nullptr;           /* R + 1 */
	const unsigned char *bytes = nullptr;
	const uint64_t *major = nullptr;         /* R, or null */
	uint64_t R = 0, nbytes = 0;
	int trim = -1, sep = -1;
	bool reverse = false, major_desc = false, text = false;
	/* per record */
	uint64_t *kbeg = nullptr, *klen = nullptr;
	/* per position */
	uint32_t *order = nullptr, *bucket = nullptr;
	uint64_t *dep = nullptr, *skip = nullptr;
	/* per entry of a round */
	uint32_t *apos = nullptr, *napos = nullptr;
	uint64_t *eword = nullptr;
	uint32_t *ebkt = nullptr, *eval = nullptr, *eord = nullptr, *eflag = nullptr;
	uint32_t *perm0 = nullptr, *perm1 = nullptr;
	uint32_t *thist = nullptr;               /* SRT_BINS * tiles: bin-major */
	uint32_t *ghist = nullptr;               /* SRT_DIGITS * SRT_BINS, then par[SRT_PAR] */
	uint64_t *blk = nullptr;                 /* per block of entries: (active, last head + 1), then those before it */
	uint64_t *meta = nullptr;                /* SRT_META */
	uint64_t A = 0;                          /* the round's entries */
	uint32_t ntiles = 0, digit = 0, ndigits = 0;
	bool major_round = false;
	/* the finish */
	uint64_t *pairs = nullptr;               /* per block of positions (heads, text bytes), then (scanned) those before it; + 2 */
	uint64_t *order64 = nullptr;             /* R */
	uint32_t *rank = nullptr;                /* R */
	uint64_t *soff = nullptr;                /* R + 1, or null (NO_TEXT) */
	uint64_t *src = nullptr;                 /* R: where each key's bytes begin in `bytes`; with soff */
	uint64_t *bfirst = nullptr;              /* ngb + 1 */
	uint64_t total = 0, ngb = 0;
};

}

using namespace fsmhip;

namespace {

typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
typedef u32x4s __attribute__((aligned(1))) u32x4s_any;
typedef uint64_t u64x2s __attribute__((ext_vector_type(2)));
typedef const u32x4s_any __attribute__((address_space(1))) *g_chunkp;
typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
typedef uint32_t __attribute__((address_space(1))) *g_u32w;
typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
typedef uint64_t __attribute__((address_space(1))) *g_u64w;
typedef u64x2s __attribute__((address_space(1))) *g_u64x2w;
typedef const u64x2s __attribute__((address_space(1))) *g_u64x2p;

#define G32(p) ((g_u32p)(uintptr_t)(p))
#define W32(p) ((g_u32w)(uintptr_t)(p))
#define G64(p) ((g_u64p)(uintptr_t)(p))
#define W64(p) ((g_u64w)(uintptr_t)(p))

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t min32(uint32_t a, uint32_t b) { return a < b ? a : b; }

/* the bytes that may be read: off[R] and nbytes, whichever is less */
__device__ __forceinline__ uint64_t read_limit(const SrtRun &a) { return min64(G64(a.off)[a.R], a.nbytes); }

/* the n (0 .. 16) bytes at byte `at`, as two little-endian words, those behind the n as 0: one load where sixteen bytes may be
 * read, byte loads at the end of the text (the distinct records' load) */
__device__ __forceinline__ void load_chunk(uint64_t bx, uint64_t at, uint32_t n, uint64_t limit, uint64_t *lo, uint64_t *hi)
{
	uint64_t x0 = 0, x1 = 0;
	if (n == 0u) {
	} else if (limit >= 16u && at <= limit - 16u) {
		const u32x4s v = *(g_chunkp)(bx + at);
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

/* the wavefront's inclusive sum / maximum */
__device__ __forceinline__ uint64_t wave_incl_sum(uint64_t x, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t y = __shfl_up(x, d, 64);
		if (lane >= (uint32_t)d) x += y;
	}
	return x;
}

__device__ __forceinline__ uint64_t wave_incl_max(uint64_t x, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t y = __shfl_up(x, d, 64);
		if (lane >= (uint32_t)d && y > x) x = y;
	}
	return x;
}

/* the round's digit d has one occupied bin: nothing to sort by (all threads of the workgroup call it) */
__device__ __forceinline__ bool digit_is_flat(const SrtRun &a)
{
	bool one = false;
	if (threadIdx.x < SRT_BINS) one = G32(a.ghist)[a.digit * SRT_BINS + threadIdx.x] == (uint32_t)a.A;
	return __syncthreads_or(one ? 1 : 0) != 0;
}

__device__ __forceinline__ uint32_t entry_digit(const SrtRun &a, uint32_t e)
{
	const uint32_t d = a.digit;                      /* (uniform) one array per kind of digit */
	if (d == 0u) return G32(a.eval)[e] & 0xffu;
	if (d < SRT_DIGIT_BUCKET) return srt_digit(G64(a.eword)[e], 0u, 0u, d);
	return srt_digit(0u, 0u, G32(a.ebkt)[e], d);
}

/* the start (grid: srt_blocks(R)): the keys, position p holds record p in the one bucket [0, R) */
__global__ void __launch_bounds__(SRT_THREADS)
srt_init(const SrtRun a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t r = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
	uint64_t out = 0;
	if (r < a.R) {
		uint64_t beg, raw;
		marks_clip(G64(a.off)[r], G64(a.off)[r + 1u], limit, &beg, &raw);
		const uint32_t last = raw != 0u ? ((g_u8p)bx)[beg + raw - 1u] : 0u;
		const uint64_t len = dst_trimmed(raw, last, a.trim);
		W64(a.kbeg)[r] = beg;
		W64(a.klen)[r] = len;
		W32(a.order)[r] = (uint32_t)r;
		W32(a.bucket)[r] = 0u;
		W32(a.apos)[r] = (uint32_t)r;
		W64(a.dep)[r] = 0u;
		W64(a.skip)[r] = ~(uint64_t)0;
		out = a.text ? len + (a.sep >= 0 ? 1u : 0u) : 0u;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) out += __shfl_xor(out, d, 64);
	if (lane == 0u && out != 0u) (void)__hip_atomic_fetch_add(W64(a.meta) + 1, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (r == 0u) W64(a.meta)[2] = limit;             /* rides along to the host */
}

/* the round before the first (grid: srt_blocks(A), A == R): the entries from the major key */
__global__ void __launch_bounds__(SRT_THREADS)
srt_major(const SrtRun a)
{
	const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	if (i >= a.A) return;
	const uint32_t p = min32(G32(a.apos)[i], (uint32_t)(a.R - 1u));
	const uint32_t r = min32(G32(a.order)[p], (uint32_t)(a.R - 1u));
	const uint64_t m = G64(a.major)[r];
	W64(a.eword)[i] = a.major_desc ? ~m : m;
	W32(a.eval)[i] = SRT_WORD;
	W32(a.ebkt)[i] = G32(a.bucket)[p];
	W32(a.eord)[i] = r;
	W32(a.perm0)[i] = (uint32_t)i;
}

/* pass 0a (grid: srt_blocks(A)): the bytes every member of a bucket shares with its head from dep on */
__global__ void __launch_bounds__(SRT_THREADS)
srt_prefix(const SrtRun a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
	const bool valid = i < a.A;
	uint64_t common = ~(uint64_t)0;
	uint32_t B = 0;
	if (valid) {
		const uint32_t p = min32(G32(a.apos)[i], (uint32_t)(a.R - 1u));
		B = min32(G32(a.bucket)[p], (uint32_t)(a.R - 1u));
		const uint32_t r = min32(G32(a.order)[p], (uint32_t)(a.R - 1u)), h = min32(G32(a.order)[B], (uint32_t)(a.R - 1u));
		const uint64_t d = G64(a.dep)[p];
		const uint64_t lr = G64(a.klen)[r], lh = G64(a.klen)[h];
		const uint64_t m = min64(lr > d ? lr - d : 0u, lh > d ? lh - d : 0u);
		common = m;
		if (r != h) {
			const uint64_t ka = G64(a.kbeg)[r] + d, kb = G64(a.kbeg)[h] + d;
			uint64_t c = 0;
#pragma unroll 1
			while (c < m) {
				const uint32_t n = m - c < SRT_CHUNK ? (uint32_t)(m - c) : SRT_CHUNK;
				uint64_t alo, ahi, blo, bhi;
				load_chunk(bx, ka + c, n, limit, &alo, &ahi);
				load_chunk(bx, kb + c, n, limit, &blo, &bhi);
				const uint32_t s = srt_common_chunk(alo, ahi, blo, bhi, n);
				c += s;
				if (s < n) break;
			}
			common = c;
		}
	}
	/* a wavefront inside one bucket -- the common case while buckets are large -- takes one atomic */
	const uint64_t vm = __ballot(valid);
	if (vm == 0u) return;
	const uint32_t B0 = (uint32_t)__shfl((int)B, (int)__builtin_ctzll(vm), 64);
	if (__ballot(valid && B == B0) == vm) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) common = min64(common, __shfl_xor(common, d, 64));
		if (lane == 0u) (void)__hip_atomic_fetch_min(W64(a.skip) + B0, common, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	} else if (valid) {
		(void)__hip_atomic_fetch_min(W64(a.skip) + B, common, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

/* pass 0b (grid: srt_blocks(A)): the round's entries */
__global__ void __launch_bounds__(SRT_THREADS)
srt_fetch(const SrtRun a)
{
	const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	if (i >= a.A) return;
	const uint64_t limit = read_limit(a), bx = (uint64_t)(uintptr_t)a.bytes;
	const uint32_t p = min32(G32(a.apos)[i], (uint32_t)(a.R - 1u));
	const uint32_t B = min32(G32(a.bucket)[p], (uint32_t)(a.R - 1u));
	const uint32_t r = min32(G32(a.order)[p], (uint32_t)(a.R - 1u));
	const uint64_t len = G64(a.klen)[r];
	uint64_t d = min64(G64(a.dep)[p], len);
	d += srt_skip(min64(G64(a.skip)[B], len - d));
	const uint32_t valid = srt_valid(len, d);
	uint64_t lo, hi;
	load_chunk(bx, G64(a.kbeg)[r] + d, valid, limit, &lo, &hi);
	W64(a.eword)[i] = srt_sort_word(srt_word(lo, valid), a.reverse);
	W32(a.eval)[i] = srt_sort_valid(valid, a.reverse);
	W32(a.ebkt)[i] = B;
	W32(a.eord)[i] = r;
	W32(a.perm0)[i] = (uint32_t)i;
	W64(a.dep)[p] = d + SRT_WORD;
}

/* pass 1a (grid: ntiles): every digit's histogram over the round's entries */
__global__ void __launch_bounds__(SRT_THREADS)
srt_digits(const SrtRun a)
{
	__shared__ uint32_t hist[SRT_DIGITS * SRT_BINS];
	for (uint32_t k = threadIdx.x; k < SRT_DIGITS * SRT_BINS; k += SRT_THREADS) hist[k] = 0u;
	__syncthreads();
	const uint64_t base = (uint64_t)blockIdx.x * SRT_TILE;
#pragma unroll 1
	for (uint32_t s = 0; s < SRT_ITEMS; s++) {
		const uint64_t i = base + (uint64_t)s * SRT_THREADS + threadIdx.x;
		if (i >= a.A) break;
		const uint64_t w = G64(a.eword)[i];
		const uint32_t v = G32(a.eval)[i], b = G32(a.ebkt)[i];
#pragma unroll
		for (uint32_t d = 0; d < SRT_DIGITS; d++)
			if (d < a.ndigits) atomicAdd(&hist[d * SRT_BINS + srt_digit(w, v, b, d)], 1u);
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < a.ndigits * SRT_BINS; k += SRT_THREADS)
		if (hist[k] != 0u) (void)__hip_atomic_fetch_add(W32(a.ghist) + k, hist[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* pass 1b (grid: ntiles): the tile's histogram of the digit, bin-major */
__global__ void __launch_bounds__(SRT_THREADS)
srt_tile_hist(const SrtRun a)
{
	__shared__ uint32_t hist[SRT_BINS];
	if (digit_is_flat(a)) return;
	const g_u32p src = G32(a.ghist)[SRT_DIGITS * SRT_BINS + a.digit] != 0u ? G32(a.perm1) : G32(a.perm0);
	hist[threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t base = (uint64_t)blockIdx.x * SRT_TILE;
#pragma unroll 1
	for (uint32_t s = 0; s < SRT_ITEMS; s++) {
		const uint64_t i = base + (uint64_t)s * SRT_THREADS + threadIdx.x;
		if (i >= a.A) break;
		atomicAdd(&hist[entry_digit(a, min32(src[i], (uint32_t)(a.A - 1u)))], 1u);
	}
	__syncthreads();
	W32(a.thist)[(uint64_t)threadIdx.x * a.ntiles + blockIdx.x] = hist[threadIdx.x];
}

/* pass 1c (one workgroup): flat or not, for the two kernels around it and the passes behind it; the exclusive scan of the tile
 * histograms, bin-major, which is where each tile's entries of each bin begin */
__global__ void __launch_bounds__(SRT_SCAN_THREADS)
srt_hist_scan(const SrtRun a)
{
	__shared__ uint32_t wtot[SRT_SCAN_THREADS / 64u];
	__shared__ uint32_t carry;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const bool flat = digit_is_flat(a);
	if (threadIdx.x == 0u) {
		const g_u32w par = W32(a.ghist) + SRT_DIGITS * SRT_BINS;
		par[a.digit + 1u] = par[a.digit] ^ (flat ? 0u : 1u);
		W64(a.meta)[flat ? 5 : 4] += 1u;
		carry = 0u;
	}
	if (flat) return;
	__syncthreads();
	const uint64_t n = (uint64_t)SRT_BINS * a.ntiles;
	const g_u32w rec = W32(a.thist);
#pragma unroll 1
	for (uint64_t b0 = 0; b0 < n; b0 += (uint64_t)SRT_SCAN_THREADS * SRT_SCAN_PER) {
		const uint64_t b = b0 + (uint64_t)SRT_SCAN_PER * threadIdx.x;
		uint32_t e[SRT_SCAN_PER], mine = 0;
#pragma unroll
		for (uint32_t k = 0; k < SRT_SCAN_PER; k++) {
			e[k] = b + k < n ? rec[b + k] : 0u;
			mine += e[k];
		}
		const uint32_t x = (uint32_t)wave_incl_sum(mine, lane);
		if (lane == 63u) wtot[wave] = x;
		__syncthreads();
		uint32_t before = carry;
		for (uint32_t w = 0; w < wave; w++) before += wtot[w];
		uint32_t run = before + x - mine;
#pragma unroll
		for (uint32_t k = 0; k < SRT_SCAN_PER; k++) {
			if (b + k < n) rec[b + k] = run;
			run += e[k];
		}
		__syncthreads();
		if (threadIdx.x == SRT_SCAN_THREADS - 1u) carry = before + x;
		__syncthreads();
	}
}

/* pass 1d (grid: ntiles): the tile's entries to where their bins begin, in their order.  Wavefront w takes the tile's entries
 * [w, w + 1) * 64 * SRT_ITEMS, 64 a step: the lanes with a lane's digit by eight ballots, its rank among them, the wavefront's
 * running count of the digit in LDS; then the counts of the wavefronts before it. */
__global__ void __launch_bounds__(SRT_THREADS)
srt_scatter(const SrtRun a)
{
	__shared__ uint32_t wcnt[SRT_WAVES][SRT_BINS];
	if (digit_is_flat(a)) return;
	const bool odd = G32(a.ghist)[SRT_DIGITS * SRT_BINS + a.digit] != 0u;
	const g_u32p src = odd ? G32(a.perm1) : G32(a.perm0);
	const g_u32w dst = odd ? W32(a.perm0) : W32(a.perm1);
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll
	for (uint32_t w = 0; w < SRT_WAVES; w++) wcnt[w][threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t base = (uint64_t)blockIdx.x * SRT_TILE + (uint64_t)wave * (64u * SRT_ITEMS) + lane;
	const uint64_t below = ((uint64_t)1 << lane) - 1u;
	uint32_t ent[SRT_ITEMS], dig[SRT_ITEMS], loc[SRT_ITEMS];
#pragma unroll
	for (uint32_t s = 0; s < SRT_ITEMS; s++) {
		const uint64_t i = base + (uint64_t)s * 64u;
		const bool valid = i < a.A;
		ent[s] = valid ? min32(src[i], (uint32_t)(a.A - 1u)) : 0u;
		dig[s] = valid ? entry_digit(a, ent[s]) : SRT_BINS;
		uint64_t peers = __ballot(valid);
#pragma unroll
		for (uint32_t b = 0; b < 8u; b++) {
			const bool bit = (dig[s] >> b & 1u) != 0u;
			const uint64_t m = __ballot(bit);
			peers &= bit ? m : ~m;
		}
		const uint32_t rnk = (uint32_t)__builtin_popcountll(peers & below);
		uint32_t pre = 0;
		if (valid) pre = wcnt[wave][dig[s]];                 /* every lane of the digit reads, then its first lane adds */
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (valid && rnk == 0u) wcnt[wave][dig[s]] = pre + (uint32_t)__builtin_popcountll(peers);
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		loc[s] = pre + rnk;
	}
	__syncthreads();
	{	/* bin threadIdx.x: where the entries of each wavefront begin */
		uint32_t at = G32(a.thist)[(uint64_t)threadIdx.x * a.ntiles + blockIdx.x];
#pragma unroll
		for (uint32_t w = 0; w < SRT_WAVES; w++) {
			const uint32_t c = wcnt[w][threadIdx.x];
			wcnt[w][threadIdx.x] = at;
			at += c;
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t s = 0; s < SRT_ITEMS; s++) {
		if (dig[s] >= SRT_BINS) continue;
		const uint64_t to = (uint64_t)wcnt[wave][dig[s]] + loc[s];
		if (to < a.A) dst[to] = ent[s];
	}
}

/* sorted entry i: its bucket, word, valid */
struct SrtKey {
	uint32_t bucket, valid;
	uint64_t word;
};
__device__ __forceinline__ SrtKey key_of(const SrtRun &a, g_u32p fin, uint64_t i)
{
	const uint32_t e = min32(fin[i], (uint32_t)(a.A - 1u));
	return SrtKey{G32(a.ebkt)[e], G32(a.eval)[e], G64(a.eword)[e]};
}

/* pass 2a (grid: srt_blocks(A)) */
__global__ void __launch_bounds__(SRT_THREADS)
srt_mark(const SrtRun a)
{
	__shared__ uint64_t wtot[SRT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	const g_u32p fin = G32(a.ghist)[SRT_DIGITS * SRT_BINS + a.ndigits] != 0u ? G32(a.perm1) : G32(a.perm0);
	uint64_t act = 0, lasthead = 0;
	if (i < a.A) {
		const SrtKey k = key_of(a, fin, i);
		SrtKey q = k, nx = k;
		if (i != 0u) q = key_of(a, fin, i - 1u);
		if (i + 1u < a.A) nx = key_of(a, fin, i + 1u);
		const bool head = srt_head(i == 0u, k.bucket, k.word, k.valid, q.bucket, q.word, q.valid);
		const bool member = i + 1u < a.A && !srt_head(false, nx.bucket, nx.word, nx.valid, k.bucket, k.word, k.valid);
		const bool active = srt_active(head, member, a.major_round ? SRT_WORD : srt_raw_valid(k.valid, a.reverse));
		const uint32_t p = min32(G32(a.apos)[i], (uint32_t)(a.R - 1u));
		W32(a.order)[p] = G32(a.eord)[min32(fin[i], (uint32_t)(a.A - 1u))];
		W32(a.eflag)[i] = (head ? 1u : 0u) | (active ? 2u : 0u);
		act = active ? 1u : 0u;
		lasthead = head ? (uint64_t)p + 1u : 0u;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		act += __shfl_xor(act, d, 64);
		const uint64_t y = __shfl_xor(lasthead, d, 64);
		lasthead = y > lasthead ? y : lasthead;
	}
	if (lane == 0u) { wtot[wave][0] = act; wtot[wave][1] = lasthead; }
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint64_t sa = 0, sh = 0;
#pragma unroll
		for (uint32_t w = 0; w < SRT_WAVES; w++) { sa += wtot[w][0]; sh = wtot[w][1] > sh ? wtot[w][1] : sh; }
		*(g_u64x2w)(uintptr_t)(a.blk + 2u * blockIdx.x) = u64x2s{sa, sh};
	}
}

/* pass 2b (one workgroup): per block the active entries and the last head before it; meta[0] = the active entries */
__global__ void __launch_bounds__(SRT_SCAN_THREADS)
srt_blocks_scan(const SrtRun a)
{
	__shared__ uint64_t wtot[SRT_SCAN_THREADS / 64u][2];
	__shared__ uint64_t carry[2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t n = srt_blocks(a.A);
	if (threadIdx.x == 0u) carry[0] = carry[1] = 0u;
	__syncthreads();
#pragma unroll 1
	for (uint64_t b0 = 0; b0 < n; b0 += SRT_SCAN_THREADS) {
		const uint64_t b = b0 + threadIdx.x;
		u64x2s e = u64x2s{0u, 0u};
		if (b < n) e = *(g_u64x2p)(uintptr_t)(a.blk + 2u * b);
		const uint64_t xs = wave_incl_sum(e.x, lane), xm = wave_incl_max(e.y, lane);
		if (lane == 63u) { wtot[wave][0] = xs; wtot[wave][1] = xm; }
		__syncthreads();
		uint64_t bs = carry[0], bm = carry[1];
		for (uint32_t w = 0; w < wave; w++) { bs += wtot[w][0]; bm = wtot[w][1] > bm ? wtot[w][1] : bm; }
		const uint64_t pm = __shfl_up(xm, 1, 64);            /* exclusive: the maximum of the lanes before */
		const uint64_t em = lane != 0u && pm > bm ? pm : bm;
		if (b < n) *(g_u64x2w)(uintptr_t)(a.blk + 2u * b) = u64x2s{bs + xs - e.x, em};
		__syncthreads();
		if (threadIdx.x == SRT_SCAN_THREADS - 1u) { carry[0] = bs + xs; carry[1] = xm > bm ? xm : bm; }
		__syncthreads();
	}
	if (threadIdx.x == 0u) W64(a.meta)[0] = carry[0];
}

/* pass 2c (grid: srt_blocks(A)) */
__global__ void __launch_bounds__(SRT_THREADS)
srt_assign(const SrtRun a)
{
	__shared__ uint64_t wtot[SRT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	uint32_t flag = 0, p = 0;
	if (i < a.A) {
		flag = G32(a.eflag)[i];
		p = min32(G32(a.apos)[i], (uint32_t)(a.R - 1u));
	}
	const uint64_t act = flag >> 1 & 1u, hd = (flag & 1u) != 0u ? (uint64_t)p + 1u : 0u;
	const uint64_t xs = wave_incl_sum(act, lane), xm = wave_incl_max(hd, lane);
	if (lane == 63u) { wtot[wave][0] = xs; wtot[wave][1] = xm; }
	__syncthreads();
	const u64x2s base = *(g_u64x2p)(uintptr_t)(a.blk + 2u * blockIdx.x);
	uint64_t j = base.x + (xs - act), h = base.y > xm ? base.y : xm;
#pragma unroll
	for (uint32_t w = 0; w < SRT_WAVES; w++) {
		j += w < wave ? wtot[w][0] : 0u;
		h = w < wave && wtot[w][1] > h ? wtot[w][1] : h;
	}
	if (i >= a.A) return;
	const uint32_t head = h != 0u ? (uint32_t)(h - 1u) : 0u;     /* (entry 0 is a head: h != 0) */
	W32(a.bucket)[p] = min32(head, p);
	if (act != 0u) {
		if (j < a.A) W32(a.napos)[j] = p;
		if ((flag & 1u) != 0u) W64(a.skip)[p] = ~(uint64_t)0;
	}
}

/* position p opens a group, and the bytes its record takes in the sorted text */
__device__ __forceinline__ void group_of(const SrtRun &a, uint64_t p, uint64_t *head, uint64_t *len, uint32_t *r)
{
	*head = *len = 0;
	*r = 0;
	if (p >= a.R) return;
	*r = min32(G32(a.order)[p], (uint32_t)(a.R - 1u));
	*head = G32(a.bucket)[p] == (uint32_t)p ? 1u : 0u;
	*len = a.text ? G64(a.klen)[*r] + (a.sep >= 0 ? 1u : 0u) : 0u;
}

/* pass 3a (grid: srt_blocks(R)) */
__global__ void __launch_bounds__(SRT_THREADS)
srt_ranks(const SrtRun a)
{
	__shared__ uint64_t wtot[SRT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t cnt, len;
	uint32_t r;
	group_of(a, (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x, &cnt, &len, &r);
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
		for (uint32_t w = 0; w < SRT_WAVES; w++) { sc += wtot[w][0]; sb += wtot[w][1]; }
		*(g_u64x2w)(uintptr_t)(a.pairs + 2u * blockIdx.x) = u64x2s{sc, sb};
	}
}

/* pass 3b (grid: srt_blocks(R)): the block's own scan redone */
__global__ void __launch_bounds__(SRT_THREADS)
srt_finish(const SrtRun a)
{
	__shared__ uint64_t wtot[SRT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t p = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
	uint64_t cnt, len;
	uint32_t r;
	group_of(a, p, &cnt, &len, &r);
	const uint64_t xc = wave_incl_sum(cnt, lane), xl = wave_incl_sum(len, lane);
	if (lane == 63u) { wtot[wave][0] = xc; wtot[wave][1] = xl; }
	__syncthreads();
	const u64x2s base = *(g_u64x2p)(uintptr_t)(a.pairs + 2u * blockIdx.x);
	uint64_t g = base.x + xc, at = base.y + (xl - len);
#pragma unroll
	for (uint32_t w = 0; w < SRT_WAVES; w++) {
		g += w < wave ? wtot[w][0] : 0u;
		at += w < wave ? wtot[w][1] : 0u;
	}
	if (p < a.R) {
		W64(a.order64)[p] = r;
		W32(a.rank)[p] = g != 0u ? (uint32_t)(g - 1u) : 0u;     /* (position 0 opens a group: g != 0) */
		if (a.soff != nullptr) {
			W64(a.soff)[p] = at;
			W64(a.src)[p] = G64(a.kbeg)[r];
			if (a.bfirst != nullptr && len != 0u)        /* records with bytes tile the output: one covers each block boundary */
				for (uint64_t b = (at + EXT_BLOCK - 1u) / EXT_BLOCK; b < a.ngb && b * EXT_BLOCK < at + len; b++) W64(a.bfirst)[b] = p;
		}
	}
	if (p == 0u && a.soff != nullptr) {
		W64(a.soff)[a.R] = a.total;
		if (a.bfirst != nullptr) W64(a.bfirst)[a.ngb] = a.R;
	}
}

bool launched() { return HIP_OK(hipGetLastError()); }

#define SRT_LAUNCH(kernel, blocks, threads, s, run)                                        \
	do {                                                                                   \
		hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(threads), 0, s, run);    \
		if (!launched()) return -1;                                                        \
	} while (0)

}   // namespace

/* ---- the fronts: the sorted object (front.h) --------------------------------------------------------------------------------------
 * Four event pairs: keys, radix passes, rebucket, finish + write.  The first three are recorded anew every round and read after
 * the round's wait, so their times are sums over the rounds; the last pair is in flight at return. */
extern "C" size_t fsm_hip_sort_tile_records(void) { return fsmhip::SRT_TILE; }

struct __attribute__((visibility("hidden"))) fsm_hip_sorted : RunObject<4> {
	uint64_t nbytes = 0;                     /* (m is R) */
	size_t rounds = 0;
	double acc_ms[3] = {0.0, 0.0, 0.0};      /* keys, radix passes, rebucket: over the rounds */
	DevBuf<uint64_t> d_kbeg, d_klen, d_dep, d_skip, d_eword;   /* R each: internal */
	DevBuf<uint32_t> d_order32, d_bucket, d_apos, d_napos, d_ebkt, d_eval, d_eord, d_eflag, d_perm0, d_perm1;
	DevBuf<uint32_t> d_thist, d_ghist;
	DevBuf<uint64_t> d_blk, d_meta, d_pairs;
	DevBuf<uint64_t> d_order;                /* R */
	DevBuf<uint32_t> d_rank;                 /* R */
	DevBuf<uint64_t> d_soff;                 /* R + 1; NULL under NO_TEXT */
	DevBuf<uint64_t> d_src;                  /* R: internal */
	DevBuf<uint64_t> d_bfirst;               /* per block of the output, + 1: internal */
	DevBuf<unsigned char> d_sbytes;          /* nbytes, in whole blocks */
	DevBuf<uint64_t> own_off, own_major;     /* the host form's staged input */
	DevBuf<unsigned char> own_bytes;
};

extern "C" void fsm_hip_sorted_free(struct fsm_hip_sorted *sx) { run_free(sx); }

/* one round on stream s: the entries, the radix passes, the rebucket, the wait; *A becomes the next round's entries */
static int sort_round(struct fsm_hip_sorted *sx, fsmhip::SrtRun &r, bool major_round, bool begun, uint64_t *tot, bool *have_tot, hipStream_t s)
{
	const uint64_t nb = fsmhip::srt_blocks(r.A);
	r.ntiles = (uint32_t)fsmhip::srt_tiles(r.A);
	r.major_round = major_round;
	if (!begun && !sx->begin(0, s)) return -1;
	if (!HIP_OK(hipMemsetAsync(r.ghist, 0, (fsmhip::SRT_DIGITS * fsmhip::SRT_BINS + fsmhip::SRT_PAR) * sizeof(uint32_t), s))) return -1;
	if (major_round) {
		SRT_LAUNCH(srt_major, nb, SRT_THREADS, s, r);
	} else {
		SRT_LAUNCH(srt_prefix, nb, SRT_THREADS, s, r);
		SRT_LAUNCH(srt_fetch, nb, SRT_THREADS, s, r);
	}
	if (!sx->end(0, s) || !sx->begin(1, s)) return -1;
	SRT_LAUNCH(srt_digits, r.ntiles, SRT_THREADS, s, r);
	for (r.digit = 0; r.digit < r.ndigits; r.digit++) {
		SRT_LAUNCH(srt_tile_hist, r.ntiles, SRT_THREADS, s, r);
		SRT_LAUNCH(srt_hist_scan, 1, SRT_SCAN_THREADS, s, r);
		SRT_LAUNCH(srt_scatter, r.ntiles, SRT_THREADS, s, r);
	}
	if (!sx->end(1, s) || !sx->begin(2, s)) return -1;
	SRT_LAUNCH(srt_mark, nb, SRT_THREADS, s, r);
	SRT_LAUNCH(srt_blocks_scan, 1, SRT_SCAN_THREADS, s, r);
	SRT_LAUNCH(srt_assign, nb, SRT_THREADS, s, r);
	if (!sx->end(2, s)) return -1;
	/* the round's ONE wait: the active entries (the first one: the text's bytes and the read limit too) */
	if (!HIP_OK(hipMemcpyAsync(tot, r.meta, (*have_tot ? 1u : 3u) * sizeof(uint64_t), hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return -1;
	*have_tot = true;
	for (int p = 0; p < 3; p++) {
		float ms = 0.f;
		if (!HIP_OK(hipEventElapsedTime(&ms, sx->ev[2 * p], sx->ev[2 * p + 1]))) return -1;
		sx->acc_ms[p] += (double)ms;
	}
	r.A = tot[0] <= r.R ? tot[0] : r.R;
	std::swap(r.apos, r.napos);
	return 0;
}

/* the passes on stream s into *sx, its device current; r: the packed text, the bytes and the flags (the rest is set here) */
static int sort_passes(struct fsm_hip_sorted *sx, fsmhip::SrtRun r, hipStream_t s)
{
	if (r.R == 0) {                                  /* no record: soff[0] alone, and nothing is launched */
		if (r.text && (!HIP_OK(sx->d_soff.alloc(1)) || !HIP_OK(hipMemsetAsync(sx->d_soff.p, 0, sizeof(uint64_t), s)))) return -1;
		for (DevEvent &ev : sx->ev)
			if (!HIP_OK(hipEventRecord(ev, s))) return -1;
		return 0;
	}
	const uint64_t R = r.R, nblocks = fsmhip::srt_blocks(R), ntiles = fsmhip::srt_tiles(R);
	if (!HIP_OK(sx->d_kbeg.alloc(R)) || !HIP_OK(sx->d_klen.alloc(R)) || !HIP_OK(sx->d_dep.alloc(R)) || !HIP_OK(sx->d_skip.alloc(R)) ||
	    !HIP_OK(sx->d_eword.alloc(R)) || !HIP_OK(sx->d_order32.alloc(R)) || !HIP_OK(sx->d_bucket.alloc(R)) || !HIP_OK(sx->d_apos.alloc(R)) ||
	    !HIP_OK(sx->d_napos.alloc(R)) || !HIP_OK(sx->d_ebkt.alloc(R)) || !HIP_OK(sx->d_eval.alloc(R)) || !HIP_OK(sx->d_eord.alloc(R)) ||
	    !HIP_OK(sx->d_eflag.alloc(R)) || !HIP_OK(sx->d_perm0.alloc(R)) || !HIP_OK(sx->d_perm1.alloc(R)) ||
	    !HIP_OK(sx->d_thist.alloc(fsmhip::SRT_BINS * ntiles)) || !HIP_OK(sx->d_ghist.alloc(fsmhip::SRT_DIGITS * fsmhip::SRT_BINS + fsmhip::SRT_PAR)) ||
	    !HIP_OK(sx->d_blk.alloc(2u * nblocks)) || !HIP_OK(sx->d_meta.alloc(fsmhip::SRT_META)) || !HIP_OK(sx->d_pairs.alloc(2u * nblocks + 2u)) ||
	    !HIP_OK(sx->d_order.alloc(R)) || !HIP_OK(sx->d_rank.alloc(R)))
		return -1;
	r.kbeg = sx->d_kbeg;
	r.klen = sx->d_klen;
	r.dep = sx->d_dep;
	r.skip = sx->d_skip;
	r.eword = sx->d_eword;
	r.order = sx->d_order32;
	r.bucket = sx->d_bucket;
	r.apos = sx->d_apos;
	r.napos = sx->d_napos;
	r.ebkt = sx->d_ebkt;
	r.eval = sx->d_eval;
	r.eord = sx->d_eord;
	r.eflag = sx->d_eflag;
	r.perm0 = sx->d_perm0;
	r.perm1 = sx->d_perm1;
	r.thist = sx->d_thist;
	r.ghist = sx->d_ghist;
	r.blk = sx->d_blk;
	r.meta = sx->d_meta;
	r.pairs = sx->d_pairs;
	r.order64 = sx->d_order;
	r.rank = sx->d_rank;
	r.ndigits = fsmhip::SRT_DIGIT_BUCKET + fsmhip::srt_bucket_digits(R);
	uint64_t tot[3] = {0, 0, 0};                     /* the active entries, the text's bytes, the bytes that may be read */
	bool have_tot = false, begun = true;
	if (!sx->begin(0, s)) return -1;
	if (!HIP_OK(hipMemsetAsync(r.meta, 0, fsmhip::SRT_META * sizeof(uint64_t), s))) return -1;
	SRT_LAUNCH(srt_init, nblocks, SRT_THREADS, s, r);
	r.A = R > 1u ? R : 0u;
	if (r.A != 0 && r.major != nullptr) {
		if (sort_round(sx, r, true, begun, tot, &have_tot, s) != 0) return -1;
		begun = false;
	}
	while (r.A != 0) {
		if (sx->rounds > srt_rounds_bound(r.nbytes)) { errno = EIO; return -1; }   /* (no key is longer than the text) */
		if (sort_round(sx, r, false, begun, tot, &have_tot, s) != 0) return -1;
		begun = false;
		sx->rounds++;
	}
	if (!have_tot) {                                 /* one record: no round, and the text's bytes are still to be read */
		if (!HIP_OK(hipMemcpyAsync(tot, r.meta, sizeof tot, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return -1;
	}
	sx->nbytes = r.text ? tot[1] : 0u;
	r.total = sx->nbytes;
	r.ngb = (r.total + fsmhip::EXT_BLOCK - 1u) / fsmhip::EXT_BLOCK;
	if (r.text && (!HIP_OK(sx->d_soff.alloc(R + 1u)) || !HIP_OK(sx->d_src.alloc(R)))) return -1;
	if (r.total != 0 && (!HIP_OK(sx->d_sbytes.alloc(r.ngb * fsmhip::EXT_BLOCK)) || !HIP_OK(sx->d_bfirst.alloc(r.ngb + 1u)))) return -1;
	r.soff = sx->d_soff;
	r.src = sx->d_src;
	r.bfirst = sx->d_bfirst;
	if (!sx->begin(3, s)) return -1;
	SRT_LAUNCH(srt_ranks, nblocks, SRT_THREADS, s, r);
	if (pairs_scan_launch(r.pairs, nblocks, s) != 0) return -1;
	SRT_LAUNCH(srt_finish, nblocks, SRT_THREADS, s, r);
	if (r.total != 0) {                              /* the extraction's write pass: record p is the key of order[p] */
		fsmhip::ExtRun w;
		w.base = r.bytes;
		w.limit = tot[2];
		w.sep = r.sep;
		w.out_off = r.soff;
		w.src = r.src;
		w.first = r.bfirst;
		w.out = sx->d_sbytes;
		w.nrec = R;
		w.total = r.total;
		w.ngb = r.ngb;
		const Grid g = grid_of(r.ngb, sx->device);
		w.wgs = g.wgs;
		w.per = g.per;
		if (fsmhip::ext_launch_write(w, s) != 0) return -1;
	}
	return sx->end(3, s) ? 0 : -1;
}

namespace fsmhip {

bool sort_args(size_t R, int trim_byte, int sep_byte, unsigned flags, unsigned allowed, bool has_major)
{
	if (trim_byte < -1 || trim_byte > 255 || sep_byte < -1 || sep_byte > 255 || (flags & ~allowed) != 0u ||
	    ((flags & FSM_HIP_SORT_MAJOR_DESC) != 0u && !has_major)) {
		errno = EINVAL;
		return false;
	}
	if ((uint64_t)R > SRT_MAX_RECORDS) { errno = EOVERFLOW; return false; }
	return true;
}

static SrtRun run_of(const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte, const uint64_t *d_major, int sep_byte, unsigned flags)
{
	SrtRun r;
	r.off = d_off;
	r.bytes = static_cast<const unsigned char *>(d_bytes);
	r.major = d_major;
	r.R = R;
	r.nbytes = nbytes;
	r.trim = trim_byte;
	r.sep = sep_byte;
	r.reverse = (flags & FSM_HIP_SORT_REVERSE) != 0u;
	r.major_desc = (flags & FSM_HIP_SORT_MAJOR_DESC) != 0u;
	r.text = (flags & FSM_HIP_SORT_NO_TEXT) == 0u;
	return r;
}

struct fsm_hip_sorted *sorted_new(int device, const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint64_t *d_major, int sep_byte, unsigned flags, hipEvent_t after, hipStream_t s)
{
	const SrtRun r = run_of(d_off, d_bytes, R, nbytes, trim_byte, d_major, sep_byte, flags);
	return run_new<struct fsm_hip_sorted>(device, R, true, s, [&](struct fsm_hip_sorted *sx) {
		if (after != nullptr && !HIP_OK(hipStreamWaitEvent(s, after, 0))) return -1;
		return sort_passes(sx, r, s);
	});
}

}   // namespace fsmhip

static constexpr unsigned SORT_FLAGS = FSM_HIP_SORT_NO_TEXT | FSM_HIP_SORT_REVERSE | FSM_HIP_SORT_MAJOR_DESC;

extern "C" struct fsm_hip_sorted *fsm_hip_sort_device(const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint64_t *d_major, int sep_byte, unsigned flags, void *hip_stream)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (d_off == nullptr || (d_bytes == nullptr && nbytes != 0)) { errno = EINVAL; return nullptr; }
	if (!fsmhip::sort_args(R, trim_byte, sep_byte, flags, SORT_FLAGS, d_major != nullptr)) return nullptr;
	return fsmhip::sorted_new(dev, d_off, d_bytes, R, nbytes, trim_byte, d_major, sep_byte, flags, nullptr, static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_sorted *fsm_hip_sort(const uint64_t *off, const void *bytes, size_t R, int trim_byte, const uint64_t *major, int sep_byte,
	unsigned flags)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (off == nullptr) { errno = EINVAL; return nullptr; }
	if (!fsmhip::sort_args(R, trim_byte, sep_byte, flags, SORT_FLAGS, major != nullptr)) return nullptr;
	for (size_t r = 0; r < R; r++)
		if (off[r] > off[r + 1u]) { errno = EINVAL; return nullptr; }
	const uint64_t nbytes = R != 0 ? off[R] : 0u;
	if (bytes == nullptr && nbytes != 0) { errno = EINVAL; return nullptr; }
	DevStream own;
	if (!HIP_OK(own.create(hipStreamNonBlocking))) return nullptr;
	const hipStream_t s = own;
	fsmhip::SrtRun r = fsmhip::run_of(nullptr, nullptr, R, nbytes, trim_byte, nullptr, sep_byte, flags);
	struct fsm_hip_sorted *sx = run_new<struct fsm_hip_sorted>(dev, R, true, s, [&](struct fsm_hip_sorted *o) {
		if (!HIP_OK(o->own_off.alloc(R + 1u)) || !HIP_OK(hipMemcpyAsync(o->own_off.p, off, (R + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, s))) return -1;
		if (nbytes != 0 && (!HIP_OK(o->own_bytes.alloc(nbytes)) || !HIP_OK(hipMemcpyAsync(o->own_bytes.p, bytes, nbytes, hipMemcpyHostToDevice, s)))) return -1;
		if (major != nullptr && R != 0 &&
		    (!HIP_OK(o->own_major.alloc(R)) || !HIP_OK(hipMemcpyAsync(o->own_major.p, major, R * sizeof(uint64_t), hipMemcpyHostToDevice, s))))
			return -1;
		r.off = o->own_off;
		r.bytes = o->own_bytes;
		r.major = o->own_major;
		return sort_passes(o, r, s);
	});
	if (sx == nullptr || HIP_OK(hipStreamSynchronize(s))) return sx;   /* (null: run_new left the stream idle) the stream goes at return */
	const int e = errno;
	run_free(sx);
	errno = e;
	return nullptr;
}

extern "C" struct fsm_hip_sorted *fsm_hip_extracted_sort(const struct fsm_hip_extracted *x, int sep_byte, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (x == nullptr) { errno = EINVAL; return nullptr; }
	if (!fsmhip::sort_args(x->nrec, x->sep, sep_byte, flags, SORT_FLAGS, false)) return nullptr;
	DevGuard dg(x->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return fsmhip::sorted_new(x->device, x->d_off, x->d_bytes, x->nrec, x->nbytes, x->sep, nullptr, sep_byte, flags, x->done(), static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_sorted *fsm_hip_text_hits_sort(const struct fsm_hip_text_hits *h, int sep_byte, unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (h == nullptr || h->d_off.p == nullptr) { errno = EINVAL; return nullptr; }   /* (no offsets: FSM_HIP_HITS_NO_BYTES) */
	if (!fsmhip::sort_args(h->m, h->delim, sep_byte, flags, SORT_FLAGS, false)) return nullptr;
	DevGuard dg(h->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return fsmhip::sorted_new(h->device, h->d_off, h->d_bytes, h->m, h->nbytes, h->delim, nullptr, sep_byte, flags, h->ev[5], static_cast<hipStream_t>(hip_stream));
}

extern "C" size_t fsm_hip_sorted_records(const struct fsm_hip_sorted *sx) { return sx == nullptr ? 0 : sx->m; }
extern "C" uint64_t fsm_hip_sorted_nbytes(const struct fsm_hip_sorted *sx) { return sx == nullptr ? 0 : sx->nbytes; }
extern "C" size_t fsm_hip_sorted_rounds(const struct fsm_hip_sorted *sx) { return sx == nullptr ? 0 : sx->rounds; }

/* the groups: the heads' total, which the finish leaves behind the block pairs; it waits for the finish */
extern "C" size_t fsm_hip_sorted_groups(const struct fsm_hip_sorted *sx)
{
	uint64_t g = 0;
	if (sx == nullptr || sx->m == 0) return 0;
	if (copy_out(sx->device, sx->done(), {{&g, sx->d_pairs.p + 2u * fsmhip::srt_blocks(sx->m), sizeof g}}) != 0) return 0;
	return (size_t)g;
}

/* the radix passes the rounds ran (skipped != 0: skipped, their digit had one occupied bin); it waits for nothing: the rounds are over */
extern "C" size_t fsm_hip_sorted_radix_passes(const struct fsm_hip_sorted *sx, int skipped)
{
	uint64_t n = 0;
	if (sx == nullptr || sx->m == 0) return 0;
	if (copy_out(sx->device, sx->done(), {{&n, sx->d_meta.p + (skipped != 0 ? 5 : 4), sizeof n}}) != 0) return 0;
	return (size_t)n;
}

extern "C" const uint64_t *fsm_hip_sorted_order_device(const struct fsm_hip_sorted *sx) { return sx == nullptr ? nullptr : sx->d_order.p; }
extern "C" const uint32_t *fsm_hip_sorted_rank_device(const struct fsm_hip_sorted *sx) { return sx == nullptr ? nullptr : sx->d_rank.p; }
extern "C" const uint64_t *fsm_hip_sorted_off_device(const struct fsm_hip_sorted *sx) { return sx == nullptr ? nullptr : sx->d_soff.p; }
extern "C" const unsigned char *fsm_hip_sorted_bytes_device(const struct fsm_hip_sorted *sx) { return sx == nullptr ? nullptr : sx->d_sbytes.p; }

extern "C" int fsm_hip_sorted_copy(const struct fsm_hip_sorted *sx, uint64_t *order, uint32_t *rank, uint64_t *soff, void *sbytes)
{
	if (sx == nullptr || (soff != nullptr && sx->d_soff.p == nullptr)) { errno = EINVAL; return -1; }
	return copy_out(sx->device, sx->done(), {{order, sx->d_order, sx->m * sizeof(uint64_t)}, {rank, sx->d_rank, sx->m * sizeof(uint32_t)},
	                                         {soff, sx->d_soff, (sx->m + 1u) * sizeof(uint64_t)}, {sbytes, sx->d_sbytes, (size_t)sx->nbytes}});
}

extern "C" double fsm_hip_sorted_pass_ms(const struct fsm_hip_sorted *sx, int pass)
{
	if (sx == nullptr || pass < 0 || pass > 3) { errno = EINVAL; return -1.0; }
	return pass < 3 ? sx->acc_ms[pass] : run_ms(sx, 3, 3);
}

extern "C" double fsm_hip_sorted_ms(const struct fsm_hip_sorted *sx)
{
	if (sx == nullptr) { errno = EINVAL; return -1.0; }
	const double last = run_ms(sx, 3, 3);
	return last < 0.0 ? last : sx->acc_ms[0] + sx->acc_ms[1] + sx->acc_ms[2] + last;
}
