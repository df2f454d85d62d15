/*
 * replace.hip -- replace every match by a per-rule replacement: the splice of a text and a table into a fresh packed text, on
 * the device.  include/fsm_hip.h, section "replace", is the definition; replace_seg.h holds the arithmetic of one line, shared
 * with tests/c/test_replace_seg.cpp.
 *
 * The matches (start, end, id per match, match_off per input) are on the device already, and so is the text.  Four passes, of
 * which the second is text.hip's (its sum_scan):
 *     repl_lengths  one lane per input walks its matches: mpos[k], xlen[k] (replace_seg.h) per match, the output length per
 *                   input, the sum of a block of REPL_LINES inputs per workgroup
 *     (scan)        the exclusive scan of the BLOCK sums by one workgroup; the total for the host
 *     repl_offsets  out_off[j] = the block's base + the block's own exclusive scan, redone (a wave scan and an LDS exchange);
 *                   first[g] = the input whose output covers byte g * REPL_BLOCK.  Only an input with output covers anything, so
 *                   runs of empty output lines leave no entry and need none
 *     repl_write    partitions the OUTPUT: a workgroup owns blocks of REPL_BLOCK bytes, a lane 16-byte chunks.  The chunk's
 *                   first byte p belongs to the LAST input j with out_off[j] <= p -- empty output lines share their offset with
 *                   their successor and are stepped over by the search itself -- found between first[g] and first[g + 1];
 *                   inside the line, to the last match with mpos <= p - out_off[j].  A chunk that lies in one copied stretch
 *                   of one line is one 16-byte load of any alignment; every other chunk is assembled stretch by stretch -- a
 *                   16-byte window per stretch, placed so that the stretch's bytes fall where they belong, and masked -- with
 *                   a new lookup whenever a stretch, a replacement or a line ends.
 * A template table (fsm_hip_repl_create_template: insert positions per rule, at which the match's own bytes stand inside the
 * replacement) runs repl_lengths<true> and repl_write<., true>: another repl_at(), in which a copy of the match is one more text
 * stretch; every other table runs the <false> kernels, which hold nothing of it.
 * No line belongs to a lane in the write pass: a line of 64 MiB is 4 096 blocks like any other 64 MiB.  In the lengths pass a lane
 * walks ITS line's matches alone, so a line of many matches holds its wavefront for that long.
 * Every global access names its address space (no FLAT instruction), every index read from an array is clamped to the array it
 * is used on, every text byte lies below the clipped line's end and with it below the limit (marks_clip, as in match.hip), every
 * store is below the counted sizes: arrays that changed between the passes give wrong bytes, not an overrun.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <new>
#include <optional>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "match.h"
#include "match_marks.h"
#include "replace_seg.h"
#include "text_objects.h"

namespace fsmhip {

constexpr uint32_t REPL_THREADS = 256;
constexpr uint32_t REPL_LINES = REPL_THREADS;               /* inputs of a block of the lengths and the offsets pass, one per lane */
constexpr uint32_t REPL_TILES = 4;
constexpr uint32_t REPL_TILE = REPL_THREADS * 16u;          /* output bytes one store instruction of the workgroup covers */
constexpr uint32_t REPL_BLOCK = REPL_TILES * REPL_TILE;     /* output bytes a workgroup writes per step: 16 KiB */
/* the table is read from LDS by the write pass when its bytes and its rules are both within these: 16 KiB + 4 KiB of a CU's
 * 160 KiB, so eight workgroups still fit a CU */
constexpr uint32_t REPL_LDS_BYTES = 16384;
constexpr uint32_t REPL_LDS_RULES = 1023;

static bool repl_table_fits_lds(uint64_t nrepl, uint64_t rbytes) { return nrepl <= REPL_LDS_RULES && rbytes <= REPL_LDS_BYTES; }
/* a table with nins inserts: its insert offsets and its positions, two bytes each, take their room out of the 16 KiB of bytes, behind
 * the table's bytes rounded up to 16 -- so every position and every insert offset fits a u16 */
static bool repl_tmpl_fits_lds(uint64_t nrepl, uint64_t rbytes, uint64_t nins)
{
	return repl_table_fits_lds(nrepl, rbytes) && nins <= REPL_LDS_BYTES && ((rbytes + 15u) & ~(uint64_t)15u) + 2u * (nrepl + 1u) + 2u * nins <= REPL_LDS_BYTES;
}

/* m inputs fit one launch's grid */
static bool repl_grid_fits(uint64_t m) { return (m + REPL_LINES - 1u) / REPL_LINES <= 0x7fffffffu; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself, so it spells the batch's fields
 * out where TokRun and MatchRun carry a LineBatch (line_batch.h): replaced_new copies them from one. */
struct ReplRun {
	/* the batch */
	const void *base = nullptr;
	const uint64_t *off = nullptr;           /* n + 1 */
	const uint64_t *pick = nullptr;          /* m, or null: input j is line j */
	uint64_t n = 0, m = 0, limit = 0;
	/* the matches */
	const uint64_t *moff = nullptr;          /* m + 1 */
	const uint64_t *start = nullptr, *end = nullptr;   /* nmatch */
	const uint32_t *id = nullptr;
	uint64_t nmatch = 0;
	/* the table */
	const unsigned char *rbytes_p = nullptr;
	const uint64_t *roff = nullptr;          /* nrepl + 1 */
	uint64_t nrepl = 0, rbytes = 0;
	unsigned flags = 0;                      /* FSM_HIP_REPL_* */
	bool table_in_lds = false;
	/* the object's arrays */
	uint64_t *out_off = nullptr;             /* m + 1: the lengths pass leaves the lengths, the offsets pass the offsets */
	uint64_t *mpos = nullptr, *xlen = nullptr;   /* nmatch each */
	uint64_t *sums = nullptr;                /* blocks of REPL_LINES inputs: their bytes, then (scanned) the bytes before them */
	uint64_t *first = nullptr;               /* ngb + 1 */
	unsigned char *out = nullptr;            /* ngb * REPL_BLOCK */
	uint64_t total = 0, ngb = 0;             /* known after the scan */
	uint64_t wgs = 1, per = 1;               /* the write pass's grid: wgs workgroups of `per` consecutive output blocks */
	/* the table's inserts (a template table with at least one): last, so that the fields above stay where the plain kernels read them */
	const uint64_t *ioff = nullptr;          /* nrepl + 1, or null: no rule has an insert */
	const uint64_t *ins = nullptr;           /* nins positions */
	uint64_t nins = 0;
};

/* the table has inserts: the template kernels run, for every other table the plain ones */
static bool repl_is_template(const ReplRun &r) { return r.nins != 0 && r.ioff != nullptr && r.ins != nullptr; }

}

using namespace fsmhip;

namespace {

constexpr uint32_t REPL_WAVES = REPL_THREADS / 64u;

typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
typedef u32x4r __attribute__((aligned(1))) u32x4r_any;
typedef const u32x4r_any __attribute__((address_space(1))) *g_chunkp;
typedef const u32x4r __attribute__((address_space(1))) *g_chunk16p;
typedef u32x4r __attribute__((address_space(1))) *g_chunkw;
typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
typedef uint64_t __attribute__((address_space(1))) *g_u64w;
typedef const uint8_t __attribute__((address_space(3))) *l_u8p;
typedef const uint32_t __attribute__((address_space(3))) *l_u32p;
typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
typedef const u32x4r_any __attribute__((address_space(3))) *l_chunkp;

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

/* the n lowest bytes of a word, n in 0 .. 8 */
__device__ __forceinline__ uint64_t low_bytes(uint32_t n) { return n >= 8u ? ~(uint64_t)0 : ((uint64_t)1 << (8u * n)) - 1u; }

/* byte k (0 .. 15) of the sixteen bytes (x0, x1) */
__device__ __forceinline__ void put_byte(uint64_t *x0, uint64_t *x1, uint32_t k, uint32_t b)
{
	const uint64_t bits = (uint64_t)b << ((k & 7u) * 8u);
	*x0 |= k < 8u ? bits : 0u;
	*x1 |= k < 8u ? 0u : bits;
}

/* the matches of input j: [k0, k0 + nm) of the match arrays, whatever match_off holds */
__device__ __forceinline__ void matches_of(g_u64p moff, uint64_t j, uint64_t nmatch, uint64_t *k0, uint64_t *nm)
{
	const uint64_t a = min64(moff[j], nmatch), b = min64(moff[j + 1u], nmatch);
	*k0 = a;
	*nm = b > a ? b - a : 0u;
}

/* the line of input j: its first byte from base and its bytes, clipped to the limit; a pick beyond the lines: nothing */
__device__ __forceinline__ void line_of(const ReplRun &a, uint64_t j, uint64_t *beg, uint64_t *raw)
{
	uint64_t i = j;
	if (a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	*beg = 0;
	*raw = 0;
	if (i < a.n) marks_clip(((g_u64p)(uintptr_t)a.off)[i], ((g_u64p)(uintptr_t)a.off)[i + 1u], a.limit, beg, raw);
}

/* pass 1: workgroup b takes inputs [b * REPL_LINES, (b + 1) * REPL_LINES), one per lane.  out_off[j] = the output length of input
 * j (the offsets pass turns it into the offset), sums[b] = the block's bytes; mpos and xlen of every match.  TMPL: the table has
 * inserts (never under MASK), and a rule's count of them is read from ioff. */
template <bool TMPL>
__global__ void __launch_bounds__(REPL_THREADS)
repl_lengths(const ReplRun a)
{
	__shared__ uint64_t wtot[REPL_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t j = (uint64_t)blockIdx.x * REPL_LINES + threadIdx.x;
	const bool mask = (a.flags & FSM_HIP_REPL_MASK) != 0u;
	const g_u64p start = (g_u64p)(uintptr_t)a.start, end = (g_u64p)(uintptr_t)a.end, roff = (g_u64p)(uintptr_t)a.roff;
	const g_u32p id = (g_u32p)(uintptr_t)a.id;
	const g_u64w mpos = (g_u64w)(uintptr_t)a.mpos, xlen = (g_u64w)(uintptr_t)a.xlen;
	uint64_t outlen = 0;
	if (j < a.m) {
		uint64_t beg, raw, k0, nm;
		line_of(a, j, &beg, &raw);
		matches_of((g_u64p)(uintptr_t)a.moff, j, a.nmatch, &k0, &nm);
		uint64_t delta = 0, floor = 0;               /* (delta wraps where a line shrinks; outlen does not: repl_clamp_match) */
		for (uint64_t k = k0; k < k0 + nm; k++) {
			uint64_t st = start[k], en = end[k];
			repl_clamp_match(floor, raw, &st, &en);
			const uint64_t i = id[k], mlen = en - st;
			uint64_t rlen = 0;
			if (i < a.nrepl) {
				const uint64_t r0 = roff[i], r1 = roff[i + 1u];
				rlen = r1 > r0 ? r1 - r0 : 0u;
			}
			uint64_t xl = repl_xlen(mlen, repl_uses_table(i, a.nrepl, rlen, mask), rlen, mask);
			if (TMPL && i < a.nrepl) {
				uint64_t i0;
				xl = repl_xlen(mlen, rlen, repl_inserts_of((g_u64p)(uintptr_t)a.ioff, i, a.nrepl, a.nins, &i0));
			}
			mpos[k] = st + delta;
			xlen[k] = xl;
			delta += xl - mlen;
			floor = en;
		}
		outlen = raw + delta;
		((g_u64w)(uintptr_t)a.out_off)[j] = outlen;
	}
	uint64_t s = outlen;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
	if (lane == 0) wtot[wave] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t all = 0;
#pragma unroll
		for (uint32_t w = 0; w < REPL_WAVES; w++) all += wtot[w];
		((g_u64w)(uintptr_t)a.sums)[blockIdx.x] = all;
	}
}

/* pass 3: out_off[j] = sums[b] (scanned: the bytes of the blocks before b) + the lengths of the block's inputs before j.
 * first[g] = j for every block boundary g * REPL_BLOCK inside j's output: inputs with output tile the output, so exactly one of
 * them covers a boundary below the total, and an input without output covers none. */
__global__ void __launch_bounds__(REPL_THREADS)
repl_offsets(const ReplRun a)
{
	__shared__ uint64_t wtot[REPL_WAVES];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t j = (uint64_t)blockIdx.x * REPL_LINES + threadIdx.x;
	const g_u64w oo = (g_u64w)(uintptr_t)a.out_off, fi = (g_u64w)(uintptr_t)a.first;
	const bool valid = j < a.m;
	const uint64_t len = valid ? oo[j] : 0u;
	uint64_t x = len;                                /* inclusive over the wave */
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t y = __shfl_up(x, d, 64);
		if (lane >= (uint32_t)d) x += y;
	}
	if (lane == 63u) wtot[wave] = x;
	__syncthreads();
	uint64_t p = ((g_u64p)(uintptr_t)a.sums)[blockIdx.x] + (x - len);
#pragma unroll
	for (uint32_t w = 0; w < REPL_WAVES; w++) p += w < wave ? wtot[w] : 0u;
	if (valid) {
		oo[j] = p;
		if (a.first != nullptr)
			for (uint64_t g = (p + REPL_BLOCK - 1u) / REPL_BLOCK; g < a.ngb && g * REPL_BLOCK < p + len; g++) fi[g] = j;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		oo[a.m] = a.total;
		if (a.first != nullptr) fi[a.ngb] = a.m;      /* the search's upper end in the last block */
	}
}

/* an input as the write pass sees it */
struct ReplLine {
	uint64_t o0, o1;         /* its output range */
	uint64_t beg, raw;       /* its bytes in the text */
	uint64_t k0, nm;         /* its matches */
};

__device__ __forceinline__ void open_line(const ReplRun &a, uint64_t j, ReplLine *L)
{
	const g_u64p oo = (g_u64p)(uintptr_t)a.out_off;
	L->o0 = oo[j];
	L->o1 = oo[j + 1u];
	line_of(a, j, &L->beg, &L->raw);
	matches_of((g_u64p)(uintptr_t)a.moff, j, a.nmatch, &L->k0, &L->nm);
}

/* the last j in [lo, hi] with out_off[j] <= p (lo, when there is none) */
__device__ __forceinline__ uint64_t line_at(g_u64p oo, uint64_t lo, uint64_t hi, uint64_t p)
{
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1u) / 2u;
		if (oo[mid] <= p) lo = mid; else hi = mid - 1u;
	}
	return lo;
}

/* pass 4.  IN_LDS: the table's bytes and its offsets (as u32) are copied to LDS first: the dynamic region, its base 16-byte
 * aligned, no static LDS in front of it.  TMPL: the table has inserts, and a stretch inside X_k may be the match's own bytes --
 * a text stretch like any other (replace_seg.h); in LDS the insert offsets and the positions follow the offsets, as u16
 * (repl_tmpl_fits_lds: both fit). */
template <bool IN_LDS, bool TMPL>
__global__ void __launch_bounds__(REPL_THREADS)
repl_write(const ReplRun a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char repl_smem[];
	const uint32_t roff_at = ((uint32_t)a.rbytes + 15u) & ~15u;
	const uint32_t ioff_at = roff_at + 4u * ((uint32_t)a.nrepl + 1u), ins_at = ioff_at + 2u * ((uint32_t)a.nrepl + 1u);
	if (IN_LDS) {
		__attribute__((address_space(3))) u32x4r *dst = (__attribute__((address_space(3))) u32x4r *)repl_smem;
		for (uint32_t c = threadIdx.x; c < roff_at / 16u; c += REPL_THREADS) dst[c] = ((g_chunk16p)(uintptr_t)a.rbytes_p)[c];
		__attribute__((address_space(3))) uint32_t *ro = (__attribute__((address_space(3))) uint32_t *)(repl_smem + roff_at);
		for (uint32_t e = threadIdx.x; e <= (uint32_t)a.nrepl; e += REPL_THREADS)
			ro[e] = (uint32_t)min64(((g_u64p)(uintptr_t)a.roff)[e], a.rbytes);
		if (TMPL) {
			__attribute__((address_space(3))) uint16_t *io = (__attribute__((address_space(3))) uint16_t *)(repl_smem + ioff_at);
			__attribute__((address_space(3))) uint16_t *in = (__attribute__((address_space(3))) uint16_t *)(repl_smem + ins_at);
			for (uint32_t e = threadIdx.x; e <= (uint32_t)a.nrepl; e += REPL_THREADS)
				io[e] = (uint16_t)min64(((g_u64p)(uintptr_t)a.ioff)[e], a.nins);
			for (uint32_t e = threadIdx.x; e < (uint32_t)a.nins; e += REPL_THREADS)
				in[e] = (uint16_t)min64(((g_u64p)(uintptr_t)a.ins)[e], a.rbytes);
		}
		__syncthreads();
	}
	const l_u8p tab_lds = (l_u8p)(__attribute__((address_space(3))) unsigned char *)repl_smem;
	const l_u32p roff_lds = (l_u32p)(__attribute__((address_space(3))) unsigned char *)(repl_smem + roff_at);
	const l_u16p ioff_lds = (l_u16p)(__attribute__((address_space(3))) unsigned char *)(repl_smem + ioff_at);
	const l_u16p ins_lds = (l_u16p)(__attribute__((address_space(3))) unsigned char *)(repl_smem + ins_at);
	const g_u8p tab_glb = (g_u8p)(uintptr_t)a.rbytes_p;
	const g_u64p roff_glb = (g_u64p)(uintptr_t)a.roff;
	const g_u64p oo = (g_u64p)(uintptr_t)a.out_off, fi = (g_u64p)(uintptr_t)a.first;
	const g_u64p mpos = (g_u64p)(uintptr_t)a.mpos, xlen = (g_u64p)(uintptr_t)a.xlen;
	const g_u64p start = (g_u64p)(uintptr_t)a.start, end = (g_u64p)(uintptr_t)a.end;
	const g_u32p id = (g_u32p)(uintptr_t)a.id;
	const uint64_t tx = (uint64_t)(uintptr_t)a.base, ox = (uint64_t)(uintptr_t)a.out;
	const uint64_t m = a.m, total = a.total, limit = a.limit;
	const bool mask = (a.flags & FSM_HIP_REPL_MASK) != 0u;

	auto source = [&](const ReplLine &L, uint64_t p) {
		const uint64_t outlen = L.o1 > L.o0 ? L.o1 - L.o0 : 0u;
		if (TMPL && IN_LDS)
			return repl_at(mpos + L.k0, xlen + L.k0, start + L.k0, end + L.k0, id + L.k0, L.nm, roff_lds, ioff_lds, ins_lds, a.nrepl, a.rbytes,
			               a.nins, p - L.o0, outlen, L.raw);
		if (TMPL)
			return repl_at(mpos + L.k0, xlen + L.k0, start + L.k0, end + L.k0, id + L.k0, L.nm, roff_glb, (g_u64p)(uintptr_t)a.ioff,
			               (g_u64p)(uintptr_t)a.ins, a.nrepl, a.rbytes, a.nins, p - L.o0, outlen, L.raw);
		if (IN_LDS)
			return repl_at(mpos + L.k0, xlen + L.k0, start + L.k0, end + L.k0, id + L.k0, L.nm, roff_lds, a.nrepl, a.rbytes, mask, p - L.o0,
			               outlen, L.raw);
		return repl_at(mpos + L.k0, xlen + L.k0, start + L.k0, end + L.k0, id + L.k0, L.nm, roff_glb, a.nrepl, a.rbytes, mask, p - L.o0, outlen,
		               L.raw);
	};

	uint64_t g = (uint64_t)blockIdx.x * a.per;
	const uint64_t gend = g + a.per < a.ngb ? g + a.per : a.ngb;
	for (; g < gend; g++) {
		uint64_t j = min64(fi[g], m - 1u);
		const uint64_t hi = min64(fi[g + 1u], m - 1u);
#pragma unroll 1
		for (uint32_t u = 0; u < REPL_TILES; u++) {
			const uint64_t p = g * REPL_BLOCK + (uint64_t)u * REPL_TILE + 16u * threadIdx.x;
			if (p >= total) break;
			j = line_at(oo, j, hi, p);                   /* the tiles of a lane ascend, so j only grows */
			ReplLine L;
			open_line(a, j, &L);
			ReplAt s = source(L, p);
			u32x4r v;
			if (s.from == REPL_FROM_TEXT && s.run >= 16u && L.beg + s.at + 16u <= limit) {
				v = *(g_chunkp)(tx + L.beg + s.at);      /* the whole chunk in one copied stretch of one line: any alignment */
			} else {
				uint64_t w0 = 0, w1 = 0, jj = j;
				uint32_t t = 0;
#pragma unroll 1
				while (t < 16u && p + t < total) {
					const uint64_t pos = p + t;
					if (s.run == 0u) {                   /* a stretch, a replacement or the line ended: look again */
						if (pos >= L.o1 && jj < hi) {    /* the next line WITH output: the search steps over the empty ones */
							jj = line_at(oo, jj + 1u, hi, pos);
							open_line(a, jj, &L);
						}
						s = source(L, pos);
					}
					const uint32_t cnt = s.run < 16u - t ? (uint32_t)s.run : 16u - t;   /* this stretch's bytes in the chunk: 1 .. 16 */
					/* a window of 16 bytes whose byte t is the source byte at s.at: one load where the window lies inside the
					 * readable bytes (of the text: outside the line, inside the limit), byte loads at the two edges */
					uint64_t x0 = 0, x1 = 0;
					if (s.from == REPL_FROM_TEXT) {
						const uint64_t src = L.beg + s.at;
						if (src >= t && src - t + 16u <= limit) {
							const u32x4r y = *(g_chunkp)(tx + src - t);
							x0 = y.x | (uint64_t)y.y << 32;
							x1 = y.z | (uint64_t)y.w << 32;
						} else {
							for (uint32_t k = 0; k < cnt; k++)
								if (src + k < limit) put_byte(&x0, &x1, t + k, ((g_u8p)tx)[src + k]);
						}
					} else if (s.from == REPL_FROM_TABLE) {
						if (s.at >= t && s.at - t + 16u <= roff_at) {    /* (both copies of the table are whole sixteens) */
							const u32x4r y = IN_LDS ? *(l_chunkp)(tab_lds + (s.at - t)) : *(g_chunkp)((uint64_t)(uintptr_t)a.rbytes_p + (s.at - t));
							x0 = y.x | (uint64_t)y.y << 32;
							x1 = y.z | (uint64_t)y.w << 32;
						} else {
							for (uint32_t k = 0; k < cnt; k++)
								if (s.at + k < a.rbytes) put_byte(&x0, &x1, t + k, IN_LDS ? (uint32_t)tab_lds[s.at + k] : (uint32_t)tab_glb[s.at + k]);
						}
					}
					const uint32_t e = t + cnt;
					w0 |= x0 & low_bytes(e < 8u ? e : 8u) & ~low_bytes(t < 8u ? t : 8u);
					w1 |= x1 & low_bytes(e > 8u ? e - 8u : 0u) & ~low_bytes(t > 8u ? t - 8u : 0u);
					t = e;
					s.at += cnt;
					s.run -= cnt;
				}
				v = u32x4r{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
			}
			*(g_chunkw)(ox + p) = v;                     /* the buffer is whole blocks: the last chunk is stored whole */
		}
	}
}

}   // namespace

namespace fsmhip {

/* each on stream s, the objects' device current; 0, or -1 + errno */
static int repl_launch_lengths(const ReplRun &r, hipStream_t s)
{
	if (r.m == 0) return 0;
	if (!repl_grid_fits(r.m)) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)((r.m + REPL_LINES - 1u) / REPL_LINES)), block(REPL_THREADS);
	if (repl_is_template(r)) hipLaunchKernelGGL(repl_lengths<true>, grid, block, 0, s, r);
	else hipLaunchKernelGGL(repl_lengths<false>, grid, block, 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

static int repl_launch_offsets(const ReplRun &r, hipStream_t s)
{
	if (r.m == 0) return 0;
	if (!repl_grid_fits(r.m)) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)((r.m + REPL_LINES - 1u) / REPL_LINES)), block(REPL_THREADS);
	hipLaunchKernelGGL(repl_offsets, grid, block, 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

static int repl_launch_write(const ReplRun &r, hipStream_t s)
{
	if (r.m == 0 || r.total == 0 || r.ngb == 0) return 0;
	if (r.wgs == 0 || r.wgs > 0x7fffffffu) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)r.wgs), block(REPL_THREADS);
	const bool tmpl = repl_is_template(r);
	if (tmpl && (r.flags & FSM_HIP_REPL_MASK) != 0u) { errno = EINVAL; return -1; }
	if (r.table_in_lds) {
		if (!(tmpl ? repl_tmpl_fits_lds(r.nrepl, r.rbytes, r.nins) : repl_table_fits_lds(r.nrepl, r.rbytes))) { errno = EINVAL; return -1; }
		const size_t lds = (((size_t)r.rbytes + 15u) & ~(size_t)15u) + 4u * ((size_t)r.nrepl + 1u);
		if (tmpl) hipLaunchKernelGGL((repl_write<true, true>), grid, block, lds + 2u * ((size_t)r.nrepl + 1u) + 2u * (size_t)r.nins, s, r);
		else hipLaunchKernelGGL((repl_write<true, false>), grid, block, lds, s, r);
	} else {
		if (tmpl) hipLaunchKernelGGL((repl_write<false, true>), grid, block, 0, s, r);
		else hipLaunchKernelGGL((repl_write<false, false>), grid, block, 0, s, r);
	}
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

}   // namespace fsmhip

/* ---- the fronts: the table, and the replaced text as an object of four passes (front.h) -------------------------------------------
 * lengths pass (per input, per match, per block of REPL_LINES inputs) -> exclusive scan of the BLOCK sums by one workgroup -> ONE
 * wait for the total -> allocation -> offsets pass (the block's own scan redone, first[]) -> write pass.  The scan runs over
 * m / REPL_LINES records, not over m: a text of short lines does not pay the one-workgroup scan per line that the tokens and
 * the matches pay.  first[] has an entry per block of the output, so the offsets pass that fills it follows the wait; it and the
 * write pass are in flight at return. */
struct __attribute__((visibility("hidden"))) fsm_hip_repl {
	int device = 0;
	size_t nrepl = 0;
	uint64_t rbytes = 0;
	unsigned flags = 0;
	bool in_lds = false;
	DevBuf<unsigned char> d_bytes;           /* rbytes, rounded up to 16 and never nothing */
	DevBuf<uint64_t> d_roff;                 /* nrepl + 1 */
	uint64_t nins = 0;                       /* a template table's inserts; 0: a plain table, and the two arrays below are not there */
	DevBuf<uint64_t> d_ioff;                 /* nrepl + 1 */
	DevBuf<uint64_t> d_ins;                  /* nins */
};

/* the table on device `dev`; the arguments are checked.  nins != 0: ioff[nrepl + 1] and ins[nins] go along */
static struct fsm_hip_repl *repl_new(int dev, const void *bytes, const uint64_t *roff, size_t nrepl, const uint64_t *ins, const uint64_t *ioff,
	uint64_t nins, unsigned flags)
{
	const uint64_t rbytes = nrepl != 0 ? roff[nrepl] : 0u;
	struct fsm_hip_repl *rp = new (std::nothrow) struct fsm_hip_repl;
	if (rp == nullptr) { errno = ENOMEM; return nullptr; }
	rp->device = dev;
	rp->nrepl = nrepl;
	rp->rbytes = rbytes;
	rp->flags = flags;
	rp->nins = nins;
	rp->in_lds = nins != 0 ? fsmhip::repl_tmpl_fits_lds(nrepl, rbytes, nins) : fsmhip::repl_table_fits_lds(nrepl, rbytes);
	const uint64_t zero = 0;
	if (HIP_OK(rp->d_bytes.upload_bytes(bytes, (size_t)rbytes, 16)) &&
	    HIP_OK(rp->d_roff.upload_bytes(nrepl != 0 ? roff : &zero, (nrepl + 1u) * sizeof(uint64_t), sizeof(uint64_t))) &&
	    (nins == 0 || (HIP_OK(rp->d_ioff.upload_bytes(ioff, (nrepl + 1u) * sizeof(uint64_t), sizeof(uint64_t))) &&
	                   HIP_OK(rp->d_ins.upload_bytes(ins, (size_t)nins * sizeof(uint64_t), sizeof(uint64_t))))))
		return rp;
	const int e = errno;
	delete rp;
	errno = e;
	return nullptr;
}

/* what both kinds of table refuse: roff NULL with rules, roff that decreases, bytes NULL with bytes to copy */
static bool repl_table_ok(const void *bytes, const uint64_t *roff, size_t nrepl)
{
	if (roff == nullptr && nrepl != 0) return false;
	for (size_t i = 0; i < nrepl; i++)
		if (roff[i] > roff[i + 1u]) return false;
	return !(nrepl != 0 && roff[nrepl] != 0 && bytes == nullptr);
}

extern "C" struct fsm_hip_repl *fsm_hip_repl_create(const void *bytes, const uint64_t *roff, size_t nrepl, unsigned flags)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if ((flags & ~FSM_HIP_REPL_MASK) != 0u || !repl_table_ok(bytes, roff, nrepl)) { errno = EINVAL; return nullptr; }
	return repl_new(dev, bytes, roff, nrepl, nullptr, nullptr, 0, flags);
}

extern "C" struct fsm_hip_repl *fsm_hip_repl_create_template(const void *bytes, const uint64_t *roff, size_t nrepl, const uint64_t *ins,
	const uint64_t *ioff, unsigned flags)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if (flags != 0u || !repl_table_ok(bytes, roff, nrepl)) { errno = EINVAL; return nullptr; }
	uint64_t nins = 0;
	if (ioff != nullptr) {
		if (ioff[0] != 0u) { errno = EINVAL; return nullptr; }
		for (size_t i = 0; i < nrepl; i++) {
			if (ioff[i] > ioff[i + 1u] || ioff[i + 1u] - ioff[i] > fsmhip::REPL_MAX_INSERTS || (ins == nullptr && ioff[i + 1u] != 0u)) { errno = EINVAL; return nullptr; }
			const uint64_t rlen = roff[i + 1u] - roff[i];
			for (uint64_t x = ioff[i]; x < ioff[i + 1u]; x++)
				if (ins[x] > rlen || (x > ioff[i] && ins[x] < ins[x - 1u])) { errno = EINVAL; return nullptr; }
		}
		nins = ioff[nrepl];
	}
	return repl_new(dev, bytes, roff, nrepl, ins, ioff, nins, 0u);
}

extern "C" void fsm_hip_repl_free(struct fsm_hip_repl *rp)
{
	if (rp == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(rp->device);
		delete rp;
	}
	errno = e;
}

extern "C" int fsm_hip_repl_in_lds(const struct fsm_hip_repl *rp) { return rp != nullptr && rp->in_lds ? 1 : 0; }
extern "C" size_t fsm_hip_repl_lds_bytes(void) { return fsmhip::REPL_LDS_BYTES; }
extern "C" size_t fsm_hip_repl_lds_rules(void) { return fsmhip::REPL_LDS_RULES; }
extern "C" size_t fsm_hip_repl_inserts(const struct fsm_hip_repl *rp) { return rp != nullptr ? (size_t)rp->nins : 0u; }
extern "C" size_t fsm_hip_repl_max_inserts(void) { return fsmhip::REPL_MAX_INSERTS; }
extern "C" size_t fsm_hip_replaced_block_lines(void) { return fsmhip::REPL_LINES; }
extern "C" size_t fsm_hip_replaced_block_bytes(void) { return fsmhip::REPL_BLOCK; }

struct __attribute__((visibility("hidden"))) fsm_hip_replaced : RunObject<4> {   /* the lengths, the scan, the offsets, the write pass */
	uint64_t nbytes = 0;
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_mpos, d_xlen;         /* one per match: internal */
	DevBuf<uint64_t> d_sums;                 /* per block of inputs, + the total: internal */
	DevBuf<uint64_t> d_first;                /* per block of the output, + 1: internal */
	DevBuf<unsigned char> d_bytes;           /* nbytes, in whole blocks */
};

extern "C" void fsm_hip_replaced_free(struct fsm_hip_replaced *r) { run_free(r); }

/* the passes on stream s into *rd, the objects' device current; r: the batch, the matches and the table (its outputs are set here) */
static int replaced_passes(struct fsm_hip_replaced *rd, fsmhip::ReplRun r, hipStream_t s)
{
	const uint64_t m = r.m, nblocks = (m + fsmhip::REPL_LINES - 1u) / fsmhip::REPL_LINES;
	uint64_t total = 0;
	if (!HIP_OK(rd->d_off.alloc(m + 1u))) return -1;
	if (m != 0 && !HIP_OK(rd->d_sums.alloc(nblocks + 1u))) return -1;
	if (m != 0 && r.nmatch != 0 && (!HIP_OK(rd->d_mpos.alloc(r.nmatch)) || !HIP_OK(rd->d_xlen.alloc(r.nmatch)))) return -1;
	r.out_off = rd->d_off;
	r.sums = rd->d_sums;
	r.mpos = rd->d_mpos;
	r.xlen = rd->d_xlen;
	if (!rd->begin(0, s)) return -1;
	if (fsmhip::repl_launch_lengths(r, s) != 0) return -1;
	if (!rd->end(0, s) || !rd->begin(1, s)) return -1;
	/* the total sizes the bytes and first[]; without inputs there are no sums, and out_off[0] is cleared */
	if (scan_total(m != 0 ? rd->d_sums.p : rd->d_off.p, nblocks, rd->ev[3], s, &total) != 0) return -1;
	rd->nbytes = total;
	r.total = total;
	r.ngb = (total + fsmhip::REPL_BLOCK - 1u) / fsmhip::REPL_BLOCK;
	if (total != 0 && (!HIP_OK(rd->d_bytes.alloc(r.ngb * fsmhip::REPL_BLOCK)) || !HIP_OK(rd->d_first.alloc(r.ngb + 1u)))) return -1;
	r.out = rd->d_bytes;
	r.first = rd->d_first;
	const Grid g = grid_of(r.ngb, rd->device);
	r.wgs = g.wgs;
	r.per = g.per;
	if (!rd->begin(2, s)) return -1;
	if (fsmhip::repl_launch_offsets(r, s) != 0) return -1;
	if (!rd->end(2, s) || !rd->begin(3, s)) return -1;
	if (fsmhip::repl_launch_write(r, s) != 0) return -1;
	return rd->end(3, s) ? 0 : -1;
}

static struct fsm_hip_replaced *replaced_new(const struct fsm_hip_matches *mt, const struct fsm_hip_repl *rp, const fsmhip::LineBatch &in, hipStream_t s)
{
	fsmhip::ReplRun r;
	r.base = in.base;
	r.off = in.off;
	r.pick = in.pick;
	r.n = in.n;
	r.m = in.m;
	r.limit = in.limit;
	r.moff = mt->d_off;
	r.start = mt->d_start;
	r.end = mt->d_end;
	r.id = mt->d_id;
	r.nmatch = mt->total;
	r.rbytes_p = rp->d_bytes;
	r.roff = rp->d_roff;
	r.nrepl = rp->nrepl;
	r.rbytes = rp->rbytes;
	r.flags = rp->flags;
	r.table_in_lds = rp->in_lds;
	if (rp->nins != 0) {
		r.ioff = rp->d_ioff;
		r.ins = rp->d_ins;
		r.nins = rp->nins;
	}
	return run_new<struct fsm_hip_replaced>(mt->device, in.m, fsmhip::repl_grid_fits(in.m), s, [&](struct fsm_hip_replaced *rd) {
		return HIP_OK(hipStreamWaitEvent(s, mt->done(), 0)) ? replaced_passes(rd, r, s) : -1;   /* behind the matches' emit pass */
	});
}

/* the arguments both forms refuse alike; *in: the batch as given, which is the matches' own: it passes what theirs passed */
static bool replaced_check(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b, const struct fsm_hip_repl *rp, fsmhip::LineBatch *in)
{
	if (!have_device()) { errno = ENODEV; return false; }
	if (mt == nullptr || rp == nullptr || rp->device != mt->device) { errno = EINVAL; return false; }
	if (!fsmhip::batch_shape(b, FSM_HIP_MATCHES_DROP_EMPTY, in)) return false;
	if (in->m != (uint64_t)mt->m) { errno = EINVAL; return false; }
	return true;
}

extern "C" struct fsm_hip_replaced *fsm_hip_matches_replace_device(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b,
	const struct fsm_hip_repl *rp, void *hip_stream)
{
	fsmhip::LineBatch in;
	if (!replaced_check(mt, b, rp, &in) || !fsmhip::batch_device_ok(in)) return nullptr;
	DevGuard dg(mt->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (!fsmhip::batch_read_limit(&in, s)) return nullptr;   /* as the matches: line extents are clamped to the limit */
	return replaced_new(mt, rp, in, s);
}

extern "C" struct fsm_hip_replaced *fsm_hip_matches_replace(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b,
	const struct fsm_hip_repl *rp)
{
	fsmhip::LineBatch host;
	if (!replaced_check(mt, b, rp, &host) || !fsmhip::batch_host_arrays_ok(host)) return nullptr;
	return run_host(mt->device, host, [&](const fsmhip::LineBatch &in, hipStream_t s) { return replaced_new(mt, rp, in, s); });
}

extern "C" struct fsm_hip_replaced *fsm_hip_text_replace(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t,
	const struct fsm_hip_text_hits *h, const struct fsm_hip_repl *rp, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (mt == nullptr || t == nullptr || rp == nullptr || mt->m != (h != nullptr ? h->m : t->n)) { errno = EINVAL; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	std::optional<DevGuard> dg;
	fsmhip::LineBatch in;
	if (!text_batch(t, h, {mt->device, rp->device}, s, &dg, &in)) return nullptr;
	return replaced_new(mt, rp, in, s);
}

extern "C" size_t fsm_hip_replaced_count(const struct fsm_hip_replaced *r) { return r == nullptr ? 0 : r->m; }
extern "C" uint64_t fsm_hip_replaced_nbytes(const struct fsm_hip_replaced *r) { return r == nullptr ? 0 : r->nbytes; }
extern "C" const uint64_t *fsm_hip_replaced_off_device(const struct fsm_hip_replaced *r) { return r == nullptr ? nullptr : r->d_off.p; }
extern "C" const unsigned char *fsm_hip_replaced_bytes_device(const struct fsm_hip_replaced *r) { return r == nullptr ? nullptr : r->d_bytes.p; }

extern "C" int fsm_hip_replaced_copy(const struct fsm_hip_replaced *r, uint64_t *off, void *bytes)
{
	if (r == nullptr) { errno = EINVAL; return -1; }
	return copy_out(r->device, r->done(), {{off, r->d_off, (r->m + 1u) * sizeof(uint64_t)}, {bytes, r->d_bytes, (size_t)r->nbytes}});
}

extern "C" double fsm_hip_replaced_ms(const struct fsm_hip_replaced *r) { return run_ms(r, 0, 3); }
extern "C" double fsm_hip_replaced_pass_ms(const struct fsm_hip_replaced *r, int pass) { return run_ms(r, pass, pass); }
