/*
 * extract.hip -- every kept match's bytes as a record of a fresh packed text, on the device.  include/fsm_hip.h, section
 * "extract", is the definition; extract_seg.h holds the arithmetic of one lookup, shared with tests/c/test_extract_seg.cpp.
 *
 * The matches (start, end, id per match, match_off per input) are on the device already, and so is the text.  Four passes, of
 * which the second is text.hip's (its sum_scan):
 *     ext_lengths   one lane per MATCH, a workgroup per block of EXT_MATCHES matches.  Two lanes find the inputs of the block's
 *                   first and last match in match_off, every lane then its own input between those two: the last j with
 *                   match_off[j] <= k, so inputs without matches, which share their offset with their successor, are stepped
 *                   over.  Per match: kept or not and the record's bytes (mrec), the text index of its first byte (msrc), its
 *                   input (mline); per workgroup the pair (records kept, bytes)
 *     (scan)        the exclusive scan of the BLOCK pairs by one workgroup; the totals for the host
 *     ext_offsets   the block's own exclusive scan redone (a wave scan and an LDS exchange) and the compaction: the kept match of
 *                   rank r writes off[r], src[r], line[r], match[r]; first[g] = r for every boundary g * EXT_BLOCK of the output
 *                   inside record r.  A record without bytes covers no boundary
 *     ext_write     partitions the OUTPUT: a workgroup owns blocks of EXT_BLOCK bytes, a lane 16-byte chunks.  The chunk's first
 *                   byte p belongs to the LAST r with off[r] <= p, found between first[g] and first[g + 1].  A chunk inside the
 *                   text part of one record is one 16-byte load of any alignment; every other chunk is assembled record by
 *                   record -- r, r + 1, ... without a search, a 16-byte window per record, placed so that the record's bytes fall
 *                   where they belong, and masked.  Only a run of records without bytes (no separator, empty matches kept) is
 *                   stepped over by the same search.
 * Every global access names its address space (no FLAT instruction), every index read from an array is clamped to the array it
 * is used on, every text byte lies below the limit, every store is below the counted sizes: arrays that changed between the
 * passes give wrong bytes, not an overrun.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <new>
#include <optional>
#include <vector>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "match.h"
#include "match_marks.h"
#include "extract.h"
#include "extract_seg.h"
#include "text_objects.h"

namespace fsmhip {

constexpr uint32_t EXT_MATCHES = EXT_THREADS;               /* matches of a block of the lengths and the offsets pass, one per lane */

/* nmatch matches fit one launch's grid */
static bool ext_grid_fits(uint64_t nmatch) { return (nmatch + EXT_MATCHES - 1u) / EXT_MATCHES <= 0x7fffffffu; }

}

using namespace fsmhip;

namespace {

constexpr uint32_t EXT_WAVES = EXT_THREADS / 64u;

typedef uint32_t u32x4e __attribute__((ext_vector_type(4)));
typedef u32x4e __attribute__((aligned(1))) u32x4e_any;
typedef uint64_t u64x2e __attribute__((ext_vector_type(2)));
typedef const u32x4e_any __attribute__((address_space(1))) *g_chunkp;
typedef u32x4e __attribute__((address_space(1))) *g_chunkw;
typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
typedef uint64_t __attribute__((address_space(1))) *g_u64w;
typedef u64x2e __attribute__((address_space(1))) *g_u64x2w;
typedef const u64x2e __attribute__((address_space(1))) *g_u64x2p;

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

/* the line of input j: its first byte from base and its bytes, clipped to the limit; a pick beyond the lines: nothing */
__device__ __forceinline__ void line_of(const ExtRun &a, uint64_t j, uint64_t *beg, uint64_t *raw)
{
	uint64_t i = j;
	if (a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	*beg = 0;
	*raw = 0;
	if (i < a.n) marks_clip(((g_u64p)(uintptr_t)a.off)[i], ((g_u64p)(uintptr_t)a.off)[i + 1u], a.limit, beg, raw);
}

/* pass 1: workgroup b takes matches [b * EXT_MATCHES, (b + 1) * EXT_MATCHES), one per lane (the launch sees to m >= 1 and
 * nmatch >= 1).  match_off[m] is never read: the last j with match_off[j] <= k is looked for in [0, m - 1]. */
__global__ void __launch_bounds__(EXT_THREADS)
ext_lengths(const ExtRun a)
{
	__shared__ uint64_t jrange[2];
	__shared__ uint64_t wtot[EXT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t k0 = (uint64_t)blockIdx.x * EXT_MATCHES, k = k0 + threadIdx.x;
	const g_u64p moff = (g_u64p)(uintptr_t)a.moff;
	if (threadIdx.x < 2u)                            /* side by side in one wavefront: one instruction stream for both */
		jrange[threadIdx.x] = ext_last_le(moff, 0u, a.m - 1u, threadIdx.x == 0u ? k0 : min64(k0 + EXT_MATCHES - 1u, a.nmatch - 1u));
	__syncthreads();
	uint64_t cnt = 0, len = 0;
	if (k < a.nmatch) {
		const uint64_t j = min64(ext_last_le(moff, jrange[0], jrange[1], k), a.m - 1u);
		uint64_t beg, raw;
		line_of(a, j, &beg, &raw);
		uint64_t st = ((g_u64p)(uintptr_t)a.start)[k], en = ((g_u64p)(uintptr_t)a.end)[k];
		ext_clamp_match(raw, &st, &en);
		if (ext_kept((g_u32p)(uintptr_t)a.keep, a.keep != nullptr, a.nrules, a.keep_other, ((g_u32p)(uintptr_t)a.id)[k])) {
			cnt = 1u;
			len = ext_record_len(st, en, a.sep >= 0);
		}
		((g_u64w)(uintptr_t)a.mrec)[k] = len << 1 | cnt;
		((g_u64w)(uintptr_t)a.msrc)[k] = beg + st;
		((g_u64w)(uintptr_t)a.mline)[k] = j;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		cnt += __shfl_xor(cnt, d, 64);
		len += __shfl_xor(len, d, 64);
	}
	if (lane == 0) { wtot[wave][0] = cnt; wtot[wave][1] = len; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t sc = 0, sb = 0;
#pragma unroll
		for (uint32_t w = 0; w < EXT_WAVES; w++) { sc += wtot[w][0]; sb += wtot[w][1]; }
		*(g_u64x2w)(uintptr_t)(a.pairs + 2u * blockIdx.x) = u64x2e{sc, sb};
	}
}

/* pass 3: the rank of a kept match = pairs[b] (scanned: the records of the blocks before b) + the kept matches of the block
 * before it; its offset likewise.  Stores are made for ranks below nrec alone.  first[g] = r for every block boundary
 * g * EXT_BLOCK inside r's bytes: records with bytes tile the output, so exactly one covers a boundary below the total. */
__global__ void __launch_bounds__(EXT_THREADS)
ext_offsets(const ExtRun a)
{
	__shared__ uint64_t wtot[EXT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t k = (uint64_t)blockIdx.x * EXT_MATCHES + threadIdx.x;
	const g_u64w oo = (g_u64w)(uintptr_t)a.out_off, fi = (g_u64w)(uintptr_t)a.first;
	const uint64_t rec = k < a.nmatch ? ((g_u64p)(uintptr_t)a.mrec)[k] : 0u;
	const uint64_t cnt = rec & 1u, len = rec >> 1;
	uint64_t xc = cnt, xl = len;                     /* inclusive over the wave, side by side */
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t yc = __shfl_up(xc, d, 64), yl = __shfl_up(xl, d, 64);
		if (lane >= (uint32_t)d) { xc += yc; xl += yl; }
	}
	if (lane == 63u) { wtot[wave][0] = xc; wtot[wave][1] = xl; }
	__syncthreads();
	const u64x2e base = *(g_u64x2p)(uintptr_t)(a.pairs + 2u * blockIdx.x);
	uint64_t r = base.x + (xc - cnt), p = base.y + (xl - len);
#pragma unroll
	for (uint32_t w = 0; w < EXT_WAVES; w++) {
		r += w < wave ? wtot[w][0] : 0u;
		p += w < wave ? wtot[w][1] : 0u;
	}
	if (cnt != 0u && r < a.nrec) {
		oo[r] = p;
		((g_u64w)(uintptr_t)a.src)[r] = ((g_u64p)(uintptr_t)a.msrc)[k];
		((g_u64w)(uintptr_t)a.line)[r] = ((g_u64p)(uintptr_t)a.mline)[k];
		((g_u64w)(uintptr_t)a.match)[r] = k;
		if (a.first != nullptr && len != 0u)
			for (uint64_t g = (p + EXT_BLOCK - 1u) / EXT_BLOCK; g < a.ngb && g * EXT_BLOCK < p + len; g++) fi[g] = r;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		oo[a.nrec] = a.total;
		if (a.first != nullptr) fi[a.ngb] = a.nrec;  /* the search's upper end in the last block */
	}
}

/* a record as the write pass sees it */
struct ExtRec {
	uint64_t o0, o1;         /* its output range */
	uint64_t src;            /* the text index of its first byte */
};

__device__ __forceinline__ void open_rec(g_u64p oo, g_u64p src, uint64_t r, ExtRec *R)
{
	R->o0 = oo[r];
	R->o1 = oo[r + 1u];
	R->src = src[r];
}

/* pass 4 (the launch sees to nrec >= 1 and total >= 1) */
__global__ void __launch_bounds__(EXT_THREADS)
ext_write(const ExtRun a)
{
	const g_u64p oo = (g_u64p)(uintptr_t)a.out_off, fi = (g_u64p)(uintptr_t)a.first, sr = (g_u64p)(uintptr_t)a.src;
	const uint64_t tx = (uint64_t)(uintptr_t)a.base, ox = (uint64_t)(uintptr_t)a.out;
	const uint64_t nrec = a.nrec, total = a.total, limit = a.limit;
	const bool has_sep = a.sep >= 0;
	const uint32_t sep = (uint32_t)a.sep & 0xffu;

	uint64_t g = (uint64_t)blockIdx.x * a.per;
	const uint64_t gend = g + a.per < a.ngb ? g + a.per : a.ngb;
	for (; g < gend; g++) {
		uint64_t r = min64(fi[g], nrec - 1u);
		const uint64_t hi = min64(fi[g + 1u], nrec - 1u);
#pragma unroll 1
		for (uint32_t u = 0; u < EXT_TILES; u++) {
			const uint64_t p = g * EXT_BLOCK + (uint64_t)u * EXT_TILE + 16u * threadIdx.x;
			if (p >= total) break;
			r = ext_last_le(oo, r, hi, p);               /* the tiles of a lane ascend, so r only grows */
			ExtRec R;
			open_rec(oo, sr, r, &R);
			ExtAt s = ext_at(R.o0, R.o1, R.src, has_sep, p);
			u32x4e v;
			if (ext_chunk_in_text(s, limit)) {
				v = *(g_chunkp)(tx + s.at);                  /* the whole chunk in the text of one record: any alignment */
			} else {
				uint64_t w0 = 0, w1 = 0, rr = r;
				uint32_t t = 0;
				bool fresh = true;                           /* s is the source of byte p + t */
#pragma unroll 1
				while (t < 16u && p + t < total) {
					const uint64_t pos = p + t;
					if (!fresh) {
						if (pos >= R.o1 && rr < hi) {        /* the record ended: the next one, or, behind records without bytes, */
							rr++;                            /* the last of them at or below pos */
							open_rec(oo, sr, rr, &R);
							if (R.o1 <= pos && rr < hi) {
								rr = ext_last_le(oo, rr + 1u, hi, pos);
								open_rec(oo, sr, rr, &R);
							}
						}
						s = ext_at(R.o0, R.o1, R.src, has_sep, pos);
					}
					fresh = false;
					const uint32_t cnt = s.run < 16u - t ? (uint32_t)s.run : 16u - t;   /* this record's bytes in the chunk: 1 .. 16 */
					uint64_t x0 = 0, x1 = 0;
					if (s.from == EXT_FROM_TEXT) {
						/* a window of 16 bytes whose byte t is the text byte at s.at: one load where the window lies inside the
						 * readable bytes (outside the record, inside the limit), byte loads at the two edges of the text */
						if (ext_window_ok(s.at, t, limit)) {
							const u32x4e y = *(g_chunkp)(tx + s.at - t);
							x0 = y.x | (uint64_t)y.y << 32;
							x1 = y.z | (uint64_t)y.w << 32;
						} else {
							for (uint32_t i = 0; i < cnt; i++)
								if (s.at + i < limit) put_byte(&x0, &x1, t + i, ((g_u8p)tx)[s.at + i]);
						}
					} else if (s.from == EXT_FROM_SEP) {
						put_byte(&x0, &x1, t, sep);
					}
					const uint32_t e = t + cnt;
					w0 |= x0 & low_bytes(e < 8u ? e : 8u) & ~low_bytes(t < 8u ? t : 8u);
					w1 |= x1 & low_bytes(e > 8u ? e - 8u : 0u) & ~low_bytes(t > 8u ? t - 8u : 0u);
					t = e;
					s.at += cnt;
					s.run -= cnt;
					fresh = s.run != 0u;                     /* more of the same record's text (cnt hit the chunk's end): never looped on */
				}
				v = u32x4e{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
			}
			*(g_chunkw)(ox + p) = v;                     /* the buffer is whole blocks: the last chunk is stored whole */
		}
	}
}

}   // namespace

namespace fsmhip {

/* each on stream s, the objects' device current; 0, or -1 + errno */
static int ext_launch_lengths(const ExtRun &r, hipStream_t s)
{
	if (r.m == 0 || r.nmatch == 0) return 0;
	if (!ext_grid_fits(r.nmatch)) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)((r.nmatch + EXT_MATCHES - 1u) / EXT_MATCHES)), block(EXT_THREADS);
	hipLaunchKernelGGL(ext_lengths, grid, block, 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

static int ext_launch_offsets(const ExtRun &r, hipStream_t s)
{
	if (r.m == 0 || r.nmatch == 0 || r.nrec == 0) return 0;
	if (!ext_grid_fits(r.nmatch)) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)((r.nmatch + EXT_MATCHES - 1u) / EXT_MATCHES)), block(EXT_THREADS);
	hipLaunchKernelGGL(ext_offsets, grid, block, 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

int ext_launch_write(const ExtRun &r, hipStream_t s)
{
	if (r.nrec == 0 || r.total == 0 || r.ngb == 0) return 0;
	if (r.wgs == 0 || r.wgs > 0x7fffffffu) { errno = ENOMEM; return -1; }
	const dim3 grid((unsigned)r.wgs), block(EXT_THREADS);
	hipLaunchKernelGGL(ext_write, grid, block, 0, s, r);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

}   // namespace fsmhip

/* ---- the fronts: the rule set, and the extracted text as an object of four passes (extract.h, front.h) --------------------------- */
struct __attribute__((visibility("hidden"))) fsm_hip_rules {
	int device = 0;
	size_t nrules = 0;
	unsigned flags = 0;
	DevBuf<uint32_t> d_bits;                 /* nrules bits in words of 32, never nothing */
};

extern "C" struct fsm_hip_rules *fsm_hip_rules_create(const void *bits, size_t nrules, unsigned flags)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return nullptr; }
	if ((flags & ~FSM_HIP_RULES_KEEP_OTHER) != 0u || (bits == nullptr && nrules != 0)) { errno = EINVAL; return nullptr; }
	struct fsm_hip_rules *rs = new (std::nothrow) struct fsm_hip_rules;
	if (rs == nullptr) { errno = ENOMEM; return nullptr; }
	rs->device = dev;
	rs->nrules = nrules;
	rs->flags = flags;
	std::vector<uint32_t> words((nrules + 31u) / 32u, 0u);   /* byte i >> 3, bit i & 7 = word i >> 5, bit i & 31: hosts here are little-endian */
	if (nrules != 0) memcpy(words.data(), bits, (nrules + 7u) / 8u);
	if (HIP_OK(rs->d_bits.upload(words))) return rs;
	const int e = errno;
	delete rs;
	errno = e;
	return nullptr;
}

extern "C" void fsm_hip_rules_free(struct fsm_hip_rules *rs)
{
	if (rs == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(rs->device);
		delete rs;
	}
	errno = e;
}

extern "C" size_t fsm_hip_extracted_block_matches(void) { return fsmhip::EXT_MATCHES; }
extern "C" size_t fsm_hip_extracted_block_bytes(void) { return fsmhip::EXT_BLOCK; }

extern "C" void fsm_hip_extracted_free(struct fsm_hip_extracted *x) { run_free(x); }

/* the passes on stream s into *ex, the objects' device current; r: the batch, the matches and the set (its outputs are set here) */
static int extracted_passes(struct fsm_hip_extracted *ex, fsmhip::ExtRun r, hipStream_t s)
{
	if (r.m == 0) r.nmatch = 0;
	const uint64_t nblocks = (r.nmatch + fsmhip::EXT_MATCHES - 1u) / fsmhip::EXT_MATCHES;
	uint64_t tot[2] = {0, 0};
	ex->sep = r.sep;
	if (r.nmatch != 0 && (!HIP_OK(ex->d_mrec.alloc(r.nmatch)) || !HIP_OK(ex->d_msrc.alloc(r.nmatch)) || !HIP_OK(ex->d_mline.alloc(r.nmatch)) ||
	                      !HIP_OK(ex->d_pairs.alloc(2u * nblocks + 2u))))
		return -1;
	r.mrec = ex->d_mrec;
	r.msrc = ex->d_msrc;
	r.mline = ex->d_mline;
	r.pairs = ex->d_pairs;
	if (!ex->begin(0, s)) return -1;
	if (fsmhip::ext_launch_lengths(r, s) != 0) return -1;
	if (!ex->end(0, s) || !ex->begin(1, s)) return -1;
	if (pairs_scan_launch(r.pairs, nblocks, s) != 0) return -1;
	if (!ex->end(1, s)) return -1;
	/* the ONE wait: the records size off, line and match, the bytes the text and first[] */
	if (nblocks != 0 && (!HIP_OK(hipMemcpyAsync(tot, r.pairs + 2u * nblocks, sizeof tot, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))))
		return -1;
	ex->nrec = (size_t)tot[0];
	ex->nbytes = tot[1];
	r.nrec = tot[0];
	r.total = tot[1];
	r.ngb = (r.total + fsmhip::EXT_BLOCK - 1u) / fsmhip::EXT_BLOCK;
	if (!HIP_OK(ex->d_off.alloc(r.nrec + 1u))) return -1;
	if (r.nrec != 0 && (!HIP_OK(ex->d_src.alloc(r.nrec)) || !HIP_OK(ex->d_line.alloc(r.nrec)) || !HIP_OK(ex->d_match.alloc(r.nrec)))) return -1;
	if (r.total != 0 && (!HIP_OK(ex->d_bytes.alloc(r.ngb * fsmhip::EXT_BLOCK)) || !HIP_OK(ex->d_first.alloc(r.ngb + 1u)))) return -1;
	r.out_off = ex->d_off;
	r.src = ex->d_src;
	r.line = ex->d_line;
	r.match = ex->d_match;
	r.out = ex->d_bytes;
	r.first = ex->d_first;
	const Grid g = grid_of(r.ngb, ex->device);
	r.wgs = g.wgs;
	r.per = g.per;
	if (!ex->begin(2, s)) return -1;
	if (r.nrec == 0) {                               /* no record: off[0] alone, and nothing is launched */
		if (!HIP_OK(hipMemsetAsync(ex->d_off.p, 0, sizeof(uint64_t), s))) return -1;
	} else if (fsmhip::ext_launch_offsets(r, s) != 0) {
		return -1;
	}
	if (!ex->end(2, s) || !ex->begin(3, s)) return -1;
	if (fsmhip::ext_launch_write(r, s) != 0) return -1;
	return ex->end(3, s) ? 0 : -1;
}

static struct fsm_hip_extracted *extracted_new(const struct fsm_hip_matches *mt, const struct fsm_hip_rules *keep, int sep, const fsmhip::LineBatch &in,
	hipStream_t s)
{
	fsmhip::ExtRun r;
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
	if (keep != nullptr) {
		r.keep = keep->d_bits;
		r.nrules = keep->nrules;
		r.keep_other = (keep->flags & FSM_HIP_RULES_KEEP_OTHER) != 0u;
	}
	r.sep = sep;
	return run_new<struct fsm_hip_extracted>(mt->device, in.m, fsmhip::ext_grid_fits(mt->total), s, [&](struct fsm_hip_extracted *ex) {
		return HIP_OK(hipStreamWaitEvent(s, mt->done(), 0)) ? extracted_passes(ex, r, s) : -1;   /* behind the matches' emit pass */
	});
}

/* what all three forms refuse alike about the matches, the set and the separator */
static bool extracted_args(const struct fsm_hip_matches *mt, const struct fsm_hip_rules *keep, int sep)
{
	if (!have_device()) { errno = ENODEV; return false; }
	if (mt == nullptr || (keep != nullptr && keep->device != mt->device) || sep < -1 || sep > 255) { errno = EINVAL; return false; }
	return true;
}

/* ... and the two batch forms about the batch; *in: the batch as given, which is the matches' own: it passes what theirs passed */
static bool extracted_check(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b, const struct fsm_hip_rules *keep, int sep,
	fsmhip::LineBatch *in)
{
	if (!extracted_args(mt, keep, sep)) return false;
	if (!fsmhip::batch_shape(b, FSM_HIP_MATCHES_DROP_EMPTY, in)) return false;
	if (in->m != (uint64_t)mt->m) { errno = EINVAL; return false; }
	return true;
}

extern "C" struct fsm_hip_extracted *fsm_hip_matches_extract_device(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b,
	const struct fsm_hip_rules *keep, int sep_byte, void *hip_stream)
{
	fsmhip::LineBatch in;
	if (!extracted_check(mt, b, keep, sep_byte, &in) || !fsmhip::batch_device_ok(in)) return nullptr;
	DevGuard dg(mt->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (!fsmhip::batch_read_limit(&in, s)) return nullptr;   /* as the matches: line extents are clamped to the limit */
	return extracted_new(mt, keep, sep_byte, in, s);
}

extern "C" struct fsm_hip_extracted *fsm_hip_matches_extract(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *b,
	const struct fsm_hip_rules *keep, int sep_byte)
{
	fsmhip::LineBatch host;
	if (!extracted_check(mt, b, keep, sep_byte, &host) || !fsmhip::batch_host_arrays_ok(host)) return nullptr;
	return run_host(mt->device, host, [&](const fsmhip::LineBatch &in, hipStream_t s) { return extracted_new(mt, keep, sep_byte, in, s); });
}

extern "C" struct fsm_hip_extracted *fsm_hip_text_extract(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t,
	const struct fsm_hip_text_hits *h, const struct fsm_hip_rules *keep, int sep_byte, void *hip_stream)
{
	if (!extracted_args(mt, keep, sep_byte)) return nullptr;
	if (t == nullptr || mt->m != (h != nullptr ? h->m : t->n)) { errno = EINVAL; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	std::optional<DevGuard> dg;
	fsmhip::LineBatch in;
	if (!text_batch(t, h, {mt->device}, s, &dg, &in)) return nullptr;
	return extracted_new(mt, keep, sep_byte, in, s);
}

extern "C" size_t fsm_hip_extracted_count(const struct fsm_hip_extracted *x) { return x == nullptr ? 0 : x->nrec; }
extern "C" uint64_t fsm_hip_extracted_nbytes(const struct fsm_hip_extracted *x) { return x == nullptr ? 0 : x->nbytes; }
extern "C" const uint64_t *fsm_hip_extracted_off_device(const struct fsm_hip_extracted *x) { return x == nullptr ? nullptr : x->d_off.p; }
extern "C" const unsigned char *fsm_hip_extracted_bytes_device(const struct fsm_hip_extracted *x) { return x == nullptr ? nullptr : x->d_bytes.p; }
extern "C" const uint64_t *fsm_hip_extracted_line_device(const struct fsm_hip_extracted *x) { return x == nullptr ? nullptr : x->d_line.p; }
extern "C" const uint64_t *fsm_hip_extracted_match_device(const struct fsm_hip_extracted *x) { return x == nullptr ? nullptr : x->d_match.p; }

extern "C" int fsm_hip_extracted_copy(const struct fsm_hip_extracted *x, uint64_t *off, void *bytes, uint64_t *line, uint64_t *match)
{
	if (x == nullptr) { errno = EINVAL; return -1; }
	return copy_out(x->device, x->done(), {{off, x->d_off, (x->nrec + 1u) * sizeof(uint64_t)}, {bytes, x->d_bytes, (size_t)x->nbytes},
	                                       {line, x->d_line, x->nrec * sizeof(uint64_t)}, {match, x->d_match, x->nrec * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_extracted_ms(const struct fsm_hip_extracted *x) { return run_ms(x, 0, 3); }
extern "C" double fsm_hip_extracted_pass_ms(const struct fsm_hip_extracted *x, int pass) { return run_ms(x, pass, pass); }
