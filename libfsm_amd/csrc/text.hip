/*
 * text.hip -- the text front: ONE buffer of bytes with a delimiter between records, cut into lines on the device and walked
 * in one call.
 *
 * Every other front takes inputs the caller has already cut (rows of a stride, or packed bytes with offsets / lengths); a
 * grep-like caller starts from a file.  examples/hipgrep.c cuts it on one host core, byte by byte, and memmoves every line
 * to squeeze the newlines out, because off[i] .. off[i + 1] of the untouched buffer would include the '\n'.  Here nothing is
 * squeezed or copied: the line matcher (lines.cpp) walks an automaton in which the delimiter is a self-loop of every
 * state, so [off[i], off[i + 1]) of the untouched text -- trailing delimiter included -- is an ordinary packed input of
 * fsm_hip_exec_batch_packed_all_device, and what remains is the offsets array:
 *     off[0] = 0, off[k] = position of the k-th delimiter + 1, off[n] = nbytes.
 * Three passes over a grid of workgroups that each own consecutive BLOCKs of the text:
 *     text_count    cnt[block] = delimiters in the block          (reads the text)
 *     text_scan     exclusive u64 scan of cnt[] by one workgroup; the total and "is the last byte a delimiter" for the host
 *     text_offsets  re-reads the block; rank of a hit = cnt[block] + hits before it in the block; off[1 + rank] = position + 1
 * The text is read twice.  A single-pass scan with decoupled look-back would read it once, at the price of workgroups that
 * spin on their predecessors' flags; the second read is cheap next to a hang.
 * Every global access names its address space (no FLAT instruction, as in the walk kernels: tests/test_abi.py), a lane's 16
 * bytes are loaded from the text's own first byte whatever its alignment (gfx950 takes any: tools/probes/unaligned_dma.hip), and
 * no byte outside [text, text + nbytes) is read: the last, partial block assembles its chunks from byte loads.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <optional>
#include <vector>

#include "../../include/fsm_hip.h"
#include "distinct.h"
#include "distinct_seg.h"
#include "extract.h"
#include "hip_host.h"
#include "line_batch.h"
#include "match.h"
#include "match_marks.h"
#include "replace.h"
#include "replace_seg.h"
#include "span.h"
#include "tally.h"
#include "tok.h"

namespace {

constexpr uint32_t TEXT_WAVES = 4;                          /* wavefronts per workgroup */
constexpr uint32_t TEXT_THREADS = TEXT_WAVES * 64u;
constexpr uint32_t TEXT_TILES = 4;                          /* 16-byte loads a lane keeps in flight */
constexpr uint32_t TEXT_TILE = TEXT_THREADS * 16u;          /* bytes one load instruction of the workgroup covers */
constexpr uint32_t TEXT_BLOCK = TEXT_TILES * TEXT_TILE;     /* bytes a workgroup scans per step: 16 KiB */
constexpr uint32_t TEXT_WG_PER_CU = 8;                      /* 8 x 4 wavefronts: a full CU */

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_any;       /* the text starts at any byte */
typedef const u32x4_any __attribute__((address_space(1))) *glb_chunk_p;
typedef const unsigned char __attribute__((address_space(1))) *glb_u8p;
typedef const uint64_t __attribute__((address_space(1))) *glb_u64p;
typedef uint64_t __attribute__((address_space(1))) *glb_u64w;

/* bit 7 of every byte of x that EQUALS the splat's byte, and of no other.  (x & 0x7f..) + 0x7f.. carries into bit 7 iff the low
 * seven bits are not all zero and never out of the byte; | x adds the byte's own bit 7.  The shorter (x - 0x01..) & ~x & 0x80..
 * borrows across bytes and flags a byte 0x01 above a true hit: it must not be used for counting. */
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t splat)
{
	x ^= splat;
	return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

/* bits 7, 15, 23, 31 -> bits 0 .. 3 (the partial products land on distinct bits: nothing carries) */
__device__ __forceinline__ uint32_t nibble_of(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 0xfu; }

/* bit k <=> byte k of the lane's 16 bytes is the delimiter */
__device__ __forceinline__ uint32_t hit_mask16(const u32x4 &v, uint32_t splat)
{
	return nibble_of(eq_bytes(v.x, splat)) | nibble_of(eq_bytes(v.y, splat)) << 4 | nibble_of(eq_bytes(v.z, splat)) << 8 |
	       nibble_of(eq_bytes(v.w, splat)) << 12;
}

__device__ __forceinline__ uint32_t hit_count16(const u32x4 &v, uint32_t splat)
{
	return (uint32_t)(__builtin_popcount(eq_bytes(v.x, splat)) + __builtin_popcount(eq_bytes(v.y, splat)) +
	                  __builtin_popcount(eq_bytes(v.z, splat)) + __builtin_popcount(eq_bytes(v.w, splat)));
}

/* 16 bytes of which only [addr, limit) exist (the text's last block): the others read as a byte that is not the delimiter,
 * so they never count -- also when the delimiter is 0 */
__device__ __noinline__ u32x4 load16_edge(uint64_t addr, uint64_t limit, uint32_t splat)
{
	if (addr + 16u <= limit) return *(glb_chunk_p)addr;
	uint32_t d[4] = {~splat, ~splat, ~splat, ~splat};
#pragma unroll
	for (uint32_t k = 0; k < 16u; k++) {
		if (addr + k < limit) {
			const uint32_t sh = (k & 3u) * 8u;
			d[k >> 2] = (d[k >> 2] & ~(0xffu << sh)) | (uint32_t)((glb_u8p)addr)[k] << sh;
		}
	}
	return u32x4{d[0], d[1], d[2], d[3]};
}

/* the lane's TEXT_TILES chunks of block b: chunk u = the 16 bytes at 16 * (u * TEXT_THREADS + tid) of the block, all loads
 * issued before the first use (a pure read stream: one load at a time leaves most of the memory system idle) */
__device__ __forceinline__ void load_block(u32x4 (&v)[TEXT_TILES], uint64_t text, uint64_t nbytes, uint64_t b, uint32_t splat)
{
	const uint64_t at = text + b * TEXT_BLOCK + 16u * threadIdx.x;
	if ((b + 1u) * TEXT_BLOCK <= nbytes) {   /* the same for the whole workgroup */
#pragma unroll
		for (uint32_t u = 0; u < TEXT_TILES; u++) v[u] = *(glb_chunk_p)(at + (uint64_t)u * TEXT_TILE);
	} else {
#pragma unroll
		for (uint32_t u = 0; u < TEXT_TILES; u++) v[u] = load16_edge(at + (uint64_t)u * TEXT_TILE, text + nbytes, splat);
	}
}

/* pass 1: workgroup g owns blocks [g * per, (g + 1) * per); cnt[b] = delimiters in block b.  The wave totals alternate
 * between two LDS rows, so one barrier per block is enough: a row is rewritten only after the barrier that follows its use. */
__global__ void __launch_bounds__(TEXT_THREADS)
text_count(const unsigned char *text, uint64_t nbytes, uint32_t splat, uint64_t nblocks, uint64_t per, uint64_t *cnt)
{
	__shared__ uint32_t wtot[2][TEXT_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t b = (uint64_t)blockIdx.x * per;
	const uint64_t bend = b + per < nblocks ? b + per : nblocks;
	for (uint32_t it = 0; b < bend; b++, it ^= 1u) {
		u32x4 v[TEXT_TILES];
		load_block(v, (uint64_t)(uintptr_t)text, nbytes, b, splat);
		uint32_t c = 0;
#pragma unroll
		for (uint32_t u = 0; u < TEXT_TILES; u++) c += hit_count16(v[u], splat);
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
		if (lane == 0) wtot[it][wave] = c;
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t s = 0;
#pragma unroll
			for (uint32_t w = 0; w < TEXT_WAVES; w++) s += wtot[it][w];
			*(glb_u64w)(uintptr_t)(cnt + b) = s;
		}
	}
}

/* inclusive scan of x over the wavefront: lane l leaves op over the x of lanes 0 .. l */
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T x, uint32_t lane, Op op)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const T y = __shfl_up(x, d, 64);
		if (lane >= (uint32_t)d) x = op(x, y);
	}
	return x;
}

struct op_add {
	template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

/* exclusive sum scan of rec[0, nrec), records of WORDS 64-bit words each, in place by ONE workgroup of THREADS (the shape of
 * tile_bases_pass2, walk_aux.h); meta[0 .. WORDS) = the totals.  A thread takes PER consecutive records a round, so one memory
 * round trip serves THREADS * PER records; the wave scans and an LDS exchange of the wave totals order the threads of a round, a
 * carry in LDS the rounds. */
template <uint32_t THREADS, uint32_t WORDS, uint32_t PER>
__device__ __forceinline__ void sum_scan(uint64_t *rec, uint64_t nrec, uint64_t *meta)
{
	typedef uint64_t rec_t __attribute__((ext_vector_type(WORDS)));
	typedef rec_t __attribute__((address_space(1))) *glb_rec_w;
	__shared__ uint64_t wtot[THREADS / 64u][WORDS];
	__shared__ uint64_t carry[WORDS];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0)
		for (uint32_t i = 0; i < WORDS; i++) carry[i] = 0;
	__syncthreads();
	for (uint64_t b0 = 0; b0 < nrec; b0 += (uint64_t)THREADS * PER) {
		const uint64_t b = b0 + (uint64_t)PER * threadIdx.x;
		rec_t e[PER], mine, run, x;
		uint64_t before[WORDS];
#pragma unroll
		for (uint32_t k = 0; k < PER; k++)
			e[k] = b + k < nrec ? *(glb_rec_w)(uintptr_t)(rec + WORDS * (b + k)) : (rec_t)(0u);
		mine = e[0];
#pragma unroll
		for (uint32_t k = 1; k < PER; k++) mine += e[k];
		x = mine;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {   /* the words' inclusive scans over the wave, side by side */
			rec_t y;
#pragma unroll
			for (uint32_t i = 0; i < WORDS; i++) y[i] = __shfl_up(x[i], d, 64);
			if (lane >= (uint32_t)d) x += y;
		}
		if (lane == 63u)
			for (uint32_t i = 0; i < WORDS; i++) wtot[wave][i] = x[i];
		__syncthreads();
#pragma unroll
		for (uint32_t i = 0; i < WORDS; i++) before[i] = carry[i];
		for (uint32_t w = 0; w < wave; w++)
			for (uint32_t i = 0; i < WORDS; i++) before[i] += wtot[w][i];
#pragma unroll
		for (uint32_t i = 0; i < WORDS; i++) run[i] = before[i] + x[i] - mine[i];
#pragma unroll
		for (uint32_t k = 0; k < PER; k++) {
			if (b + k < nrec) *(glb_rec_w)(uintptr_t)(rec + WORDS * (b + k)) = run;
			run += e[k];
		}
		__syncthreads();
		if (threadIdx.x == THREADS - 1u)
			for (uint32_t i = 0; i < WORDS; i++) carry[i] = before[i] + x[i];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		for (uint32_t i = 0; i < WORDS; i++) ((glb_u64w)(uintptr_t)meta)[i] = carry[i];
}

/* pass 2: the exclusive scan of cnt[]; meta[0] = the number of delimiters, meta[1] = 1 iff the text's last byte is one: the 16
 * bytes the host waits for */
__global__ void __launch_bounds__(1024)
text_scan(uint64_t *cnt, uint64_t nblocks, const unsigned char *text, uint64_t nbytes, uint32_t delim, uint64_t *meta)
{
	sum_scan<1024, 1, 1>(cnt, nblocks, meta);
	if (threadIdx.x == 0)
		((glb_u64w)(uintptr_t)meta)[1] = nbytes != 0 && ((glb_u8p)(uintptr_t)text)[nbytes - 1u] == delim ? 1u : 0u;
}

/* pass 3: off[1 + rank] = position + 1 of every delimiter.  Positions run tile by tile, lane by lane inside a tile, so the
 * rank of a lane's first hit in tile u is: base[b] (the scanned cnt) + the hits of the tiles before u + the hits of tile u in
 * the waves before this one + those of the lanes before this one.  The four tiles' counts (<= 16 a lane, <= 1024 a wave)
 * ride in 16-bit fields of two words: two wave scans, one LDS exchange and one barrier per block serve all of them.
 * A store is made only for rank < ndelim: if the caller's buffer changed between the passes the array is wrong, not overrun. */
__global__ void __launch_bounds__(TEXT_THREADS)
text_offsets(const unsigned char *text, uint64_t nbytes, uint32_t splat, uint64_t nblocks, uint64_t per, const uint64_t *base,
             uint64_t ndelim, uint64_t nlines, uint64_t *off)
{
	static_assert(TEXT_TILES == 4, "two words of two 16-bit fields");
	__shared__ uint32_t wtot[2][TEXT_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const glb_u64w out = (glb_u64w)(uintptr_t)off;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		out[0] = 0;
		if (nlines > ndelim) out[nlines] = nbytes;   /* bytes after the last delimiter: a last line without one */
	}
	uint64_t b = (uint64_t)blockIdx.x * per;
	const uint64_t bend = b + per < nblocks ? b + per : nblocks;
	for (uint32_t it = 0; b < bend; b++, it ^= 1u) {
		u32x4 v[TEXT_TILES];
		load_block(v, (uint64_t)(uintptr_t)text, nbytes, b, splat);
		const uint64_t rank0 = *(glb_u64p)(uintptr_t)(base + b);
		uint32_t m[TEXT_TILES], c[TEXT_TILES];
#pragma unroll
		for (uint32_t u = 0; u < TEXT_TILES; u++) {
			m[u] = hit_mask16(v[u], splat);
			c[u] = (uint32_t)__builtin_popcount(m[u]);
		}
		uint32_t x0 = c[0] | c[1] << 16, x1 = c[2] | c[3] << 16;   /* inclusive scans over the wave, the two interleaved */
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t y0 = (uint32_t)__shfl_up((int)x0, d, 64), y1 = (uint32_t)__shfl_up((int)x1, d, 64);
			if (lane >= (uint32_t)d) { x0 += y0; x1 += y1; }
		}
		if (lane == 63u) { wtot[it][wave][0] = x0; wtot[it][wave][1] = x1; }
		__syncthreads();
		uint32_t tot[TEXT_TILES] = {0u, 0u, 0u, 0u}, before[TEXT_TILES] = {0u, 0u, 0u, 0u};
#pragma unroll
		for (uint32_t w = 0; w < TEXT_WAVES; w++) {
			const uint32_t t0 = wtot[it][w][0], t1 = wtot[it][w][1];
			const uint32_t f[TEXT_TILES] = {t0 & 0xffffu, t0 >> 16, t1 & 0xffffu, t1 >> 16};
#pragma unroll
			for (uint32_t u = 0; u < TEXT_TILES; u++) {
				tot[u] += f[u];
				before[u] += w < wave ? f[u] : 0u;
			}
		}
		const uint32_t incl[TEXT_TILES] = {x0 & 0xffffu, x0 >> 16, x1 & 0xffffu, x1 >> 16};
		uint64_t tile_rank = rank0;
		const uint64_t pos1 = b * TEXT_BLOCK + 16u * threadIdx.x + 1u;
#pragma unroll
		for (uint32_t u = 0; u < TEXT_TILES; u++) {
			uint64_t r = tile_rank + before[u] + (incl[u] - c[u]);
			for (uint32_t mm = m[u]; mm != 0; mm &= mm - 1u, r++)
				if (r < ndelim) out[1u + r] = pos1 + (uint64_t)u * TEXT_TILE + (uint32_t)__builtin_ctz(mm);
			tile_rank += tot[u];
		}
	}
}

bool have_device()
{
	int ndev = 0;
	return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

unsigned max_workgroups(int dev)
{
	int ncu = 0;
	if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
	return (unsigned)ncu * TEXT_WG_PER_CU;
}

/* the grid for nblocks blocks: at most max_workgroups workgroups of `per` consecutive blocks each, none without a block (one
 * workgroup for no block: the kernels that run then do their first thread's work alone) */
struct Grid {
	uint64_t wgs = 1, per = 1;
};
Grid grid_of(uint64_t nblocks, int dev)
{
	Grid g;
	if (nblocks == 0) return g;
	g.wgs = max_workgroups(dev);
	if (g.wgs > nblocks) g.wgs = nblocks;
	g.per = (nblocks + g.wgs - 1u) / g.wgs;
	g.wgs = (nblocks + g.per - 1u) / g.per;
	return g;
}

/* wait for `done`, then copy every {dst, src, nbytes} with a dst and bytes out of the device */
struct OutCopy {
	void *dst;
	const void *src;
	size_t nbytes;
};
int copy_out(int device, hipEvent_t done, std::initializer_list<OutCopy> copies)
{
	DevGuard dg(device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (!HIP_OK(hipEventSynchronize(done))) return -1;
	for (const OutCopy &c : copies)
		if (c.dst != nullptr && c.nbytes != 0 && !HIP_OK(hipMemcpy(c.dst, c.src, c.nbytes, hipMemcpyDeviceToHost))) return -1;
	return 0;
}

/* wait for `done`, then the milliseconds between the events of every pair, summed; -1 when it fails */
struct EventPair {
	hipEvent_t from, to;
};
double elapsed_ms(int device, hipEvent_t done, const EventPair *pairs, size_t npairs)
{
	double ms = 0.0;
	DevGuard dg(device);
	if (!dg.ok()) { errno = ENODEV; return -1.0; }
	if (!HIP_OK(hipEventSynchronize(done))) return -1.0;
	for (size_t k = 0; k < npairs; k++) {
		float one = 0.f;
		if (!HIP_OK(hipEventElapsedTime(&one, pairs[k].from, pairs[k].to))) return -1.0;
		ms += (double)one;
	}
	return ms;
}
double elapsed_ms(int device, hipEvent_t done, std::initializer_list<EventPair> pairs) { return elapsed_ms(device, done, pairs.begin(), pairs.size()); }

}   // namespace

/* the types are the library's own: their destructors are no exported symbols */
struct __attribute__((visibility("hidden"))) fsm_hip_text {
	int device = 0, delim = 0;
	size_t nbytes = 0, n = 0;
	const unsigned char *d_text = nullptr;   /* the caller's bytes (open_device) or `owned` */
	DevBuf<unsigned char> owned;
	DevBuf<uint64_t> d_off;                  /* n + 1 */
	DevBuf<uint64_t> d_cnt;                  /* per block: its delimiters, then their exclusive scan; + the 2 (files: 4) words of meta */
	DevEvent ev[4];                          /* around count + scan, around offsets; ev[3]: the offsets are there */
	/* a text of files (fsm_hip_text_open_files*): all NULL / 0 in a plain text */
	size_t nfiles = 0;
	const uint64_t *d_file_off = nullptr;    /* nfiles + 1: the caller's (open_files_device) or `owned_file_off` */
	DevBuf<uint64_t> owned_file_off;
	DevBuf<uint64_t> d_file_lines;           /* nfiles + 1 */
	DevBuf<uint64_t> d_plain;                /* the plain offsets the merge reads; the host form frees them once its stream is idle */
	DevBuf<uint64_t> d_frank;                /* per file end: (added ends before it in its block) << 1 | it adds one */
	DevBuf<uint64_t> d_fpairs;               /* per block of file ends: (added ends, invalid entries), then their exclusive scan */
	DevEvent fev[3];                         /* around mark + scan; fev[2]: the plain offsets are there, the merge runs to ev[3] */
	DevStream own;                           /* the host-pointer forms run here, never on the NULL stream (last: it goes first) */
};

extern "C" void fsm_hip_text_free(struct fsm_hip_text *t)
{
	if (t == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(t->device);
		if (t->ev[3] != nullptr) (void)hipEventSynchronize(t->ev[3]);   /* the scan may still be reading the caller's bytes */
		delete t;
	}
	errno = e;
}

extern "C" size_t fsm_hip_text_lines(const struct fsm_hip_text *t) { return t == nullptr ? 0 : t->n; }

extern "C" const uint64_t *fsm_hip_text_offsets_device(const struct fsm_hip_text *t) { return t == nullptr ? nullptr : t->d_off.p; }

extern "C" int fsm_hip_text_offsets(const struct fsm_hip_text *t, uint64_t *off)
{
	if (t == nullptr || off == nullptr) { errno = EINVAL; return -1; }
	return copy_out(t->device, t->ev[3], {{off, t->d_off, (t->n + 1u) * sizeof(uint64_t)}});
}

extern "C" size_t fsm_hip_text_block_bytes(void) { return TEXT_BLOCK; }

extern "C" size_t fsm_hip_text_max_workgroups(void)
{
	int dev = 0;
	if (!have_device() || hipGetDevice(&dev) != hipSuccess) { errno = ENODEV; return 0; }
	return max_workgroups(dev);
}

extern "C" double fsm_hip_text_scan_ms(const struct fsm_hip_text *t)
{
	if (t == nullptr) { errno = EINVAL; return -1.0; }
	/* files: the merge after the plain offsets is not the scan's */
	return elapsed_ms(t->device, t->ev[3], {{t->ev[0], t->ev[1]}, {t->ev[2], t->nfiles != 0 ? t->fev[2] : t->ev[3]}});
}

/* ---- the walk: the untouched text + its offsets are a packed batch of the twin automaton ---- */

static int text_exec_check(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t)
{
	struct fsm_hip_dfa_info info;
	if (ld == nullptr || t == nullptr || fsm_hip_lines_dfa_delim(ld) != t->delim) { errno = EINVAL; return -1; }
	if (fsm_hip_dfa_info(fsm_hip_lines_dfa_inner(ld), &info) != 0) return -1;
	if ((int)info.device != t->device) { errno = EINVAL; return -1; }   /* the text lives where it was opened */
	return 0;
}

extern "C" int fsm_hip_text_exec_device(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream)
{
	if (text_exec_check(ld, t) != 0) return -1;
	if (t->n == 0) return 0;
	return fsm_hip_exec_batch_packed_all_device(fsm_hip_lines_dfa_inner(ld), t->d_text, FSM_HIP_META_OFF64, t->d_off, t->n,
	                                            d_end_out, d_accept_bitmap, ids_mode, d_id_out, d_eager_out, hip_stream);
}

extern "C" int fsm_hip_text_exec(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t,
	uint32_t *end_out, uint64_t *accept_bitmap, int ids_mode, uint32_t *id_out, uint64_t *eager_out)
{
	if (text_exec_check(ld, t) != 0) return -1;
	const size_t n = t->n;
	if (n == 0) return 0;
	if (end_out == nullptr && accept_bitmap == nullptr && id_out == nullptr && eager_out == nullptr) return 0;
	DevGuard dg(t->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	const size_t W = fsm_hip_eager_words(fsm_hip_lines_dfa_inner(ld));
	/* the outputs that are asked for, staged one after the other in one allocation, each at a multiple of 16 bytes */
	auto up16 = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
	const size_t n_end = n * 4u, n_bm = (n + 63u) / 64u * 8u, n_id = n * 4u, n_eo = n * W * 8u;
	const size_t at_bm = end_out ? up16(n_end) : 0, at_id = at_bm + (accept_bitmap ? up16(n_bm) : 0), at_eo = at_id + (id_out ? up16(n_id) : 0);
	DevBuf<unsigned char> d;
	if (!HIP_OK(d.alloc(at_eo + (eager_out ? up16(n_eo) : 0)))) return -1;
	uint32_t *d_end = end_out ? (uint32_t *)d.p : nullptr, *d_id = id_out ? (uint32_t *)(d + at_id) : nullptr;
	uint64_t *d_bm = accept_bitmap ? (uint64_t *)(d + at_bm) : nullptr, *d_eo = eager_out ? (uint64_t *)(d + at_eo) : nullptr;
	auto fail = [&] {   /* the stream idle before the staging memory goes */
		const int e = errno;
		(void)hipStreamSynchronize(t->own);
		errno = e;
		return -1;
	};
	if (!HIP_OK(hipStreamWaitEvent(t->own, t->ev[3], 0))) return fail();   /* a text opened on the caller's stream: its offsets first */
	if (fsm_hip_text_exec_device(ld, t, d_end, d_bm, ids_mode, d_id, d_eo, t->own) != 0) return fail();
	if (end_out && !HIP_OK(hipMemcpyAsync(end_out, d_end, n_end, hipMemcpyDeviceToHost, t->own))) return fail();
	if (accept_bitmap && !HIP_OK(hipMemcpyAsync(accept_bitmap, d_bm, n_bm, hipMemcpyDeviceToHost, t->own))) return fail();
	if (id_out && !HIP_OK(hipMemcpyAsync(id_out, d_id, n_id, hipMemcpyDeviceToHost, t->own))) return fail();
	if (eager_out && !HIP_OK(hipMemcpyAsync(eager_out, d_eo, n_eo, hipMemcpyDeviceToHost, t->own))) return fail();
	if (!HIP_OK(hipStreamSynchronize(t->own))) return fail();
	return 0;
}

/* ---- the hits: the selected lines' numbers, ranges and bytes ----------------------------------------------------
 * A caller like grep does not want n answers, it wants the lines that matched.  A bitmap (bit i = line i, the layout the walk
 * writes) and the offsets become: m line numbers, m + 1 output offsets and the lines' bytes, packed.  A select in three
 * passes, shaped as the delimiter scan is, and a gather that partitions the OUTPUT:
 *     hits_count   pair[block] = (lines selected, their bytes) of a block of HITS_LINES lines    (reads bitmap and offsets)
 *     hits_scan    exclusive scan of the pairs by one workgroup, HITS_SCAN_PER pairs a thread and round; m and the bytes for the host
 *     hits_emit    re-reads the block; lines[rank] = i, out_off[rank], src[rank] = off[i]; the line whose output range covers
 *                  byte g * HITS_BLOCK leaves first[g] = rank (ranges are non-empty and tile the output: exactly one does)
 *     hits_gather  a workgroup owns blocks of HITS_BLOCK output bytes, a lane 16-byte chunks: the line of the chunk's first byte
 *                  by an upper-bound search of out_off between first[g] and first[g + 1]; a chunk inside one line is one
 *                  unaligned 16-byte load, a chunk across boundaries is assembled from byte loads line by line
 * No line belongs to a lane or a wavefront: a 64 MiB line is 4 096 output blocks like any other 64 MiB.  No workgroup waits on
 * another.  Stores are made only below the counted totals and loads only inside [text, text + nbytes): a bitmap that changes
 * between the passes gives wrong arrays, not an overrun. */
namespace {

constexpr uint32_t HITS_WAVES = 4;
constexpr uint32_t HITS_THREADS = HITS_WAVES * 64u;
constexpr uint32_t HITS_PER = 4;                            /* consecutive lines a lane tests: never across a bitmap word */
constexpr uint32_t HITS_LINES = HITS_THREADS * HITS_PER;    /* lines a workgroup selects per step: 1 024 */
constexpr uint32_t HITS_TILES = 4;
constexpr uint32_t HITS_TILE = HITS_THREADS * 16u;          /* output bytes one store instruction of the workgroup covers */
constexpr uint32_t HITS_BLOCK = HITS_TILES * HITS_TILE;     /* output bytes a workgroup gathers per step: 16 KiB */
constexpr uint32_t HITS_SCAN_PER = 4;                       /* pairs a thread of the scan takes per round: 4 096 a round */

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef const u64x2 __attribute__((address_space(1))) *glb_u64x2p;
typedef u64x2 __attribute__((address_space(1))) *glb_u64x2w;
typedef u32x4 __attribute__((address_space(1))) *glb_chunk_w;

/* the lane's HITS_PER lines from i0 (a multiple of HITS_PER): bit j <=> line i0 + j < n is selected; o[j], o[j + 1] its range */
__device__ __forceinline__ uint32_t lane_lines(uint64_t bitmap, uint64_t off, uint64_t n, uint64_t i0, uint32_t invert, uint64_t (&o)[HITS_PER + 1])
{
	static_assert(HITS_PER == 4, "two 16-byte loads and one word");
#pragma unroll
	for (uint32_t j = 0; j <= HITS_PER; j++) o[j] = 0;
	if (i0 >= n) return 0u;
	const uint64_t w = ((glb_u64p)bitmap)[i0 >> 6];
	uint32_t sel = (uint32_t)((invert != 0u ? ~w : w) >> (i0 & 63u)) & 0xfu;
	if (i0 + HITS_PER <= n) {
		const glb_u64x2p p = (glb_u64x2p)(off + 8u * i0);   /* 32-byte aligned: the offsets are the text's own allocation */
		const u64x2 a = p[0], b = p[1];
		o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
		o[4] = ((glb_u64p)off)[i0 + 4u];
	} else {
		sel &= (1u << (uint32_t)(n - i0)) - 1u;              /* bits at and above n are no lines, whatever they hold */
#pragma unroll
		for (uint32_t j = 0; j <= HITS_PER; j++)
			if (i0 + j <= n) o[j] = ((glb_u64p)off)[i0 + j];
	}
	return sel;
}

/* the bytes of the lane's selected lines */
__device__ __forceinline__ uint64_t lane_bytes(uint32_t sel, const uint64_t (&o)[HITS_PER + 1])
{
	uint64_t by = 0;
#pragma unroll
	for (uint32_t j = 0; j < HITS_PER; j++) by += (sel >> j & 1u) != 0u ? o[j + 1u] - o[j] : 0u;
	return by;
}

/* the first index in a[0, n) whose entry is >= v (n if none) */
__device__ __forceinline__ uint64_t lower_bound_glb(glb_u64p a, uint64_t n, uint64_t v)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2u;
		if (a[mid] < v) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

/* pass 1: workgroup g owns blocks [g * per, (g + 1) * per) of HITS_LINES lines; pairs[2b], pairs[2b + 1] = lines and bytes
 * selected in block b.  Two LDS rows in turn, one barrier a block, as text_count. */
__global__ void __launch_bounds__(HITS_THREADS)
hits_count(const uint64_t *bitmap, const uint64_t *off, uint64_t n, uint32_t invert, uint64_t nblocks, uint64_t per, uint64_t *pairs)
{
	__shared__ uint64_t wtot[2][HITS_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t b = (uint64_t)blockIdx.x * per;
	const uint64_t bend = b + per < nblocks ? b + per : nblocks;
	for (uint32_t it = 0; b < bend; b++, it ^= 1u) {
		uint64_t o[HITS_PER + 1];
		const uint32_t sel = lane_lines((uint64_t)(uintptr_t)bitmap, (uint64_t)(uintptr_t)off, n, b * HITS_LINES + HITS_PER * threadIdx.x, invert, o);
		uint32_t c = (uint32_t)__builtin_popcount(sel);
		uint64_t by = lane_bytes(sel, o);
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			c += (uint32_t)__shfl_xor((int)c, d, 64);
			by += __shfl_xor(by, d, 64);
		}
		if (lane == 0) { wtot[it][wave][0] = c; wtot[it][wave][1] = by; }
		__syncthreads();
		if (threadIdx.x == 0) {
			uint64_t sc = 0, sb = 0;
#pragma unroll
			for (uint32_t w = 0; w < HITS_WAVES; w++) { sc += wtot[it][w][0]; sb += wtot[it][w][1]; }
			*(glb_u64x2w)(uintptr_t)(pairs + 2u * b) = u64x2{sc, sb};
		}
	}
}

/* pass 2: the exclusive scan of the pairs; meta[0] = m, meta[1] = the bytes of the m lines.  HITS_SCAN_PER consecutive pairs a
 * thread: one memory round trip serves 4 096 blocks (4 Mi lines). */
__global__ void __launch_bounds__(1024)
hits_scan(uint64_t *pairs, uint64_t nblocks, uint64_t *meta)
{
	sum_scan<1024, 2, HITS_SCAN_PER>(pairs, nblocks, meta);
}

/* pass 3: the rank of a selected line = base[block] + the selected lines of the waves and lanes before it (a wave scan and an
 * LDS exchange); the bytes before it likewise.  out_off == NULL (NO_BYTES): the numbers alone.  ngb = output blocks. */
__global__ void __launch_bounds__(HITS_THREADS)
hits_emit(const uint64_t *bitmap, const uint64_t *off, uint64_t n, uint32_t invert, uint64_t nblocks, uint64_t per, const uint64_t *base,
          uint64_t m, uint64_t total, uint64_t *lines, uint64_t *out_off, uint64_t *src, uint64_t *first, uint64_t ngb)
{
	__shared__ uint64_t wtot[2][HITS_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const glb_u64w ln = (glb_u64w)(uintptr_t)lines, oo = (glb_u64w)(uintptr_t)out_off, sr = (glb_u64w)(uintptr_t)src,
	               fi = (glb_u64w)(uintptr_t)first;
	const bool bytes = out_off != nullptr;
	if (blockIdx.x == 0 && threadIdx.x == 0 && bytes) {
		oo[m] = total;
		if (first != nullptr) fi[ngb] = m;   /* the search's upper end in the last block */
	}
	uint64_t b = (uint64_t)blockIdx.x * per;
	const uint64_t bend = b + per < nblocks ? b + per : nblocks;
	for (uint32_t it = 0; b < bend; b++, it ^= 1u) {
		uint64_t o[HITS_PER + 1];
		const uint64_t i0 = b * HITS_LINES + HITS_PER * threadIdx.x;
		const uint32_t sel = lane_lines((uint64_t)(uintptr_t)bitmap, (uint64_t)(uintptr_t)off, n, i0, invert, o);
		const u64x2 bs = *(glb_u64x2p)(uintptr_t)(base + 2u * b);
		const uint32_t c = (uint32_t)__builtin_popcount(sel);
		const uint64_t by = lane_bytes(sel, o);
		const uint32_t xc = wave_scan(c, lane, op_add());
		const uint64_t xb = wave_scan(by, lane, op_add());
		if (lane == 63u) { wtot[it][wave][0] = xc; wtot[it][wave][1] = xb; }
		__syncthreads();
		uint64_t r = bs.x + (xc - c), p = bs.y + (xb - by);
#pragma unroll
		for (uint32_t w = 0; w < HITS_WAVES; w++) {
			r += w < wave ? wtot[it][w][0] : 0u;
			p += w < wave ? wtot[it][w][1] : 0u;
		}
#pragma unroll
		for (uint32_t j = 0; j < HITS_PER; j++) {
			if ((sel >> j & 1u) == 0u) continue;
			const uint64_t len = o[j + 1u] - o[j];
			if (r < m) {
				ln[r] = i0 + j;
				if (bytes) {
					oo[r] = p;
					sr[r] = o[j];
					/* the block boundaries inside [p, p + len): one for most lines that have any, many for a long line */
					for (uint64_t g = (p + HITS_BLOCK - 1u) / HITS_BLOCK; g < ngb && g * HITS_BLOCK < p + len; g++) fi[g] = r;
				}
			}
			r++;
			p += len;
		}
	}
}

/* the gather: workgroup w owns output blocks [w * per, (w + 1) * per).  The lane's chunk starts at output byte p; its line is
 * the last k in [first[g], first[g + 1]] with out_off[k] <= p.  Everything read through a rank is clamped below m and every
 * text byte is tested against nbytes, so arrays gone wrong (a bitmap that changed) cannot send a load outside. */
__global__ void __launch_bounds__(HITS_THREADS)
hits_gather(const unsigned char *text, uint64_t nbytes, const uint64_t *out_off, const uint64_t *src, const uint64_t *first,
            uint64_t m, uint64_t total, uint64_t ngb, uint64_t per, unsigned char *out)
{
	const glb_u64p oo = (glb_u64p)(uintptr_t)out_off, sr = (glb_u64p)(uintptr_t)src, fi = (glb_u64p)(uintptr_t)first;
	const uint64_t tx = (uint64_t)(uintptr_t)text, ox = (uint64_t)(uintptr_t)out;
	uint64_t g = (uint64_t)blockIdx.x * per;
	const uint64_t gend = g + per < ngb ? g + per : ngb;
	for (; g < gend; g++) {
		uint64_t k = fi[g], hi = fi[g + 1u];
		if (k > m - 1u) k = m - 1u;
		if (hi > m - 1u) hi = m - 1u;
#pragma unroll 1
		for (uint32_t u = 0; u < HITS_TILES; u++) {
			const uint64_t p = g * HITS_BLOCK + (uint64_t)u * HITS_TILE + 16u * threadIdx.x;
			if (p >= total) break;
			uint64_t z = hi;
			while (k < z) {                                   /* upper bound; the tiles of a lane ascend, so k only grows */
				const uint64_t mid = k + (z - k + 1u) / 2u;
				if (oo[mid] <= p) k = mid; else z = mid - 1u;
			}
			uint64_t end = oo[k + 1u];
			uint64_t delta = sr[k] - oo[k];                   /* text position = output position + delta, inside line k */
			u32x4 v;
			if (end >= p + 16u && nbytes >= 16u && p + delta <= nbytes - 16u) {
				v = *(glb_chunk_p)(tx + p + delta);           /* the whole chunk inside one line: any alignment */
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				uint64_t kk = k;
#pragma unroll
				for (uint32_t j = 0; j < 16u; j++) {
					const uint64_t pos = p + j;
					if (pos < total) {
						if (pos >= end && kk + 1u < m) {          /* lines are non-empty: one step reaches the byte's line */
							kk++;
							end = oo[kk + 1u];
							delta = sr[kk] - oo[kk];
						}
						const uint64_t s = pos + delta;
						if (s < nbytes) d[j >> 2] |= (uint32_t)((glb_u8p)tx)[s] << ((j & 3u) * 8u);
					}
				}
				v = u32x4{d[0], d[1], d[2], d[3]};
			}
			*(glb_chunk_w)(ox + p) = v;                       /* the buffer is whole blocks: the last chunk is stored whole */
		}
	}
}

/* the hits of a text of files: one lane per file end, file_first[j] = the selected lines with index below file_lines[j], a
 * lower-bound search in the ascending lines[0, m).  m == 0: every entry is 0 and lines (NULL then) is never read. */
__global__ void __launch_bounds__(HITS_THREADS)
hits_file_first(const uint64_t *lines, uint64_t m, const uint64_t *file_lines, uint64_t nends, uint64_t *file_first)
{
	const uint64_t j = (uint64_t)blockIdx.x * HITS_THREADS + threadIdx.x;
	if (j >= nends) return;
	const uint64_t v = ((glb_u64p)(uintptr_t)file_lines)[j];
	((glb_u64w)(uintptr_t)file_first)[j] = lower_bound_glb((glb_u64p)(uintptr_t)lines, m, v);
}

}   // namespace

/* ---- context: the lines within reach of a selected line of the same file (grep -A / -B / -C) -------------------------
 * S = the selected lines (bitmap ^ invert, below n), F = the lines that begin a file after the first (none in a plain text).
 * W[i] <=> some selected p of i's file has p - before <= i <= p + after; the hits of W are made by the five kernels above,
 * unchanged.  The nearest selected line on either side is the best witness, so with
 *     prevS(i) / nextS(i) = the last / first selected line <= i / >= i,   prevF(i) = the last file start <= i (0 if none),
 *     nextF(i) = the first file start > i (n if none)
 * W[i] <=> (prevS exists, i - prevS <= after, prevF(i) <= prevS) or (nextS exists, nextS - i <= before, nextS < nextF(i)):
 * arithmetic on two bitmaps whose cost does not know before or after.  A lane owns a WORD of 64 lines, CTX_TEAM lanes a block
 * of HITS_LINES lines.  The passes:
 *     ctx_file_starts  one lane per entry of file_lines: a bit of F for every distinct value in (0, n)       (vector atomic or)
 *     ctx_summary      per block: (last selected + 1, last file start; first selected, first file start); the selected lines
 *                      are counted on the way (core_count)
 *     ctx_scan         one workgroup: exclusive max-scan forward of the first pair, exclusive min-scan backward of the second,
 *                      CTX_SCAN_THREADS blocks a round from either end, a carry from round to round
 *     ctx_apply        re-reads the words; the team's exclusive scans continue the block's carries to every word; a word is
 *                      the union of what reaches it from the nearest selected line on its left, on its right, and from its
 *                      own selected lines, each cut at the file starts: masks, no loop over before or after
 *     ctx_marks        after hits_emit, one lane per hit: core = S[lines[k]], group = "a -- goes before it"; whole words by ballot
 * Distances are compared, never positions added: before = after = 2^64 - 1 cannot wrap.  No workgroup waits for another; every
 * workgroup of summary / apply takes ONE step of CTX_WG_BLOCKS blocks and carries nothing.  Loads stay below ceil(n / 64) words
 * and stores below the counted totals, whatever the bitmap or lines hold. */
namespace {

constexpr uint32_t CTX_TEAM = HITS_LINES / 64u;             /* lanes (words) of a block: 16, a team never straddles a wavefront */
constexpr uint32_t CTX_THREADS = 256;
constexpr uint32_t CTX_WG_BLOCKS = CTX_THREADS / CTX_TEAM;  /* blocks a workgroup of summary / apply takes */
constexpr uint32_t CTX_SCAN_THREADS = 1024;                 /* blocks a round of ctx_scan takes from either end */
constexpr uint64_t CTX_NONE = ~(uint64_t)0;
static_assert(CTX_TEAM == 16 && 64u % CTX_TEAM == 0, "a team is a quarter of a wavefront");

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
/* bits lo .. hi of a word, 0 <= lo <= hi <= 63 */
__device__ __forceinline__ uint64_t bits_between(uint32_t lo, uint32_t hi) { return (~(uint64_t)0 >> (63u - hi)) & (~(uint64_t)0 << lo); }

/* word wi of S and of F (0 beyond the last word; the bits at and above n are no lines) */
__device__ __forceinline__ void ctx_words(uint64_t bitmap, uint64_t fmap, uint64_t n, uint64_t nwords, uint32_t invert, uint64_t wi,
                                          uint64_t &w, uint64_t &f)
{
	w = 0;
	f = 0;
	if (wi >= nwords) return;
	const uint64_t live = n - 64u * wi >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << (uint32_t)(n - 64u * wi)) - 1u;
	const uint64_t x = ((glb_u64p)bitmap)[wi];
	w = (invert != 0u ? ~x : x) & live;
	if (fmap != 0) f = ((glb_u64p)fmap)[wi] & live;
}

/* the word's own summary: s[0] = last selected + 1 (0: none), s[1] = last file start (0: none), s[2] = first selected (NONE),
 * s[3] = first file start (n: none) */
__device__ __forceinline__ void ctx_own(uint64_t w, uint64_t f, uint64_t base, uint64_t n, uint64_t (&s)[4])
{
	s[0] = w != 0 ? base + (63u - (uint32_t)__builtin_clzll(w)) + 1u : 0u;
	s[1] = f != 0 ? base + (63u - (uint32_t)__builtin_clzll(f)) : 0u;
	s[2] = w != 0 ? base + (uint32_t)__builtin_ctzll(w) : CTX_NONE;
	s[3] = f != 0 ? base + (uint32_t)__builtin_ctzll(f) : n;
}

__global__ void __launch_bounds__(CTX_THREADS)
ctx_file_starts(const uint64_t *file_lines, uint64_t nends, uint64_t n, uint64_t *fmap)
{
	const uint64_t j = (uint64_t)blockIdx.x * CTX_THREADS + threadIdx.x;
	if (j >= nends) return;
	const glb_u64p fl = (glb_u64p)(uintptr_t)file_lines;
	const uint64_t v = fl[j];
	if (v == 0 || v >= n || (j != 0 && fl[j - 1u] == v)) return;   /* the first of a run sets the bit; line 0 and n begin no later file */
	(void)__hip_atomic_fetch_or((glb_u64w)(uintptr_t)(fmap + (v >> 6)), (uint64_t)1 << (uint32_t)(v & 63u), __ATOMIC_RELAXED,
	                            __HIP_MEMORY_SCOPE_AGENT);
}

/* sum[4b .. 4b + 3] = the summary of block b; meta[0] += the selected lines */
__global__ void __launch_bounds__(CTX_THREADS)
ctx_summary(const uint64_t *bitmap, const uint64_t *fmap, uint64_t n, uint64_t nwords, uint32_t invert, uint64_t nblocks, uint64_t *sum,
            uint64_t *meta)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t wi = (uint64_t)blockIdx.x * CTX_THREADS + threadIdx.x;
	uint64_t w, f, s[4];
	ctx_words((uint64_t)(uintptr_t)bitmap, (uint64_t)(uintptr_t)fmap, n, nwords, invert, wi, w, f);
	ctx_own(w, f, 64u * wi, n, s);
#pragma unroll
	for (int d = 1; d < (int)CTX_TEAM; d <<= 1) {
		s[0] = umax64(s[0], __shfl_xor(s[0], d, (int)CTX_TEAM));
		s[1] = umax64(s[1], __shfl_xor(s[1], d, (int)CTX_TEAM));
		s[2] = umin64(s[2], __shfl_xor(s[2], d, (int)CTX_TEAM));
		s[3] = umin64(s[3], __shfl_xor(s[3], d, (int)CTX_TEAM));
	}
	const uint64_t b = wi / CTX_TEAM;
	if ((lane & (CTX_TEAM - 1u)) == 0u && b < nblocks) {
		const glb_u64x2w out = (glb_u64x2w)(uintptr_t)(sum + 4u * b);
		out[0] = u64x2{s[0], s[1]};
		out[1] = u64x2{s[2], s[3]};
	}
	uint32_t c = (uint32_t)__builtin_popcountll(w);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
	if (lane == 0 && c != 0u)
		(void)__hip_atomic_fetch_add((glb_u64w)(uintptr_t)meta, (uint64_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* in place: sum[4b], sum[4b + 1] become the max over the blocks BEFORE b, sum[4b + 2], sum[4b + 3] the min over the blocks AFTER b.
 * Thread k of a round takes block b0 + k for the forward pair and block nblocks - 1 - (b0 + k) for the backward pair: one loop,
 * one carry of four words, the two directions never touch the same word. */
__global__ void __launch_bounds__(CTX_SCAN_THREADS)
ctx_scan(uint64_t *sum, uint64_t nblocks, uint64_t n)
{
	__shared__ uint64_t wtot[CTX_SCAN_THREADS / 64u][4];
	__shared__ uint64_t carry[4];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (threadIdx.x == 0) { carry[0] = 0; carry[1] = 0; carry[2] = CTX_NONE; carry[3] = n; }
	__syncthreads();
	for (uint64_t b0 = 0; b0 < nblocks; b0 += CTX_SCAN_THREADS) {
		const uint64_t k = b0 + threadIdx.x;
		const bool act = k < nblocks;
		const glb_u64x2w fw = (glb_u64x2w)(uintptr_t)(sum + 4u * (act ? k : 0u));
		const glb_u64x2w bw = (glb_u64x2w)(uintptr_t)(sum + 4u * (act ? nblocks - 1u - k : 0u) + 2u);
		const u64x2 mf = act ? *fw : u64x2{0u, 0u}, mb = act ? *bw : u64x2{CTX_NONE, n};
		uint64_t x0 = mf.x, x1 = mf.y, x2 = mb.x, x3 = mb.y;   /* inclusive over the wave, the four side by side */
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint64_t y0 = __shfl_up(x0, d, 64), y1 = __shfl_up(x1, d, 64), y2 = __shfl_up(x2, d, 64), y3 = __shfl_up(x3, d, 64);
			if (lane >= (uint32_t)d) { x0 = umax64(x0, y0); x1 = umax64(x1, y1); x2 = umin64(x2, y2); x3 = umin64(x3, y3); }
		}
		if (lane == 63u) { wtot[wave][0] = x0; wtot[wave][1] = x1; wtot[wave][2] = x2; wtot[wave][3] = x3; }
		__syncthreads();
		uint64_t c0 = carry[0], c1 = carry[1], c2 = carry[2], c3 = carry[3];
		for (uint32_t w = 0; w < wave; w++) {
			c0 = umax64(c0, wtot[w][0]); c1 = umax64(c1, wtot[w][1]); c2 = umin64(c2, wtot[w][2]); c3 = umin64(c3, wtot[w][3]);
		}
		/* exclusive: the lanes before this one */
		const uint64_t p0 = __shfl_up(x0, 1, 64), p1 = __shfl_up(x1, 1, 64), p2 = __shfl_up(x2, 1, 64), p3 = __shfl_up(x3, 1, 64);
		if (act) {
			*fw = lane == 0 ? u64x2{c0, c1} : u64x2{umax64(c0, p0), umax64(c1, p1)};
			*bw = lane == 0 ? u64x2{c2, c3} : u64x2{umin64(c2, p2), umin64(c3, p3)};
		}
		__syncthreads();
		if (threadIdx.x == CTX_SCAN_THREADS - 1u) {
			carry[0] = umax64(c0, x0); carry[1] = umax64(c1, x1); carry[2] = umin64(c2, x2); carry[3] = umin64(c3, x3);
		}
		__syncthreads();
	}
}

/* out[wi] = word wi of W.  ps1 / pf: the last selected line + 1 / the last file start before the word (0: none); ns / nf: the
 * first selected line / file start after it (NONE / n): the block's carries continued through the team. */
__global__ void __launch_bounds__(CTX_THREADS)
ctx_apply(const uint64_t *bitmap, const uint64_t *fmap, uint64_t n, uint64_t nwords, uint32_t invert, const uint64_t *sum, uint64_t before,
          uint64_t after, uint64_t *out)
{
	const uint32_t sub = threadIdx.x & (CTX_TEAM - 1u);
	const uint64_t wi = (uint64_t)blockIdx.x * CTX_THREADS + threadIdx.x, base = 64u * wi;
	uint64_t w, f, s[4];
	ctx_words((uint64_t)(uintptr_t)bitmap, (uint64_t)(uintptr_t)fmap, n, nwords, invert, wi, w, f);
	ctx_own(w, f, base, n, s);
#pragma unroll
	for (int d = 1; d < (int)CTX_TEAM; d <<= 1) {   /* inclusive over the team: up for the forward pair, down for the backward */
		const uint64_t y0 = __shfl_up(s[0], d, (int)CTX_TEAM), y1 = __shfl_up(s[1], d, (int)CTX_TEAM);
		const uint64_t y2 = __shfl_down(s[2], d, (int)CTX_TEAM), y3 = __shfl_down(s[3], d, (int)CTX_TEAM);
		if (sub >= (uint32_t)d) { s[0] = umax64(s[0], y0); s[1] = umax64(s[1], y1); }
		if (sub + (uint32_t)d < CTX_TEAM) { s[2] = umin64(s[2], y2); s[3] = umin64(s[3], y3); }
	}
	const uint64_t e0 = __shfl_up(s[0], 1, (int)CTX_TEAM), e1 = __shfl_up(s[1], 1, (int)CTX_TEAM);
	const uint64_t e2 = __shfl_down(s[2], 1, (int)CTX_TEAM), e3 = __shfl_down(s[3], 1, (int)CTX_TEAM);
	if (wi >= nwords) return;   /* after the last shuffle: the lanes of a team are all there for them */
	const uint64_t b = wi / CTX_TEAM;   /* a block of the summary, as wi < nwords */
	const u64x2 cf = *(glb_u64x2p)(uintptr_t)(sum + 4u * b), cb = *(glb_u64x2p)(uintptr_t)(sum + 4u * b + 2u);
	const uint64_t ps1 = sub == 0u ? cf.x : umax64(cf.x, e0), pf = sub == 0u ? cf.y : umax64(cf.y, e1);
	const uint64_t ns = sub == CTX_TEAM - 1u ? cb.x : umin64(cb.x, e2), nf = sub == CTX_TEAM - 1u ? cb.y : umin64(cb.y, e3);
	uint64_t W = 0;
	/* from the left: lines up to `after` past p, as long as no file starts in (p, i] */
	if (ps1 != 0u && pf <= ps1 - 1u && (f & 1u) == 0u) {
		const uint64_t d = base - (ps1 - 1u);           /* >= 1: from p to the word's first line */
		if (after >= d) {
			uint32_t hi = after - d >= 63u ? 63u : (uint32_t)(after - d);
			if (f != 0) { const uint32_t c = (uint32_t)__builtin_ctzll(f) - 1u; hi = hi < c ? hi : c; }
			W |= bits_between(0u, hi);
		}
	}
	/* from the right: lines down to `before` ahead of q, as long as no file starts in (i, q] */
	if (ns != CTX_NONE && ns < nf) {
		const uint64_t d = ns - (base + 63u);           /* >= 1: from the word's last line to q */
		if (before >= d) {
			uint32_t lo = before - d >= 63u ? 0u : 63u - (uint32_t)(before - d);
			if (f != 0) { const uint32_t c = 63u - (uint32_t)__builtin_clzll(f); lo = lo > c ? lo : c; }
			W |= bits_between(lo, 63u);
		}
	}
	/* the word's own selected lines: [max(j - before, last file start <= j), min(j + after, first file start > j - 1)] */
	for (uint64_t ww = w; ww != 0; ww &= ww - 1u) {
		const uint32_t j = (uint32_t)__builtin_ctzll(ww);
		const uint64_t upto = ((uint64_t)2 << j) - 1u;  /* bits 0 .. j (j == 63: all) */
		const uint64_t fa = f & ~upto, fb = f & upto;
		uint32_t hi = fa != 0 ? (uint32_t)__builtin_ctzll(fa) - 1u : 63u;
		uint32_t lo = fb != 0 ? 63u - (uint32_t)__builtin_clzll(fb) : 0u;
		if (after < hi - j) hi = j + (uint32_t)after;
		if (before < j - lo) lo = j - (uint32_t)before;
		W |= bits_between(lo, hi);
	}
	if (n - base < 64u) W &= ((uint64_t)1 << (uint32_t)(n - base)) - 1u;
	((glb_u64w)(uintptr_t)out)[wi] = W;
}

/* one lane per hit; word k / 64 of core and of group by ballot, stored by the wavefront's first lane; meta[1] += the groups.
 * A line number that is none (arrays gone wrong) reads nothing. */
__global__ void __launch_bounds__(CTX_THREADS)
ctx_marks(const uint64_t *lines, uint64_t m, const uint64_t *bitmap, const uint64_t *fmap, uint64_t n, uint32_t invert, uint64_t *core,
          uint64_t *group, uint64_t *meta)
{
	const uint64_t k = (uint64_t)blockIdx.x * CTX_THREADS + threadIdx.x;
	const glb_u64p ln = (glb_u64p)(uintptr_t)lines;
	bool c = false, g = false;
	if (k < m) {
		const uint64_t i = ln[k];
		if (i < n) {
			const uint64_t x = ((glb_u64p)(uintptr_t)bitmap)[i >> 6];
			c = (((invert != 0u ? ~x : x) >> (uint32_t)(i & 63u)) & 1u) != 0u;
			g = k == 0 || ln[k - 1u] + 1u != i || (fmap != nullptr && ((((glb_u64p)(uintptr_t)fmap)[i >> 6] >> (uint32_t)(i & 63u)) & 1u) != 0u);
		}
	}
	const uint64_t mc = __ballot(c), mg = __ballot(g);
	if ((threadIdx.x & 63u) == 0u && k < m) {
		((glb_u64w)(uintptr_t)core)[k >> 6] = mc;
		((glb_u64w)(uintptr_t)group)[k >> 6] = mg;
		if (mg != 0)
			(void)__hip_atomic_fetch_add((glb_u64w)(uintptr_t)(meta + 1), (uint64_t)__builtin_popcountll(mg), __ATOMIC_RELAXED,
			                             __HIP_MEMORY_SCOPE_AGENT);
	}
}

}   // namespace

struct __attribute__((visibility("hidden"))) fsm_hip_text_hits {
	int device = 0, delim = 0;                   /* delim: the text's */
	size_t m = 0, nbytes = 0;
	DevBuf<uint64_t> d_pairs;                /* per block of lines: (lines, bytes) selected, then their exclusive scan; + m and the bytes */
	DevBuf<uint64_t> d_lines;                /* m */
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_src;                  /* m: where each selected line starts in the text */
	DevBuf<uint64_t> d_first;                /* per output block + 1: the rank of the line that covers its first byte */
	DevBuf<unsigned char> d_bytes;           /* nbytes, rounded up to whole blocks */
	DevEvent ev[6];                          /* around count + scan, emit, gather; ev[5]: all is there */
	size_t nfiles = 0;                       /* a text of files: its hits per file; 0 / NULL for a plain text */
	DevBuf<uint64_t> d_file_first;           /* nfiles + 1 */
	DevEvent fev[2];                         /* around hits_file_first, between emit and gather */
	/* hits with context (fsm_hip_text_hits_context*): all NULL / 0 in plain hits */
	bool context = false;
	size_t core_count = 0;
	DevBuf<uint64_t> d_wide;                 /* ceil(n / 64): W, the bitmap the select reads */
	DevBuf<uint64_t> d_fmap;                 /* ceil(n / 64): F, the file starts; NULL for a plain text */
	DevBuf<uint64_t> d_sum;                  /* per block of lines: its summary, then the carries; + the 2 words of d_cmeta */
	uint64_t *d_cmeta = nullptr;             /* inside d_sum: (core_count, groups), counted by atomics from 0 */
	DevBuf<uint64_t> d_core;                 /* ceil(m / 64) */
	DevBuf<uint64_t> d_group;                /* ceil(m / 64) */
	DevEvent cev[4];                         /* around the widening, around the marks */
};

extern "C" void fsm_hip_text_hits_free(struct fsm_hip_text_hits *h)
{
	if (h == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(h->device);
		if (h->ev[5] != nullptr) (void)hipEventSynchronize(h->ev[5]);
		delete h;
	}
	errno = e;
}

/* the passes over d_bitmap on stream s into *h, t's device current: with a context (ctx = {before, after}) the widening first,
 * and the select then reads W with no invert.  One wait in the middle (m and the bytes size the arrays, the core count rides
 * along); emit, marks and gather in flight at return. */
static int text_hits_run(struct fsm_hip_text_hits *h, const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags,
	const uint64_t *ctx, hipStream_t s)
{
	const uint64_t n = t->n, nwords = (n + 63u) / 64u;
	const uint32_t invert = (flags & FSM_HIP_HITS_INVERT) != 0u ? 1u : 0u;
	const bool bytes = (flags & FSM_HIP_HITS_NO_BYTES) == 0u;
	uint64_t nblocks = (n + HITS_LINES - 1u) / HITS_LINES;
	const uint64_t *d_sel = d_bitmap;   /* what the select reads */
	uint32_t sel_invert = invert;
	uint64_t meta[2] = {0, 0}, core = 0;
	for (DevEvent &ev : h->ev)
		if (!HIP_OK(ev.create())) return -1;
	if (!HIP_OK(hipStreamWaitEvent(s, t->ev[3], 0))) return -1;   /* the text's offsets and file_lines first */
	if (ctx != nullptr) {
		const uint64_t wgrid = (nblocks + CTX_WG_BLOCKS - 1u) / CTX_WG_BLOCKS;
		if (wgrid > 0x7fffffffu) { errno = ENOMEM; return -1; }
		h->context = true;
		for (DevEvent &ev : h->cev)
			if (!HIP_OK(ev.create())) return -1;
		if (n != 0) {
			if (!HIP_OK(h->d_wide.alloc(nwords)) || !HIP_OK(h->d_sum.alloc(4u * nblocks + 2u))) return -1;
			if (t->nfiles != 0 && !HIP_OK(h->d_fmap.alloc(nwords))) return -1;
		}
		if (!HIP_OK(hipEventRecord(h->cev[0], s))) return -1;
		if (n != 0) {
			h->d_cmeta = h->d_sum + 4u * nblocks;
			if (!HIP_OK(hipMemsetAsync(h->d_cmeta, 0, 2u * sizeof(uint64_t), s))) return -1;
			if (t->nfiles != 0) {
				const uint64_t nends = (uint64_t)t->nfiles + 1u;
				if (!HIP_OK(hipMemsetAsync(h->d_fmap, 0, nwords * sizeof(uint64_t), s))) return -1;
				hipLaunchKernelGGL(ctx_file_starts, dim3((unsigned)((nends + CTX_THREADS - 1u) / CTX_THREADS)), dim3(CTX_THREADS), 0, s,
				                   t->d_file_lines, nends, n, h->d_fmap);
				if (!HIP_OK(hipGetLastError())) return -1;
			}
			hipLaunchKernelGGL(ctx_summary, dim3((unsigned)wgrid), dim3(CTX_THREADS), 0, s, d_bitmap, h->d_fmap, n, nwords, invert, nblocks,
			                   h->d_sum, h->d_cmeta);
			if (!HIP_OK(hipGetLastError())) return -1;
			hipLaunchKernelGGL(ctx_scan, dim3(1), dim3(CTX_SCAN_THREADS), 0, s, h->d_sum, nblocks, n);
			if (!HIP_OK(hipGetLastError())) return -1;
			hipLaunchKernelGGL(ctx_apply, dim3((unsigned)wgrid), dim3(CTX_THREADS), 0, s, d_bitmap, h->d_fmap, n, nwords, invert, h->d_sum,
			                   ctx[0], ctx[1], h->d_wide);
			if (!HIP_OK(hipGetLastError())) return -1;
		}
		if (!HIP_OK(hipEventRecord(h->cev[1], s))) return -1;
		d_sel = h->d_wide;
		sel_invert = 0u;
	}
	Grid g = grid_of(nblocks, t->device);
	if (!HIP_OK(hipEventRecord(h->ev[0], s))) return -1;
	if (n != 0) {
		if (!HIP_OK(h->d_pairs.alloc(2u * nblocks + 2u))) return -1;
		uint64_t *d_meta = h->d_pairs + 2u * nblocks;
		hipLaunchKernelGGL(hits_count, dim3((unsigned)g.wgs), dim3(HITS_THREADS), 0, s, d_sel, t->d_off, n, sel_invert, nblocks, g.per, h->d_pairs);
		if (!HIP_OK(hipGetLastError())) return -1;
		hipLaunchKernelGGL(hits_scan, dim3(1), dim3(1024), 0, s, h->d_pairs, nblocks, d_meta);
		if (!HIP_OK(hipGetLastError())) return -1;
		if (!HIP_OK(hipEventRecord(h->ev[1], s))) return -1;
		if (!HIP_OK(hipMemcpyAsync(meta, d_meta, sizeof meta, hipMemcpyDeviceToHost, s))) return -1;
		if (ctx != nullptr && !HIP_OK(hipMemcpyAsync(&core, h->d_cmeta, sizeof core, hipMemcpyDeviceToHost, s))) return -1;
		if (!HIP_OK(hipStreamSynchronize(s))) return -1;
	} else if (!HIP_OK(hipEventRecord(h->ev[1], s))) {
		return -1;
	}
	h->core_count = (size_t)core;
	h->m = (size_t)meta[0];
	h->nbytes = bytes ? (size_t)meta[1] : 0;
	if (h->m == 0) { nblocks = 0; g = Grid(); }   /* nothing to re-read: the emit kernel leaves out_off = {0} alone */
	const uint64_t m = h->m, ngb = ((uint64_t)h->nbytes + HITS_BLOCK - 1u) / HITS_BLOCK;
	if (m != 0 && !HIP_OK(h->d_lines.alloc(m))) return -1;
	if (bytes) {
		if (!HIP_OK(h->d_off.alloc(m + 1u))) return -1;
		if (m != 0 && (!HIP_OK(h->d_src.alloc(m)) || !HIP_OK(h->d_first.alloc(ngb + 1u)) || !HIP_OK(h->d_bytes.alloc(ngb * HITS_BLOCK)))) return -1;
	}
	if (!HIP_OK(hipEventRecord(h->ev[2], s))) return -1;
	if (m != 0 || bytes) {
		hipLaunchKernelGGL(hits_emit, dim3((unsigned)g.wgs), dim3(HITS_THREADS), 0, s, d_sel, t->d_off, n, sel_invert, nblocks, g.per, h->d_pairs,
		                   m, (uint64_t)h->nbytes, h->d_lines, h->d_off, h->d_src, h->d_first, ngb);
		if (!HIP_OK(hipGetLastError())) return -1;
	}
	if (!HIP_OK(hipEventRecord(h->ev[3], s))) return -1;
	if (ctx != nullptr) {   /* the marks of the m hits: core and group, ceil(m / 64) words each; they read the caller's bitmap */
		if (!HIP_OK(hipEventRecord(h->cev[2], s))) return -1;
		if (m != 0) {
			const uint64_t mwords = (m + 63u) / 64u, mgrid = (m + CTX_THREADS - 1u) / CTX_THREADS;
			if (mgrid > 0x7fffffffu) { errno = ENOMEM; return -1; }
			if (!HIP_OK(h->d_core.alloc(mwords)) || !HIP_OK(h->d_group.alloc(mwords))) return -1;
			hipLaunchKernelGGL(ctx_marks, dim3((unsigned)mgrid), dim3(CTX_THREADS), 0, s, h->d_lines, m, d_bitmap, h->d_fmap, n, invert, h->d_core,
			                   h->d_group, h->d_cmeta);
			if (!HIP_OK(hipGetLastError())) return -1;
		}
		if (!HIP_OK(hipEventRecord(h->cev[3], s))) return -1;
	}
	if (t->nfiles != 0) {   /* also under NO_BYTES and when m == 0 */
		const uint64_t nends = (uint64_t)t->nfiles + 1u;
		h->nfiles = t->nfiles;
		for (DevEvent &ev : h->fev)
			if (!HIP_OK(ev.create())) return -1;
		if (!HIP_OK(h->d_file_first.alloc(nends))) return -1;
		if (!HIP_OK(hipEventRecord(h->fev[0], s))) return -1;
		hipLaunchKernelGGL(hits_file_first, dim3((unsigned)((nends + HITS_THREADS - 1u) / HITS_THREADS)), dim3(HITS_THREADS), 0, s, h->d_lines, m,
		                   t->d_file_lines, nends, h->d_file_first);
		if (!HIP_OK(hipGetLastError())) return -1;
		if (!HIP_OK(hipEventRecord(h->fev[1], s))) return -1;
	}
	if (!HIP_OK(hipEventRecord(h->ev[4], s))) return -1;
	if (ngb != 0) {
		const Grid gg = grid_of(ngb, t->device);
		hipLaunchKernelGGL(hits_gather, dim3((unsigned)gg.wgs), dim3(HITS_THREADS), 0, s, t->d_text, (uint64_t)t->nbytes, h->d_off, h->d_src,
		                   h->d_first, m, (uint64_t)h->nbytes, ngb, gg.per, h->d_bytes);
		if (!HIP_OK(hipGetLastError())) return -1;
	}
	return HIP_OK(hipEventRecord(h->ev[5], s)) ? 0 : -1;
}

/* the hits object of a run on stream s; when the run fails, the stream is made idle before what it has launched on is released */
static struct fsm_hip_text_hits *text_hits_new(const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags, const uint64_t *ctx,
	hipStream_t s)
{
	DevGuard dg(t->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	struct fsm_hip_text_hits *h = new (std::nothrow) struct fsm_hip_text_hits;
	if (h == nullptr) { errno = ENOMEM; return nullptr; }
	h->device = t->device;
	h->delim = t->delim;
	if (text_hits_run(h, t, d_bitmap, flags, ctx, s) == 0) return h;
	const int e = errno;
	(void)hipStreamSynchronize(s);
	fsm_hip_text_hits_free(h);
	errno = e;
	return nullptr;
}

static int text_hits_check(const struct fsm_hip_text *t, unsigned flags)
{
	if (t == nullptr || (flags & ~(FSM_HIP_HITS_INVERT | FSM_HIP_HITS_NO_BYTES)) != 0u) { errno = EINVAL; return -1; }
	return 0;
}

/* the device forms: the caller's bitmap, the caller's stream, nothing waited for beyond the run's own wait */
static struct fsm_hip_text_hits *text_hits_device(const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags, const uint64_t *ctx,
	void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (text_hits_check(t, flags) != 0) return nullptr;
	if (d_bitmap == nullptr && t->n != 0) { errno = EINVAL; return nullptr; }
	return text_hits_new(t, d_bitmap, flags, ctx, static_cast<hipStream_t>(hip_stream));
}

/* the host forms: the walk's bitmap on the text's own stream, which is idle at return: the bitmap is released then, and the
 * gather and the marks have read it */
static struct fsm_hip_text_hits *text_hits_host(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t, unsigned flags,
	const uint64_t *ctx)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (text_hits_check(t, flags) != 0 || text_exec_check(ld, t) != 0) return nullptr;
	DevGuard dg(t->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	DevBuf<uint64_t> d_bm;
	struct fsm_hip_text_hits *h = nullptr;
	bool ok = true;
	if (t->n != 0)
		ok = HIP_OK(d_bm.alloc((t->n + 63u) / 64u)) && HIP_OK(hipStreamWaitEvent(t->own, t->ev[3], 0)) &&
		     fsm_hip_text_exec_device(ld, t, nullptr, d_bm, 0, nullptr, nullptr, t->own) == 0;
	ok = ok && (h = text_hits_new(t, d_bm, flags, ctx, t->own)) != nullptr;
	ok = ok && HIP_OK(hipStreamSynchronize(t->own));
	if (ok) return h;
	const int e = errno;
	(void)hipStreamSynchronize(t->own);
	if (h != nullptr) fsm_hip_text_hits_free(h);
	errno = e;
	return nullptr;
}

extern "C" struct fsm_hip_text_hits *fsm_hip_text_hits_device(const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags,
	void *hip_stream)
{
	return text_hits_device(t, d_bitmap, flags, nullptr, hip_stream);
}

extern "C" struct fsm_hip_text_hits *fsm_hip_text_hits(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t, unsigned flags)
{
	return text_hits_host(ld, t, flags, nullptr);
}

extern "C" struct fsm_hip_text_hits *fsm_hip_text_hits_context_device(const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags,
	uint64_t before, uint64_t after, void *hip_stream)
{
	const uint64_t ctx[2] = {before, after};
	return text_hits_device(t, d_bitmap, flags, ctx, hip_stream);
}

extern "C" struct fsm_hip_text_hits *fsm_hip_text_hits_context(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t, unsigned flags,
	uint64_t before, uint64_t after)
{
	const uint64_t ctx[2] = {before, after};
	return text_hits_host(ld, t, flags, ctx);
}

extern "C" const uint64_t *fsm_hip_text_hits_core_device(const struct fsm_hip_text_hits *h) { return h == nullptr ? nullptr : h->d_core.p; }
extern "C" const uint64_t *fsm_hip_text_hits_group_device(const struct fsm_hip_text_hits *h) { return h == nullptr ? nullptr : h->d_group.p; }
extern "C" size_t fsm_hip_text_hits_core_count(const struct fsm_hip_text_hits *h) { return h == nullptr ? 0 : h->core_count; }
extern "C" size_t fsm_hip_text_context_scan_block(void) { return CTX_SCAN_THREADS; }

extern "C" int fsm_hip_text_hits_marks(const struct fsm_hip_text_hits *h, uint64_t *core, uint64_t *group)
{
	if (h == nullptr || !h->context) { errno = EINVAL; return -1; }
	const size_t nb = (h->m + 63u) / 64u * sizeof(uint64_t);
	return copy_out(h->device, h->ev[5], {{core, h->d_core, nb}, {group, h->d_group, nb}});
}

extern "C" size_t fsm_hip_text_hits_groups(const struct fsm_hip_text_hits *h)
{
	uint64_t g = 0;
	if (h == nullptr || !h->context || h->m == 0) return 0;
	(void)copy_out(h->device, h->ev[5], {{&g, h->d_cmeta + 1, sizeof g}});   /* g stays 0 when it fails */
	return (size_t)g;
}

extern "C" double fsm_hip_text_hits_context_ms(const struct fsm_hip_text_hits *h)
{
	if (h == nullptr || !h->context) { errno = EINVAL; return -1.0; }
	return elapsed_ms(h->device, h->ev[5], {{h->cev[0], h->cev[1]}, {h->cev[2], h->cev[3]}});
}

extern "C" size_t fsm_hip_text_hits_count(const struct fsm_hip_text_hits *h) { return h == nullptr ? 0 : h->m; }
extern "C" size_t fsm_hip_text_hits_nbytes(const struct fsm_hip_text_hits *h) { return h == nullptr ? 0 : h->nbytes; }
extern "C" const uint64_t *fsm_hip_text_hits_lines_device(const struct fsm_hip_text_hits *h) { return h == nullptr ? nullptr : h->d_lines.p; }
extern "C" const uint64_t *fsm_hip_text_hits_offsets_device(const struct fsm_hip_text_hits *h) { return h == nullptr ? nullptr : h->d_off.p; }
extern "C" const unsigned char *fsm_hip_text_hits_bytes_device(const struct fsm_hip_text_hits *h) { return h == nullptr ? nullptr : h->d_bytes.p; }
extern "C" size_t fsm_hip_text_hits_block_lines(void) { return HITS_LINES; }
extern "C" size_t fsm_hip_text_hits_block_bytes(void) { return HITS_BLOCK; }

extern "C" int fsm_hip_text_hits_copy(const struct fsm_hip_text_hits *h, uint64_t *lines, uint64_t *out_off, void *bytes)
{
	if (h == nullptr || (out_off != nullptr && h->d_off == nullptr)) { errno = EINVAL; return -1; }
	return copy_out(h->device, h->ev[5], {{lines, h->d_lines, h->m * sizeof(uint64_t)}, {out_off, h->d_off, (h->m + 1u) * sizeof(uint64_t)},
	                                      {bytes, h->d_bytes, h->nbytes}});
}

extern "C" const uint64_t *fsm_hip_text_hits_file_first_device(const struct fsm_hip_text_hits *h)
{
	return h == nullptr ? nullptr : h->d_file_first.p;
}

extern "C" int fsm_hip_text_hits_file_first(const struct fsm_hip_text_hits *h, uint64_t *out)
{
	if (h == nullptr || out == nullptr || h->d_file_first == nullptr) { errno = EINVAL; return -1; }
	return copy_out(h->device, h->ev[5], {{out, h->d_file_first, (h->nfiles + 1u) * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_text_hits_file_first_ms(const struct fsm_hip_text_hits *h)
{
	if (h == nullptr || h->d_file_first == nullptr) { errno = EINVAL; return -1.0; }
	return elapsed_ms(h->device, h->ev[5], {{h->fev[0], h->fev[1]}});
}

extern "C" double fsm_hip_text_hits_ms(const struct fsm_hip_text_hits *h)
{
	if (h == nullptr) { errno = EINVAL; return -1.0; }
	return elapsed_ms(h->device, h->ev[5], {{h->ev[0], h->ev[1]}, {h->ev[2], h->ev[3]}, {h->ev[4], h->ev[5]}});
}

extern "C" double fsm_hip_text_hits_gather_ms(const struct fsm_hip_text_hits *h)
{
	if (h == nullptr) { errno = EINVAL; return -1.0; }
	return elapsed_ms(h->device, h->ev[5], {{h->ev[4], h->ev[5]}});
}

/* ---- files of a text: lines cut at every file end as well ----------------------------------------------------------
 * file_off[0 .. nfiles] are byte positions (0 first, non-decreasing, nbytes last); the offsets of the text become the sorted
 * union of the plain offsets P (the scan above, untouched) and the file ends.  A file end p adds an entry iff it is not in P
 * already: 0 < p < nbytes and text[p - 1] != delim -- one text byte tells, so the added ends S are COUNTED before any offset
 * exists and their total rides the one wait with the delimiter count.  Of a run of equal ends the LAST member carries the
 * flag: then the flags before any member j of the run belong to smaller values only, and
 *     R(j) = #{S < file_off[j]} = scanned pair of j's block + flags before j in its block
 * holds for every member alike.  The passes:
 *     files_mark    one lane per file end: validates it against its neighbours, flags "adds an entry", leaves the flags before
 *                   it in its block and the block's (flags, invalid entries)                       (reads file_off, one text byte)
 *     files_scan    exclusive scan of the pairs by one workgroup in rounds; the totals for the host  (text_scan's shape)
 *     files_merge   one lane per entry of P and per file end, a binary search each:
 *                     P[i]         -> off[i + #{S < P[i]}]            #{S < v} = R(lower_bound(file_off, v))
 *                     added end j  -> off[lower_bound(P, file_off[j]) + R(j)]
 *                     file_lines[j] =   lower_bound(P, file_off[j]) + R(j)    for every j
 * Every slot of off is written exactly once when the array is what files_mark validated.  Loads from the text are made only
 * for 0 < p < nbytes and stores only below the counted totals: a file_off that changes between the passes gives wrong arrays,
 * never an overrun. */
namespace {

constexpr uint32_t FILES_WAVES = 4;
constexpr uint32_t FILES_THREADS = FILES_WAVES * 64u;       /* file ends a workgroup of files_mark takes */
constexpr uint32_t FILES_SCAN_THREADS = 256;                /* pairs a round of files_scan takes */

__global__ void __launch_bounds__(FILES_THREADS)
files_mark(const unsigned char *text, uint64_t nbytes, uint32_t delim, const uint64_t *file_off, uint64_t nends, uint64_t *rank,
           uint64_t *pairs)
{
	__shared__ uint32_t wtot[FILES_WAVES][2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const glb_u64p fo = (glb_u64p)(uintptr_t)file_off;
	const uint64_t j = (uint64_t)blockIdx.x * FILES_THREADS + threadIdx.x;
	bool flag = false, bad = false;
	if (j < nends) {
		const uint64_t p = fo[j];
		bad = j == 0 ? p != 0 : fo[j - 1u] > p;
		if (j + 1u == nends) bad = bad || p != nbytes;
		const bool last_of_run = j + 1u == nends || fo[j + 1u] != p;
		if (last_of_run && p > 0 && p < nbytes) flag = ((glb_u8p)(uintptr_t)text)[p - 1u] != delim;   /* p - 1 is inside the text */
	}
	const uint64_t mf = __ballot(flag), mb = __ballot(bad);
	if (lane == 0) { wtot[wave][0] = (uint32_t)__builtin_popcountll(mf); wtot[wave][1] = mb != 0 ? 1u : 0u; }
	__syncthreads();
	uint32_t before = (uint32_t)__builtin_popcountll(mf & ((1ull << lane) - 1ull)), tot = 0, anybad = 0;
#pragma unroll
	for (uint32_t w = 0; w < FILES_WAVES; w++) {
		before += w < wave ? wtot[w][0] : 0u;
		tot += wtot[w][0];
		anybad |= wtot[w][1];
	}
	if (j < nends) ((glb_u64w)(uintptr_t)rank)[j] = (uint64_t)before << 1 | (flag ? 1u : 0u);
	if (threadIdx.x == 0) *(glb_u64x2w)(uintptr_t)(pairs + 2u * blockIdx.x) = u64x2{tot, anybad};
}

/* the exclusive scan of the pairs, FILES_SCAN_THREADS a round; meta[0] = the added ends, meta[1] != 0 iff the array is invalid:
 * the second half of the 32 bytes the host waits for */
__global__ void __launch_bounds__(FILES_SCAN_THREADS)
files_scan(uint64_t *pairs, uint64_t nblocks, uint64_t *meta)
{
	sum_scan<FILES_SCAN_THREADS, 2, 1>(pairs, nblocks, meta);
}

/* lanes [0, np1) take the plain offsets, lanes [np1, np1 + nends) the file ends; n + 1 = np1 + added entries of off */
__global__ void __launch_bounds__(FILES_THREADS)
files_merge(const uint64_t *plain, uint64_t np1, const uint64_t *file_off, uint64_t nends, const uint64_t *rank, const uint64_t *base,
            uint64_t added, uint64_t n, uint64_t *off, uint64_t *file_lines)
{
	const glb_u64p pl = (glb_u64p)(uintptr_t)plain, fo = (glb_u64p)(uintptr_t)file_off, rk = (glb_u64p)(uintptr_t)rank,
	               bs = (glb_u64p)(uintptr_t)base;
	const glb_u64w out = (glb_u64w)(uintptr_t)off;
	const uint64_t g = (uint64_t)blockIdx.x * FILES_THREADS + threadIdx.x;
	if (g < np1) {
		const uint64_t v = pl[g];
		const uint64_t lb = lower_bound_glb(fo, nends, v);
		const uint64_t dst = g + (lb < nends ? bs[2u * (lb / FILES_THREADS)] + (rk[lb] >> 1) : added);
		if (dst <= n) out[dst] = v;
	} else if (g - np1 < nends) {
		const uint64_t j = g - np1, v = fo[j], r = rk[j];
		const uint64_t dst = lower_bound_glb(pl, np1, v) + bs[2u * (j / FILES_THREADS)] + (r >> 1);
		((glb_u64w)(uintptr_t)file_lines)[j] = dst;
		if ((r & 1u) != 0u && dst <= n) out[dst] = v;
	}
}

}   // namespace

/* ---- opening a text: plain (nfiles == 0) or of files ---- */

/* on stream s over t->d_text: count + scan of the delimiters and, for files, mark + scan of the file ends; ONE wait (the totals
 * size the arrays, and tell a file_off that is none); then the plain offsets and, for files, the merge */
static int text_cut(struct fsm_hip_text *t, hipStream_t s)
{
	const bool files = t->nfiles != 0;
	const uint64_t nbytes = t->nbytes, nends = files ? (uint64_t)t->nfiles + 1u : 0u;
	const uint32_t splat = (uint32_t)t->delim * 0x01010101u;
	const uint64_t nblocks = (nbytes + TEXT_BLOCK - 1u) / TEXT_BLOCK, nfb = (nends + FILES_THREADS - 1u) / FILES_THREADS;
	const uint64_t nmeta = files ? 4u : 2u;
	uint64_t meta[4] = {0, 0, 0, 0};
	if (nfb > 0x7fffffffu) { errno = ENOMEM; return -1; }
	for (DevEvent &ev : t->ev)
		if (!HIP_OK(ev.create())) return -1;
	if (!files && nbytes == 0) {   /* no byte, no line: off[0] = 0 alone */
		if (!HIP_OK(t->d_off.alloc(1)) || !HIP_OK(hipMemsetAsync(t->d_off, 0, sizeof(uint64_t), s))) return -1;
		for (DevEvent &ev : t->ev)
			if (!HIP_OK(hipEventRecord(ev, s))) return -1;
		return 0;
	}
	const Grid g = grid_of(nblocks, t->device);
	if (!HIP_OK(t->d_cnt.alloc(nblocks + nmeta))) return -1;
	uint64_t *d_meta = t->d_cnt + nblocks;
	if (files) {
		for (DevEvent &ev : t->fev)
			if (!HIP_OK(ev.create())) return -1;
		if (!HIP_OK(t->d_frank.alloc(nends)) || !HIP_OK(t->d_fpairs.alloc(2u * nfb)) || !HIP_OK(t->d_file_lines.alloc(nends))) return -1;
	}
	if (!HIP_OK(hipEventRecord(t->ev[0], s))) return -1;
	if (nbytes != 0) {
		hipLaunchKernelGGL(text_count, dim3((unsigned)g.wgs), dim3(TEXT_THREADS), 0, s, t->d_text, nbytes, splat, nblocks, g.per, t->d_cnt);
		if (!HIP_OK(hipGetLastError())) return -1;
		hipLaunchKernelGGL(text_scan, dim3(1), dim3(1024), 0, s, t->d_cnt, nblocks, t->d_text, nbytes, (uint32_t)t->delim, d_meta);
		if (!HIP_OK(hipGetLastError())) return -1;
	} else if (!HIP_OK(hipMemsetAsync(d_meta, 0, 2u * sizeof(uint64_t), s))) {
		return -1;
	}
	if (!HIP_OK(hipEventRecord(t->ev[1], s))) return -1;
	if (files) {
		if (!HIP_OK(hipEventRecord(t->fev[0], s))) return -1;
		hipLaunchKernelGGL(files_mark, dim3((unsigned)nfb), dim3(FILES_THREADS), 0, s, t->d_text, nbytes, (uint32_t)t->delim, t->d_file_off, nends,
		                   t->d_frank, t->d_fpairs);
		if (!HIP_OK(hipGetLastError())) return -1;
		hipLaunchKernelGGL(files_scan, dim3(1), dim3(FILES_SCAN_THREADS), 0, s, t->d_fpairs, nfb, d_meta + 2);
		if (!HIP_OK(hipGetLastError())) return -1;
		if (!HIP_OK(hipEventRecord(t->fev[1], s))) return -1;
	}
	if (!HIP_OK(hipMemcpyAsync(meta, d_meta, nmeta * sizeof(uint64_t), hipMemcpyDeviceToHost, s))) return -1;
	if (!HIP_OK(hipStreamSynchronize(s))) return -1;
	if (meta[3] != 0) { errno = EINVAL; return -1; }
	/* the plain offsets: bytes after the last delimiter form a last line */
	const uint64_t np1 = nbytes == 0 ? 1u : meta[0] + (meta[1] != 0 ? 0u : 1u) + 1u;
	const uint64_t nmerge = (np1 + nends + FILES_THREADS - 1u) / FILES_THREADS;
	t->n = (size_t)(np1 - 1u + meta[2]);
	if (files) {
		if (nmerge > 0x7fffffffu) { errno = ENOMEM; return -1; }
		if (!HIP_OK(t->d_plain.alloc(np1))) return -1;
	}
	if (!HIP_OK(t->d_off.alloc((uint64_t)t->n + 1u))) return -1;
	uint64_t *d_plain = files ? t->d_plain : t->d_off;
	if (!HIP_OK(hipEventRecord(t->ev[2], s))) return -1;
	if (nbytes != 0) {
		hipLaunchKernelGGL(text_offsets, dim3((unsigned)g.wgs), dim3(TEXT_THREADS), 0, s, t->d_text, nbytes, splat, nblocks, g.per, t->d_cnt, meta[0],
		                   np1 - 1u, d_plain);
		if (!HIP_OK(hipGetLastError())) return -1;
	} else if (!HIP_OK(hipMemsetAsync(d_plain, 0, sizeof(uint64_t), s))) {
		return -1;
	}
	if (files) {
		if (!HIP_OK(hipEventRecord(t->fev[2], s))) return -1;
		hipLaunchKernelGGL(files_merge, dim3((unsigned)nmerge), dim3(FILES_THREADS), 0, s, d_plain, np1, t->d_file_off, nends, t->d_frank,
		                   t->d_fpairs, meta[2], (uint64_t)t->n, t->d_off, t->d_file_lines);
		if (!HIP_OK(hipGetLastError())) return -1;
	}
	return HIP_OK(hipEventRecord(t->ev[3], s)) ? 0 : -1;
}

/* what the four open entry points share once their own arguments are checked */
static struct fsm_hip_text *text_open(const void *text, size_t nbytes, int delim, const uint64_t *file_off, size_t nfiles, void *hip_stream,
	bool host)
{
	if (delim < 0 || delim > 255) { errno = EINVAL; return nullptr; }
	if (!have_device()) { errno = ENODEV; return nullptr; }   /* no CPU path, as everywhere in this library */
	struct fsm_hip_text *t = new (std::nothrow) fsm_hip_text;
	if (t == nullptr) { errno = ENOMEM; return nullptr; }
	t->nbytes = nbytes;
	t->delim = delim;
	t->nfiles = nfiles;
	if (hipGetDevice(&t->device) != hipSuccess) { delete t; errno = ENODEV; return nullptr; }
	if (!HIP_OK(t->own.create(hipStreamNonBlocking))) { delete t; return nullptr; }
	hipStream_t s = host ? t->own : static_cast<hipStream_t>(hip_stream);
	bool ok = true;
	if (!host) {   /* the caller's device memory, the caller's stream: the offsets are in flight at return */
		t->d_text = static_cast<const unsigned char *>(text);
		t->d_file_off = file_off;
	} else {       /* copied to the device on the text's own stream, which is idle at return */
		const uint64_t nends = (uint64_t)nfiles + 1u;
		if (nbytes != 0) ok = HIP_OK(t->owned.alloc(nbytes)) && HIP_OK(hipMemcpyAsync(t->owned, text, nbytes, hipMemcpyHostToDevice, s));
		if (ok && nfiles != 0)
			ok = HIP_OK(t->owned_file_off.alloc(nends)) &&
			     HIP_OK(hipMemcpyAsync(t->owned_file_off, file_off, nends * sizeof(uint64_t), hipMemcpyHostToDevice, s));
		t->d_text = t->owned;
		t->d_file_off = t->owned_file_off;
	}
	ok = ok && text_cut(t, s) == 0 && (!host || HIP_OK(hipStreamSynchronize(s)));
	if (ok) {
		if (host) t->d_plain.reset();   /* the merge has read them */
		return t;
	}
	const int e = errno;
	(void)hipStreamSynchronize(s);   /* nothing of this text is in flight when it is freed */
	fsm_hip_text_free(t);
	errno = e;
	return nullptr;
}

extern "C" struct fsm_hip_text *fsm_hip_text_open_device(const void *d_text, size_t nbytes, int delim, void *hip_stream)
{
	if (d_text == nullptr && nbytes != 0) { errno = EINVAL; return nullptr; }
	return text_open(d_text, nbytes, delim, nullptr, 0, hip_stream, false);
}

extern "C" struct fsm_hip_text *fsm_hip_text_open(const void *text, size_t nbytes, int delim)
{
	if (text == nullptr && nbytes != 0) { errno = EINVAL; return nullptr; }
	return text_open(text, nbytes, delim, nullptr, 0, nullptr, true);
}

extern "C" struct fsm_hip_text *fsm_hip_text_open_files_device(const void *d_text, size_t nbytes, int delim, const uint64_t *d_file_off,
	size_t nfiles, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if ((d_text == nullptr && nbytes != 0) || d_file_off == nullptr || nfiles == 0) { errno = EINVAL; return nullptr; }
	return text_open(d_text, nbytes, delim, d_file_off, nfiles, hip_stream, false);
}

extern "C" struct fsm_hip_text *fsm_hip_text_open_files(const void *text, size_t nbytes, int delim, const uint64_t *file_off, size_t nfiles)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if ((text == nullptr && nbytes != 0) || file_off == nullptr || nfiles == 0) { errno = EINVAL; return nullptr; }
	if (file_off[0] != 0 || file_off[nfiles] != nbytes) { errno = EINVAL; return nullptr; }
	for (size_t j = 0; j < nfiles; j++)
		if (file_off[j] > file_off[j + 1u]) { errno = EINVAL; return nullptr; }
	return text_open(text, nbytes, delim, file_off, nfiles, nullptr, true);
}

extern "C" size_t fsm_hip_text_files(const struct fsm_hip_text *t) { return t == nullptr ? 0 : t->nfiles; }

extern "C" const uint64_t *fsm_hip_text_file_lines_device(const struct fsm_hip_text *t) { return t == nullptr ? nullptr : t->d_file_lines.p; }

extern "C" int fsm_hip_text_file_lines(const struct fsm_hip_text *t, uint64_t *out)
{
	if (t == nullptr || out == nullptr || t->nfiles == 0) { errno = EINVAL; return -1; }
	return copy_out(t->device, t->ev[3], {{out, t->d_file_lines, (t->nfiles + 1u) * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_text_files_ms(const struct fsm_hip_text *t)
{
	if (t == nullptr || t->nfiles == 0) { errno = EINVAL; return -1.0; }
	return elapsed_ms(t->device, t->ev[3], {{t->fev[0], t->fev[1]}, {t->fev[2], t->ev[3]}});
}

extern "C" size_t fsm_hip_text_files_block(void) { return (size_t)FILES_THREADS * FILES_SCAN_THREADS; }

/* ---- spans of the hits: where in a selected line the match is -----------------------------------------------------------
 * Two accept-position walks (span.hip) over the hits' lines of the untouched text, trim_byte = the text's delimiter: `starts`
 * backward over [p, len) gives the leftmost start at or after p (its LAST accept in walking order), `ends` forward over
 * [start, len) the longest match from there.  spans_close makes a half-found span none and counts the hits with one;
 * spans_advance moves p behind the match (an empty match: one byte on).  One lane per hit, the rounds driven by the host. */
namespace {

constexpr uint32_t SPANS_THREADS = 256;

__global__ void __launch_bounds__(SPANS_THREADS)
spans_close(uint64_t *start, const uint64_t *end, uint64_t m, uint64_t *count)
{
	const uint64_t k = (uint64_t)blockIdx.x * SPANS_THREADS + threadIdx.x;
	bool has = false;
	if (k < m) {
		has = ((glb_u64p)(uintptr_t)end)[k] != FSM_HIP_NO_POS;   /* (end is NO_POS where start is: that input was not walked) */
		if (!has) ((glb_u64w)(uintptr_t)start)[k] = FSM_HIP_NO_POS;
	}
	const uint64_t b = __ballot(has);
	if ((threadIdx.x & 63u) == 0u && b != 0)
		(void)__hip_atomic_fetch_add((glb_u64w)(uintptr_t)count, (uint64_t)__builtin_popcountll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(SPANS_THREADS)
spans_advance(const uint64_t *start, const uint64_t *end, uint64_t m, uint64_t *p)
{
	const uint64_t k = (uint64_t)blockIdx.x * SPANS_THREADS + threadIdx.x;
	if (k >= m) return;
	const uint64_t s = ((glb_u64p)(uintptr_t)start)[k], e = ((glb_u64p)(uintptr_t)end)[k];
	((glb_u64w)(uintptr_t)p)[k] = s == FSM_HIP_NO_POS ? FSM_HIP_NO_POS : e > s ? e : e + 1u;
}

}   // namespace

struct __attribute__((visibility("hidden"))) fsm_hip_text_spans {
	int device = 0;
	size_t m = 0;
	const struct fsm_hip_text *t = nullptr;
	const struct fsm_hip_text_hits *h = nullptr;
	const struct fsm_hip_pos_dfa *starts = nullptr, *ends = nullptr;
	hipStream_t s = nullptr;                 /* the caller's */
	DevBuf<uint64_t> d_p;                    /* m: the search position of every hit */
	DevBuf<uint64_t> d_start, d_end;         /* m each */
	DevBuf<uint64_t> d_count;                /* 1: the hits with a span, counted from 0 every round */
	DevEvent ev[2];                          /* around the round's kernels; ev[1]: the round is there */
};

extern "C" void fsm_hip_text_spans_free(struct fsm_hip_text_spans *sp)
{
	if (sp == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(sp->device);
		if (sp->ev[1] != nullptr) (void)hipEventSynchronize(sp->ev[1]);
		delete sp;
	}
	errno = e;
}

/* one round on sp's stream, its device current: (advance), starts backward, ends forward, close */
static int spans_round(struct fsm_hip_text_spans *sp, bool advance)
{
	const uint64_t m = sp->m;
	hipStream_t s = sp->s;
	if (!HIP_OK(hipEventRecord(sp->ev[0], s))) return -1;
	if (m != 0) {
		const dim3 grid((unsigned)((m + SPANS_THREADS - 1u) / SPANS_THREADS)), block(SPANS_THREADS);
		if (advance) {
			hipLaunchKernelGGL(spans_advance, grid, block, 0, s, sp->d_start, sp->d_end, m, sp->d_p);
			if (!HIP_OK(hipGetLastError())) return -1;
		}
		if (!HIP_OK(hipMemsetAsync(sp->d_count, 0, sizeof(uint64_t), s))) return -1;
		struct fsm_hip_pos_batch b;
		memset(&b, 0, sizeof b);
		b.base = sp->t->d_text;
		b.off = sp->t->d_off;
		b.n = sp->t->n;
		b.pick = sp->h->d_lines;
		b.m = (size_t)m;
		b.trim_byte = sp->t->delim;
		b.limit = sp->t->nbytes;
		b.from = sp->d_p;
		b.flags = FSM_HIP_POS_BACKWARD;
		b.last_out = sp->d_start;
		if (fsm_hip_exec_accept_pos_device(sp->starts, &b, s) != 0) return -1;
		b.from = sp->d_start;
		b.flags = 0;
		b.last_out = sp->d_end;
		if (fsm_hip_exec_accept_pos_device(sp->ends, &b, s) != 0) return -1;
		hipLaunchKernelGGL(spans_close, grid, block, 0, s, sp->d_start, sp->d_end, m, sp->d_count);
		if (!HIP_OK(hipGetLastError())) return -1;
	}
	return HIP_OK(hipEventRecord(sp->ev[1], s)) ? 0 : -1;
}

extern "C" struct fsm_hip_text_spans *fsm_hip_text_hits_spans(const struct fsm_hip_text_hits *h, const struct fsm_hip_text *t,
	const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_pos_dfa *ends, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (h == nullptr || t == nullptr || starts == nullptr || ends == nullptr) { errno = EINVAL; return nullptr; }
	if (h->device != t->device || fsmhip::pos_dfa_device(starts) != t->device || fsmhip::pos_dfa_device(ends) != t->device) { errno = EINVAL; return nullptr; }
	if (((uint64_t)h->m + SPANS_THREADS - 1u) / SPANS_THREADS > 0x7fffffffu) { errno = ENOMEM; return nullptr; }
	DevGuard dg(t->device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	struct fsm_hip_text_spans *sp = new (std::nothrow) struct fsm_hip_text_spans;
	if (sp == nullptr) { errno = ENOMEM; return nullptr; }
	sp->device = t->device;
	sp->m = h->m;
	sp->t = t;
	sp->h = h;
	sp->starts = starts;
	sp->ends = ends;
	sp->s = static_cast<hipStream_t>(hip_stream);
	bool ok = HIP_OK(sp->ev[0].create()) && HIP_OK(sp->ev[1].create());
	if (ok && sp->m != 0)
		ok = HIP_OK(sp->d_p.alloc(sp->m)) && HIP_OK(sp->d_start.alloc(sp->m)) && HIP_OK(sp->d_end.alloc(sp->m)) && HIP_OK(sp->d_count.alloc(1)) &&
		     HIP_OK(hipStreamWaitEvent(sp->s, h->ev[5], 0)) &&                              /* the hits' lines (and, behind them, the text's offsets) first */
		     HIP_OK(hipMemsetAsync(sp->d_p, 0, sp->m * sizeof(uint64_t), sp->s));           /* round 0: p = 0 for every hit */
	ok = ok && spans_round(sp, false) == 0;
	if (ok) return sp;
	const int e = errno;
	(void)hipStreamSynchronize(sp->s);
	fsm_hip_text_spans_free(sp);
	errno = e;
	return nullptr;
}

extern "C" int fsm_hip_text_spans_next(struct fsm_hip_text_spans *sp)
{
	if (sp == nullptr) { errno = EINVAL; return -1; }
	DevGuard dg(sp->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	return spans_round(sp, true);
}

extern "C" size_t fsm_hip_text_spans_count(const struct fsm_hip_text_spans *sp)
{
	uint64_t c = 0;
	if (sp == nullptr || sp->m == 0) return 0;
	(void)copy_out(sp->device, sp->ev[1], {{&c, sp->d_count, sizeof c}});   /* c stays 0 when it fails */
	return (size_t)c;
}

extern "C" const uint64_t *fsm_hip_text_spans_start_device(const struct fsm_hip_text_spans *sp) { return sp == nullptr ? nullptr : sp->d_start.p; }
extern "C" const uint64_t *fsm_hip_text_spans_end_device(const struct fsm_hip_text_spans *sp) { return sp == nullptr ? nullptr : sp->d_end.p; }

extern "C" int fsm_hip_text_spans_copy(const struct fsm_hip_text_spans *sp, uint64_t *start, uint64_t *end)
{
	if (sp == nullptr) { errno = EINVAL; return -1; }
	return copy_out(sp->device, sp->ev[1], {{start, sp->d_start, sp->m * sizeof(uint64_t)}, {end, sp->d_end, sp->m * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_text_spans_ms(const struct fsm_hip_text_spans *sp)
{
	if (sp == nullptr) { errno = EINVAL; return -1.0; }
	return elapsed_ms(sp->device, sp->ev[1], {{sp->ev[0], sp->ev[1]}});
}

/* ---- what the tokens, the matches and the replacement share: the object's skeleton, the scan, the batch of a text --------------
 * Each is an object of NPASS passes on a stream with ONE wait in the middle: the passes before it leave counts, one workgroup
 * scans them, the host reads the total and sizes the arrays by it, the passes after it fill them and are in flight at return.
 * Their input is one LineBatch (line_batch.h), whichever of the three entry forms it came through. */

/* what every such object begins with: events ev[2p], ev[2p + 1] around pass p; the last one: all is there */
template <int NPASS>
struct __attribute__((visibility("hidden"))) RunObject {
	static constexpr int npass = NPASS;
	int device = 0;
	size_t m = 0;
	DevEvent ev[2 * NPASS];
	hipEvent_t done() const { return ev[2 * NPASS - 1]; }
	bool begin(int pass, hipStream_t s) { return HIP_OK(hipEventRecord(ev[2 * pass], s)); }
	bool end(int pass, hipStream_t s) { return HIP_OK(hipEventRecord(ev[2 * pass + 1], s)); }
};

namespace {

constexpr uint32_t SCAN_PER = 4;                            /* counts a thread of the scan takes a round: 4 096 a round trip */

__global__ void __launch_bounds__(1024)
counts_scan(uint64_t *cnt, uint64_t k)
{
	sum_scan<1024, 1, SCAN_PER>(cnt, k, cnt + k);
}

template <typename T>
void run_free(T *o)
{
	if (o == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(o->device);
		if (o->done() != nullptr) (void)hipEventSynchronize(o->done());
		delete o;
	}
	errno = e;
}

/* the object of a run of passes(o) on stream s over m inputs, `device` current; when the run fails, the stream is made idle
 * before what it has launched on is released */
template <typename T, typename Passes>
T *run_new(int device, uint64_t m, bool grid_fits, hipStream_t s, Passes passes)
{
	if (!grid_fits) { errno = ENOMEM; return nullptr; }
	T *o = new (std::nothrow) T;
	if (o == nullptr) { errno = ENOMEM; return nullptr; }
	o->device = device;
	o->m = (size_t)m;
	bool ok = true;
	for (DevEvent &ev : o->ev) ok = ok && HIP_OK(ev.create());
	if (ok && passes(o) == 0) return o;
	const int e = errno;
	(void)hipStreamSynchronize(s);
	run_free(o);
	errno = e;
	return nullptr;
}

/* A host form behind its checks: the batch staged on a stream of its own (never the NULL stream), the object of make(batch on
 * the device, stream), and a last wait, since the stream and the staged batch go at return: the last pass has read them. */
template <typename Make>
auto run_host(int device, const fsmhip::LineBatch &host, Make make) -> decltype(make(host, hipStream_t()))
{
	DevGuard dg(device);
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	DevStream own;
	if (!HIP_OK(own.create(hipStreamNonBlocking))) return nullptr;
	fsmhip::StagedBatch staged;
	fsmhip::LineBatch in;
	if (!staged.stage(host, own, &in)) return nullptr;
	auto *o = make(in, own);
	if (o == nullptr || HIP_OK(hipStreamSynchronize(own))) return o;   /* (null: run_new left the stream idle) */
	const int e = errno;
	run_free(o);
	errno = e;
	return nullptr;
}

/* passes from .. to by the object's events, summed */
template <typename T>
double run_ms(const T *o, int from, int to)
{
	if (o == nullptr || from < 0 || to >= T::npass) { errno = EINVAL; return -1.0; }
	EventPair pairs[T::npass];
	for (int p = from; p <= to; p++) pairs[p - from] = {o->ev[2 * p], o->ev[2 * p + 1]};
	return elapsed_ms(o->device, o->done(), pairs, (size_t)(to - from + 1));
}

/* The scan pass and the ONE wait of a run: cnt[0 .. k) scanned in place, exclusive, by one workgroup, the total in cnt[k] (k ==
 * 0: cnt[0] is cleared and nothing waits), `after` recorded, the total read back. */
int scan_total(uint64_t *cnt, uint64_t k, hipEvent_t after, hipStream_t s, uint64_t *total)
{
	*total = 0;
	if (k != 0) {
		hipLaunchKernelGGL(counts_scan, dim3(1), dim3(1024), 0, s, cnt, k);
		if (!HIP_OK(hipGetLastError())) return -1;
	} else if (!HIP_OK(hipMemsetAsync(cnt, 0, sizeof(uint64_t), s))) {
		return -1;
	}
	if (!HIP_OK(hipEventRecord(after, s))) return -1;
	if (k == 0) return 0;
	if (!HIP_OK(hipMemcpyAsync(total, cnt + k, sizeof *total, hipMemcpyDeviceToHost, s))) return -1;
	return HIP_OK(hipStreamSynchronize(s)) ? 0 : -1;
}

/* The lines of a text, or (h != null) of its hits, as a batch for a front on stream s: every object of `devices` is on the
 * text's device, which *dg makes current for the caller; the stream waits for the hits' lines (and, behind them, the text's
 * offsets).  false + errno. */
bool text_batch(const struct fsm_hip_text *t, const struct fsm_hip_text_hits *h, std::initializer_list<int> devices, hipStream_t s,
	std::optional<DevGuard> *dg, fsmhip::LineBatch *in)
{
	for (int d : devices)
		if (d != t->device) { errno = EINVAL; return false; }
	if (h != nullptr && h->device != t->device) { errno = EINVAL; return false; }
	dg->emplace(t->device);
	if (!(*dg)->ok()) { errno = ENODEV; return false; }
	if (!HIP_OK(hipStreamWaitEvent(s, h != nullptr ? h->ev[5] : t->ev[3], 0))) return false;
	in->base = t->d_text;
	in->off = t->d_off;
	in->n = t->n;
	in->pick = h != nullptr ? h->d_lines.p : nullptr;
	in->m = h != nullptr ? h->m : t->n;
	in->limit = t->nbytes;
	in->has_limit = true;
	in->trim = t->delim;
	return true;
}

}   // namespace

/* ---- tokens: every line cut into longest-match tokens (tok.hip, walk_tok) ------------------------------------------------
 * count pass -> exclusive scan of the counts by one workgroup -> ONE wait for the total -> allocation -> emit pass.  The counts
 * are scanned in place: d_off is count[m] first, tok_off[m + 1] afterwards (the total lands in its last entry). */
struct __attribute__((visibility("hidden"))) fsm_hip_tokens : RunObject<3> {   /* the count pass, the scan, the emit pass */
	size_t total = 0;
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_err;                  /* m */
	DevBuf<uint64_t> d_end;                  /* total */
	DevBuf<uint32_t> d_id;                   /* total */
};

extern "C" void fsm_hip_tokens_free(struct fsm_hip_tokens *tk) { run_free(tk); }

/* the passes on stream s into *tk, the image's device current; r: the inputs (its outputs are set here) */
static int tokens_passes(struct fsm_hip_tokens *tk, const struct fsm_hip_tok_dfa *td, fsmhip::TokRun r, hipStream_t s)
{
	const uint64_t m = r.in.m;
	uint64_t total = 0;
	if (!HIP_OK(tk->d_off.alloc(m + 1u))) return -1;
	if (m != 0 && !HIP_OK(tk->d_err.alloc(m))) return -1;
	r.count = tk->d_off;
	r.err = tk->d_err;
	if (!tk->begin(0, s)) return -1;
	if (m != 0 && fsmhip::tok_launch(td, r, false, s) != 0) return -1;
	if (!tk->end(0, s) || !tk->begin(1, s)) return -1;
	if (scan_total(tk->d_off, m, tk->ev[3], s, &total) != 0) return -1;   /* the total sizes the arrays */
	tk->total = (size_t)total;
	if (total != 0 && (!HIP_OK(tk->d_end.alloc(total)) || !HIP_OK(tk->d_id.alloc(total)))) return -1;
	if (!tk->begin(2, s)) return -1;
	if (total != 0) {
		r.tok_off = tk->d_off;
		r.end_out = tk->d_end;
		r.id_out = tk->d_id;
		if (fsmhip::tok_launch(td, r, true, s) != 0) return -1;
	}
	return tk->end(2, s) ? 0 : -1;
}

static struct fsm_hip_tokens *tokens_new(const struct fsm_hip_tok_dfa *td, const fsmhip::LineBatch &in, hipStream_t s)
{
	fsmhip::TokRun r;
	r.in = in;
	return run_new<struct fsm_hip_tokens>(fsmhip::tok_dfa_device(td), in.m, (in.m + fsmhip::TOK_THREADS - 1u) / fsmhip::TOK_THREADS <= 0x7fffffffu, s,
	                                      [&](struct fsm_hip_tokens *tk) { return tokens_passes(tk, td, r, s); });
}

/* the arguments both forms refuse alike; *in: the batch as given */
static bool tokens_check(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_tok_batch *b, fsmhip::LineBatch *in)
{
	if (!have_device()) { errno = ENODEV; return false; }
	if (td == nullptr) { errno = EINVAL; return false; }
	return fsmhip::batch_shape(b, FSM_HIP_TOKENS_NO_BACKTRACK | FSM_HIP_TOKENS_SKIP_BAD, in);
}

extern "C" struct fsm_hip_tokens *fsm_hip_tokens_run_device(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_tok_batch *b, void *hip_stream)
{
	fsmhip::LineBatch in;
	if (!tokens_check(td, b, &in) || !fsmhip::batch_device_ok(in)) return nullptr;
	DevGuard dg(fsmhip::tok_dfa_device(td));
	if (!dg.ok()) { errno = ENODEV; return nullptr; }
	return tokens_new(td, in, static_cast<hipStream_t>(hip_stream));
}

extern "C" struct fsm_hip_tokens *fsm_hip_tokens_run(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_tok_batch *b)
{
	fsmhip::LineBatch host;
	if (!tokens_check(td, b, &host) || !fsmhip::batch_host_arrays_ok(host)) return nullptr;
	return run_host(fsmhip::tok_dfa_device(td), host, [&](const fsmhip::LineBatch &in, hipStream_t s) { return tokens_new(td, in, s); });
}

extern "C" struct fsm_hip_tokens *fsm_hip_text_tokens(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *h,
	unsigned flags, void *hip_stream)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }
	if (td == nullptr || t == nullptr || (flags & ~(FSM_HIP_TOKENS_NO_BACKTRACK | FSM_HIP_TOKENS_SKIP_BAD)) != 0u) { errno = EINVAL; return nullptr; }
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	std::optional<DevGuard> dg;
	fsmhip::LineBatch in;
	if (!text_batch(t, h, {fsmhip::tok_dfa_device(td)}, s, &dg, &in)) return nullptr;
	in.flags = flags;
	return tokens_new(td, in, s);
}

extern "C" size_t fsm_hip_tokens_count(const struct fsm_hip_tokens *tk) { return tk == nullptr ? 0 : tk->m; }
extern "C" size_t fsm_hip_tokens_total(const struct fsm_hip_tokens *tk) { return tk == nullptr ? 0 : tk->total; }
extern "C" const uint64_t *fsm_hip_tokens_off_device(const struct fsm_hip_tokens *tk) { return tk == nullptr ? nullptr : tk->d_off.p; }
extern "C" const uint64_t *fsm_hip_tokens_end_device(const struct fsm_hip_tokens *tk) { return tk == nullptr ? nullptr : tk->d_end.p; }
extern "C" const uint32_t *fsm_hip_tokens_id_device(const struct fsm_hip_tokens *tk) { return tk == nullptr ? nullptr : tk->d_id.p; }
extern "C" const uint64_t *fsm_hip_tokens_err_device(const struct fsm_hip_tokens *tk) { return tk == nullptr ? nullptr : tk->d_err.p; }

extern "C" int fsm_hip_tokens_copy(const struct fsm_hip_tokens *tk, uint64_t *off, uint64_t *end, uint32_t *id, uint64_t *err)
{
	if (tk == nullptr) { errno = EINVAL; return -1; }
	return copy_out(tk->device, tk->done(), {{off, tk->d_off, (tk->m + 1u) * sizeof(uint64_t)}, {end, tk->d_end, tk->total * sizeof(uint64_t)},
	                                         {id, tk->d_id, tk->total * sizeof(uint32_t)}, {err, tk->d_err, tk->m * sizeof(uint64_t)}});
}

extern "C" double fsm_hip_tokens_ms(const struct fsm_hip_tokens *tk) { return run_ms(tk, 0, 2); }
extern "C" double fsm_hip_tokens_pass_ms(const struct fsm_hip_tokens *tk, int pass) { return run_ms(tk, pass, pass); }

/* ---- matches: every match of every line (match.hip, walk_mark / walk_match) -------------------------------------------------
 * marks pass -> count pass -> exclusive scan of the counts by one workgroup -> ONE wait for the total -> allocation -> emit
 * pass.  The counts are scanned in place, as the tokens' are: d_off is count[m] first, match_off[m + 1] afterwards. */
struct __attribute__((visibility("hidden"))) fsm_hip_matches : RunObject<4> {   /* the marks pass, the count pass, the scan, the emit pass */
	size_t total = 0;
	DevBuf<uint16_t> d_marks;                /* marks_words(limit, n): internal */
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_start, d_end;         /* total each */
	DevBuf<uint32_t> d_id;                   /* total */
};

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

/* ---- replace: every match replaced by its rule's replacement, a fresh packed text (replace.hip) --------------------------------
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

/* ---- extract: every kept match's bytes as a record of a fresh packed text (extract.hip) -----------------------------------------
 * lengths pass (per MATCH: kept, the record's bytes, its first byte, its input; per block of EXT_MATCHES matches the pair records /
 * bytes) -> exclusive scan of the BLOCK pairs by one workgroup -> ONE wait for the two totals -> allocation -> offsets pass (the
 * block's own scan redone, the compaction, first[]) -> write pass.  The scan runs over total / EXT_MATCHES records.  The offsets
 * and the write pass are in flight at return. */
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

struct __attribute__((visibility("hidden"))) fsm_hip_extracted : RunObject<4> {   /* the lengths, the scan, the offsets, the write pass */
	size_t nrec = 0;
	uint64_t nbytes = 0;
	int sep = -1;                            /* the separator the records were made with */
	DevBuf<uint64_t> d_off;                  /* nrec + 1 */
	DevBuf<uint64_t> d_line, d_match;        /* nrec */
	DevBuf<uint64_t> d_src;                  /* nrec: internal */
	DevBuf<uint64_t> d_mrec, d_msrc, d_mline;   /* one per match: internal */
	DevBuf<uint64_t> d_pairs;                /* per block of matches, + the totals: internal */
	DevBuf<uint64_t> d_first;                /* per block of the output, + 1: internal */
	DevBuf<unsigned char> d_bytes;           /* nbytes, in whole blocks */
};

extern "C" void fsm_hip_extracted_free(struct fsm_hip_extracted *x) { run_free(x); }

namespace {

__global__ void __launch_bounds__(1024)
pairs_scan(uint64_t *pairs, uint64_t nblocks)
{
	sum_scan<1024, 2, SCAN_PER>(pairs, nblocks, pairs + 2u * nblocks);
}

}   // namespace

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
	if (nblocks != 0) {
		hipLaunchKernelGGL(pairs_scan, dim3(1), dim3(1024), 0, s, r.pairs, nblocks);
		if (!HIP_OK(hipGetLastError())) return -1;
	}
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

/* ---- tally: counts of entries and of inputs per group and per rule (tally.hip, tally_spans) --------------------------------------
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

/* ---- distinct: the distinct records of a packed text with their counts (distinct.hip) ---------------------------------------------
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
};

extern "C" void fsm_hip_distinct_free(struct fsm_hip_distinct *dx) { run_free(dx); }

/* the passes on stream s into *dx, its device current; r: the packed text, the bytes and the flag (the rest is set here) */
static int distinct_passes(struct fsm_hip_distinct *dx, fsmhip::DstRun r, bool text, hipStream_t s)
{
	if (r.R == 0) {                                  /* no record: doff[0] alone, and nothing is launched */
		if (text && (!HIP_OK(dx->d_doff.alloc(1)) || !HIP_OK(hipMemsetAsync(dx->d_doff.p, 0, sizeof(uint64_t), s)))) return -1;
		for (DevEvent &ev : dx->ev)
			if (!HIP_OK(hipEventRecord(ev, s))) return -1;
		return 0;
	}
	const uint64_t nblocks = fsmhip::dst_blocks(r.R);
	uint64_t tot[3] = {0, 0, 0};                     /* the firsts, the key bytes, the bytes that may be read */
	r.slots = fsmhip::dst_table_slots(r.R);
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
	hipLaunchKernelGGL(pairs_scan, dim3(1), dim3(1024), 0, s, r.pairs, nblocks);
	if (!HIP_OK(hipGetLastError())) return -1;
	if (!dx->end(2, s)) return -1;
	/* the ONE wait: D sizes first and count, the bytes the text of the keys */
	if (!HIP_OK(hipMemcpyAsync(tot, r.pairs + 2u * nblocks, sizeof tot, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return -1;
	dx->D = (size_t)tot[0];
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
