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
 * Behind the text come its hits, their context, the files and the spans; at the end, the two scans that the objects of the other
 * units run between their passes (front.h declares them): their kernels instantiate the sum_scan of this file.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/fsm_hip.h"
#include "front.h"
#include "span.h"
#include "text_objects.h"

namespace {

constexpr uint32_t TEXT_WAVES = 4;                          /* wavefronts per workgroup */
constexpr uint32_t TEXT_THREADS = TEXT_WAVES * 64u;
constexpr uint32_t TEXT_TILES = 4;                          /* 16-byte loads a lane keeps in flight */
constexpr uint32_t TEXT_TILE = TEXT_THREADS * 16u;          /* bytes one load instruction of the workgroup covers */
constexpr uint32_t TEXT_BLOCK = TEXT_TILES * TEXT_TILE;     /* bytes a workgroup scans per step: 16 KiB */

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

}   // namespace

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

/* ---- the scans between the passes of the other units' objects (front.h): counts, and pairs of words -------------------------- */
namespace {

constexpr uint32_t SCAN_PER = 4;                            /* counts a thread of the scan takes a round: 4 096 a round trip */

__global__ void __launch_bounds__(1024)
counts_scan(uint64_t *cnt, uint64_t k)
{
	sum_scan<1024, 1, SCAN_PER>(cnt, k, cnt + k);
}

__global__ void __launch_bounds__(1024)
pairs_scan(uint64_t *pairs, uint64_t nblocks)
{
	sum_scan<1024, 2, SCAN_PER>(pairs, nblocks, pairs + 2u * nblocks);
}

}   // namespace

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

int pairs_scan_launch(uint64_t *pairs, uint64_t nblocks, hipStream_t s)
{
	if (nblocks == 0) return 0;
	hipLaunchKernelGGL(pairs_scan, dim3(1), dim3(1024), 0, s, pairs, nblocks);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}
