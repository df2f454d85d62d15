/*
 * tok.hip -- tokens: every line cut into longest-match tokens with the end-id of the state each was accepted in, the whole
 * line in ONE launch.
 *
 * The classic loop around a DFA in a lexer (what the reference's lx generates, src/lx/print/c.c, the z*() functions): at a
 * cursor p walk from the start state until the walk stops, take the longest accepted prefix as a token, put the cursor behind
 * it, again.  span.hip's walk_pos delivers one such match per launch and no state; here every lane carries its own cursor and
 * restarts by itself, so a line of k tokens costs no host round at all.  include/fsm_hip.h, section "tokens", is the definition.
 *
 * walk_tok<EMIT> has walk_pos's shape: one workgroup = 256 consecutive inputs, one input per lane, the table copied to LDS
 * once (the image of image.h build_tok_image: the end bit rides in every entry), the input taken in 16-byte chunks by an
 * unaligned global load, the sixteen class lookups issued together, then the chain of sixteen dependent table lookups.  Beside
 * the chain -- never on it -- a lane keeps what a lexer must remember: the state and the byte count of the last accept (two
 * selects on the entry's end bit) and the count of steps that ended in a non-absorbing state (where the walk stopped, for
 * FSM_HIP_TOKENS_NO_BACKTRACK).  After a chunk a lane whose walk stopped -- DEAD, an absorbing state, the line's end --
 * closes its attempt (a token, or a bad byte), moves its cursor and starts again from the start state in the next turn; the
 * other lanes go on with their next chunk.  No branch per byte; the turn ends when no lane has bytes left.
 * EMIT = false counts (count[j], err[j]); the front scans the counts; EMIT = true walks again and stores end / id at
 * tok_off[j] + t, never more than tok_off[j + 1] - tok_off[j] of them: if the text changed between the passes the result is
 * wrong, not overrun.  Nothing outside [base, base + limit) is read (walk_pos's clipping rule).  Every pointer names its
 * address space (no FLAT instruction: tests/test_abi.py).
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <vector>

#include "../../include/fsm_hip.h"
#include "dfa_access.h"
#include "front.h"
#include "image.h"
#include "text_objects.h"
#include "tok.h"

namespace fsmhip {

constexpr uint32_t TOK_THREADS = 256;        /* inputs per workgroup, one per lane */

/* one pass over m inputs; every pointer is device memory */
struct TokRun {
	LineBatch in;                            /* flags: FSM_HIP_TOKENS_* */
	uint64_t *count = nullptr, *err = nullptr;           /* the count pass writes them: m each */
	const uint64_t *tok_off = nullptr;                   /* the emit pass reads it: m + 1 */
	uint64_t *end_out = nullptr;                         /* ... and stores at tok_off[j] + t */
	uint32_t *id_out = nullptr;
};

}

using namespace fsmhip;

namespace {

static_assert(TOK_THREADS == 256, "one thread per byte value copies the class map");

typedef uint32_t u32x4t __attribute__((ext_vector_type(4)));

/* the launch's arguments, by value: every pointer is device memory */
struct TokArgs {
	const void *tab;         /* [entries]: u16 (LDS form) or u32, the end-state bit of the target folded in */
	const uint16_t *col;     /* [256] */
	const uint32_t *ids;     /* by TokImage::id_index() */
	const uint8_t *base;
	const uint64_t *off, *pick;
	uint64_t *count, *err;
	const uint64_t *tok_off;
	uint64_t *end_out;
	uint32_t *id_out;
	uint64_t n, m, limit;
	uint32_t entries, C;
	uint32_t start, abs_min, dead;   /* in the walk's unit (TokImage) */
	uint32_t in_lds, has_limit, flags;
	int32_t trim;
};

__device__ __forceinline__ uint32_t tok_byte_at(const u32x4t &w, int k)
{
	const uint32_t d = (k < 4) ? w.x : (k < 8) ? w.y : (k < 12) ? w.z : w.w;
	return (d >> (8 * (k & 3))) & 0xffu;
}

template <bool EMIT>
__global__ void __launch_bounds__(TOK_THREADS)
walk_tok(const TokArgs a)
{
	typedef const uint16_t __attribute__((address_space(1))) *g_u16p;
	typedef const uint32_t __attribute__((address_space(1))) *g_u32p;
	typedef const uint64_t __attribute__((address_space(1))) *g_u64p;
	typedef const uint8_t __attribute__((address_space(1))) *g_u8p;
	typedef uint64_t __attribute__((address_space(1))) *g_u64w;
	typedef uint32_t __attribute__((address_space(1))) *g_u32w;
	typedef u32x4t __attribute__((aligned(1))) u32x4_any;
	typedef const u32x4_any __attribute__((address_space(1))) *g_chunkp;
	typedef const uint16_t __attribute__((address_space(3))) *l_u16p;
	__shared__ uint16_t col[256];
	__shared__ uint16_t tab[TOK_LDS_ENTRIES];
	const uint32_t tid = threadIdx.x;
	const bool in_lds = a.in_lds != 0u;
	const uint32_t C = a.C;
	col[tid] = ((g_u16p)(uintptr_t)a.col)[tid];
	if (in_lds)
		for (uint32_t e = tid; e < a.entries; e += TOK_THREADS) tab[e] = ((g_u16p)(uintptr_t)a.tab)[e];
	__syncthreads();

	const g_u64p off = (g_u64p)(uintptr_t)a.off;
	const g_u32p dense = (g_u32p)(uintptr_t)a.tab;
	const g_u32p ids = (g_u32p)(uintptr_t)a.ids;
	const uint64_t base = reinterpret_cast<uint64_t>(a.base);
	const uint64_t j = (uint64_t)blockIdx.x * TOK_THREADS + tid;
	const bool valid = j < a.m;
	uint64_t i = j;
	if (valid && a.pick != nullptr) i = ((g_u64p)(uintptr_t)a.pick)[j];
	const bool have = valid && i < a.n;              /* a pick beyond the lines: no token, nothing read */
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
	uint64_t cap = 0, out_at = 0;                    /* EMIT: the lane's slots */
	if (EMIT && valid) {
		out_at = ((g_u64p)(uintptr_t)a.tok_off)[j];
		const uint64_t nx = ((g_u64p)(uintptr_t)a.tok_off)[j + 1u];
		cap = nx > out_at ? nx - out_at : 0u;
	}
	const g_u64w end_out = (g_u64w)(uintptr_t)a.end_out;
	const g_u32w id_out = (g_u32w)(uintptr_t)a.id_out;

	const uint32_t end_bit = in_lds ? 1u : 0x80000000u;
	const uint32_t absorbing = a.abs_min;            /* (even in the LDS form: comparing the state with its bit still on is the same) */
	const bool no_backtrack = (a.flags & FSM_HIP_TOKENS_NO_BACKTRACK) != 0u, skip_bad = (a.flags & FSM_HIP_TOKENS_SKIP_BAD) != 0u;
	const uint32_t col_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)col;
	const uint32_t tab_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)tab;

	uint64_t p = 0;                                  /* the cursor: the attempt's first byte */
	uint64_t t = 0;                                  /* bytes of the attempt walked in earlier chunks */
	uint64_t acc = 0;                                /* the attempt's last accept: bytes from p (0: none; the start state does not count) */
	uint32_t accs = 0;                               /* ... and the state there */
	uint32_t s = a.start;
	uint64_t ntok = 0, err = FSM_HIP_NO_POS;

	for (;;) {
		const bool live = p < len;
		if (!__any(live)) break;
		const uint64_t left = live ? len - p - t : 0u;   /* > 0 in a live lane: an attempt that reached len was closed */
		const uint32_t cnt = left < 16u ? (uint32_t)left : 16u;
		u32x4t w = {0u, 0u, 0u, 0u};
		if (live) {
			const uint64_t at = beg + p + t;         /* the chunk's first byte, from base */
			if (at + 16u <= limit) {
				w = *(g_chunkp)(base + at);
			} else {
				uint32_t d[4] = {0u, 0u, 0u, 0u};
				for (uint32_t k = 0; k < cnt; k++) d[k >> 2] |= (uint32_t)((g_u8p)(base + at))[k] << ((k & 3u) * 8u);
				w = u32x4t{d[0], d[1], d[2], d[3]};
			}
		}
		uint32_t c2[16];
#pragma unroll
		for (int k = 0; k < 16; k++) c2[k] = *(l_u16p)(uintptr_t)(col_at + tok_byte_at(w, k) * 2u);
		uint32_t acck = 0;                           /* bytes of this chunk at the last accept in it (0: none) */
		uint32_t as = accs;
		uint32_t nl = 0;                             /* steps of this chunk that ended in a non-absorbing state: they come first */
		if (in_lds) {
			if (__all(cnt == 16u || cnt == 0u)) {    /* whole chunks everywhere */
				uint32_t sn = s;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					sn = *(l_u16p)(uintptr_t)(tab_at + (sn & 0xfffeu) + c2[k]);
					const bool hit = (sn & 1u) != 0u;
					as = hit ? sn : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
					nl += sn < absorbing ? 1u : 0u;
				}
				s = cnt != 0u ? sn : s;
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const uint32_t sn = *(l_u16p)(uintptr_t)(tab_at + (s & 0xfffeu) + c2[k]);
					const bool in = (uint32_t)k < cnt;
					const bool hit = in && (sn & 1u) != 0u;
					s = in ? sn : s;
					as = hit ? sn : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
					nl += in && sn < absorbing ? 1u : 0u;
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) {
				if ((uint32_t)k < cnt) {
					s = dense[(uint64_t)(s & 0x7fffffffu) * C + c2[k]];
					const bool hit = (s >> 31) != 0u;
					as = hit ? s : as;
					acck = hit ? (uint32_t)(k + 1) : acck;
					nl += (s & 0x7fffffffu) < absorbing ? 1u : 0u;
				}
			}
		}
		if (live) {
			if (acck != 0u) { acc = t + acck; accs = as; }
			const uint32_t sc = s & ~end_bit;
			const bool absorbed = sc >= absorbing, s_ends = (s & end_bit) != 0u;
			if (absorbed || cnt == left) {           /* the walk stopped: close the attempt */
				uint64_t e;                              /* the token's bytes; 0: none */
				uint32_t q = accs;
				if (absorbed && s_ends) {                /* an absorbing end state */
					q = s;
					e = no_backtrack ? t + nl + 1u : len - p;    /* where it was entered : it accepts at every later position */
				} else if (no_backtrack) {
					/* stop: the bytes consumed; the byte with the missing edge is not */
					const uint64_t stop = t + nl + (absorbed && sc != a.dead ? 1u : 0u);
					e = acc == stop ? acc : 0u;
				} else {
					e = acc;
				}
				const bool bad = e == 0u;                /* no token at p */
				if (bad && err == FSM_HIP_NO_POS) err = p;
				if (!bad || skip_bad) {
					if (bad) e = 1u;                     /* the bad byte as a one-byte token */
					if (EMIT && ntok < cap) {
						end_out[out_at + ntok] = p + e;
						id_out[out_at + ntok] = bad ? FSM_HIP_NO_MATCH : ids[in_lds ? q >> 1 : q & 0x7fffffffu];
					}
					ntok++;
					p += e;                              /* at least one byte on */
				} else {
					p = len;                             /* the line stops here */
				}
				t = 0;
				acc = 0;
				s = a.start;
			} else {
				t += 16u;
			}
		}
	}
	if (!EMIT && valid) {
		((g_u64w)(uintptr_t)a.count)[j] = ntok;
		((g_u64w)(uintptr_t)a.err)[j] = err;
	}
}

}   // namespace

/* the type is the library's own: its destructor is no exported symbol */
struct __attribute__((visibility("hidden"))) fsm_hip_tok_dfa {
	int device = 0;
	uint32_t entries = 0, C = 0, start = 0, abs_min = 0, dead = 0, in_lds = 0;
	DevBuf<unsigned char> d_tab;
	DevBuf<uint16_t> d_col;
	DevBuf<uint32_t> d_ids;                          /* device memory: read once per token, not per byte */
};

namespace fsmhip {

int tok_dfa_device(const fsm_hip_tok_dfa *td) { return td->device; }

TokView tok_dfa_view(const fsm_hip_tok_dfa *td)
{
	TokView v;
	v.tab = td->d_tab.p;
	v.col = td->d_col.p;
	v.ids = td->d_ids.p;
	v.entries = td->entries;
	v.C = td->C;
	v.start = td->start;
	v.abs_min = td->abs_min;
	v.in_lds = td->in_lds;
	return v;
}

/* walk_tok<emit> on stream s, td's device current; 0, or -1 + errno */
static int tok_launch(const fsm_hip_tok_dfa *td, const TokRun &r, bool emit, hipStream_t s)
{
	if (r.in.m == 0) return 0;
	if ((r.in.m + TOK_THREADS - 1u) / TOK_THREADS > 0x7fffffffu) { errno = ENOMEM; return -1; }
	TokArgs a;
	a.tab = td->d_tab.p;
	a.col = td->d_col.p;
	a.ids = td->d_ids.p;
	a.base = static_cast<const uint8_t *>(r.in.base);
	a.off = r.in.off;
	a.pick = r.in.pick;
	a.count = r.count;
	a.err = r.err;
	a.tok_off = r.tok_off;
	a.end_out = r.end_out;
	a.id_out = r.id_out;
	a.n = r.in.n;
	a.m = r.in.m;
	a.limit = r.in.limit;
	a.entries = td->entries;
	a.C = td->C;
	a.start = td->start;
	a.abs_min = td->abs_min;
	a.dead = td->dead;
	a.in_lds = td->in_lds;
	a.has_limit = r.in.has_limit ? 1u : 0u;
	a.flags = r.in.flags;
	a.trim = r.in.trim;
	const dim3 grid((unsigned)((r.in.m + TOK_THREADS - 1u) / TOK_THREADS)), block(TOK_THREADS);
	if (emit) hipLaunchKernelGGL(walk_tok<true>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(walk_tok<false>, grid, block, 0, s, a);
	return HIP_OK(hipGetLastError()) ? 0 : -1;
}

}   // namespace fsmhip

extern "C" struct fsm_hip_tok_dfa *fsm_hip_tok_dfa_create(const struct fsm_hip_dfa *dfa, int ids_mode)
{
	if (!have_device()) { errno = ENODEV; return nullptr; }   /* no CPU path, as everywhere in this library */
	if (dfa == nullptr) { errno = EINVAL; return nullptr; }
	TokImage im;
	const int r = build_tok_image(*dfa_plan(dfa), ids_mode, im);
	if (r != 0) { errno = r; return nullptr; }
	struct fsm_hip_tok_dfa *td = new (std::nothrow) fsm_hip_tok_dfa;
	if (td == nullptr) { errno = ENOMEM; return nullptr; }
	td->device = dfa_device(dfa);
	td->entries = im.entries;
	td->C = im.C;
	td->start = im.start;
	td->abs_min = im.abs_min;
	td->dead = im.dead;
	td->in_lds = im.in_lds ? 1u : 0u;
	bool ok = true;
	DevGuard dg(td->device);
	if (!dg.ok()) { errno = ENODEV; ok = false; }
	if (im.in_lds) ok = ok && HIP_OK(td->d_tab.upload_bytes(im.tab16.data(), im.tab16.size() * sizeof(uint16_t), 16));
	else ok = ok && HIP_OK(td->d_tab.upload_bytes(im.tab32.data(), im.tab32.size() * sizeof(uint32_t), 16));
	ok = ok && HIP_OK(td->d_col.upload(im.col)) && HIP_OK(td->d_ids.upload(im.ids));
	if (ok) return td;
	const int e = errno;
	delete td;
	errno = e;
	return nullptr;
}

extern "C" void fsm_hip_tok_dfa_free(struct fsm_hip_tok_dfa *td)
{
	if (td == nullptr) return;
	const int e = errno;
	{
		DevGuard dg(td->device);
		delete td;                                   /* (hipFree waits for the device: no walk still reads the image) */
	}
	errno = e;
}

extern "C" int fsm_hip_tok_dfa_in_lds(const struct fsm_hip_tok_dfa *td) { return td != nullptr && td->in_lds != 0u ? 1 : 0; }

/* ---- the tokens object (tok.h): count pass -> scan -> ONE wait for the total -> allocation -> emit pass (front.h) ---------------- */
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
