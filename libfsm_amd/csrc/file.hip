/*
 * file.hip -- the large-input front: ONE input (a file, a big buffer) walked by the whole device.
 *
 * fsm_vm_match_file() keeps a struct vm_state across 4 KiB fread()s and stops reading as soon as the VM has decided
 * (src/libfsm/vm.c:188-216); re(1) -x hands it every file named on the command line (src/re/main.c:1106-1181).  A DFA walk
 * over one input is a dependent chain -- one lane, ~100 ns a byte: rounds 2-5 carried the state through
 * fsm_hip_exec_batch_resume() 64 KiB at a time and managed ~10 MB/s, seventy times slower than the reference's VM on one
 * host core.  Here the input is cut into CHUNK-byte pieces that are walked AT ONCE, one per lane, each from a GUESSED
 * state, and the guesses are corrected until they stand:
 *     in[0] = the state carried into the window, in[i] = START            (first pass)
 *     out[i] = delta*(in[i], piece i)                                      one fsm_hip_exec_batch_resume_device over all pieces
 *     in'[i] = out[i - 1]; stop when in' == in                             (the host compares two small arrays)
 * At the fixed point in[i] is delta*(carry, pieces 0 .. i-1) for every i -- by induction over i, whatever the guesses were
 * -- so the answer is exactly the sequential walk's.  Every pass makes at least one more piece right (piece 0 is right from
 * the start), so there are at most n passes: the bound is the sequential cost.  What makes it fast is that a DFA built from a
 * pattern FORGETS: walking a KiB of text from START and from the true state nearly always ends in the same state, so the
 * second pass already stands (a counter such as (aa)* does not forget and pays pass after pass; it is no slower than before).
 * The window's bytes cross PCIe once; the passes re-read them from HBM at the fixed-stride kernels' rate.
 * Reading stops once the state can no longer change -- DEAD (a missing edge: the VM's STOP fail) or an absorbing state (its
 * STOP success shortcut, vm/ir.c:763-766).  A read error gives 0, as the reference's ferror() check does.
 *
 * With eager-output sets (fsm_hip_match_file_eager / _buffer_big_eager): the same passes through the resumed eager walk,
 * one set per piece in device memory (zeroed before each pass).  Two rules keep the answer exact.  A guess must not emit:
 * a piece walked from FSM_HIP_STATE_START would fire the start state's outputs in the middle of the input, so pieces i >= 1
 * are guessed from the start state by its caller's id, whose outputs do not fire (only piece 0 of the first window starts
 * from START).  And the sets of wrong guesses are thrown away: only at the fixed point, where every piece has walked from
 * its true in-state, are the window's per-piece sets OR-ed into one accumulated set on the device (walk_or_rows below).
 * A state's outputs fire when it is entered, so a piece that starts in a state adds nothing for it: the set over the whole
 * input is the OR of the pieces' sets, and stopping at DEAD or an absorbing state loses nothing.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fsm_hip.h"
#include "dfa_access.h"
#include "hip_host.h"

using namespace fsmhip;

namespace {

constexpr size_t CHUNK = 1024;                 /* bytes a lane walks per pass */
constexpr size_t WINDOW = (size_t)32 << 20;    /* bytes staged per window (two of them in flight: read k + 1 while k is walked) */
constexpr size_t SMALL = (size_t)256 << 10;    /* an input up to this size is one plain call */

/* eager: n rows of W words (the window's per-piece sets) OR-ed into acc[0 .. W): one workgroup per word, each thread a
 * strided slice of the rows, a cross-lane and a cross-wave reduction, one vector store per word -- a single writer per word
 * on one stream, no atomics.  Every global load and store names its address space (no FLAT access: tests/test_abi.py). */
__global__ void __launch_bounds__(256) walk_or_rows(const uint64_t *rows, uint32_t n, uint32_t W, uint64_t *acc)
{
	typedef const uint64_t __attribute__((address_space(1))) *glb_u64p;
	typedef uint64_t __attribute__((address_space(1))) *glb_u64w;
	__shared__ uint64_t part[4];
	const uint32_t w = blockIdx.x;
	uint64_t v = 0;
	for (uint32_t i = threadIdx.x; i < n; i += 256u) v |= *(glb_u64p)(uintptr_t)(rows + (size_t)i * W + w);
	uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
	for (int o = 32; o > 0; o >>= 1) {
		lo |= (uint32_t)__shfl_xor((int)lo, o, 64);
		hi |= (uint32_t)__shfl_xor((int)hi, o, 64);
	}
	if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = (uint64_t)hi << 32 | lo;
	__syncthreads();
	if (threadIdx.x == 0) {
		glb_u64w dst = (glb_u64w)(uintptr_t)(acc + w);
		*dst = *dst | part[0] | part[1] | part[2] | part[3];
	}
}

/* a failing HIP call inside the file engine is EIO, never EINVAL: EINVAL here means the caller's arguments */
bool file_ok(hipError_t e, const char *what) { const bool ok = hip_ok(e, what); if (!ok && errno == EINVAL) errno = EIO; return ok; }
#define FILE_OK(expr) file_ok((expr), #expr)

struct Engine {
	const fsm_hip_dfa *d;
	DevGuard dg;                                    /* first: the caller's device comes back after everything below has gone */
	PinBuf<unsigned char> pin[2];
	DevBuf<unsigned char> dbuf[2];
	DevBuf<uint32_t> d_st;                          /* states: device array, pinned host copies */
	PinBuf<uint32_t> h_in, h_out;
	unsigned passes = 0, windows = 0;
	size_t W = 0;                                   /* eager: words per set (0: the plain walk) */
	DevBuf<uint64_t> d_sets, d_acc;                 /* eager: one set per piece of a window; the set of the windows walked so far */
	uint32_t guess = FSM_HIP_STATE_START;           /* where pieces i >= 1 start on the first pass */
	DevStream s;                                    /* last: it goes first, once ~Engine has waited for it */

	explicit Engine(const fsm_hip_dfa *dfa) : d(dfa), dg(dfa_device(dfa)) {}
	int open(size_t eager_words)
	{
		if (!dg.ok()) { errno = ENODEV; return -1; }
		if (!FILE_OK(s.create(hipStreamNonBlocking))) return -1;
		for (int k = 0; k < 2; k++) {
			if (!FILE_OK(pin[k].alloc(WINDOW))) return -1;
			if (!FILE_OK(dbuf[k].alloc(WINDOW))) return -1;
		}
		const size_t n = WINDOW / CHUNK;
		if (!FILE_OK(d_st.alloc(n))) return -1;
		if (!FILE_OK(h_in.alloc(n))) return -1;
		if (!FILE_OK(h_out.alloc(n))) return -1;
		W = eager_words;
		if (W != 0) {
			if (!FILE_OK(d_sets.alloc(n * W))) return -1;
			if (!FILE_OK(d_acc.alloc(W))) return -1;
			if (!FILE_OK(hipMemsetAsync(d_acc, 0, W * sizeof(uint64_t), s))) return -1;
			const Plan *p = dfa_plan(d);
			guess = p->new2old[p->start];   /* the start state by its caller's id: a guess must not fire its outputs */
		}
		return 0;
	}
	/* nothing goes while the stream still works */
	~Engine() { if (s) { const int e = errno; (void)hipStreamSynchronize(s); errno = e; } }
	/* the window's bytes on their way to the device (returns at once) */
	int upload(int k, size_t bytes)
	{
		if (!FILE_OK(hipMemcpyAsync(dbuf[k], pin[k], bytes, hipMemcpyHostToDevice, s))) return -1;
		return 0;
	}
	/* n whole pieces of window k, from `carry`: the state after them */
	int walk(int k, size_t n, uint32_t carry, uint32_t *out_state)
	{
		windows++;
		h_in[0] = carry;
		for (size_t i = 1; i < n; i++) h_in[i] = guess;
		for (;;) {
			passes++;
			if (!FILE_OK(hipMemcpyAsync(d_st, h_in, n * 4u, hipMemcpyHostToDevice, s))) return -1;
			if (W != 0) {
				/* every piece is walked again: its set from this pass's in-state only */
				if (!FILE_OK(hipMemsetAsync(d_sets, 0, n * W * sizeof(uint64_t), s))) return -1;
				if (fsm_hip_exec_batch_eager_resume_device(d, dbuf[k], CHUNK, nullptr, nullptr, n, d_st, nullptr, d_sets, s) != 0) return -1;
			} else if (fsm_hip_exec_batch_resume_device(d, dbuf[k], CHUNK, nullptr, n, d_st, nullptr, nullptr, s) != 0) return -1;
			if (!FILE_OK(hipMemcpyAsync(h_out, d_st, n * 4u, hipMemcpyDeviceToHost, s))) return -1;
			if (!FILE_OK(hipStreamSynchronize(s))) return -1;
			bool same = true;
			for (size_t i = 1; i < n; i++) {
				if (h_in[i] != h_out[i - 1]) { h_in[i] = h_out[i - 1]; same = false; }
			}
			if (same) break;
		}
		*out_state = h_out[n - 1];
		if (W != 0) {
			/* the fixed point: every piece's set is from its true in-state */
			hipLaunchKernelGGL(walk_or_rows, dim3((unsigned)W), dim3(256), 0, s, (const uint64_t *)d_sets.p, (uint32_t)n, (uint32_t)W, d_acc.p);
			if (!FILE_OK(hipGetLastError())) return -1;
		}
		return 0;
	}
	/* eager: the accumulated set into host memory */
	int sets_out(uint64_t *h)
	{
		if (!FILE_OK(hipMemcpyAsync(h, d_acc, W * sizeof(uint64_t), hipMemcpyDeviceToHost, s))) return -1;
		if (!FILE_OK(hipStreamSynchronize(s))) return -1;
		return 0;
	}
};

bool settled(const fsm_hip_dfa *d, uint32_t st)
{
	return st == FSM_HIP_STATE_DEAD || fsm_hip_state_is_absorbing(d, st) == 1;
}

/* the last bytes of an input (fewer than a piece), or a small input: one plain call; *end = the caller's end state or NO_MATCH;
 * eager (not NULL): the set of these bytes OR-ed into it */
int tail_call(const fsm_hip_dfa *d, const unsigned char *p, size_t n, uint32_t *st, uint32_t *end, uint64_t *eager)
{
	const uint32_t len = (uint32_t)n;
	unsigned char none = 0;
	if (eager != nullptr) return fsm_hip_exec_batch_eager_resume(d, n ? p : &none, n ? n : 1u, &len, nullptr, 1, st, end, eager);
	return fsm_hip_exec_batch_resume(d, n ? p : &none, n ? n : 1u, &len, 1, st, end);
}

/* read: fills up to `cap` bytes, returns how many (0: the end), or (size_t)-1 on error.  eager (W words, or NULL for the plain
 * walk) receives the set of the whole input */
template <class Read>
int match_stream(const fsm_hip_dfa *dfa, Read read, uint32_t *end_out, unsigned *passes, unsigned *windows, uint64_t *eager)
{
	const size_t W = eager != nullptr ? fsm_hip_eager_words(dfa) : 0;
	if (eager != nullptr) memset(eager, 0, W * sizeof(uint64_t));
	uint32_t st = FSM_HIP_STATE_START, end = FSM_HIP_NO_MATCH;
	/* the first SMALL bytes into plain memory: most inputs end there */
	std::vector<unsigned char> head(SMALL);
	size_t got = 0;
	while (got < SMALL) {
		const size_t r = read(head.data() + got, SMALL - got);
		if (r == (size_t)-1) return -2;
		if (r == 0) break;
		got += r;
	}
	if (got < SMALL) {
		if (tail_call(dfa, head.data(), got, &st, &end, eager) != 0) return -1;
		*end_out = end;
		return 0;
	}
	Engine en(dfa);
	if (en.open(W) != 0) return -1;
	memcpy(en.pin[0], head.data(), SMALL);
	size_t have = SMALL;       /* bytes in the window being filled */
	int k = 0;
	bool eof = false;
	std::vector<unsigned char> rest;      /* the input's last bytes that are no whole piece */
	for (;;) {
		while (!eof && have < WINDOW) {
			const size_t r = read(en.pin[k] + have, WINDOW - have);
			if (r == (size_t)-1) return -2;
			if (r == 0) eof = true;
			else have += r;
		}
		const size_t n = have / CHUNK, whole = n * CHUNK;
		if (n != 0) {
			if (en.upload(k, whole) != 0) return -1;
			if (en.walk(k, n, st, &st) != 0) return -1;
		}
		if (eof || settled(dfa, st)) {
			rest.assign(en.pin[k] + whole, en.pin[k] + have);
			break;
		}
		/* (a full window is a whole number of pieces: nothing is carried over) */
		k ^= 1;
		have = 0;
	}
	if (passes) *passes = en.passes;
	if (windows) *windows = en.windows;
	if (settled(dfa, st) && !eof) rest.clear();      /* nothing that follows can change the state (nor the set) */
	if (eager != nullptr && en.sets_out(eager) != 0) return -1;
	if (tail_call(dfa, rest.data(), rest.size(), &st, &end, eager) != 0) return -1;
	*end_out = end;
	return 0;
}

unsigned g_last_passes = 0, g_last_windows = 0;

int match_file(const fsm_hip_dfa *dfa, FILE *f, uint32_t *end_state, uint64_t *eager)
{
	uint32_t end = FSM_HIP_NO_MATCH;
	unsigned passes = 0, windows = 0;
	const int r = match_stream(dfa, [&](unsigned char *p, size_t cap) -> size_t {
		const size_t got = fread(p, 1, cap, f);
		if (got == 0 && ferror(f)) return (size_t)-1;
		return got;
	}, &end, &passes, &windows, eager);
	g_last_passes = passes;
	g_last_windows = windows;
	if (r == -2 || ferror(f)) {      /* a read error: no match, as vm.c:205-208 (and no set) */
		if (eager != nullptr) memset(eager, 0, fsm_hip_eager_words(dfa) * sizeof(uint64_t));
		return 0;
	}
	if (r != 0) return -1;
	if (end_state) *end_state = end;
	return end != FSM_HIP_NO_MATCH;
}

int match_buffer_big(const fsm_hip_dfa *dfa, const char *buf, size_t n, uint32_t *end_state, uint64_t *eager)
{
	size_t pos = 0;
	uint32_t end = FSM_HIP_NO_MATCH;
	unsigned passes = 0, windows = 0;
	const int r = match_stream(dfa, [&](unsigned char *p, size_t cap) -> size_t {
		const size_t take = n - pos < cap ? n - pos : cap;
		if (take) memcpy(p, buf + pos, take);
		pos += take;
		return take;
	}, &end, &passes, &windows, eager);
	g_last_passes = passes;
	g_last_windows = windows;
	if (r != 0) return -1;
	if (end_state) *end_state = end;
	return end != FSM_HIP_NO_MATCH;
}

} // namespace

extern "C" int fsm_hip_match_file(const struct fsm_hip_dfa *dfa, FILE *f)
{
	if (dfa == nullptr || f == nullptr) { errno = EINVAL; return -1; }
	return match_file(dfa, f, nullptr, nullptr);
}

/* the same engine over memory: fsm_vm_match_buffer() for inputs worth the whole device (shim.c sends the small ones the plain way) */
extern "C" int fsm_hip_match_buffer_big(const struct fsm_hip_dfa *dfa, const char *buf, size_t n, uint32_t *end_state)
{
	if (dfa == nullptr || (n != 0 && buf == nullptr)) { errno = EINVAL; return -1; }
	return match_buffer_big(dfa, buf, n, end_state, nullptr);
}

/* ... and with the set of eager outputs fsm_exec's callback would have received over the whole input */
extern "C" int fsm_hip_match_file_eager(const struct fsm_hip_dfa *dfa, FILE *f, uint32_t *end_state, uint64_t *eager_out)
{
	if (dfa == nullptr || f == nullptr || eager_out == nullptr) { errno = EINVAL; return -1; }
	return match_file(dfa, f, end_state, eager_out);
}

extern "C" int fsm_hip_match_buffer_big_eager(const struct fsm_hip_dfa *dfa, const char *buf, size_t n, uint32_t *end_state, uint64_t *eager_out)
{
	if (dfa == nullptr || (n != 0 && buf == nullptr) || eager_out == nullptr) { errno = EINVAL; return -1; }
	return match_buffer_big(dfa, buf, n, end_state, eager_out);
}

/* how the last fsm_hip_match_file / _buffer_big of this process went: windows walked and passes over them (2 per window when
 * every guess stood after the first correction; 0 / 0: the input was small and took one plain call) */
extern "C" void fsm_hip_match_last_passes(unsigned *windows, unsigned *passes)
{
	if (windows) *windows = g_last_windows;
	if (passes) *passes = g_last_passes;
}
