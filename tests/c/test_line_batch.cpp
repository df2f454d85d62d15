/*
 * test_line_batch.cpp -- libfsm_amd/csrc/line_batch.h (the batch of lines every text front takes: what is refused about it,
 * where its pieces lie in the staging allocation, the owner of that allocation) against counting stand-ins of the HIP entry
 * points it reaches: no GPU, no libamdhip64.  Built with -fsanitize=address,undefined by tests/test_line_batch.py; exit status
 * 0 = every check held.
 *
 * The stand-ins hand out real heap blocks and really copy, so an upload that leaves its piece, a release that happens twice, or
 * not at all, is also the sanitizer's finding.
 */
#include "../../include/fsm_hip.h"
#include "../../libfsm_amd/csrc/line_batch.h"

#include <cstring>
#include <set>
#include <string>

using namespace fsmhip;

namespace {

int nmalloc = 0, nfree = 0, ncopy = 0, nsync = 0;
size_t last_alloc = 0;
std::string ops;                 /* A: allocation, U: copy, S: stream wait, F: release -- in the order they happened */
std::set<void *> live;
int fail_copy_at = 0;            /* fail the k-th copy from now; 0: none */
bool null_stream_seen = false;
hipStream_t const STREAM = reinterpret_cast<hipStream_t>(0x51);
const int SCRIBBLE = 4242;       /* what a wait and a release leave in errno */

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

void reset_counts()
{
	nmalloc = nfree = ncopy = nsync = 0;
	ops.clear();
	fail_copy_at = 0;
}

} // namespace

extern "C" {

hipError_t hipMalloc(void **p, size_t bytes)
{
	nmalloc++;
	ops += 'A';
	last_alloc = bytes;
	*p = malloc(bytes ? bytes : 1);      /* exactly what was asked for: a piece beyond it is the sanitizer's finding */
	live.insert(*p);
	return hipSuccess;
}
hipError_t hipFree(void *p)
{
	nfree++;
	ops += 'F';
	errno = SCRIBBLE;
	if (live.erase(p) != 1) { failures++; return hipErrorInvalidValue; }
	free(p);
	return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s)
{
	ncopy++;
	ops += 'U';
	if (s != STREAM) null_stream_seen = true;
	if (fail_copy_at != 0 && --fail_copy_at == 0) return hipErrorLaunchFailure;   /* EIO */
	memcpy(dst, src, bytes);
	return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
	nsync++;
	ops += 'S';
	errno = SCRIBBLE;
	if (s != STREAM) null_stream_seen = true;
	return hipSuccess;
}
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in"; }

} // extern "C"

namespace {

uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

/* ---- the layout: where the four host forms put their pieces before there was one function for it ---- */
void test_layout()
{
	const uint64_t sizes[] = {0, 1, 15, 16, 17}, lines[] = {0, 1, 5};
	for (uint64_t nbytes : sizes)
		for (uint64_t n : lines)
			for (int pick = 0; pick < 2; pick++)
				for (unsigned mask = 0; mask < 16u; mask++) {
					const uint64_t m = pick ? 3u : n, n_off = (n + 1u) * 8u, n_m = m * 8u;
					const bool from = mask & 1u, to = mask & 2u, first = mask & 4u, last = mask & 8u;
					/* the expressions of the spans' host form; without extras they are the other three fronts' */
					const uint64_t at_off = up16(nbytes), at_pick = at_off + up16(n_off), at_from = at_pick + (pick ? up16(n_m) : 0u),
					               at_to = at_from + (from ? up16(n_m) : 0u), at_first = at_to + (to ? up16(n_m) : 0u),
					               at_last = at_first + (first ? up16(n_m) : 0u), all = at_last + (last ? up16(n_m) : 0u);
					const StageLayout L = stage_layout(nbytes, n, m, pick != 0, mask);
					CHECK(L.at_off == at_off && L.at_pick == at_pick && L.all == all);
					CHECK(L.at_extra[0] == at_from && L.at_extra[1] == at_to && L.at_extra[2] == at_first && L.at_extra[3] == at_last);
					/* every piece at a multiple of 16; text / off / pick / extras in this order, none into the next */
					uint64_t end = nbytes;
					CHECK(L.at_off % 16u == 0 && L.at_off >= end);
					end = L.at_off + n_off;
					CHECK(L.at_pick % 16u == 0 && L.at_pick >= end);
					if (pick) end = L.at_pick + n_m;
					for (int k = 0; k < STAGE_EXTRAS; k++) {
						CHECK(L.at_extra[k] % 16u == 0 && L.at_extra[k] >= end);
						if (mask >> k & 1u) end = L.at_extra[k] + n_m;
					}
					CHECK(L.all % 16u == 0 && L.all >= end && L.all - end < 16u);
				}
	/* and three by hand */
	StageLayout L = stage_layout(0, 0, 0, false);
	CHECK(L.at_off == 0 && L.at_pick == 16 && L.all == 16);
	L = stage_layout(16, 1, 1, false);
	CHECK(L.at_off == 16 && L.at_pick == 32 && L.all == 32);
	L = stage_layout(17, 5, 3, true, 5u);           /* from and first_out: 24 bytes each, 32 with their padding */
	CHECK(L.at_off == 32 && L.at_pick == 80 && L.at_extra[0] == 112 && L.at_extra[1] == 144 && L.at_extra[2] == 144 && L.at_extra[3] == 176 && L.all == 176);
}

/* ---- the predicates ---- */
const unsigned char TEXT[] = "ab\n\nxab ab\nb\nab";
const uint64_t OFF[6] = {0, 3, 4, 11, 13, 15};

template <typename B>
B good_batch()
{
	B b;
	memset(&b, 0, sizeof b);
	b.base = TEXT;
	b.off = OFF;
	b.n = 5;
	b.trim_byte = 0x0A;
	return b;
}

template <typename B>
void shape_of(unsigned mask, unsigned unknown_flag)
{
	LineBatch lb;
	B b = good_batch<B>();
	b.flags = mask;
	b.limit = 15;
	errno = 0;
	CHECK(batch_shape(&b, mask, &lb) && errno == 0);
	CHECK(lb.base == TEXT && lb.off == OFF && lb.pick == nullptr && lb.n == 5 && lb.m == 5 && lb.limit == 15 && lb.has_limit && lb.trim == 0x0A &&
	      lb.flags == mask);
	b.limit = 0;
	CHECK(batch_shape(&b, mask, &lb) && !lb.has_limit);       /* limit 0 with a text: off[n] is the limit */
	b.base = nullptr;
	CHECK(batch_shape(&b, mask, &lb) && lb.has_limit);        /* no text: no byte may be read */
	const uint64_t pick[4] = {4, 0, 0, 2};
	b = good_batch<B>();
	b.pick = pick;
	b.m = 4;
	CHECK(batch_shape(&b, mask, &lb) && lb.m == 4 && lb.pick == pick);
	b.m = 0;                                                  /* an empty pick is still a pick */
	b.off = nullptr;
	CHECK(batch_shape(&b, mask, &lb) && lb.m == 0);           /* ... and without inputs there need be no offsets */
	b = good_batch<B>();
	b.n = 0;
	b.off = nullptr;
	CHECK(batch_shape(&b, mask, &lb) && lb.m == 0);
	struct { int trim; unsigned flags; bool no_off; } bad[] = {{-2, 0, false}, {256, 0, false}, {-1, unknown_flag, false}, {-1, 0x80000000u, false}, {-1, 0, true}};
	for (const auto &c : bad) {
		b = good_batch<B>();
		b.trim_byte = c.trim;
		b.flags = c.flags;
		if (c.no_off) b.off = nullptr;
		errno = 0;
		CHECK(!batch_shape(&b, mask, &lb) && errno == EINVAL);
	}
	errno = 0;
	CHECK(!batch_shape((const B *)nullptr, mask, &lb) && errno == EINVAL);
	for (int trim : {-1, 0, 255}) {
		b = good_batch<B>();
		b.trim_byte = trim;
		CHECK(batch_shape(&b, mask, &lb) && lb.trim == trim);
	}
}

void test_predicates()
{
	shape_of<struct fsm_hip_tok_batch>(FSM_HIP_TOKENS_NO_BACKTRACK | FSM_HIP_TOKENS_SKIP_BAD, 4u);
	shape_of<struct fsm_hip_match_batch>(FSM_HIP_MATCHES_DROP_EMPTY, 2u);
	shape_of<struct fsm_hip_pos_batch>(FSM_HIP_POS_BACKWARD, 2u);

	LineBatch good;
	good.base = TEXT;
	good.off = OFF;
	good.n = good.m = 5;
	errno = 0;
	CHECK(batch_host_arrays_ok(good) && errno == 0);
	for (int at : {0, 2, 4}) {                                /* offsets that decrease: the first pair, a middle one, the last */
		uint64_t off[6];
		memcpy(off, OFF, sizeof off);
		off[at] = off[at + 1] + 1u;
		LineBatch b = good;
		b.off = off;
		errno = 0;
		CHECK(!batch_host_arrays_ok(b) && errno == EINVAL);
	}
	{
		const uint64_t ok_pick[4] = {4, 0, 0, 2}, bad_pick[4] = {4, 0, 5, 2};
		LineBatch b = good;
		b.pick = ok_pick;
		b.m = 4;
		CHECK(batch_host_arrays_ok(b));
		b.pick = bad_pick;                                    /* pick[j] == n */
		errno = 0;
		CHECK(!batch_host_arrays_ok(b) && errno == EINVAL);
		b.m = 2;                                              /* (the bad one is not among the first two) */
		CHECK(batch_host_arrays_ok(b));
	}
	{
		LineBatch b = good;
		b.base = nullptr;                                     /* bytes without a text */
		errno = 0;
		CHECK(!batch_host_arrays_ok(b) && errno == EINVAL);
		const uint64_t empty[6] = {0, 0, 0, 0, 0, 0};
		b.off = empty;
		CHECK(batch_host_arrays_ok(b));                       /* five empty lines need none */
	}
	{
		LineBatch b;                                          /* no inputs: no array is looked at, a NULL off passes */
		b.n = 5;
		b.m = 0;
		b.pick = OFF;
		errno = 0;
		CHECK(batch_host_arrays_ok(b) && errno == 0);
	}
	{
		LineBatch b = good;                                   /* the device form */
		b.limit = 15;
		CHECK(batch_device_ok(b));
		b.limit = 0;
		CHECK(batch_device_ok(b));
		b.base = nullptr;
		CHECK(batch_device_ok(b));
		b.limit = 1;
		errno = 0;
		CHECK(!batch_device_ok(b) && errno == EINVAL);
	}
}

/* ---- the limit of the device form ---- */
void test_read_limit()
{
	LineBatch b;
	b.base = TEXT;
	b.off = OFF;
	b.n = b.m = 5;
	reset_counts();
	CHECK(batch_read_limit(&b, STREAM) && b.limit == 15 && b.has_limit && ops == "US");   /* off[n], one short wait */
	reset_counts();
	b.limit = 7;
	CHECK(batch_read_limit(&b, STREAM) && b.limit == 7 && ops.empty());                   /* given: nothing is read */
	b.limit = 0;
	b.m = 0;
	CHECK(batch_read_limit(&b, STREAM) && b.limit == 0 && ops.empty());                   /* no inputs */
	b.m = 5;
	b.base = nullptr;
	CHECK(batch_read_limit(&b, STREAM) && b.limit == 0 && ops.empty());                   /* no text */
	b.base = TEXT;
	fail_copy_at = 1;
	errno = 0;
	CHECK(!batch_read_limit(&b, STREAM) && errno == EIO);
	reset_counts();
}

/* ---- the staging ---- */
void test_staged()
{
	const uint64_t pick[4] = {4, 0, 0, 2}, from[4] = {1, 2, 3, 4}, to[4] = {5, 6, 7, 8};
	LineBatch host;
	host.base = TEXT;
	host.off = OFF;
	host.n = host.m = 5;
	host.trim = 0x0A;
	host.flags = 1u;
	{   /* the three text fronts' batch: the text and the offsets */
		reset_counts();
		StagedBatch st;
		LineBatch dev;
		CHECK(st.stage(host, STREAM, &dev));
		CHECK(ops == "AUU" && last_alloc == 16 + 48);
		CHECK(dev.base == st.d.p && dev.limit == 15 && dev.has_limit && dev.pick == nullptr && dev.n == 5 && dev.m == 5 && dev.trim == 0x0A && dev.flags == 1u);
		CHECK((const unsigned char *)dev.off == st.d.p + 16 && memcmp(dev.base, TEXT, 15) == 0 && memcmp(dev.off, OFF, 48) == 0);
		errno = 77;
	}
	CHECK(errno == 77 && ops == "AUUF");
	{   /* with a pick, and as the spans stage: from, no to, room for first_out, none for last_out */
		reset_counts();
		LineBatch h = host, dev;
		h.pick = pick;
		h.m = 4;
		StagedBatch st;
		uint64_t first_out[4];                                /* the caller's: an output is not uploaded, and not touched */
		memset(first_out, 0x11, sizeof first_out);
		CHECK(st.stage(h, STREAM, &dev, {{from}, {nullptr}, {first_out, false}, {nullptr, false}}));
		CHECK(ops == "AUUUU" && last_alloc == 16 + 48 + 32 + 32 + 32);
		CHECK((const unsigned char *)dev.pick == st.d.p + 64 && memcmp(dev.pick, pick, 32) == 0 && dev.m == 4);
		CHECK((unsigned char *)st.extra(0) == st.d.p + 96 && memcmp(st.extra(0), from, 32) == 0);
		CHECK(st.extra(1) == nullptr && st.extra(3) == nullptr);
		CHECK((unsigned char *)st.extra(2) == st.d.p + 128);
		memset(st.extra(2), 0xee, 32);                        /* the room is there to its last byte */
		CHECK(first_out[0] == 0x1111111111111111u && first_out[3] == 0x1111111111111111u);
	}
	{   /* all four extras */
		reset_counts();
		LineBatch h = host, dev;
		h.pick = pick;
		h.m = 4;
		StagedBatch st;
		uint64_t out[2][4];
		CHECK(st.stage(h, STREAM, &dev, {{from}, {to}, {out[0], false}, {out[1], false}}));
		CHECK(ops == "AUUUUU" && last_alloc == 16 + 48 + 32 * 5);
		CHECK(memcmp(st.extra(1), to, 32) == 0);
		memset(st.extra(3), 0xee, 32);
	}
	{   /* lines without a byte: no text on the device, and none is copied */
		reset_counts();
		const uint64_t empty[3] = {0, 0, 0};
		LineBatch h, dev;
		h.off = empty;
		h.n = h.m = 2;
		StagedBatch st;
		CHECK(st.stage(h, STREAM, &dev));
		CHECK(ops == "AU" && last_alloc == 32 && dev.base == nullptr && dev.limit == 0 && dev.has_limit && (const unsigned char *)dev.off == st.d.p);
	}
	{   /* no inputs: nothing is staged and no host pointer is handed on */
		reset_counts();
		LineBatch h = host, dev;
		h.pick = pick;
		h.m = 0;
		StagedBatch st;
		CHECK(st.stage(h, STREAM, &dev));
		CHECK(ops.empty() && dev.base == nullptr && dev.off == nullptr && dev.pick == nullptr && dev.m == 0 && dev.limit == 0 && dev.has_limit);
	}
	CHECK(live.empty());
	/* the k-th upload fails: the stream is idle before the memory goes, errno is the upload's, nothing is left */
	for (int k = 1; k <= 5; k++) {
		reset_counts();
		LineBatch h = host, dev;
		h.pick = pick;
		h.m = 4;
		{
			StagedBatch st;
			fail_copy_at = k;
			errno = 0;
			uint64_t out[2][4];
			CHECK(!st.stage(h, STREAM, &dev, {{from}, {to}, {out[0], false}, {out[1], false}}));
			CHECK(errno == EIO);
			CHECK(ops == std::string("A") + std::string((size_t)k, 'U') + "SF");   /* nothing is issued behind the failure */
			CHECK(live.empty());
		}
		CHECK(errno == EIO && nmalloc == 1 && nfree == 1 && nsync == 1);
	}
	CHECK(!null_stream_seen);
}

} // namespace

int main()
{
	test_layout();
	test_predicates();
	test_read_limit();
	test_staged();
	CHECK(live.empty());
	if (failures) { fprintf(stderr, "test_line_batch: %d check(s) failed\n", failures); return 1; }
	printf("test_line_batch: ok\n");
	return 0;
}
