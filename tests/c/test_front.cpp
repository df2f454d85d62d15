/*
 * test_front.cpp -- libfsm_amd/csrc/front.h (the skeleton of the text objects' host fronts: run_new / run_free / run_host /
 * run_ms, copy_out, grid_of) against stand-ins of the HIP entry points it calls that record the ORDER of the calls: no GPU, no
 * libamdhip64.  Built with -fsanitize=address,undefined by tests/test_front.py; exit status 0 = every check held.
 *
 * The stand-ins hand out real heap blocks, so a release that happens twice, or not at all, is also the sanitizer's finding.
 */
#include "../../libfsm_amd/csrc/front.h"

#include <cstring>
#include <set>
#include <vector>

namespace {

enum Kind { GET_DEV, SET_DEV, DEV_COUNT, DEV_ATTR, MALLOC, FREE, MEMCPY, MEMCPY_ASYNC, EV_CREATE, EV_DESTROY, EV_RECORD, EV_SYNC, EV_ELAPSED,
            ST_CREATE, ST_DESTROY, ST_SYNC };
struct Call {
	Kind kind;
	const void *a, *b;       /* the handle(s) the call was made with */
};
std::vector<Call> calls;
std::set<void *> live_dev, live_ev, live_st;
std::vector<void *> ev_order;    /* the events in the order of their creation: index k is ev[k] of the object made last */
int cur_dev = 0, fail_set_dev = -1, ndev = 1, ncu = 4;
int fail_event_at = 0, fail_memcpy_at = 0;   /* fail the n-th such call from now; 0: none */
bool fail_stream_create = false, fail_attr = false;
const int SCRIBBLE = 4242;   /* what every releasing stand-in leaves in errno */

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

void note(Kind k, const void *a = nullptr, const void *b = nullptr) { calls.push_back({k, a, b}); }
size_t live() { return live_dev.size() + live_ev.size() + live_st.size(); }
int count(Kind k)
{
	int c = 0;
	for (const Call &x : calls) c += x.kind == k;
	return c;
}
/* the index of the first call of kind k, or of the first release of anything (any = true); calls.size() when there is none */
size_t first(Kind k, bool any_release = false)
{
	for (size_t i = 0; i < calls.size(); i++)
		if (any_release ? (calls[i].kind == FREE || calls[i].kind == EV_DESTROY || calls[i].kind == ST_DESTROY) : calls[i].kind == k) return i;
	return calls.size();
}
size_t first_release() { return first(FREE, true); }
void fresh(int dev = 0)
{
	calls.clear();
	ev_order.clear();
	cur_dev = dev;
	fail_set_dev = -1;
	fail_event_at = fail_memcpy_at = 0;
	fail_stream_create = fail_attr = false;
}

} // namespace

extern "C" {

hipError_t hipGetDeviceCount(int *n) { note(DEV_COUNT); *n = ndev; return ndev < 0 ? hipErrorNoDevice : hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int)
{
	note(DEV_ATTR);
	if (fail_attr) return hipErrorInvalidValue;
	*v = ncu;
	return hipSuccess;
}
hipError_t hipGetDevice(int *d) { note(GET_DEV); *d = cur_dev; return hipSuccess; }
hipError_t hipSetDevice(int d)
{
	note(SET_DEV);
	errno = SCRIBBLE;
	if (d == fail_set_dev) return hipErrorInvalidDevice;
	cur_dev = d;
	return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes)
{
	*p = calloc(bytes ? bytes : 1, 1);
	note(MALLOC, *p);
	live_dev.insert(*p);
	return hipSuccess;
}
hipError_t hipFree(void *p)
{
	note(FREE, p);
	errno = SCRIBBLE;
	if (live_dev.erase(p) != 1) { failures++; return hipErrorInvalidValue; }
	free(p);
	return hipSuccess;
}
hipError_t hipHostMalloc(void **, size_t, unsigned) { failures++; return hipErrorOutOfMemory; }   /* (PinBuf: not front.h's) */
hipError_t hipHostFree(void *) { failures++; return hipErrorInvalidValue; }
static hipError_t copy(Kind k, void *dst, const void *src, size_t bytes)
{
	note(k, dst, src);
	if (fail_memcpy_at != 0 && --fail_memcpy_at == 0) return hipErrorLaunchFailure;
	memcpy(dst, src, bytes);
	return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { return copy(MEMCPY, dst, src, bytes); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { return copy(MEMCPY_ASYNC, dst, src, bytes); }
hipError_t hipEventCreate(hipEvent_t *e)
{
	note(EV_CREATE);
	if (fail_event_at != 0 && --fail_event_at == 0) return hipErrorInvalidValue;   /* (*e is left as it was: null) */
	*e = static_cast<hipEvent_t>(malloc(1));
	live_ev.insert(*e);
	ev_order.push_back(*e);
	return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e)
{
	note(EV_DESTROY, e);
	errno = SCRIBBLE;
	if (live_ev.erase(e) != 1) { failures++; return hipErrorInvalidValue; }
	free(e);
	return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { note(EV_RECORD, e, s); return live_ev.count(e) == 1 ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { note(EV_SYNC, e); return live_ev.count(e) == 1 ? hipSuccess : hipErrorInvalidHandle; }
/* 2^p milliseconds between ev[2p] and ev[2p + 1] of the object made last; every other pair is an error */
hipError_t hipEventElapsedTime(float *ms, hipEvent_t from, hipEvent_t to)
{
	note(EV_ELAPSED, from, to);
	for (size_t p = 0; 2 * p + 1 < ev_order.size(); p++)
		if (ev_order[2 * p] == from && ev_order[2 * p + 1] == to) { *ms = (float)(1u << p); return hipSuccess; }
	return hipErrorInvalidHandle;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
	note(ST_CREATE);
	if (fail_stream_create) return hipErrorOutOfMemory;
	*s = static_cast<hipStream_t>(malloc(1));
	live_st.insert(*s);
	return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
	note(ST_DESTROY, s);
	errno = SCRIBBLE;
	if (live_st.erase(s) != 1) { failures++; return hipErrorInvalidValue; }
	free(s);
	return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { note(ST_SYNC, s); errno = SCRIBBLE; return hipSuccess; }   /* (a wait may touch errno too) */
const char *hipGetErrorString(hipError_t) { return "stand-in"; }

} // extern "C"

namespace {

struct Obj : RunObject<3> {
	DevBuf<uint64_t> a;
	DevBuf<unsigned char> b;
};
int fake_stream;                 /* a caller's stream: only its address is used */
const hipStream_t STREAM = reinterpret_cast<hipStream_t>(&fake_stream);

/* passes that allocate both buffers and then end with `rc` (errno = `err` when that is a failure) */
auto passes_ending(int rc, int err, int *ran)
{
	return [=](Obj *o) {
		++*ran;
		if (!HIP_OK(o->a.alloc(8)) || !HIP_OK(o->b.alloc(100))) return -1;
		if (rc != 0) errno = err;
		return rc;
	};
}

/* after a failed run_new: one wait for the caller's stream, before anything is released, and nothing is left */
void check_failed_run(Obj *o, int want_errno)
{
	CHECK(o == nullptr && errno == want_errno);
	CHECK(count(ST_SYNC) == 1 && calls[first(ST_SYNC)].a == STREAM);
	CHECK(first_release() < calls.size() && first(ST_SYNC) < first_release());
	CHECK(live() == 0);
}

void test_run_new()
{
	int ran = 0;
	fresh();
	errno = 0;
	CHECK(run_new<Obj>(0, 5, false, STREAM, passes_ending(0, 0, &ran)) == nullptr && errno == ENOMEM);
	CHECK(calls.empty() && ran == 0);                            /* a grid that does not fit: no HIP call at all */

	for (int k = 1; k <= 2 * Obj::npass; k++) {                  /* the k-th event cannot be made */
		fresh();
		fail_event_at = k;
		errno = 0;
		Obj *o = run_new<Obj>(0, 5, true, STREAM, passes_ending(0, 0, &ran));
		CHECK(count(EV_CREATE) == k && ran == 0);                /* no further event is tried, the passes never run */
		CHECK(count(EV_DESTROY) == k - 1 && count(EV_SYNC) == 0);   /* (no last event to wait for) */
		if (k == 1) { CHECK(o == nullptr && errno == EINVAL && count(ST_SYNC) == 1 && first_release() == calls.size() && live() == 0); }
		else check_failed_run(o, EINVAL);
	}

	fresh();
	errno = 0;
	Obj *o = run_new<Obj>(0, 5, true, STREAM, passes_ending(-1, EIO, &ran));
	CHECK(ran == 1 && count(MALLOC) == 2 && count(FREE) == 2 && count(EV_DESTROY) == 2 * Obj::npass);
	check_failed_run(o, EIO);                                    /* the passes' errno, not a release's */
	CHECK(count(EV_SYNC) == 1 && first(ST_SYNC) < first(EV_SYNC) && first(EV_SYNC) < first_release());

	fresh();
	o = run_new<Obj>(2, 5, true, STREAM, passes_ending(0, 0, &ran));
	CHECK(o != nullptr && o->device == 2 && o->m == 5 && ran == 2);
	CHECK(count(ST_SYNC) == 0 && first_release() == calls.size());   /* a run that succeeds waits for nothing */
	CHECK(o->done() == ev_order[2 * Obj::npass - 1]);
	CHECK(o->begin(1, STREAM) && o->end(1, STREAM) && count(EV_RECORD) == 2);
	CHECK(calls[first(EV_RECORD)].a == ev_order[2] && calls.back().a == ev_order[3] && calls.back().b == STREAM);
	run_free(o);
	CHECK(live() == 0);
}

void test_run_free()
{
	int ran = 0;
	fresh();
	errno = 77;
	run_free(static_cast<Obj *>(nullptr));
	CHECK(calls.empty() && errno == 77);

	Obj *o = run_new<Obj>(3, 1, true, STREAM, passes_ending(0, 0, &ran));   /* (made with device 0 current: run_new sets none) */
	CHECK(o != nullptr);
	const void *done = o->done();
	calls.clear();
	errno = 77;
	run_free(o);
	CHECK(errno == 77);                                          /* errno survives the releases and the guard */
	CHECK(count(EV_SYNC) == 1 && calls[first(EV_SYNC)].a == done && first(EV_SYNC) < first_release());
	CHECK(count(FREE) == 2 && count(EV_DESTROY) == 2 * Obj::npass && live() == 0);
	CHECK(count(SET_DEV) == 2 && first(SET_DEV) < first(EV_SYNC) && calls.back().kind == SET_DEV && cur_dev == 0);   /* the object's device, then the caller's */
}

void test_run_ms()
{
	int ran = 0;
	fresh();
	Obj *o = run_new<Obj>(0, 1, true, STREAM, passes_ending(0, 0, &ran));
	CHECK(o != nullptr);
	calls.clear();
	errno = 0;
	CHECK(run_ms(static_cast<const Obj *>(nullptr), 0, 0) == -1.0 && errno == EINVAL);
	errno = 0;
	CHECK(run_ms(o, -1, 1) == -1.0 && errno == EINVAL);
	errno = 0;
	CHECK(run_ms(o, 0, Obj::npass) == -1.0 && errno == EINVAL);
	CHECK(calls.empty());                                        /* refused before any HIP call */
	const struct { int from, to; double want; } cases[] = {{0, 2, 7.0}, {1, 2, 6.0}, {0, 0, 1.0}, {2, 2, 4.0}, {1, 1, 2.0}};
	for (const auto &c : cases) {
		calls.clear();
		CHECK(run_ms(o, c.from, c.to) == c.want);                /* exactly the pairs from .. to */
		CHECK(count(EV_ELAPSED) == c.to - c.from + 1);
		CHECK(count(EV_SYNC) == 1 && calls[first(EV_SYNC)].a == o->done() && first(EV_SYNC) < first(EV_ELAPSED));
	}
	run_free(o);
	CHECK(live() == 0);
}

void test_copy_out()
{
	fresh();
	DevEvent done;
	CHECK(done.create() == hipSuccess);
	const char src[3][4] = {"abc", "def", "ghi"};
	char d0[4] = "", d1[4] = "", d2[4] = "";
	calls.clear();
	CHECK(copy_out(0, done, {{d0, src[0], 4}, {nullptr, src[1], 4}, {d1, src[1], 0}, {d2, src[2], 4}}) == 0);
	CHECK(count(MEMCPY) == 2 && !strcmp(d0, "abc") && d1[0] == 0 && !strcmp(d2, "ghi"));   /* no destination, no bytes: skipped */
	CHECK(count(EV_SYNC) == 1 && calls[first(EV_SYNC)].a == done.e && first(EV_SYNC) < first(MEMCPY));

	calls.clear();
	d0[0] = d1[0] = d2[0] = 0;
	fail_memcpy_at = 2;
	errno = 0;
	CHECK(copy_out(0, done, {{d0, src[0], 4}, {d1, src[1], 4}, {d2, src[2], 4}}) == -1 && errno == EIO);
	CHECK(count(MEMCPY) == 2 && !strcmp(d0, "abc") && d2[0] == 0);   /* it stops at the first copy that fails */

	calls.clear();
	fail_memcpy_at = 0;
	fail_set_dev = 6;
	errno = 0;
	CHECK(copy_out(6, done, {{d0, src[0], 4}}) == -1 && errno == ENODEV);
	CHECK(count(EV_SYNC) == 0 && count(MEMCPY) == 0 && cur_dev == 0);
	errno = 0;
	CHECK(elapsed_ms(6, done, {}) == -1.0 && errno == ENODEV);
	fail_set_dev = -1;
}

void test_grid()
{
	fresh();
	ndev = 0;
	CHECK(!have_device());
	ndev = -1;
	CHECK(!have_device());
	ndev = 1;
	CHECK(have_device());

	const uint64_t cap = max_workgroups(0);
	CHECK(cap == (uint64_t)ncu * FRONT_WG_PER_CU && cap > 2);
	fail_attr = true;
	CHECK(max_workgroups(0) == 256u * FRONT_WG_PER_CU);          /* a device that does not say: the MI355X's 256 CUs */
	fail_attr = false;
	calls.clear();
	const Grid none = grid_of(0, 0);
	CHECK(none.wgs == 1 && none.per == 1 && calls.empty());
	for (uint64_t nblocks : {(uint64_t)1, cap - 1, cap, cap + 1, 3 * cap + 1}) {
		const Grid g = grid_of(nblocks, 0);
		CHECK(g.wgs >= 1 && g.wgs <= cap && g.per >= 1);
		CHECK(g.wgs * g.per >= nblocks);                         /* every block has a workgroup */
		CHECK((g.wgs - 1) * g.per < nblocks);                    /* no workgroup is without a block */
	}
}

void test_run_host()
{
	int made = 0, ran = 0;
	const unsigned char text[] = "ab\ncd\n";
	const uint64_t off[3] = {0, 3, 6};
	fsmhip::LineBatch host;
	host.base = text;
	host.off = off;
	host.n = host.m = 2;
	auto make = [&](const fsmhip::LineBatch &in, hipStream_t s) {
		made++;
		CHECK(s != nullptr && live_st.count(s) == 1 && in.limit == 6 && in.m == 2 && in.base != text && in.off != off);
		CHECK(live_dev.count(const_cast<void *>(in.base)) == 1 && !memcmp(in.base, text, 6) && in.off[2] == 6);   /* the batch as staged */
		return run_new<Obj>(1, in.m, true, s, passes_ending(0, 0, &ran));
	};

	fresh();
	fail_stream_create = true;
	errno = 0;
	CHECK(run_host(1, host, make) == nullptr && errno == ENOMEM);
	CHECK(made == 0 && count(MALLOC) == 0 && live() == 0 && cur_dev == 0);   /* no stream of its own: nothing is staged or made */

	fresh();
	fail_set_dev = 1;
	errno = 0;
	CHECK(run_host(1, host, make) == nullptr && errno == ENODEV && made == 0 && count(ST_CREATE) == 0);

	fresh();
	Obj *o = run_host(1, host, make);
	CHECK(o != nullptr && made == 1 && ran == 1 && o->device == 1 && o->m == 2);
	CHECK(count(ST_SYNC) == 1 && first(ST_SYNC) < first_release());   /* the last wait, before the stream and the staged batch go */
	CHECK(count(ST_DESTROY) == 1 && count(FREE) == 1 && live_st.empty() && cur_dev == 0);
	run_free(o);
	CHECK(live() == 0);
}

} // namespace

int main()
{
	test_run_new();
	test_run_free();
	test_run_ms();
	test_copy_out();
	test_grid();
	test_run_host();
	CHECK(live() == 0);
	if (failures) { fprintf(stderr, "test_front: %d check(s) failed\n", failures); return 1; }
	printf("test_front: ok\n");
	return 0;
}
