/*
 * test_hip_host.cpp -- libfsm_amd/csrc/hip_host.h against counting stand-ins of the HIP entry points it calls: no GPU, no
 * libamdhip64.  Built with -fsanitize=address,undefined by tests/test_hip_host.py; exit status 0 = every check held.
 *
 * The stand-ins hand out real heap blocks, so a release that happens twice, or not at all, is also the sanitizer's finding.
 */
#include "../../libfsm_amd/csrc/hip_host.h"

#include <cstring>
#include <set>
#include <utility>

namespace {

struct Counts {
	int dmalloc = 0, dfree = 0, hmalloc = 0, hfree = 0, memcpy_ = 0;
	int ev_create = 0, ev_destroy = 0, st_create = 0, st_destroy = 0, get_dev = 0, set_dev = 0;
	size_t last_alloc = 0, last_copy = 0;
	unsigned last_ev_flags = 0xdeadu, last_st_flags = 0xdeadu;
} C;
std::set<void *> live_dev, live_pin, live_ev, live_st;
int fail_alloc_at = 0;       /* fail the n-th allocation (device and pinned counted together) from now; 0: none */
int cur_dev = 0;
bool fail_get = false;
int fail_set_dev = -1;       /* hipSetDevice of this device fails */
int set_log[8], nset = 0;
const int SCRIBBLE = 4242;   /* what every releasing stand-in leaves in errno */

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

bool alloc_fails() { return fail_alloc_at != 0 && --fail_alloc_at == 0; }
size_t live() { return live_dev.size() + live_pin.size() + live_ev.size() + live_st.size(); }

} // namespace

extern "C" {

hipError_t hipMalloc(void **p, size_t bytes)
{
	C.dmalloc++;
	C.last_alloc = bytes;
	if (alloc_fails()) { *p = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }   /* (junk: the owner must not keep it) */
	*p = malloc(bytes ? bytes : 1);
	live_dev.insert(*p);
	return hipSuccess;
}
hipError_t hipFree(void *p)
{
	C.dfree++;
	errno = SCRIBBLE;
	if (live_dev.erase(p) != 1) { failures++; return hipErrorInvalidValue; }
	free(p);
	return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
	C.hmalloc++;
	C.last_alloc = bytes;
	if (alloc_fails()) { *p = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }
	*p = malloc(bytes ? bytes : 1);
	live_pin.insert(*p);
	return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
	C.hfree++;
	errno = SCRIBBLE;
	if (live_pin.erase(p) != 1) { failures++; return hipErrorInvalidValue; }
	free(p);
	return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
	C.memcpy_++;
	C.last_copy = bytes;
	memcpy(dst, src, bytes);
	return hipSuccess;
}
static hipError_t event_new(hipEvent_t *e)
{
	C.ev_create++;
	*e = static_cast<hipEvent_t>(malloc(1));
	live_ev.insert(*e);
	return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { C.last_ev_flags = 0; return event_new(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { C.last_ev_flags = flags; return event_new(e); }
hipError_t hipEventDestroy(hipEvent_t e)
{
	C.ev_destroy++;
	errno = SCRIBBLE;
	if (live_ev.erase(e) != 1) { failures++; return hipErrorInvalidValue; }
	free(e);
	return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
	C.st_create++;
	C.last_st_flags = flags;
	*s = static_cast<hipStream_t>(malloc(1));
	live_st.insert(*s);
	return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
	C.st_destroy++;
	errno = SCRIBBLE;
	if (live_st.erase(s) != 1) { failures++; return hipErrorInvalidValue; }
	free(s);
	return hipSuccess;
}
hipError_t hipGetDevice(int *d)
{
	C.get_dev++;
	if (fail_get) return hipErrorNoDevice;
	*d = cur_dev;
	return hipSuccess;
}
hipError_t hipSetDevice(int d)
{
	C.set_dev++;
	errno = SCRIBBLE;
	if (nset < 8) set_log[nset++] = d;
	if (d == fail_set_dev) return hipErrorInvalidDevice;
	cur_dev = d;
	return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "stand-in"; }

} // extern "C"

namespace {

/* one owner type through its whole life; make(o) acquires; made / gone: the stand-ins' counters for it */
template <class Owner, class Make>
void lifecycle(const char *name, Make make, const int &made, const int &gone)
{
	const int m0 = made, g0 = gone;
	{
		Owner a;
		CHECK(!a);                                  /* empty: converts to a null handle */
	}
	CHECK(made == m0 && gone == g0);                 /* an empty owner releases nothing */
	{
		Owner a;
		CHECK(make(a) == hipSuccess && a);
		errno = 77;
	}
	CHECK(errno == 77);                              /* errno survives the release */
	CHECK(made == m0 + 1 && gone == g0 + 1);         /* exactly once */
	{
		Owner a;
		CHECK(make(a) == hipSuccess);
		Owner b(std::move(a));
		CHECK(!a && b);
	}
	CHECK(made == m0 + 2 && gone == g0 + 2);         /* the moved-from owner released nothing */
	{
		Owner a, b;
		CHECK(make(a) == hipSuccess && make(b) == hipSuccess);
		const void *was_a = a;
		b = std::move(a);
		CHECK(gone == g0 + 3);                      /* move-assignment released the target's old resource */
		const void *now_b = b;
		CHECK(!a && now_b == was_a);
	}
	CHECK(made == m0 + 4 && gone == g0 + 4);
	{
		Owner a;
		CHECK(make(a) == hipSuccess);
		a.reset();
		a.reset();
		CHECK(!a && gone == g0 + 5);                /* reset() twice is one release */
	}
	CHECK(gone == g0 + 5);
	{
		Owner a;
		CHECK(make(a) == hipSuccess && make(a) == hipSuccess);
		CHECK(made == m0 + 7 && gone == g0 + 6);     /* acquiring over a held resource releases it first */
	}
	CHECK(gone == g0 + 7);
	CHECK(live() == 0);
	if (failures) fprintf(stderr, "(after %s)\n", name);
}

void test_owners()
{
	lifecycle<DevBuf<uint32_t>>("DevBuf", [](DevBuf<uint32_t> &b) { return b.alloc(10); }, C.dmalloc, C.dfree);
	CHECK(C.last_alloc == 40);
	lifecycle<DevBuf<uint64_t>>("DevBuf::upload", [](DevBuf<uint64_t> &b) { return b.upload(std::vector<uint64_t>(3, 5)); }, C.dmalloc, C.dfree);
	lifecycle<PinBuf<unsigned char>>("PinBuf", [](PinBuf<unsigned char> &b) { return b.alloc(100); }, C.hmalloc, C.hfree);
	CHECK(C.last_alloc == 100);
	lifecycle<DevEvent>("DevEvent", [](DevEvent &e) { return e.create(); }, C.ev_create, C.ev_destroy);
	CHECK(C.last_ev_flags == 0);
	lifecycle<DevEvent>("DevEvent(flags)", [](DevEvent &e) { return e.create(hipEventDisableTiming); }, C.ev_create, C.ev_destroy);
	CHECK(C.last_ev_flags == hipEventDisableTiming);
	lifecycle<DevStream>("DevStream", [](DevStream &s) { return s.create(hipStreamNonBlocking); }, C.st_create, C.st_destroy);
	CHECK(C.last_st_flags == hipStreamNonBlocking);
	/* movable where a container needs it */
	{
		std::vector<DevBuf<unsigned char>> old;
		const int f0 = C.dfree;
		for (int k = 0; k < 5; k++) {
			DevBuf<unsigned char> b;
			CHECK(b.alloc(16) == hipSuccess);
			old.push_back(std::move(b));
		}
		CHECK(C.dfree == f0 && live_dev.size() == 5);
		old.clear();
		CHECK(C.dfree == f0 + 5);
	}
	CHECK(live() == 0);
}

void test_upload()
{
	{
		DevBuf<uint32_t> b;
		const int c0 = C.memcpy_;
		CHECK(b.upload(std::vector<uint32_t>()) == hipSuccess && b);
		CHECK(C.last_alloc == 16 && C.memcpy_ == c0);             /* empty: sizeof(T) rounded up to 16, nothing copied */
		const std::vector<uint32_t> v = {1, 2, 3, 4, 5};
		CHECK(b.upload(v) == hipSuccess);
		CHECK(C.last_alloc == 32 && C.memcpy_ == c0 + 1 && C.last_copy == 20);
		CHECK(memcmp(b.p, v.data(), 20) == 0);
		CHECK(live_dev.size() == 1);                              /* the first block went */
	}
	{
		DevBuf<uint64_t> w;
		CHECK(w.upload(std::vector<uint64_t>()) == hipSuccess && C.last_alloc == 16);
		CHECK(w.upload(std::vector<uint64_t>(2, 9)) == hipSuccess && C.last_alloc == 16 && C.last_copy == 16);
		DevBuf<unsigned char> t;                                  /* a table owned as bytes: its element's size is the least */
		const std::vector<uint16_t> h(9, 7);
		CHECK(t.upload_bytes(h.data(), 18, 2) == hipSuccess && C.last_alloc == 32 && C.last_copy == 18);
		CHECK(t.upload_bytes(nullptr, 0, 2) == hipSuccess && C.last_alloc == 16);
	}
	CHECK(live() == 0);
}

/* the n-th allocation fails: the owner is empty, nothing is live, and what it held before is gone (released first) */
void test_failed_allocation()
{
	for (int n = 1; n <= 2; n++) {
		{
			DevBuf<uint32_t> a, b;
			fail_alloc_at = n;
			const hipError_t e1 = a.alloc(4), e2 = b.upload(std::vector<uint32_t>(4, 1));
			CHECK((n == 1 ? e1 : e2) == hipErrorOutOfMemory && (n == 1 ? e2 : e1) == hipSuccess);
			CHECK(n == 1 ? !a && b : a && !b);
			CHECK(live_dev.size() == 1);
		}
		CHECK(live() == 0);
		{
			PinBuf<uint32_t> a, b;
			fail_alloc_at = n;
			const hipError_t e1 = a.alloc(4), e2 = b.alloc(4);
			CHECK((n == 1 ? e1 : e2) == hipErrorOutOfMemory && (n == 1 ? e2 : e1) == hipSuccess);
			CHECK(n == 1 ? !a && b : a && !b);
			CHECK(live_pin.size() == 1);
		}
		CHECK(live() == 0);
	}
	{
		/* the ensure_* shape: two tables, the second upload fails, the call is made again */
		DevBuf<uint32_t> t0, t1;
		const std::vector<uint32_t> v(8, 3);
		fail_alloc_at = 2;
		CHECK(t0.upload(v) == hipSuccess && t1.upload(v) == hipErrorOutOfMemory);
		CHECK(t0 && !t1 && live_dev.size() == 1);
		CHECK(t0.upload(v) == hipSuccess && t1.upload(v) == hipSuccess);
		CHECK(live_dev.size() == 2);                              /* the block of the first attempt is not lost */
		fail_alloc_at = 1;
		CHECK(t0.alloc(8) == hipErrorOutOfMemory && !t0 && live_dev.size() == 1);   /* over a held buffer: released, then empty */
	}
	CHECK(live() == 0);
}

void reset_devices(int dev)
{
	cur_dev = dev;
	fail_get = false;
	fail_set_dev = -1;
	nset = 0;
	C.set_dev = 0;
}

void test_guard()
{
	reset_devices(2);
	{
		DevGuard g(2);
		CHECK(g.ok());
		errno = 55;
	}
	CHECK(errno == 55 && C.set_dev == 0);                         /* same device: no hipSetDevice at all */

	reset_devices(0);
	{
		DevGuard g(3);
		CHECK(g.ok() && cur_dev == 3 && C.set_dev == 1);
		errno = 56;
	}
	CHECK(errno == 56);                                           /* errno survives the guard */
	CHECK(C.set_dev == 2 && set_log[0] == 3 && set_log[1] == 0 && cur_dev == 0);   /* other device: set, then set back */

	reset_devices(0);
	fail_set_dev = 5;
	{
		DevGuard g(5);
		CHECK(!g.ok() && C.set_dev == 1);
	}
	CHECK(C.set_dev == 1 && cur_dev == 0);                        /* failed set: nothing is set back */

	reset_devices(1);
	fail_get = true;
	{
		DevGuard g(1);
		CHECK(g.ok() && C.set_dev == 1 && set_log[0] == 1);       /* the caller's device is unknown: set ... */
	}
	CHECK(C.set_dev == 1);                                        /* ... and nothing to set back */
	reset_devices(0);
}

void test_errno_map()
{
	CHECK(hip_errno(hipSuccess) == 0);
	CHECK(hip_errno(hipErrorOutOfMemory) == ENOMEM);
	CHECK(hip_errno(hipErrorNoDevice) == ENODEV);
	CHECK(hip_errno(hipErrorInvalidDevice) == ENODEV);
	CHECK(hip_errno(hipErrorInsufficientDriver) == ENODEV);
	CHECK(hip_errno(hipErrorInvalidValue) == EINVAL);
	for (hipError_t e : {hipErrorNotInitialized, hipErrorInvalidHandle, hipErrorLaunchFailure, hipErrorIllegalAddress, hipErrorNotReady, hipErrorUnknown})
		CHECK(hip_errno(e) == EIO);                               /* the default */
	errno = 0;
	CHECK(HIP_OK(hipSuccess) && errno == 0);
	CHECK(!HIP_OK(hipErrorOutOfMemory) && errno == ENOMEM);
	CHECK(!HIP_OK(hipErrorLaunchFailure) && errno == EIO);
}

} // namespace

int main()
{
	test_owners();
	test_upload();
	test_failed_allocation();
	test_guard();
	test_errno_map();
	CHECK(live() == 0);
	CHECK(C.dmalloc > 0 && C.hmalloc > 0 && C.ev_create > 0 && C.st_create > 0);
	if (failures) { fprintf(stderr, "test_hip_host: %d check(s) failed\n", failures); return 1; }
	printf("test_hip_host: ok\n");
	return 0;
}
