/*
 * hip_host.h -- the host side's HIP plumbing, in one place: the errno of a HIP error, the `if (!HIP_OK(call)) return -1;` form
 * of a failing call, "make this device current, give the caller's back", and the owners of device memory, pinned host
 * memory, events and streams.  Not part of the C ABI: everything here has hidden visibility.  Host code only -- it needs
 * <hip/hip_runtime_api.h> and no device compiler (tests/c/test_hip_host.cpp compiles it with g++ against counting stand-ins).
 *
 * An owner releases what it holds when it goes; its user sees to it that the resource's device is current (DevGuard) and that
 * no kernel still touches it (a wait for its last event or its stream; hipFree itself waits for the device).  errno survives
 * every release.  None can be copied; all can be moved.  Each converts to its raw handle, so call sites read as with one.
 */
#ifndef FSM_HIP_HOST_H
#define FSM_HIP_HOST_H

#include <hip/hip_runtime_api.h>

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#pragma GCC visibility push(hidden)

inline int hip_errno(hipError_t e)
{
	switch (e) {
	case hipSuccess: return 0;
	case hipErrorOutOfMemory: return ENOMEM;
	case hipErrorNoDevice:
	case hipErrorInvalidDevice:
	case hipErrorInsufficientDriver: return ENODEV;
	case hipErrorInvalidValue: return EINVAL;
	default: return EIO;
	}
}

/* false, with errno set, when a HIP call failed: `if (!HIP_OK(call)) return -1;` */
inline bool hip_ok(hipError_t e, const char *what)
{
	if (e == hipSuccess) return true;
	if (getenv("FSM_HIP_DEBUG")) fprintf(stderr, "fsm_hip: %s -> %s\n", what, hipGetErrorString(e));
	errno = hip_errno(e);
	return false;
}
#define HIP_OK(expr) hip_ok((expr), #expr)

/* make a device current for the duration of a call and give the caller's back */
struct DevGuard {
	int prev = -1;
	bool good = true;
	explicit DevGuard(int dev)
	{
		if (hipGetDevice(&prev) != hipSuccess) prev = -1;
		if (prev != dev && hipSetDevice(dev) != hipSuccess) good = false;
		if (prev == dev) prev = -1;
	}
	DevGuard(const DevGuard &) = delete;
	DevGuard &operator=(const DevGuard &) = delete;
	~DevGuard() { if (prev >= 0 && good) { int e = errno; (void)hipSetDevice(prev); errno = e; } }
	bool ok() const { return good; }
};

/* device memory */
template <typename T>
struct DevBuf {
	T *p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		if (this != &o) { reset(); p = o.p; o.p = nullptr; }
		return *this;
	}
	~DevBuf() { reset(); }
	void reset()
	{
		if (p == nullptr) return;
		const int e = errno;
		(void)hipFree(p);
		p = nullptr;
		errno = e;
	}
	hipError_t alloc(uint64_t count)
	{
		reset();
		const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
		if (e != hipSuccess) p = nullptr;
		return e;
	}
	/* a block of `bytes` bytes from src: at least `least` bytes, rounded up to 16; nothing is copied when there is nothing */
	hipError_t upload_bytes(const void *src, size_t bytes, size_t least)
	{
		reset();
		const hipError_t e = hipMalloc((void **)&p, ((bytes != 0 ? bytes : least) + 15) & ~(size_t)15);
		if (e != hipSuccess) { p = nullptr; return e; }
		return bytes != 0 ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
	}
	hipError_t upload(const std::vector<T> &src) { return upload_bytes(src.data(), src.size() * sizeof(T), sizeof(T)); }
	operator T *() const { return p; }
};

/* pinned host memory */
template <typename T>
struct PinBuf {
	T *p = nullptr;
	PinBuf() = default;
	PinBuf(const PinBuf &) = delete;
	PinBuf &operator=(const PinBuf &) = delete;
	PinBuf(PinBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
	PinBuf &operator=(PinBuf &&o) noexcept
	{
		if (this != &o) { reset(); p = o.p; o.p = nullptr; }
		return *this;
	}
	~PinBuf() { reset(); }
	void reset()
	{
		if (p == nullptr) return;
		const int e = errno;
		(void)hipHostFree(p);
		p = nullptr;
		errno = e;
	}
	hipError_t alloc(uint64_t count)
	{
		reset();
		const hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
		if (e != hipSuccess) p = nullptr;
		return e;
	}
	operator T *() const { return p; }
};

struct DevEvent {
	hipEvent_t e = nullptr;
	DevEvent() = default;
	DevEvent(const DevEvent &) = delete;
	DevEvent &operator=(const DevEvent &) = delete;
	DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
	DevEvent &operator=(DevEvent &&o) noexcept
	{
		if (this != &o) { reset(); e = o.e; o.e = nullptr; }
		return *this;
	}
	~DevEvent() { reset(); }
	void reset()
	{
		if (e == nullptr) return;
		const int en = errno;
		(void)hipEventDestroy(e);
		e = nullptr;
		errno = en;
	}
	hipError_t create() { reset(); return hipEventCreate(&e); }
	hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&e, flags); }   /* hipEventDisableTiming */
	operator hipEvent_t() const { return e; }
};

struct DevStream {
	hipStream_t s = nullptr;
	DevStream() = default;
	DevStream(const DevStream &) = delete;
	DevStream &operator=(const DevStream &) = delete;
	DevStream(DevStream &&o) noexcept : s(o.s) { o.s = nullptr; }
	DevStream &operator=(DevStream &&o) noexcept
	{
		if (this != &o) { reset(); s = o.s; o.s = nullptr; }
		return *this;
	}
	~DevStream() { reset(); }
	void reset()
	{
		if (s == nullptr) return;
		const int e = errno;
		(void)hipStreamDestroy(s);
		s = nullptr;
		errno = e;
	}
	hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&s, flags); }   /* hipStreamNonBlocking */
	operator hipStream_t() const { return s; }
};

#pragma GCC visibility pop

#endif
