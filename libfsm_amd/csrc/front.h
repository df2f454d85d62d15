/*
 * front.h -- the skeleton the host fronts of the text objects share (tokens, matches, replaced, extracted, distinct; the text,
 * its hits and its spans use the helpers): is there a device, the grid of a pass over blocks, "wait for the last event, then copy
 * out / sum the event pairs", and the object of NPASS passes on a stream with ONE wait in the middle -- the passes before it leave
 * counts, one workgroup scans them, the host reads the total and sizes the arrays by it, the passes after it fill them and are in
 * flight at return.  Their input is one LineBatch (line_batch.h), whichever of the three entry forms it came through.  Not part of
 * the C ABI: everything here has hidden visibility.  Host code only, as hip_host.h is: it needs no device compiler
 * (tests/c/test_front.cpp compiles it with g++ against counting stand-ins).  The two scans are declared here and live in
 * text.hip, beside the sum_scan their kernels instantiate.
 */
#ifndef FSMHIP_CSRC_FRONT_H
#define FSMHIP_CSRC_FRONT_H

#include <hip/hip_runtime_api.h>

#include <initializer_list>
#include <new>

#include "hip_host.h"
#include "line_batch.h"

#pragma GCC visibility push(hidden)

constexpr uint32_t FRONT_WG_PER_CU = 8;                     /* 8 x 4 wavefronts: a full CU */

inline bool have_device()
{
	int ndev = 0;
	return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

inline unsigned max_workgroups(int dev)
{
	int ncu = 0;
	if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
	return (unsigned)ncu * FRONT_WG_PER_CU;
}

/* the grid for nblocks blocks: at most max_workgroups workgroups of `per` consecutive blocks each, none without a block (one
 * workgroup for no block: the kernels that run then do their first thread's work alone) */
struct Grid {
	uint64_t wgs = 1, per = 1;
};
inline Grid grid_of(uint64_t nblocks, int dev)
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
inline int copy_out(int device, hipEvent_t done, std::initializer_list<OutCopy> copies)
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
inline double elapsed_ms(int device, hipEvent_t done, const EventPair *pairs, size_t npairs)
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
inline double elapsed_ms(int device, hipEvent_t done, std::initializer_list<EventPair> pairs) { return elapsed_ms(device, done, pairs.begin(), pairs.size()); }

/* what every such object begins with: events ev[2p], ev[2p + 1] around pass p; the last one: all is there */
template <int NPASS>
struct RunObject {
	static constexpr int npass = NPASS;
	int device = 0;
	size_t m = 0;
	DevEvent ev[2 * NPASS];
	hipEvent_t done() const { return ev[2 * NPASS - 1]; }
	bool begin(int pass, hipStream_t s) { return HIP_OK(hipEventRecord(ev[2 * pass], s)); }
	bool end(int pass, hipStream_t s) { return HIP_OK(hipEventRecord(ev[2 * pass + 1], s)); }
};

template <typename T>
inline void run_free(T *o)
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
inline T *run_new(int device, uint64_t m, bool grid_fits, hipStream_t s, Passes passes)
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
inline auto run_host(int device, const fsmhip::LineBatch &host, Make make) -> decltype(make(host, hipStream_t()))
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
inline double run_ms(const T *o, int from, int to)
{
	if (o == nullptr || from < 0 || to >= T::npass) { errno = EINVAL; return -1.0; }
	EventPair pairs[T::npass];
	for (int p = from; p <= to; p++) pairs[p - from] = {o->ev[2 * p], o->ev[2 * p + 1]};
	return elapsed_ms(o->device, o->done(), pairs, (size_t)(to - from + 1));
}

/* The scan pass and the ONE wait of a run: cnt[0 .. k) scanned in place, exclusive, by one workgroup, the total in cnt[k] (k ==
 * 0: cnt[0] is cleared and nothing waits), `after` recorded, the total read back.  0, or -1 + errno. */
int scan_total(uint64_t *cnt, uint64_t k, hipEvent_t after, hipStream_t s, uint64_t *total);

/* The scan of nblocks pairs of words in place, exclusive, by one workgroup on stream s, the two totals (and whatever the caller
 * keeps behind them) from pairs[2 * nblocks] on; nothing is launched for no block.  0, or -1 + errno. */
int pairs_scan_launch(uint64_t *pairs, uint64_t nblocks, hipStream_t s);

#pragma GCC visibility pop

#endif
