/*
 * line_batch.h -- the input every text front takes, said once: lines off[0 .. n] of a packed text `base`, optionally picked by
 * pick[0 .. m), clipped to `limit`, with an optional trimmed last byte.  Here are its description (LineBatch), what the fronts
 * refuse about it, where the pieces of a host batch lie in the one staging allocation, and the owner of that allocation.  Not
 * part of the C ABI: everything here has hidden visibility.  Host code only, as hip_host.h is: it needs no device compiler
 * (tests/c/test_line_batch.cpp compiles it with g++ against counting stand-ins).
 */
#ifndef FSMHIP_CSRC_LINE_BATCH_H
#define FSMHIP_CSRC_LINE_BATCH_H

#include <initializer_list>

#include "hip_host.h"

#pragma GCC visibility push(hidden)

namespace fsmhip {

/* m inputs over n lines; every pointer is device memory once staged */
struct LineBatch {
	const void *base = nullptr;
	const uint64_t *off = nullptr;           /* n + 1 */
	const uint64_t *pick = nullptr;          /* m, or null: input j is line j */
	uint64_t n = 0, m = 0;
	uint64_t limit = 0;                      /* has_limit: the bytes of base that may be read; else off[n] is */
	bool has_limit = false;
	int trim = -1;
	unsigned flags = 0;                      /* the front's own */
};

/* The shape of a public batch (fsm_hip_tok_batch, fsm_hip_match_batch, fsm_hip_pos_batch name these fields alike), read into
 * *lb as it stands.  false + EINVAL: no batch, trim_byte outside -1 .. 255, a flag outside `mask`, off NULL with inputs. */
template <typename B>
inline bool batch_shape(const B *b, unsigned mask, LineBatch *lb)
{
	if (b == nullptr || (b->flags & ~mask) != 0u || b->trim_byte < -1 || b->trim_byte > 255) { errno = EINVAL; return false; }
	lb->base = b->base;
	lb->off = b->off;
	lb->pick = b->pick;
	lb->n = b->n;
	lb->m = b->pick != nullptr ? (uint64_t)b->m : (uint64_t)b->n;
	lb->limit = b->limit;
	lb->has_limit = b->limit != 0u || b->base == nullptr;   /* no text: no byte may be read */
	lb->trim = b->trim_byte;
	lb->flags = b->flags;
	if (lb->m != 0 && lb->off == nullptr) { errno = EINVAL; return false; }
	return true;
}

/* a batch of host arrays: false + EINVAL for offsets that decrease, bytes without a text, a pick at or beyond n */
inline bool batch_host_arrays_ok(const LineBatch &b)
{
	if (b.m == 0) return true;                       /* nothing is read, nothing is looked at */
	for (uint64_t i = 0; i < b.n; i++)
		if (b.off[i] > b.off[i + 1u]) { errno = EINVAL; return false; }
	if (b.base == nullptr && b.off[b.n] != 0u) { errno = EINVAL; return false; }
	if (b.pick != nullptr)
		for (uint64_t j = 0; j < b.m; j++)
			if (b.pick[j] >= b.n) { errno = EINVAL; return false; }
	return true;
}

/* a batch of device arrays: false + EINVAL for bytes that may be read of no text */
inline bool batch_device_ok(const LineBatch &b)
{
	if (b.base == nullptr && b.limit != 0u) { errno = EINVAL; return false; }
	return true;
}

/* limit == 0 says off[n] (device form): read it on stream s, a short wait of its own, for the fronts that size by the limit */
inline bool batch_read_limit(LineBatch *b, hipStream_t s)
{
	if (b->m != 0 && b->limit == 0u && b->base != nullptr) {
		uint64_t last = 0;
		if (!HIP_OK(hipMemcpyAsync(&last, b->off + b->n, sizeof last, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return false;
		b->limit = last;
	}
	b->has_limit = true;
	return true;
}

/* Where the pieces of a host batch lie in the one staging allocation: the text at 0, the offsets, the pick, then up to
 * STAGE_EXTRAS more arrays of m u64 (the spans' from / to / first_out / last_out; bit k of `extras`: extra k is there), each
 * piece at a multiple of 16 bytes; a piece that is not there takes no room. */
constexpr int STAGE_EXTRAS = 4;
struct StageLayout {
	uint64_t at_off = 0, at_pick = 0, at_extra[STAGE_EXTRAS] = {0, 0, 0, 0}, all = 0;
};
inline uint64_t stage_up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
inline StageLayout stage_layout(uint64_t nbytes, uint64_t n, uint64_t m, bool has_pick, unsigned extras = 0u)
{
	StageLayout L;
	L.at_off = stage_up16(nbytes);
	L.at_pick = L.at_off + stage_up16((n + 1u) * 8u);
	L.all = L.at_pick + (has_pick ? stage_up16(m * 8u) : 0u);
	for (int k = 0; k < STAGE_EXTRAS; k++) {
		L.at_extra[k] = L.all;
		if ((extras >> k & 1u) != 0u) L.all += stage_up16(m * 8u);
	}
	return L;
}

/* an extra array of m u64 behind the pick, there when the caller's `host` is: uploaded from it, or (an output) room alone */
struct StageExtra {
	const void *host = nullptr;
	bool upload = true;
};

/* The owner of the one staging allocation of a host batch.  Its user waits for the stream before it goes. */
struct StagedBatch {
	DevBuf<unsigned char> d;
	StageLayout at;
	unsigned extras = 0u;                    /* bit k: extra k is there */

	/* Allocate, issue the uploads on stream s (never the NULL stream: the caller's own) and give the batch as the device sees it
	 * in *dev: off[n] bytes of text, which is the limit.  A batch without inputs stages nothing.  false + errno when it fails;
	 * after a failed upload the stream is idle and the memory gone. */
	bool stage(const LineBatch &host, hipStream_t s, LineBatch *dev, std::initializer_list<StageExtra> more = {})
	{
		*dev = host;
		dev->base = nullptr;
		dev->off = dev->pick = nullptr;
		dev->limit = 0;
		dev->has_limit = true;
		if (host.m == 0) return true;
		const uint64_t nbytes = host.off[host.n], n_m = host.m * 8u;
		int k = 0;
		extras = 0u;
		for (const StageExtra &x : more) extras |= (x.host != nullptr ? 1u : 0u) << k++;
		at = stage_layout(nbytes, host.n, host.m, host.pick != nullptr, extras);
		if (!HIP_OK(d.alloc(at.all))) return false;
		bool ok = nbytes == 0 || HIP_OK(hipMemcpyAsync(d, host.base, nbytes, hipMemcpyHostToDevice, s));
		ok = ok && HIP_OK(hipMemcpyAsync(d + at.at_off, host.off, (host.n + 1u) * 8u, hipMemcpyHostToDevice, s));
		ok = ok && (host.pick == nullptr || HIP_OK(hipMemcpyAsync(d + at.at_pick, host.pick, n_m, hipMemcpyHostToDevice, s)));
		k = 0;
		for (const StageExtra &x : more) {
			ok = ok && (x.host == nullptr || !x.upload || HIP_OK(hipMemcpyAsync(d + at.at_extra[k], x.host, n_m, hipMemcpyHostToDevice, s)));
			k++;
		}
		if (!ok) {   /* the stream idle before the staging memory goes */
			const int e = errno;
			(void)hipStreamSynchronize(s);
			d.reset();
			errno = e;
			return false;
		}
		dev->base = nbytes != 0 ? d.p : nullptr;
		dev->limit = nbytes;
		dev->off = (const uint64_t *)(d + at.at_off);
		dev->pick = host.pick != nullptr ? (const uint64_t *)(d + at.at_pick) : nullptr;
		return true;
	}
	/* extra k on the device, or null when it is not there */
	uint64_t *extra(int k) const { return (extras >> k & 1u) != 0u ? (uint64_t *)(d.p + at.at_extra[k]) : nullptr; }
};

}

#pragma GCC visibility pop

#endif
