/*
 * distinct.h -- how text.hip launches the passes of the distinct records (distinct.hip).  The fronts (the checks, the object, the
 * scan of the block pairs, the write pass, which is the extraction's) are in text.hip.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_DISTINCT_H
#define FSMHIP_CSRC_DISTINCT_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fsmhip {

constexpr uint32_t DST_THREADS = 256;
constexpr uint32_t DST_RECORDS = DST_THREADS;               /* records of a block of every pass, one per lane */
constexpr uint32_t DST_LONG_BYTES = 256;                    /* keys above it are hashed by a wavefront each */
constexpr uint32_t DST_PAIRS_EXTRA = 4;                     /* behind the block pairs: the two totals, the limit, the long records */

constexpr uint64_t dst_blocks(uint64_t R) { return (R + DST_RECORDS - 1u) / DST_RECORDS; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself. */
struct DstRun {
	/* the packed text */
	const uint64_t *off = nullptr;           /* R + 1 */
	const unsigned char *bytes = nullptr;
	const uint32_t *tag = nullptr;           /* R, or null */
	uint64_t R = 0, nbytes = 0;
	int trim = -1, sep = -1;
	bool weak = false;
	/* internal, sized by R */
	uint64_t slots = 0;
	uint64_t *len = nullptr;                 /* R: the trimmed lengths */
	uint64_t *hash = nullptr;                /* R: the hashes; from the insert pass on, the slot of each record */
	uint32_t *cls = nullptr;                 /* R: class; until the insert pass, the list of the long records */
	uint64_t *table = nullptr, *cnt = nullptr;   /* slots each: the slot words; the records of a slot, then its dense number */
	uint64_t *pairs = nullptr;               /* per block (firsts, key bytes), then (scanned) those before it; + DST_PAIRS_EXTRA */
	/* the object's arrays, sized after the scan */
	uint64_t *first = nullptr, *count = nullptr;   /* D each */
	uint64_t *doff = nullptr;                /* D + 1, or null (NO_TEXT) */
	uint64_t *src = nullptr;                 /* D: where each key's bytes begin in `bytes`; with doff */
	uint64_t *bfirst = nullptr;              /* ngb + 1: the key that covers the first byte of each output block; with doff */
	uint64_t D = 0, total = 0, ngb = 0;      /* known after the scan */
};

/* each on stream s, the object's device current, R >= 1; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int dst_launch_hash(const DstRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int dst_launch_insert(const DstRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int dst_launch_mark(const DstRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int dst_launch_number(const DstRun &r, hipStream_t s);

}

#endif
