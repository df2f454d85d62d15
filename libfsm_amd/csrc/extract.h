/*
 * extract.h -- what another unit reads of extract.hip: the extracted object, whose packed text the distinct records take as their
 * input, and the write pass (ext_write) with its arguments and its block, which writes the distinct keys as well.  Not part of the
 * C ABI.
 */
#ifndef FSMHIP_CSRC_EXTRACT_H
#define FSMHIP_CSRC_EXTRACT_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "front.h"

/* lengths pass (per MATCH: kept, the record's bytes, its first byte, its input; per block of EXT_MATCHES matches the pair records /
 * bytes) -> exclusive scan of the BLOCK pairs by one workgroup -> ONE wait for the two totals -> allocation -> offsets pass (the
 * block's own scan redone, the compaction, first[]) -> write pass.  The scan runs over total / EXT_MATCHES records.  The offsets
 * and the write pass are in flight at return. */
struct __attribute__((visibility("hidden"))) fsm_hip_extracted : RunObject<4> {   /* the lengths, the scan, the offsets, the write pass */
	size_t nrec = 0;
	uint64_t nbytes = 0;
	int sep = -1;                            /* the separator the records were made with */
	DevBuf<uint64_t> d_off;                  /* nrec + 1 */
	DevBuf<uint64_t> d_line, d_match;        /* nrec */
	DevBuf<uint64_t> d_src;                  /* nrec: internal */
	DevBuf<uint64_t> d_mrec, d_msrc, d_mline;   /* one per match: internal */
	DevBuf<uint64_t> d_pairs;                /* per block of matches, + the totals: internal */
	DevBuf<uint64_t> d_first;                /* per block of the output, + 1: internal */
	DevBuf<unsigned char> d_bytes;           /* nbytes, in whole blocks */
};

namespace fsmhip {

constexpr uint32_t EXT_THREADS = 256;
constexpr uint32_t EXT_TILES = 4;
constexpr uint32_t EXT_TILE = EXT_THREADS * 16u;            /* output bytes one store instruction of the workgroup covers */
constexpr uint32_t EXT_BLOCK = EXT_TILES * EXT_TILE;        /* output bytes a workgroup writes per step: 16 KiB */

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself, so it spells the batch's fields
 * out, as the replacement's does: extracted_new copies them from a LineBatch. */
struct ExtRun {
	/* the batch */
	const void *base = nullptr;
	const uint64_t *off = nullptr;           /* n + 1 */
	const uint64_t *pick = nullptr;          /* m, or null: input j is line j */
	uint64_t n = 0, m = 0, limit = 0;
	/* the matches */
	const uint64_t *moff = nullptr;          /* m + 1 */
	const uint64_t *start = nullptr, *end = nullptr;   /* nmatch */
	const uint32_t *id = nullptr;
	uint64_t nmatch = 0;
	/* the rule set (null: every match is kept) and the separator (-1: none) */
	const uint32_t *keep = nullptr;          /* nrules bits in words of 32 */
	uint64_t nrules = 0;
	bool keep_other = false;
	int sep = -1;
	/* per match, internal: (the record's bytes) * 2 + kept, the text index of its first byte, its input */
	uint64_t *mrec = nullptr, *msrc = nullptr, *mline = nullptr;
	uint64_t *pairs = nullptr;               /* per block of EXT_MATCHES matches (records kept, bytes), then (scanned) those before it */
	/* the object's arrays, sized after the scan */
	uint64_t *out_off = nullptr;             /* nrec + 1 */
	uint64_t *src = nullptr, *line = nullptr, *match = nullptr;   /* nrec each */
	uint64_t *first = nullptr;               /* ngb + 1 */
	unsigned char *out = nullptr;            /* ngb * EXT_BLOCK */
	uint64_t nrec = 0, total = 0, ngb = 0;   /* known after the scan */
	uint64_t wgs = 1, per = 1;               /* the write pass's grid: wgs workgroups of `per` consecutive output blocks */
};

/* ext_write on stream s, the objects' device current; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int ext_launch_write(const ExtRun &r, hipStream_t s);

}

#endif
