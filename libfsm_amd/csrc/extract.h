/*
 * extract.h -- how text.hip launches the passes of the extraction (extract.hip): ext_lengths, ext_offsets, ext_write.  The
 * fronts (the rule set, the extracted object, the scan of the block pairs) are in text.hip.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_EXTRACT_H
#define FSMHIP_CSRC_EXTRACT_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fsmhip {

constexpr uint32_t EXT_THREADS = 256;
constexpr uint32_t EXT_MATCHES = EXT_THREADS;               /* matches of a block of the lengths and the offsets pass, one per lane */
constexpr uint32_t EXT_TILES = 4;
constexpr uint32_t EXT_TILE = EXT_THREADS * 16u;            /* output bytes one store instruction of the workgroup covers */
constexpr uint32_t EXT_BLOCK = EXT_TILES * EXT_TILE;        /* output bytes a workgroup writes per step: 16 KiB */

/* nmatch matches fit one launch's grid */
inline bool ext_grid_fits(uint64_t nmatch) { return (nmatch + EXT_MATCHES - 1u) / EXT_MATCHES <= 0x7fffffffu; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself, so it spells the batch's fields
 * out, as ReplRun does: text.hip copies them from a LineBatch. */
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

/* each on stream s, the objects' device current; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int ext_launch_lengths(const ExtRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int ext_launch_offsets(const ExtRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int ext_launch_write(const ExtRun &r, hipStream_t s);

}

#endif
