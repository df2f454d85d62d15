/*
 * replace.h -- how text.hip launches the passes of the replacement (replace.hip): repl_lengths, repl_offsets, repl_write.  The
 * fronts (the table, the replaced object, the scan of the block sums) are in text.hip.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_REPLACE_H
#define FSMHIP_CSRC_REPLACE_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fsmhip {

constexpr uint32_t REPL_THREADS = 256;
constexpr uint32_t REPL_LINES = REPL_THREADS;               /* inputs of a block of the lengths and the offsets pass, one per lane */
constexpr uint32_t REPL_TILES = 4;
constexpr uint32_t REPL_TILE = REPL_THREADS * 16u;          /* output bytes one store instruction of the workgroup covers */
constexpr uint32_t REPL_BLOCK = REPL_TILES * REPL_TILE;     /* output bytes a workgroup writes per step: 16 KiB */
/* the table is read from LDS by the write pass when its bytes and its rules are both within these: 16 KiB + 4 KiB of a CU's
 * 160 KiB, so eight workgroups still fit a CU */
constexpr uint32_t REPL_LDS_BYTES = 16384;
constexpr uint32_t REPL_LDS_RULES = 1023;

inline bool repl_table_fits_lds(uint64_t nrepl, uint64_t rbytes) { return nrepl <= REPL_LDS_RULES && rbytes <= REPL_LDS_BYTES; }
/* a table with nins inserts: its insert offsets and its positions, two bytes each, take their room out of the 16 KiB of bytes, behind
 * the table's bytes rounded up to 16 -- so every position and every insert offset fits a u16 */
inline bool repl_tmpl_fits_lds(uint64_t nrepl, uint64_t rbytes, uint64_t nins)
{
	return repl_table_fits_lds(nrepl, rbytes) && nins <= REPL_LDS_BYTES && ((rbytes + 15u) & ~(uint64_t)15u) + 2u * (nrepl + 1u) + 2u * nins <= REPL_LDS_BYTES;
}

/* m inputs fit one launch's grid */
inline bool repl_grid_fits(uint64_t m) { return (m + REPL_LINES - 1u) / REPL_LINES <= 0x7fffffffu; }

/* the passes' arguments; every pointer is device memory.  The kernels take this struct itself, so it spells the batch's fields
 * out where TokRun and MatchRun carry a LineBatch (line_batch.h): text.hip copies them from one. */
struct ReplRun {
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
	/* the table */
	const unsigned char *rbytes_p = nullptr;
	const uint64_t *roff = nullptr;          /* nrepl + 1 */
	uint64_t nrepl = 0, rbytes = 0;
	unsigned flags = 0;                      /* FSM_HIP_REPL_* */
	bool table_in_lds = false;
	/* the object's arrays */
	uint64_t *out_off = nullptr;             /* m + 1: the lengths pass leaves the lengths, the offsets pass the offsets */
	uint64_t *mpos = nullptr, *xlen = nullptr;   /* nmatch each */
	uint64_t *sums = nullptr;                /* blocks of REPL_LINES inputs: their bytes, then (scanned) the bytes before them */
	uint64_t *first = nullptr;               /* ngb + 1 */
	unsigned char *out = nullptr;            /* ngb * REPL_BLOCK */
	uint64_t total = 0, ngb = 0;             /* known after the scan */
	uint64_t wgs = 1, per = 1;               /* the write pass's grid: wgs workgroups of `per` consecutive output blocks */
	/* the table's inserts (a template table with at least one): last, so that the fields above stay where the plain kernels read them */
	const uint64_t *ioff = nullptr;          /* nrepl + 1, or null: no rule has an insert */
	const uint64_t *ins = nullptr;           /* nins positions */
	uint64_t nins = 0;
};

/* the table has inserts: the template kernels run, for every other table the plain ones */
inline bool repl_is_template(const ReplRun &r) { return r.nins != 0 && r.ioff != nullptr && r.ins != nullptr; }

/* each on stream s, the objects' device current; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int repl_launch_lengths(const ReplRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int repl_launch_offsets(const ReplRun &r, hipStream_t s);
__attribute__((visibility("hidden"))) int repl_launch_write(const ReplRun &r, hipStream_t s);

}

#endif
