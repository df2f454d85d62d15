/*
 * tally.h -- how text.hip launches the tally (tally.hip, tally_spans).  The fronts (the checks, the clearing of the tables, the
 * staging of the host forms) are in text.hip.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_TALLY_H
#define FSMHIP_CSRC_TALLY_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fsmhip {

constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_WINDOW = TALLY_THREADS;            /* entries a workgroup takes a step, one per lane */
constexpr uint32_t TALLY_SPAN = 64;                         /* inputs of a granule: a workgroup takes whole granules */
constexpr uint32_t TALLY_LDS_COLS = 4096;                   /* columns counted in LDS: 2 x 16 KiB of u32, count and lines */
constexpr uint32_t TALLY_LINE_COLS = 65536;                 /* columns of the bitmap of one input: 8 KiB of LDS */
constexpr uint32_t TALLY_WG_PER_CU = 3;                     /* 47 KiB of LDS a workgroup: three fit a CU's 160 KiB */

/* the kernel's arguments; every pointer is device memory.  count or lines may be null, not both; group_off null: one group. */
struct TallyRun {
	const uint64_t *off = nullptr;           /* m + 1 */
	const uint32_t *id = nullptr;            /* total */
	uint64_t m = 0, total = 0;
	const uint64_t *group_off = nullptr;     /* ngroups + 1, or null */
	uint64_t ngroups = 1;
	uint64_t nrules = 0;                     /* nrules + 1 columns */
	uint64_t *count = nullptr, *lines = nullptr;   /* ngroups * (nrules + 1) each */
	uint64_t per = 1;                        /* granules of a workgroup; set by the launch */
};

/* on stream s, `device` current; m >= 1 and total >= 1.  0, or -1 + errno */
__attribute__((visibility("hidden"))) int tally_launch(TallyRun r, int device, hipStream_t s);

}

#endif
