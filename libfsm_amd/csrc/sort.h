/*
 * sort.h -- what another unit reads of sort.hip: the sort of a packed text that lies on the device, for the unit whose object
 * holds such a text (distinct.hip sorts its keys, with its counts as the major key).  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_SORT_H
#define FSMHIP_CSRC_SORT_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

struct fsm_hip_sorted;

namespace fsmhip {

/* what every form refuses alike: a byte argument outside -1 .. 255, an unknown flag bit (`allowed`: the form's), MAJOR_DESC without
 * a major key (EINVAL), R above 2^32 - 2 (EOVERFLOW) */
__attribute__((visibility("hidden"))) bool sort_args(size_t R, int trim_byte, int sep_byte, unsigned flags, unsigned allowed, bool has_major);

/* the sorted object over device arrays on stream s, `device` current, behind `after` (or nothing); NULL + errno */
__attribute__((visibility("hidden"))) struct fsm_hip_sorted *sorted_new(int device, const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes,
	int trim_byte, const uint64_t *d_major, int sep_byte, unsigned flags, hipEvent_t after, hipStream_t s);

}

#endif
