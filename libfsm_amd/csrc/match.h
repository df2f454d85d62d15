/*
 * match.h -- what another unit reads of match.hip: the matches object, whose arrays the replacement, the extraction and the tally
 * take as their input.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_MATCH_H
#define FSMHIP_CSRC_MATCH_H

#include <cstdint>

#include "front.h"

/* marks pass -> count pass -> exclusive scan of the counts by one workgroup -> ONE wait for the total -> allocation -> emit
 * pass.  The counts are scanned in place, as the tokens' are: d_off is count[m] first, match_off[m + 1] afterwards. */
struct __attribute__((visibility("hidden"))) fsm_hip_matches : RunObject<4> {   /* the marks pass, the count pass, the scan, the emit pass */
	size_t total = 0;
	DevBuf<uint16_t> d_marks;                /* marks_words(limit, n): internal */
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_start, d_end;         /* total each */
	DevBuf<uint32_t> d_id;                   /* total */
};

#endif
