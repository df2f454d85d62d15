/*
 * tok.h -- what another unit reads of tok.hip: of a struct fsm_hip_tok_dfa (defined there) its device and its image as a walk
 * reads it, for match.hip; and the tokens object, whose offsets and ids the tally counts.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_TOK_H
#define FSMHIP_CSRC_TOK_H

#include <cstdint>

#include "front.h"

struct fsm_hip_tok_dfa;

/* count pass -> exclusive scan of the counts by one workgroup -> ONE wait for the total -> allocation -> emit pass.  The counts
 * are scanned in place: d_off is count[m] first, tok_off[m + 1] afterwards (the total lands in its last entry). */
struct __attribute__((visibility("hidden"))) fsm_hip_tokens : RunObject<3> {   /* the count pass, the scan, the emit pass */
	size_t total = 0;
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_err;                  /* m */
	DevBuf<uint64_t> d_end;                  /* total */
	DevBuf<uint32_t> d_id;                   /* total */
};

namespace fsmhip {

/* the image as walk_tok reads it (image.h, TokImage), for match.hip; every pointer is device memory and lives as long as the image */
struct TokView {
	const void *tab = nullptr;               /* [entries]: u16 (LDS form) or u32, the end-state bit of the target folded in */
	const uint16_t *col = nullptr;           /* [256] */
	const uint32_t *ids = nullptr;           /* by TokImage::id_index() */
	uint32_t entries = 0, C = 0;
	uint32_t start = 0, abs_min = 0;         /* in the walk's unit */
	uint32_t in_lds = 0;
};

__attribute__((visibility("hidden"))) int tok_dfa_device(const fsm_hip_tok_dfa *td);
__attribute__((visibility("hidden"))) TokView tok_dfa_view(const fsm_hip_tok_dfa *td);

}

#endif
