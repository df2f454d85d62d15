/*
 * tok.h -- what text.hip may know about a struct fsm_hip_tok_dfa (defined in tok.hip): its device, and how one pass of the
 * tokeniser's walk is launched.  The fronts (the tokens object, its scan) are in text.hip; the batch a pass runs over is
 * line_batch.h's.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_TOK_H
#define FSMHIP_CSRC_TOK_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "line_batch.h"

struct fsm_hip_tok_dfa;

namespace fsmhip {

constexpr uint32_t TOK_THREADS = 256;        /* inputs per workgroup, one per lane */

/* one pass over m inputs; every pointer is device memory */
struct TokRun {
	LineBatch in;                            /* flags: FSM_HIP_TOKENS_* */
	uint64_t *count = nullptr, *err = nullptr;           /* the count pass writes them: m each */
	const uint64_t *tok_off = nullptr;                   /* the emit pass reads it: m + 1 */
	uint64_t *end_out = nullptr;                         /* ... and stores at tok_off[j] + t */
	uint32_t *id_out = nullptr;
};

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
/* walk_tok<emit> on stream s, td's device current; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int tok_launch(const fsm_hip_tok_dfa *td, const TokRun &r, bool emit, hipStream_t s);

}

#endif
