/*
 * match.h -- how text.hip launches the passes of the matches (match.hip): walk_mark over a struct fsm_hip_pos_dfa, then
 * walk_match<false> / walk_match<true> over a struct fsm_hip_tok_dfa.  The fronts (the matches object, its scan) are in
 * text.hip; the batch a pass runs over is line_batch.h's.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_MATCH_H
#define FSMHIP_CSRC_MATCH_H

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "line_batch.h"

struct fsm_hip_pos_dfa;
struct fsm_hip_tok_dfa;

namespace fsmhip {

constexpr uint32_t MATCH_THREADS = 256;      /* inputs per workgroup, one per lane */

/* m inputs fit one launch's grid */
inline bool match_grid_fits(uint64_t m) { return (m + MATCH_THREADS - 1u) / MATCH_THREADS <= 0x7fffffffu; }

/* one pass over m inputs; every pointer is device memory */
struct MatchRun {
	LineBatch in;                            /* its limit always given (the marks are sized by it); flags: FSM_HIP_MATCHES_* */
	uint16_t *marks = nullptr;               /* marks_words(limit, n) words (match_marks.h): walk_mark writes, walk_match reads */
	uint64_t nwords = 0;
	uint64_t *count = nullptr;               /* the count pass writes it: m */
	const uint64_t *match_off = nullptr;     /* the emit pass reads it: m + 1 */
	uint64_t *start_out = nullptr, *end_out = nullptr;   /* ... and stores at match_off[j] + t */
	uint32_t *id_out = nullptr;
};

/* walk_mark on stream s, the image's device current; 0, or -1 + errno */
__attribute__((visibility("hidden"))) int match_launch_mark(const fsm_hip_pos_dfa *starts, const MatchRun &r, hipStream_t s);
/* walk_match<emit> */
__attribute__((visibility("hidden"))) int match_launch(const fsm_hip_tok_dfa *ends, const MatchRun &r, bool emit, hipStream_t s);

}

#endif
