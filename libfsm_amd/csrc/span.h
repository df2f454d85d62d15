/*
 * span.h -- what text.hip and match.hip may know about a struct fsm_hip_pos_dfa (defined in span.hip): its device, and where
 * its image lies on the device.  The accept-position walks themselves go through the public fsm_hip_exec_accept_pos_device.
 * Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_SPAN_H
#define FSMHIP_CSRC_SPAN_H

#include <cstdint>

struct fsm_hip_pos_dfa;

namespace fsmhip {

constexpr uint32_t POS_LDS_ENTRIES = 16384;  /* a table of up to this many (state, class) entries is walked from LDS */

/* the image as walk_pos reads it; every pointer is device memory and lives as long as the image */
struct PosView {
	const void *tab = nullptr;               /* [entries]: u16 (LDS form) or u32, the end-state bit of the target folded in */
	const uint16_t *col = nullptr;           /* [256] */
	uint32_t entries = 0, C = 0;
	uint32_t start = 0, abs_min = 0;         /* in the walk's unit */
	uint32_t in_lds = 0;
};

__attribute__((visibility("hidden"))) int pos_dfa_device(const fsm_hip_pos_dfa *pd);
__attribute__((visibility("hidden"))) PosView pos_dfa_view(const fsm_hip_pos_dfa *pd);
}

#endif
