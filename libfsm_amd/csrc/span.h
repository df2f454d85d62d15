/*
 * span.h -- what text.hip may know about a struct fsm_hip_pos_dfa (defined in span.hip): its device.  The walks themselves
 * go through the public fsm_hip_exec_accept_pos_device.  Not part of the C ABI.
 */
#ifndef FSMHIP_CSRC_SPAN_H
#define FSMHIP_CSRC_SPAN_H

struct fsm_hip_pos_dfa;

namespace fsmhip {
__attribute__((visibility("hidden"))) int pos_dfa_device(const fsm_hip_pos_dfa *pd);
}

#endif
