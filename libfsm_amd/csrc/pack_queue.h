/*
 * pack_queue.h -- the bookkeeping of walk_ldsdma_pack's pending queue (walk_kernels.h), host and device.
 *
 * A wavefront keeps the rows that outlive their first segment in a queue of up to 128 entries (two register sets of 64:
 * positions 0-63 and 64-127) and walks positions 0-63 as one packed tile whenever 64 are pending.  Everything here is
 * arithmetic on the wave-uniform count and a 64-bit lane ballot: no HIP type, so that tests/test_ldsdma_pack_cases.py can
 * compile it with a plain C++ compiler and hold it against a model.
 */
#ifndef FSM_HIP_PACK_QUEUE_H
#define FSM_HIP_PACK_QUEUE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSMHIP_HD __host__ __device__
#else
#define FSMHIP_HD
#endif

namespace fsmhip {

/* a tile with more live rows than this after its first 16 bytes is walked in place (walk_ldsdma's own loop) */
#ifndef FSMHIP_PACK_MAX_LIVE
#define FSMHIP_PACK_MAX_LIVE 48
#endif
constexpr uint32_t PACK_MAX_LIVE = FSMHIP_PACK_MAX_LIVE;
constexpr uint32_t PACK_TILE = 64;       /* rows of a packed walk: one per lane */
static_assert(PACK_MAX_LIVE <= PACK_TILE, "count < 64 before a push and <= 64 new entries: two sets of 64 hold them");

FSMHIP_HD inline uint32_t pack_popc(uint64_t m) { return (uint32_t)__builtin_popcountll((unsigned long long)m); }

/* the first decision of a tile, from the ballot "alive after 16 bytes" */
FSMHIP_HD inline bool pack_in_place(uint64_t live) { return pack_popc(live) > PACK_MAX_LIVE; }

/* queue position of the survivor in `lane` (bit `lane` of `live` is set): behind the `count` pending entries, in row order */
FSMHIP_HD inline uint32_t pack_pos(uint32_t count, uint64_t live, uint32_t lane)
{
	return count + pack_popc(live & (((uint64_t)1 << lane) - 1u));
}

/* the count after a tile's survivors went in; a packed walk of positions 0-63 fires while it is >= 64 */
FSMHIP_HD inline uint32_t pack_push(uint32_t count, uint64_t live) { return count + pack_popc(live); }
FSMHIP_HD inline bool pack_fires(uint32_t count) { return count >= PACK_TILE; }
/* ... and after that walk: the second set moves into the first */
FSMHIP_HD inline uint32_t pack_pop(uint32_t count) { return count - PACK_TILE; }

} // namespace fsmhip

#endif
