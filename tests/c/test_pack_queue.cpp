/* libfsm_amd/csrc/pack_queue.h on the host: one wavefront's pending queue driven by the ballots on stdin.
 *
 * Each input line is one tile: the ballot "alive after the first 16 bytes" and the ballot "alive after the first segment", as
 * hex.  Per tile the program prints
 *   I                                   the tile is walked in place (the queue is not touched), or
 *   Q <count after the push> <fired 0|1> <count after the pop> <position of every survivor, in lane order>
 * and at the end  F <entries left for the flush>.  tests/test_ldsdma_pack_cases.py holds that against its own model. */
#include <cinttypes>
#include <cstdio>

#include "../../libfsm_amd/csrc/pack_queue.h"

int main()
{
	using namespace fsmhip;
	uint32_t count = 0;
	uint64_t live16, live;
	std::printf("M %u\n", (unsigned)PACK_MAX_LIVE);
	while (std::scanf("%" SCNx64 " %" SCNx64, &live16, &live) == 2) {
		if (pack_in_place(live16)) {
			std::printf("I\n");
			continue;
		}
		const uint32_t pushed = pack_push(count, live);
		const bool fired = pack_fires(pushed);
		std::printf("Q %u %d %u", (unsigned)pushed, fired ? 1 : 0, (unsigned)(fired ? pack_pop(pushed) : pushed));
		for (uint32_t lane = 0; lane < 64; lane++)
			if ((live >> lane) & 1u) std::printf(" %u", (unsigned)pack_pos(count, live, lane));
		std::printf("\n");
		count = fired ? pack_pop(pushed) : pushed;
		if (pack_fires(count)) {   /* one walk per tile must be enough: count < 64 before every push */
			std::printf("OVERFLOW\n");
			return 1;
		}
	}
	std::printf("F %u\n", (unsigned)count);
	return 0;
}
