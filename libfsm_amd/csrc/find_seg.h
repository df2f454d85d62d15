/*
 * find_seg.h -- the arithmetic of the lookup of a packed text's records among the keys of a distinct object (distinct.hip, the
 * fnd_* kernels; include/fsm_hip.h, "find"): no HIP header, so that tests/c/test_find_seg.cpp checks it on the CPU against std::map.
 * Not part of the C ABI.
 *
 *   Lookup.  The table is the one distinct_seg.h describes, as the insert and the number pass left it: a slot is tag32(hash) << 32 |
 *   the lowest r of its key, or DST_EMPTY, and beside every taken slot stands the dense number d of its key.  A probe walks the chain
 *   of ITS hash from dst_probe_start by dst_probe_next, at most `slots` steps: an empty slot ends it (slots are never emptied, so a
 *   key that is in the table lies before the first empty slot of its chain); a slot with another tag, or one that names no record of
 *   the dictionary, is passed; on a slot with its tag the KEYS are compared -- length, tag, bytes: equal hashes decide nothing -- and
 *   where they are equal the slot's dense number is the class.  Nothing is written.  fnd_lookup is that walk, with the three reads
 *   (the slot word, the key comparison, the dense number) handed in: the kernels read the table by agent-scope atomic loads, the CPU
 *   test from vectors.
 *   Bitmap.  Bit r & 63 of word r >> 6; ceil(R / 64) words; a block of 256 records is four words, a wavefront's ballot is one.
 *   Pick.  With before(r) the present records below r and P all of them: a present r stands at before(r), an absent one at
 *   P + r - before(r), which is P + the absent records below r.
 */
#ifndef FSMHIP_CSRC_FIND_SEG_H
#define FSMHIP_CSRC_FIND_SEG_H

#include <cstdint>

#include "distinct_seg.h"

namespace fsmhip {

constexpr uint32_t FND_NONE = 0xffffffffu;                /* D <= 2^32 - 2: no key's number */

/* the class of the key with this hash: slot_word(i) is the word of slot i, key_equal(q) compares the probe's key with that of the
 * dictionary's record q (< R_dict), dense(i) is the number beside slot i */
template <typename SlotWord, typename KeyEqual, typename Dense>
FSMHIP_DST_FN uint32_t fnd_lookup(uint64_t hash, uint64_t slots, uint64_t R_dict, SlotWord slot_word, KeyEqual key_equal, Dense dense)
{
	const uint64_t mine = dst_slot_word(hash, 0u);
	uint64_t i = dst_probe_start(hash, slots);
	for (uint64_t step = 0; step < slots; step++, i = dst_probe_next(i, slots)) {
		const uint64_t cur = slot_word(i);
		if (cur == DST_EMPTY) return FND_NONE;
		if (!dst_same_tag(cur, mine)) continue;
		const uint64_t q = dst_slot_record(cur);
		if (q >= R_dict) continue;
		if (key_equal(q)) return dense(i);
	}
	return FND_NONE;
}

FSMHIP_DST_FN uint64_t fnd_bitmap_words(uint64_t R) { return R / 64u + (R % 64u != 0u ? 1u : 0u); }
FSMHIP_DST_FN uint64_t fnd_bitmap_word(uint64_t r) { return r >> 6; }
FSMHIP_DST_FN uint32_t fnd_bitmap_bit(uint64_t r) { return (uint32_t)(r & 63u); }

/* where r stands in pick: before = the present records below r, P = all present records */
FSMHIP_DST_FN uint64_t fnd_pick_present(uint64_t before) { return before; }
FSMHIP_DST_FN uint64_t fnd_pick_absent(uint64_t r, uint64_t before, uint64_t P) { return P + (r - before); }

}

#endif
