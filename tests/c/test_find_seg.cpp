/*
 * test_find_seg.cpp -- libfsm_amd/csrc/find_seg.h on the CPU: the lookup of a probe key in a table built by sequential insertion,
 * the bitmap's word and bit, and the pick positions, against std::map.  A stand-alone program (tests/test_find_seg.py builds it with
 * -fsanitize=address,undefined and runs it): it links nothing of HIP.
 *
 * build() inserts the dictionary's records ONE AFTER THE OTHER in a given order, as tests/c/test_distinct_seg.cpp does, and numbers
 * the slots as the number pass does; look() is fnd_lookup over that table, the three reads from vectors.  Whatever the order and
 * the hash, the class of every probe must be what the map gives.  Every record's bytes are a heap block of exactly its size: a
 * chunk read past a key stops the program.
 */
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../libfsm_amd/csrc/find_seg.h"

using namespace fsmhip;

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}
uint64_t below(uint64_t n) { return n == 0 ? 0 : rnd() % n; }

struct Rec {
	std::vector<unsigned char> raw;      /* exactly the record's bytes */
	uint32_t tag = 0;
};

Rec rec_of(const std::string &s, uint32_t tag = 0)
{
	Rec r;
	r.raw.assign(s.begin(), s.end());
	r.tag = tag;
	return r;
}

std::string random_string(uint64_t len, uint32_t letters)
{
	std::string s(len, 'a');
	for (char &c : s) c = (char)('a' + below(letters));
	return s;
}

void chunk_of(const Rec &r, uint64_t len, uint64_t i, uint64_t *lo, uint64_t *hi)
{
	const uint32_t n = dst_chunk_bytes(len, i);
	uint64_t x0 = 0, x1 = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint64_t b = (uint64_t)r.raw.at(i * DST_CHUNK + k) << ((k & 7u) * 8u);
		if (k < 8u) x0 |= b; else x1 |= b;
	}
	*lo = x0 & dst_mask_lo(n);
	*hi = x1 & dst_mask_hi(n);
}

uint64_t trimmed_len(const Rec &r, int trim) { return dst_trimmed(r.raw.size(), r.raw.empty() ? 0u : r.raw.back(), trim); }

uint64_t hash_of(const Rec &r, uint64_t len, bool weak, uint64_t slots)
{
	if (weak) return dst_weak_hash(len, slots);
	uint64_t sum = 0;
	for (uint64_t i = 0; i < dst_chunks(len); i++) {
		uint64_t lo, hi;
		chunk_of(r, len, i, &lo, &hi);
		sum += dst_chunk_hash(lo, hi, i);
	}
	return dst_hash_finish(sum, len, r.tag);
}

/* the keys of two DIFFERENT texts, chunk by chunk */
bool keys_equal(const Rec &a, const Rec &b, uint64_t len)
{
	for (uint64_t i = 0; i < dst_chunks(len); i++) {
		uint64_t alo, ahi, blo, bhi;
		chunk_of(a, len, i, &alo, &ahi);
		chunk_of(b, len, i, &blo, &bhi);
		if (!dst_chunk_equal(alo, ahi, blo, bhi, dst_chunk_bytes(len, i))) return false;
	}
	return true;
}

struct Table {
	uint64_t slots = 0, D = 0;
	std::vector<uint64_t> word, dense, len;
};

/* the dictionary's table: sequential insertion in `order`, then the number pass */
Table build(const std::vector<Rec> &recs, int trim, bool weak, const std::vector<uint64_t> &order)
{
	Table t;
	const uint64_t R = recs.size();
	t.slots = dst_table_slots(R);
	t.word.assign(t.slots, DST_EMPTY);
	t.dense.assign(t.slots, 0);
	t.len.resize(R);
	std::vector<uint64_t> slot(R);
	for (uint64_t r = 0; r < R; r++) t.len[r] = trimmed_len(recs[r], trim);
	for (uint64_t r : order) {
		const uint64_t mine = dst_slot_word(hash_of(recs[r], t.len[r], weak, t.slots), r);
		uint64_t i = dst_probe_start(hash_of(recs[r], t.len[r], weak, t.slots), t.slots);
		for (uint64_t steps = 0;; i = dst_probe_next(i, t.slots), steps++) {
			assert(steps < t.slots);
			if (t.word.at(i) == DST_EMPTY) { t.word[i] = mine; break; }
			if (!dst_same_tag(t.word[i], mine)) continue;
			const uint64_t q = dst_slot_record(t.word[i]);
			if (t.len[q] != t.len[r] || recs[q].tag != recs[r].tag || !keys_equal(recs[r], recs[q], t.len[r])) continue;
			t.word[i] = std::min(t.word[i], mine);
			break;
		}
		slot[r] = i;
	}
	for (uint64_t r = 0; r < R; r++)
		if (dst_slot_record(t.word.at(slot[r])) == r) t.dense[slot[r]] = t.D++;
	return t;
}

struct Walk {
	uint64_t steps = 0, tag_hits_unequal = 0;
	bool wrapped = false;
};

uint32_t look(const Table &t, const std::vector<Rec> &recs, const Rec &probe, int trim, bool weak, Walk *walk)
{
	const uint64_t len = trimmed_len(probe, trim);
	uint64_t last = ~(uint64_t)0;
	return fnd_lookup(
		hash_of(probe, len, weak, t.slots), t.slots, recs.size(),
		[&](uint64_t i) {
			walk->steps++;
			if (last != ~(uint64_t)0 && i < last) walk->wrapped = true;
			last = i;
			return t.word.at(i);
		},
		[&](uint64_t q) {
			const bool eq = t.len.at(q) == len && recs.at(q).tag == probe.tag && keys_equal(probe, recs[q], len);
			if (!eq) walk->tag_hits_unequal++;
			return eq;
		},
		[&](uint64_t i) { return (uint32_t)t.dense.at(i); });
}

struct Seen {
	uint64_t present = 0, absent = 0, wraps_absent = 0, wraps_present = 0, behind_run = 0;
};

/* every probe against the dictionary, under both hashes and three insertion orders */
void check(const std::vector<Rec> &dict, int dtrim, const std::vector<Rec> &probes, int ptrim, const char *what, Seen *seen)
{
	std::map<std::pair<std::string, uint32_t>, uint32_t> number;
	for (const Rec &r : dict) {
		const uint64_t len = trimmed_len(r, dtrim);
		number.emplace(std::make_pair(std::string(r.raw.begin(), r.raw.begin() + (long)len), r.tag), (uint32_t)number.size());
	}
	/* (emplace keeps the first: number.size() before the insertion is the d by first occurrence) */
	std::vector<uint64_t> fwd(dict.size());
	for (uint64_t r = 0; r < dict.size(); r++) fwd[r] = r;
	std::vector<uint64_t> back(fwd.rbegin(), fwd.rend()), mixed(fwd);
	for (uint64_t r = mixed.size(); r > 1; r--) std::swap(mixed[r - 1u], mixed[below(r)]);
	for (int weak = 0; weak < 2; weak++)
		for (const std::vector<uint64_t> *order : {&fwd, &back, &mixed}) {
			const Table t = build(dict, dtrim, weak != 0, *order);
			assert(t.D == number.size());
			for (const Rec &p : probes) {
				const uint64_t len = trimmed_len(p, ptrim);
				const auto it = number.find(std::make_pair(std::string(p.raw.begin(), p.raw.begin() + (long)len), p.tag));
				const uint32_t want = it == number.end() ? FND_NONE : it->second;
				Walk walk;
				const uint32_t got = dict.empty() ? FND_NONE : look(t, dict, p, ptrim, weak != 0, &walk);
				if (got != want) {
					std::printf("test_find_seg: %s: class %u, the map says %u (weak %d)\n", what, got, want, weak);
					std::exit(1);
				}
				assert(walk.steps <= t.slots);
				if (want == FND_NONE) {
					seen->absent++;
					if (walk.wrapped) seen->wraps_absent++;
					if (walk.tag_hits_unequal >= 3) seen->behind_run++;
				} else {
					seen->present++;
					if (walk.wrapped) seen->wraps_present++;
				}
			}
		}
}

}   // namespace

int main()
{
	/* the bitmap and the pick positions */
	assert(fnd_bitmap_words(0) == 0 && fnd_bitmap_words(1) == 1 && fnd_bitmap_words(64) == 1 && fnd_bitmap_words(65) == 2);
	assert(fnd_bitmap_words(DST_MAX_RECORDS) == ((uint64_t)1 << 26));
	assert(fnd_bitmap_word(63) == 0 && fnd_bitmap_bit(63) == 63 && fnd_bitmap_word(64) == 1 && fnd_bitmap_bit(64) == 0 && fnd_bitmap_word(257) == 4);
	for (int c = 0; c < 200; c++) {
		const uint64_t R = below(c % 2 == 0 ? 10 : 700);
		std::vector<bool> present(R);
		uint64_t P = 0;
		for (uint64_t r = 0; r < R; r++) P += (present[r] = c % 7 == 0 ? true : c % 7 == 1 ? false : below(2) != 0) ? 1u : 0u;
		std::vector<uint64_t> pick(R, ~(uint64_t)0), bitmap(fnd_bitmap_words(R), 0);
		uint64_t before = 0;
		for (uint64_t r = 0; r < R; r++) {
			const uint64_t at = present[r] ? fnd_pick_present(before) : fnd_pick_absent(r, before, P);
			assert(at < R && pick.at(at) == ~(uint64_t)0);
			pick[at] = r;
			if (present[r]) bitmap.at(fnd_bitmap_word(r)) |= (uint64_t)1 << fnd_bitmap_bit(r);
			before += present[r] ? 1u : 0u;
		}
		for (uint64_t k = 0; k < R; k++) {
			assert(present[pick[k]] == (k < P) && (bitmap[pick[k] >> 6] >> (pick[k] & 63u) & 1u) == (k < P ? 1u : 0u));
			assert(k == 0 || k == P || pick[k - 1u] < pick[k]);
		}
	}

	Seen seen;
	/* five keys in sixteen slots: under the weak hash the chains of the one-byte keys start in slot 13 and wrap to slot 0, and every
	 * slot of the run has the probe's tag.  "e" is the present key at the end of the wrapped chain; "z" is absent behind the whole
	 * run, across the wrap; "zzzzz" (len & 3 the same) too; "zz" starts at slot 14, inside the run, with another tag */
	const std::vector<Rec> five = {rec_of("a"), rec_of("b"), rec_of("c"), rec_of("a"), rec_of("e"), rec_of("d")};
	check(five, -1, {rec_of("e"), rec_of("d"), rec_of("a"), rec_of("z"), rec_of("zzzzz"), rec_of("zz"), rec_of(""), rec_of("a\n")}, -1, "five keys", &seen);
	assert(seen.wraps_present > 0 && seen.wraps_absent > 0 && seen.behind_run > 0);
	/* no key, no probe, the empty key present and absent */
	check({}, '\n', {rec_of(""), rec_of("a")}, '\n', "no key", &seen);
	check({rec_of("a")}, '\n', {}, '\n', "no probe", &seen);
	check({rec_of("\n"), rec_of("a")}, '\n', {rec_of(""), rec_of("\n"), rec_of("\n\n")}, '\n', "the empty key, present", &seen);
	check({rec_of("a"), rec_of("b")}, '\n', {rec_of(""), rec_of("\n")}, '\n', "the empty key, absent", &seen);
	/* the two sides trim for themselves */
	check({rec_of("a\n"), rec_of("b;")}, '\n', {rec_of("a;"), rec_of("b;;"), rec_of("a\n"), rec_of("b")}, ';', "two trim bytes", &seen);
	check({rec_of("a\n")}, '\n', {rec_of("a\n"), rec_of("a")}, -1, "trim on one side", &seen);
	/* tags */
	check({rec_of("x", 1), rec_of("x", 2), rec_of("y", 0)}, -1, {rec_of("x", 2), rec_of("x", 1), rec_of("x", 0), rec_of("y", 0), rec_of("y", 2)}, -1, "tags", &seen);
	/* keys at the chunk edges: present, and absent by the first and by the last byte alone */
	for (uint64_t len : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 255ull, 256ull, 257ull, 1025ull}) {
		std::vector<Rec> dict, probes;
		for (int k = 0; k < 6; k++) dict.push_back(rec_of(random_string(len, 26)));
		for (const Rec &d : dict) {
			Rec first = d, last = d;
			first.raw.front() ^= 0x40u;
			last.raw.back() ^= 0x01u;
			probes.push_back(d);
			probes.push_back(first);
			probes.push_back(last);
			probes.push_back(rec_of(std::string(d.raw.begin(), d.raw.end() - 1)));
		}
		check(dict, -1, probes, -1, "chunk edges", &seen);
	}
	/* random: few keys with heavy repeats, and keys that are mostly different; about half the probes present */
	for (int c = 0; c < 200; c++) {
		std::vector<Rec> dict(below(c % 3 == 0 ? 9 : 150)), probes(below(120));
		const bool tags = c % 4 == 1;
		for (Rec &r : dict) {
			r = rec_of(c % 2 == 0 ? random_string(below(6), 2) : random_string(below(40), 26), tags ? (uint32_t)below(3) : 0u);
			if (below(3) == 0) r.raw.push_back('\n');
		}
		for (Rec &p : probes) {
			if (!dict.empty() && below(2) == 0) p = dict[below(dict.size())];
			else p = rec_of(c % 2 == 0 ? random_string(below(7), 2) : random_string(below(40), 26), tags ? (uint32_t)below(3) : 0u);
			if (below(4) == 0) p.raw.push_back('\n');
		}
		check(dict, c % 5 == 0 ? -1 : '\n', probes, c % 7 == 0 ? -1 : '\n', "random", &seen);
	}
	assert(seen.present > 1000 && seen.absent > 1000 && seen.wraps_absent > 100 && seen.wraps_present > 100 && seen.behind_run > 100);
	std::printf("test_find_seg: ok (%llu present, %llu absent, %llu + %llu across the wrap, %llu absent behind a run of equal tags)\n",
	            (unsigned long long)seen.present, (unsigned long long)seen.absent, (unsigned long long)seen.wraps_present,
	            (unsigned long long)seen.wraps_absent, (unsigned long long)seen.behind_run);
	return 0;
}
