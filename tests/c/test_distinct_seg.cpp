/*
 * test_distinct_seg.cpp -- libfsm_amd/csrc/distinct_seg.h on the CPU: the trimmed length, the hash with its split-independent sum,
 * the table size, the slot word, the probe sequence with its wrap, the chunk comparison with its tail mask and the weak hash,
 * against std::map.  A stand-alone program (tests/test_distinct_seg.py builds it with -fsanitize=address,undefined and runs it): it
 * links nothing of HIP.
 *
 * run() inserts the records ONE AFTER THE OTHER, in a given order, exactly as distinct.hip's insert() does for one lane -- the chain
 * from dst_probe_start by dst_probe_next, the first empty slot claimed, on a slot with the record's tag the key of the record it
 * names compared chunk by chunk, the slot lowered to the minimum where the keys are equal -- and then numbers the slots as the
 * number pass does.  Whatever the order, first / count / class must be what the map gives: they are functions of the input alone.
 * Every record's bytes are a heap block of exactly its size: a chunk read past the key stops the program.
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

#include "../../libfsm_amd/csrc/distinct_seg.h"

using namespace fsmhip;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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

/* chunk i of a key of len bytes, assembled byte by byte as the kernel's edge path does: nothing behind the key is read */
void chunk_of(const Rec &r, uint64_t len, uint64_t i, uint64_t *lo, uint64_t *hi)
{
	const uint32_t n = dst_chunk_bytes(len, i);
	assert(n >= 1 && n <= 16);
	uint64_t x0 = 0, x1 = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint64_t b = (uint64_t)r.raw.at(i * DST_CHUNK + k) << ((k & 7u) * 8u);
		if (k < 8u) x0 |= b; else x1 |= b;
	}
	*lo = x0 & dst_mask_lo(n);
	*hi = x1 & dst_mask_hi(n);
}

uint64_t trimmed_len(const Rec &r, int trim) { return dst_trimmed(r.raw.size(), r.raw.empty() ? 0u : r.raw.back(), trim); }

/* the hash lane by lane ... */
uint64_t hash_serial(const Rec &r, uint64_t len, bool tags)
{
	uint64_t sum = 0;
	for (uint64_t i = 0; i < dst_chunks(len); i++) {
		uint64_t lo, hi;
		chunk_of(r, len, i, &lo, &hi);
		sum += dst_chunk_hash(lo, hi, i);
	}
	return dst_hash_finish(sum, len, tags ? r.tag : 0u);
}

/* ... and by `lanes` lanes that take strided chunks and add their partial sums in a tree */
uint64_t hash_split(const Rec &r, uint64_t len, bool tags, uint32_t lanes)
{
	std::vector<uint64_t> part(lanes, 0);
	for (uint32_t l = 0; l < lanes; l++)
		for (uint64_t i = l; i < dst_chunks(len); i += lanes) {
			uint64_t lo, hi;
			chunk_of(r, len, i, &lo, &hi);
			part[l] += dst_chunk_hash(lo, hi, i);
		}
	for (uint32_t d = 1; d < lanes; d <<= 1)
		for (uint32_t l = 0; l + d < lanes; l += 2u * d) part[l] += part[l + d];
	return dst_hash_finish(part[0], len, tags ? r.tag : 0u);
}

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

struct Result {
	std::vector<uint64_t> first, count;
	std::vector<uint32_t> cls;
	uint64_t wraps = 0, tag_hits_unequal = 0, longest = 0;
};

/* the definition */
Result by_map(const std::vector<Rec> &recs, int trim, bool tags)
{
	Result res;
	std::map<std::pair<std::string, uint32_t>, uint32_t> number;
	for (uint64_t r = 0; r < recs.size(); r++) {
		const uint64_t len = trimmed_len(recs[r], trim);
		const std::pair<std::string, uint32_t> key(std::string(recs[r].raw.begin(), recs[r].raw.begin() + (long)len), tags ? recs[r].tag : 0u);
		auto it = number.find(key);
		if (it == number.end()) {
			it = number.emplace(key, (uint32_t)res.first.size()).first;
			res.first.push_back(r);
			res.count.push_back(0);
		}
		res.count[it->second]++;
		res.cls.push_back(it->second);
	}
	return res;
}

/* the table, sequentially, the records in `order` */
Result run(const std::vector<Rec> &recs, int trim, bool tags, bool weak, const std::vector<uint64_t> &order)
{
	const uint64_t R = recs.size(), slots = dst_table_slots(R);
	assert(slots >= DST_MIN_SLOTS && slots >= 2u * R && (slots & (slots - 1u)) == 0u && (slots == DST_MIN_SLOTS || slots / 2u < 2u * R));
	std::vector<uint64_t> table(slots, DST_EMPTY), counter(slots, 0), len(R), hash(R), slot(R);
	Result res;
	for (uint64_t r = 0; r < R; r++) {
		len[r] = trimmed_len(recs[r], trim);
		hash[r] = weak ? dst_weak_hash(len[r], slots) : hash_serial(recs[r], len[r], tags);
		if (weak) assert(dst_probe_start(hash[r], slots) == slots - 4u + (len[r] & 3u));
		assert(dst_slot_word(hash[r], r) != DST_EMPTY && dst_slot_record(dst_slot_word(hash[r], r)) == r);
	}
	for (uint64_t r : order) {
		const uint64_t mine = dst_slot_word(hash[r], r);
		uint64_t i = dst_probe_start(hash[r], slots), steps = 0;
		assert(i < slots);
		for (;; i = dst_probe_next(i, slots), steps++) {
			assert(steps < slots);
			if (dst_probe_next(i, slots) == 0u && table.at(i) != DST_EMPTY) res.wraps++;
			if (table.at(i) == DST_EMPTY) {
				table[i] = mine;
				break;
			}
			if (!dst_same_tag(table[i], mine)) continue;
			const uint64_t q = dst_slot_record(table[i]);
			assert(q < R);
			const bool tag_equal = !tags || recs[q].tag == recs[r].tag;
			if (len[q] != len[r] || !tag_equal || !keys_equal(recs[r], recs[q], len[r])) {
				res.tag_hits_unequal++;
				continue;
			}
			if (q > r) table[i] = std::min(table[i], mine);
			break;
		}
		res.longest = std::max(res.longest, steps);
		counter.at(i)++;
		slot[r] = i;
	}
	/* a key lives in one slot; the number pass */
	std::vector<uint64_t> dense(slots, DST_EMPTY);
	for (uint64_t r = 0; r < R; r++) {
		if (dst_slot_record(table.at(slot[r])) != r) continue;
		dense[slot[r]] = res.first.size();
		res.first.push_back(r);
		res.count.push_back(counter[slot[r]]);
	}
	for (uint64_t r = 0; r < R; r++) {
		assert(dense[slot[r]] != DST_EMPTY);
		res.cls.push_back((uint32_t)dense[slot[r]]);
	}
	return res;
}

void check(const std::vector<Rec> &recs, int trim, bool tags, const char *what, uint64_t *wraps, uint64_t *unequal)
{
	const Result want = by_map(recs, trim, tags);
	std::vector<uint64_t> fwd(recs.size());
	for (uint64_t r = 0; r < recs.size(); r++) fwd[r] = r;
	std::vector<uint64_t> back(fwd.rbegin(), fwd.rend()), mixed(fwd);
	for (uint64_t r = mixed.size(); r > 1; r--) std::swap(mixed[r - 1u], mixed[below(r)]);
	for (int weak = 0; weak < 2; weak++) {
		for (const std::vector<uint64_t> *order : {&fwd, &back, &mixed}) {
			const Result got = run(recs, trim, tags, weak != 0, *order);
			if (got.first != want.first || got.count != want.count || got.cls != want.cls) {
				std::printf("test_distinct_seg: %s differs from the map (weak %d)\n", what, weak);
				std::exit(1);
			}
			if (weak != 0) {
				*wraps += got.wraps;
				*unequal += got.tag_hits_unequal;
			}
		}
	}
	uint64_t sum = 0;
	for (uint64_t c : want.count) sum += c;
	assert(sum == recs.size());
	for (uint64_t d = 1; d < want.first.size(); d++) assert(want.first[d - 1u] < want.first[d]);
}

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

}   // namespace

int main()
{
	/* the arithmetic on its own */
	assert(dst_trimmed(0, '\n', '\n') == 0 && dst_trimmed(1, '\n', '\n') == 0 && dst_trimmed(2, 'a', '\n') == 2 && dst_trimmed(2, '\n', -1) == 2);
	assert(dst_trimmed(5, 0, 0) == 4 && dst_trimmed(5, 255, 255) == 4 && dst_trimmed(5, 255, -1) == 5);
	assert(dst_chunks(0) == 0 && dst_chunks(1) == 1 && dst_chunks(16) == 1 && dst_chunks(17) == 2 && dst_chunks(32) == 2 && dst_chunks(33) == 3);
	assert(dst_chunk_bytes(33, 0) == 16 && dst_chunk_bytes(33, 2) == 1 && dst_chunk_bytes(32, 1) == 16 && dst_chunk_bytes(15, 0) == 15);
	assert(dst_mask_lo(0) == 0 && dst_mask_hi(0) == 0 && dst_mask_lo(8) == ~(uint64_t)0 && dst_mask_hi(8) == 0 && dst_mask_lo(3) == 0xffffffu);
	assert(dst_mask_hi(9) == 0xffu && dst_mask_hi(16) == ~(uint64_t)0 && dst_mask_lo(16) == ~(uint64_t)0);
	assert(dst_chunk_equal(0x11223344u, 7, 0xff223344u, 9, 3) && !dst_chunk_equal(0x11223344u, 7, 0xff223344u, 9, 4));
	assert(dst_chunk_equal(1, 0x0100u, 1, 0x0200u, 9) && !dst_chunk_equal(1, 0x0100u, 1, 0x0200u, 10));
	for (uint64_t R : {0ull, 1ull, 7ull, 8ull, 9ull, 300ull, 65536ull, 65537ull, (unsigned long long)DST_MAX_RECORDS}) {
		const uint64_t s = dst_table_slots(R);
		assert(s >= 16 && s >= 2u * R && (s & (s - 1u)) == 0u && (s == 16 || s < 4u * R));
	}
	assert(dst_table_slots(8) == 16 && dst_table_slots(9) == 32 && dst_table_slots(DST_MAX_RECORDS) == (uint64_t)1 << 33);
	assert(dst_probe_next(15, 16) == 0 && dst_probe_next(14, 16) == 15);
	for (uint64_t slots : {16ull, 1ull << 20, 1ull << 33})
		for (uint64_t len = 0; len < 9; len++) {
			const uint64_t h = dst_weak_hash(len, slots);
			assert(dst_probe_start(h, slots) == slots - 4u + (len & 3u));
			assert(dst_same_tag(dst_slot_word(h, 5), dst_slot_word(dst_weak_hash(len + 4u, slots), 9)));
			assert(!dst_same_tag(dst_slot_word(h, 5), dst_slot_word(dst_weak_hash(len + 1u, slots), 5)));
		}
	assert(dst_slot_word(~(uint64_t)0, DST_MAX_RECORDS - 1u) != DST_EMPTY);

	/* the sum does not depend on the split; the tail is masked; the length and the tag count */
	for (uint64_t len : {0ull, 1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 255ull, 256ull, 257ull, 1000ull, 5000ull}) {
		const Rec r = rec_of(random_string(len, 26), 77);
		const uint64_t h = hash_serial(r, len, true);
		for (uint32_t lanes : {1u, 2u, 3u, 64u}) assert(hash_split(r, len, true, lanes) == h);
		assert(hash_serial(r, len, false) != h);
		if (len != 0) {
			Rec other = r;
			other.raw.back() ^= 1u;
			assert(hash_serial(other, len, true) != h && !keys_equal(r, other, len) && keys_equal(r, other, len - 1u));
			assert(hash_serial(r, len - 1u, true) != h);
		}
	}
	/* zero bytes at the end are bytes: "a" and "a\0" differ */
	assert(hash_serial(rec_of(std::string("a\0", 2)), 2, false) != hash_serial(rec_of("a"), 1, false));

	uint64_t wraps = 0, unequal = 0;
	/* five records in a sixteen-slot table: under the weak hash every chain starts in slots 12 .. 15 and wraps */
	check({rec_of("a"), rec_of("b"), rec_of("c"), rec_of("a"), rec_of("e")}, -1, false, "five records", &wraps, &unequal);
	assert(wraps > 0 && unequal > 0);
	check({}, '\n', false, "no record", &wraps, &unequal);
	check({rec_of("")}, '\n', false, "one empty record", &wraps, &unequal);
	check({rec_of("a\n"), rec_of("a"), rec_of("\n"), rec_of(""), rec_of("a\n\n"), rec_of("ab"), rec_of("abc")}, '\n', false, "the trim byte", &wraps, &unequal);
	{
		const Result w = by_map({rec_of("a\n"), rec_of("a"), rec_of("\n"), rec_of(""), rec_of("a\n\n")}, '\n', false);
		assert(w.first == (std::vector<uint64_t>{0, 2, 4}) && w.count == (std::vector<uint64_t>{2, 2, 1}));
	}
	check({rec_of("x", 1), rec_of("x", 2), rec_of("x", 1), rec_of("y", 2), rec_of("x", 2)}, -1, true, "tags", &wraps, &unequal);
	/* pairs that differ in their last byte only, at the chunk edges; eight records or fewer stay in sixteen slots */
	for (uint64_t len : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull}) {
		std::string a = random_string(len, 26), b = a;
		b.back() = (char)(b.back() ^ 0x40);
		check({rec_of(a), rec_of(b), rec_of(a), rec_of(b + "\n"), rec_of(a.substr(0, len - 1u)), rec_of("")}, '\n', false, "last byte", &wraps, &unequal);
	}
	/* random cases: few keys with heavy repeats, and keys that are mostly different */
	for (int c = 0; c < 300; c++) {
		std::vector<Rec> recs(below(c % 3 == 0 ? 9 : 200));
		const bool tags = c % 4 == 1;
		for (Rec &r : recs) {
			r = rec_of(c % 2 == 0 ? random_string(below(6), 2) : random_string(below(40), 26), (uint32_t)below(3));
			if (below(3) == 0) r.raw.push_back('\n');
		}
		check(recs, c % 5 == 0 ? -1 : '\n', tags, "random", &wraps, &unequal);
	}
	assert(wraps > 100 && unequal > 100);
	std::printf("test_distinct_seg: ok (%llu wraps, %llu equal tags with unequal keys)\n", (unsigned long long)wraps, (unsigned long long)unequal);
	return 0;
}
