/*
 * test_sort_seg.cpp -- libfsm_amd/csrc/sort_seg.h on the CPU, a stand-alone program: the rounds of sort.hip run sequentially with
 * the header's arithmetic -- the prefix skip in 16-byte chunks, the word and its valid bytes, the REVERSE complement, the digits of
 * a least-significant-digit radix sort with its skipped passes, the head and active predicates, the positional bookkeeping --
 * against std::stable_sort with a memcmp-and-length comparator: with and without a major key, REVERSE and MAJOR_DESC, in three
 * record orders, key lengths 0, 1, 7, 8, 9, 15, 16, 17 and 3 000, the bytes 0x00, 0x7f, 0x80 and 0xff; and the rounds bound.
 * Built with -fsanitize=address,undefined by tests/test_sort_seg.py.  Links nothing of HIP.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../libfsm_amd/csrc/sort_seg.h"

using namespace fsmhip;

static int failures = 0;
#define CHECK(cond, ...)                                                  \
	do {                                                                  \
		if (!(cond)) {                                                    \
			std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);   \
			std::printf(__VA_ARGS__);                                     \
			std::printf("\n");                                            \
			if (++failures > 20) std::exit(1);                            \
		}                                                                 \
	} while (0)

/* the n (0 .. 16) bytes of key k at byte `at`, as two little-endian words, those behind the n as 0 */
static void load_chunk(const std::string &k, uint64_t at, uint32_t n, uint64_t *lo, uint64_t *hi)
{
	*lo = *hi = 0;
	for (uint32_t i = 0; i < n; i++) {
		const uint64_t b = (uint64_t)(unsigned char)k[at + i] << ((i & 7u) * 8u);
		if (i < 8u) *lo |= b;
		else *hi |= b;
	}
}

struct Result {
	std::vector<uint32_t> order, rank;
	uint64_t rounds = 0, passes = 0, skipped = 0;
};

struct Sim {
	const std::vector<std::string> &keys;
	const std::vector<uint64_t> *major;
	bool reverse, major_desc;
	uint64_t R;
	std::vector<uint32_t> order, bucket, apos;
	std::vector<uint64_t> dep, skip;
	Result res;

	Sim(const std::vector<std::string> &k, const std::vector<uint64_t> *m, bool rev, bool desc) : keys(k), major(m), reverse(rev), major_desc(desc), R(k.size())
	{
		order.resize(R);
		bucket.assign(R, 0u);
		apos.resize(R);
		dep.assign(R, 0u);
		skip.assign(R, ~(uint64_t)0);
		for (uint64_t r = 0; r < R; r++) order[r] = apos[r] = (uint32_t)r;
	}

	void round(bool major_round)
	{
		const uint64_t A = apos.size();
		std::vector<uint64_t> eword(A);
		std::vector<uint32_t> ebkt(A), eval(A), eord(A), perm(A), next(A);
		if (!major_round) {
			for (uint64_t i = 0; i < A; i++) {           /* the prefix skip */
				const uint32_t p = apos[i], B = bucket[p], r = order[p], h = order[B];
				const uint64_t d = dep[p], lr = keys[r].size(), lh = keys[h].size();
				CHECK(d <= lr && d <= lh, "depth %llu beyond a key", (unsigned long long)d);
				const uint64_t m = std::min(lr - d, lh - d);
				uint64_t c = 0;
				while (c < m) {
					const uint32_t n = m - c < SRT_CHUNK ? (uint32_t)(m - c) : SRT_CHUNK;
					uint64_t alo, ahi, blo, bhi;
					load_chunk(keys[r], d + c, n, &alo, &ahi);
					load_chunk(keys[h], d + c, n, &blo, &bhi);
					const uint32_t s = srt_common_chunk(alo, ahi, blo, bhi, n);
					c += s;
					if (s < n) break;
				}
				skip[B] = std::min(skip[B], c);
			}
		}
		for (uint64_t i = 0; i < A; i++) {               /* the entries */
			const uint32_t p = apos[i], B = bucket[p], r = order[p];
			if (major_round) {
				eword[i] = major_desc ? ~(*major)[r] : (*major)[r];
				eval[i] = SRT_WORD;
			} else {
				const uint64_t len = keys[r].size();
				uint64_t d = std::min(dep[p], len);
				d += srt_skip(std::min(skip[B], len - d));
				const uint32_t valid = srt_valid(len, d);
				uint64_t lo, hi;
				load_chunk(keys[r], d, valid, &lo, &hi);
				eword[i] = srt_sort_word(srt_word(lo, valid), reverse);
				eval[i] = srt_sort_valid(valid, reverse);
				CHECK(srt_raw_valid(eval[i], reverse) == valid, "valid does not come back");
				dep[p] = d + SRT_WORD;
			}
			ebkt[i] = B;
			eord[i] = r;
			perm[i] = (uint32_t)i;
		}
		const uint32_t ndigits = SRT_DIGIT_BUCKET + srt_bucket_digits(R);
		CHECK(ndigits <= SRT_DIGITS, "digits");
		for (uint32_t d = 0; d < ndigits; d++) {         /* the stable passes, least significant digit first */
			uint64_t hist[SRT_BINS + 1] = {0};
			for (uint64_t i = 0; i < A; i++) hist[srt_digit(eword[i], eval[i], ebkt[i], d) + 1u]++;
			bool flat = false;
			for (uint32_t b = 0; b < SRT_BINS; b++) flat = flat || hist[b + 1u] == A;
			if (flat) { res.skipped++; continue; }
			res.passes++;
			for (uint32_t b = 0; b < SRT_BINS; b++) hist[b + 1u] += hist[b];
			for (uint64_t i = 0; i < A; i++) {
				const uint32_t e = perm[i];
				next[hist[srt_digit(eword[e], eval[e], ebkt[e], d)]++] = e;
			}
			perm.swap(next);
		}
		std::vector<uint32_t> napos;                     /* the rebucket */
		std::vector<bool> head(A + 1u, true);
		for (uint64_t i = 1; i < A; i++) {
			const uint32_t e = perm[i], q = perm[i - 1u];
			head[i] = srt_head(false, ebkt[e], eword[e], eval[e], ebkt[q], eword[q], eval[q]);
		}
		std::vector<uint32_t> nord(A);
		for (uint64_t i = 0; i < A; i++) nord[i] = eord[perm[i]];
		uint32_t last = 0;
		for (uint64_t i = 0; i < A; i++) {
			const uint32_t p = apos[i], e = perm[i];
			order[p] = nord[i];
			if (head[i]) last = p;
			CHECK(last >= bucket[p] && last <= p, "a bucket left its parent");
			bucket[p] = last;
			if (srt_active(head[i], i + 1u < A && !head[i + 1u], major_round ? SRT_WORD : srt_raw_valid(eval[e], reverse))) {
				napos.push_back(p);
				if (head[i]) skip[p] = ~(uint64_t)0;
			}
		}
		apos.swap(napos);
	}

	Result run()
	{
		if (R < 2u) apos.clear();
		if (!apos.empty() && major != nullptr) round(true);
		while (!apos.empty()) {
			round(false);
			res.rounds++;
			CHECK(res.rounds < 1000u, "no end");
			if (res.rounds >= 1000u) break;
		}
		res.order = order;
		res.rank.resize(R);
		uint32_t g = 0;
		for (uint64_t p = 0; p < R; p++) {
			if (bucket[p] == p) g++;
			res.rank[p] = g - 1u;
		}
		return res;
	}
};

static int key_cmp(const std::string &a, const std::string &b)
{
	const size_t n = std::min(a.size(), b.size());
	const int c = n != 0 ? std::memcmp(a.data(), b.data(), n) : 0;
	if (c != 0) return c;
	return a.size() < b.size() ? -1 : a.size() > b.size();
}

static void one(const std::vector<std::string> &keys, const std::vector<uint64_t> *major, bool reverse, bool major_desc, const char *what)
{
	const uint64_t R = keys.size();
	std::vector<uint32_t> want(R);
	for (uint64_t r = 0; r < R; r++) want[r] = (uint32_t)r;
	auto less = [&](uint32_t x, uint32_t y) {
		if (major != nullptr && (*major)[x] != (*major)[y]) return major_desc ? (*major)[x] > (*major)[y] : (*major)[x] < (*major)[y];
		const int c = key_cmp(keys[x], keys[y]);
		return reverse ? c > 0 : c < 0;
	};
	std::stable_sort(want.begin(), want.end(), less);
	Sim sim(keys, major, reverse, major_desc);
	const Result got = sim.run();
	uint64_t maxlen = 0;
	bool all_equal = true;
	for (uint64_t r = 0; r < R; r++) {
		maxlen = std::max<uint64_t>(maxlen, keys[r].size());
		all_equal = all_equal && keys[r] == keys[0];
	}
	CHECK(got.order == want, "%s: order (R = %llu)", what, (unsigned long long)R);
	uint32_t g = 0;
	for (uint64_t p = 0; p < R; p++) {
		if (p != 0 && (less(want[p - 1u], want[p]) || less(want[p], want[p - 1u]))) g++;
		CHECK(got.rank[p] == g, "%s: rank[%llu] = %u, not %u", what, (unsigned long long)p, got.rank[p], g);
		if (got.rank[p] != g) break;
	}
	CHECK(got.rounds <= srt_rounds_bound(maxlen), "%s: %llu rounds for keys of at most %llu bytes", what, (unsigned long long)got.rounds, (unsigned long long)maxlen);
	if (all_equal) CHECK(got.rounds <= 2u, "%s: %llu rounds for equal keys", what, (unsigned long long)got.rounds);
}

static void every_form(std::vector<std::string> keys, const char *what)
{
	uint64_t seed = 12345;
	for (int ord = 0; ord < 3; ord++) {
		if (ord == 1) std::reverse(keys.begin(), keys.end());
		if (ord == 2)
			for (size_t i = keys.size(); i > 1; i--) {
				seed = seed * 6364136223846793005ull + 1442695040888963407ull;
				std::swap(keys[i - 1u], keys[(seed >> 33) % i]);
			}
		std::vector<uint64_t> major(keys.size()), same(keys.size(), 7u);
		for (size_t r = 0; r < keys.size(); r++) major[r] = r % 5u == 0u ? 0u : r % 5u == 1u ? ~(uint64_t)0 : r % 5u == 2u ? (uint64_t)1 << 40 : 3u;
		for (int rev = 0; rev < 2; rev++) {
			one(keys, nullptr, rev != 0, false, what);
			one(keys, &major, rev != 0, false, what);
			one(keys, &major, rev != 0, true, what);
			one(keys, &same, rev != 0, true, what);
		}
	}
}

int main()
{
	/* the arithmetic by hand */
	CHECK(srt_word(0x0000000000006261ull, 2u) == 0x6162000000000000ull, "ab");
	CHECK(srt_word(0xffffffffffffffffull, 0u) == 0u && srt_word(0x1122334455667788ull, 8u) == 0x8877665544332211ull, "tail");
	CHECK(srt_valid(10u, 8u) == 2u && srt_valid(16u, 8u) == 8u && srt_valid(8u, 8u) == 0u && srt_valid(3u, 9u) == 0u, "valid");
	CHECK(srt_common_chunk(0u, 0u, 0u, 0u, 16u) == 16u && srt_common_chunk(0u, 0u, 0u, 0u, 5u) == 5u, "equal chunks");
	CHECK(srt_common_chunk(0xff00u, 0u, 0x0100u, 0u, 16u) == 1u && srt_common_chunk(1u, 0u, 0u, 0u, 16u) == 0u, "low word");
	CHECK(srt_common_chunk(7u, (uint64_t)1 << 56, 7u, 0u, 16u) == 15u && srt_common_chunk(7u, 1u, 7u, 0u, 3u) == 3u, "high word");
	CHECK(srt_skip(7u) == 0u && srt_skip(8u) == 8u && srt_skip(3000u) == 3000u && srt_skip(3004u) == 3000u, "skip");
	CHECK(srt_bucket_digits(0u) == 0u && srt_bucket_digits(1u) == 0u && srt_bucket_digits(2u) == 1u && srt_bucket_digits(256u) == 1u && srt_bucket_digits(257u) == 2u &&
	      srt_bucket_digits(65537u) == 3u && srt_bucket_digits(SRT_MAX_RECORDS) == 4u, "bucket digits");
	CHECK(srt_digit(0x1122334455667788ull, 5u, 0xa1b2c3d4u, 0u) == 5u && srt_digit(0x1122334455667788ull, 5u, 0xa1b2c3d4u, 1u) == 0x88u &&
	      srt_digit(0x1122334455667788ull, 5u, 0xa1b2c3d4u, 8u) == 0x11u && srt_digit(0u, 0u, 0xa1b2c3d4u, 9u) == 0xd4u && srt_digit(0u, 0u, 0xa1b2c3d4u, 12u) == 0xa1u, "digits");
	CHECK(srt_rounds_bound(0u) == 1u && srt_rounds_bound(8u) == 2u && srt_rounds_bound(9u) == 3u && srt_rounds_bound(65u) == 10u, "bound");
	CHECK(srt_active(true, true, 8u) && srt_active(false, false, 8u) && !srt_active(true, false, 8u) && !srt_active(false, true, 7u), "active");

	/* every length with every byte, the last byte changed, and each twice */
	const size_t lens[] = {0, 1, 7, 8, 9, 15, 16, 17, 3000};
	const unsigned char fill[] = {0x00, 0x7f, 0x80, 0xff};
	std::vector<std::string> keys;
	for (size_t n : lens)
		for (unsigned char b : fill) {
			std::string k(n, (char)b);
			keys.push_back(k);
			if (n != 0) {
				k[n - 1u] = (char)(b ^ 0x80);
				keys.push_back(k);
				k[n - 1u] = (char)b;
				k[0] = (char)(b ^ 0x01);
				keys.push_back(k);
			}
			keys.push_back(std::string(n, (char)b));
		}
	every_form(keys, "every length and byte");
	every_form({"", std::string(1, '\0'), std::string(2, '\0'), "ab", std::string("ab\0", 3), "abcdefgh", std::string("abcdefgh\0", 9), "abcdefghi", "abcdefgh"}, "edges");
	every_form(std::vector<std::string>(100, std::string(3000, 'x')), "equal keys of 3 000 bytes");
	every_form(std::vector<std::string>(300, ""), "empty keys");
	every_form({}, "no record");
	every_form({"one"}, "one record");
	{
		std::vector<std::string> ab;
		for (size_t i = 0; i < 64; i++) ab.push_back(std::string(i, 'a') + "b");
		every_form(ab, "a^i b");
		std::vector<std::string> shared;                 /* a shared prefix of 20 bytes and two letters behind it */
		for (size_t i = 0; i < 700; i++) shared.push_back("2024-01-02T03:04:05 " + std::string(1, (char)('a' + i % 3)) + std::string(1, (char)('a' + i % 7)));
		every_form(shared, "shared prefix");
		Sim sim(shared, nullptr, false, false);
		const Result r = sim.run();
		CHECK(r.rounds <= 2u, "the prefix skip: %llu rounds", (unsigned long long)r.rounds);
	}
	if (failures != 0) return 1;
	std::printf("test_sort_seg: ok\n");
	return 0;
}
