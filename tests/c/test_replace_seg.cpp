/*
 * test_replace_seg.cpp -- libfsm_amd/csrc/replace_seg.h on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_replace_abi.py builds and runs it).  For random lines and random WELL-FORMED match lists -- adjacent matches, empty
 * matches, empty replacements (runs of equal mpos), rules beyond the table, MASK with |R| = 0, 1 and 3 -- the output line is
 * spliced by brute force, piece by piece, and every byte of it is compared with what repl_at() names as its source, after the
 * lengths were computed as repl_lengths computes them (repl_clamp_match, repl_uses_table, repl_xlen); the run that repl_at()
 * promises is checked byte by byte, too.  For ILL-FORMED lists (any starts, ends, ids, mpos, xlen) the result is any byte, but
 * every index stays in range: the arrays are exact-size vectors, so ASan is the bound check of the lookups, and the source index
 * is checked against raw and rbytes here.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libfsm_amd/csrc/replace_seg.h"

using namespace fsmhip;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Table {
	std::vector<uint8_t> bytes;
	std::vector<uint64_t> roff;      /* nrepl + 1 */
	uint64_t nrepl() const { return roff.size() - 1u; }
};

static Table table_of(const std::vector<uint64_t> &lens)
{
	Table t;
	t.roff.push_back(0);
	for (uint64_t l : lens) {
		for (uint64_t i = 0; i < l; i++) t.bytes.push_back((uint8_t)(0x80u + rnd() % 0x70u));   /* never a text byte */
		t.roff.push_back(t.bytes.size());
	}
	return t;
}

/* the lengths pass for one line, as repl_lengths does it: mpos, xlen, the output length */
static uint64_t lengths(const std::vector<uint64_t> &start, const std::vector<uint64_t> &end, const std::vector<uint32_t> &id, const Table &t, bool mask,
                        uint64_t raw, std::vector<uint64_t> &mpos, std::vector<uint64_t> &xlen)
{
	uint64_t delta = 0, floor = 0;
	mpos.assign(start.size(), 0);
	xlen.assign(start.size(), 0);
	for (size_t k = 0; k < start.size(); k++) {
		uint64_t st = start[k], en = end[k];
		repl_clamp_match(floor, raw, &st, &en);
		CHECK(floor <= st && st <= en && en <= raw);
		const uint64_t i = id[k], mlen = en - st;
		uint64_t rlen = 0;
		if (i < t.nrepl()) rlen = t.roff[i + 1] - t.roff[i];
		const uint64_t xl = repl_xlen(mlen, repl_uses_table(i, t.nrepl(), rlen, mask), rlen, mask);
		mpos[k] = st + delta;
		xlen[k] = xl;
		delta += xl - mlen;
		floor = en;
	}
	return raw + delta;
}

static uint8_t fetch(const ReplAt &s, uint64_t plus, const std::vector<uint8_t> &text, const Table &t)
{
	if (s.from == REPL_FROM_TEXT) {
		CHECK(s.at + plus < text.size());
		return text[s.at + plus];
	}
	if (s.from == REPL_FROM_TABLE) {
		CHECK(s.at + plus < t.bytes.size());
		return t.bytes[s.at + plus];
	}
	CHECK(s.from == REPL_FROM_NONE);
	return 0;
}

static void well_formed(int round, bool mask)
{
	const uint64_t raw = round < 20 ? (uint64_t)round : rnd() % 120;
	const uint64_t len = raw != 0 && rnd() % 2 ? raw - 1 : raw;       /* a trimmed delimiter, or none */
	std::vector<uint8_t> text(raw);
	for (auto &b : text) b = (uint8_t)('a' + rnd() % 26);
	Table t = table_of(mask ? std::vector<uint64_t>{1, 3, 0, 2} : std::vector<uint64_t>{0, 1, 15, 16, 17, 40, 0, 3});
	/* matches in order inside [0, len]: gaps of 0 (adjacent) or more, lengths of 0 (empty) or more */
	std::vector<uint64_t> start, end;
	std::vector<uint32_t> id;
	const int style = round % 4;                                      /* 0: mixed, 1: all adjacent, 2: all empty, 3: every replacement empty */
	for (uint64_t p = 0; p <= len;) {
		const uint64_t gap = style == 1 ? 0 : rnd() % 4;
		const uint64_t ml = style == 2 ? 0 : rnd() % 6;
		if (p + gap + ml > len) break;
		start.push_back(p + gap);
		end.push_back(p + gap + ml);
		id.push_back(style == 3 ? (mask ? 2u : (rnd() % 2 ? 0u : 6u)) : rnd() % 5 == 0 ? (uint32_t)(t.nrepl() + rnd() % 3) : (uint32_t)(rnd() % t.nrepl()));
		p = end.back() + (ml == 0 ? 1 : 0);                           /* behind an empty match the cursor moves a byte on */
		if (rnd() % 16 == 0) break;
	}
	if (rnd() % 8 == 0 && !id.empty()) id[rnd() % id.size()] = rnd() % 2 ? 0xFFFFFFFEu : 0xFFFFFFFFu;   /* NO_ID, NO_MATCH: stays */
	/* the brute-force splice */
	std::vector<uint8_t> want;
	uint64_t at = 0;
	for (size_t k = 0; k < start.size(); k++) {
		for (uint64_t i = at; i < start[k]; i++) want.push_back(text[i]);
		const uint64_t i = id[k], rlen = i < t.nrepl() ? t.roff[i + 1] - t.roff[i] : 0;
		if (i >= t.nrepl() || (mask && rlen == 0)) {
			for (uint64_t b = start[k]; b < end[k]; b++) want.push_back(text[b]);
		} else if (mask) {
			for (uint64_t b = 0; b < end[k] - start[k]; b++) want.push_back(t.bytes[t.roff[i] + b % rlen]);
		} else {
			for (uint64_t b = 0; b < rlen; b++) want.push_back(t.bytes[t.roff[i] + b]);
		}
		at = end[k];
	}
	for (uint64_t i = at; i < raw; i++) want.push_back(text[i]);
	std::vector<uint64_t> mpos, xlen;
	const uint64_t outlen = lengths(start, end, id, t, mask, raw, mpos, xlen);
	CHECK(outlen == want.size());
	if (mask) CHECK(outlen == raw);
	for (size_t k = 0; k + 1 < mpos.size(); k++) CHECK(mpos[k] <= mpos[k + 1]);
	for (uint64_t q = 0; q < outlen; q++) {
		const ReplAt s = repl_at(mpos.data(), xlen.data(), start.data(), end.data(), id.data(), (uint64_t)start.size(), t.roff.data(), t.nrepl(),
		                         (uint64_t)t.bytes.size(), mask, q, outlen, raw);
		CHECK(s.from != REPL_FROM_NONE && s.run >= 1 && q + s.run <= outlen && s.k <= start.size());
		for (uint64_t r = 0; r < s.run; r++) CHECK(fetch(s, r, text, t) == want[q + r]);
	}
}

static void ill_formed(int round)
{
	const bool mask = round % 2 != 0;
	const uint64_t raw = rnd() % 64;
	std::vector<uint8_t> text(raw, 'x');
	Table t = table_of(round % 5 == 0 ? std::vector<uint64_t>{} : std::vector<uint64_t>{2, 0, 5});
	const size_t nm = rnd() % 12;
	std::vector<uint64_t> start(nm), end(nm), mpos(nm), xlen(nm);
	std::vector<uint32_t> id(nm);
	auto any = [&]() { return rnd() % 3 == 0 ? rnd() : rnd() % 3 == 0 ? UINT64_MAX - rnd() % 4 : rnd() % 80; };
	for (size_t k = 0; k < nm; k++) {
		start[k] = any();
		end[k] = any();
		mpos[k] = any();
		xlen[k] = any();
		id[k] = (uint32_t)any();
	}
	/* the lookup over arrays that belong to nothing ... */
	for (int i = 0; i < 200; i++) {
		const uint64_t q = any(), outlen = any();
		const ReplAt s = repl_at(mpos.data(), xlen.data(), start.data(), end.data(), id.data(), (uint64_t)nm, t.roff.data(), t.nrepl(),
		                         (uint64_t)t.bytes.size(), mask, q, outlen, raw);
		CHECK(s.run >= 1 && s.k <= nm);
		if (s.from == REPL_FROM_TEXT) CHECK(s.at < raw && s.run <= raw - s.at);
		else if (s.from == REPL_FROM_TABLE) CHECK(s.at < t.bytes.size() && s.run <= t.bytes.size() - s.at);
		else CHECK(s.from == REPL_FROM_NONE);
		(void)fetch(s, s.run - 1u, text, t);
	}
	/* ... and the lengths pass over any starts and ends: the clamp keeps every match inside the line and the sum from wrapping */
	std::vector<uint64_t> mp, xl;
	const uint64_t outlen = lengths(start, end, id, t, mask, raw, mp, xl);
	uint64_t most = raw;
	for (size_t k = 0; k < nm; k++) most += xl[k];
	CHECK(outlen <= most);
	for (uint64_t q = 0; q < outlen && q < 300; q++) {
		const ReplAt s = repl_at(mp.data(), xl.data(), start.data(), end.data(), id.data(), (uint64_t)nm, t.roff.data(), t.nrepl(),
		                         (uint64_t)t.bytes.size(), mask, q, outlen, raw);
		CHECK(s.run >= 1);
		(void)fetch(s, s.run - 1u, text, t);
	}
}

int main()
{
	for (int round = 0; round < 4000; round++) {
		well_formed(round, false);
		well_formed(round, true);
	}
	for (int round = 0; round < 4000; round++) ill_formed(round);
	/* the cases by hand: two empty replacements side by side share their mpos, and the byte belongs to the text behind the last */
	{
		const uint8_t text[] = "abcdef";
		const uint64_t start[] = {1, 2}, end[] = {2, 3}, mpos[] = {1, 1}, xlen[] = {0, 0}, roff[] = {0, 0};
		const uint32_t id[] = {0, 0};
		const ReplAt s = repl_at(mpos, xlen, start, end, id, (uint64_t)2, roff, (uint64_t)1, (uint64_t)0, false, (uint64_t)1, (uint64_t)4, (uint64_t)6);
		CHECK(s.from == REPL_FROM_TEXT && s.at == 3 && s.run == 3 && s.k == 1 && text[s.at] == 'd');
		const ReplAt h = repl_at(mpos, xlen, start, end, id, (uint64_t)2, roff, (uint64_t)1, (uint64_t)0, false, (uint64_t)0, (uint64_t)4, (uint64_t)6);
		CHECK(h.from == REPL_FROM_TEXT && h.at == 0 && h.run == 1 && h.k == 2);
	}
	std::printf("test_replace_seg: ok\n");
	return 0;
}
