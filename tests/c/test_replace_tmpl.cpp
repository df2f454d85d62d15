/*
 * test_replace_tmpl.cpp -- the template form of libfsm_amd/csrc/replace_seg.h on the CPU, under AddressSanitizer and
 * UndefinedBehaviorSanitizer (tests/test_template_seg.py builds and runs it).  A template table has, per rule, insert positions at
 * which the match's own bytes stand inside the replacement (include/fsm_hip.h, "replace").  For random lines, WELL-FORMED match
 * lists and well-formed templates -- 0, 1, 2, 3 and 255 inserts, equal positions, an insert at 0 and one at |R|, empty matches, an
 * empty R, matches of 1, 15, 16, 17 and 40 bytes, rules beyond the table -- the output line is spliced by brute force, piece by
 * piece, and for every output byte q the source that the template repl_at() names is compared with it, and its run with the rest of
 * the piece q lies in: the longest stretch the splice allows.  The lengths are computed as repl_lengths computes them.  For
 * ILL-FORMED arrays (positions that descend or exceed |R|, more inserts than the cap, insert offsets beyond the positions, xlen and
 * mpos that belong to nothing) the result is any byte, but the source is in range, the run at least 1, and a walk over the line by
 * runs ends: the arrays are exact-size vectors, so ASan is the bound check of the lookups.  Where no rule has an insert the answer
 * is the plain repl_at()'s, field by field.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libfsm_amd/csrc/replace_seg.h"

using namespace fsmhip;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
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
	std::vector<uint64_t> ioff;      /* nrepl + 1 */
	std::vector<uint64_t> ins;
	uint64_t nrepl() const { return roff.size() - 1u; }
	uint64_t rlen(uint64_t i) const { return roff[i + 1] - roff[i]; }
	void rule(uint64_t len, const std::vector<uint64_t> &at)
	{
		if (roff.empty()) { roff.push_back(0); ioff.push_back(0); }
		for (uint64_t i = 0; i < len; i++) bytes.push_back((uint8_t)(0x80u + rnd() % 0x70u));   /* never a text byte */
		roff.push_back(bytes.size());
		for (uint64_t a : at) ins.push_back(a);
		ioff.push_back(ins.size());
	}
};

/* c ascending positions in 0 .. len; style 0: any, 1: all equal, 2: the first at 0 and the last at len */
static std::vector<uint64_t> positions(uint64_t len, uint64_t c, int style)
{
	std::vector<uint64_t> at(c);
	uint64_t last = 0;
	const uint64_t same = rnd() % (len + 1);
	for (uint64_t s = 0; s < c; s++) {
		if (style == 1) at[s] = same;
		else at[s] = last = last + rnd() % (len - last + 1) / (rnd() % 3 + 1);
	}
	if (style == 2 && c != 0) { at[0] = 0; at[c - 1] = len; }
	return at;
}

/* a well-formed table: rules of 0, 1, 2, 3 and 255 inserts in literals of 0 .. 40 bytes, and some without any */
static Table random_table(int round)
{
	static const uint64_t counts[] = {0, 1, 2, 3, 255, 1, 0, 2};
	static const uint64_t lens[] = {0, 1, 15, 16, 17, 40, 3, 0};
	Table t;
	for (int i = 0; i < 8; i++) {
		const uint64_t len = lens[(i + round) % 8], c = round % 7 == 6 ? 0 : counts[(i + round / 8) % 8];
		t.rule(len, positions(len, c, (round / 3 + i) % 3));
	}
	return t;
}

/* the lengths pass for one line, as repl_lengths<true> does it */
static uint64_t lengths(const std::vector<uint64_t> &start, const std::vector<uint64_t> &end, const std::vector<uint32_t> &id, const Table &t, uint64_t raw,
                        std::vector<uint64_t> &mpos, std::vector<uint64_t> &xlen)
{
	uint64_t delta = 0, floor = 0;
	mpos.assign(start.size(), 0);
	xlen.assign(start.size(), 0);
	for (size_t k = 0; k < start.size(); k++) {
		uint64_t st = start[k], en = end[k];
		repl_clamp_match(floor, raw, &st, &en);
		CHECK(floor <= st && st <= en && en <= raw);
		const uint64_t i = id[k], mlen = en - st;
		uint64_t xl = mlen;
		if (i < t.nrepl()) {
			const uint64_t r0 = t.roff[i], r1 = t.roff[i + 1];
			uint64_t i0;
			xl = repl_xlen(mlen, r1 > r0 ? r1 - r0 : 0u, repl_inserts_of(t.ioff.data(), i, t.nrepl(), (uint64_t)t.ins.size(), &i0));
		}
		mpos[k] = st + delta;
		xlen[k] = xl;
		delta += xl - mlen;
		floor = en;
	}
	return raw + delta;
}

static ReplAt at_of(const std::vector<uint64_t> &mpos, const std::vector<uint64_t> &xlen, const std::vector<uint64_t> &start, const std::vector<uint64_t> &end,
                    const std::vector<uint32_t> &id, const Table &t, uint64_t q, uint64_t outlen, uint64_t raw)
{
	return repl_at(mpos.data(), xlen.data(), start.data(), end.data(), id.data(), (uint64_t)start.size(), t.roff.data(), t.ioff.data(), t.ins.data(), t.nrepl(),
	               (uint64_t)t.bytes.size(), (uint64_t)t.ins.size(), q, outlen, raw);
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

/* the brute-force splice: the bytes, and for every byte how many bytes of its piece are left -- a piece is one stretch of the text
 * between two matches, one literal stretch of a template, one copy of a match */
struct Splice {
	std::vector<uint8_t> bytes;
	std::vector<uint64_t> left;
	void piece(const uint8_t *p, uint64_t n)
	{
		for (uint64_t i = 0; i < n; i++) {
			bytes.push_back(p[i]);
			left.push_back(n - i);
		}
	}
};

static void well_formed(int round)
{
	static const uint64_t sizes[] = {1, 15, 16, 17, 40};
	const uint64_t raw = round < 20 ? (uint64_t)round : rnd() % 200;
	const uint64_t len = raw != 0 && rnd() % 2 ? raw - 1 : raw;       /* a trimmed delimiter, or none */
	std::vector<uint8_t> text(raw);
	for (auto &b : text) b = (uint8_t)('a' + rnd() % 26);
	const Table t = random_table(round);
	std::vector<uint64_t> start, end;
	std::vector<uint32_t> id;
	const int style = round % 4;                                      /* 0: mixed, 1: all adjacent, 2: all empty, 3: the sizes 1, 15, 16, 17, 40 */
	for (uint64_t p = 0; p <= len;) {
		const uint64_t gap = style == 1 ? 0 : rnd() % 4;
		const uint64_t ml = style == 2 ? 0 : style == 3 ? sizes[rnd() % 5] : rnd() % 6;
		if (p + gap + ml > len) break;
		start.push_back(p + gap);
		end.push_back(p + gap + ml);
		id.push_back(rnd() % 5 == 0 ? (uint32_t)(t.nrepl() + rnd() % 3) : (uint32_t)(rnd() % t.nrepl()));
		p = end.back() + (ml == 0 ? 1 : 0);
		if (rnd() % 16 == 0) break;
	}
	if (rnd() % 8 == 0 && !id.empty()) id[rnd() % id.size()] = rnd() % 2 ? 0xFFFFFFFEu : 0xFFFFFFFFu;   /* NO_ID, NO_MATCH: stays */
	Splice want;
	uint64_t at = 0;
	for (size_t k = 0; k < start.size(); k++) {
		want.piece(text.data() + at, start[k] - at);
		const uint64_t i = id[k], ml = end[k] - start[k];
		if (i >= t.nrepl()) {
			want.piece(text.data() + start[k], ml);
		} else if (ml == 0 || t.ioff[i] == t.ioff[i + 1]) {               /* X = R[i]: one piece */
			want.piece(t.bytes.data() + t.roff[i], t.rlen(i));
		} else {
			uint64_t last = 0;
			for (uint64_t x = t.ioff[i]; x < t.ioff[i + 1]; x++) {
				want.piece(t.bytes.data() + t.roff[i] + last, t.ins[x] - last);
				want.piece(text.data() + start[k], ml);
				last = t.ins[x];
			}
			want.piece(t.bytes.data() + t.roff[i] + last, t.rlen(i) - last);
		}
		at = end[k];
	}
	want.piece(text.data() + at, raw - at);
	std::vector<uint64_t> mpos, xlen;
	const uint64_t outlen = lengths(start, end, id, t, raw, mpos, xlen);
	CHECK(outlen == want.bytes.size());
	for (size_t k = 0; k + 1 < mpos.size(); k++) CHECK(mpos[k] <= mpos[k + 1]);
	const bool plain = t.ins.empty();
	for (uint64_t q = 0; q < outlen; q++) {
		const ReplAt s = at_of(mpos, xlen, start, end, id, t, q, outlen, raw);
		CHECK(s.from != REPL_FROM_NONE && s.k <= start.size());
		CHECK(s.run == want.left[q]);
		for (uint64_t r = 0; r < s.run; r++) CHECK(fetch(s, r, text, t) == want.bytes[q + r]);
		if (plain) {                                                  /* no rule has an insert: the plain lookup, field by field */
			const ReplAt p = repl_at(mpos.data(), xlen.data(), start.data(), end.data(), id.data(), (uint64_t)start.size(), t.roff.data(), t.nrepl(),
			                         (uint64_t)t.bytes.size(), false, q, outlen, raw);
			CHECK(p.from == s.from && p.at == s.at && p.run == s.run && p.k == s.k);
		}
	}
}

static void check_in_range(const ReplAt &s, uint64_t nm, uint64_t raw, const std::vector<uint8_t> &text, const Table &t)
{
	CHECK(s.run >= 1 && s.k <= nm);
	if (s.from == REPL_FROM_TEXT) CHECK(s.at < raw && s.run <= raw - s.at);
	else if (s.from == REPL_FROM_TABLE) CHECK(s.at < t.bytes.size() && s.run <= t.bytes.size() - s.at);
	else CHECK(s.from == REPL_FROM_NONE);
	(void)fetch(s, s.run - 1u, text, t);
}

static void ill_formed(int round)
{
	const uint64_t raw = rnd() % 64;
	std::vector<uint8_t> text(raw, 'x');
	auto any = [&]() { return rnd() % 3 == 0 ? rnd() : rnd() % 3 == 0 ? UINT64_MAX - rnd() % 4 : rnd() % 80; };
	/* the table's literals are well-formed (fsm_hip_repl_create_template refuses others); the inserts are not */
	Table t;
	const int kind = round % 5;
	for (int i = 0; i < 3 && round % 11 != 0; i++) {
		const uint64_t len = i == 1 ? 0 : 2 + rnd() % 9;
		std::vector<uint64_t> at(kind == 3 ? 300 + rnd() % 300 : rnd() % 6);                  /* 3: a count above the cap */
		for (auto &a : at) a = kind == 0 ? rnd() % (len + 1) : kind == 1 ? len + 1 + rnd() % 5 : kind == 2 ? any() : rnd() % (len + 1);
		t.rule(len, at);                                              /* 0, 3: positions that descend; 1: that exceed |R|; 2: anything */
	}
	if (t.roff.empty()) { t.roff.push_back(0); t.ioff.push_back(0); }
	if (kind == 4)                                                    /* insert offsets that belong to nothing */
		for (auto &o : t.ioff) o = any();
	const size_t nm = rnd() % 12;
	std::vector<uint64_t> start(nm), end(nm), mpos(nm), xlen(nm);
	std::vector<uint32_t> id(nm);
	for (size_t k = 0; k < nm; k++) {
		start[k] = any();
		end[k] = any();
		mpos[k] = any();
		xlen[k] = any();
		id[k] = rnd() % 2 ? (uint32_t)(rnd() % 4) : (uint32_t)any();
	}
	/* the lookup over arrays that belong to nothing: xlen disagrees with everything ... */
	for (int i = 0; i < 200; i++) check_in_range(at_of(mpos, xlen, start, end, id, t, any(), any(), raw), nm, raw, text, t);
	/* ... and over the lengths pass's own arrays for any starts and ends: the walk by runs covers the line in at most outlen steps */
	std::vector<uint64_t> mp, xl;
	const uint64_t outlen = lengths(start, end, id, t, raw, mp, xl);
	uint64_t most = raw;
	for (size_t k = 0; k < nm; k++) {
		CHECK(xl[k] <= 40 + REPL_MAX_INSERTS * raw);                  /* the cap holds whatever ioff says */
		most += xl[k];
	}
	CHECK(outlen <= most);
	uint64_t steps = 0;
	for (uint64_t q = 0; q < outlen; steps++) {
		const ReplAt s = at_of(mp, xl, start, end, id, t, q, outlen, raw);
		check_in_range(s, nm, raw, text, t);
		CHECK(s.run <= outlen - q);
		q += s.run;
	}
	CHECK(steps <= outlen);
	/* ... and with an xlen that disagrees with the lengths pass in one place */
	if (nm != 0) {
		xl[rnd() % nm] = any();
		steps = 0;
		for (uint64_t q = 0; q < outlen && steps <= outlen; steps++) {
			const ReplAt s = at_of(mp, xl, start, end, id, t, q, outlen, raw);
			check_in_range(s, nm, raw, text, t);
			q += s.run < outlen - q ? s.run : outlen - q;
		}
		CHECK(steps <= outlen);
	}
}

int main()
{
	CHECK(REPL_MAX_INSERTS == 255);
	for (int round = 0; round < 3000; round++) well_formed(round);
	for (int round = 0; round < 4000; round++) ill_formed(round);
	/* the cases by hand: "<&>" and "&&" on the match cd of abcdef; the identity (an empty R, one insert at 0) */
	{
		const uint8_t text[] = "abcdef";
		const uint64_t start[] = {2}, end[] = {4}, mpos[] = {2};
		const uint32_t id[] = {0};
		const uint64_t roff[] = {0, 2}, ioff[] = {0, 1}, ins[] = {1}, xlen[] = {4};                  /* R = "<>", a_0 = 1 */
		const uint32_t from[] = {REPL_FROM_TEXT, REPL_FROM_TEXT, REPL_FROM_TABLE, REPL_FROM_TEXT, REPL_FROM_TEXT, REPL_FROM_TABLE, REPL_FROM_TEXT, REPL_FROM_TEXT};
		const uint64_t at[] = {0, 1, 0, 2, 3, 1, 4, 5}, run[] = {2, 1, 1, 2, 1, 1, 2, 1};
		for (uint64_t q = 0; q < 8; q++) {
			const ReplAt s = repl_at(mpos, xlen, start, end, id, (uint64_t)1, roff, ioff, ins, (uint64_t)1, (uint64_t)2, (uint64_t)1, q, (uint64_t)8, (uint64_t)6);
			CHECK(s.from == from[q] && s.at == at[q] && s.run == run[q]);
		}
		const uint64_t roff2[] = {0, 0}, ioff2[] = {0, 2}, ins2[] = {0, 0}, xlen2[] = {4};            /* "&&": cdcd */
		const uint64_t at2[] = {0, 1, 2, 3, 2, 3, 4, 5}, run2[] = {2, 1, 2, 1, 2, 1, 2, 1};
		for (uint64_t q = 0; q < 8; q++) {
			const ReplAt s = repl_at(mpos, xlen2, start, end, id, (uint64_t)1, roff2, ioff2, ins2, (uint64_t)1, (uint64_t)0, (uint64_t)2, q, (uint64_t)8, (uint64_t)6);
			CHECK(s.from == REPL_FROM_TEXT && s.at == at2[q] && s.run == run2[q] && text[s.at] == "abcdcdef"[q]);
		}
		const uint64_t ioff3[] = {0, 1}, xlen3[] = {2};                                             /* "&": the identity */
		for (uint64_t q = 0; q < 6; q++) {
			const ReplAt s = repl_at(mpos, xlen3, start, end, id, (uint64_t)1, roff2, ioff3, ins2, (uint64_t)1, (uint64_t)0, (uint64_t)1, q, (uint64_t)6, (uint64_t)6);
			CHECK(s.from == REPL_FROM_TEXT && s.at == q);
		}
	}
	std::printf("test_replace_tmpl: ok\n");
	return 0;
}
