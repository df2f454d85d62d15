/*
 * test_extract_seg.cpp -- libfsm_amd/csrc/extract_seg.h on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_extract_seg.py builds and runs it).  Random texts of lines of 0-70 bytes behind a few bytes that belong to no line,
 * with matches that are empty, leave their line or have start > end, every kind of rule set and every separator are extracted by
 * brute force, record by record.  The same is then done with the header's pieces as the passes use them: the input of a match by
 * ext_last_le between the inputs of its block's first and last match, ext_clamp_match, ext_kept, ext_record_len; then every output
 * byte by ext_last_le over the records' offsets and ext_at; then every 16-byte chunk walked from record to record as ext_write
 * walks it, with the 16-byte windows that ext_window_ok and ext_chunk_in_text allow read from an exact-size vector, so ASan is
 * the bound check of the window test.  For ILL-FORMED arrays the result is any byte, but every index stays in range and every
 * loop advances.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libfsm_amd/csrc/extract_seg.h"

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

constexpr uint64_t BLOCK = 8;            /* matches of a block of the lengths pass here: small, so that blocks end inside lines */
constexpr uint64_t OUT_BLOCK = 64;       /* output bytes of a block of the write pass here: whole chunks */

struct Case {
	std::vector<uint8_t> text;           /* exactly `limit` bytes */
	std::vector<uint64_t> loff;          /* m + 1 line offsets */
	std::vector<uint64_t> moff;          /* m + 1 */
	std::vector<uint64_t> start, end;
	std::vector<uint32_t> id;
	std::vector<uint32_t> bits;
	bool has_set = false, keep_other = false;
	uint64_t nrules = 0;
	int sep = -1;
};

struct Packed {
	std::vector<uint64_t> off, src, line, match;
	std::vector<uint8_t> bytes;
};

static void clip(const Case &c, uint64_t j, uint64_t *beg, uint64_t *raw)
{
	const uint64_t limit = c.text.size(), o0 = c.loff[j], o1 = c.loff[j + 1];
	uint64_t l = o1 > o0 ? o1 - o0 : 0;
	if (o0 > limit) l = 0;
	else if (l > limit - o0) l = limit - o0;
	*beg = o0;
	*raw = l;
}

/* the definition, record by record */
static Packed brute(const Case &c)
{
	Packed w;
	w.off.push_back(0);
	const uint64_t m = c.moff.size() - 1;
	for (uint64_t j = 0; j < m; j++) {
		uint64_t beg, raw;
		clip(c, j, &beg, &raw);
		for (uint64_t k = c.moff[j]; k < c.moff[j + 1]; k++) {
			bool keep = true;
			if (c.has_set) keep = c.id[k] < c.nrules ? (c.bits[c.id[k] / 32] >> (c.id[k] % 32) & 1u) != 0 : c.keep_other;
			if (!keep) continue;
			const uint64_t en = c.end[k] < raw ? c.end[k] : raw, st = c.start[k] < en ? c.start[k] : en;
			for (uint64_t i = st; i < en; i++) w.bytes.push_back(c.text[beg + i]);
			if (c.sep >= 0) w.bytes.push_back((uint8_t)c.sep);
			w.off.push_back(w.bytes.size());
			w.src.push_back(beg + st);
			w.line.push_back(j);
			w.match.push_back(k);
		}
	}
	return w;
}

/* the lengths and the offsets pass by the header's pieces */
static Packed by_passes(const Case &c)
{
	Packed g;
	const uint64_t m = c.moff.size() - 1, nmatch = c.start.size();
	g.off.push_back(0);
	uint64_t p = 0;
	for (uint64_t k0 = 0; k0 < nmatch; k0 += BLOCK) {
		const uint64_t klast = k0 + BLOCK - 1 < nmatch - 1 ? k0 + BLOCK - 1 : nmatch - 1;
		const uint64_t jlo = ext_last_le(c.moff.data(), (uint64_t)0, m - 1, k0), jhi = ext_last_le(c.moff.data(), (uint64_t)0, m - 1, klast);
		CHECK(jlo <= jhi);
		for (uint64_t k = k0; k <= klast; k++) {
			const uint64_t j = ext_last_le(c.moff.data(), jlo, jhi, k);
			CHECK(j < m && c.moff[j] <= k && k < c.moff[j + 1]);
			uint64_t beg, raw, st = c.start[k], en = c.end[k];
			clip(c, j, &beg, &raw);
			ext_clamp_match(raw, &st, &en);
			CHECK(st <= en && en <= raw);
			if (!ext_kept(c.bits.data(), c.has_set, c.nrules, c.keep_other, c.id[k])) continue;
			p += ext_record_len(st, en, c.sep >= 0);
			g.off.push_back(p);
			g.src.push_back(beg + st);
			g.line.push_back(j);
			g.match.push_back(k);
		}
	}
	return g;
}

/* first[g] as ext_offsets leaves it; entry ngb = R */
static std::vector<uint64_t> firsts(const std::vector<uint64_t> &off)
{
	const uint64_t R = off.size() - 1, total = off[R], ngb = (total + OUT_BLOCK - 1) / OUT_BLOCK;
	std::vector<uint64_t> first(ngb + 1, UINT64_MAX);
	for (uint64_t r = 0; r < R; r++)
		if (off[r + 1] > off[r])
			for (uint64_t g = (off[r] + OUT_BLOCK - 1) / OUT_BLOCK; g < ngb && g * OUT_BLOCK < off[r + 1]; g++) {
				CHECK(first[g] == UINT64_MAX);       /* exactly one record covers a boundary */
				first[g] = r;
			}
	first[ngb] = R;
	for (uint64_t g = 0; g < ngb; g++) CHECK(first[g] != UINT64_MAX);
	return first;
}

static void put(uint8_t *x, uint32_t k, uint8_t b) { x[k] = b; }

/* one chunk as ext_write assembles it; *steps counts the records opened and the search steps are bounded by the search itself */
static void chunk(const std::vector<uint64_t> &off, const std::vector<uint64_t> &src, const std::vector<uint8_t> &text, int sep, uint64_t lo, uint64_t hi,
                  uint64_t p, uint8_t out[16], uint64_t *opened)
{
	const uint64_t total = off.back(), limit = text.size();
	const bool has_sep = sep >= 0;
	uint64_t r = ext_last_le(off.data(), lo, hi, p);
	uint64_t o0 = off[r], o1 = off[r + 1], sr = src[r];
	ExtAt s = ext_at(o0, o1, sr, has_sep, p);
	std::memset(out, 0, 16);
	if (ext_chunk_in_text(s, limit)) {
		std::memcpy(out, text.data() + s.at, 16);
		return;
	}
	uint32_t t = 0;
	bool fresh = true;
	uint64_t rounds = 0;
	while (t < 16u && p + t < total) {
		CHECK(++rounds <= 16);
		const uint64_t pos = p + t;
		if (!fresh) {
			if (pos >= o1 && r < hi) {
				r++;
				(*opened)++;
				o0 = off[r], o1 = off[r + 1], sr = src[r];
				if (o1 <= pos && r < hi) {
					r = ext_last_le(off.data(), r + 1, hi, pos);
					(*opened)++;
					o0 = off[r], o1 = off[r + 1], sr = src[r];
				}
			}
			s = ext_at(o0, o1, sr, has_sep, pos);
		}
		CHECK(s.run >= 1);
		const uint32_t cnt = s.run < 16u - t ? (uint32_t)s.run : 16u - t;
		uint8_t x[16] = {0};
		if (s.from == EXT_FROM_TEXT) {
			if (ext_window_ok(s.at, t, limit)) {
				std::memcpy(x, text.data() + (s.at - t), 16);    /* ASan: the window lies inside the text */
			} else {
				for (uint32_t i = 0; i < cnt; i++)
					if (s.at + i < limit) put(x, t + i, text[s.at + i]);
			}
		} else if (s.from == EXT_FROM_SEP) {
			put(x, t, (uint8_t)sep);
		}
		for (uint32_t i = t; i < t + cnt; i++) out[i] = x[i];
		t += cnt;
		s.at += cnt;
		s.run -= cnt;
		fresh = s.run != 0;
	}
}

/* every output byte, one by one and chunk by chunk */
static void check_bytes(const Case &c, const Packed &w, const Packed &g)
{
	const uint64_t R = g.off.size() - 1, total = g.off[R];
	if (R == 0 || total == 0) return;
	const std::vector<uint64_t> first = firsts(g.off);
	const uint64_t ngb = first.size() - 1;
	for (uint64_t p = 0; p < total; p++) {
		const uint64_t gb = p / OUT_BLOCK, lo = first[gb] < R - 1 ? first[gb] : R - 1, hi = first[gb + 1] < R - 1 ? first[gb + 1] : R - 1;
		const uint64_t r = ext_last_le(g.off.data(), lo, hi, p);
		CHECK(g.off[r] <= p && p < g.off[r + 1]);
		const ExtAt s = ext_at(g.off[r], g.off[r + 1], g.src[r], c.sep >= 0, p);
		CHECK(s.from != EXT_FROM_NONE && s.run >= 1 && p + s.run <= g.off[r + 1]);
		if (s.from == EXT_FROM_TEXT) {
			for (uint64_t i = 0; i < s.run; i++) CHECK(s.at + i < c.text.size() && c.text[s.at + i] == w.bytes[p + i]);
		} else {
			CHECK(c.sep >= 0 && w.bytes[p] == (uint8_t)c.sep && p + 1 == g.off[r + 1]);
		}
	}
	for (uint64_t gb = 0; gb < ngb; gb++) {
		const uint64_t lo = first[gb] < R - 1 ? first[gb] : R - 1, hi = first[gb + 1] < R - 1 ? first[gb + 1] : R - 1;
		for (uint64_t p = gb * OUT_BLOCK; p < (gb + 1) * OUT_BLOCK && p < total; p += 16) {
			uint8_t out[16];
			uint64_t opened = 0;
			chunk(g.off, g.src, c.text, c.sep, lo, hi, p, out, &opened);
			CHECK(opened <= 32);
			for (uint32_t t = 0; t < 16 && p + t < total; t++) CHECK(out[t] == w.bytes[p + t]);
		}
	}
}

static void compare(const Case &c)
{
	const Packed w = brute(c), g = by_passes(c);
	CHECK(w.off == g.off && w.src == g.src && w.line == g.line && w.match == g.match);
	check_bytes(c, w, g);
}

static void rule_set(Case &c, int kind)
{
	c.has_set = kind != 0;
	c.keep_other = kind == 3 || kind == 5;
	c.nrules = kind == 4 || kind == 5 ? 0 : kind == 0 ? 0 : 1 + rnd() % 40;
	c.bits.assign((c.nrules + 31) / 32 + 1, 0);                  /* (+ 1: never an empty vector's null data()) */
	for (uint64_t i = 0; i < c.nrules; i++)
		if (kind != 2 && rnd() % 2) c.bits[i / 32] |= 1u << (i % 32);    /* kind 2: an empty set */
}

static void random_case(int round)
{
	Case c;
	const uint64_t lead = rnd() % 6, m = 1 + rnd() % 12;
	for (uint64_t i = 0; i < lead; i++) c.text.push_back('#');
	c.loff.push_back(lead);
	c.moff.push_back(0);
	for (uint64_t j = 0; j < m; j++) {
		const uint64_t len = round % 7 == 0 ? rnd() % 3 : rnd() % 71;
		for (uint64_t i = 0; i < len; i++) c.text.push_back((uint8_t)('a' + rnd() % 26));
		c.loff.push_back(c.text.size());
		const uint64_t nm = rnd() % 3 == 0 ? 0 : rnd() % 9;       /* inputs without matches share their offset with their successor */
		for (uint64_t k = 0; k < nm; k++) {
			uint64_t st = rnd() % (len + 1), en = st + (rnd() % 3 == 0 ? 0 : rnd() % 24);
			switch (rnd() % 8) {
			case 0: en = len + rnd() % 50; break;                 /* leaves the line */
			case 1: st = len + 1 + rnd() % 50; en = st + rnd() % 5; break;   /* wholly outside */
			case 2: { const uint64_t x = st; st = en + 1; en = x; break; }   /* start > end */
			case 3: en = UINT64_MAX - rnd() % 3; break;
			default: break;
			}
			c.start.push_back(st);
			c.end.push_back(en);
			c.id.push_back(rnd() % 6 == 0 ? (rnd() % 2 ? 0xFFFFFFFEu : 0xFFFFFFFFu) : (uint32_t)(rnd() % 48));
		}
		c.moff.push_back(c.start.size());
	}
	if (round % 5 == 0 && c.text.size() > lead) c.text.resize(c.text.size() - 1 - rnd() % ((c.text.size() - lead + 1) / 2));   /* a limit that cuts the last lines */
	rule_set(c, round % 6);
	const int seps[] = {-1, '\n', 0, 255, (int)(rnd() % 256)};
	for (int sep : seps) {
		c.sep = sep;
		compare(c);
	}
}

/* `before` and `after` empty records around one record of one byte, no separator: the run crosses blocks of the lengths pass and
 * blocks of the write pass; with a separator the same matches give 1-byte and one 2-byte record */
static void empty_runs(uint64_t before, uint64_t after, uint64_t lines)
{
	Case c;
	c.text = {'#', 'q', 'r', 's'};
	c.loff.push_back(1);
	c.moff.push_back(0);
	const uint64_t n = before + after + 1;
	for (uint64_t j = 0; j < lines; j++) {
		const uint64_t ka = n * j / lines, kb = n * (j + 1) / lines;
		c.loff.push_back(before < kb ? 4 : 1);                    /* the line of the one byte holds the text, the others are empty */
		for (uint64_t k = ka; k < kb; k++) {
			c.start.push_back(k == before ? 1 : (k % 4));
			c.end.push_back(k == before ? 2 : (k % 4));
			c.id.push_back(0);
		}
		c.moff.push_back(c.start.size());
	}
	rule_set(c, 0);
	for (int sep : {-1, 10}) {
		c.sep = sep;
		const Packed w = brute(c);
		CHECK(w.off.size() == n + 1 && w.bytes.size() == (sep < 0 ? 1u : n + 1));
		if (sep < 0) CHECK(w.bytes[0] == 'r');
		compare(c);
	}
}

/* arrays that belong to nothing: every index in range, every loop advances */
static void ill_formed(int)
{
	const uint64_t R = 1 + rnd() % 20, limit = rnd() % 40;
	std::vector<uint8_t> text(limit, 'x');
	std::vector<uint64_t> off(R + 1), src(R);
	auto any = [&]() { return rnd() % 3 == 0 ? rnd() : rnd() % 3 == 0 ? UINT64_MAX - rnd() % 20 : rnd() % 60; };
	for (auto &v : off) v = any();
	for (auto &v : src) v = any();
	for (int i = 0; i < 100; i++) {
		const uint64_t lo = rnd() % R, hi = rnd() % R, p = any();
		const uint64_t r = ext_last_le(off.data(), lo, hi, p);
		CHECK(r < R);
		const ExtAt s = ext_at(off[r], off[r + 1], src[r], rnd() % 2 != 0, p);
		CHECK(s.run >= 1);
		if (s.from == EXT_FROM_TEXT) CHECK(s.at >= src[r]);
		if (ext_chunk_in_text(s, limit)) CHECK(s.at + 16 <= limit);
		const uint32_t t = (uint32_t)(rnd() % 16);
		if (ext_window_ok(s.at, t, limit)) CHECK(s.at >= t && s.at - t + 16 <= limit);
		/* the chunk walk over them, its total the last offset: at most sixteen rounds, no read outside the text */
		if (off[R] != 0 && p < off[R] && p % 16 == 0) {
			uint8_t out[16];
			uint64_t opened = 0;
			chunk(off, src, text, rnd() % 2 ? -1 : 7, lo < hi ? lo : hi, lo < hi ? hi : lo, p, out, &opened);
		}
	}
	uint64_t st = any(), en = any();
	const uint64_t raw = any();
	ext_clamp_match(raw, &st, &en);
	CHECK(st <= en && en <= raw);
}

int main()
{
	for (int round = 0; round < 3000; round++) random_case(round);
	empty_runs(150, 149, 1);
	empty_runs(150, 149, 7);
	empty_runs(0, 299, 3);
	empty_runs(299, 0, 3);
	empty_runs(35000, 34999, 5);
	for (int round = 0; round < 3000; round++) ill_formed(round);
	/* the window test at the limit: a window is allowed exactly where its sixteen bytes end at or below the limit */
	for (uint64_t limit : {(uint64_t)0, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)100}) {
		std::vector<uint8_t> text(limit, 'w');
		for (uint64_t at = limit > 15 ? limit - 15 : 0; at <= limit + 1; at++)
			for (uint32_t t = 0; t < 16; t++) {
				const bool ok = ext_window_ok(at, t, limit);
				CHECK(ok == (at >= t && at - t + 16 <= limit));
				if (ok) { uint8_t x[16]; std::memcpy(x, text.data() + (at - t), 16); CHECK(x[15] == 'w'); }
			}
		for (uint64_t at = 0; at <= limit + 1; at++) CHECK(ext_window_below(at, limit) == (at + 16 <= limit));
		CHECK(!ext_window_below(UINT64_MAX - 3, limit) && !ext_window_ok(UINT64_MAX - 3, 2, limit));
	}
	/* both searches over repeated entries: the LAST index at or below p; lo where there is none */
	{
		const uint64_t a[] = {0, 0, 0, 3, 3, 5, 5, 5, 9};
		CHECK(ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)0) == 2 && ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)2) == 2);
		CHECK(ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)3) == 4 && ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)5) == 7);
		CHECK(ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)8) == 7 && ext_last_le(a, (uint64_t)0, (uint64_t)8, (uint64_t)100) == 8);
		CHECK(ext_last_le(a, (uint64_t)3, (uint64_t)8, (uint64_t)1) == 3 && ext_last_le(a, (uint64_t)5, (uint64_t)2, (uint64_t)100) == 5);
		CHECK(ext_last_le(a, (uint64_t)1, (uint64_t)6, (uint64_t)5) == 6);
	}
	std::printf("test_extract_seg: ok\n");
	return 0;
}
