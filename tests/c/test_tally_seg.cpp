/*
 * test_tally_seg.cpp -- libfsm_amd/csrc/tally_seg.h on the CPU: the column of an id, the clamp, the group of an input, the
 * 64-ary search of a wavefront against the binary one, and the rule "first of its column in its input" over windows with a
 * carried bitmap, against a brute-force count.  A stand-alone program
 * (tests/test_tally_seg.py builds it with -fsanitize=address,undefined and runs it): it links nothing of HIP.
 *
 * walk() goes through the entries exactly as tally.hip's tally_spans does -- spans of whole granules of inputs, windows of W
 * entries, the inputs of a window's two ends first, every entry's input between them, its group between their positions, the
 * backward look, tally_carry -- with the lanes of a window taken one after the other.  Every array is a heap block of exactly
 * its size, so a read outside off[0 .. m], id[0 .. total) or group_off[0 .. G] and a store outside the tables stop the program.
 */
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libfsm_amd/csrc/tally_seg.h"

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

struct Case {
	std::vector<uint64_t> off;       /* m + 1 */
	std::vector<uint32_t> id;        /* total */
	std::vector<uint64_t> goff;      /* G + 1, or empty: one group */
	uint64_t nrules = 0;
	uint64_t m() const { return off.size() - 1u; }
	uint64_t G() const { return goff.empty() ? 1u : goff.size() - 1u; }
	uint64_t C() const { return nrules + 1u; }
};

struct Tables {
	std::vector<uint64_t> count, lines;
};

/* the definition, entry by entry and input by input */
Tables brute(const Case &k)
{
	const uint64_t total = k.id.size(), C = k.C(), G = k.G();
	Tables t;
	t.count.assign(G * C, 0);
	t.lines.assign(G * C, 0);
	for (uint64_t j = 0; j < k.m(); j++) {
		uint64_t g = TALLY_NONE;
		if (k.goff.empty()) {
			g = 0;
		} else if (j < k.goff[G]) {
			for (uint64_t x = 0; x < G; x++)
				if (k.goff[x] <= j) g = x;
		}
		if (g == TALLY_NONE) continue;
		std::vector<bool> has(C, false);
		const uint64_t a = tally_clamp(k.off[j], total), b = tally_clamp(k.off[j + 1u], total);
		for (uint64_t e = a; e < b; e++) {
			const uint64_t c = k.id[e] < k.nrules ? k.id[e] : k.nrules;
			t.count[g * C + c]++;
			if (!has[c]) t.lines[g * C + c]++;
			has[c] = true;
		}
	}
	return t;
}

/* ext_last_le as a wavefront does it (tally.hip, wave_last_le): TALLY_KARY probes a round, taken one after the other; `rounds`
 * counts them */
uint64_t kary_last_le(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t p, uint32_t *rounds = nullptr)
{
	const uint64_t lo0 = lo, hi0 = hi;
	while (lo < hi) {
		uint32_t c = 0;
		for (uint32_t lane = 0; lane < TALLY_KARY; lane++) {
			const uint64_t at = tally_kary_probe(lo, hi, lane);
			assert(at > lo && at <= hi);
			c += a[at] <= p ? 1u : 0u;
		}
		const uint64_t before = hi - lo;
		tally_kary_narrow(&lo, &hi, c);
		assert(lo >= lo0 && hi <= hi0 && lo <= hi && hi - lo < before);
		if (rounds != nullptr) ++*rounds;
	}
	return lo;
}

/* the kernel's walk: spans of `per` granules of `span` inputs, windows of W entries */
Tables walk(const Case &k, uint64_t span, uint64_t per, uint32_t W)
{
	const uint64_t total = k.id.size(), C = k.C(), G = k.G(), m = k.m();
	const uint64_t *off = k.off.data(), *goff = k.goff.empty() ? nullptr : k.goff.data();
	const uint32_t *id = k.id.data();
	Tables t;
	t.count.assign(G * C, 0);
	t.lines.assign(G * C, 0);
	if (m == 0 || total == 0) return t;
	std::vector<uint32_t> seen(tally_bit_words(C));
	std::vector<uint64_t> win_j(W), cs(W), gs(W);
	std::vector<uint32_t> win_c(W);
	std::vector<char> valid(W), counts(W), first(W);
	for (uint64_t j0 = 0; j0 < m; j0 += per * span) {
		const uint64_t j1 = j0 + per * span < m ? j0 + per * span : m;
		const uint64_t k0 = tally_clamp(off[j0], total);
		uint64_t k1 = tally_clamp(off[j1], total);
		if (k1 < k0) k1 = k0;
		std::fill(seen.begin(), seen.end(), 0u);
		uint64_t carried = TALLY_NONE, jlo = j0, plo = 0;
		for (uint64_t w = k0; w < k1; w += W) {
			const uint64_t wend = w + W < k1 ? w + W : k1;
			const uint32_t n = (uint32_t)(wend - w);
			const uint64_t jf = kary_last_le(off, jlo, j1 - 1u, w), jl = kary_last_le(off, jlo, j1 - 1u, wend - 1u);
			const uint64_t pf = goff != nullptr ? tally_group_pos(goff, jf, plo, G + 1u) : 1u;
			const uint64_t pl = goff != nullptr ? tally_group_pos(goff, jl, plo, G + 1u) : 1u;
			assert(jf >= j0 && jf < j1 && jl >= j0 && jl < j1 && pf <= G + 1u && pl <= G + 1u);
			for (uint32_t x = 0; x < n; x++) {
				const uint64_t e = w + x;
				const uint64_t j = ext_last_le(off, jf, jl, e);
				assert(e < total && j >= j0 && j < j1);
				const uint64_t c = tally_col(id[e], k.nrules);
				const uint64_t pos = pf != pl ? tally_group_pos(goff, j, pf, pl) : pf;
				assert(c < C && pos <= G + 1u);
				valid[x] = tally_pos_counts(pos, G);
				win_j[x] = j;
				win_c[x] = (uint32_t)c;
				cs[x] = c;
				gs[x] = pos - 1u;
				if (valid[x]) {
					assert(gs[x] < G);
					t.count[gs[x] * C + c]++;
				}
			}
			const TallyCarry cy = tally_carry(jf, jl, carried);
			for (uint32_t x = 0; x < n; x++) {
				first[x] = tally_window_first(win_j.data(), win_c.data(), x);
				counts[x] = first[x];
				if (first[x] && win_j[x] == jf && jf != jl)
					counts[x] = !cy.carry_in || (seen[tally_bit_word(win_c[x])] & tally_bit_mask(win_c[x])) == 0u;
			}
			if (cy.clear) std::fill(seen.begin(), seen.end(), 0u);
			for (uint32_t x = 0; x < n; x++) {
				if (first[x] && win_j[x] == jl) {
					uint32_t &word = seen.at(tally_bit_word(win_c[x]));
					counts[x] = (word & tally_bit_mask(win_c[x])) == 0u;
					word |= tally_bit_mask(win_c[x]);
				}
				if (counts[x] && valid[x]) t.lines[gs[x] * C + cs[x]]++;
			}
			carried = jl;
			jlo = jl;
			plo = pl;
		}
	}
	return t;
}

void same(const Case &k, const char *what, int no)
{
	const Tables want = brute(k);
	static const uint32_t WS[] = {1, 2, 3, 4, 7, 64, 256};
	for (uint32_t W : WS) {
		for (uint64_t span : {1u, 3u, 64u}) {
			for (uint64_t per : {1u, 2u}) {
				const Tables got = walk(k, span, per, W);
				if (got.count != want.count || got.lines != want.lines) {
					printf("test_tally_seg: %s %d: W=%u span=%llu per=%llu differs (m=%llu total=%zu G=%llu C=%llu)\n", what, no, W,
					       (unsigned long long)span, (unsigned long long)per, (unsigned long long)k.m(), k.id.size(), (unsigned long long)k.G(),
					       (unsigned long long)k.C());
					exit(1);
				}
			}
		}
	}
}

Case random_case(int no)
{
	Case k;
	const uint64_t m = below(40) + (no % 7 == 0 ? 0 : 1);
	k.nrules = no % 5 == 0 ? 0 : below(no % 3 == 0 ? 70 : 6);
	k.off.push_back(below(3));
	for (uint64_t j = 0; j < m; j++) {
		const uint64_t kind = below(10);
		const uint64_t n = kind < 4 ? 0 : kind < 8 ? below(4) : kind == 8 ? below(30) : below(600);
		k.off.push_back(k.off.back() + n);
	}
	uint64_t total = k.off.back();
	if (no % 11 == 0 && total > 0) total -= below(total / 2u + 1u);      /* entries of off above the total */
	if (no % 13 == 0) total += 3;                                        /* ... and ids that no input owns */
	const uint64_t kinds = below(3);
	for (uint64_t e = 0; e < total; e++) {
		const uint64_t r = below(20);
		uint32_t x = kinds == 0 ? (uint32_t)below(k.nrules + 2u) : kinds == 1 ? (uint32_t)(e % (k.nrules + 1u)) : 0u;
		if (r == 0) x = 0xFFFFFFFFu;
		if (r == 1) x = 0xFFFFFFFEu;
		if (r == 2 && k.nrules > 0) x = (uint32_t)k.nrules - 1u;
		if (r == 3) x = (uint32_t)k.nrules;
		k.id.push_back(x);
	}
	if (no % 4 != 0) {                                                   /* groups: empty ones, a first above 0, a last below m */
		uint64_t at = below(3) == 0 ? below(m / 2u + 1u) : 0;
		k.goff.push_back(at);
		const uint64_t G = 1u + below(12);
		for (uint64_t g = 0; g < G; g++) {
			if (below(3) != 0) at += below(m / 3u + 2u);
			if (at > m) at = m;
			k.goff.push_back(at);
		}
		if (below(2) == 0) k.goff.back() = m;
	}
	return k;
}

void units()
{
	assert(tally_col(0, 0) == 0 && tally_col(5, 5) == 5 && tally_col(4, 5) == 4 && tally_col(0xFFFFFFFFu, 5) == 5);
	assert(tally_col(0xFFFFFFFEu, 0x100000000ull) == 0xFFFFFFFEull);
	assert(tally_clamp(3, 7) == 3 && tally_clamp(7, 7) == 7 && tally_clamp(~0ull, 7) == 7 && tally_clamp(1, 0) == 0);
	const uint64_t g[] = {2, 2, 2, 5, 9};                                /* G = 4: groups 0 and 1 empty, 2 = [2, 5), 3 = [5, 9) */
	assert(tally_group_pos(g, 0, 0, 5) == 0 && tally_group_pos(g, 1, 0, 5) == 0);
	assert(tally_group_pos(g, 2, 0, 5) == 3 && tally_group_pos(g, 4, 0, 5) == 3);    /* the LAST g with group_off[g] <= j */
	assert(tally_group_pos(g, 5, 0, 5) == 4 && tally_group_pos(g, 8, 0, 5) == 4);
	assert(tally_group_pos(g, 9, 0, 5) == 5 && tally_group_pos(g, ~0ull - 1u, 0, 5) == 5);
	assert(tally_group_pos(g, 4, 3, 4) == 3 && tally_group_pos(g, 5, 3, 4) == 4 && tally_group_pos(g, 7, 4, 4) == 4);
	assert(!tally_pos_counts(0, 4) && tally_pos_counts(1, 4) && tally_pos_counts(4, 4) && !tally_pos_counts(5, 4));
	const uint64_t wj[] = {7, 7, 7, 8, 8, 7};
	const uint32_t wc[] = {1, 2, 1, 1, 1, 1};
	assert(tally_window_first(wj, wc, 0) && tally_window_first(wj, wc, 1) && !tally_window_first(wj, wc, 2));
	assert(tally_window_first(wj, wc, 3) && !tally_window_first(wj, wc, 4) && tally_window_first(wj, wc, 5));   /* stops at the other input */
	/* the 64-ary search is the binary one on every ascending array, repeats and all, in at most 1 + log64 rounds */
	for (int no = 0; no < 400; no++) {
		const uint64_t n = 1u + below(no % 10 == 0 ? 70000 : no % 3 == 0 ? 5000 : 200);
		std::vector<uint64_t> a(n);
		uint64_t x = below(5);
		for (uint64_t i = 0; i < n; i++) {
			a[i] = x;
			if (below(3) != 0) x += below(no % 2 == 0 ? 3 : 40);
		}
		for (int q = 0; q < 60; q++) {
			uint64_t lo = below(n), hi = below(n);
			if (q % 4 == 0) { lo = 0; hi = n - 1u; }
			const uint64_t p = q % 7 == 0 ? ~0ull : below(a[n - 1u] + 3u);
			uint32_t rounds = 0;
			assert(kary_last_le(a.data(), lo, hi, p, &rounds) == ext_last_le(a.data(), lo, hi, p));
			assert(rounds <= (n <= 64 ? 1u : n <= 4096 ? 2u : 3u));
		}
	}
	TallyCarry c = tally_carry(3, 3, 3);
	assert(c.carry_in && !c.clear);
	c = tally_carry(3, 4, 3);
	assert(c.carry_in && c.clear);
	c = tally_carry(3, 3, 2);
	assert(!c.carry_in && c.clear);
	c = tally_carry(0, 0, TALLY_NONE);
	assert(!c.carry_in && c.clear);
	assert(tally_bit_words(1) == 1 && tally_bit_words(32) == 1 && tally_bit_words(33) == 2 && tally_bit_words(65536) == 2048);
	assert(tally_bit_word(65535) == 2047 && tally_bit_mask(65535) == 0x80000000u && tally_bit_mask(32) == 1u);
}

/* one long input between short ones: all one column, cycling over the columns, random */
void long_lines()
{
	for (int kind = 0; kind < 3; kind++) {
		Case k;
		k.nrules = 5;
		k.off = {0, 2, 2, 3};
		k.off.push_back(3 + 3000);
		k.off.push_back(k.off.back());
		k.off.push_back(k.off.back() + 1);
		for (uint64_t e = 0; e < k.off.back(); e++) k.id.push_back(kind == 0 ? 2u : kind == 1 ? (uint32_t)(e % 6u) : (uint32_t)below(7));
		same(k, "long", kind);
		k.goff = {0, 3, 3, 4, 6};                                        /* a boundary directly before and behind the long input */
		same(k, "long, groups", kind);
	}
}

/* arrays that do not ascend: whatever comes out, nothing leaves the arrays (the sanitizer and walk()'s asserts look on) */
void broken()
{
	for (int no = 0; no < 300; no++) {
		Case k = random_case(1000 + no);
		for (uint64_t &x : k.off)
			if (below(4) == 0) x = below(2) == 0 ? below(k.id.size() + 5u) : ~0ull - below(3);
		for (uint64_t &x : k.goff)
			if (below(3) == 0) x = below(2) == 0 ? below(k.m() + 3u) : ~0ull - below(3);
		for (uint32_t W : {1u, 4u, 256u}) (void)walk(k, 3, 2, W);
	}
}

}   // namespace

int main()
{
	units();
	for (int no = 0; no < 1500; no++) same(random_case(no), "random", no);
	long_lines();
	broken();
	printf("test_tally_seg: ok\n");
	return 0;
}
