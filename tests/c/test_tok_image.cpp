/*
 * test_tok_image.cpp -- the tokeniser's image (libfsm_amd/csrc/image.cpp build_tok_image) against the Plan, on the CPU: the end
 * bit of every entry, the two forms at the 16 384 / 16 400-entry boundary, the ids under EARLIEST and RET, EINVAL under ERROR on
 * a conflicting automaton.  Links plan.cpp and image.cpp and nothing of HIP.  Built with -fsanitize=address,undefined by
 * tests/test_tokens_abi.py; exit status 0 = every check held.
 *
 * The automata are the affine family of tests/global_ref.py restated: dense[s][c] = (s * a_c + 1 + 37 c) mod S over K
 * contiguous byte classes, every a_c odd and coprime to S.
 */
#include "../../libfsm_amd/csrc/image.h"

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>

using namespace fsmhip;

namespace {

int failures = 0;
std::string where;
#define CHECK(cond) do { if (!(cond)) { if (failures++ < 40) fprintf(stderr, "%s:%d: %s: CHECK(%s) failed\n", __FILE__, __LINE__, where.c_str(), #cond); } } while (0)
#define CHECK_AT(cond, n) if (!(cond)) { if (failures++ < 40) fprintf(stderr, "%s:%d: %s: at %u: CHECK(%s) failed\n", __FILE__, __LINE__, where.c_str(), (unsigned)(n), #cond); break; }

const uint32_t NO = FSM_HIP_NO_MATCH;

struct Automaton {
	uint32_t S = 0, K = 0;
	std::vector<uint32_t> edge_off, endid_off, endids;
	std::vector<fsm_hip_range> ranges;
	std::vector<uint8_t> is_end;
	fsm_hip_dfa_desc desc() const
	{
		fsm_hip_dfa_desc d;
		memset(&d, 0, sizeof d);
		d.nstates = S;
		d.start = 0;
		d.edge_off = edge_off.data();
		d.ranges = ranges.data();
		d.is_end = is_end.data();
		if (!endid_off.empty()) { d.endid_off = endid_off.data(); d.endids = endids.data(); }
		return d;
	}
};

/* global_ref.affine(S, K, holes, sinks); ids: 0 none, 1 one per end state (s % 5), 3 one to three (global_ref.endid_slots) */
Automaton affine(uint32_t S, uint32_t K, uint32_t holes, uint32_t sinks, int ids, bool start_ends = false)
{
	Automaton A;
	A.S = S; A.K = K;
	std::vector<uint64_t> mult;
	for (uint64_t a = 3; a < 200 && mult.size() < 8; a += 2) if (std::gcd(a, (uint64_t)S) == 1) mult.push_back(a);
	A.is_end.resize(S);
	A.edge_off.assign(1, 0);
	if (ids) A.endid_off.assign(1, 0);
	for (uint64_t s = 0; s < S; s++) {
		const bool sink = s >= S - sinks;
		A.is_end[s] = s % 7 == 3 || sink || (start_ends && s == 0);
		for (uint64_t c = 0; c < K; c++) {
			if (!sink && holes && s % holes == 0 && c == K - 1) continue;
			fsm_hip_range r;
			r.lo = (uint8_t)(256 * c / K);
			r.hi = (uint8_t)(256 * (c + 1) / K - 1);
			r.reserved = 0;
			r.to = sink ? (uint32_t)s : (uint32_t)((s * mult[c % mult.size()] + 1 + 37 * c) % S);
			A.ranges.push_back(r);
		}
		A.edge_off.push_back((uint32_t)A.ranges.size());
		if (ids) {
			const uint32_t q = (uint32_t)s / 7, three[3] = { q % 5, 300 + q % 3, 1000 + q % 2 };
			if (A.is_end[s]) A.endids.insert(A.endids.end(), three, three + (ids == 1 ? 1 : 1 + q % 3));
			A.endid_off.push_back((uint32_t)A.endids.size());
		}
	}
	return A;
}

bool seen_lds = false, seen_global = false, seen_conflict = false, seen_no_id = false;

void check(const char *name, const Automaton &A, bool want_lds)
{
	where = name;
	const fsm_hip_dfa_desc d = A.desc();
	Plan p;
	CHECK(build_plan(&d, FSM_HIP_LAYOUT_AUTO, 160u * 1024u, p) == 0);
	if (p.S1 != A.S + 1) { CHECK(p.S1 == A.S + 1); return; }
	const uint64_t entries = (uint64_t)p.S1 * p.C;
	TokImage bad;
	CHECK(build_tok_image(p, 0, bad) == EINVAL && build_tok_image(p, 4, bad) == EINVAL);
	for (int mode : { FSM_HIP_IDS_EARLIEST, FSM_HIP_IDS_RET, FSM_HIP_IDS_ERROR }) {
		where = std::string(name) + " / mode " + std::to_string(mode);
		std::vector<uint32_t> by;
		uint32_t conflict = NO;
		ids_by_state(p, mode == FSM_HIP_IDS_RET ? FSM_HIP_IDS_RET : FSM_HIP_IDS_EARLIEST, by, &conflict);
		TokImage im;
		const int r = build_tok_image(p, mode, im);
		if (mode == FSM_HIP_IDS_ERROR && conflict != NO) {
			CHECK(r == EINVAL);
			seen_conflict = true;
			continue;
		}
		CHECK(r == 0);
		if (r != 0) continue;
		CHECK(im.in_lds == want_lds && im.in_lds == (entries <= 16384u) && im.entries == entries && im.C == p.C);
		CHECK(im.col.size() == 256 && (im.in_lds ? im.tab16.size() == entries && im.tab32.empty() : im.tab32.size() == entries && im.tab16.empty()));
		const uint32_t end_bit = im.in_lds ? 1u : 0x80000000u;
		auto is_end = [&](uint32_t n) { return p.fin[n] != NO; };
		/* every entry: the target's code, and the end bit iff the TARGET is an end state */
		for (uint64_t e = 0; e < entries; e++) {
			const uint32_t v = im.in_lds ? im.tab16[e] : im.tab32[e], to = p.dense[e];
			CHECK_AT((v & ~end_bit) == im.code_of(to) && ((v & end_bit) != 0u) == is_end(to), e);
		}
		for (uint32_t b = 0; b < 256; b++) CHECK_AT(im.col[b] == (im.in_lds ? p.cls[b] * 2u : p.cls[b]), b);
		CHECK((im.start & ~end_bit) == im.code_of(p.start) && ((im.start & end_bit) != 0u) == is_end(p.start));
		CHECK(im.abs_min == im.code_of(p.abs_min) && im.dead == im.code_of(p.S1 - 1u) && !is_end(p.S1 - 1u));
		if (im.in_lds) {
			/* a row offset in bytes, even, below 2^15 + the row: bit 0 is free and the code is the entry's byte address */
			CHECK(im.code_of(p.S1 - 1u) == (p.S1 - 1u) * p.C * 2u && (uint64_t)(p.S1 - 1u) * p.C * 2u < 0x10000u);
			CHECK(im.ids.size() == entries);
		} else CHECK(im.ids.size() == p.S1);
		/* the ids: by id_index(code), what fsm_hip_exec_batch_ids writes for an input ending in that state */
		size_t named = 0;
		for (uint32_t n = 0; n < p.S1; n++) {
			const uint32_t code = im.code_of(n) | (is_end(n) ? end_bit : 0u);
			CHECK_AT(im.id_index(code) < im.ids.size() && im.ids[im.id_index(code)] == by[n], n);
			CHECK_AT(is_end(n) == (by[n] != NO), n);
			if (by[n] == FSM_HIP_NO_ID) seen_no_id = true;
			named++;
		}
		/* ... and nothing else in the table */
		size_t set = 0;
		for (uint32_t v : im.ids) set += v != NO;
		size_t ends = 0;
		for (uint32_t n = 0; n < p.S1; n++) ends += is_end(n);
		CHECK(set == ends && named == p.S1);
		if (mode == FSM_HIP_IDS_EARLIEST) {   /* the lowest id of the description, state by state */
			for (uint32_t n = 0; n + 1 < p.S1; n++) {
				const uint32_t o = p.new2old[n];
				if (!A.is_end[o]) continue;
				const uint32_t want = A.endid_off.empty() || A.endid_off[o] == A.endid_off[o + 1] ? FSM_HIP_NO_ID : A.endids[A.endid_off[o]];
				CHECK_AT(im.ids[im.id_index(im.code_of(n))] == want, n);
			}
		}
		(im.in_lds ? seen_lds : seen_global) = true;
	}
}

} // namespace

int main()
{
	check("affine(15, 4)", affine(15, 4, 0, 0, 0), true);
	check("affine(15, 4) start ends, one id", affine(15, 4, 0, 0, 1, true), true);
	check("affine(200, 4) holes 16 sinks 3 ids", affine(200, 4, 16, 3, 3), true);
	check("affine(1023, 16) holes 8 sinks 4 ids: 16 384 entries", affine(1023, 16, 8, 4, 3), true);
	check("affine(1024, 16) holes 4 ids: 16 400 entries", affine(1024, 16, 4, 0, 3), false);
	check("affine(1024, 16) one id", affine(1024, 16, 4, 0, 1), false);
	where = "coverage";
	CHECK(seen_lds && seen_global && seen_conflict && seen_no_id);
	if (failures != 0) { fprintf(stderr, "test_tok_image: %d check(s) failed\n", failures); return 1; }
	printf("test_tok_image: ok\n");
	return 0;
}
