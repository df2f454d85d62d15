/*
 * test_image.cpp -- libfsm_amd/csrc/image.cpp against the Plan members tests/test_plan.py ties to the reference: the step from
 * a Plan to the words a kernel reads, on the CPU.  Links plan.cpp and image.cpp and nothing of HIP.  Built with
 * -fsanitize=address,undefined by tests/test_image.py; exit status 0 = every check held and every form was seen.
 *
 * The automata are the affine family of tests/global_ref.py restated: dense[s][c] = (s * a_c + 1 + 37 c) mod S over K
 * contiguous byte classes, every a_c odd and coprime to S.
 */
#include "../../libfsm_amd/csrc/image.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <set>
#include <string>

using namespace fsmhip;

namespace {

int failures = 0;
std::string where;
#define CHECK(cond) do { if (!(cond)) { if (failures++ < 40) fprintf(stderr, "%s:%d: %s: CHECK(%s) failed\n", __FILE__, __LINE__, where.c_str(), #cond); } } while (0)
/* inside a loop over states: say which one, once, and leave the loop */
#define CHECK_AT(cond, n) if (!(cond)) { if (failures++ < 40) fprintf(stderr, "%s:%d: %s: state %u: CHECK(%s) failed\n", __FILE__, __LINE__, where.c_str(), (unsigned)(n), #cond); break; }

const uint32_t NO = FSM_HIP_NO_MATCH;

struct Automaton {
	uint32_t S = 0, K = 0;
	std::vector<uint32_t> edge_off, endid_off, endids, eager_off, eager_ids;
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
		if (!eager_off.empty()) { d.eager_off = eager_off.data(); d.eager_ids = eager_ids.data(); }
		return d;
	}
};

/* global_ref.affine(S, K, holes, sinks, endids, eager, every) */
Automaton affine(uint32_t S, uint32_t K, uint32_t holes, uint32_t sinks, bool endids, uint32_t eager, uint32_t every = 11)
{
	Automaton A;
	A.S = S; A.K = K;
	std::vector<uint64_t> mult;
	for (uint64_t a = 3; a < 200 && mult.size() < 8; a += 2) if (std::gcd(a, (uint64_t)S) == 1) mult.push_back(a);
	A.is_end.resize(S);
	A.edge_off.assign(1, 0);
	if (endids) A.endid_off.assign(1, 0);
	if (eager) A.eager_off.assign(1, 0);
	for (uint64_t s = 0; s < S; s++) {
		const bool sink = s >= S - sinks;
		A.is_end[s] = s % 7 == 3 || sink;
		for (uint64_t c = 0; c < K; c++) {
			if (!sink && holes && s % holes == 0 && c == K - 1) continue;      /* DEAD is one step of the last class away */
			fsm_hip_range r;
			r.lo = (uint8_t)(256 * c / K);
			r.hi = (uint8_t)(256 * (c + 1) / K - 1);
			r.reserved = 0;
			r.to = sink ? (uint32_t)s : (uint32_t)((s * mult[c % mult.size()] + 1 + 37 * c) % S);
			A.ranges.push_back(r);
		}
		A.edge_off.push_back((uint32_t)A.ranges.size());
		if (endids) {   /* 1 to 3 per end state, ascending, some >= 256, few distinct sets */
			const uint32_t q = (uint32_t)s / 7, ids[3] = { q % 5, 300 + q % 3, 1000 + q % 2 };
			if (A.is_end[s]) A.endids.insert(A.endids.end(), ids, ids + 1 + q % 3);
			A.endid_off.push_back((uint32_t)A.endids.size());
		}
		if (eager) {    /* every `every`-th state emits one or two; the id of index k is 5 + 3 k */
			if (s % every == 0) {
				const uint32_t q = (uint32_t)s / every, k1 = q % eager, k2 = (q * 7 + 3) % eager;
				if (q % 2 == 1 && k2 != k1) {
					A.eager_ids.push_back(5 + 3 * std::min(k1, k2));
					A.eager_ids.push_back(5 + 3 * std::max(k1, k2));
				} else A.eager_ids.push_back(5 + 3 * k1);
			}
			A.eager_off.push_back((uint32_t)A.eager_ids.size());
		}
	}
	return A;
}

/* what has been checked at least once */
struct Seen {
	bool layout[10] = {};
	bool tiny5 = false, tiny64 = false, glob16 = false, glob32 = false, eager_reg = false, eager_wide = false;
} seen;

template <class T>
bool is_view_of(const Image &im, const std::vector<T> &v)
{
	return im.tab == v.data() && im.tab_size == v.size() * sizeof(T) && im.tab_elem == sizeof(T) && im.own.empty();
}

void check_assembled(const Plan &p, const Image &im)
{
	const uint32_t *img = static_cast<const uint32_t *>(im.tab);
	const size_t n = p.comb.size();
	switch (p.layout) {
	case FSM_HIP_LAYOUT_COMB:
		CHECK(im.tab == im.own.data() && im.tab_size == (n + 256) * 4 && im.tab_elem == 4);
		CHECK(im.s.tab_bytes == im.tab_size);
		for (size_t k = 0; k < n; k++) CHECK_AT(img[k] == p.comb[k], k);
		for (uint32_t c = 0; c < 256; c++) CHECK_AT(img[n + c] == (c < p.C ? p.comb_dflt[c] : 0u), c);
		break;
	case FSM_HIP_LAYOUT_COMBSELF: {
		const size_t rw = (n + 1) / 2;
		CHECK(im.tab == im.own.data() && im.tab_elem == 4);
		CHECK(im.s.tab_bytes == (2 * n + 64 + rw) * 4);            /* comb64 | dsm | rng16: the LDS part */
		CHECK(im.tab_size == im.s.tab_bytes + n * 4);              /* ... then smask */
		CHECK(im.s.dflt == n);
		CHECK(p.C <= 32);
		for (size_t k = 0; k < n; k++) {
			const uint32_t owner = p.comb[k] >> 16, next = p.comb[k] & 0xffffu;
			CHECK_AT(img[2 * k] == p.comb[k], k);
			CHECK_AT(img[2 * k + 1] == (owner == 0xFFFFu || next >= n ? 0u : p.comb_smask[next]), k);
			CHECK_AT(((img[2 * n + 64 + k / 2] >> (16 * (k & 1))) & 0xffffu) == p.comb_rng[k], k);
			CHECK_AT(img[2 * n + 64 + rw + k] == p.comb_smask[k], k);
		}
		for (uint32_t c = 0; c < 32; c++) {
			CHECK_AT(img[2 * n + 2 * c] == (c < p.C ? p.comb_dflt[c] : 0u), c);
			CHECK_AT(img[2 * n + 2 * c + 1] == (c < p.C ? p.comb_smask[p.comb_dflt[c]] : 0u), c);
		}
		if (n % 2 == 1) CHECK((img[2 * n + 64 + rw - 1] >> 16) == 0);
		break;
	}
	case FSM_HIP_LAYOUT_TINY:
		if (!p.tiny5_col.empty()) { CHECK(is_view_of(im, p.tiny5_col)); seen.tiny5 = true; }
		else { CHECK(is_view_of(im, p.tiny_col)); seen.tiny64 = true; }
		CHECK(im.s.tab_bytes == im.tab_size);
		break;
	case FSM_HIP_LAYOUT_LDS:
	case FSM_HIP_LAYOUT_LDSSELF:
	case FSM_HIP_LAYOUT_LDS2:
		CHECK(is_view_of(im, p.lds_tab));
		CHECK(im.s.tab_bytes == im.tab_size);
		break;
	case FSM_HIP_LAYOUT_COMB256:
		CHECK(is_view_of(im, p.comb256));
		CHECK(im.s.tab_bytes == im.tab_size);
		break;
	case FSM_HIP_LAYOUT_SPARSE:
		CHECK(is_view_of(im, p.sparse_img));
		CHECK(im.s.tab_bytes == p.sparse_lds_bytes);
		break;
	case FSM_HIP_LAYOUT_GLOBAL:
		if (!p.glob_tab16.empty()) { CHECK(is_view_of(im, p.glob_tab16)); CHECK(im.glob16 && im.glob_row_bytes == p.C * 2); seen.glob16 = true; }
		else { CHECK(is_view_of(im, p.glob_tab)); CHECK(!im.glob16 && im.glob_row_bytes == p.C * 4); seen.glob32 = true; }
		CHECK(im.glob_tab_bytes == im.tab_size);
		break;
	default:
		CHECK(!"a layout this test knows");
	}
}

void check_pair(const Automaton &A, const Plan &p)
{
	Image im;
	CHECK(build_image(p, im) == 0);
	if (im.fin == nullptr) return;
	const ImageScalars &s = im.s;
	const size_t F = im.fin->size();
	const uint32_t S1 = p.S1;
	check_assembled(p, im);
	/* 1. encoding */
	CHECK(im.enc.size() == S1 && s.fin_div != 0);
	CHECK(std::set<uint32_t>(im.enc.begin(), im.enc.end()).size() == S1);
	CHECK(im.enc[p.start] == s.start);
	for (uint32_t n = 0; n < S1; n++) CHECK_AT((im.enc[n] >= s.abs_min) == (n >= p.abs_min), n);
	/* 2. fin */
	std::vector<uint8_t> mapped(F, 0);
	for (uint32_t n = 0; n < S1; n++) {
		CHECK_AT(im.enc[n] / s.fin_div < F, n);
		CHECK_AT(im.fin_index(n) == im.enc[n] / s.fin_div, n);
		CHECK_AT((*im.fin)[im.enc[n] / s.fin_div] == p.fin[n], n);
		mapped[im.enc[n] / s.fin_div] = 1;
	}
	for (size_t i = 0; i < F; i++) CHECK_AT(mapped[i] || (*im.fin)[i] == NO, i);
	/* 3. fin_mul */
	const uint64_t maxenc = *std::max_element(im.enc.begin(), im.enc.end());
	if (s.fin_mul != 0) {
		for (uint32_t n = 0; n < S1; n++) CHECK_AT((((uint64_t)im.enc[n] * s.fin_mul) >> 32) == im.enc[n] / s.fin_div, n);
	} else CHECK(s.fin_div == 1 || maxenc * s.fin_div >= ((uint64_t)1 << 32));
	/* the byte table and the spare class */
	CHECK(im.btab.size() == 256);
	const bool classes = p.layout != FSM_HIP_LAYOUT_TINY && p.layout != FSM_HIP_LAYOUT_COMB256 && p.layout != FSM_HIP_LAYOUT_SPARSE;
	for (unsigned b = 0; b < 256 && im.btab.size() == 256; b++) CHECK_AT(im.btab[b] == (classes ? p.cls[b] : 0u), b);
	CHECK(s.ident_class == ((p.layout == FSM_HIP_LAYOUT_COMBSELF || p.layout == FSM_HIP_LAYOUT_LDSSELF) && p.C <= 31 ? 31u : 0xFFFFFFFFu));
	/* 4. eager masks and thresholds */
	if (p.emask.empty()) {
		CHECK(im.emask.empty() && im.ew_off.empty() && s.eager_words == 0);
	} else {
		CHECK(im.emask.size() == F && s.eager_words == p.eager_words);
		for (uint32_t n = 0; n < S1 && im.emask.size() == F; n++) {
			CHECK_AT(im.emask[im.enc[n] / s.fin_div] == p.emask[n], n);
			/* (DEAD, the last state, lies beyond eager_hi_begin as in Plan's own numbering, with an empty mask: OR-ing it is harmless) */
			if (n + 1 < S1) { CHECK_AT((p.emask[n] != 0) == (im.enc[n] < s.eager_lo_end || im.enc[n] >= s.eager_hi_begin), n); }
			else CHECK_AT(p.emask[n] == 0, n);
		}
		for (size_t i = 0; i < F && im.emask.size() == F; i++) CHECK_AT(mapped[i] || im.emask[i] == 0, i);
		(p.eager_words > 1 ? seen.eager_wide : seen.eager_reg) = true;
	}
	/* 5. wide sets */
	if (p.eager_words > 1) {
		CHECK(im.ew_off.size() == F + 1 && im.ew_word.size() == im.ew_mask.size());
		bool ok = im.ew_off.size() == F + 1 && std::is_sorted(im.ew_off.begin(), im.ew_off.end());
		CHECK(ok);
		/* (an automaton none of whose states emits keeps one zero pair, so that nothing uploaded is empty) */
		if (ok) CHECK(im.ew_off[F] == im.ew_word.size() || (im.ew_off[F] == 0 && im.ew_word.size() == 1 && im.ew_mask[0] == 0));
		for (uint32_t n = 0; n < S1 && ok; n++) {
			const size_t i = im.enc[n] / s.fin_div, len = p.ew_off[n + 1] - p.ew_off[n];
			CHECK_AT(im.ew_off[i + 1] - im.ew_off[i] == len && im.ew_off[i + 1] <= im.ew_word.size(), n);
			CHECK_AT(std::equal(p.ew_word.begin() + p.ew_off[n], p.ew_word.begin() + p.ew_off[n + 1], im.ew_word.begin() + im.ew_off[i]), n);
			CHECK_AT(std::equal(p.ew_mask.begin() + p.ew_off[n], p.ew_mask.begin() + p.ew_off[n + 1], im.ew_mask.begin() + im.ew_off[i]), n);
		}
	} else CHECK(im.ew_off.empty() && im.ew_word.empty() && im.ew_mask.empty());
	/* 7. resume */
	ResumeTables rt;
	build_resume_tables(p, im, rt);
	CHECK(rt.enc_of.size() == p.nstates + 1 && rt.orig_of.size() == F);
	for (uint32_t o = 0; o <= p.nstates && rt.enc_of.size() == p.nstates + 1; o++) CHECK_AT(rt.enc_of[o] == im.enc[p.old2new[o]], o);
	if (rt.orig_of.size() == F) {
		std::vector<uint32_t> want(F, FSM_HIP_STATE_DEAD);
		for (uint32_t n = 0; n + 1 < S1; n++) want[im.enc[n] / s.fin_div] = p.new2old[n];
		CHECK(rt.orig_of == want);
		CHECK(rt.orig_of[im.enc[S1 - 1] / s.fin_div] == FSM_HIP_STATE_DEAD);
	}
	/* 8. end ids */
	IdTables it;
	build_id_tables(p, im, it);
	std::vector<uint32_t> by_e, by_r;
	uint32_t cf_e = 1, cf_r = 1;
	ids_by_state(p, FSM_HIP_IDS_EARLIEST, by_e, &cf_e);
	ids_by_state(p, FSM_HIP_IDS_RET, by_r, &cf_r);
	CHECK(by_e.size() == S1 && by_r.size() == S1 && it.earliest.size() == F && it.ret.size() == F);
	if (by_e.size() == S1 && by_r.size() == S1 && it.earliest.size() == F && it.ret.size() == F) {
		std::vector<uint32_t> we(F, NO), wr(F, NO);
		for (uint32_t n = 0; n < S1; n++) { we[im.enc[n] / s.fin_div] = by_e[n]; wr[im.enc[n] / s.fin_div] = by_r[n]; }
		CHECK(it.earliest == we && it.ret == wr);
	}
	uint32_t conflict = NO;
	const size_t nsets = it.ret_off.empty() ? 0 : it.ret_off.size() - 1;
	CHECK(nsets >= 1 || std::count(p.fin.begin(), p.fin.end(), NO) == (ptrdiff_t)S1);
	CHECK(it.ret_off.empty() || (it.ret_off[0] == 0 && it.ret_off.back() == it.ret_ids.size() && std::is_sorted(it.ret_off.begin(), it.ret_off.end())));
	for (uint32_t n = 0; n < S1 && by_e.size() == S1 && by_r.size() == S1; n++) {
		const uint32_t o = p.fin[n];
		if (o == NO) { CHECK_AT(by_e[n] == NO && by_r[n] == NO, n); continue; }
		/* the state's ids, from the description */
		const uint32_t *ids = A.endid_off.empty() ? nullptr : A.endids.data() + A.endid_off[o];
		const size_t cnt = A.endid_off.empty() ? 0 : A.endid_off[o + 1] - A.endid_off[o];
		if (cnt > 1 && o < conflict) conflict = o;
		CHECK_AT(by_e[n] == (cnt ? ids[0] : FSM_HIP_NO_ID), n);
		CHECK_AT(by_r[n] < nsets, n);
		CHECK_AT(it.ret_off[by_r[n] + 1] - it.ret_off[by_r[n]] == cnt && std::equal(ids, ids + cnt, it.ret_ids.begin() + it.ret_off[by_r[n]]), n);
	}
	CHECK(it.conflict == conflict && cf_e == conflict && cf_r == conflict);
	for (size_t k = 0; k + 1 < nsets; k++) {   /* strictly ascending by count, then memcmp: sorted and distinct */
		const size_t a = it.ret_off[k + 1] - it.ret_off[k], b = it.ret_off[k + 2] - it.ret_off[k + 1];
		CHECK_AT(a < b || (a == b && a != 0 && memcmp(&it.ret_ids[it.ret_off[k]], &it.ret_ids[it.ret_off[k + 1]], a * 4) < 0), k);
	}
	/* 9. trace */
	TraceTables tt;
	build_trace_tables(p, tt);
	CHECK(tt.eoff.size() == S1 + 1 && tt.cls4.size() == 64);
	if (tt.eoff.size() == S1 + 1) {
		CHECK(tt.eoff[0] == 0 && tt.eoff[S1] == tt.eids.size() && std::is_sorted(tt.eoff.begin(), tt.eoff.end()));
		for (uint32_t n = 0; n < S1 && tt.eoff[S1] == tt.eids.size(); n++) {
			const uint32_t o = n + 1 < S1 ? p.new2old[n] : NO;
			const uint32_t *b = tt.eids.data() + tt.eoff[n], *e = tt.eids.data() + tt.eoff[n + 1];
			CHECK_AT(tt.eoff[n] <= tt.eoff[n + 1] && std::adjacent_find(b, e, std::greater_equal<uint32_t>()) == e, n);
			if (o == NO || A.eager_off.empty()) { CHECK_AT(b == e, n); }
			else CHECK_AT((size_t)(e - b) == A.eager_off[o + 1] - A.eager_off[o] && std::equal(b, e, A.eager_ids.begin() + A.eager_off[o]), n);
		}
	}
	for (unsigned b = 0; b < 256 && tt.cls4.size() == 64; b++) CHECK_AT(((tt.cls4[b >> 2] >> ((b & 3) * 8)) & 0xffu) == p.cls[b], b);
	/* what an upload leaves behind: the codes, the fin view, the scalars and the sizes */
	const size_t tab_size = im.tab_size;
	const std::vector<uint32_t> enc = im.enc;
	im.drop_upload_parts();
	CHECK(im.own.empty() && im.btab.empty() && im.emask.empty() && im.ew_off.empty() && im.ew_word.empty() && im.ew_mask.empty());
	CHECK(im.enc == enc && im.fin != nullptr && im.fin->size() == F && im.tab_size == tab_size);
	seen.layout[p.layout] = true;
}

const char *const LAYOUT_NAME[10] = { "auto", "tiny", "lds", "comb", "global", "comb256", "combself", "sparse", "ldsself", "lds2" };

void check_automaton(const char *name, const Automaton &A)
{
	const fsm_hip_dfa_desc d = A.desc();
	unsigned granted = 0;
	for (unsigned layout = 1; layout <= 9; layout++) {
		Plan p;
		where = std::string(name) + " / " + LAYOUT_NAME[layout];
		const int r = build_plan(&d, layout, 160u * 1024u, p);
		if (r == ENOTSUP) continue;
		CHECK(r == 0);
		if (r != 0) continue;
		CHECK(p.layout == layout);
		check_pair(A, p);
		granted |= 1u << layout;
	}
	printf("%s: layouts granted 0x%03x\n", name, granted);
}

} // namespace

int main()
{
	check_automaton("affine(5, 4)", affine(5, 4, 0, 0, false, 0));
	check_automaton("affine(15, 4) holes 16 sinks 3 endids", affine(15, 4, 16, 3, true, 0));   /* all nine flags */
	check_automaton("affine(15, 4) eager 40 / 3 sinks endids", affine(15, 4, 0, 3, true, 40, 3));
	check_automaton("affine(200, 4) eager 40", affine(200, 4, 0, 0, false, 40));
	check_automaton("affine(200, 4) eager 100", affine(200, 4, 0, 0, false, 100));
	check_automaton("affine(1000, 4) eager 100", affine(1000, 4, 0, 0, false, 100));   /* 94 ids: two words (19 emitting states of 200 carry 28) */
	check_automaton("affine(65534, 4)", affine(65534, 4, 0, 0, false, 0));
	check_automaton("affine(65535, 4)", affine(65535, 4, 0, 0, false, 0));
	where = "coverage";
	for (unsigned layout = 1; layout <= 9; layout++) {
		if (!seen.layout[layout]) fprintf(stderr, "layout %s was never granted\n", LAYOUT_NAME[layout]);
		CHECK(seen.layout[layout]);
	}
	CHECK(seen.tiny5);
	CHECK(seen.tiny64);
	CHECK(seen.glob16);
	CHECK(seen.glob32);
	CHECK(seen.eager_reg);
	CHECK(seen.eager_wide);
	if (failures != 0) { fprintf(stderr, "test_image: %d check(s) failed\n", failures); return 1; }
	printf("test_image: ok\n");
	return 0;
}
