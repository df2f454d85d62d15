/*
 * image.cpp -- a Plan's device image and first-use tables, built on the host (see image.h).
 */
#include "image.h"

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <map>

namespace fsmhip {

namespace {

template <class T>
void view(Image &im, const std::vector<T> &v)
{
	im.tab = v.data();
	im.tab_size = v.size() * sizeof(T);
	im.tab_elem = (uint32_t)sizeof(T);
}

/* COMB: comb[n], dflt[256] */
void assemble_comb(const Plan &p, std::vector<uint32_t> &img)
{
	img = p.comb;
	img.resize(p.comb.size() + 256, 0);
	for (uint32_t c = 0; c < p.C; c++) img[p.comb.size() + c] = p.comb_dflt[c];
}

/* COMBSELF: comb64[n] = {entry, smask(next)}, dsm[32] (mask of each class's default state), rng16[n] (self-loop byte range by
 * row offset) -- these three parts go to LDS (the returned byte count) -- then smask[n] by row offset (global only: seeds a walk) */
uint32_t assemble_combself(const Plan &p, std::vector<uint32_t> &img)
{
	const size_t n = p.comb.size(), rw = (n + 1) / 2;   /* rng16[n] in u32 words */
	img.assign(2 * n + 64 + rw + n, 0);
	for (size_t k = 0; k < n; k++) {
		img[2 * k] = p.comb[k];
		const uint32_t nxt = p.comb[k] & 0xffffu;
		img[2 * k + 1] = (p.comb[k] >> 16) != 0xFFFFu && nxt < n ? p.comb_smask[nxt] : 0u;
	}
	for (uint32_t c = 0; c < p.C; c++) {
		img[2 * n + 2 * c] = p.comb_dflt[c];
		img[2 * n + 2 * c + 1] = p.comb_smask[p.comb_dflt[c]];
	}
	for (size_t k = 0; k < n; k++) img[2 * n + 64 + k / 2] |= (uint32_t)p.comb_rng[k] << (16 * (k & 1));
	for (size_t k = 0; k < n; k++) img[2 * n + 64 + rw + k] = p.comb_smask[k];
	return (uint32_t)((2 * n + 64 + rw) * 4);
}

/* eager masks and the wide sets' runs, re-laid in fin-index order (= renumbered state except where the code is a row offset) */
void build_eager(const Plan &p, Image &im)
{
	const size_t F = im.fin->size();
	std::vector<uint32_t> state_of(F, 0xFFFFFFFFu);   /* fin index -> renumbered state */
	im.emask.assign(F, 0);
	for (uint32_t n = 0; n < p.S1; n++) {
		im.emask[im.fin_index(n)] = p.emask[n];
		state_of[im.fin_index(n)] = n;
	}
	im.s.eager_words = p.eager_words;
	if (p.eager_words <= 1) return;
	im.ew_off.assign(F + 1, 0);
	for (size_t i = 0; i < F; i++) {
		im.ew_off[i] = (uint32_t)im.ew_word.size();
		const uint32_t n = state_of[i];
		if (n == 0xFFFFFFFFu) continue;
		im.ew_word.insert(im.ew_word.end(), p.ew_word.begin() + p.ew_off[n], p.ew_word.begin() + p.ew_off[n + 1]);
		im.ew_mask.insert(im.ew_mask.end(), p.ew_mask.begin() + p.ew_off[n], p.ew_mask.begin() + p.ew_off[n + 1]);
	}
	im.ew_off[F] = (uint32_t)im.ew_word.size();
	if (im.ew_word.empty()) { im.ew_word.push_back(0); im.ew_mask.push_back(0); }
}

} // namespace

int build_image(const Plan &p, Image &im)
{
	im = Image();
	ImageScalars &s = im.s;
	/* what differs per layout: the table, the fin vector, whether the kernel reads the byte table, and the code of state n --
	 * n * unit, or codes[n] where rows lie at offsets of their own */
	uint32_t unit = 1;
	const std::vector<uint32_t> *codes = nullptr;
	bool classes = true;
	/* the comb forms place rows region by region (plan.cpp build_comb): the absorbing and the eager thresholds are row offsets
	 * the planner chose; elsewhere codes ascend with the state */
	bool placed = false;
	uint32_t placed_lo = 0, placed_hi = 0;
	im.fin = &p.fin;
	switch (p.layout) {
	case FSM_HIP_LAYOUT_TINY:
		classes = false;
		if (!p.tiny5_col.empty()) {   /* <= 6 states: Tiny5Pol, code = 5 * state */
			view(im, p.tiny5_col);
			unit = 5;
		} else {
			/* 7..16 states: 64-bit columns; a 32-bit format for <= 8 states measured slower on the same box
			 * (4.95-5.06 vs 5.10-5.61 TB/s, profiles/r01_tiny_by_states.txt) and was dropped */
			view(im, p.tiny_col);
		}
		s.tab_bytes = 256u * im.tab_elem;
		break;
	case FSM_HIP_LAYOUT_LDS:
	case FSM_HIP_LAYOUT_LDSSELF:
		view(im, p.lds_tab);
		unit = p.row_bytes;
		s.tab_bytes = (uint32_t)im.tab_size;
		break;
	case FSM_HIP_LAYOUT_LDS2:
		view(im, p.lds_tab);
		unit = p.lds2_c1 * p.lds2_c1;      /* entries per state */
		s.tab_bytes = (uint32_t)im.tab_size;
		s.dflt = p.lds2_c1;
		break;
	case FSM_HIP_LAYOUT_COMB:
	case FSM_HIP_LAYOUT_COMBSELF:
		if (p.layout == FSM_HIP_LAYOUT_COMB) {
			assemble_comb(p, im.own);
			s.tab_bytes = (uint32_t)(im.own.size() * 4);
		} else {
			s.tab_bytes = assemble_combself(p, im.own);
			s.dflt = (uint32_t)p.comb.size();   /* entries: tells the kernel where dsm[] and rng16[] start */
		}
		view(im, im.own);
		im.fin = &p.comb_fin;
		codes = &p.comb_off;
		placed = true;
		s.abs_min = p.comb_abs_min_off;
		placed_lo = p.comb_eager_lo_off;
		placed_hi = p.comb_eager_hi_off;
		break;
	case FSM_HIP_LAYOUT_COMB256:
		classes = false;
		view(im, p.comb256);
		im.fin = &p.comb256_fin;
		codes = &p.comb256_off;
		s.tab_bytes = (uint32_t)im.tab_size;
		placed = true;
		s.abs_min = p.comb256_abs_min_off;
		placed_lo = p.comb256_eager_lo_off;
		placed_hi = p.comb256_eager_hi_off;
		s.dflt = p.comb256_dflt;
		break;
	case FSM_HIP_LAYOUT_GLOBAL:
		if (!p.glob_tab16.empty()) {
			/* <= 65 535 states: 2-byte entries = the next state's row (Glob16Pol), rows in visit-frequency order where
			 * the planner ranked them: fin follows */
			view(im, p.glob_tab16);
			im.fin = &p.glob16_fin;
			if (!p.glob16_rank.empty()) codes = &p.glob16_rank;
			s.dflt = p.C * 2u;          /* bytes per row */
			im.glob16 = true;
		} else {
			view(im, p.glob_tab);
			unit = p.C * 4u;            /* the row's byte offset */
		}
		im.glob_row_bytes = p.C * im.tab_elem;
		im.glob_tab_bytes = im.tab_size;
		break;
	case FSM_HIP_LAYOUT_SPARSE:
		classes = false;
		view(im, p.sparse_img);
		s.tab_bytes = p.sparse_lds_bytes;
		break;
	default:
		return EINVAL;
	}
	im.btab.assign(256, 0);
	if (classes) for (int b = 0; b < 256; b++) im.btab[b] = p.cls[b];
	im.enc.resize(p.S1);
	for (uint32_t n = 0; n < p.S1; n++) im.enc[n] = codes != nullptr ? (*codes)[n] : n * unit;
	s.start = im.enc[p.start];
	s.fin_div = codes != nullptr ? 1u : unit;
	if (!placed) s.abs_min = p.abs_min * unit;
	/* fin_index(): code / fin_div as a multiply where that is exact for every code the walk can produce */
	if (s.fin_div > 1u) {
		const uint32_t maxcode = *std::max_element(im.enc.begin(), im.enc.end());
		if ((uint64_t)maxcode * s.fin_div < ((uint64_t)1 << 32)) s.fin_mul = (uint32_t)((((uint64_t)1 << 32) / s.fin_div) + 1u);
	}
	/* the spare class of the self-loop-mask layouts (plan.cpp sets bit 31 in every mask when there are <= 31 classes) */
	if ((p.layout == FSM_HIP_LAYOUT_COMBSELF || p.layout == FSM_HIP_LAYOUT_LDSSELF) && p.C <= 31u) s.ident_class = 31u;
	if (p.emask.empty()) return 0;
	build_eager(p, im);
	/* a state emits iff code < eager_lo_end || code >= eager_hi_begin */
	if (placed) {
		s.eager_lo_end = placed_lo;
		s.eager_hi_begin = placed_hi;
	} else {
		s.eager_lo_end = p.eager_lo_end < p.S1 ? im.enc[p.eager_lo_end] : 0xFFFFFFFFu;
		s.eager_hi_begin = p.eager_hi_begin < p.S1 ? im.enc[p.eager_hi_begin] : 0xFFFFFFFFu;
	}
	return 0;
}

void Image::drop_upload_parts()
{
	if (!own.empty()) tab = nullptr;
	std::vector<uint32_t>().swap(own);
	std::vector<uint32_t>().swap(btab);
	std::vector<uint64_t>().swap(emask);
	std::vector<uint32_t>().swap(ew_off);
	std::vector<uint32_t>().swap(ew_word);
	std::vector<uint64_t>().swap(ew_mask);
}

/* ---- end ids ---- */

namespace {

typedef std::vector<uint32_t> IdSet;

IdSet ids_of(const Plan &p, uint32_t s) { return IdSet(p.endids.begin() + p.endid_off[s], p.endids.begin() + p.endid_off[s + 1]); }

/* the de-duplicated id sets of the end states in build_retlist()'s order (src/libfsm/vm/retlist.c:93-138) */
struct RetSets {
	std::vector<uint32_t> off, ids;
	std::map<IdSet, uint32_t> index;
	explicit RetSets(const Plan &p)
	{
		std::vector<IdSet> sets;
		/* end states = those appearing in fin */
		std::vector<uint8_t> is_end(p.nstates, 0);
		for (uint32_t v : p.fin) if (v != FSM_HIP_NO_MATCH) is_end[v] = 1;
		for (uint32_t s = 0; s < p.nstates; s++) if (is_end[s]) sets.push_back(ids_of(p, s));
		/* cmp_ret (src/libfsm/vm/retlist.c:63-79): by count, then memcmp over the raw id array -- byte-wise,
		 * i.e. NOT numeric for ids >= 256 on a little-endian host ({256} sorts before {1}) */
		std::sort(sets.begin(), sets.end(), [](const IdSet &a, const IdSet &b) {
			if (a.size() != b.size()) return a.size() < b.size();
			return !a.empty() && memcmp(a.data(), b.data(), a.size() * sizeof(uint32_t)) < 0;
		});
		sets.erase(std::unique(sets.begin(), sets.end()), sets.end());
		off.assign(1, 0);
		for (uint32_t k = 0; k < sets.size(); k++) {
			index[sets[k]] = k;
			ids.insert(ids.end(), sets[k].begin(), sets[k].end());
			off.push_back((uint32_t)ids.size());
		}
	}
};

/* rs: the sets whose index a state gets (mode RET), or null: its lowest id (AMBIG_EARLIEST, src/libfsm/print/c.c:67-85) */
void by_state(const Plan &p, const RetSets *rs, std::vector<uint32_t> &out, uint32_t *conflict)
{
	out.assign(p.S1, FSM_HIP_NO_MATCH);
	uint32_t cf = FSM_HIP_NO_MATCH;
	for (uint32_t n = 0; n < p.S1; n++) {
		const uint32_t s = p.fin[n];
		if (s == FSM_HIP_NO_MATCH) continue;
		const uint32_t a = p.endid_off[s], b = p.endid_off[s + 1];
		if (b - a > 1 && s < cf) cf = s;
		out[n] = rs != nullptr ? rs->index.at(ids_of(p, s)) : (b > a ? p.endids[a] : FSM_HIP_NO_ID);
	}
	if (conflict) *conflict = cf;
}

void by_fin_index(const Image &img, const std::vector<uint32_t> &by, std::vector<uint32_t> &out)
{
	out.assign(img.fin->size(), FSM_HIP_NO_MATCH);
	for (uint32_t n = 0; n < by.size(); n++) out[img.fin_index(n)] = by[n];
}

} // namespace

void ids_by_state(const Plan &p, int mode, std::vector<uint32_t> &out, uint32_t *conflict)
{
	if (mode == FSM_HIP_IDS_RET) {
		const RetSets rs(p);
		by_state(p, &rs, out, conflict);
	} else by_state(p, nullptr, out, conflict);
}

int build_tok_image(const Plan &p, int ids_mode, TokImage &im)
{
	im = TokImage();
	const uint64_t entries = (uint64_t)p.S1 * p.C;
	if (entries == 0 || p.S1 > 0x7fffffffu || entries > 0xffffffffu) return EINVAL;
	if (ids_mode != FSM_HIP_IDS_EARLIEST && ids_mode != FSM_HIP_IDS_RET && ids_mode != FSM_HIP_IDS_ERROR) return EINVAL;
	std::vector<uint32_t> by;
	uint32_t conflict = FSM_HIP_NO_MATCH;
	ids_by_state(p, ids_mode == FSM_HIP_IDS_RET ? FSM_HIP_IDS_RET : FSM_HIP_IDS_EARLIEST, by, &conflict);
	if (ids_mode == FSM_HIP_IDS_ERROR && conflict != FSM_HIP_NO_MATCH) return EINVAL;
	im.in_lds = entries <= TOK_LDS_ENTRIES;
	im.entries = (uint32_t)entries;
	im.C = p.C;
	auto is_end = [&](uint32_t n) { return p.fin[n] != FSM_HIP_NO_MATCH ? 1u : 0u; };
	im.col.resize(256);
	if (im.in_lds) {
		const uint32_t unit = p.C * 2u;          /* a row's bytes: (S1 - 1) * unit < 2^15, bit 0 is free */
		im.tab16.resize(entries);
		for (uint64_t e = 0; e < entries; e++) im.tab16[e] = (uint16_t)(p.dense[e] * unit | is_end(p.dense[e]));
		for (uint32_t b = 0; b < 256u; b++) im.col[b] = (uint16_t)(p.cls[b] * 2u);
		im.start = p.start * unit | is_end(p.start);
		im.ids.assign(entries, FSM_HIP_NO_MATCH);
	} else {
		im.tab32.resize(entries);
		for (uint64_t e = 0; e < entries; e++) im.tab32[e] = p.dense[e] | is_end(p.dense[e]) << 31;
		for (uint32_t b = 0; b < 256u; b++) im.col[b] = p.cls[b];
		im.start = p.start | is_end(p.start) << 31;
		im.ids.assign(p.S1, FSM_HIP_NO_MATCH);
	}
	im.abs_min = im.code_of(p.abs_min);
	im.dead = im.code_of(p.S1 - 1u);
	for (uint32_t n = 0; n < p.S1; n++) im.ids[im.id_index(im.code_of(n))] = by[n];
	return 0;
}

void build_id_tables(const Plan &p, const Image &img, IdTables &t)
{
	RetSets rs(p);
	std::vector<uint32_t> by;
	by_state(p, nullptr, by, &t.conflict);
	by_fin_index(img, by, t.earliest);
	by_state(p, &rs, by, nullptr);
	by_fin_index(img, by, t.ret);
	t.ret_off.swap(rs.off);
	t.ret_ids.swap(rs.ids);
}

/* ---- resume ---- */

void build_resume_tables(const Plan &p, const Image &img, ResumeTables &t)
{
	t.enc_of.resize(p.nstates + 1);
	for (uint32_t o = 0; o <= p.nstates; o++) t.enc_of[o] = img.enc[p.old2new[o]];
	t.orig_of.assign(img.fin->size(), FSM_HIP_STATE_DEAD);
	for (uint32_t n = 0; n + 1 < p.S1; n++) t.orig_of[img.fin_index(n)] = p.new2old[n];
}

/* ---- trace ---- */

void pack_cls4(const uint8_t cls[256], uint32_t out[64])
{
	for (unsigned w = 0; w < 64; w++)
		out[w] = (uint32_t)cls[4 * w] | ((uint32_t)cls[4 * w + 1] << 8) | ((uint32_t)cls[4 * w + 2] << 16) | ((uint32_t)cls[4 * w + 3] << 24);
}

void build_trace_tables(const Plan &p, TraceTables &t)
{
	/* id lists per renumbered state, ascending (fsm_eager_output_get order: eager_output.c:317-329) */
	t.eoff.assign(p.S1 + 1, 0);
	t.eids.clear();
	for (uint32_t n = 0; n < p.S1; n++) {
		if (!p.emask.empty() && p.emask[n] != 0) {
			if (p.eager_words <= 1) {
				for (unsigned b = 0; b < 64; b++) if (p.emask[n] >> b & 1u) t.eids.push_back(p.eager_ids[b]);
			} else {
				const size_t first = t.eids.size();
				for (uint32_t k = p.ew_off[n]; k < p.ew_off[n + 1]; k++)
					for (unsigned b = 0; b < 64; b++) if (p.ew_mask[k] >> b & 1u) t.eids.push_back(p.eager_ids[(size_t)p.ew_word[k] * 64u + b]);
				std::sort(t.eids.begin() + (ptrdiff_t)first, t.eids.end());
			}
		}
		t.eoff[n + 1] = (uint32_t)t.eids.size();
	}
	t.cls4.resize(64);
	pack_cls4(p.cls, t.cls4.data());
}

} // namespace fsmhip
