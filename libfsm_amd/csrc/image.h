/*
 * image.h -- from a Plan to the words a walk kernel reads: the layout's device image and the tables made on first use
 * (end ids, resume, trace).  Host code only, no HIP header: fsm_hip.hip uploads what this builds and makes the decisions that
 * need the device; tests/c/test_image.cpp checks every member against the Plan on the CPU.
 *
 * An encoded state ("code") is what a kernel keeps for a renumbered state: the state itself, a multiple of it (row offset in
 * bytes or entries), or a row offset / row rank from a vector of the Plan.  The per-state tables (fin, eager masks, orig_of,
 * end ids) are indexed by code / fin_div.
 */
#ifndef FSMHIP_CSRC_IMAGE_H
#define FSMHIP_CSRC_IMAGE_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "plan.h"

#pragma GCC visibility push(hidden)   /* not part of the C ABI */

namespace fsmhip {

/* what fsm_hip.hip copies into its WalkArgs prototype (walk_kernels.h has each member's meaning) */
struct ImageScalars {
	uint32_t tab_bytes = 0;      /* the part of the table a kernel mirrors in LDS (GLOBAL: set by the device's side, the hot head) */
	uint32_t start = 0, abs_min = 0;
	uint32_t fin_div = 1, fin_mul = 0;
	uint32_t dflt = 0;
	uint32_t ident_class = 0xFFFFFFFFu;
	uint32_t eager_lo_end = 0, eager_hi_begin = 0, eager_words = 0;   /* all 0 without eager outputs */
};

struct Image {
	/* the table to upload: the Plan's own vector wherever the image IS that vector (never copied: a global table can be
	 * hundreds of megabytes); `own` holds it for COMB and COMBSELF, which are assembled */
	const void *tab = nullptr;
	size_t tab_size = 0;         /* bytes */
	uint32_t tab_elem = 4;       /* bytes per entry */
	std::vector<uint32_t> own;
	const std::vector<uint32_t> *fin = nullptr;   /* the Plan's fin vector this layout indexes */
	std::vector<uint32_t> btab;  /* [256] byte -> class (all 0 where the layout has no byte table) */
	std::vector<uint32_t> enc;   /* [S1] renumbered state -> code */
	ImageScalars s;
	/* eager outputs by fin index (empty without): masks; wide sets' (word, mask) runs, state i's at [ew_off[i], ew_off[i + 1]) */
	std::vector<uint64_t> emask;
	std::vector<uint32_t> ew_off, ew_word;
	std::vector<uint64_t> ew_mask;
	/* GLOBAL layout */
	bool glob16 = false;         /* 2-byte entries (<= 65 535 states) */
	uint32_t glob_row_bytes = 4;
	uint64_t glob_tab_bytes = 0;

	size_t fin_index(uint32_t n) const { return enc[n] / s.fin_div; }
	/* the parts only an upload reads go once it is done; enc, fin, the scalars and the sizes stay */
	void drop_upload_parts();
};

/* 0, or EINVAL for a Plan without a known layout.  `out` points into `p`: the Plan outlives it and does not move. */
int build_image(const Plan &p, Image &out);

/* what fsm_hip_exec_batch_ids (mode FSM_HIP_IDS_EARLIEST or _RET) writes for an input ending in renumbered state n; *conflict
 * (optional): the lowest caller's end state that carries more than one id, or FSM_HIP_NO_MATCH */
void ids_by_state(const Plan &p, int mode, std::vector<uint32_t> &out, uint32_t *conflict);

/* the tokeniser's image (tok.hip, walk_tok): the table in the two forms of the accept-position walk -- up to TOK_LDS_ENTRIES
 * (state, class) entries a u16 row offset in bytes with "the target is an end state" in bit 0, walked from LDS; otherwise the
 * u32 index of the target with that bit in bit 31, walked from device memory -- and one u32 id per state, read once per token.
 * A state as the walk carries it ("code") is an entry of the table; id_index() is where its id lies in `ids`: the row's first
 * entry in the LDS form (code >> 1, no division on the device; the other entries of `ids` hold FSM_HIP_NO_MATCH), the state
 * itself otherwise. */
constexpr uint32_t TOK_LDS_ENTRIES = 16384;
struct TokImage {
	bool in_lds = false;
	uint32_t entries = 0, C = 0;
	uint32_t start = 0;          /* code, its end bit folded in */
	uint32_t abs_min = 0;        /* code (no end bit): states from here up are absorbing */
	uint32_t dead = 0;           /* code of DEAD, the last state */
	std::vector<uint16_t> tab16; /* [entries], LDS form */
	std::vector<uint32_t> tab32; /* [entries], global form */
	std::vector<uint16_t> col;   /* [256]: LDS form 2 * class (the byte offset of the byte's column), else the class */
	std::vector<uint32_t> ids;   /* what a token accepted in a state gets, by id_index() */
	uint32_t code_of(uint32_t n) const { return in_lds ? n * C * 2u : n; }
	uint32_t id_index(uint32_t code) const { return in_lds ? code >> 1 : code & 0x7fffffffu; }
};
/* 0; EINVAL for an empty or oversized table, an unknown ids_mode, and for FSM_HIP_IDS_ERROR on an automaton with an end state
 * of more than one id (a conflict-free one is built as FSM_HIP_IDS_EARLIEST) */
int build_tok_image(const Plan &p, int ids_mode, TokImage &out);

struct IdTables {
	std::vector<uint32_t> earliest, ret;     /* by fin index: ids_by_state() carried through enc / fin_div */
	std::vector<uint32_t> ret_off, ret_ids;  /* the de-duplicated id sets (CSR), ordered by count, then memcmp */
	uint32_t conflict = FSM_HIP_NO_MATCH;
};
void build_id_tables(const Plan &p, const Image &img, IdTables &out);

/* resume: caller's state id (nstates = DEAD) -> code; fin index -> caller's id, FSM_HIP_STATE_DEAD for DEAD and for no state */
struct ResumeTables { std::vector<uint32_t> enc_of, orig_of; };
void build_resume_tables(const Plan &p, const Image &img, ResumeTables &out);

/* byte -> class, four to a word: byte b is bits 8 (b & 3) .. of word b >> 2 */
void pack_cls4(const uint8_t cls[256], uint32_t out[64]);

/* the emission stream: per renumbered state its eager ids ascending (CSR), and the packed classes */
struct TraceTables { std::vector<uint32_t> eoff, eids, cls4; };
void build_trace_tables(const Plan &p, TraceTables &out);

} // namespace fsmhip

#pragma GCC visibility pop

#endif
