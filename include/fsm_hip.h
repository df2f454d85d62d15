/*
 * fsm_hip.h -- C ABI of libfsm_hip.so: batched DFA execution on MI355X (gfx950).
 *
 * Drop-in boundary for ONE path of katef/libfsm: "walk a finished DFA over
 * input bytes and report accept/reject + the end state".  Every entry point
 * cites the reference interface it replaces (paths relative to the reference
 * tree).  Plain pointers and sizes only; no C++/torch types.
 *
 * Two layers live in the one shared object:
 *
 *   1. core   -- takes a flat DFA description (struct fsm_hip_dfa_desc) and
 *                raw byte buffers.  No dependency on libfsm at all.
 *   2. shim   -- takes libfsm's own `const struct fsm *` and reads it through
 *                libfsm's PUBLIC API only (fsm_countstates, fsm_getstart,
 *                fsm_isend, fsm_walk_edges, fsm_all/fsm_isdfa,
 *                fsm_countcaptures, fsm_eager_output_count, fsm_endid_count/get).
 *                Those symbols are resolved with dlsym(RTLD_DEFAULT) on first
 *                use, i.e. from whichever libfsm the host program already
 *                links, so libfsm_hip.so itself loads without libfsm.
 *
 * Error convention follows the reference: functions returning int give
 * -1 + errno on failure (cf. fsm_exec, src/libfsm/exec.c:106-114), pointer
 * returning functions give NULL + errno (cf. fsm_vm_compile, src/libfsm/vm.c:88-131).
 * There is NO CPU fallback: without a usable HIP device every exec call fails
 * with -1/ENODEV.
 *
 * Threading: the table of a struct fsm_hip_dfa is immutable after creation.  What
 * exec calls do mutate -- the staging arena of the host-pointer fronts, the
 * timing events, the lazily built end-id / resume tables -- sits behind a
 * per-dfa mutex, so several host threads may share one dfa: host-pointer calls
 * on it run one after the other, device-pointer calls only serialise their
 * enqueue (tuning knobs are not locked: set them before sharing).  Distinct dfa
 * objects are fully independent.  A call makes the dfa's device current while
 * it runs and restores the caller's device before it returns; host-pointer
 * fronts run on a private non-blocking stream, never on the NULL stream.
 */
#ifndef FSM_HIP_H
#define FSM_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libfsm's own opaque/public types, forward-declared exactly as the reference
 * does (include/fsm/fsm.h:13, :24, :28; include/fsm/capture.h:21-24). */
struct fsm;
struct fsm_capture;
typedef unsigned int fsm_state_t;   /* include/fsm/fsm.h:24 */
typedef unsigned int fsm_end_id_t;  /* include/fsm/fsm.h:28 */

/* Value written to end_out[i] for a rejected input.  The reference leaves *end
 * untouched on reject (src/libfsm/exec.c:133-138, :153-155); a batch needs a
 * sentinel instead.  fsm_edge.state is 24 bit (src/libfsm/internal.h:48) so
 * no real state id can collide with it. */
#define FSM_HIP_NO_MATCH 0xFFFFFFFFu

/* ------------------------------------------------------------------ */
/* flat DFA description (core layer input)                            */
/* ------------------------------------------------------------------ */

/* One labelled edge group: bytes lo..hi (inclusive) go to state `to`.
 * This is the byte-range form of the reference's struct edge_group
 * {uint64 symbols[4]; fsm_state_t to} (src/adt/edgeset.c:34-41) and of the
 * codegen IR's struct ir_range (src/libfsm/print/ir.h:23-108). */
struct fsm_hip_range {
	uint8_t  lo, hi;
	uint16_t reserved;
	uint32_t to;
};

struct fsm_hip_dfa_desc {
	uint32_t nstates;                    /* fsm_countstates() */
	uint32_t start;                      /* fsm_getstart()    */
	const uint32_t *edge_off;            /* nstates+1 CSR offsets into ranges[] */
	const struct fsm_hip_range *ranges;  /* ranges of one state must not overlap (DFA) */
	const uint8_t  *is_end;              /* nstates; fsm_isend() */
	const uint32_t *endid_off;           /* nstates+1 CSR offsets into endids[], or NULL */
	const uint32_t *endids;              /* sorted unique per state (fsm_endid_get order) */
	/* eager outputs (src/libfsm/eager_output.c): ids emitted whenever the state is entered,
	 * start state included (exec.c:126-144).  NULL = none. */
	const uint32_t *eager_off;           /* nstates+1 CSR offsets into eager_ids[], or NULL */
	const uint32_t *eager_ids;           /* sorted unique per state (fsm_eager_output_get order) */
};

/* flags for fsm_hip_dfa_create / fsm_hip_compile */
enum {
	FSM_HIP_LAYOUT_AUTO   = 0,   /* planner picks by table size            */
	FSM_HIP_LAYOUT_TINY   = 1,   /* <=16 states: column-in-register walk   */
	FSM_HIP_LAYOUT_LDS    = 2,   /* class-compressed dense table in LDS    */
	FSM_HIP_LAYOUT_COMB   = 3,   /* column-default + comb exceptions, LDS  */
	FSM_HIP_LAYOUT_GLOBAL = 4,   /* class-compressed table in HBM/L2       */
	FSM_HIP_LAYOUT_COMB256 = 5,  /* byte-indexed comb, one default state, LDS */
	FSM_HIP_LAYOUT_COMBSELF = 6, /* comb + self-loop mask per state (<= 32 classes) */
	FSM_HIP_LAYOUT_SPARSE = 7,   /* base-row records (failure-link form) in HBM/L2, hottest in LDS */
	FSM_HIP_LAYOUT_LDSSELF = 8,  /* dense table in LDS + self-loop mask per state (<= 32 classes) */
	FSM_HIP_LAYOUT_LDS2   = 9,   /* dense table over PAIRS of byte classes in LDS: one lookup per two input bytes (plain walks) */
	FSM_HIP_LAYOUT_MASK   = 0xf,
	FSM_HIP_NO_EARLY_RETIRE = 0x10, /* stream every byte of every input: never stop a wavefront early on absorbing states, never leave
	                                 * out the rest of an input whose state is absorbing.  Without it a plain walk (end states, bitmap,
	                                 * end-ids) does both, as fsm_exec stops pulling bytes at a missing edge; the eager-output and the
	                                 * resumed walks only retire whole wavefronts (no test yet shows their id sets / carried states equal
	                                 * with the per-input skip on).  The results are the same either way. */
	FSM_HIP_DEFER_UPLOAD  = 0x20    /* plan now, upload the layout's device image at the first call that needs it: a dfa used only
	                                 * through fsm_hip_exec_multi (a new DFA per retest record, src/retest/main.c:1056) never does */
};

struct fsm_hip_dfa;   /* opaque: device-resident transition table + host-side end-id table */

struct fsm_hip_dfa_info {
	uint32_t nstates;        /* as given (without the synthetic dead state) */
	uint32_t nclasses;       /* byte equivalence classes */
	uint32_t layout;         /* FSM_HIP_LAYOUT_* actually chosen */
	uint32_t nabsorbing;     /* states whose every byte loops to itself (+ dead state) */
	uint64_t table_bytes;    /* bytes of the device transition table */
	uint32_t lds_bytes;      /* LDS bytes per workgroup */
	uint32_t waves_per_block;
	uint32_t device;         /* HIP device ordinal the table lives on */
	uint32_t reserved;
};

/* Build the device table from a flat description.  Replaces, for this path,
 * fsm_vm_compile_with_options() (src/libfsm/vm.c:88-131): DFA -> executable
 * form, self-contained after return (the caller may free `desc`, like retest
 * frees the fsm right after fsm_runner_initialize, src/retest/main.c:1056-1058).
 * NULL + errno=EINVAL if desc is not a DFA (overlapping ranges, bad ids),
 * ENODEV without a HIP device, ENOMEM. */
struct fsm_hip_dfa *fsm_hip_dfa_create(const struct fsm_hip_dfa_desc *desc, unsigned flags);

/* cf. fsm_vm_free() include/fsm/vm.h:56 */
void fsm_hip_dfa_free(struct fsm_hip_dfa *dfa);

int fsm_hip_dfa_info(const struct fsm_hip_dfa *dfa, struct fsm_hip_dfa_info *out);

/* Everything a later call on batches of up to n inputs would allocate, now: the tile-base block of the lengths-only front (and
 * the layout's tables, for a dfa created with FSM_HIP_DEFER_UPLOAD).  After it the device-pointer fronts make no allocation
 * for such batches: they can be captured into a HIP graph from the first launch (an allocation that would be needed during a
 * stream capture fails with ENOMEM instead of breaking the capture). */
int fsm_hip_reserve(struct fsm_hip_dfa *dfa, size_t n);

/* ------------------------------------------------------------------ */
/* batched execution (the hot path)                                   */
/* ------------------------------------------------------------------ */

/* Run n independent inputs through the DFA.  Input i is the len[i] bytes at
 * base + i*stride (len == NULL: every input is exactly `stride` bytes).
 * For each input this computes exactly what
 *     fsm_exec(fsm, getc_over(ptr,len), &opaque, &end, NULL)
 * computes (src/libfsm/exec.c:85-167): end_out[i] = end state if it returned 1,
 * FSM_HIP_NO_MATCH if it returned 0.  accept_bitmap (optional, may be NULL)
 * gets bit (i%64) of word (i/64) set iff input i matched; it must hold
 * ceil(n/64) words.  end_out may be NULL if only the bitmap is wanted.
 * Host pointers; data is staged through HBM (PCIe-inclusive).
 * Replaces the per-input loop over fsm_runner_run() in retest/reperf
 * (src/retest/main.c:1114, src/retest/reperf.c:772-784).
 * Returns 0, or -1 + errno.  One input may be up to 2^36 - 1 bytes long (the kernels count its 16-byte
 * chunks in 32 bits); longer ones go through fsm_hip_exec_batch_resume() in pieces. */
int fsm_hip_exec_batch(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);

/* Same, inputs packed back to back: input i is bytes [off[i], off[i+1]) of base. */
int fsm_hip_exec_batch_offsets(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);

/* Same as fsm_hip_exec_batch but every pointer is a DEVICE pointer on the
 * dfa's device and the launch is asynchronous on `hip_stream` (a hipStream_t
 * passed as void *, NULL = default stream).  Nothing crosses PCIe.
 * CONTRACT of every *_device entry point: the metadata is the caller's to get right -- the host fronts check
 * len[i] <= stride and off[i] <= off[i + 1], a device front cannot without a synchronising copy.  d_len[i] <= stride,
 * d_off[] non-decreasing.  The kernels read an input 16 bytes at a time from its own first byte: up to 15 bytes past
 * an input's end are READ (never past the batch's last byte, base + n * stride or base + d_off[n]), and the bytes
 * between inputs (stride > len) must therefore be addressable.  Bad metadata is undefined behaviour, not EINVAL.
 * HIP GRAPHS: once a dfa is warm (one call of the same front and size class has run: lazily built tables and scratch
 * blocks exist) a *_device call allocates nothing and synchronises nothing, so it can be captured into a HIP graph on
 * the capturing stream and replayed on new bytes / metadata in the same buffers (tests/test_gpu_round4.py; small batches
 * are launch-bound: 13 us per replay against 23 us per launch at 4 096 inputs).  A captured launch keeps the slot of the
 * per-dfa rings (device-side kernel choice, tile counters: 64 slots) it was captured with: replay one graph at a time per
 * dfa, not concurrently with other launches on the same dfa.  fsm_hip_last_kernel_ms is meaningless for replays. */
int fsm_hip_exec_batch_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);

/* Device pointers, packed inputs with a device-resident offsets array. */
int fsm_hip_exec_batch_offsets_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);

/* Every output of one batch from ONE walk (device pointers, asynchronous): end states and / or the accept bitmap (as
 * fsm_hip_exec_batch_device), device-side end-ids (ids_mode = FSM_HIP_IDS_*, d_id_out: as fsm_hip_exec_batch_ids_device) and
 * eager-output sets (d_eager_out: as fsm_hip_exec_batch_eager_device), whichever pointers are not NULL.  Rows with a
 * stride (+ d_len) or packed with d_off (then stride is ignored and d_len must be NULL). */
int fsm_hip_exec_batch_all_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream);

/* Compact metadata for packed inputs (round 4).  The generated matchers of the reference take a line as a (b, e)
 * pointer pair (src/libfsm/print/c.c:569-619) and retest / reperf hand lines over one by one (src/retest/main.c:1114,
 * src/retest/reperf.c:772-784): a batch of them is bytes packed back to back plus, per line, 8 bytes of u64 offsets
 * (above), or
 *   4 bytes: u32 offsets off32[n + 1], for batches below 4 GiB;
 *   4 bytes: the lengths alone, len[n] -- input i is the len[i] bytes after input i - 1.  The offsets are never
 *            materialised: a pre-pass leaves the byte offset of every 64th input (8 bytes per 64 inputs) and the walk
 *            kernels add a wavefront prefix sum of the 64 lengths they read anyway.
 * Results as for fsm_hip_exec_batch (end_out and/or the 1-bit-per-input accept_bitmap, either may be NULL).  The host
 * forms check their metadata (off32 non-decreasing); the device forms follow the *_device contract above.  A device
 * call of the lengths form uses a per-dfa scratch block that grows (a blocking allocation) the first time a batch
 * needs more than its predecessors. */
int fsm_hip_exec_batch_offsets32(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint32_t *off32, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);
int fsm_hip_exec_batch_offsets32_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint32_t *d_off32, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);
int fsm_hip_exec_batch_lengths(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);
int fsm_hip_exec_batch_lengths_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);

/* Every output of one PACKED batch from one walk, whatever the metadata form: what the generated matchers with ids return
 * (`int fsm_main(const char *b, const char *e, unsigned *id)` and the ids / count form, src/libfsm/print/c.c:569-619) for a
 * batch of (b, e) lines, without widening their offsets first.  meta_form says what `meta` is: u64 offsets [n + 1], u32 offsets
 * [n + 1], or u32 lengths [n].  end_out / accept_bitmap / id_out (ids_mode = FSM_HIP_IDS_*) / eager_out as in
 * fsm_hip_exec_batch_all_device, whichever are not NULL. */
enum { FSM_HIP_META_OFF64 = 0, FSM_HIP_META_OFF32 = 1, FSM_HIP_META_LENGTHS = 2 };
int fsm_hip_exec_batch_packed_all(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, int meta_form, const void *meta, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap, int ids_mode, uint32_t *id_out, uint64_t *eager_out);
int fsm_hip_exec_batch_packed_all_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, int meta_form, const void *d_meta, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream);

/* Time of the most recent *_device launch on this dfa, measured with HIP
 * events recorded on the launch stream around the walk kernel only.
 * Blocks until that launch finished.  Returns milliseconds, or <0 on error. */
double fsm_hip_last_kernel_ms(const struct fsm_hip_dfa *dfa);

/* The walk kernel of the most recent launch on this dfa by its own (demangled) name, as rocprofv3 lists it -- e.g.
 * "fsmhip::walk_ldsdma<fsmhip::CombSelfPol, 128, 2, 768>"; two names separated by " | " when the choice between them was
 * made on the device.  Valid until the next launch on this dfa. */
const char *fsm_hip_last_kernel_name(const struct fsm_hip_dfa *dfa);

/* ------------------------------------------------------------------ */
/* end-ids (host side, by end state)                                  */
/* ------------------------------------------------------------------ */

/* cf. fsm_endid_count() src/libfsm/endids.c:653-684 */
size_t fsm_hip_endid_count(const struct fsm_hip_dfa *dfa, uint32_t end_state);

/* cf. fsm_endid_get() src/libfsm/endids.c:686-755: ids sorted ascending,
 * unique; returns 0 if id_buf_count is too small, 1 otherwise. */
int fsm_hip_endid_get(const struct fsm_hip_dfa *dfa, uint32_t end_state,
	size_t id_buf_count, uint32_t *id_buf);

/* ------------------------------------------------------------------ */
/* libfsm-facing shim                                                 */
/* ------------------------------------------------------------------ */

/* struct fsm * -> device table.  Checks ONCE what fsm_exec checks on every
 * call (fsm_all(fsm, fsm_isdfa) and fsm_getstart, src/libfsm/exec.c:106-114).
 * NULL + errno=EINVAL if not a DFA / no start; errno=ENOTSUP if the fsm uses
 * captures (fsm_countcaptures > 0: per-byte host callbacks); errno=ENOSYS if
 * libfsm's symbols are not present in the process.  Eager outputs are carried
 * into the table and delivered by fsm_hip_exec_batch_eager*(); the plain exec
 * calls ignore them. */
struct fsm_hip_dfa *fsm_hip_compile(const struct fsm *fsm, unsigned flags);

/* Same signature and result as fsm_exec() (include/fsm/fsm.h:560-562):
 * 1 and *end on match, 0 on no match (*end untouched), -1 + errno on error.
 * Drains fsm_getc to EOF (the reference stops pulling at the first missing
 * edge, src/libfsm/exec.c:133-138; the result is the same).  captures must
 * be NULL.  One input = one GPU launch: for plumbing/compat, not speed. */
int fsm_hip_exec(const struct fsm_hip_dfa *dfa,
	int (*fsm_getc)(void *opaque), void *opaque,
	fsm_state_t *end, struct fsm_capture *captures);

/* cf. fsm_vm_match_buffer() src/libfsm/vm.c:218-229: 1 / 0, -1 on error.  (1 MiB and more: the engine below.) */
int fsm_hip_match_buffer(const struct fsm_hip_dfa *dfa, const char *buf, size_t n);

/* cf. fsm_vm_match_file() src/libfsm/vm.c:188-216 (what re(1) -x runs on every file it is given, src/re/main.c:1106-1181):
 * 1 / 0, -1 + errno on error; a read error gives 0 as the reference's does.  A file of up to 256 KiB is one plain call.  A
 * bigger one is read in 32 MiB windows (two pinned buffers: window k + 1 is read while k is walked); a window crosses PCIe
 * once and is walked as 1 KiB pieces AT ONCE, one per lane, each from a guessed state (START), the guesses then corrected
 * from the previous piece's result until none changes -- at that fixed point every piece has started where the sequential
 * walk would have, so the result is exactly fsm_exec's over the whole file (file.hip).  A DFA built from patterns forgets
 * within a piece and the second pass already stands; an automaton that counts pays one pass per piece, the sequential cost.
 * Reading stops once the state can no longer change (DEAD or absorbing), as the VM's STOP does. */
int fsm_hip_match_file(const struct fsm_hip_dfa *dfa, FILE *f);
/* the same engine over memory; *end_state (optional) receives the caller's end state id or FSM_HIP_NO_MATCH */
int fsm_hip_match_buffer_big(const struct fsm_hip_dfa *dfa, const char *buf, size_t n, uint32_t *end_state);
/* The same engine with eager outputs: ONE input walked by the whole device, returning what fsm_hip_match_buffer_big /
 * fsm_hip_match_file return, and eager_out (W = fsm_hip_eager_words(dfa) words, required; the encoding of
 * fsm_hip_exec_batch_eager) is overwritten with the set fsm_exec's callback would have received over the whole input
 * (exec.c:126-151).  The pieces walk through fsm_hip_exec_batch_eager_resume_device, one set per piece kept on the device;
 * guesses start from the start state by its caller's id (a guess must not fire the start state's outputs), and a window's
 * sets are OR-ed into the result only at the fixed point, when every piece has walked from its true in-state (file.hip).
 * A read error gives 0, as fsm_hip_match_file, and leaves eager_out zeroed.  NULL dfa / f / eager_out: -1, EINVAL. */
int fsm_hip_match_buffer_big_eager(const struct fsm_hip_dfa *dfa, const char *buf, size_t n,
	uint32_t *end_state, uint64_t *eager_out);
int fsm_hip_match_file_eager(const struct fsm_hip_dfa *dfa, FILE *f, uint32_t *end_state, uint64_t *eager_out);
/* how the last such call of this process went (the four above): windows walked and passes over them (2 per window where every
 * guess stood after its first correction; 0 / 0: a small input, one plain call) */
void fsm_hip_match_last_passes(unsigned *windows, unsigned *passes);

/* Flatten a struct fsm * into a malloc'd description (free with
 * fsm_hip_desc_free).  Exposed so callers can serialise the table. */
struct fsm_hip_dfa_desc *fsm_hip_flatten(const struct fsm *fsm);
void fsm_hip_desc_free(struct fsm_hip_dfa_desc *desc);

/* On-disk form of a flat description ("FSMHIP01", little-endian, layout in
 * libfsm_amd/csrc/shim.c): write returns 0 / -1; read returns a malloc'd
 * description (fsm_hip_desc_free) or NULL + errno=EINVAL on a bad or truncated
 * file.  Plays the role of the reference's DFAVM save/load
 * (src/libfsm/vm.c:39-71) for this path's executable form. */
int fsm_hip_desc_write(const struct fsm_hip_dfa_desc *desc, FILE *f);
struct fsm_hip_dfa_desc *fsm_hip_desc_read(FILE *f);

/* One more "language" in the shape of fsm_print()'s printers (src/libfsm/print.c:242-416):
 * flatten `fsm` and write its table in the on-disk form.  0, or -1 + errno. */
int fsm_hip_print(FILE *f, const struct fsm *fsm);

/* ------------------------------------------------------------------ */
/* streaming: inputs that arrive in pieces                            */
/* ------------------------------------------------------------------ */

/* The batched form of fsm_vm_match_file()'s chunk carry (struct vm_state kept
 * across 4 KiB fread chunks, src/libfsm/vm.c:188-216, src/libfsm/vm/vm.h:177-181):
 * input i starts from state_io[i] -- FSM_HIP_STATE_START, FSM_HIP_STATE_DEAD
 * (an earlier piece already hit a missing edge), or a state id of the caller's
 * fsm returned by a previous call -- consumes its bytes, and state_io[i]
 * receives the state reached.  end_out / accept_bitmap (optional) say whether
 * that state is an end state, i.e. what fsm_exec would return if the input
 * ended here. */
#define FSM_HIP_STATE_START 0xFFFFFFFDu
#define FSM_HIP_STATE_DEAD  0xFFFFFFFCu

/* 1 if no input byte can move the DFA out of `state` (a caller's state id, FSM_HIP_STATE_START or
 * FSM_HIP_STATE_DEAD) -- the condition under which the reference VM stops reading (STOP success on an
 * absorbing end state, src/libfsm/vm/ir.c:763-766; STOP fail on a missing edge); 0 otherwise;
 * -1 + errno=EINVAL for a bad id.  A streaming caller may stop feeding such an input. */
int fsm_hip_state_is_absorbing(const struct fsm_hip_dfa *dfa, uint32_t state);

int fsm_hip_exec_batch_resume(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *state_io, uint32_t *end_out);

int fsm_hip_exec_batch_resume_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);

/* the same over packed inputs (base + off[n + 1], as fsm_hip_exec_batch_offsets): the form retest / rx lines take
 * (src/retest/main.c:1114) when a line arrives in pieces */
int fsm_hip_exec_batch_resume_offsets(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *state_io, uint32_t *end_out);
int fsm_hip_exec_batch_resume_offsets_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);
/* ... and over the compact forms (meta_form = FSM_HIP_META_OFF64 / _OFF32 / _LENGTHS, as fsm_hip_exec_batch_packed_all): the carry
 * of fsm_vm_match_file (src/libfsm/vm.c:188-216) for batches whose metadata is u32 offsets or lengths alone (round 5) */
int fsm_hip_exec_batch_resume_packed(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, int meta_form, const void *meta, size_t n,
	uint32_t *state_io, uint32_t *end_out);
int fsm_hip_exec_batch_resume_packed_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, int meta_form, const void *d_meta, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream);

/* ------------------------------------------------------------------ */
/* end-ids delivered by the device (no host lookup per input)         */
/* ------------------------------------------------------------------ */

/* What id_out[i] holds, after enum fsm_ambig (include/fsm/options.h:35-43):
 *   FSM_HIP_IDS_EARLIEST  the lowest end-id of the end state (AMBIG_EARLIEST,
 *                         src/libfsm/print/c.c:67-85);
 *   FSM_HIP_IDS_RET       the index of the end state's id SET in the
 *                         de-duplicated, sorted list of sets (AMBIG_MULTIPLE; the
 *                         list is built like build_retlist, src/libfsm/vm/retlist.c:93-138:
 *                         ordered by count, then by memcmp of the id arrays, cmp_ret :63-79 --
 *                         so the index equals the reference's ret index); resolve it
 *                         with fsm_hip_ret_get().
 * Rejected inputs get FSM_HIP_NO_MATCH, accepted inputs whose end state carries
 * no id get FSM_HIP_NO_ID (EARLIEST) or the index of the empty set (RET). */
#define FSM_HIP_NO_ID 0xFFFFFFFEu
enum { FSM_HIP_IDS_EARLIEST = 1, FSM_HIP_IDS_RET = 2, FSM_HIP_IDS_ERROR = 3 };

/* AMBIG_ERROR (include/fsm/options.h:35-43): "emit a single endid", refusing DFAs in which some
 * end state carries more than one -- fsm_print fails with EINVAL there (src/libfsm/print/c.c:67-72)
 * after calling hook.conflict().  FSM_HIP_IDS_ERROR makes fsm_hip_exec_batch_ids*() fail the same
 * way (-1, errno = EINVAL, nothing launched); on a conflict-free DFA it is FSM_HIP_IDS_EARLIEST.
 * fsm_hip_ids_conflict() plays the hook: 1 and *state = the lowest such end state, 0 if none,
 * -1 + errno on error. */
int fsm_hip_ids_conflict(const struct fsm_hip_dfa *dfa, fsm_state_t *state);

int fsm_hip_exec_batch_ids(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	int mode, uint32_t *id_out);

int fsm_hip_exec_batch_ids_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	int mode, uint32_t *d_id_out, void *hip_stream);

/* the same over packed inputs: what a generated rx matcher hands its caller per line -- the id(s) of the pattern(s)
 * that matched (src/libfsm/print/c.c:569-619) -- for a whole file of lines in one launch */
int fsm_hip_exec_batch_ids_offsets(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint64_t *off, size_t n,
	int mode, uint32_t *id_out);
int fsm_hip_exec_batch_ids_offsets_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint64_t *d_off, size_t n,
	int mode, uint32_t *d_id_out, void *hip_stream);

size_t fsm_hip_ret_count(const struct fsm_hip_dfa *dfa);

/* Borrowed pointer to the sorted unique ids of set `ret_index` (valid until
 * fsm_hip_dfa_free).  0 on success, -1 + errno=EINVAL for a bad index. */
int fsm_hip_ret_get(const struct fsm_hip_dfa *dfa, uint32_t ret_index,
	const uint32_t **ids, size_t *count);

/* ------------------------------------------------------------------ */
/* eager outputs                                                      */
/* ------------------------------------------------------------------ */

/* fsm_exec with an eager-output callback installed (fsm_eager_output_set_cb,
 * include/fsm/fsm.h:311-312; exec.c:126-144) calls it with every output id of
 * the start state and of every state entered, also on inputs that finally do
 * not match.  The batch form returns, per input, the SET of ids emitted as a
 * bit set of W = fsm_hip_eager_words(dfa) 64-bit words (W = 1 for up to 64
 * distinct ids): bit k%64 of eager_out[i*W + k/64] <=> id fsm_hip_eager_id(dfa, k)
 * was emitted (ids numbered in ascending order).  eager_out holds n*W words.
 * end_out is as in fsm_hip_exec_batch.
 * The result is a SET: fsm_exec calls the callback once per id per state entered, in stream order, repeats
 * included (exec.c:126-144); these calls keep neither the order nor the multiplicity of the emissions (the
 * reference's own tests compare sets: tests/eager_output/utils.c:227-231).  A caller that needs the callback
 * stream itself uses fsm_hip_exec_batch_eager_trace below. */
int fsm_hip_exec_batch_eager(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *eager_out);

int fsm_hip_exec_batch_eager_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_eager_out, void *hip_stream);

/* the same over packed inputs */
int fsm_hip_exec_batch_eager_offsets(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *end_out, uint64_t *eager_out);
int fsm_hip_exec_batch_eager_offsets_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_eager_out, void *hip_stream);

/* Eager outputs of inputs that arrive in pieces: the resumed walk (fsm_hip_exec_batch_resume) with eager-output sets, after
 * fsm_exec (exec.c:126-151).  Per input i:
 *   - from FSM_HIP_STATE_START, the start state's outputs fire before the first byte;
 *   - from a caller's state id carried over from an earlier piece, that state's outputs do NOT fire again (they fired when
 *     it was entered); from FSM_HIP_STATE_DEAD nothing fires;
 *   - every byte that enters a state fires that state's outputs (a set: re-entering a state adds nothing);
 *   - after a missing edge nothing fires, and the state becomes FSM_HIP_STATE_DEAD.
 * eager_io holds n * W words (W = fsm_hip_eager_words(dfa), the encoding of fsm_hip_exec_batch_eager) and is OR-ed into,
 * never cleared: the caller zeroes it before a stream's first piece.  So: zero eager_io, set state_io = START, feed an input's
 * pieces through successive calls -- after the last one eager_io is the set fsm_exec's callback receives over the
 * concatenated input, state_io its final state and end_out what fsm_exec returns (whatever the cut points, empty pieces
 * included).  Inputs: packed (off != NULL: n + 1 offsets, stride and len ignored; decreasing host offsets: EINVAL) or fixed
 * stride (+ len, may be NULL), as fsm_hip_exec_batch_eager_trace takes them.  end_out optional.  NULL dfa, state_io or
 * eager_io: -1, EINVAL. */
int fsm_hip_exec_batch_eager_resume(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, const uint64_t *off, size_t n,
	uint32_t *state_io, uint32_t *end_out, uint64_t *eager_io);
int fsm_hip_exec_batch_eager_resume_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_eager_io, void *hip_stream);

/* The callback STREAM of fsm_exec (exec.c:120-144, match_eager_outputs_for_state :62-78), order and repeats kept:
 * for input i, count_out[i] = how many times the reference would have called the eager-output callback, and the
 * first min(count_out[i], cap) calls are recorded as ids_out[i*cap + k] = the id passed, pos_out[i*cap + k] = the
 * number of input bytes consumed when it fired (0: the start state's outputs, which fire before the first byte;
 * t + 1: the state entered on byte t).  Nothing fires after a missing edge.  count_out[i] > cap: the stream of
 * input i was cut at cap records -- call again with a larger cap.  Within ONE state's set the ids come in ascending
 * order (fsm_eager_output_get's order, eager_output.c:317-329); the reference's callback order inside one state is
 * the insertion order of its internal table (eager_output.c:264-266), which no public getter exposes.
 * Inputs: packed (off != NULL: n + 1 offsets, stride/len ignored) or stride (+ len, may be NULL).  end_out and
 * pos_out may be NULL.  This is an exact-semantics path over the plain table in device memory (uploaded on first
 * use: nstates * classes * 4 bytes), one input per lane; the set-valued calls above are the fast ones. */
int fsm_hip_exec_batch_eager_trace(const struct fsm_hip_dfa *dfa,
	const unsigned char *base, size_t stride, const uint32_t *len, const uint64_t *off, size_t n, size_t cap,
	uint32_t *end_out, uint32_t *count_out, uint32_t *ids_out, uint32_t *pos_out);
int fsm_hip_exec_batch_eager_trace_device(const struct fsm_hip_dfa *dfa,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n, size_t cap,
	uint32_t *d_end_out, uint32_t *d_count_out, uint32_t *d_ids_out, uint32_t *d_pos_out, void *hip_stream);

size_t fsm_hip_eager_id_count(const struct fsm_hip_dfa *dfa);
size_t fsm_hip_eager_words(const struct fsm_hip_dfa *dfa);   /* ceil(id_count / 64), at least 1 */
uint32_t fsm_hip_eager_id(const struct fsm_hip_dfa *dfa, unsigned bit);

/* ------------------------------------------------------------------ */
/* many-DFA front: K automata x their own lines, ONE submission        */
/* ------------------------------------------------------------------ */

/* retest compiles a DFA per record and runs a handful of lines through it (src/retest/main.c:1056-1058
 * fsm_runner_initialize + fsm_free, :1114 fsm_runner_run; tests/retest/ *.tst: 37 DFAs x ~3 lines): one table upload and
 * one launch per DFA is all overhead.  fsm_hip_exec_multi takes K (dfa, lines, outputs) jobs at once.  Every small job
 * (<= 65 536 lines, <= 1 MiB of text, a plain table <= 1 MiB) rides in ONE host-to-device copy -- descriptors, the
 * automaton's plain next-state table, offsets, lines -- ONE kernel whose workgroups map to (dfa, tile of 64 lines), and
 * ONE copy back; a bigger job goes through its dfa's own walk (fsm_hip_exec_batch_offsets).  A dfa created with
 * FSM_HIP_DEFER_UPLOAD and used only here never uploads a table of its own.
 * Job q: input i is bytes off[i]..off[i+1] of base (as fsm_hip_exec_batch_offsets); end_out (n entries) and
 * accept_bitmap (ceil(n/64) words) are optional and get exactly what fsm_hip_exec_batch_offsets gives.
 * 0 / -1 + errno (EINVAL: NULL dfa, decreasing offsets; ENODEV; ENOMEM).  The dfas may live on several devices. */
struct fsm_hip_multi_batch {
	const unsigned char *base;
	const uint64_t *off;          /* n + 1 */
	size_t n;
	uint32_t *end_out;
	uint64_t *accept_bitmap;
};
int fsm_hip_exec_multi(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch *b, size_t k);
/* the same with DEVICE pointers inside b[] (the array itself is host memory); enqueued on hip_stream, not waited for.
 * Not capturable into a HIP graph (the descriptors ride in a staging block that the next call reuses): fsm_hip_multi_prepare
 * + fsm_hip_multi_launch below are. */
int fsm_hip_exec_multi_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch *b, size_t k, void *hip_stream);
/* ... with end-ids delivered by the device, per job (what the reference's multi-pattern consumers want beside accept / reject:
 * re(1) -z src/re/main.c:1152-1166, the generated matchers' `unsigned *id` src/libfsm/print/c.c:569-619): id_out (n entries,
 * optional) gets what fsm_hip_exec_batch_ids writes under ids_mode -- the lowest id of the end state (FSM_HIP_IDS_EARLIEST),
 * the index of its id set (FSM_HIP_IDS_RET, the dfa's own fsm_hip_ret_* tables), FSM_HIP_NO_ID for an end state without ids,
 * FSM_HIP_NO_MATCH for a rejected input; FSM_HIP_IDS_ERROR refuses the whole submission (EINVAL, nothing launched) when a dfa
 * that is asked for ids has an end state with more than one.  The id tables ride in the same copy as the automata's: a dfa
 * created with FSM_HIP_DEFER_UPLOAD still uploads nothing of its own.  Jobs without id_out cost what they cost above. */
struct fsm_hip_multi_batch_ids {
	const unsigned char *base;
	const uint64_t *off;          /* n + 1 */
	size_t n;
	uint32_t *end_out;
	uint64_t *accept_bitmap;
	uint32_t *id_out;
};
int fsm_hip_exec_multi_ids(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode);
int fsm_hip_exec_multi_ids_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode, void *hip_stream);
/* The device-pointer forms fuse every job whose plain next-state table fits the kernel's LDS copy (16 384 entries), whatever
 * its line count: workgroups of four wavefronts map to (dfa, 256 consecutive lines) and share one copy of that dfa's table --
 * 1 024 small automata x 1e5 lines each are ONE launch (round 5 sent every job above 65 536 lines through its dfa's own walk,
 * one launch each).  A job of few but very long lines is fused too (correct, one lane per line): hand such a job to its dfa's
 * own fronts.  Every dfa of a device-pointer submission is launched on the one hip_stream: they must live on that stream's
 * device (fsm_hip_node_exec_multi shards a submission by DFA over several). */
/* The PREPARED form of a device-pointer submission: descriptors, tile map and the automata's tables go to the device ONCE
 * (fsm_hip_multi_prepare: allocates, copies, waits); fsm_hip_multi_launch is then one kernel launch on hip_stream (plus one
 * per job whose table is too big to fuse) -- no copy, no allocation, no wait, so it can be captured into a HIP graph and
 * replayed on whatever the jobs' buffers hold by then (reperf runs the same matcher over and over, src/retest/reperf.c:772-784;
 * this is that loop for K matchers at once).  All dfas on one device (EINVAL otherwise); they and the buffers named in b[]
 * must outlive the handle; b[] itself is copied.  ids_mode as fsm_hip_exec_multi_ids (ignored when no job has id_out). */
struct fsm_hip_multi_prepared;
int fsm_hip_multi_prepare(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_ids *b, size_t k, int ids_mode,
	struct fsm_hip_multi_prepared **out);
int fsm_hip_multi_launch(const struct fsm_hip_multi_prepared *p, void *hip_stream);
void fsm_hip_multi_prepared_free(struct fsm_hip_multi_prepared *p);
/* ... with eager-output sets per job: what K automata built by fsm_union_repeated_pattern_group (include/fsm/bool.h:55-75; the
 * callback of src/libfsm/exec.c:126-144) otherwise need K fsm_hip_exec_batch_eager_offsets calls for -- the reference's
 * tests/eager_output programs are such a corpus.  eager_out (optional) holds n * fsm_hip_eager_words(dfa[q]) words and receives,
 * word for word, what fsm_hip_exec_batch_eager_offsets(dfa[q], base, off, n, ...) writes (the encoding of fsm_hip_eager_words /
 * fsm_hip_eager_id): the start state's outputs fire on every input, the empty one included; nothing fires after a missing edge;
 * the result is a set, and it is OVERWRITTEN, never OR-ed into (a replayed prepared launch shows nothing of the replay before);
 * a dfa without eager outputs gets all-zero words (W = 1).  end_out / accept_bitmap / id_out are exactly what
 * fsm_hip_exec_multi_ids gives, from the same walk; errors as there.  A submission in which some job has eager_out is still ONE
 * fused launch (the kernel's eager form; jobs without eager_out ride in it and take its plain path), one in which none has is
 * the launch of fsm_hip_exec_multi_ids.  The eager masks ride in the submission's one copy, as the id tables do: a dfa created
 * with FSM_HIP_DEFER_UPLOAD still uploads nothing of its own.  Sets of up to 64 ids are collected in registers; wider ones, up to
 * 16 words (1 024 ids), in the line's own words of eager_out, which the kernel zeroes itself; a job whose automaton has more
 * than 1 024 eager ids goes through its dfa's own walk (fsm_hip_exec_batch_packed_all*), as the jobs too big to fuse do, with
 * eager_out passed through.  The prepared form is launched and freed by fsm_hip_multi_launch / fsm_hip_multi_prepared_free. */
struct fsm_hip_multi_batch_eager {
	const unsigned char *base;
	const uint64_t *off;          /* n + 1 */
	size_t n;
	uint32_t *end_out;            /* optional */
	uint64_t *accept_bitmap;      /* optional */
	uint32_t *id_out;             /* optional, as fsm_hip_multi_batch_ids */
	uint64_t *eager_out;          /* optional: n * fsm_hip_eager_words(dfa[q]) words */
};
int fsm_hip_exec_multi_eager(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode);
int fsm_hip_exec_multi_eager_device(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode, void *hip_stream);
int fsm_hip_multi_prepare_eager(const struct fsm_hip_dfa *const *dfa, const struct fsm_hip_multi_batch_eager *b, size_t k, int ids_mode,
	struct fsm_hip_multi_prepared **out);
/* kernels the last fsm_hip_exec_multi* / fsm_hip_multi_launch call of this process launched (1 when every job was small), and how many jobs rode
 * in the fused one */
unsigned fsm_hip_multi_last_launches(void);
unsigned fsm_hip_multi_last_fused_jobs(void);
/* Which device takes which job when a submission is sharded BY DFA over ndev devices: largest cost first,
 * each to the device with the least work so far (ties: the lower device; equal costs keep their order).  Pure host
 * arithmetic -- every rank of a multi-process run computes the same split.  dev_of[k] receives 0..ndev-1. */
int fsm_hip_multi_assign(const uint64_t *cost, size_t k, int ndev, int *dev_of);

/* ------------------------------------------------------------------ */
/* multi-device front: one table replica per GPU of the node           */
/* ------------------------------------------------------------------ */

/* The path shards by input: inputs are independent and the table is small enough
 * to replicate, so a node handle = one struct fsm_hip_dfa per device, and a batch of n inputs is split into
 * contiguous index shards of whole bitmap words -- shard k = inputs [k*per, min(n, (k+1)*per)) with
 * per = 64 * ceil(ceil(n/64) / ndev) -- each driven by its own host thread on its own device and stream.
 * This is what lets a C host (rx, retest, re(1)) use all 8 GPUs without torch.distributed.
 *
 * devices == NULL or ndev == 0: every device of the node.  The list may repeat a device (several replicas on
 * one GPU: a test rig).  NULL + errno as fsm_hip_dfa_create / fsm_hip_compile. */
struct fsm_hip_node;

struct fsm_hip_node *fsm_hip_node_create(const struct fsm_hip_dfa_desc *desc, unsigned flags, const int *devices, int ndev);
struct fsm_hip_node *fsm_hip_node_compile(const struct fsm *fsm, unsigned flags, const int *devices, int ndev);
void fsm_hip_node_free(struct fsm_hip_node *node);
int fsm_hip_node_ndev(const struct fsm_hip_node *node);
/* the k-th replica (borrowed: end-ids, ret sets, knobs, info are per replica and identical) */
struct fsm_hip_dfa *fsm_hip_node_dfa(struct fsm_hip_node *node, int k);
/* shard k of a batch of n inputs */
void fsm_hip_node_shard(const struct fsm_hip_node *node, size_t n, int k, size_t *first, size_t *count);
/* 1 if the device-resident exchange below runs over RCCL (distinct devices, librccl present), 0 if it is done
 * with peer-to-peer copies */
int fsm_hip_node_uses_rccl(const struct fsm_hip_node *node);
/* The shared object the node front's RCCL entry points were bound from (dlopen + dladdr; "" before the first node that
 * wanted RCCL, or when there is none): a process that has torch's RCCL bundle mapped binds that one, a plain C host
 * /opt/rocm/lib's. */
const char *fsm_hip_node_rccl_path(void);

/* fsm_hip_exec_batch / _offsets over the whole node: same arguments, same results.  Every device stages its
 * own slice from the caller's pages and copies its results straight into the caller's arrays at the shard's
 * offset -- no collective is needed for host-side results. */
int fsm_hip_node_exec_batch(struct fsm_hip_node *node,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);
int fsm_hip_node_exec_batch_offsets(struct fsm_hip_node *node,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);
/* ... and the compact packed forms of fsm_hip_exec_batch_offsets32 / _lengths, sharded the same way (round 5) */
int fsm_hip_node_exec_batch_offsets32(struct fsm_hip_node *node,
	const unsigned char *base, const uint32_t *off32, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);
int fsm_hip_node_exec_batch_lengths(struct fsm_hip_node *node,
	const unsigned char *base, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap);

/* Device-resident shards (inputs generated or loaded on the GPUs): d_base[k] = shard k's rows on device k,
 * uniform `stride`-byte inputs, 16-byte aligned.  d_end_out[k] (optional array, optional entries) receives
 * shard k's end states on device k.  d_bitmap_all[k] (optional) is a buffer of
 * fsm_hip_node_bitmap_words(node, n) words on device k: device k writes its slice at word k * (words / ndev)
 * and ONE in-place ncclAllGather over RCCL/xGMI (the path's only collective) leaves the whole batch's accept
 * bitmap on every device; *match_count (optional, needs d_bitmap_all) = accepted inputs of the whole batch,
 * one ncclAllReduce of a u64.  Returns after every device has finished. */
size_t fsm_hip_node_bitmap_words(const struct fsm_hip_node *node, size_t n);
int fsm_hip_node_exec_batch_device(struct fsm_hip_node *node,
	const void *const *d_base, size_t stride, size_t n,
	uint32_t *const *d_end_out, uint64_t *const *d_bitmap_all, uint64_t *match_count);

/* The general device-resident form: every per-device array is indexed by replica k and lives on device k; unused
 * members are NULL / 0 (memset the struct first).
 *   d_base[k]            shard k's input bytes;
 *   stride, d_len        fixed stride (+ optional lengths, d_len[k] = shard k's) -- or
 *   d_off[k]             shard k's packed offsets, count + 1 of them, relative to d_base[k] (stride ignored);
 *   d_end_out[k]         end states;  d_id_out[k] + ids_mode: end-ids as fsm_hip_exec_batch_ids;
 *   d_eager_out[k]       eager-output sets as fsm_hip_exec_batch_eager;
 *   d_bitmap_all[k]      the whole batch's accept bitmap on every device (all entries non-NULL), exchanged as above;
 *   want_count           also reduce the number of accepted inputs (read by fsm_hip_node_wait).
 * async = 0: returns after every device has finished, *match_count (optional) = accepted inputs.
 * async = 1: returns once the work is enqueued (match_count must be NULL).  The exchange runs on a second stream per
 * device, so the NEXT call's walk overlaps it -- provided that call uses other output buffers: alternate between two
 * sets.  fsm_hip_node_wait() returns when everything enqueued has finished (*match_count, optional: the last call's,
 * if it asked for one).  A failed call returns with nothing of it in flight. */
struct fsm_hip_node_batch {
	const void *const *d_base;
	size_t stride;
	const uint32_t *const *d_len;
	const uint64_t *const *d_off;
	uint32_t *const *d_end_out;
	uint32_t *const *d_id_out;
	int ids_mode;
	uint64_t *const *d_eager_out;
	uint64_t *const *d_bitmap_all;
	int want_count;
};
int fsm_hip_node_exec_device(struct fsm_hip_node *node, const struct fsm_hip_node_batch *batch, size_t n,
	uint64_t *match_count, int async);
int fsm_hip_node_wait(struct fsm_hip_node *node, uint64_t *match_count);

/* fsm_hip_exec_batch_ids / _eager over the whole node (host pointers; results land in the caller's arrays in place) */
int fsm_hip_node_exec_batch_ids(struct fsm_hip_node *node,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n, int mode, uint32_t *id_out);
int fsm_hip_node_exec_batch_eager(struct fsm_hip_node *node,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n, uint32_t *end_out, uint64_t *eager_out);

/* A many-DFA submission sharded BY DFA over the node's devices: nodes[q] holds job q's automaton (every node over the same
 * device list), fsm_hip_multi_assign(cost = text bytes + 64 per line) picks the device, each device runs ONE
 * fsm_hip_exec_multi over its jobs on its replicas (its own host thread), results land in the caller's arrays. */
int fsm_hip_node_exec_multi(struct fsm_hip_node *const *nodes, const struct fsm_hip_multi_batch *b, size_t k);

/* ------------------------------------------------------------------ */
/* text front: one buffer with a delimiter between records             */
/* ------------------------------------------------------------------ */

/* Every front above takes inputs the caller has cut already.  A grep-like caller (re(1) over a file, rx, retest's +/- lines,
 * examples/hipgrep.c) starts from ONE buffer with a delimiter between records.  Lines never contain the delimiter, and every
 * line but possibly the last is followed by exactly one: in an automaton whose delimiter column is the identity, walking
 * [off[i], off[i + 1]) of the UNTOUCHED text -- trailing delimiter included -- ends where walking the line alone ends in the
 * original.  So nothing is squeezed or copied: a delimiter scan on the device leaves the offsets, and the text is a plain
 * packed batch of the twin automaton. */

/* A copy of desc in which `byte` is a self-loop of every state (free with fsm_hip_desc_free).  States, start, end states,
 * end-ids and eager ids are unchanged; a range that contains `byte` is split around it, the ranges of a state come out sorted,
 * neighbours to one target merged.  Applying it twice gives what applying it once gives.  Host arithmetic only: works without
 * a device.  NULL + EINVAL for byte outside 0..255 or a bad desc (no states, bad ids, overlapping ranges). */
struct fsm_hip_dfa_desc *fsm_hip_desc_identity_byte(const struct fsm_hip_dfa_desc *desc, int byte);

/* A line matcher: the fsm_hip_dfa built from fsm_hip_desc_identity_byte(desc, delim), and the delimiter it was built for.
 * flags and errors as fsm_hip_dfa_create (fsm_hip_lines_compile: as fsm_hip_compile).  The inner dfa (borrowed, valid until
 * fsm_hip_lines_dfa_free) is the handle for fsm_hip_endid_get, fsm_hip_ret_get, fsm_hip_eager_id, fsm_hip_dfa_info,
 * fsm_hip_last_kernel_ms and tuning: its state ids, end-ids and eager ids are the original's.  The ordered emission stream
 * (fsm_hip_exec_batch_eager_trace) of the inner dfa sees the delimiter's extra step and is not the original's. */
struct fsm_hip_lines_dfa;
struct fsm_hip_lines_dfa *fsm_hip_lines_dfa_create(const struct fsm_hip_dfa_desc *desc, int delim, unsigned flags);
struct fsm_hip_lines_dfa *fsm_hip_lines_compile(const struct fsm *fsm, int delim, unsigned flags);
const struct fsm_hip_dfa *fsm_hip_lines_dfa_inner(const struct fsm_hip_lines_dfa *ld);
int fsm_hip_lines_dfa_delim(const struct fsm_hip_lines_dfa *ld);
void fsm_hip_lines_dfa_free(struct fsm_hip_lines_dfa *ld);

/* A text: bytes on the device plus the offsets of their lines.  Every delimiter ends a line; bytes after the last delimiter
 * form a last line iff there are any; an empty text has 0 lines; two delimiters in a row enclose an empty line; any byte value
 * may be the delimiter (0: grep -z); a '\r' stays part of its line (the rule of examples/hipgrep.c).
 *   off[0] = 0, off[k] = position of the k-th delimiter + 1, off[n] = nbytes       (n + 1 entries, device memory)
 * fsm_hip_text_open copies host bytes to the current device once and returns when the offsets are there.
 * fsm_hip_text_open_device borrows device bytes (any alignment; they must outlive the text and stay as they are); no byte
 * outside [d_text, d_text + nbytes) is read.  The scan is enqueued on hip_stream, which is synchronised ONCE inside the call
 * (the line count has to reach the host: it sizes the offsets and, later, the caller's outputs); the kernel that fills the
 * offsets is still in flight at return -- work enqueued on hip_stream afterwards sees them, another stream has to wait for
 * hip_stream first.  Not capturable into a HIP graph.  NULL + errno: EINVAL (delim outside 0..255), ENODEV, ENOMEM (a text
 * that does not fit the device: windows are a later step). */
struct fsm_hip_text;
struct fsm_hip_text *fsm_hip_text_open(const void *text, size_t nbytes, int delim);
struct fsm_hip_text *fsm_hip_text_open_device(const void *d_text, size_t nbytes, int delim, void *hip_stream);
size_t fsm_hip_text_lines(const struct fsm_hip_text *t);                      /* n */
const uint64_t *fsm_hip_text_offsets_device(const struct fsm_hip_text *t);   /* n + 1 entries, device memory */
int fsm_hip_text_offsets(const struct fsm_hip_text *t, uint64_t *off);      /* copy the n + 1 entries out (waits for the scan) */
void fsm_hip_text_free(struct fsm_hip_text *t);
/* for tests and probes: bytes one workgroup scans per step; the most workgroups a scan launches on the current device (a
 * longer text gives every workgroup several consecutive blocks); milliseconds of the three scan kernels of this text, from
 * HIP events around them (the host's wait between the second and the third is left out; blocks until the scan has finished) */
size_t fsm_hip_text_block_bytes(void);
size_t fsm_hip_text_max_workgroups(void);
double fsm_hip_text_scan_ms(const struct fsm_hip_text *t);

/* Walk every line of the text: the outputs of fsm_hip_exec_batch_packed_all{,_device} for the n = fsm_hip_text_lines(t) lines
 * WITHOUT their delimiters under the original automaton -- end_out (n), accept_bitmap (ceil(n / 64) words), id_out under
 * ids_mode (FSM_HIP_IDS_*), eager_out (n * fsm_hip_eager_words(inner) words), whichever are not NULL.  The device form is
 * one fsm_hip_exec_batch_packed_all_device(inner, d_text, FSM_HIP_META_OFF64, d_off, n, ...) on hip_stream and nothing else
 * (its contract, HIP graphs included); the host form allocates the outputs on the device, calls it on the text's own stream
 * and copies back.  One text may be walked by any number of line matchers, also from several host threads: the host form's
 * calls on ONE text share that text's stream, so they run one after the other and each returns only when the stream is idle
 * (the answers are each call's own); threads that want to overlap use the device form on streams of their own.  A text
 * without a delimiter is one line of
 * nbytes, walked as a long packed input is.  0, or -1 + errno: EINVAL when ld's delimiter differs from t's or they live on
 * different devices (no output is touched); n == 0 returns 0 and touches no output. */
int fsm_hip_text_exec(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t,
	uint32_t *end_out, uint64_t *accept_bitmap, int ids_mode, uint32_t *id_out, uint64_t *eager_out);
int fsm_hip_text_exec_device(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream);

/* The hits: the lines a bitmap selects -- their numbers, their byte ranges and their bytes, packed, on the device.  What a
 * grep-like caller wants from a text is not n answers but the lines that matched; this is the stream compaction and the
 * ragged gather that deliver them without a host loop over the answers or the offsets.
 *   Selected: line i is selected iff i < n and (bit i of the bitmap) ^ (FSM_HIP_HITS_INVERT given) is set.  The bitmap has
 *     ceil(n / 64) words, bit i = line i (the layout fsm_hip_text_exec_device writes); the bits at and above n of its last word
 *     are ignored whatever they hold: INVERT does not turn them into lines.
 *   lines    m line indices, 0-based, ascending.
 *   bytes    text[off[i], off[i + 1]) of every selected line in that order, verbatim: the trailing delimiter where the line has
 *            one, none added to a last line without.  Every selected line therefore contributes at least one byte.
 *   out_off  m + 1 entries: out_off[k] = bytes before the k-th selected line, out_off[0] = 0, out_off[m] = nbytes.
 *   Under FSM_HIP_HITS_NO_BYTES (grep -c, grep -n without the text) only m and lines are made: nbytes is 0, the offsets and the
 *   bytes are NULL.  n == 0 or m == 0 gives a valid handle with count 0, out_off = {0} and no bytes.
 * fsm_hip_text_hits walks t with ld (accept bitmap only, kept on the device) on the text's own stream, as fsm_hip_text_exec
 * does, and returns when everything is there.  fsm_hip_text_hits_device takes any caller-made bitmap: the work is enqueued on
 * hip_stream after a wait for the text's "offsets are there" event, and hip_stream is synchronised ONCE inside the call (m and
 * the byte total size the arrays: fsm_hip_text_open_device's rule); the kernels that fill the arrays are still in flight at
 * return -- later work on hip_stream sees the arrays, fsm_hip_text_hits_copy and _ms wait for the hits' own event.  Not
 * capturable into a HIP graph.  The bitmap and the text must stay as they are until that event (if they do not, the arrays are
 * wrong, never overrun, and no byte outside the text is read).  The hits must be freed before their text.
 * NULL + errno: EINVAL (t NULL, d_bitmap NULL with n > 0, an unknown flag bit; in the host form ld NULL or its delimiter or
 * device not the text's), ENOMEM, ENODEV (checked first: there is no CPU path). */
#define FSM_HIP_HITS_INVERT   1u   /* select the lines whose bit is 0 (grep -v) */
#define FSM_HIP_HITS_NO_BYTES 2u   /* numbers and count only: no gather, no output offsets */
struct fsm_hip_text_hits;
struct fsm_hip_text_hits *fsm_hip_text_hits(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t, unsigned flags);
struct fsm_hip_text_hits *fsm_hip_text_hits_device(const struct fsm_hip_text *t, const uint64_t *d_bitmap, unsigned flags, void *hip_stream);
size_t fsm_hip_text_hits_count(const struct fsm_hip_text_hits *h);                    /* m */
size_t fsm_hip_text_hits_nbytes(const struct fsm_hip_text_hits *h);                   /* bytes of the m lines; 0 under NO_BYTES */
const uint64_t *fsm_hip_text_hits_lines_device(const struct fsm_hip_text_hits *h);    /* m entries; NULL when m == 0 */
const uint64_t *fsm_hip_text_hits_offsets_device(const struct fsm_hip_text_hits *h);  /* m + 1 entries; NULL under NO_BYTES */
const unsigned char *fsm_hip_text_hits_bytes_device(const struct fsm_hip_text_hits *h);   /* nbytes; NULL when there are none */
/* copy out whichever are not NULL (lines: m, out_off: m + 1, bytes: nbytes); waits for the hits.  -1 + EINVAL: h NULL, or out_off
 * asked of hits made under NO_BYTES */
int fsm_hip_text_hits_copy(const struct fsm_hip_text_hits *h, uint64_t *lines, uint64_t *out_off, void *bytes);
/* milliseconds of the hits' kernels from HIP events around them, the host's wait in the middle left out (as fsm_hip_text_scan_ms;
 * blocks until the hits are there); _gather_ms: the gather kernel's share of it, 0 when there was none */
double fsm_hip_text_hits_ms(const struct fsm_hip_text_hits *h);
double fsm_hip_text_hits_gather_ms(const struct fsm_hip_text_hits *h);
void fsm_hip_text_hits_free(struct fsm_hip_text_hits *h);
/* for tests: lines one workgroup selects per step; output bytes one workgroup gathers per step (the most workgroups of either:
 * fsm_hip_text_max_workgroups) */
size_t fsm_hip_text_hits_block_lines(void);
size_t fsm_hip_text_hits_block_bytes(void);

/* Files of a text: many files back to back in ONE text, lines cut at every file end as well, hits per file.  A grep-like
 * caller has many files; one text per file costs an allocation, a wait and four launches each, and the plain text over the
 * concatenation glues a file's last line without a delimiter to the next file's first and maps no hit back to its file.
 *   file_off  nfiles + 1 byte positions: file_off[0] = 0, non-decreasing, file_off[nfiles] = nbytes.  File j is
 *     text[file_off[j], file_off[j + 1]); equal neighbours are an empty file.
 *   off       the sorted union, without duplicates, of the plain offsets (fsm_hip_text_open's rule) and the file_off values:
 *     strictly increasing, n + 1 entries, off[0] = 0, off[n] = nbytes.  Equivalently: the lines of every file cut on its own,
 *     in file order.  An empty file has no line; a file's last line has no delimiter iff the file does not end in one; a file
 *     that begins with the delimiter begins with an empty line.  Every line still has at least one byte.
 *   file_lines  nfiles + 1 entries with off[file_lines[j]] == file_off[j]: file_lines[0] = 0, file_lines[nfiles] = n, the lines
 *     of file j are [file_lines[j], file_lines[j + 1]); all members of a run of equal file_off values get the same index.
 * The result is an ordinary text: fsm_hip_text_exec{,_device}, fsm_hip_text_hits{,_device}, fsm_hip_text_offsets* and
 * fsm_hip_text_lines take it unchanged (a line without a trailing delimiter in mid-buffer is a packed input like any other).
 * fsm_hip_text_open_files follows fsm_hip_text_open's contract and copies file_off too; the array is checked on the host before
 * any device work.  fsm_hip_text_open_files_device follows fsm_hip_text_open_device's: d_file_off is device memory that must
 * outlive the text and stay as it is, it is checked in a kernel and the verdict rides the call's ONE wait on hip_stream with the
 * line count (an added line end is counted from one text byte: a file end p with 0 < p < nbytes, once per run of equal values,
 * adds one iff text[p - 1] != delim); the kernels that fill off and file_lines may be in flight at return, later work on
 * hip_stream sees the arrays, the accessors that copy out wait for the text's event.  Whatever d_file_off holds, no byte outside
 * [d_text, d_text + nbytes) is read and no store lands outside the arrays sized from the counted totals.
 * NULL + errno: ENODEV (checked first), EINVAL (nfiles == 0, file_off NULL, an array that breaks the three conditions, delim
 * outside 0..255; nothing is leaked and the next call works), ENOMEM.
 *   The hits of a text of files carry file_first, nfiles + 1 entries: file_first[j] = the selected lines with index below
 * file_lines[j], file_first[nfiles] = m.  The hits of file j are hits [file_first[j], file_first[j + 1]) of lines, out_off and
 * bytes: their count is grep -c per file, non-zero / zero is -l / -L, lines[k] - file_lines[j] + 1 the number -n prints.  Both
 * hits forms make it on their own stream and under their own event, also under FSM_HIP_HITS_NO_BYTES and when m == 0. */
struct fsm_hip_text *fsm_hip_text_open_files(const void *text, size_t nbytes, int delim,
	const uint64_t *file_off, size_t nfiles);
struct fsm_hip_text *fsm_hip_text_open_files_device(const void *d_text, size_t nbytes, int delim,
	const uint64_t *d_file_off, size_t nfiles, void *hip_stream);
size_t fsm_hip_text_files(const struct fsm_hip_text *t);                       /* 0: a plain text (or NULL) */
const uint64_t *fsm_hip_text_file_lines_device(const struct fsm_hip_text *t);  /* nfiles + 1; NULL: plain */
int fsm_hip_text_file_lines(const struct fsm_hip_text *t, uint64_t *out);      /* copy out, waits; -1 + EINVAL: plain / NULL */
double fsm_hip_text_files_ms(const struct fsm_hip_text *t);                    /* the added kernels alone, by HIP events; -1 + EINVAL: plain / NULL */
size_t fsm_hip_text_files_block(void);                                         /* for tests: file ends one scan round takes */
const uint64_t *fsm_hip_text_hits_file_first_device(const struct fsm_hip_text_hits *h);  /* nfiles + 1; NULL: plain text */
int fsm_hip_text_hits_file_first(const struct fsm_hip_text_hits *h, uint64_t *out);      /* copy out, waits; -1 + EINVAL: plain / NULL */
double fsm_hip_text_hits_file_first_ms(const struct fsm_hip_text_hits *h);               /* its one kernel; -1 + EINVAL: plain / NULL */

/* Context: the hits of the lines within reach of a selected line of the same file (grep -A NUM, -B NUM, -C NUM), with the two
 * marks a printer needs, and no host pass over the n lines.  The rule, for a text of n lines:
 *   S[i]     = i < n and (bit i of the bitmap ^ FSM_HIP_HITS_INVERT given); the spare bits of the last word are ignored.  INVERT
 *              applies BEFORE the widening (grep -v -A).
 *   file(i)  = 0 for a plain text; for a text of files the j with file_lines[j] <= i < file_lines[j + 1].
 *   W[i]     holds iff there is a p with S[p], file(p) == file(i) and p - before <= i <= p + after, over the integers: before
 *              and after are any uint64_t, before = after = 2^64 - 1 means "the whole file" and does not wrap.
 *   The hits are those of W: m, lines, out_off, bytes and file_first are exactly what fsm_hip_text_hits_device would make of a
 *   bitmap holding W (FSM_HIP_HITS_NO_BYTES still makes lines, core, group and file_first).
 *   core     ceil(m / 64) words, bit k set iff S[lines[k]]: the hit is a selected line (grep's ':'), not context ('-').  The
 *            spare bits are 0.
 *   group    ceil(m / 64) words, bit k set iff k == 0, or lines[k] != lines[k - 1] + 1, or file(lines[k]) != file(lines[k - 1]):
 *            grep prints "--" before every group but the first.  The spare bits are 0.
 *   core_count = the number of i with S[i] (what -c prints: context does not change it); groups = the set group bits.
 *   before = after = 0 gives the lines of the plain hits, core all ones and group marking the runs; no selected line gives
 *   m == 0 whatever the context.
 * The two forms follow the contracts of fsm_hip_text_hits and fsm_hip_text_hits_device word for word: the same two flags (an
 * unknown bit: EINVAL), ENODEV checked first, the device form waits for the text's offsets event and synchronises hip_stream
 * ONCE (m, the byte total and core_count ride that wait); emit, marks and gather may be in flight at return; stores land only
 * below the counted totals and no byte outside the text is read, whatever the bitmap holds or becomes.  The cost does not grow
 * with before or after.  The widened bitmap belongs to the hits and is freed with them.
 * On hits made by fsm_hip_text_hits{,_device}: the two _device accessors return NULL, _marks returns -1 + EINVAL, _core_count and
 * _groups return 0, _context_ms returns -1 + EINVAL. */
struct fsm_hip_text_hits *fsm_hip_text_hits_context(const struct fsm_hip_lines_dfa *ld, const struct fsm_hip_text *t,
	unsigned flags, uint64_t before, uint64_t after);
struct fsm_hip_text_hits *fsm_hip_text_hits_context_device(const struct fsm_hip_text *t, const uint64_t *d_bitmap,
	unsigned flags, uint64_t before, uint64_t after, void *hip_stream);
const uint64_t *fsm_hip_text_hits_core_device(const struct fsm_hip_text_hits *h);    /* ceil(m / 64) words; NULL: m == 0 or hits without context */
const uint64_t *fsm_hip_text_hits_group_device(const struct fsm_hip_text_hits *h);   /* likewise */
int fsm_hip_text_hits_marks(const struct fsm_hip_text_hits *h, uint64_t *core, uint64_t *group);  /* copy out whichever are not NULL; waits */
size_t fsm_hip_text_hits_core_count(const struct fsm_hip_text_hits *h);
size_t fsm_hip_text_hits_groups(const struct fsm_hip_text_hits *h);                  /* may wait for the hits' event */
double fsm_hip_text_hits_context_ms(const struct fsm_hip_text_hits *h);              /* the added kernels alone, by HIP events */
size_t fsm_hip_text_context_scan_block(void);                                        /* for tests: blocks of lines one round of the context scan takes */

/* ------------------------------------------------------------------ */
/* match positions: first / last accepting offset, spans of a hit      */
/* ------------------------------------------------------------------ */

/* Accept positions: WHERE in an input the walk's state is an end state.  Every front above answers with the state a walk ends
 * in; this one with the first and the last position on the way at which the state is an end state -- what grep -o, -b -o,
 * --color, a lexer's longest match and "offset of the first hit in this record" need.
 *   The input has bytes b[0 .. len).  s_0 = start, s_{k+1} = delta(s_k, b[k]); DEAD after a missing edge is sticky.  A(k) means
 *   "s_k is an end state", for k in 0 .. len inclusive: k = 0 is the start state, before any byte.  first = the smallest k with
 *   A(k), last = the largest; both FSM_HIP_NO_POS when there is none.  As fsm_exec stops pulling bytes at a missing edge, a lane
 *   stops at DEAD; in an absorbing end state every later position accepts, so last = len and the lane stops.
 * Range, direction, trim:
 *   Input j is line i = pick[j] of a packed text with n + 1 u64 offsets (pick == NULL: j = i and m = n).  len = off[i + 1] -
 *   off[i]; with trim_byte >= 0 a non-empty line whose last byte equals trim_byte is one byte shorter (the delimiter the text
 *   front leaves at the end of every line but possibly the last of a text or of a file: this path takes the ORIGINAL automaton,
 *   not the identity-column twin of fsm_hip_lines_dfa_create).  to' = min(to[j], len), to == NULL: len.  from' = from[j], from ==
 *   NULL: 0.  If from' > to' the input is not walked and both outputs are NO_POS; this includes from[j] == FSM_HIP_NO_POS.
 *   Forward: bytes from' .. to' - 1 ascending; the position after c bytes is from' + c.  FSM_HIP_POS_BACKWARD: bytes to' - 1 down
 *   to from'; the position after c bytes is to' - c.  Positions are byte boundaries relative to the line's first byte, in
 *   [from', to'].  first and last are in WALKING order: backward, first is the largest position and last the smallest.
 * struct fsm_hip_pos_dfa is the device image of a dfa for this walk, made from its host-side plan (a FSM_HIP_DEFER_UPLOAD dfa
 * serves as well and is not uploaded by it); the dfa may be freed once the image exists.  The image lives on the dfa's device.
 * fsm_hip_exec_accept_pos takes host pointers: it stages, launches and copies back; offsets that decrease and a pick[j] >= n are
 * EINVAL before any launch; `limit` is ignored (off[n] bytes of base are read).  fsm_hip_exec_accept_pos_device takes device
 * pointers and is asynchronous on hip_stream; a pick[j] >= n gives NO_POS and nothing is read for it; no byte outside
 * [base, base + limit) is read whatever the offsets hold (limit == 0: off[n], read on the device).  Either output may be NULL.
 * m == 0 (n == 0 without a pick) launches nothing and returns 0.  0, or -1 + errno: ENODEV (checked first: there is no CPU
 * path), EINVAL (pd or the batch NULL, off NULL, base NULL with bytes to read, an unknown flag bit, trim_byte outside -1 .. 255;
 * no buffer is touched and the next call answers), ENOMEM. */
#define FSM_HIP_NO_POS UINT64_MAX
#define FSM_HIP_POS_BACKWARD 1u
struct fsm_hip_pos_dfa;
struct fsm_hip_pos_batch {
	const void *base;          /* the text's bytes */
	const uint64_t *off;       /* n + 1 line offsets into base */
	size_t n;                  /* lines */
	const uint64_t *pick;      /* m line indices, or NULL: every line in order */
	size_t m;                  /* inputs; ignored (n) when pick == NULL */
	const uint64_t *from;      /* m, or NULL: 0 */
	const uint64_t *to;        /* m, or NULL: the line's length */
	int trim_byte;             /* -1: none */
	unsigned flags;            /* FSM_HIP_POS_BACKWARD */
	uint64_t *first_out;       /* m, or NULL */
	uint64_t *last_out;        /* m, or NULL */
	uint64_t limit;            /* device form: bytes of base that may be read; 0: off[n] */
};
struct fsm_hip_pos_dfa *fsm_hip_pos_dfa_create(const struct fsm_hip_dfa *dfa);
void fsm_hip_pos_dfa_free(struct fsm_hip_pos_dfa *pd);
int fsm_hip_pos_dfa_in_lds(const struct fsm_hip_pos_dfa *pd);   /* 1: the table is walked from LDS (S1 * C <= 16 384 entries); 0: from device memory, or NULL */
int fsm_hip_exec_accept_pos(const struct fsm_hip_pos_dfa *pd, const struct fsm_hip_pos_batch *batch);
int fsm_hip_exec_accept_pos_device(const struct fsm_hip_pos_dfa *pd, const struct fsm_hip_pos_batch *d_batch, void *hip_stream);

/* Spans of a text's hits: the leftmost-longest match of every hit, advanced match by match on the device.  The caller gives two
 * automata: `starts` is walked backward, `ends` forward, both as ORIGINAL automata with trim_byte = the text's delimiter.  For
 * a hit whose (trimmed) line has length len, and a search position p:
 *   start = last of `starts` walked backward over [p, len); if start != NO_POS, end = last of `ends` walked forward over
 *   [start, len).  If either is NO_POS the hit has no span: both are NO_POS.
 * Round 0 has p = 0 for every hit.  fsm_hip_text_spans_next sets p = end if end > start, else end + 1 (an empty match advances by
 * one; it is reported as it is and the caller drops it as grep does), runs the two walks again and returns 0 or -1 + errno.  A hit
 * without a span gets p = NO_POS and stays without one.  When `starts` accepts the reversal of pat preceded by anything and
 * `ends` accepts exactly pat, the rounds deliver POSIX leftmost-longest, non-overlapping matches: what grep -o prints.  The
 * library does not check that the two automata belong together: the result is defined for any pair.
 * It works on every kind of hits: inverted hits and context lines simply have no span; FSM_HIP_HITS_NO_BYTES hits are fine (the
 * text is read, not the gathered bytes).  The work is enqueued on hip_stream after the hits' last event; _next uses the same
 * stream.  m == 0 gives a valid object with count 0 and nothing launched.  _count: the hits with a span in the current round,
 * counted on the device; one wait.  _copy copies out whichever of start / end are not NULL (m entries each) and waits; _ms: the
 * current round's kernels by HIP events.  The spans must be freed before their hits, their text and the two images.
 * NULL + errno: ENODEV (checked first), EINVAL (an argument NULL, an image on another device than the text), ENOMEM. */
struct fsm_hip_text_spans;
struct fsm_hip_text_spans *fsm_hip_text_hits_spans(const struct fsm_hip_text_hits *h, const struct fsm_hip_text *t,
	const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_pos_dfa *ends, void *hip_stream);
int fsm_hip_text_spans_next(struct fsm_hip_text_spans *sp);
size_t fsm_hip_text_spans_count(const struct fsm_hip_text_spans *sp);
const uint64_t *fsm_hip_text_spans_start_device(const struct fsm_hip_text_spans *sp);   /* m entries; NULL when m == 0 */
const uint64_t *fsm_hip_text_spans_end_device(const struct fsm_hip_text_spans *sp);
int fsm_hip_text_spans_copy(const struct fsm_hip_text_spans *sp, uint64_t *start, uint64_t *end);
double fsm_hip_text_spans_ms(const struct fsm_hip_text_spans *sp);
void fsm_hip_text_spans_free(struct fsm_hip_text_spans *sp);

/* ------------------------------------------------------------------ */
/* tokens: every line cut into longest-match tokens with end-ids       */
/* ------------------------------------------------------------------ */

/* The loop around a DFA in a lexer, for every line at once and in one launch per pass: a token is the longest prefix at a
 * cursor that the automaton accepts, with the end-id of the state it was accepted in; after a token the cursor moves behind it
 * and the same happens again until the line ends.
 *   Input j is line pick[j] of a packed text: base, off[n + 1], pick / m or NULL, trim_byte, limit exactly as in struct
 *   fsm_hip_pos_batch; len is the trimmed length; positions are byte boundaries relative to the line's first byte.
 *   The cursor p starts at 0.  While p < len:
 *   1. Walk the automaton from its start state over bytes p, p + 1, ...  The walk stops at a missing edge (DEAD), at len, or on
 *      entering an absorbing state (one whose every byte leads back to it).  stop is the number of bytes consumed when it
 *      stops, counted from the line's first byte; the byte with the missing edge is not consumed.
 *   2. Longest-match rule (the default): e is the largest position in (p, len] at which the walk's state is an end state.  The
 *      start state before any byte does not count: tokens are never empty.  An absorbing end state accepts at every later
 *      position, so there e = len, and the bytes are not read.  q is the state at e.
 *   3. FSM_HIP_TOKENS_NO_BACKTRACK: the token is (stop, the state at stop) if stop > p and that state is an end state;
 *      otherwise there is none.  This is what lx's generated lexers do: they push back one character and never return to an
 *      earlier accept.
 *   4. A token: (end = e, id = id(q)) is emitted and p = e.  id() follows the image's ids mode: FSM_HIP_IDS_EARLIEST the lowest
 *      end-id of q (a lower id is a higher rule priority), FSM_HIP_IDS_RET the index of its id set (the dfa's fsm_hip_ret_*
 *      tables); an end state without ids gives FSM_HIP_NO_ID under EARLIEST.  FSM_HIP_IDS_ERROR is refused at create (EINVAL)
 *      when fsm_hip_ids_conflict says so, and is EARLIEST otherwise.
 *   5. No token at p: err[j] is the first such p (FSM_HIP_NO_POS if there is none).  By default the line stops there.  With
 *      FSM_HIP_TOKENS_SKIP_BAD the one-byte token (p + 1, FSM_HIP_NO_MATCH) is emitted and the loop continues at p + 1.
 *   Token t of a line starts where token t - 1 ended, the first at 0: only end and id are stored.  The tokens of a line tile
 *   [0, err) by default and the whole line under SKIP_BAD.
 * Cost: the bytes WALKED, which includes every overrun -- the bytes walked past e before the walk stopped are walked again
 * from the next cursor.  The worst case is quadratic in the line's length.  Every step of the loop moves p forward by at least
 * one byte or ends the line.
 * struct fsm_hip_tok_dfa is the device image of a dfa for this walk, made from its host-side plan as fsm_hip_pos_dfa_create
 * makes its own (a FSM_HIP_DEFER_UPLOAD dfa serves; the dfa may be freed afterwards), with one id per state under ids_mode.
 * fsm_hip_tokens_run_device takes device pointers and hip_stream: a count pass, a scan of the counts, ONE wait for the total
 * (as the hits have), the allocation, the emit pass, which is in flight at return.  A pick[j] >= n has no tokens and nothing is
 * read for it; no byte outside [base, base + limit) is read whatever the offsets hold (limit == 0: off[n], read on the device).
 * fsm_hip_tokens_run takes host pointers, stages them and waits; decreasing offsets and a pick[j] >= n are EINVAL before any
 * launch; `limit` is ignored.  The object owns, on the device: off[m + 1] (the exclusive scan of the lines' token counts; off[m]
 * = total), end[total] u64, id[total] u32, err[m].  _count is m.  _copy copies out whichever of off / end / id / err are not
 * NULL and waits; _ms: the two walks and the scan by HIP events.  m == 0 or total == 0 gives a valid object and launches
 * nothing that stores (the pointers of empty arrays are NULL, but off is always there).
 * fsm_hip_text_tokens tokenises every line of a text object, or (hits != NULL) the lines of its hits in their order, with
 * trim_byte = the text's delimiter: it takes the ORIGINAL automaton, as the spans do.  Its work is enqueued on hip_stream after
 * the text's (the hits') last event.  The tokens must be freed before the image, and before the text where they came from one.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (an argument NULL, off NULL, base NULL with bytes to read,
 * an unknown flag bit, trim_byte outside -1 .. 255, an image on another device than the text), ENOMEM. */
#define FSM_HIP_TOKENS_NO_BACKTRACK 1u
#define FSM_HIP_TOKENS_SKIP_BAD 2u
struct fsm_hip_tok_dfa;
struct fsm_hip_tokens;
struct fsm_hip_tok_batch {
	const void *base;          /* the text's bytes */
	const uint64_t *off;       /* n + 1 line offsets into base */
	size_t n;                  /* lines */
	const uint64_t *pick;      /* m line indices, or NULL: every line in order */
	size_t m;                  /* inputs; ignored (n) when pick == NULL */
	int trim_byte;             /* -1: none */
	unsigned flags;            /* FSM_HIP_TOKENS_* */
	uint64_t limit;            /* device form: bytes of base that may be read; 0: off[n] */
};
struct fsm_hip_tok_dfa *fsm_hip_tok_dfa_create(const struct fsm_hip_dfa *dfa, int ids_mode);
void fsm_hip_tok_dfa_free(struct fsm_hip_tok_dfa *td);
int fsm_hip_tok_dfa_in_lds(const struct fsm_hip_tok_dfa *td);   /* 1: the table is walked from LDS (S1 * C <= 16 384 entries); 0: from device memory, or NULL */
struct fsm_hip_tokens *fsm_hip_tokens_run(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_tok_batch *batch);
struct fsm_hip_tokens *fsm_hip_tokens_run_device(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_tok_batch *d_batch, void *hip_stream);
struct fsm_hip_tokens *fsm_hip_text_tokens(const struct fsm_hip_tok_dfa *td, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits,
	unsigned flags, void *hip_stream);
size_t fsm_hip_tokens_count(const struct fsm_hip_tokens *tk);    /* m: the inputs */
size_t fsm_hip_tokens_total(const struct fsm_hip_tokens *tk);    /* the tokens of all inputs */
const uint64_t *fsm_hip_tokens_off_device(const struct fsm_hip_tokens *tk);    /* m + 1 */
const uint64_t *fsm_hip_tokens_end_device(const struct fsm_hip_tokens *tk);    /* total; NULL when total == 0 */
const uint32_t *fsm_hip_tokens_id_device(const struct fsm_hip_tokens *tk);     /* total; NULL when total == 0 */
const uint64_t *fsm_hip_tokens_err_device(const struct fsm_hip_tokens *tk);    /* m; NULL when m == 0 */
int fsm_hip_tokens_copy(const struct fsm_hip_tokens *tk, uint64_t *off, uint64_t *end, uint32_t *id, uint64_t *err);
double fsm_hip_tokens_ms(const struct fsm_hip_tokens *tk);
double fsm_hip_tokens_pass_ms(const struct fsm_hip_tokens *tk, int pass);      /* 0: the count pass, 1: the scan, 2: the emit pass */
void fsm_hip_tokens_free(struct fsm_hip_tokens *tk);

/* ------------------------------------------------------------------ */
/* matches: every match of every line: start, end, end-id, in one call */
/* ------------------------------------------------------------------ */

/* All occurrences of a pattern in every line, without a host round per match: what grep -o, --color and a scanner with a union
 * of rules need, and which rule it was.  The caller gives two images: `starts`, a struct fsm_hip_pos_dfa, walked backward, and
 * `ends`, a struct fsm_hip_tok_dfa, walked forward; `ends` carries the end bit of every state, the start state included, and one
 * id per state under its ids mode.
 *   Input j is line pick[j] of a packed text: base, off[n + 1], pick / m or NULL, trim_byte, limit exactly as in struct
 *   fsm_hip_tok_batch; len is the trimmed length; positions are byte boundaries relative to the line's first byte.
 *   M(s), for s in [0, len]: the state of `starts` after walking bytes len - 1 down to s from its start state is an end state.
 *   s = len is the start state, before any byte.  DEAD after a missing edge is sticky; once the walk is in an absorbing end state
 *   every smaller s has M(s).
 *   The cursor p starts at 0.  While p <= len:
 *   1. start = the smallest s in [p, len] with M(s).  If there is none the input is done.
 *   2. Walk `ends` from its start state over bytes start, start + 1, ...  The walk stops at a missing edge (DEAD), at len, or on
 *      entering an absorbing state.
 *   3. end = the largest e in [start, len] at which the walk's state is an end state.  e = start counts (the start state before
 *      any byte): an empty match.  An absorbing end state accepts at every later position, so there end = len, and the bytes are
 *      not read.  q is the state at end.
 *   4. If there is no such e the input is done: a hit without a span stays without one (the rule of the rounds).
 *   5. The match (start, end, id(q)) is emitted; id() follows the `ends` image's ids mode, as for tokens.
 *   6. With FSM_HIP_MATCHES_DROP_EMPTY a match with end == start is not emitted (what grep does); the cursor moves the same.
 *   7. p = end if end > start, else end + 1.
 *   This is the sequence the rounds of fsm_hip_text_hits_spans / fsm_hip_text_spans_next deliver for the same two automata:
 *   per input, round after round up to the first FSM_HIP_NO_POS.  When `starts` accepts the reversal of pat preceded by anything
 *   and `ends` accepts exactly pat it is POSIX leftmost-longest, non-overlapping.  The library does not check that the two belong
 *   together: the result is defined for any pair.
 * Cost: `starts` walks every byte of a line at most ONCE however many matches the line has, and leaves one bit per position
 * (the marks: internal to the object, len / 8 bytes of a walked line are written, addressed from the line's offset so that no
 * scan is needed and no offsets can make a store leave the array; the array itself is sized by the limit, not by the lines that
 * are walked -- limit / 8 + 2 n bytes, 128 MiB for a text of 1 GiB even for a single hit -- and is freed with the object); a lane
 * then goes from mark to mark, sixteen positions a load, and never takes a position behind len.
 * `ends` walks the bytes of every match and its overrun -- the bytes walked past end before the walk stopped are walked again
 * from a later start, as for tokens.  Every step of the loop moves p forward by at least one byte or ends the input.
 * fsm_hip_matches_run_device takes device pointers and hip_stream: the marks pass, a count pass, a scan of the counts, ONE wait
 * for the total, the allocation, the emit pass, which is in flight at return.  The marks are sized by the bytes that may be
 * read, so limit == 0 costs a second, short wait up front in which off[n] is read: give the limit.  A pick[j] >= n has no match
 * and nothing is read for it; no byte outside [base, base + limit) is read whatever the offsets hold.  Offsets that decrease can
 * give wrong matches, never a store outside the object's arrays.
 * fsm_hip_matches_run takes host pointers, stages them and waits; decreasing offsets and a pick[j] >= n are EINVAL before any
 * launch; `limit` is ignored.  The object owns, on the device: off[m + 1] (the exclusive scan of the inputs' match counts; off[m]
 * = total), start[total] and end[total] u64, id[total] u32.  _count is m.  _copy copies out whichever of off / start / end / id
 * are not NULL and waits; _ms: the four passes by HIP events; _pass_ms: one of them.  m == 0 or total == 0 gives a valid object
 * and launches nothing that stores into its arrays (the pointers of empty arrays are NULL, but off is always there).
 * fsm_hip_text_matches covers every line of a text object, or (hits != NULL) the lines of its hits in their order -- every kind
 * of hits, FSM_HIP_HITS_NO_BYTES too: the text is read -- with trim_byte = the text's delimiter: both images are of ORIGINAL
 * automata, as for the spans.  Its work is enqueued on hip_stream after the text's (the hits') last event.  The matches must be
 * freed before both images, and before the text where they came from one.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (an argument NULL, off NULL, base NULL with bytes to read,
 * an unknown flag bit, trim_byte outside -1 .. 255, the two images or the text on different devices), ENOMEM. */
#define FSM_HIP_MATCHES_DROP_EMPTY 1u
struct fsm_hip_matches;
struct fsm_hip_match_batch {
	const void *base;          /* the text's bytes */
	const uint64_t *off;       /* n + 1 line offsets into base */
	size_t n;                  /* lines */
	const uint64_t *pick;      /* m line indices, or NULL: every line in order */
	size_t m;                  /* inputs; ignored (n) when pick == NULL */
	int trim_byte;             /* -1: none */
	unsigned flags;            /* FSM_HIP_MATCHES_* */
	uint64_t limit;            /* device form: bytes of base that may be read; 0: off[n] */
};
struct fsm_hip_matches *fsm_hip_matches_run(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_match_batch *batch);
struct fsm_hip_matches *fsm_hip_matches_run_device(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_match_batch *d_batch, void *hip_stream);
struct fsm_hip_matches *fsm_hip_text_matches(const struct fsm_hip_pos_dfa *starts, const struct fsm_hip_tok_dfa *ends,
	const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits, unsigned flags, void *hip_stream);
size_t fsm_hip_matches_count(const struct fsm_hip_matches *mt);    /* m: the inputs */
size_t fsm_hip_matches_total(const struct fsm_hip_matches *mt);    /* the matches of all inputs */
const uint64_t *fsm_hip_matches_off_device(const struct fsm_hip_matches *mt);      /* m + 1 */
const uint64_t *fsm_hip_matches_start_device(const struct fsm_hip_matches *mt);    /* total; NULL when total == 0 */
const uint64_t *fsm_hip_matches_end_device(const struct fsm_hip_matches *mt);      /* total; NULL when total == 0 */
const uint32_t *fsm_hip_matches_id_device(const struct fsm_hip_matches *mt);       /* total; NULL when total == 0 */
int fsm_hip_matches_copy(const struct fsm_hip_matches *mt, uint64_t *off, uint64_t *start, uint64_t *end, uint32_t *id);
double fsm_hip_matches_ms(const struct fsm_hip_matches *mt);
double fsm_hip_matches_pass_ms(const struct fsm_hip_matches *mt, int pass);        /* 0: the marks, 1: the count pass, 2: the scan, 3: the emit pass */
void fsm_hip_matches_free(struct fsm_hip_matches *mt);

/* ------------------------------------------------------------------ */
/* replace: every match replaced by its rule's replacement, on the device */
/* ------------------------------------------------------------------ */

/* sed 's/pat/repl/g' for a union of rules, redaction, normalising: the matches are on the device and so is the text; the result
 * is a fresh packed text there, without a host loop over bytes.
 *   Input j is line pick[j] of a packed text: base, off, n, pick, m, trim_byte and limit exactly as in struct fsm_hip_match_batch.
 *   raw is the line's byte count and len its trimmed length, so raw - len is 0 or 1.  Its matches are entries moff[j] .. moff[j + 1]
 *   of a struct fsm_hip_matches, which must have been made from the same batch: m must equal fsm_hip_matches_count (EINVAL), the
 *   rest is the caller's word.  The batch's flags are not used, but they and trim_byte must be what the matches accept.
 *   A replacement table holds nrepl byte strings, R[i] = bytes[roff[i] .. roff[i + 1]).
 *   The output line is built from these pieces, in order:
 *   - the bytes [0, start_0);
 *   - then, for each match k in order, X_k followed by the bytes [end_k, start_{k+1}); the last match is followed by
 *     [end_last, len);
 *   - then the bytes [len, raw): the trimmed delimiter is copied, so replacing in every line of a text yields a text with the
 *     same delimiters.  (The output therefore does not depend on trim_byte, and nothing reads it.)
 *   X_k:
 *   - default table: X_k = R[id_k] if id_k < nrepl; otherwise the match's own bytes -- a rule without a replacement,
 *     FSM_HIP_NO_ID and FSM_HIP_NO_MATCH: the text stays.
 *   - an empty match (end == start, present when the matches were made without FSM_HIP_MATCHES_DROP_EMPTY) inserts R[id], as
 *     sed does.
 *   - a table made with FSM_HIP_REPL_MASK: X_k has the match's length and its byte t is R[id][t mod |R[id]|]; if |R[id]| == 0 or
 *     id >= nrepl the match stays.  Lengths never change under this flag: the redaction case.
 *   - a TEMPLATE table (fsm_hip_repl_create_template) puts the match itself inside its replacement: sed's `&`.  Besides the nrepl
 *     literal strings R[i] it holds, per rule, a list of insert positions ins[ioff[i] .. ioff[i + 1]): each an index into R[i] in
 *     0 .. |R[i]|, relative to the rule's own first byte, ascending, equal entries allowed (`&&`), at most
 *     fsm_hip_repl_max_inserts() = 255 of them per rule.  For a match with id i < nrepl, own bytes M and the c inserts
 *     a_0 <= ... <= a_{c-1} of its rule
 *         X_k = R[i][0:a_0]  M  R[i][a_0:a_1]  M  ...  M  R[i][a_{c-1}:|R[i]|]          |X_k| = |R[i]| + c * |M|
 *     c = 0 is the plain replacement; an empty R[i] with one insert at 0 is the identity for that rule; an empty match gives
 *     X_k = R[i]; id >= nrepl: the match stays.  The cap is an interface condition: |X_k| <= |R[i]| + 255 * raw, so no output
 *     length wraps a uint64_t, and a rule's insert count fits a byte.  A template table takes no flag: a template repeated to the
 *     match's length (MASK) has no meaning.  Captures and numbered groups are not built: the whole match needs none.
 *   The result is again a packed text, out_off[m + 1] with out_off[0] = 0 plus bytes[out_off[m]], so it can be fed to any device
 *   front of the library.
 * A pick[j] >= n (device form) gives an empty output line and nothing is read.  No byte outside [base, base + limit) is read and
 * no store leaves the object's arrays, whatever the offsets or the match arrays hold: line extents are clamped to the limit by
 * the helper the matches' passes use, so lengths agree; a match is taken inside its line and behind its predecessor.  Wrong
 * arrays may give wrong bytes, never a wild access.
 * Passes: the lengths (per input its output length, per match its place in the output line, per block of
 * fsm_hip_replaced_block_lines() inputs the block's bytes), a scan of the BLOCK sums by one workgroup -- m / block_lines records,
 * not m --, ONE wait for the total, the allocation, the offsets (the block's own scan redone; an index per block of
 * fsm_hip_replaced_block_bytes() output bytes, sized by the total, which is why this pass follows the wait), the write pass: a lane
 * owns 16 output bytes and finds their line and their match by two searches.  The offsets and the write pass are in flight at
 * return.  The table's bytes and offsets are read from LDS when nrepl <= fsm_hip_repl_lds_rules() and its bytes <=
 * fsm_hip_repl_lds_bytes() (fsm_hip_repl_in_lds), from device memory otherwise.  A template table with inserts keeps its insert
 * offsets and its positions there too, two bytes each, and their room comes out of the bytes' budget: it is read from LDS when
 * nrepl <= fsm_hip_repl_lds_rules() and (its bytes rounded up to 16) + 2 * (nrepl + 1) + 2 * fsm_hip_repl_inserts() <=
 * fsm_hip_repl_lds_bytes().  A template table without any insert (ioff == NULL, or every rule with none) is a plain table in
 * every respect: the same kernels, the same rule, byte for byte the output of fsm_hip_repl_create(bytes, roff, nrepl, 0).
 * fsm_hip_repl_create takes host pointers and leaves the table on the current device, reusable across calls; nrepl == 0 is valid
 * and gives the identity.  fsm_hip_matches_replace takes host pointers, stages them and waits; decreasing offsets and a
 * pick[j] >= n are EINVAL before any launch; `limit` is ignored.  fsm_hip_matches_replace_device takes device pointers and
 * hip_stream; limit == 0 costs a second, short wait in which off[n] is read, as for the matches.  fsm_hip_text_replace covers
 * every line of a text object or (hits != NULL) the lines of its hits, as fsm_hip_text_matches, whose result for the same text
 * and hits it takes.  The work is enqueued behind the matches' last event, and behind the text's or the hits' for the text form.
 * The replaced object must be freed before the matches, the table and the text.  It owns, on the device: off[m + 1] and the
 * bytes (NULL when there are none).  m == 0 or zero output bytes gives a valid object and launches nothing that stores into bytes.
 * _copy copies out whichever of off / bytes are not NULL and waits; _ms: the four passes by HIP events; _pass_ms: one of them.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (an argument NULL, roff NULL with nrepl > 0, roff that
 * decreases, bytes NULL with bytes to copy, an unknown flag bit, trim_byte outside -1 .. 255, m that is not the matches', objects
 * on different devices; host form: offsets that decrease, a pick[j] >= n; fsm_hip_repl_create_template: any flag, MASK included,
 * ioff[0] != 0, ioff that decreases, ins NULL with ioff[nrepl] > 0, a position above |R[i]|, positions of one rule that decrease,
 * more than fsm_hip_repl_max_inserts() inserts in one rule -- all before any upload), ENOMEM. */
#define FSM_HIP_REPL_MASK 1u
struct fsm_hip_repl;       /* a replacement table resident on the current device, reusable across calls */
struct fsm_hip_repl *fsm_hip_repl_create(const void *bytes, const uint64_t *roff, size_t nrepl, unsigned flags);
void fsm_hip_repl_free(struct fsm_hip_repl *rp);
int fsm_hip_repl_in_lds(const struct fsm_hip_repl *rp);            /* 1: the write pass reads the table from LDS */
size_t fsm_hip_repl_lds_bytes(void);
size_t fsm_hip_repl_lds_rules(void);
/* a template table: ins[ioff[i] .. ioff[i + 1]) are rule i's insert positions; ioff == NULL: no rule has an insert */
struct fsm_hip_repl *fsm_hip_repl_create_template(const void *bytes, const uint64_t *roff, size_t nrepl,
	const uint64_t *ins, const uint64_t *ioff, unsigned flags);
size_t fsm_hip_repl_inserts(const struct fsm_hip_repl *rp);        /* ioff[nrepl]; 0 for NULL and for a plain table */
size_t fsm_hip_repl_max_inserts(void);                             /* per rule: 255 */

struct fsm_hip_replaced;
struct fsm_hip_replaced *fsm_hip_matches_replace(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *batch,
	const struct fsm_hip_repl *rp);
struct fsm_hip_replaced *fsm_hip_matches_replace_device(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *d_batch,
	const struct fsm_hip_repl *rp, void *hip_stream);
struct fsm_hip_replaced *fsm_hip_text_replace(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t,
	const struct fsm_hip_text_hits *hits, const struct fsm_hip_repl *rp, void *hip_stream);
size_t fsm_hip_replaced_count(const struct fsm_hip_replaced *r);               /* m */
uint64_t fsm_hip_replaced_nbytes(const struct fsm_hip_replaced *r);            /* out_off[m] */
const uint64_t *fsm_hip_replaced_off_device(const struct fsm_hip_replaced *r); /* m + 1, always there */
const unsigned char *fsm_hip_replaced_bytes_device(const struct fsm_hip_replaced *r); /* NULL when nbytes == 0 */
int fsm_hip_replaced_copy(const struct fsm_hip_replaced *r, uint64_t *off, void *bytes);
double fsm_hip_replaced_ms(const struct fsm_hip_replaced *r);
double fsm_hip_replaced_pass_ms(const struct fsm_hip_replaced *r, int pass);   /* 0: lengths, 1: scan of the block sums, 2: offsets, 3: write */
size_t fsm_hip_replaced_block_lines(void);     /* inputs of a block of the lengths and the offsets pass */
size_t fsm_hip_replaced_block_bytes(void);     /* output bytes of a block of the write pass */
void fsm_hip_replaced_free(struct fsm_hip_replaced *r);

/* ------------------------------------------------------------------ */
/* extract: every kept match's bytes as a record of a packed text, on the device */
/* ------------------------------------------------------------------ */

/* grep -o for a union of rules, or the first half of "extract, then match the extracts against a second automaton": the
 * complement of replace.  Replace keeps the text around the matches; extraction keeps the matches and drops the text around them.
 * The matches are on the device and so is the text; the result is a fresh packed text there, one record per kept match, without
 * a host loop over bytes.
 *   Input j is line pick[j] of a packed text: base, off, n, pick, m, trim_byte and limit exactly as in struct fsm_hip_match_batch.
 *   The line is clipped to the limit by the helper the matches' and the replacement's passes use; raw is its clipped byte count.
 *   Its matches are entries moff[j] .. moff[j + 1] of a struct fsm_hip_matches, which must have been made from the same batch: m
 *   must equal fsm_hip_matches_count (EINVAL), the rest is the caller's word.  The batch's flags are not used, but they and
 *   trim_byte must be what the matches accept.
 *   Every match k is clamped on its own: en = min(end_k, raw), st = min(start_k, en).  Records do not depend on each other, so
 *   there is no "behind its predecessor" rule as in replace.  Indices read from moff are clamped to the matches' total.
 *   A rule set says which matches are kept: a bitmap of nrules bits, rule i = bit (i & 7) of byte i >> 3 of `bits`, made once
 *   from host memory by fsm_hip_rules_create, resident on the current device and reusable across calls.  keep == NULL keeps every
 *   match.  Otherwise match k is kept when id_k < nrules and bit id_k is set; a set made with FSM_HIP_RULES_KEEP_OTHER also keeps
 *   the matches with id_k >= nrules: rules beyond the set, FSM_HIP_NO_ID and FSM_HIP_NO_MATCH.  nrules == 0 is valid.
 *   Record r is the r-th kept match in the order of k.  Its bytes are the text's [beg + st, beg + en), beg the line's first byte,
 *   followed by the one byte sep_byte if sep_byte >= 0; -1 means no separator.  With '\n' the bytes are what grep -o prints.
 *   Without a separator, empty matches (present when the matches were made without FSM_HIP_MATCHES_DROP_EMPTY) give empty records.
 *   The result is again a packed text, off[R + 1] with off[0] = 0 plus bytes[off[R]], so it can be fed to any device front of
 *   the library (with trim_byte = sep_byte where there is a separator); line[R] is the input j of each record and match[R] its
 *   index k into the matches' arrays, so start, end and id are a gather away.
 * No byte outside [base, base + limit) is read and no store leaves the object's arrays, whatever the offsets or the match arrays
 * hold.  Wrong arrays may give wrong bytes, never a wild access.
 * Passes: the lengths (one lane per MATCH: kept or not, the record's bytes, its first byte, its input, found in moff between the
 * inputs of the block's first and last match; per block of fsm_hip_extracted_block_matches() matches the pair records / bytes), a
 * scan of the BLOCK pairs by one workgroup -- total / block_matches records --, ONE wait for R and the bytes, the allocation, the
 * offsets (the block's own scan redone, the compaction into off / line / match, an index per block of
 * fsm_hip_extracted_block_bytes() output bytes), the write pass: a lane owns 16 output bytes, finds the record of the first by one
 * search and walks on from record to record.  The offsets and the write pass are in flight at return.
 * fsm_hip_matches_extract takes host pointers, stages them and waits; decreasing offsets and a pick[j] >= n are EINVAL before any
 * launch; `limit` is ignored.  fsm_hip_matches_extract_device takes device pointers and hip_stream; a pick[j] >= n has no match
 * and gives no record; limit == 0 costs a second, short wait in which off[n] is read, as for the matches.  fsm_hip_text_extract
 * covers every line of a text object or (hits != NULL, every kind of hits) the lines of its hits, as fsm_hip_text_replace, and
 * takes fsm_hip_text_matches' result for the same text and hits.  The work is enqueued behind the matches' last event, and behind
 * the text's or the hits' for the text form.  The extracted object must be freed before the matches, the set and the text.  It
 * owns, on the device: off[R + 1], the bytes (NULL when there are none), line[R] and match[R] (NULL when R == 0).  R == 0 gives a
 * valid object and launches nothing that stores into the record arrays; off is always there.  _count is R.  _copy copies out
 * whichever of off / bytes / line / match are not NULL and waits; _ms: the four passes by HIP events; _pass_ms: one of them.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (an argument other than keep NULL, bits NULL with nrules > 0,
 * an unknown flag bit, sep_byte or trim_byte outside -1 .. 255, m that is not the matches', objects on different devices; host
 * form: offsets that decrease, a pick[j] >= n), ENOMEM. */
#define FSM_HIP_RULES_KEEP_OTHER 1u
struct fsm_hip_rules;      /* a set of rules resident on the current device, reusable across calls */
struct fsm_hip_rules *fsm_hip_rules_create(const void *bits, size_t nrules, unsigned flags);
void fsm_hip_rules_free(struct fsm_hip_rules *rs);

struct fsm_hip_extracted;
struct fsm_hip_extracted *fsm_hip_matches_extract(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *batch,
	const struct fsm_hip_rules *keep, int sep_byte);
struct fsm_hip_extracted *fsm_hip_matches_extract_device(const struct fsm_hip_matches *mt, const struct fsm_hip_match_batch *d_batch,
	const struct fsm_hip_rules *keep, int sep_byte, void *hip_stream);
struct fsm_hip_extracted *fsm_hip_text_extract(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t,
	const struct fsm_hip_text_hits *hits, const struct fsm_hip_rules *keep, int sep_byte, void *hip_stream);
size_t fsm_hip_extracted_count(const struct fsm_hip_extracted *x);              /* R: the records */
uint64_t fsm_hip_extracted_nbytes(const struct fsm_hip_extracted *x);           /* off[R] */
const uint64_t *fsm_hip_extracted_off_device(const struct fsm_hip_extracted *x);   /* R + 1, always there */
const unsigned char *fsm_hip_extracted_bytes_device(const struct fsm_hip_extracted *x);   /* NULL when nbytes == 0 */
const uint64_t *fsm_hip_extracted_line_device(const struct fsm_hip_extracted *x);  /* R; NULL when R == 0 */
const uint64_t *fsm_hip_extracted_match_device(const struct fsm_hip_extracted *x); /* R; NULL when R == 0 */
int fsm_hip_extracted_copy(const struct fsm_hip_extracted *x, uint64_t *off, void *bytes, uint64_t *line, uint64_t *match);
double fsm_hip_extracted_ms(const struct fsm_hip_extracted *x);
double fsm_hip_extracted_pass_ms(const struct fsm_hip_extracted *x, int pass);  /* 0: lengths, 1: scan of the block pairs, 2: offsets, 3: write */
size_t fsm_hip_extracted_block_matches(void);  /* matches of a block of the lengths and the offsets pass */
size_t fsm_hip_extracted_block_bytes(void);    /* output bytes of a block of the write pass */
void fsm_hip_extracted_free(struct fsm_hip_extracted *x);

/* ------------------------------------------------------------------ */
/* tally: matches and lines per rule and per group, counted on the device */
/* ------------------------------------------------------------------ */

/* Which rules of a union fired, how often, in how many lines, in which files: one reduction over the off[m + 1] and id[total] that
 * a matches object and a tokens object own, without bringing either array to the host.
 *   Input.  off[m + 1] (input j owns entries off[j] .. off[j + 1]), id[total], nrules.
 *   Columns.  C = nrules + 1.  col(x) = x if x < nrules, else nrules: the last column is "other" -- rules beyond nrules,
 *   FSM_HIP_NO_ID, and FSM_HIP_NO_MATCH, which the tokens of FSM_HIP_TOKENS_SKIP_BAD carry.  nrules == 0 is valid: one column.
 *   Groups.  group_off[G + 1] holds input indices; group g is the inputs [group_off[g], group_off[g + 1]).  Equal neighbours are an
 *   empty group.  group_off == NULL means G = 1 and the one group is every input (ngroups is then ignored).  Inputs below
 *   group_off[0] or at or above group_off[G] are counted nowhere.
 *   count[g * C + c] is the number of entries k of the inputs of group g with col(id[k]) == c.
 *   lines[g * C + c] is the number of inputs j of group g that own at least one entry k with col(id[k]) == c: an input counts
 *   once per column however often the column occurs in it.  Per file this is grep -c for one rule of a union.
 *   Both tables are the caller's memory, G * C entries each, row-major.  Either may be NULL, not both.  They are cleared first,
 *   unless FSM_HIP_TALLY_ADD is given: then the new counts are added to what is there -- totals over many texts or calls, or tokens
 *   and matches into one table.
 * Nothing is allocated for the caller and there is no object.  The device forms wait for nothing and are in flight at return.
 * fsm_hip_tally_ids_device is the reduction itself over any arrays of that shape on the current device: id[k] is read for k <
 * total only, an entry of off above total is treated as total, and the group of input j is the last g in [0, G) with group_off[g]
 * <= j, provided j < group_off[G].  Arrays that do not ascend give wrong counts; they never cause a load outside off[0 .. m],
 * id[0 .. total), group_off[0 .. G], and never a store outside the two tables.
 * fsm_hip_matches_tally_device / fsm_hip_tokens_tally_device: the same over the object's own arrays, enqueued behind the object's
 * last event, as extraction is.  fsm_hip_matches_tally / fsm_hip_tokens_tally take host arrays in and out, stage them and wait; a
 * group_off that decreases or whose last entry exceeds m is EINVAL before any launch; with FSM_HIP_TALLY_ADD the host tables are
 * read and added to.  fsm_hip_text_matches_tally / fsm_hip_text_tokens_tally: the groups are the files of the text -- its
 * file_lines when hits == NULL, the hits' file_first otherwise -- so the counts are per file without the caller touching either
 * array; a plain text is one group.  EINVAL when the object's m is not the text's n, or the hits' m, as in fsm_hip_text_extract.
 * The kernel: a workgroup takes a contiguous span of inputs, whole granules of fsm_hip_tally_span_inputs(), and goes through the
 * span's entries in windows of fsm_hip_tally_window(), one lane per entry; two wavefronts find the inputs of the window's ends by a
 * 64-ary search, a lane finds its input between them by the bounded search of the extraction, then its group.  While C <=
 * fsm_hip_tally_lds_columns() the counters are u32 in LDS, flushed to the tables by one atomic add per non-zero bin at every
 * change of group, at the end of the span and before one could wrap; above it only the last column, "other", has such a counter,
 * and every other entry, like every entry of a window that spans a group boundary, adds to the table itself.  Equal destinations
 * of a wavefront are combined first.  For lines an entry counts iff no earlier entry of its input has its column: a backward look
 * through the window, of at most window - 1 steps, and, for the one input that may continue from the window before, a bitmap of
 * fsm_hip_tally_max_line_columns() bits.  No lane's work grows with the entries of an input beyond the window.  Integer adds only:
 * the result is exact and the same on every run.
 * 0, or -1 + errno: ENODEV (checked first: there is no CPU path), EINVAL (an object NULL, both tables NULL, an unknown flag bit,
 * ngroups == 0 with group_off != NULL, the objects and the text on different devices, m that is not the text's; host forms: a
 * group_off that decreases or exceeds m), EOVERFLOW (G * C * 8 does not fit size_t), ENOTSUP (lines asked for and C above
 * fsm_hip_tally_max_line_columns()).  m == 0 or total == 0 is valid: the tables are cleared, unless they are added to, and
 * nothing else is launched. */
#define FSM_HIP_TALLY_ADD 1u
int fsm_hip_tally_ids_device(const uint64_t *d_off, const uint32_t *d_id, size_t m, size_t total, const uint64_t *d_group_off,
	size_t ngroups, size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream);
int fsm_hip_matches_tally_device(const struct fsm_hip_matches *mt, const uint64_t *d_group_off, size_t ngroups, size_t nrules,
	unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream);
int fsm_hip_tokens_tally_device(const struct fsm_hip_tokens *tk, const uint64_t *d_group_off, size_t ngroups, size_t nrules,
	unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream);
int fsm_hip_matches_tally(const struct fsm_hip_matches *mt, const uint64_t *group_off, size_t ngroups, size_t nrules, unsigned flags,
	uint64_t *count, uint64_t *lines);
int fsm_hip_tokens_tally(const struct fsm_hip_tokens *tk, const uint64_t *group_off, size_t ngroups, size_t nrules, unsigned flags,
	uint64_t *count, uint64_t *lines);
int fsm_hip_text_matches_tally(const struct fsm_hip_matches *mt, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits,
	size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream);
int fsm_hip_text_tokens_tally(const struct fsm_hip_tokens *tk, const struct fsm_hip_text *t, const struct fsm_hip_text_hits *hits,
	size_t nrules, unsigned flags, uint64_t *d_count, uint64_t *d_lines, void *hip_stream);
size_t fsm_hip_tally_span_inputs(void);        /* inputs of a granule: a workgroup takes whole granules */
size_t fsm_hip_tally_window(void);             /* entries a workgroup takes a step, one per lane */
size_t fsm_hip_tally_lds_columns(void);        /* columns (nrules + 1) up to which the counters are kept in LDS */
size_t fsm_hip_tally_max_line_columns(void);   /* columns up to which lines can be counted */

/* ------------------------------------------------------------------ */
/* distinct: the distinct records of a packed text, with their counts, on the device */
/* ------------------------------------------------------------------ */

/* grep -o PATTERN | sort | uniq -c without the sort and without the host: which values occur -- addresses, URLs, names, error
 * codes -- and how often.  The tally counts by rule id; this counts by content.
 *   Input.  A packed text on the current device: off[R + 1] (ascending) and bytes; trim_byte in -1 .. 255, with the library's usual
 *   rule: with trim_byte >= 0 a non-empty record whose last byte equals trim_byte is one byte shorter, and at most one byte is
 *   dropped; optionally tag[R].
 *   The KEY of record r is its trimmed bytes, together with tag[r] where tags are given.  Two records are equal iff their keys are:
 *   "a\n" and a final "a" are equal under trim_byte = '\n', a record that is only the trim byte equals an empty record, and equal
 *   bytes under different tags are different keys.
 *   Output.  D distinct keys, numbered by first occurrence.  first[D]: the lowest r of each key, strictly ascending.  count[D]:
 *   the records with that key; the counts sum to R.  class[R]: the d of every record, so first[class[r]] <= r and the keys of r and
 *   of first[class[r]] are equal -- class is what fsm_hip_tally_ids_device takes as its id array, which gives counts per file per
 *   distinct value.  And a fresh packed text of the keys: doff[D + 1] with doff[0] = 0, plus dbytes, the trimmed bytes of record
 *   first[d], each followed by the byte sep_byte if sep_byte >= 0.  With '\n' this is what sort -u prints, in order of first
 *   appearance; it can go back into any device front (with trim_byte = sep_byte), this one included.
 *   Every output is a function of the input alone: none depends on the hash function, the table size or the order in which lanes
 *   arrive.  The result is exact and identical on every run.  The keys are not sorted: callers sort D keys, not R.
 *   Limits.  R <= 2^32 - 2 (EOVERFLOW above).  R == 0 gives a valid object with D = 0 and stores into nothing but doff[0].  No byte
 *   outside [bytes, bytes + min(off[R], nbytes)) is read.  Entries of off are clamped to that limit and to their predecessor, as
 *   the extraction clamps.  No store leaves the object's own arrays: wrong arrays may give wrong classes, never a wild access.
 * Passes.  hash: a lane per record, the key's 16-byte chunks one by one; records above fsm_hip_distinct_long_bytes() are listed
 * and hashed by a wavefront each, with a sum over the chunks that does not depend on how they are split, so no lane's work grows
 * with a record beyond that bound; the trimmed lengths are kept.  insert: an open-addressing, linear-probing table of
 * fsm_hip_distinct_table_slots(R) slots, a power of two >= 2 R; a slot is one u64, tag32(hash) << 32 | r, empty is all ones; a
 * record claims the first empty slot of its chain by a compare-and-swap, and on a slot with its tag it compares its key with the
 * key of the record the slot names -- byte for byte, always: equal hashes decide nothing -- and lowers the slot to its own r by an
 * atomic min where the keys are equal, so every key lives in one slot, which ends holding the LOWEST r of the key.  Equal records
 * of a wavefront are combined before the table is touched: one insert and one add to the slot's counter for all of them.  Slots are
 * read by returning atomics and agent-scope atomic loads alone.  number: first(r) = the slot of r names r; per block of records the
 * pair (firsts, key bytes), the scan of the block pairs by one workgroup, ONE wait for D and the bytes, the allocation, then the
 * block's own scan redone: first, count, doff, class.  write: the extraction's write pass over doff, a lane per 16 output bytes.
 * Number and write are in flight at return.
 * fsm_hip_distinct_device takes device pointers and hip_stream.  fsm_hip_distinct takes host arrays, stages them and waits;
 * nbytes is off[R]; a decreasing off is EINVAL before any launch.  fsm_hip_extracted_distinct is over the records of an extracted
 * object, with trim_byte = the separator the extraction was made with, enqueued behind the object's last event.
 * fsm_hip_text_hits_distinct is over the lines of hits, with trim_byte = the text's delimiter; hits made with
 * FSM_HIP_HITS_NO_BYTES have no lines on the device: EINVAL.  The distinct object must be freed before the objects it came from.
 * It owns, on the device: first[D] and count[D] (NULL when D == 0), class[R] (NULL when R == 0), doff[D + 1] (always there unless
 * FSM_HIP_DISTINCT_NO_TEXT) and the bytes (NULL when there are none).  _count is D, _records R, _nbytes doff[D].  _copy copies out
 * whichever of first / count / class / doff / dbytes are not NULL and waits (doff under NO_TEXT: EINVAL).  _ms: all passes by HIP
 * events; _pass_ms: one of them -- 0 hash, 1 insert (with the clearing of the table), 2 number, 3 write.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (a NULL object, d_off NULL, d_bytes NULL with nbytes > 0, a
 * byte argument outside -1 .. 255, an unknown flag bit; host form: an off that decreases), EOVERFLOW (R > 2^32 - 2), ENOMEM. */
#define FSM_HIP_DISTINCT_NO_TEXT   1u  /* no doff / dbytes: first, count, class only; no second allocation */
#define FSM_HIP_DISTINCT_WEAK_HASH 2u  /* for tests: every chain starts in one of the LAST four slots of the table (by length & 3) */
struct fsm_hip_distinct;
struct fsm_hip_distinct *fsm_hip_distinct_device(const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint32_t *d_tag, int sep_byte, unsigned flags, void *hip_stream);
struct fsm_hip_distinct *fsm_hip_distinct(const uint64_t *off, const void *bytes, size_t R, int trim_byte, const uint32_t *tag,
	int sep_byte, unsigned flags);
struct fsm_hip_distinct *fsm_hip_extracted_distinct(const struct fsm_hip_extracted *x, int sep_byte, unsigned flags, void *hip_stream);
struct fsm_hip_distinct *fsm_hip_text_hits_distinct(const struct fsm_hip_text_hits *hits, int sep_byte, unsigned flags, void *hip_stream);
size_t fsm_hip_distinct_count(const struct fsm_hip_distinct *dx);               /* D: the distinct keys */
size_t fsm_hip_distinct_records(const struct fsm_hip_distinct *dx);             /* R */
uint64_t fsm_hip_distinct_nbytes(const struct fsm_hip_distinct *dx);            /* doff[D]; 0 under NO_TEXT */
const uint64_t *fsm_hip_distinct_first_device(const struct fsm_hip_distinct *dx);   /* D; NULL when D == 0 */
const uint64_t *fsm_hip_distinct_count_device(const struct fsm_hip_distinct *dx);   /* D; NULL when D == 0 */
const uint32_t *fsm_hip_distinct_class_device(const struct fsm_hip_distinct *dx);   /* R; NULL when R == 0 */
const uint64_t *fsm_hip_distinct_off_device(const struct fsm_hip_distinct *dx);     /* D + 1, always there unless NO_TEXT */
const unsigned char *fsm_hip_distinct_bytes_device(const struct fsm_hip_distinct *dx);   /* NULL when nbytes == 0 */
int fsm_hip_distinct_copy(const struct fsm_hip_distinct *dx, uint64_t *first, uint64_t *count, uint32_t *cls, uint64_t *doff, void *dbytes);
double fsm_hip_distinct_ms(const struct fsm_hip_distinct *dx);
double fsm_hip_distinct_pass_ms(const struct fsm_hip_distinct *dx, int pass);   /* 0: hash, 1: insert, 2: number, 3: write */
size_t fsm_hip_distinct_long_bytes(void);      /* keys above it are hashed by a wavefront each */
size_t fsm_hip_distinct_table_slots(size_t R); /* a power of two >= 2 R, at least 16; 0 + EOVERFLOW above 2^32 - 2 */
void fsm_hip_distinct_free(struct fsm_hip_distinct *dx);

/* ------------------------------------------------------------------ */
/* sort: the records of a packed text in byte order, on the device: order, ranks, text */
/* ------------------------------------------------------------------ */

/* The sort of grep -o PATTERN | sort | uniq -c | sort -rn, without the host.
 *   Input.  A packed text on the current device, off[R + 1] and bytes with nbytes, trim_byte and sep_byte in -1 .. 255, and
 *   optionally major[R] (u64).  The KEY of record r is its trimmed bytes under exactly the rules of "distinct": entries of off are
 *   clamped to min(off[R], nbytes) and to their predecessor, and with trim_byte >= 0 a non-empty record whose last byte is the trim
 *   byte is one byte shorter.
 *   Order.  Keys order as memcmp does: bytes are unsigned, and a proper prefix goes before the longer key: "" < "\0" < "\0\0".
 *   With major, records order by major[r] first and by key second.  Records equal in both keep ascending r: the sort is stable.
 *   Flags.  FSM_HIP_SORT_NO_TEXT: no soff / sbytes.  FSM_HIP_SORT_REVERSE: keys descend, so the longer key goes before its prefix;
 *   ties still ascend in r.  FSM_HIP_SORT_MAJOR_DESC: major descends; EINVAL without major.  FSM_HIP_SORT_BY_COUNT: only for
 *   fsm_hip_keys_sort.  Any other bit is EINVAL.
 *   Output.  order[R], u64: order[p] is the record at sorted position p, a permutation of 0 .. R - 1, typed so that it is a valid
 *   `pick` of every device front: they walk the text in sorted order without a byte being moved.  rank[R], u32: rank[p] is the
 *   number of distinct (major, key) pairs before position p's; it is non-decreasing and steps by 0 or 1, and groups = rank[R - 1]
 *   + 1 (0 for no record) is, for equal inputs, the D that "distinct" reports.  Unless NO_TEXT, a fresh packed text soff[R + 1] /
 *   sbytes: record p is the trimmed key of order[p], followed by sep_byte if sep_byte >= 0.  This is what sort prints, and an
 *   input of any device front, this one included.  Every output is a function of the input alone and identical on every run.
 *   Limits.  R <= 2^32 - 2 (EOVERFLOW above).  R == 0 stores nothing but soff[0].  No byte outside [bytes, bytes + min(off[R],
 *   nbytes)) is read; no store leaves the object's own arrays.
 * Passes.  Most-significant-word-first rounds over a stable least-significant-digit radix sort.  Positions, not records, carry the
 * state: bucket[p] is the first position of the run of records equal on everything examined so far, and a bucket is active while
 * it has more than one member and its last word was full.  A round takes the active positions only.  keys: a lane compares its
 * key with its bucket head's from the bucket's depth on, in 16-byte chunks, the minimum over the bucket (an agent-scope atomic)
 * advances the depth in whole words -- equal keys of kilobytes and a shared prefix cost one pass; then the next 8 key bytes big
 * endian, zero-padded, and how many exist (both complemented under REVERSE).  With major, a round before the first takes the u64
 * instead (complemented under MAJOR_DESC).  radix: stable passes of 8 bits over (bucket, word, valid); all digit histograms come
 * from one kernel and a digit with one occupied bin is skipped; a pass is a per-tile histogram, a scan and a scatter whose rank
 * inside a tile of fsm_hip_sort_tile_records() entries is the wave64 match-by-ballot rank.  rebucket: a position whose (bucket,
 * word, valid) differs from its predecessor's is a head; the new buckets, the active positions compacted, and their number to the
 * host: the round's one wait.  fsm_hip_sorted_rounds() is at most ceil(maxlen / 8) + 1, and at most 2 when all keys are equal.
 * finish: rank is a scan of the heads, order is widened, and the text is written by the extraction's write pass; it is in flight
 * at return.
 * fsm_hip_sort_device takes device pointers and hip_stream.  fsm_hip_sort takes host arrays, stages them and waits; nbytes is
 * off[R]; a decreasing off is EINVAL before any launch.  fsm_hip_extracted_sort is over the records of an extracted object, with
 * trim_byte = the separator the extraction was made with; fsm_hip_text_hits_sort over the lines of hits, with trim_byte = the
 * text's delimiter (hits made with FSM_HIP_HITS_NO_BYTES: EINVAL).  fsm_hip_keys_sort sorts the D keys of a distinct object, with
 * trim_byte = the separator the keys were written with (a FSM_HIP_DISTINCT_NO_TEXT object: EINVAL); with FSM_HIP_SORT_BY_COUNT
 * major is the object's count[D] and MAJOR_DESC is implied: uniq -c | sort -rn, ties in byte order.  Each is enqueued behind its
 * object's last event, and the sorted object must be freed before the object it came from.
 * It owns, on the device: order[R] and rank[R] (NULL when R == 0), soff[R + 1] (always there unless NO_TEXT) and the bytes (NULL
 * when there are none).  _records is R, _groups the distinct (major, key) pairs (it waits for the finish), _nbytes soff[R],
 * _rounds the rounds, _radix_passes the radix passes that ran or (skipped != 0) were skipped.  _copy copies out whichever of
 * order / rank / soff / sbytes are not NULL and waits (soff under NO_TEXT: EINVAL).  _ms: all passes by HIP events; _pass_ms: 0
 * keys (major, prefix skip, fetch), 1 radix passes, 2 rebucket -- each summed over the rounds -- and 3 finish and write.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (a NULL object, d_off NULL, d_bytes NULL with nbytes > 0, a
 * byte argument outside -1 .. 255, an unknown flag bit, MAJOR_DESC without major; host form: an off that decreases), EOVERFLOW
 * (R > 2^32 - 2), ENOMEM. */
#define FSM_HIP_SORT_NO_TEXT    1u  /* no soff / sbytes: order and rank only */
#define FSM_HIP_SORT_REVERSE    2u  /* keys descend */
#define FSM_HIP_SORT_MAJOR_DESC 4u  /* major descends */
#define FSM_HIP_SORT_BY_COUNT   8u  /* fsm_hip_keys_sort: major = count[D], descending */
struct fsm_hip_sorted;
struct fsm_hip_sorted *fsm_hip_sort_device(const uint64_t *d_off, const void *d_bytes, size_t R, uint64_t nbytes, int trim_byte,
	const uint64_t *d_major, int sep_byte, unsigned flags, void *hip_stream);
struct fsm_hip_sorted *fsm_hip_sort(const uint64_t *off, const void *bytes, size_t R, int trim_byte, const uint64_t *major,
	int sep_byte, unsigned flags);
struct fsm_hip_sorted *fsm_hip_extracted_sort(const struct fsm_hip_extracted *x, int sep_byte, unsigned flags, void *hip_stream);
struct fsm_hip_sorted *fsm_hip_text_hits_sort(const struct fsm_hip_text_hits *hits, int sep_byte, unsigned flags, void *hip_stream);
struct fsm_hip_sorted *fsm_hip_keys_sort(const struct fsm_hip_distinct *dx, int sep_byte, unsigned flags, void *hip_stream);
size_t fsm_hip_sorted_records(const struct fsm_hip_sorted *sx);                 /* R */
size_t fsm_hip_sorted_groups(const struct fsm_hip_sorted *sx);                  /* rank[R - 1] + 1; 0 when R == 0 */
uint64_t fsm_hip_sorted_nbytes(const struct fsm_hip_sorted *sx);                /* soff[R]; 0 under NO_TEXT */
size_t fsm_hip_sorted_rounds(const struct fsm_hip_sorted *sx);
size_t fsm_hip_sorted_radix_passes(const struct fsm_hip_sorted *sx, int skipped);
const uint64_t *fsm_hip_sorted_order_device(const struct fsm_hip_sorted *sx);   /* R; NULL when R == 0 */
const uint32_t *fsm_hip_sorted_rank_device(const struct fsm_hip_sorted *sx);    /* R; NULL when R == 0 */
const uint64_t *fsm_hip_sorted_off_device(const struct fsm_hip_sorted *sx);     /* R + 1, always there unless NO_TEXT */
const unsigned char *fsm_hip_sorted_bytes_device(const struct fsm_hip_sorted *sx);   /* NULL when nbytes == 0 */
int fsm_hip_sorted_copy(const struct fsm_hip_sorted *sx, uint64_t *order, uint32_t *rank, uint64_t *soff, void *sbytes);
double fsm_hip_sorted_ms(const struct fsm_hip_sorted *sx);
double fsm_hip_sorted_pass_ms(const struct fsm_hip_sorted *sx, int pass);       /* 0: keys, 1: radix passes, 2: rebucket, 3: finish + write */
size_t fsm_hip_sort_tile_records(void);        /* the records one workgroup ranks in a radix pass */
void fsm_hip_sorted_free(struct fsm_hip_sorted *sx);

/* ------------------------------------------------------------------ */
/* find: the records of a packed text among the keys of a distinct object, on the device: class, bitmap, pick */
/* ------------------------------------------------------------------ */

/* grep -F -x -f LIST, comm, "the values of today's log that yesterday's did not have": the records of one text looked up among the
 * records of another, without the host and without a second automaton.
 *   Input.  A finished distinct object `keys`, the dictionary: D keys, made from a source text with a trim byte and optionally tags.
 *   And a second packed text on its device, the probe: off[R + 1], bytes with nbytes, its own trim_byte in -1 .. 255, optionally
 *   tag[R].  The KEY of a probe record is its trimmed bytes and its tag under exactly the rules of "distinct": entries of off are
 *   clamped to min(off[R], nbytes) and to their predecessor, and at most one byte is trimmed.  A NULL tag array is tag 0 for every
 *   record, on either side.  The two trim bytes need not be equal.
 *   Output, all a function of the two inputs alone, identical on every run, independent of the hash, the table size and the
 *   FSM_HIP_DISTINCT_WEAK_HASH the dictionary was built with.  class[R], u32: the d of the dictionary key equal to record r, or
 *   FSM_HIP_FOUND_NONE (D <= 2^32 - 2: no key's number); an id array for fsm_hip_tally_ids_device, where with nrules = D the absent
 *   records fall into the "other" column.  bitmap[ceil(R / 64)], u64: bit r & 63 of word r / 64 is set iff record r is present, the
 *   bits at and above R in the last word are 0; over the lines of a text object it is exactly the bitmap fsm_hip_text_hits_device
 *   takes.  pick[R], u64: the present records ascending in pick[0 .. P), the absent ones ascending in pick[P .. R); either half is a
 *   valid `pick` of every device front.  FSM_HIP_FIND_NO_PICK: no such array and no pass for it.  present = P.
 *   Limits.  R <= 2^32 - 2 (EOVERFLOW above).  No byte outside [bytes, bytes + min(off[R], nbytes)) of the probe is read, and none
 *   outside the same limit of the dictionary's source.  R == 0 and D == 0 launch nothing that reads a table: no record gives no
 *   array, no key gives every record absent.  The dictionary is const: it is bit for bit unchanged afterwards, and any number of
 *   lookups may read it at once on different streams.  No store leaves the found object's own arrays.
 * Passes.  hash: the distinct object's hash passes over the probe, with the dictionary's table size.  probe: a lane per record of at
 * most fsm_hip_distinct_long_bytes() bytes walks its chain -- an empty slot: absent; a slot with its hash tag: the lengths, the
 * tags, then the bytes of the two texts chunk by chunk, always: equal hashes decide nothing; equal: the slot's dense number -- and a
 * wavefront per longer record walks the chain as one, its lanes taking strided chunks of both keys, a ballot ending the comparison
 * at the first round of 64 chunks with a difference (under FSM_HIP_DISTINCT_WEAK_HASH no record is listed as long, as in the hash
 * pass: a lane takes any length).  The table and the numbers are read by agent-scope atomic loads; nothing is written to them and
 * there is no atomic read-modify-write.  mark: a wavefront's ballot is one bitmap word, one plain store; per block of records the
 * pair (present, absent) and the scan of the block pairs by one workgroup; P stays on the device.  pick: the block's own scan
 * redone.  Nothing waits: every array is sized by R, and everything may be in flight at return.
 * fsm_hip_keys_find_device takes device pointers on the dictionary's device, which must be current, and hip_stream; it works
 * behind the dictionary's last event.  fsm_hip_keys_find takes host arrays, stages them into the object, runs on a stream of its
 * own and waits; nbytes is off[R]; a decreasing off is EINVAL before any launch.  fsm_hip_keys_find_extracted looks up the records
 * of an extraction (trim: its separator), fsm_hip_keys_find_hits the lines of hits (trim: the text's delimiter; hits made with
 * FSM_HIP_HITS_NO_BYTES: EINVAL), fsm_hip_keys_find_text the n lines of a text object, its offsets and bytes as they stand (trim:
 * its delimiter): that bitmap goes straight into fsm_hip_text_hits_device on the same stream, with FSM_HIP_HITS_INVERT for -v.
 * Each is enqueued behind its object's last event.  The found object must be freed before the dictionary and before what it probed.
 * It owns, on the device: class[R] and the bitmap (NULL when R == 0) and pick[R] (NULL when R == 0 or under NO_PICK).  _records is
 * R; _present is P and waits for the object's last event.  _copy copies out whichever of class / bitmap / pick are not NULL and
 * waits (pick under NO_PICK: EINVAL).  _ms: all passes by HIP events; _pass_ms: 0 hash, 1 probe (both kernels), 2 mark + scan, 3
 * pick.  The getters of NULL give 0 or NULL, _copy of NULL is EINVAL, _free of NULL does nothing.
 * NULL + errno: ENODEV (checked first: there is no CPU path), EINVAL (a NULL object, d_off NULL, d_bytes NULL with nbytes > 0, a
 * trim byte outside -1 .. 255, an unknown flag bit, objects on different devices; host form: an off that decreases), EOVERFLOW
 * (R > 2^32 - 2), ENOMEM. */
#define FSM_HIP_FIND_NO_PICK 1u             /* no pick[R] and no pass for it */
#define FSM_HIP_FOUND_NONE   0xFFFFFFFFu    /* class of a record that equals no key */
struct fsm_hip_found;
struct fsm_hip_found *fsm_hip_keys_find_device(const struct fsm_hip_distinct *keys, const uint64_t *d_off, const void *d_bytes, size_t R,
	uint64_t nbytes, int trim_byte, const uint32_t *d_tag, unsigned flags, void *hip_stream);
struct fsm_hip_found *fsm_hip_keys_find(const struct fsm_hip_distinct *keys, const uint64_t *off, const void *bytes, size_t R, int trim_byte,
	const uint32_t *tag, unsigned flags);
struct fsm_hip_found *fsm_hip_keys_find_extracted(const struct fsm_hip_distinct *keys, const struct fsm_hip_extracted *x, unsigned flags,
	void *hip_stream);
struct fsm_hip_found *fsm_hip_keys_find_hits(const struct fsm_hip_distinct *keys, const struct fsm_hip_text_hits *hits, unsigned flags,
	void *hip_stream);
struct fsm_hip_found *fsm_hip_keys_find_text(const struct fsm_hip_distinct *keys, const struct fsm_hip_text *text, unsigned flags,
	void *hip_stream);
size_t fsm_hip_found_records(const struct fsm_hip_found *fx);                   /* R */
size_t fsm_hip_found_present(const struct fsm_hip_found *fx);                   /* P; waits for the last event */
const uint32_t *fsm_hip_found_class_device(const struct fsm_hip_found *fx);     /* R; NULL when R == 0 */
const uint64_t *fsm_hip_found_bitmap_device(const struct fsm_hip_found *fx);    /* ceil(R / 64); NULL when R == 0 */
const uint64_t *fsm_hip_found_pick_device(const struct fsm_hip_found *fx);      /* R; NULL when R == 0 or under NO_PICK */
int fsm_hip_found_copy(const struct fsm_hip_found *fx, uint32_t *cls, uint64_t *bitmap, uint64_t *pick);
double fsm_hip_found_ms(const struct fsm_hip_found *fx);
double fsm_hip_found_pass_ms(const struct fsm_hip_found *fx, int pass);         /* 0: hash, 1: probe, 2: mark + scan, 3: pick */
void fsm_hip_found_free(struct fsm_hip_found *fx);

/* ------------------------------------------------------------------ */
/* synthetic input generator (benchmarks and parity tests)            */
/* ------------------------------------------------------------------ */

/* Counter-based generator, identical on host and device:
 *   r(i, t)    = (mix64(seed ^ (i * 0x9E3779B97F4A7C15) ^ (t >> 3)) >> (8 * (t & 7))) & 0xff
 *   byte(i, t) = alphabet ? alphabet[r % nalpha] : r
 * with mix64 the splitmix64 finaliser and i the GLOBAL input index
 * (first_index + local row).  If plant_len > 0 (<= 64), every input with
 * i % plant_every == 0 has `plant` copied at offset
 * mix64(seed ^ i ^ 0xA5A5A5A5A5A5A5A5) % (stride - plant_len + 1).
 * d_base is a device pointer to n rows of `stride` bytes. */
int fsm_hip_gen_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *plant, unsigned plant_len, unsigned plant_every,
	void *hip_stream);

/* Lines out of rows, for the benchmarks of the variable-length fronts: input i = the first d_len[i] (<= max_len <= stride)
 * bytes of row i of d_rows, copied to d_out + d_off[i] (d_off[i] = sum of the lengths before i: the caller's prefix sum).
 * Device pointers, asynchronous on hip_stream. */
int fsm_hip_gen_pack_rows_device(const void *d_rows, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	size_t max_len, void *d_out, void *hip_stream);

/* Host twin of the generator (same bytes). */
void fsm_hip_gen_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *plant, unsigned plant_len, unsigned plant_every);

/* Affix variant for rx-style multi-pattern workloads: rows whose global index
 * is a multiple of `every` are  prefix + random bytes of `body` + suffix,
 * exactly stride bytes long (prefix = prefixes[h % npfx], suffix =
 * suffixes[(h>>32) % nsfx], h = mix64(seed ^ i ^ 0x5A5A5A5A5A5A5A5A)); every other
 * row is random over `alphabet` as above.  prefixes/suffixes are HOST arrays of
 * 8-byte entries [len<=7, b0..b6].  Synchronises the stream before returning. */
int fsm_hip_gen_affix_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every, void *hip_stream);

void fsm_hip_gen_affix_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every);

/* The same with an ALTERNATING body: positions after the prefix take bytes of `body` and `body2` in turn
 * (a transition-dense stream for patterns like ^ab([0-9][a-f])+(x|yz)$: every byte changes the state), and the
 * suffix is the first one, from the hashed choice on, that leaves a whole number of pairs.  nbody2 <= 64. */
int fsm_hip_gen_affix2_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *body2, unsigned nbody2,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every, void *hip_stream);

void fsm_hip_gen_affix2_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *body2, unsigned nbody2,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every);

/* ------------------------------------------------------------------ */
/* literal sets: the Aho-Corasick caller of the path                   */
/* ------------------------------------------------------------------ */

/* Word list -> DFA, in the shape of libre's re_strings interface
 * (include/re/strings.h:15-55, src/libre/re_strings.c:21-137, src/libre/ac.c): the same trie,
 * failure edges, output propagation and state numbering (depth-first from the root in byte
 * order, ac.c:277-346; state 0 is the shared absorbing end state when neither ANCHOR_RIGHT nor
 * AC_AUTOMATON is given, re_strings.c:105-117), so the description equals
 * fsm_hip_flatten(re_strings_build(...)) state for state -- but built iteratively, straight into
 * the flat form, without a struct fsm (the reference recurses once per trie level and keeps 2 KiB
 * per trie node).  add_* return 1 / 0 like re_strings_add_*; build returns a malloc'd description
 * (fsm_hip_desc_free) or NULL + errno.  The builder may be reused after build. */
enum {
	FSM_HIP_STRINGS_ANCHOR_LEFT  = 1 << 0,   /* RE_STRINGS_ANCHOR_LEFT  */
	FSM_HIP_STRINGS_ANCHOR_RIGHT = 1 << 1,   /* RE_STRINGS_ANCHOR_RIGHT */
	FSM_HIP_STRINGS_AC_AUTOMATON = 1 << 2    /* RE_STRINGS_AC_AUTOMATON */
};

struct fsm_hip_strings;   /* plays struct re_strings */

struct fsm_hip_strings *fsm_hip_strings_new(void);
void fsm_hip_strings_free(struct fsm_hip_strings *g);
int fsm_hip_strings_add_raw(struct fsm_hip_strings *g, const void *p, size_t n, const fsm_end_id_t *endid);
int fsm_hip_strings_add_str(struct fsm_hip_strings *g, const char *s, const fsm_end_id_t *endid);
struct fsm_hip_dfa_desc *fsm_hip_strings_build(struct fsm_hip_strings *g, unsigned flags);

/* re_strings() in one call (re_strings.c:21-52): NUL-terminated words, no end-ids. */
struct fsm_hip_dfa_desc *fsm_hip_strings(const char *const a[], size_t n, unsigned flags);

/* Library/ABI version: major*10000 + minor*100 + patch. */
int fsm_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FSM_HIP_H */
