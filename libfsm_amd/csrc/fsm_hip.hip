/*
 * fsm_hip.hip -- C ABI of libfsm_hip.so (core layer): table upload, kernel
 * selection/launch, host staging, end-id lookup, synthetic generator.
 * See include/fsm_hip.h for the contract of every entry point and the
 * reference interface (file:line) each one replaces.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cxxabi.h>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/fsm_hip.h"
#include "../../include/fsm_hip_plan.h"
#include "plan.h"
#include "image.h"
#include "dfa_access.h"
#include "launch.h"
#include "gen_kernels.h"
#include "walk_aux.h"
#include "walk_lazy.h"   /* FSMHIP_LAZY_PIECE (the kernels themselves are instantiated in kern_glob.hip) */
#include "trace_kernel.h"
#include "hip_host.h"

using namespace fsmhip;

/* ------------------------------------------------------------------ */

struct fsm_hip_dfa {
	Plan plan;
	int device = 0;
	int ncu = 256;
	uint32_t lds_limit = 160u * 1024u;
	DevBuf<unsigned char> d_tab;                     /* (its element type differs per layout: owned as bytes) */
	DevBuf<uint32_t> d_fin;
	DevBuf<uint32_t> d_btab;
	DevBuf<uint32_t> d_lazy;                         /* sparse layout: the lazy image (plan.cpp build_lazy), if the automaton has one */
	DevBuf<uint32_t> d_lazy_ctr;                     /* ... and a ring of tile counters: a launch zeroes and uses the next one (launches on
	                                                  * several streams may be in flight; LAZY_CTRS of them never are) */
	unsigned lazy_ctr_next = 0;
	int knob_lazy_lines = 1;                         /* the lazy walk also serves the variable-length fronts and resumed walks (0: walk_ragged / walk_generic over the records, for A/B runs) */
	int knob_lazy_dyn = 1;                           /* the lazy walk's wavefronts claim their tiles from a counter (0: static striding) */
	Image img;                                       /* what the layout's tables were uploaded from (image.h): built with the upload */
	/* device end-id delivery (built on first use) */
	DevBuf<uint32_t> d_fin_earliest, d_fin_ret;
	IdTables ids;                                    /* (its by-fin-index tables go once they are on the device) */
	bool ids_ready = false;
	/* resume tables (built on first use) */
	DevBuf<uint32_t> d_enc_of, d_orig_of;
	bool resume_ready = false;
	DevBuf<uint64_t> d_emask;                        /* eager-output masks, indexed like fin */
	DevBuf<uint32_t> d_ew_off, d_ew_word;            /* wide eager sets (> 64 ids) */
	DevBuf<uint64_t> d_ew_mask;
	/* the eager-output stream (trace_kernel.h; built on first use): plain renumbered table, byte classes, id lists (CSR), fin */
	DevBuf<uint32_t> d_tr_dense, d_tr_cls4, d_tr_eoff, d_tr_eids, d_tr_fin;
	bool trace_ready = false;
	/* device-side choice between walk_generic and walk_ragged: a ring of flags, one per launch (launches on several streams
	 * may be in flight; PICK_FLAGS of them never are), allocated with the dfa */
	DevBuf<uint32_t> d_pick;
	unsigned pick_next = 0;
	/* the lengths-only front: tile bases (u64 per 64 inputs) + block totals: one grow-only block per dfa.  Calls are enqueued
	 * under the dfa's lock; every call waits for the block's last user's event, so the block is never shared by two
	 * launches in flight (waiting on one's own stream costs nothing) */
	DevBuf<unsigned char> tb_scratch;
	size_t tb_scratch_bytes = 0;
	DevEvent tb_scratch_ev;
	bool tb_scratch_busy = false;
	std::vector<DevBuf<unsigned char>> tb_scratch_old;   /* outgrown blocks: they go with the dfa */
	DevBuf<unsigned char> arena;                     /* device scratch of the host-pointer front */
	size_t arena_bytes = 0;
	PinBuf<unsigned char> stage;                     /* pinned host staging for small calls */
	DevStream hs;                                    /* private stream of the host-pointer fronts */
	/* guards everything an exec call mutates: arena / stage, the timing events, the lazily built
	 * end-id and resume tables.  Host-pointer fronts hold it for the whole call (they share the
	 * arena), device-pointer fronts only while they enqueue. */
	std::recursive_mutex mu;
	WalkArgs proto;
	uint32_t table_lds = 0;      /* LDS bytes of the policy's tables */
	DevEvent ev0, ev1;
	bool timed = false;
	std::string last_kernel;     /* demangled name of the walk kernel of the last launch */
	std::string last_kernel_pick[3];   /* a device-side pick launched several (indexed by PICK_*): which one RAN is read from the flag on demand */
	const uint32_t *last_pick_flag = nullptr;
	/* tuning knobs (fsm_hip_dfa_tune) */
	int knob_input_mode = -1;    /* -1 auto */
	int knob_nb = 0;             /* 0 auto */
	int knob_seg = 0;            /* 0 auto (128) */
	int knob_prefetch = -1;      /* -1 auto (on) */
	int knob_nt = -1;            /* -1 auto */
	int knob_pack = -1;          /* walk_ldsdma_pack: -1 auto (with the per-lane load skip), 0 never, 1 wherever the kernel exists */
	int knob_rows = 0;           /* the lazy walk's inputs per lane; 0 auto */
	int knob_waves = 0;          /* 0 auto */
	int knob_blocks_per_cu = 0;  /* 0 auto */
	int knob_early = -1;         /* -1: from flags */
	int knob_noskip = 0;         /* 1: chunk skip off (measurement) */
	int knob_sparse_fast = 1;    /* sparse layout: entry-as-state walk (0: the id-as-state chain loop, for A/B runs) */
	bool sparse_fast_ok = true;  /* the record array sits inside one 4 GiB window (SparseFastPol::enter) */
	int knob_pick_mean = -1;     /* variable-length batches whose mean input length is below this many bytes go to a per-lane kernel;
	                              * -1: 128 where walk_lines32 is the per-lane kernel, 96 for walk_generic (pick_mean_of()) */
	unsigned flags = 0;
	/* The pair table (lds2) wins on fixed-stride rows but leaves no LDS for the ragged kernel's tiles: a dfa planned that way keeps a
	 * SECOND automaton image (lds / combself / ...) for its variable-length, unaligned and resumed batches */
	fsm_hip_dfa *alt = nullptr;
	std::atomic<const fsm_hip_dfa *> last_used{nullptr};   /* which of the two the last launch went to (timing / kernel name); written by concurrent callers */
	std::atomic<bool> uploaded{false};   /* the layout's tables are on the device (FSM_HIP_DEFER_UPLOAD: not before the first single-dfa call);
	                                      * release-stored under mu once everything is in place, acquire-loaded without it */
	int upload_errno = 0;        /* a failed upload is not retried: every later call fails with this */
	~fsm_hip_dfa() { fsm_hip_dfa_free(alt); }
};

/* GLOBAL layout: how much of the table head (rows nearest the start state) every workgroup
 * keeps in LDS.  The walk is bound by L2 gather requests and every lookup served from LDS is one
 * less: on a 6.7 MB table 0 / 40 / 80 / 120 KiB of hot rows measured 265 / 314 / 350 / 360 GB/s
 * (profiles/r01_c5_global_hot.txt), so the default takes what LDS offers. */
static uint32_t layout_lds_bytes(const fsm_hip_dfa *d, uint32_t tab_bytes);   /* (beside launch_layout()) */

static void set_hot_bytes(fsm_hip_dfa *d, uint32_t want)
{
	const Image &g = d->img;
	uint64_t hot = want;
	if (hot > g.glob_tab_bytes) hot = g.glob_tab_bytes;
	/* (the 4-byte table leaves room for eight wavefronts' LDS-DMA tiles; the 2-byte one is walked with per-lane loads and takes
	 * all of LDS: every row there is a step that stays out of L2) */
	const uint32_t keep = g.glob16 ? 64u : 8u * 4096u;
	if (hot + lds_bytes_btab() + keep > d->lds_limit) hot = d->lds_limit - lds_bytes_btab() - keep;
	hot -= hot % g.glob_row_bytes;
	/* never less than one row: a lane whose row is beyond the head still issues its LDS read, at offset 0 of the head
	 * (GlobPol::next, Glob16Pol::next / next2), and with no head at all that address is the first byte PAST what the
	 * per-lane kernels allocate (lds_bytes(0), no tiles behind it) */
	if (hot < g.glob_row_bytes) hot = g.glob_row_bytes < g.glob_tab_bytes ? g.glob_row_bytes : g.glob_tab_bytes;
	d->proto.tab_bytes = (uint32_t)hot;
	d->table_lds = layout_lds_bytes(d, (uint32_t)hot);
}

static const unsigned LAZY_CTRS = 64, PICK_FLAGS = 64;

typedef std::lock_guard<std::recursive_mutex> DfaLock;

/* the automaton image a batch goes to: the second one (fsm_hip_dfa::alt) for everything the fixed-stride kernels do not take */
static const fsm_hip_dfa *route(const fsm_hip_dfa *d, bool fixed_stride_fast)
{
	const fsm_hip_dfa *t = d->alt != nullptr && !fixed_stride_fast ? d->alt : d;
	const_cast<fsm_hip_dfa *>(d)->last_used.store(t, std::memory_order_relaxed);
	return t;
}

extern "C" int fsm_hip_version(void) { return 210; }

/* for multi.hip (dfa_access.h): the host-side plan and the device of a dfa */
namespace fsmhip {
const Plan *dfa_plan(const fsm_hip_dfa *d) { return &d->plan; }
int dfa_device(const fsm_hip_dfa *d) { return d->device; }
int dfa_ncu(const fsm_hip_dfa *d) { return d->ncu; }
}

/* ------------------------------------------------------------------ */
/* create / free / info                                               */
/* ------------------------------------------------------------------ */

/* the layout's device image + the per-dfa launch resources (events, private stream).  fsm_hip_dfa_create does this at once
 * unless FSM_HIP_DEFER_UPLOAD asks to wait for the first call that needs it: a dfa that is only ever used through
 * fsm_hip_exec_multi (retest: a new DFA per record, a few lines each) never needs it -- its plain table rides in that call's
 * one host-to-device copy */
static int dfa_upload_all(fsm_hip_dfa *d)
{
	const Plan &p = d->plan;
	Image &im = d->img;
	WalkArgs &a = d->proto;
	/* 1. the image: everything that needs no device (image.cpp) */
	const int r = build_image(p, im);
	if (r != 0) { errno = r; return -1; }
	/* 2. its parts go to the device and the prototype points at them */
	memset(&a, 0, sizeof a);
	if (!HIP_OK(d->d_tab.upload_bytes(im.tab, im.tab_size, im.tab_elem))) return -1;
	if (!HIP_OK(d->d_fin.upload(*im.fin))) return -1;
	if (!HIP_OK(d->d_btab.upload(im.btab))) return -1;
	a.tab = d->d_tab;
	a.fin = d->d_fin;
	a.btab = d->d_btab;
	if (!im.emask.empty()) {
		if (!HIP_OK(d->d_emask.upload(im.emask))) return -1;
		a.emask = d->d_emask;
	}
	if (!im.ew_off.empty()) {
		if (!HIP_OK(d->d_ew_off.upload(im.ew_off))) return -1;
		if (!HIP_OK(d->d_ew_word.upload(im.ew_word))) return -1;
		if (!HIP_OK(d->d_ew_mask.upload(im.ew_mask))) return -1;
		a.ew_off = d->d_ew_off;
		a.ew_word = d->d_ew_word;
		a.ew_mask = d->d_ew_mask;
	}
	a.tab_bytes = im.s.tab_bytes;
	a.start = im.s.start;
	a.abs_min = im.s.abs_min;
	a.fin_div = im.s.fin_div;
	a.fin_mul = im.s.fin_mul;
	a.dflt = im.s.dflt;
	a.ident_class = im.s.ident_class;
	a.eager_lo_end = im.s.eager_lo_end;
	a.eager_hi_begin = im.s.eager_hi_begin;
	a.eager_words = im.s.eager_words;
	im.drop_upload_parts();
	/* 3. what the device decides */
	if (p.layout == FSM_HIP_LAYOUT_GLOBAL) set_hot_bytes(d, im.glob16 ? 160u * 1024u : 120u * 1024u);
	else d->table_lds = layout_lds_bytes(d, a.tab_bytes);
	if (p.layout == FSM_HIP_LAYOUT_SPARSE) {
		/* SparseFastPol::enter builds a record's address from a 32-bit low half: the record array must not cross
		 * a 4 GiB boundary (hipMalloc hands out 2 MiB-aligned blocks, the array is a few MB: practically never) */
		const uint64_t g = reinterpret_cast<uint64_t>(d->d_tab.p) + p.sparse_img[5], bytes = (uint64_t)p.S1 * 16u;
		if ((g >> 32) != ((g + bytes) >> 32)) d->sparse_fast_ok = false;
		if (p.lazy_lds_bytes != 0 && ((p.lazy_lds_bytes + 15u) & ~15u) + FSMHIP_LAZY_QBYTES <= d->lds_limit) {
			if (!HIP_OK(d->d_lazy.upload(p.lazy_img))) return -1;
			if (!HIP_OK(d->d_lazy_ctr.alloc(LAZY_CTRS))) return -1;
			a.lazy = d->d_lazy;
			/* the default where it pays: few states beyond the LDS set whose own record sends hits the exact way
			 * (img[10]) or that carry nothing (img[9]) -- on the 1e5-literal automaton 4.5 % of them, deep in the trie */
			const uint64_t deep = p.abs_min > p.lazy_img[1] ? p.abs_min - p.lazy_img[1] : 0;
			if (((uint64_t)p.lazy_img[9] + p.lazy_img[10]) * 10u <= deep) d->knob_sparse_fast = 3;
		}
	}
	/* bit 0: a wavefront retires once all its lanes are absorbing; bit 1: an absorbing lane stops fetching its row (what
	 * fsm_exec does at a missing edge, exec.c:133-138).  Bit 1 costs a ballot per tile: set only where an absorbing
	 * state can be reached at all (launch_walk clears it again for the eager and the resumed walks) */
	a.early = (d->flags & FSM_HIP_NO_EARLY_RETIRE) ? 0u : p.abs_reachable ? 3u : 1u;
	if (!HIP_OK(d->d_pick.alloc(PICK_FLAGS))) return -1;
	if (!HIP_OK(d->tb_scratch_ev.create(hipEventDisableTiming))) return -1;
	if (!HIP_OK(d->ev0.create())) return -1;
	if (!HIP_OK(d->ev1.create())) return -1;
	if (!HIP_OK(d->hs.create(hipStreamNonBlocking))) return -1;
	d->uploaded.store(true, std::memory_order_release);
	return 0;
}

static int dfa_upload(fsm_hip_dfa *d)
{
	if (dfa_upload_all(d) == 0) return 0;
	d->upload_errno = errno != 0 ? errno : EIO;
	return -1;
}

static int ensure_uploaded(const fsm_hip_dfa *cd)
{
	if (cd->uploaded.load(std::memory_order_acquire)) return 0;
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(cd);
	DfaLock lk(d->mu);
	if (d->uploaded.load(std::memory_order_relaxed)) return 0;
	if (d->upload_errno != 0) { errno = d->upload_errno; return -1; }
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	return dfa_upload(d);
}

/* a handle that goes, when its creation fails, without touching that failure's errno */
struct __attribute__((visibility("hidden"))) DfaDrop { void operator()(fsm_hip_dfa *d) const { const int e = errno; fsm_hip_dfa_free(d); errno = e; } };

extern "C" struct fsm_hip_dfa *fsm_hip_dfa_create(const struct fsm_hip_dfa_desc *desc, unsigned flags)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		errno = ENODEV; /* no CPU fallback by design */
		return nullptr;
	}
	std::unique_ptr<fsm_hip_dfa, DfaDrop> d(new (std::nothrow) fsm_hip_dfa());
	if (d == nullptr) { errno = ENOMEM; return nullptr; }
	d->flags = flags;
	{
		int v = 0;
		if (!HIP_OK(hipGetDevice(&d->device))) return nullptr;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d->device) == hipSuccess && v > 0) d->ncu = v;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, d->device) == hipSuccess && v > 0) d->lds_limit = (uint32_t)v;
		if (d->lds_limit > 160u * 1024u) d->lds_limit = 160u * 1024u;
	}
	{
		int r = build_plan(desc, flags, d->lds_limit, d->plan);
		if (r != 0) { errno = r; return nullptr; }
	}
	if (!(flags & FSM_HIP_DEFER_UPLOAD) && dfa_upload(d.get()) != 0) return nullptr;
	if (d->plan.layout == FSM_HIP_LAYOUT_LDS2 && (flags & FSM_HIP_LAYOUT_MASK) == FSM_HIP_LAYOUT_AUTO && !(flags & FSM_HIP_PLAN_NO_LDS2)) {
		/* fewer than eight ragged wavefronts fit beside the pair table: the variable-length fronts get a table of their own */
		const uint32_t pair_lds = Lds2Pol::lds_bytes((uint32_t)(d->plan.lds_tab.size() * 2));
		if (pair_lds + 8u * FSMHIP_RAGGED_WAVE_LDS > d->lds_limit) {
			d->alt = fsm_hip_dfa_create(desc, flags | FSM_HIP_PLAN_NO_LDS2);
			if (d->alt == nullptr) return nullptr;
		}
	}
	return d.release();
}

/* everything the handle holds goes with it (the second image first: ~fsm_hip_dfa) */
extern "C" void fsm_hip_dfa_free(struct fsm_hip_dfa *d)
{
	if (d == nullptr) return;
	delete d;
}

/* ------------------------------------------------------------------ */
/* launch                                                             */
/* ------------------------------------------------------------------ */

/* Where the per-lane kernels hand over to walk_ragged (mean input length, bytes).  walk_generic: 96 (round 3).  walk_lines32 is
 * faster than that kernel and still wins at a mean of 96 (64-128 byte lines: 2.40 vs 1.86 TB/s on the column table, 2.35 vs 1.40
 * on the C3 table), walk_ragged from ~160 on (64-256 bytes: 1.81 vs 2.69, 1.86 vs 2.09): 128 (profiles/r08r_*). */
static int pick_mean_of(const fsm_hip_dfa *d, bool lines32)
{
	return d->knob_pick_mean >= 0 ? d->knob_pick_mean : lines32 ? 128 : 96;
}

/* per_lane: take walk_generic unless a knob says otherwise -- the inputs average < 96 bytes (walk_ragged works in
 * 128-byte segments: 0.7-1.2 vs 1.5-2.1 TB/s at 8-64 bytes, profiles/r03t_*); huge: the batch may hold an input the
 * ragged kernel's 32-bit piece count cannot (>= 2^36 bytes) */
static LaunchCfg pick_cfg(const fsm_hip_dfa *d, bool fast_ok, uint64_t stride, int eager, bool per_lane = false, bool huge = false, bool resumed = false, bool many = false)
{
	LaunchCfg c = LaunchCfg();    /* kfn = nullptr until a launch sets it */
	const uint32_t layout = d->plan.layout;
	c.nb = 8;
	c.seg = 128;
	/* every input line is consumed by exactly one DMA instruction (SEG = 128): nontemporal loads
	 * measured +7.5 % on the HBM-bound tiny layout (profiles/r01_sweep8*), neutral elsewhere */
	c.nt = d->knob_nt >= 0 ? (d->knob_nt != 0) : 1;
	/* CombSelfPol's branchy chain is latency-bound: drop the register double-buffer (<= 64 VGPRs)
	 * so two 16-wave workgroups share a CU (profiles/r01_sweep5*: 4.52 vs 4.32 TB/s) */
	c.prefetch = d->knob_prefetch >= 0 ? (d->knob_prefetch != 0) : (layout == FSM_HIP_LAYOUT_COMBSELF || layout == FSM_HIP_LAYOUT_SPARSE ? 0 : 1);
	/* ragged / packed / unaligned inputs: the coalesced, lane-refilling kernel whenever at least four
	 * waves' tiles and rings fit next to the table, else per-lane loads (walk_generic) */
	/* the 5-bit column table keeps the ragged kernel's ring and row records in its own holes (walk_kernels.h ragged_aux_in_holes) */
	const bool ragged_holes = layout == FSM_HIP_LAYOUT_TINY && !d->plan.tiny5_col.empty() && !eager;
	const uint32_t ragged_wave_lds = ragged_holes ? 8192u : FSMHIP_RAGGED_WAVE_LDS;
	const bool ragged_fits = d->table_lds + 4u * ragged_wave_lds <= d->lds_limit;
	int mode = ragged_fits && !per_lane && !huge ? IN_RAGGED : IN_GENERIC;
	if (d->knob_input_mode == IN_GENERIC || (d->knob_input_mode == IN_RAGGED && ragged_fits && !huge)) mode = d->knob_input_mode;
	else if (fast_ok) {
		/* measured (profiles/r01_sweep*.txt): LDS-DMA staging (8 KiB tile per wave) is the better input
		 * path whenever at least 12 waves of tiles fit next to the table (lds layout 5.1 vs 4.8 TB/s;
		 * combself, once whole self-loop chunks are skipped, 6.1 vs 5.0 TB/s: profiles/r01_sweep11*);
		 * per-lane loads with 8 chunks in flight next to a bigger LDS table */
		const bool dma_fits = d->table_lds + 12u * 8192u <= d->lds_limit;
		int m = (layout == FSM_HIP_LAYOUT_TINY || dma_fits) ? IN_LDSDMA : IN_DIRECT;
		if (d->knob_input_mode == IN_DIRECT || d->knob_input_mode == IN_LDSDMA) m = d->knob_input_mode;
		if (m == IN_LDSDMA && stride % 64u != 0) m = IN_DIRECT;
		if (m == IN_LDSDMA) {
			c.seg = d->knob_seg == 64 ? 64 : 128;
			if (stride % 128u != 0) c.seg = 64;
			/* the eager kernels exist for 128-byte segments and register-held sets only (2.3 vs 1.1 TB/s for
			 * those; wide sets measured 1.8 behind LDS-DMA vs 2.1 with per-lane loads in round 2 and 2.53 vs 2.71 in round 3:
			 * profiles/r04x_eager_wide_dma.txt) */
			if (eager && (c.seg != 128 || eager == 2)) m = IN_DIRECT;
		}
		if (m == IN_DIRECT) {
			/* the sparse layout waits on gathers, not on its input: 4 chunks keep it under 64 VGPRs;
			 * the eager kernel is instantiated for 4 chunks only */
			c.nb = d->knob_nb == 4 || d->knob_nb == 8 ? d->knob_nb : (layout == FSM_HIP_LAYOUT_SPARSE || d->img.glob16 ? 4 : 8);   /* (the 2-byte global table: 4 chunks x TWO inputs per lane, kern_glob16.hip) */
			if (eager || !c.prefetch) c.nb = 4;
			if ((stride / 16u) % 8u != 0) c.nb = 4;
			if ((stride / 16u) % 4u != 0) m = -1;   /* rows shorter than / not a multiple of 64 bytes */
		}
		if (m >= 0) mode = m;
	}
	c.sparse_fast = d->sparse_fast_ok ? d->knob_sparse_fast : (d->knob_sparse_fast == 3 ? 3 : 0);
	c.lazy_abs = 0;
	if (mode == IN_DIRECT && layout == FSM_HIP_LAYOUT_SPARSE && !eager && !resumed && d->d_lazy != nullptr && d->knob_sparse_fast == 3 &&
	    (stride / 16u) % 4u == 0) {
		/* the lazy walk: one 16-wave workgroup per CU beside its 131 KiB of tables, three inputs per lane (walk_lazy.h) */
		c.mode = IN_LAZY;
		c.nt = d->knob_nt > 0;      /* nontemporal input loads: A/B knob (FSM_HIP_KNOB_NT) */
		c.lazy_abs = d->plan.lazy_img[11] != 0;
		/* inputs per lane x chunks in flight: 3 x 4 (kern_glob.hip: 1 036 GB/s on the 1e5-literal automaton; 2 x 4: 1 000, 3 x 2: 970,
		 * 4 x 2: 758 -- profiles/r09j_*); FSM_HIP_KNOB_ROWS = 2: round 5's shape (A/B) */
		c.lazy_rows = d->knob_rows == 2 ? 2 : 3;
		c.nb = 4;
		c.waves = 16;
		c.lds = d->plan.lazy_lds_bytes;
		c.blocks_per_cu = d->knob_blocks_per_cu > 0 ? d->knob_blocks_per_cu : 1;
		return c;
	}
	if (layout == FSM_HIP_LAYOUT_SPARSE && !eager && d->d_lazy != nullptr && d->knob_sparse_fast == 3 && d->knob_input_mode < 0 && d->knob_lazy_lines && !many) {   /* (many: 2^32 inputs or more -- its queue entries hold 32-bit indexes) */
		/* ... and on everything else such an automaton is asked (round 5): inputs of any length and metadata form, strides that
		 * are not a multiple of 64, unaligned rows, resumed walks -- one input per lane slot with lane refill (walk_lazy_lines) */
		c.mode = IN_LAZY_LINES;
		c.lazy_abs = d->plan.lazy_img[11] != 0 || resumed;   /* a resumed input may start in DEAD */
		/* THREE slots per lane, three whole chunks per slot and turn (kern_glob.hip has the numbers).  FSM_HIP_KNOB_ROWS = 2 brings the
		 * two-slot forms back (FSM_HIP_KNOB_NB = 2 / 4 chunks), FSM_HIP_KNOB_NB = 2 / 4 at three slots the two- and four-chunk turns: A/B */
		c.lazy_rows = d->knob_rows == 2 ? 2 : 3;
		c.nb = c.lazy_rows == 3 ? (d->knob_nb == 2 || d->knob_nb == 4 ? d->knob_nb : 3) : d->knob_nb == 2 ? 2 : 4;
		c.waves = 16;
		/* the table + the wavefronts' queues: all the LDS there is (plan.cpp leaves at least FSMHIP_LAZY_QBYTES: 112 entries per
		 * wavefront; the kernel uses up to 128) */
		c.lds = ((d->plan.lazy_lds_bytes + 15u) & ~15u) + 16u * 128u * 16u;
		if (c.lds > d->lds_limit) c.lds = d->lds_limit;
		c.blocks_per_cu = d->knob_blocks_per_cu > 0 ? d->knob_blocks_per_cu : 1;
		return c;
	}
	if (c.sparse_fast == 3) c.sparse_fast = d->sparse_fast_ok ? 1 : 0;
	/* a staging path asked for by knob beside a table that leaves no LDS for one wavefront's tile (the 2-byte global table takes
	 * all of it): the per-lane kernel of the same class of input */
	if ((mode == IN_LDSDMA && d->table_lds + 64u * (uint32_t)c.seg > d->lds_limit) || (mode == IN_RAGGED && d->table_lds + ragged_wave_lds > d->lds_limit)) {
		mode = mode == IN_LDSDMA ? IN_DIRECT : IN_GENERIC;
		if (mode == IN_DIRECT) {
			c.nb = d->knob_nb == 8 && (stride / 16u) % 8u == 0 ? 8 : 4;
			if ((stride / 16u) % 4u != 0) mode = IN_GENERIC;
		}
	}
	c.mode = mode;
	/* the packing LDS-DMA walk exists for plain walks from the start state, 128-byte segments, rows of two segments and more, 32-bit
	 * row indexes; launch_walk drops it again where the per-lane load skip is off (FSM_HIP_KNOB_PACK = -1) */
	c.pack = mode == IN_LDSDMA && c.seg == 128 && !eager && !resumed && stride >= 256u && !many && d->knob_pack != 0;
	const uint32_t per_wave = mode == IN_LDSDMA ? 64u * (uint32_t)c.seg : mode == IN_RAGGED ? ragged_wave_lds : 0u;
	/* waves per block: as many behind one table copy as LDS holds, 16 at most: the tiny layouts keep a
	 * 64 KiB column table (one private copy per lane / bank), which leaves 12 x 8 KiB tiles of the 160 KiB.
	 * combself behind LDS-DMA: 12 waves measured best at 10^8 x 1 KiB (6.09 TB/s; 14: 5.82, 10: 5.80, 8: 5.72).
	 * Kernels compiled for fewer threads (their register budget): ragged 12 waves, eager LDS-DMA on the 64-bit column
	 * table 12 (launch.h eager_dma_threads), eager ragged / generic 8. */
	int wmax = 16;
	if (mode == IN_RAGGED) wmax = eager ? 8 : ragged_holes ? (int)FSMHIP_RAGGED_HOLE_WAVES : 12;
	else if (eager && mode == IN_GENERIC) wmax = 8;
	else if (eager && mode == IN_LDSDMA) wmax = ((layout == FSM_HIP_LAYOUT_TINY && d->plan.tiny5_col.empty()) || layout == FSM_HIP_LAYOUT_COMB ||
		                                            layout == FSM_HIP_LAYOUT_COMBSELF || layout == FSM_HIP_LAYOUT_LDSSELF) ? 12 : 16;   /* launch.h eager_dma_threads */
	else if (layout == FSM_HIP_LAYOUT_COMBSELF && mode == IN_LDSDMA) wmax = 12;
	else if (layout == FSM_HIP_LAYOUT_SPARSE && c.pack) wmax = 12;   /* launch.h ldsdma_pack_threads */
	/* the plain row table behind LDS-DMA: its walk keeps the LDS array ~85 % busy (two reads per byte, the table read
	 * replayed for bank conflicts: profiles/r04f_pmc_eager_lds.txt); 14 waves measured 4.24 / 4.01 TB/s where 16 gave
	 * 3.77 / 3.71 and 12 4.01 / 3.99 (354- and 1132-state tables, 8e6 x 1 KiB: profiles/r04h_eager_probe_8M.txt).  The
	 * eager form of the same walk wants 16 (3.53 vs 3.33 at 14, 3.12 at 12). */
	else if (layout == FSM_HIP_LAYOUT_LDS && mode == IN_LDSDMA && !eager) wmax = 14;
	/* short inputs on the column tables: 12-wave workgroups (two per CU) measured 2.29 / 1.61 / 2.52 TB/s at 8-64 / 8-16 /
	 * 32-128 bytes where 16 gave 2.05 / 1.32 / 2.26 (6e6 packed inputs, profiles/r04t_generic_waves.txt); the other
	 * layouts keep 16 (combself: 1.47 vs 1.25) */
	else if (layout == FSM_HIP_LAYOUT_TINY && mode == IN_GENERIC && !eager) wmax = 12;
	int waves = d->knob_waves > 0 && d->knob_waves < wmax ? d->knob_waves : wmax;
	if (!eager && mode != IN_RAGGED && d->knob_waves > wmax && d->knob_waves <= 16 &&
	    !(layout == FSM_HIP_LAYOUT_COMBSELF && mode == IN_LDSDMA) && !(layout == FSM_HIP_LAYOUT_SPARSE && c.pack)) waves = d->knob_waves;   /* those kernels are compiled for 12 */
	while (waves > 1 && d->table_lds + (uint32_t)waves * per_wave > d->lds_limit) waves -= (waves > 8 && mode != IN_RAGGED ? 2 : 1);
	c.waves = waves;
	c.lds = d->table_lds + (uint32_t)waves * per_wave;
	int bpc = (int)(d->lds_limit / (c.lds ? c.lds : 1u));
	if (bpc * waves > 32) bpc = 32 / waves;
	if (bpc < 1) bpc = 1;
	/* twice the resident workgroups: the tail of the persistent grid balances better (the ragged kernel
	 * partitions statically: one range per resident wave) */
	if (mode == IN_DIRECT || mode == IN_LDSDMA) bpc *= 2;
	if (d->knob_blocks_per_cu > 0) bpc = d->knob_blocks_per_cu;
	c.blocks_per_cu = bpc;
	return c;
}

/* what a front knows about its batch beyond the arguments (host fronts: everything; device fronts: nothing) */
struct BatchHint {
	uint64_t bytes = 0;        /* total input bytes, 0 = unknown */
	bool short_mean = false;   /* the inputs average < 96 bytes */
};

static hipError_t launch_layout(const fsm_hip_dfa *d, int eager, const LaunchCfg &c, const WalkArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
	const Plan &p = d->plan;
	switch (p.layout) {
	case FSM_HIP_LAYOUT_TINY:     return launch_tiny(p.tiny5_col.empty() ? POL_TINY64 : POL_TINY5, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_LDS:      return launch_lds(POL_LDS, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_LDSSELF:  return launch_lds(POL_LDSSELF, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_LDS2:     return launch_lds(POL_LDS2, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_COMB:     return launch_comb(POL_COMB, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_COMB256:  return launch_comb(POL_COMB256, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_COMBSELF: return launch_comb(POL_COMBSELF, eager, c, a, grid, block, s);
	case FSM_HIP_LAYOUT_SPARSE:   return launch_glob(POL_SPARSE, eager, c, a, grid, block, s);
	default:                      return d->img.glob16 ? launch_glob16(eager, c, a, grid, block, s) : launch_glob(POL_GLOB, eager, c, a, grid, block, s);
	}
}

/* LDS bytes of the layout's tables, as its policy counts them (tab_bytes: WalkArgs::tab_bytes) */
static uint32_t layout_lds_bytes(const fsm_hip_dfa *d, uint32_t tab_bytes)
{
	const Plan &p = d->plan;
	switch (p.layout) {
	case FSM_HIP_LAYOUT_TINY:     return p.tiny5_col.empty() ? TinyPol<uint64_t>::lds_bytes(tab_bytes) : Tiny5Pol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_LDS:      return LdsPol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_LDSSELF:  return LdsSelfPol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_LDS2:     return Lds2Pol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_COMB:     return CombPol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_COMB256:  return Comb256Pol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_COMBSELF: return CombSelfPol::lds_bytes(tab_bytes);
	case FSM_HIP_LAYOUT_SPARSE:   return SparsePol::lds_bytes(tab_bytes);
	default:                      return d->img.glob16 ? Glob16Pol::lds_bytes(tab_bytes) : GlobPol::lds_bytes(tab_bytes);
	}
}

/* FSM_HIP_DEBUG=2: synchronise after every stage of a launch and say which one it was (a GPU fault aborts the process) */
/* the launched kernel's own name, as the profiler shows it */
static std::string kernel_name(const void *kfn, hipStream_t s)
{
	if (kfn == nullptr) return "?";
	/* resolved once per kernel: the lookup + demangling is ~10 us, a small batch's walk is 20 */
	static std::mutex cache_mu;
	static std::vector<std::pair<const void *, std::string>> cache;
	{
		std::lock_guard<std::mutex> lk(cache_mu);
		for (const auto &e : cache) if (e.first == kfn) return e.second;
	}
	const char *m = hipKernelNameRefByPtr(kfn, s);
	if (m == nullptr) return "?";
	int st = 0;
	char *dm = abi::__cxa_demangle(m, nullptr, nullptr, &st);
	std::string r = st == 0 && dm != nullptr ? dm : m;
	free(dm);
	const size_t p = r.find("(fsmhip::WalkArgs");
	if (p != std::string::npos) r.resize(p);
	if (r.compare(0, 5, "void ") == 0) r.erase(0, 5);
	std::lock_guard<std::mutex> lk(cache_mu);
	cache.emplace_back(kfn, r);
	return r;
}

/* vector registers of a kernel (cached per kernel: the query is a driver call) */
static int kernel_vgprs(const void *kfn)
{
	if (kfn == nullptr) return 0;
	static std::mutex cache_mu;
	static std::vector<std::pair<const void *, int>> cache;
	{
		std::lock_guard<std::mutex> lk(cache_mu);
		for (const auto &e : cache) if (e.first == kfn) return e.second;
	}
	hipFuncAttributes at;
	if (hipFuncGetAttributes(&at, kfn) != hipSuccess) {   /* (not remembered: asked again at the next launch) */
		(void)hipGetLastError();
		return 0;
	}
	std::lock_guard<std::mutex> lk(cache_mu);
	cache.emplace_back(kfn, at.numRegs);
	return at.numRegs;
}

/* The per-lane kernels on an LDS table are bound by latency (a tile's chunks are asked for and waited for at once): what
 * counts is how many wavefronts a CU holds.  The table's LDS allows `by_lds` workgroups per CU; a SIMD holds 512 / registers
 * wavefronts (8 at most), a workgroup of W wavefronts puts ceil(W / 4) on each.  walk_lines32<CombSelfPol> (76 registers: 6 per
 * SIMD): one 16-wavefront workgroup fits (4 per SIMD), or TWO of 12 (6 per SIMD) -- 24000000 lines of 8-64 bytes on the C3 table:
 * 0.485 -> 0.418 ms, 8-16 bytes 0.294 -> 0.234 (profiles/r08d_lines32_waves.txt).  Returns the workgroup size (wavefronts)
 * that keeps most wavefronts resident, the larger one on a tie. */
static int waves_by_occupancy(int vgprs, int by_lds, int wmax)
{
	if (vgprs <= 0) return wmax;
	const int alloc = (vgprs + 7) / 8 * 8;
	int per_simd = 512 / alloc;
	if (per_simd > 8) per_simd = 8;
	int best = wmax, best_res = 0;
	for (int w = wmax; w >= 8; w -= 4) {
		const int each = (w + 3) / 4;
		int blocks = per_simd / each;
		if (blocks > by_lds) blocks = by_lds;
		if (blocks * w > 32) blocks = 32 / w;
		if (blocks * w > best_res) { best_res = blocks * w; best = w; }
	}
	return best;
}

extern "C" int fsm_hip_waves_by_occupancy(int vgprs, int workgroups_by_lds, int max_waves)
{
	if (max_waves < 8) return max_waves;
	return waves_by_occupancy(vgprs, workgroups_by_lds < 1 ? 1 : workgroups_by_lds, max_waves > 16 ? 16 : max_waves);
}

static void debug_stage(hipStream_t s, const char *what)
{
	static const int lvl = getenv("FSM_HIP_DEBUG") ? atoi(getenv("FSM_HIP_DEBUG")) : 0;
	if (lvl < 2) return;
	fprintf(stderr, "fsm_hip: %s ...", what);
	fflush(stderr);
	const hipError_t e = hipStreamSynchronize(s);
	fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
	fflush(stderr);
}

static int launch_walk(const fsm_hip_dfa *d, WalkArgs a, bool fast_ok, hipStream_t s, const BatchHint &hint = BatchHint())
{
	if (a.n == 0) return 0;
	const int eager = a.eager_out == nullptr ? 0 : a.eager_words > 1 ? 2 : 1;
	/* the kernel family: a resumed eager walk (state_io + eager_out) has instantiations of its own (launch.h: 3 / 4); the
	 * choice of kernel is the eager walk's */
	const int keager = eager != 0 && a.state_io != nullptr ? eager + 2 : eager;
	const bool varlen = a.off != nullptr || a.off32 != nullptr || a.len != nullptr;
	const uint64_t known_bytes = hint.bytes != 0 ? hint.bytes : !varlen ? (uint64_t)a.n * a.stride : 0;
	LaunchCfg c = pick_cfg(d, fast_ok, a.stride, eager, hint.short_mean, known_bytes >= ((uint64_t)1 << 36), a.state_io != nullptr, a.n >= ((uint64_t)1 << 32));
	const uint64_t ntiles = (a.n + 63u) / 64u;
	const uint64_t lazy_tile = 64u * (uint64_t)(c.lazy_rows > 0 ? c.lazy_rows : 2);      /* inputs per wavefront of the fixed-stride lazy walk */
	uint64_t nblocks = c.mode == IN_LAZY ? ((a.n + lazy_tile - 1u) / lazy_tile + c.waves - 1) / c.waves
		: c.mode == IN_LAZY_LINES ? ((a.n + FSMHIP_LAZY_PIECE - 1u) / FSMHIP_LAZY_PIECE + c.waves - 1) / c.waves : (ntiles + c.waves - 1) / c.waves;
	const uint64_t cap = (uint64_t)d->ncu * c.blocks_per_cu;
	if (nblocks > cap) nblocks = cap;
	/* bit 0 wave retire, bit 1 per-lane load skip: the knob decides, else the dfa's own default -- without bit 1 for the eager and
	 * the resumed walks, which report more than an end state: tests/test_gpu_eager_front.py judges their id sets / carried states on
	 * every layout and input path (bit 1 off, as here); nothing has run it with bit 1 on yet */
	if (d->knob_early >= 0) a.early = (uint32_t)d->knob_early;
	else if (eager != 0 || a.state_io != nullptr) a.early &= ~2u;
	if (d->knob_noskip > 0) a.early |= 4u;
	if (!(a.early & 2u) && d->knob_pack < 1) c.pack = 0;   /* (bit 1 already says that an absorbing state can be reached) */

	/* Variable-length inputs (the retest / rx front).  Short ones (mean < 96 bytes) walk fastest one per lane with per-lane
	 * loads (walk_generic; a plain walk of a packed batch below 4 GiB: its 32-bit form walk_lines32), long ones in 128-byte
	 * segments with lane refill (walk_ragged).  A host-pointer front knows the mean and the size; a device-pointer front cannot
	 * know them without a synchronising copy, so the candidates are ALL launched and a small kernel decides on the device
	 * which of them runs (offsets_pick, walk_aux.h); the others return at once. */
	const bool pick_len = varlen && known_bytes == 0 && !hint.short_mean && d->knob_input_mode < 0 && c.mode == IN_RAGGED;
	/* the 32-bit lines kernel: plain outputs, a packed front, < 2^29 inputs; the batch's size: known (1 / 0) or not (-1) */
	const bool lines_cand = !eager && a.out2 == nullptr && a.state_io == nullptr && (a.off != nullptr || a.off32 != nullptr || a.tbase != nullptr) &&
		a.n < 0x1FFFFFF0ull && !(a.early & 32u) && (c.mode == IN_GENERIC || pick_len);
	int fits32 = !lines_cand ? 0 : a.off32 != nullptr ? 1 : known_bytes != 0 ? (known_bytes < ((uint64_t)1 << 32) ? 1 : 0) : -1;
	bool skip_generic = false;
	if (fits32 < 0 && pick_len) {
		/* a device front with u64 offsets / lengths alone: the batch's size is on the device -- but it should not end beyond the
		 * ALLOCATION its base points into.  Fewer than 4 GiB from the base to the allocation's end (every batch but a huge one in
		 * a huge block): walk_generic's own body is not needed and is not launched.  The reported range is a HINT, not a proof
		 * (memory mapped in pieces may report one piece): fits32 stays "unknown", offsets_pick still looks at the batch's last
		 * offset, and is told that walk_generic was not launched (cand bit 2 clear) -- a batch of 4 GiB and more then goes to
		 * walk_ragged, which is launched and takes any batch; where walk_ragged is no candidate walk_generic is always launched.
		 * (Not asked during a stream capture: the query is not a stream operation, and an API that is not may end a capture.) */
		hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
		if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
			hipDeviceptr_t ab = nullptr;
			size_t asz = 0;
			if (hipMemGetAddressRange(&ab, &asz, (hipDeviceptr_t)const_cast<uint8_t *>(a.base)) == hipSuccess && ab != nullptr) {
				const uint64_t room = reinterpret_cast<uint64_t>(ab) + asz - reinterpret_cast<uint64_t>(a.base);
				if (room < ((uint64_t)1 << 32)) skip_generic = true;
			} else (void)hipGetLastError();
		} else (void)hipGetLastError();
	}
	const bool pick = pick_len || fits32 < 0;

	fsm_hip_dfa *md = const_cast<fsm_hip_dfa *>(d);
	DfaLock lk(md->mu);   /* the timing events, the flag ring and the tile-base block are per dfa */
	hipError_t e = hipSuccess;
	/* the ragged kernel sets bitmap bits one input at a time, the packing LDS-DMA walk ORs in the words of its packed tiles */
	if ((c.mode == IN_RAGGED || c.mode == IN_LAZY_LINES || c.pack) && a.bitmap != nullptr) e = zero_async(a.bitmap, ntiles * sizeof(uint64_t), s);
	if (e == hipSuccess && ((c.mode == IN_LAZY && d->knob_lazy_dyn) || c.mode == IN_LAZY_LINES) && d->d_lazy_ctr != nullptr) {
		a.tile_ctr = d->d_lazy_ctr + (md->lazy_ctr_next++ % LAZY_CTRS);
		e = zero_async(a.tile_ctr, sizeof(uint32_t), s);
	}
	if (e == hipSuccess) e = hipEventRecord(md->ev0, s);
	md->last_pick_flag = nullptr;
	for (auto &nm : md->last_kernel_pick) nm.clear();
	if (e == hipSuccess && pick) {
		a.pick_flag = md->d_pick + (md->pick_next++ % PICK_FLAGS);
		a.skip_flag = a.pick_flag;
		/* bit 0: walk_ragged is a candidate (else every batch counts as short); bit 1: so is walk_lines32 */
		hipLaunchKernelGGL(offsets_pick, dim3(1), dim3(256), 0, s, a, (uint32_t)pick_mean_of(d, false), (uint32_t)pick_mean_of(d, true),
		                   (pick_len ? 1u : 0u) | (fits32 != 0 ? 2u : 0u) | (fits32 != 1 && !skip_generic ? 4u : 0u));
		e = hipGetLastError();
	}
	/* the per-lane kernels (short inputs): walk_generic unless the batch is known to fit 32 bits, walk_lines32 unless known not to */
	const bool per_lane = c.mode == IN_GENERIC || pick_len;
	if (e == hipSuccess && per_lane) {
		const LaunchCfg g0 = c.mode == IN_GENERIC ? c : pick_cfg(d, false, a.stride, eager, true, false);
		for (int w32 = 0; w32 < 2 && e == hipSuccess; w32++) {
			if (w32 ? fits32 == 0 : (fits32 == 1 || skip_generic)) continue;
			WalkArgs ag = a;
			ag.run_when = w32 ? PICK_LINES32 : PICK_GENERIC;
			LaunchCfg g = g0;
			g.lines32 = w32;
			/* the workgroup size that keeps most wavefronts on a CU, from the kernel's own register count (LDS tables, plain walks,
			 * no knob) */
			if (!eager && d->knob_waves <= 0 && d->knob_blocks_per_cu <= 0 && d->table_lds != 0 && d->plan.layout != FSM_HIP_LAYOUT_TINY) {
				g.probe = 1;
				g.kfn = nullptr;
				if (launch_layout(d, keager, g, ag, dim3(1), dim3(64), s) == hipSuccess && g.kfn != nullptr) {
					const int by_lds = (int)(d->lds_limit / d->table_lds);
					g.waves = waves_by_occupancy(kernel_vgprs(g.kfn), by_lds < 1 ? 1 : by_lds, g0.waves);
					int bpc = by_lds < 1 ? 1 : by_lds;
					if (bpc * g.waves > 32) bpc = 32 / g.waves;
					g.blocks_per_cu = bpc < 1 ? 1 : bpc;
				}
				g.probe = 0;
			}
			const uint64_t gb0 = (ntiles + g.waves - 1) / g.waves, gcap = (uint64_t)d->ncu * g.blocks_per_cu;
			const dim3 ggrid((unsigned)(gb0 < gcap ? gb0 : gcap)), gblock((unsigned)g.waves * 64u);
			g.kfn = nullptr;
			e = launch_layout(d, keager, g, ag, ggrid, gblock, s);
			if (e == hipSuccess) {
				md->last_kernel = kernel_name(g.kfn, s);
				md->last_kernel_pick[ag.run_when] = md->last_kernel;
			}
		}
		debug_stage(s, "walk (per-lane)");
	}
	if (e == hipSuccess && c.mode != IN_GENERIC) {
		a.run_when = PICK_RAGGED;
		c.kfn = nullptr;
		e = launch_layout(d, keager, c, a, dim3((unsigned)nblocks), dim3((unsigned)c.waves * 64u), s);
		if (e == hipSuccess) {
			md->last_kernel = kernel_name(c.kfn, s);
			md->last_kernel_pick[PICK_RAGGED] = md->last_kernel;
		}
		debug_stage(s, "walk");
	}
	if (e == hipSuccess && pick) {   /* several were launched, one ran: fsm_hip_last_kernel_name() asks the flag which */
		md->last_pick_flag = a.pick_flag;
		std::string all;
		for (const auto &nm : md->last_kernel_pick) if (!nm.empty()) all += (all.empty() ? "" : " | ") + nm;
		md->last_kernel = all;
	}
	if (e == hipSuccess) e = hipEventRecord(md->ev1, s);
	if (e != hipSuccess) {
		if (getenv("FSM_HIP_DEBUG")) fprintf(stderr, "fsm_hip: launch -> %s\n", hipGetErrorString(e));
		errno = hip_errno(e);
		return -1;
	}
	md->timed = true;
	return 0;
}

/* The lengths-only front: byte offset of every 64th input of a batch packed back to back (walk_aux.h tile_bases_*), into the
 * dfa's grow-only block; the walk that follows on the same stream reads it.  The block's previous user (any stream) is
 * waited for first; `tbase` = the array the walk kernels take (T + 1 entries, the last one the batch's size). */
static int ensure_ids(fsm_hip_dfa *d);
static int ensure_resume(fsm_hip_dfa *d);

static size_t tb_bytes_for(size_t n)
{
	const uint64_t T1 = (n + 63u) / 64u + 1u, nb = (T1 + 1023u) / 1024u;
	return (size_t)(T1 + nb) * sizeof(uint64_t);
}

/* (grows by doubling: a handful of blocking hipMalloc calls over a dfa's life; launches in flight may still use the old block) */
static hipError_t tb_grow(fsm_hip_dfa *d, size_t want)
{
	if (want <= d->tb_scratch_bytes) return hipSuccess;
	if (d->tb_scratch) d->tb_scratch_old.push_back(std::move(d->tb_scratch));
	d->tb_scratch_bytes = 0;
	size_t cap = (size_t)1 << 16;
	while (cap < want) cap *= 2;
	const hipError_t e = d->tb_scratch.alloc(cap);
	if (e == hipSuccess) d->tb_scratch_bytes = cap;
	return e;
}

/* Everything a later call on batches of up to n inputs would allocate, now: the tile-base block of the lengths-only front
 * (the layout's tables too, for a dfa created with FSM_HIP_DEFER_UPLOAD).  After it the device-pointer fronts make no
 * allocation for such batches and can be captured into a HIP graph from the first launch. */
extern "C" int fsm_hip_reserve(struct fsm_hip_dfa *d, size_t n)
{
	if (d == nullptr) { errno = EINVAL; return -1; }
	if (ensure_uploaded(d) != 0) return -1;
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (d->alt != nullptr && fsm_hip_reserve(d->alt, n) != 0) return -1;   /* the variable-length fronts run on the second image */
	DfaLock lk(d->mu);
	const hipError_t e = tb_grow(d, tb_bytes_for(n));
	if (e != hipSuccess) { errno = hip_errno(e); return -1; }
	/* ... and the tables the end-id and resume fronts build at their first call */
	(void)ensure_ids(d);
	(void)ensure_resume(d);
	errno = 0;
	return 0;
}

static int tile_bases(fsm_hip_dfa *d, const uint32_t *d_len, size_t n, hipStream_t s, const uint64_t **tbase)
{
	DfaLock lk(d->mu);
	const uint64_t T1 = (n + 63u) / 64u + 1u, nb = (T1 + 1023u) / 1024u;
	const size_t want = tb_bytes_for(n);
	hipError_t e = hipSuccess;
	if (d->tb_scratch_busy) e = hipStreamWaitEvent(s, d->tb_scratch_ev, 0);
	if (e == hipSuccess && want > d->tb_scratch_bytes) {
		/* a blocking hipMalloc: illegal while the stream is being captured into a graph -- fsm_hip_reserve() sizes the block ahead */
		hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
		if (s != nullptr && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
			if (getenv("FSM_HIP_DEBUG")) fprintf(stderr, "fsm_hip: the lengths front needs %zu bytes of scratch during a stream capture: call fsm_hip_reserve() first\n", want);
			errno = ENOMEM;
			return -1;
		}
		e = tb_grow(d, want);
	}
	if (e == hipSuccess) {
		uint64_t *tb = reinterpret_cast<uint64_t *>(d->tb_scratch.p), *bt = tb + T1;
		hipLaunchKernelGGL(tile_bases_pass1, dim3((unsigned)nb), dim3(1024), 0, s, d_len, (uint64_t)n, T1, tb, bt);
		hipLaunchKernelGGL(tile_bases_pass2, dim3(1), dim3(1024), 0, s, bt, nb);
		uint64_t g3 = (T1 + 255u) / 256u;
		if (g3 > (uint64_t)d->ncu * 8u) g3 = (uint64_t)d->ncu * 8u;
		hipLaunchKernelGGL(tile_bases_pass3, dim3((unsigned)g3), dim3(256), 0, s, tb, T1, (const uint64_t *)bt);
		e = hipGetLastError();
		*tbase = tb;
	}
	if (e != hipSuccess) { errno = hip_errno(e); return -1; }
	return 0;
}

/* ... and once the walk is enqueued: the block is busy until this point of the stream */
static void tile_bases_done(fsm_hip_dfa *d, hipStream_t s)
{
	DfaLock lk(d->mu);
	if (hipEventRecord(d->tb_scratch_ev, s) == hipSuccess) d->tb_scratch_busy = true;
}

/* ------------------------------------------------------------------ */
/* the two fronts of the walk: a batch is described once              */
/* ------------------------------------------------------------------ */

/* Where a batch's inputs are (device pointers for walk_device, host pointers for walk_host).  The two builders are the only
 * writers, so at most one of len / off / off32 is set: offsets win over lengths, u64 offsets over u32 offsets. */
struct Inputs {
	const void *base;
	size_t stride;           /* rows: bytes between inputs (0: packed, or empty inputs) */
	const uint32_t *len;     /* rows: per-row lengths or NULL (= stride); lens_only: the packed inputs' lengths */
	const uint64_t *off;     /* packed: n+1 offsets */
	const uint32_t *off32;   /* packed, below 4 GiB: n+1 offsets */
	bool lens_only;          /* packed back to back, located by their lengths alone */
	size_t n;

	/* rows of `stride` bytes (whole, or with per-row lengths), or packed inputs where u64 offsets are given */
	static Inputs rows_or_offsets(const void *base, size_t stride, const uint32_t *len, const uint64_t *off, size_t n)
	{
		if (off != nullptr) return Inputs{ base, 0, nullptr, off, nullptr, false, n };
		return Inputs{ base, stride, len, nullptr, nullptr, false, n };
	}
	/* packed inputs whose metadata is u64 offsets, u32 offsets or lengths alone (FSM_HIP_META_*); false: no such form, or no metadata */
	static bool packed_by(int meta_form, const void *base, const void *meta, size_t n, Inputs *in)
	{
		if (n != 0 && meta == nullptr) return false;
		*in = Inputs{ base, 0, nullptr, nullptr, nullptr, false, n };
		switch (meta_form) {
		case FSM_HIP_META_OFF64:   in->off = static_cast<const uint64_t *>(meta); return true;
		case FSM_HIP_META_OFF32:   in->off32 = static_cast<const uint32_t *>(meta); return true;
		case FSM_HIP_META_LENGTHS: in->len = static_cast<const uint32_t *>(meta); in->lens_only = true; return true;
		default:                   return false;
		}
	}
	bool packed() const { return off != nullptr || off32 != nullptr || lens_only; }
	/* whole rows, stride and base 16-byte aligned: what the fixed-stride kernels take (an automaton tuned to IN_GENERIC still
	 * declines: that term is applied where launch_walk is called) */
	bool fixed_fast() const
	{
		return !packed() && len == nullptr && stride != 0 && stride % 16u == 0 && (reinterpret_cast<uintptr_t>(base) % 16u) == 0;
	}
	void fill(WalkArgs &a) const
	{
		a.base = static_cast<const uint8_t *>(base);
		a.stride = stride;
		a.len = len;
		a.off = off;
		a.off32 = off32;
		a.n = n;
	}
};

/* What the caller wants back, whichever are asked for: the walk kernels write all of them in one pass */
struct Outputs {
	uint32_t *end_out = nullptr;
	uint64_t *bitmap = nullptr;
	int ids_mode = 0;               /* FSM_HIP_IDS_*, read where id_out is set */
	uint32_t *id_out = nullptr;     /* device-side end-ids */
	uint64_t *eager_out = nullptr;  /* eager sets, written */
	uint32_t *state_io = nullptr;   /* resume: the state to start from, the state reached */
	uint64_t *eager_io = nullptr;   /* resume: eager sets carried across pieces (OR-ed into, never cleared) */

	static Outputs ends(uint32_t *end_out, uint64_t *bitmap)
	{
		Outputs o;
		o.end_out = end_out;
		o.bitmap = bitmap;
		return o;
	}
};

/* Where the entry points differ without their batch or their outputs saying so.  Each of these is how the fronts behaved
 * while they were separate functions; none has been decided on its merits yet. */
struct FrontTraits {
	/* an empty batch (n == 0): GOES_ON to the device (guard, upload of a FSM_HIP_DEFER_UPLOAD automaton, end-id tables) and
	 * leaves it to launch_walk; RETURNS 0 before anything is touched or routed; RETURNS_AFTER_IDS: routed, ids_mode checked and
	 * the end-id tables built first */
	enum Empty { GOES_ON, RETURNS, RETURNS_AFTER_IDS } empty;
	/* fsm_hip_exec_batch_eager{,_offsets}{,_device}: an automaton with eager ids walks on its own image whatever the batch's
	 * form (route() is not asked, where FRONT_ALL asks it for the same batch); one without eager ids zeroes the sets and is the
	 * plain front from there on, an empty batch included.  (Not asking route() cannot be observed today: only the pair table
	 * keeps a second image, and the planner gives no automaton with eager ids the pair table -- plan.cpp emit_lds2.) */
	bool eager_front;
	/* host pointers, packed inputs: the mean length is held against pick_mean_of(d, true) where walk_lines32 is the per-lane
	 * kernel (128, not 96) */
	bool lines32_mean;
	/* an ids_mode that does not exist is refused after route(), not with the other arguments before it: the refused call
	 * has then moved fsm_hip_last_kernel_name() to the image the batch would have gone to */
	bool ids_mode_after_route;
};
static const FrontTraits
	FRONT_ROWS   = { FrontTraits::GOES_ON, false, true, false },            /* fsm_hip_exec_batch{,_device} */
	FRONT_PACKED = { FrontTraits::RETURNS, false, true, false },            /* ..._offsets, _offsets32, _lengths {,_device} */
	FRONT_IDS    = { FrontTraits::GOES_ON, false, false, false },           /* ..._ids{,_offsets}{,_device} */
	FRONT_RESUME = { FrontTraits::RETURNS, false, false, false },           /* ..._resume*, _eager_resume {,_device} */
	FRONT_EAGER  = { FrontTraits::GOES_ON, true, false, false },            /* ..._eager{,_offsets}{,_device} */
	FRONT_ALL    = { FrontTraits::RETURNS_AFTER_IDS, false, false, true };  /* ..._all_device, _packed_all{,_device} */

/* The device-pointer front of every walk: one batch, every output asked for, one launch_walk */
static int walk_device(const fsm_hip_dfa *dc, const Inputs &in, Outputs out, void *hip_stream, const BatchHint &hint, const FrontTraits &tr)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(dc);
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	const bool no_such_mode = out.id_out != nullptr && out.ids_mode != FSM_HIP_IDS_EARLIEST && out.ids_mode != FSM_HIP_IDS_RET && out.ids_mode != FSM_HIP_IDS_ERROR;
	if (d == nullptr || (in.n != 0 && !in.packed() && in.base == nullptr && in.stride != 0) || (no_such_mode && !tr.ids_mode_after_route)) {
		errno = EINVAL;
		return -1;
	}
	if (in.n == 0 && tr.empty == FrontTraits::RETURNS) return 0;
	if (tr.eager_front && d->plan.emask.empty()) {
		/* no state emits anything: the answer is all zeros, the walk is the plain one */
		DevGuard dg(d->device);
		if (!dg.ok()) { errno = ENODEV; return -1; }
		const hipError_t e = zero_async(out.eager_out, in.n * sizeof(uint64_t), s);
		if (e != hipSuccess) { errno = hip_errno(e); return -1; }
		out.eager_out = nullptr;
		return walk_device(d, in, out, hip_stream, hint, in.off != nullptr ? FRONT_PACKED : FRONT_ROWS);
	}
	if (!tr.eager_front) {
		/* (a resumed walk never takes the fixed-stride kernels of the pair table) */
		const fsm_hip_dfa *t = route(d, out.state_io == nullptr && in.fixed_fast());
		if (t != d) return walk_device(t, in, out, hip_stream, hint, tr);
	}
	if (out.id_out != nullptr) {
		if (no_such_mode) { errno = EINVAL; return -1; }
		if (ensure_ids(d) != 0) return -1;
		if (out.ids_mode == FSM_HIP_IDS_ERROR) {
			/* AMBIG_ERROR: an end state with more than one id is refused (print/c.c:67-72 fails the
			 * print with EINVAL); without such a state it is AMBIG_EARLIEST */
			if (d->ids.conflict != FSM_HIP_NO_MATCH) { errno = EINVAL; return -1; }
			out.ids_mode = FSM_HIP_IDS_EARLIEST;
		}
	}
	if (in.n == 0 && tr.empty == FrontTraits::RETURNS_AFTER_IDS) return 0;
	if (out.state_io != nullptr && ensure_resume(d) != 0) return -1;
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (ensure_uploaded(d) != 0) return -1;
	WalkArgs a = d->proto;
	in.fill(a);
	a.end_out = out.end_out;
	a.bitmap = out.bitmap;
	if (out.id_out != nullptr) {
		a.fin2 = out.ids_mode == FSM_HIP_IDS_EARLIEST ? d->d_fin_earliest : d->d_fin_ret;
		a.out2 = out.id_out;
	}
	if (out.state_io != nullptr) {
		a.state_io = out.state_io;
		a.enc_of = d->d_enc_of;
		a.orig_of = d->d_orig_of;
		a.nstates = d->plan.nstates;
		/* where no state emits, the plain resumed walk leaves the carried sets as they are */
		if (!d->plan.emask.empty()) a.eager_out = out.eager_io;
	} else if (out.eager_out != nullptr) {
		if (d->plan.emask.empty() || d->plan.eager_words > 1) {
			/* no state emits anything: all zeros; wide sets are OR-ed in place by the kernel: start from zero */
			const size_t w = d->plan.emask.empty() ? 1 : d->plan.eager_words;
			const hipError_t e = zero_async(out.eager_out, in.n * w * sizeof(uint64_t), s);
			if (e != hipSuccess) { errno = hip_errno(e); return -1; }
		}
		if (!d->plan.emask.empty()) a.eager_out = out.eager_out;
	}
	/* The lengths-only form: ONE critical section over the pre-pass, the walk and the "block busy until here" event: another
	 * host thread's call on this dfa must not refill the tile-base block between them (the mutex is recursive: the three take
	 * it again) */
	std::unique_lock<std::recursive_mutex> lk(d->mu, std::defer_lock);
	if (in.lens_only) {
		lk.lock();
		if (tile_bases(d, in.len, in.n, s, &a.tbase) != 0) return -1;
	}
	const int r = launch_walk(d, a, in.fixed_fast() && d->knob_input_mode != IN_GENERIC, s, hint);
	if (in.lens_only) tile_bases_done(d, s);
	return r;
}

extern "C" int fsm_hip_exec_batch_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, nullptr, n), Outputs::ends(d_end_out, d_accept_bitmap), hip_stream, BatchHint(), FRONT_ROWS);
}

/* inputs packed back to back, located by u64 offsets, u32 offsets, or their lengths alone */
extern "C" int fsm_hip_exec_batch_offsets_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_OFF64, d_base, d_off, n, &in)) { errno = EINVAL; return -1; }
	return walk_device(d, in, Outputs::ends(d_end_out, d_accept_bitmap), hip_stream, BatchHint(), FRONT_PACKED);
}

extern "C" int fsm_hip_exec_batch_offsets32_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint32_t *d_off32, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_OFF32, d_base, d_off32, n, &in)) { errno = EINVAL; return -1; }
	return walk_device(d, in, Outputs::ends(d_end_out, d_accept_bitmap), hip_stream, BatchHint(), FRONT_PACKED);
}

extern "C" int fsm_hip_exec_batch_lengths_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_LENGTHS, d_base, d_len, n, &in)) { errno = EINVAL; return -1; }
	return walk_device(d, in, Outputs::ends(d_end_out, d_accept_bitmap), hip_stream, BatchHint(), FRONT_PACKED);
}

extern "C" const char *fsm_hip_last_kernel_name(const struct fsm_hip_dfa *d)
{
	if (d == nullptr) return "";
	if (const fsm_hip_dfa *lu = d->last_used.load(std::memory_order_relaxed); lu != nullptr && lu != d) return fsm_hip_last_kernel_name(lu);   /* the launch went to the second image */
	fsm_hip_dfa *md = const_cast<fsm_hip_dfa *>(d);
	DfaLock lk(md->mu);
	if (md->last_pick_flag != nullptr) {
		/* a device-pointer variable-length call: the choice between the two kernels was made on the device (offsets_pick): read it
		 * back (a 4-byte copy; waits for the launch) and name the kernel that walked the batch, as rocprofv3 would show it busy */
		uint32_t flag = 3;
		DevGuard dg(d->device);
		if (dg.ok() && md->timed && hipEventSynchronize(md->ev1) == hipSuccess &&
		    hipMemcpy(&flag, md->last_pick_flag, sizeof flag, hipMemcpyDeviceToHost) == hipSuccess && flag <= 2u && !md->last_kernel_pick[flag].empty()) {
			int cands = 0;
			for (const auto &nm : md->last_kernel_pick) cands += nm.empty() ? 0 : 1;
			md->last_kernel = md->last_kernel_pick[flag];
			md->last_kernel += flag == PICK_RAGGED ? " (decided on the device" : flag == PICK_LINES32 ? " (picked on the device: short lines, a batch below 4 GiB"
			                                                                  : " (mean length below the pick threshold, decided on the device";
			md->last_kernel += cands == 2 ? ", 1 of 2 launched)" : cands == 3 ? ", 1 of 3 launched)" : ")";
		}
		md->last_pick_flag = nullptr;
	}
	return d->last_kernel.c_str();
}

extern "C" double fsm_hip_last_kernel_ms(const struct fsm_hip_dfa *d)
{
	if (d == nullptr) return -1.0;
	if (const fsm_hip_dfa *lu = d->last_used.load(std::memory_order_relaxed); lu != nullptr && lu != d) return fsm_hip_last_kernel_ms(lu);
	DfaLock lk(const_cast<fsm_hip_dfa *>(d)->mu);
	if (!d->timed) return -1.0;
	float ms = 0.f;
	if (hipEventSynchronize(d->ev1) != hipSuccess) return -1.0;
	if (hipEventElapsedTime(&ms, d->ev0, d->ev1) != hipSuccess) return -1.0;
	return (double)ms;
}

/* ------------------------------------------------------------------ */
/* host-buffer front: stage through HBM                                */
/* ------------------------------------------------------------------ */

/*
 * Host-pointer fronts.  One device arena per dfa (grow-only up to ARENA_KEEP, so repeated calls --
 * retest / re(1) issue one per input line -- allocate and release nothing), laid out
 *     [inputs ...] [in/out arrays ...] [outputs ...]
 * Small calls gather their host arrays in one pinned buffer: one H2D copy (inputs + in/out), the
 * kernel, one D2H copy (in/out + outputs), one stream synchronise.  Large calls copy each array
 * straight from / to the caller's pages.
 */
static const size_t ARENA_KEEP = (size_t)256 << 20, STAGE_BYTES = (size_t)1 << 20;

static size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }

struct HostCall {
	enum Kind { IN = 0, INOUT = 1, OUT = 2 };
	struct Part { const void *src; void *dst; size_t bytes, pad, off; int kind; };
	fsm_hip_dfa *d;
	DfaLock lk;       /* arena and staging buffer are shared by the calls on one dfa */
	Part parts[8];
	int np = 0;
	unsigned char *arena = nullptr;
	DevBuf<unsigned char> temp;     /* a call beyond ARENA_KEEP: its own arena, gone with the call */
	bool small = false;
	size_t h2d_end = 0, d2h_begin = 0, total = 0;

	explicit HostCall(const fsm_hip_dfa *cd) : d(const_cast<fsm_hip_dfa *>(cd)), lk(d->mu) {}
	/* declare the arrays in the order IN..., INOUT..., OUT...; returns the part's index (or -1 for a NULL array) */
	int add(int kind, const void *src, void *dst, size_t bytes, size_t pad = 0)
	{
		if (kind != IN && dst == nullptr) return -1;
		if (kind == IN && src == nullptr && bytes != 0) return -1;
		Part &p = parts[np];
		p.src = src; p.dst = dst; p.bytes = bytes; p.pad = pad; p.kind = kind; p.off = 0;
		return np++;
	}
	template <class T> T *dev(int part) const { return part < 0 ? nullptr : reinterpret_cast<T *>(arena + parts[part].off); }

	int begin()
	{
		if (ensure_uploaded(d) != 0) return -1;   /* FSM_HIP_DEFER_UPLOAD: the private stream and the tables come with the first call */
		size_t o = 0;
		h2d_end = 0;
		d2h_begin = (size_t)-1;
		for (int i = 0; i < np; i++) {   /* declared in the order IN, INOUT, OUT */
			Part &p = parts[i];
			p.off = o;
			o += up256(p.bytes + p.pad);
			if (p.kind != OUT) h2d_end = o;
			if (p.kind != IN && d2h_begin == (size_t)-1) d2h_begin = p.off;
		}
		total = o;
		if (d2h_begin == (size_t)-1) d2h_begin = total;
		if (total <= d->arena_bytes) {
			arena = d->arena;
		} else if (total <= ARENA_KEEP) {
			d->arena.reset();
			d->arena_bytes = 0;
			size_t want = (size_t)2 << 20;
			while (want < total) want *= 2;
			if (!HIP_OK(d->arena.alloc(want))) return -1;
			d->arena_bytes = want;
			arena = d->arena;
		} else {
			if (!HIP_OK(temp.alloc(total))) return -1;
			arena = temp;
		}
		small = total <= STAGE_BYTES;
		if (small && d->stage == nullptr && !HIP_OK(d->stage.alloc(STAGE_BYTES))) return -1;
		if (small) {
			for (int i = 0; i < np; i++)
				if (parts[i].kind != OUT && parts[i].bytes) memcpy(d->stage + parts[i].off, parts[i].src, parts[i].bytes);
			if (h2d_end && !HIP_OK(hipMemcpyAsync(arena, d->stage, h2d_end, hipMemcpyHostToDevice, d->hs))) return -1;
		} else {
			for (int i = 0; i < np; i++)
				if (parts[i].kind != OUT && parts[i].bytes &&
				    !HIP_OK(hipMemcpyAsync(arena + parts[i].off, parts[i].src, parts[i].bytes, hipMemcpyHostToDevice, d->hs))) return -1;
		}
		return 0;
	}

	int end()
	{
		if (small) {
			if (total > d2h_begin && !HIP_OK(hipMemcpyAsync(d->stage + d2h_begin, arena + d2h_begin, total - d2h_begin, hipMemcpyDeviceToHost, d->hs))) return -1;
			if (!HIP_OK(hipStreamSynchronize(d->hs))) return -1;
			for (int i = 0; i < np; i++)
				if (parts[i].kind != IN && parts[i].bytes) memcpy(parts[i].dst, d->stage + parts[i].off, parts[i].bytes);
		} else {
			for (int i = 0; i < np; i++)
				if (parts[i].kind != IN && parts[i].bytes &&
				    !HIP_OK(hipMemcpyAsync(parts[i].dst, arena + parts[i].off, parts[i].bytes, hipMemcpyDeviceToHost, d->hs))) return -1;
			if (!HIP_OK(hipStreamSynchronize(d->hs))) return -1;
		}
		return 0;
	}
};

/* A host batch's metadata is checked before anything is staged: offsets non-decreasing, len[i] <= stride, base == NULL only
 * for a batch without bytes.  *in_bytes: what is staged; *payload: the bytes the inputs themselves hold (rows with lengths:
 * their sum, not the rows they sit in) */
static int check_host_inputs(const Inputs &in, size_t *in_bytes, uint64_t *payload)
{
	const size_t n = in.n;
	uint64_t sum = 0;
	if (!in.packed()) {
		if (n != 0 && in.base == nullptr && in.stride != 0) return -1;
		if (in.len != nullptr)
			for (size_t i = 0; i < n; i++) {
				if (in.len[i] > in.stride) return -1;
				sum += in.len[i];
			}
		*in_bytes = n * in.stride;
		*payload = in.len != nullptr ? sum : (uint64_t)*in_bytes;
		return 0;
	}
	if (in.off != nullptr) {
		for (size_t i = 0; i < n; i++)
			if (in.off[i + 1] < in.off[i]) return -1;
		sum = n ? in.off[n] : 0;
	} else if (in.off32 != nullptr) {
		for (size_t i = 0; i < n; i++)
			if (in.off32[i + 1] < in.off32[i]) return -1;
		sum = n ? in.off32[n] : 0;
	} else {
		for (size_t i = 0; i < n; i++) sum += in.len[i];
	}
	if (sum != 0 && in.base == nullptr) return -1;
	*in_bytes = (size_t)sum;
	*payload = sum;
	return 0;
}

/* what a host front knows about its batch (launch_walk picks the kernel from it): the size, and whether the inputs are short
 * on average -- asked of variable-length batches only */
static BatchHint host_hint(const fsm_hip_dfa *d, const Inputs &in, size_t in_bytes, uint64_t payload, const FrontTraits &tr)
{
	BatchHint hint;
	hint.bytes = in_bytes;
	if (in.packed() || in.len != nullptr) {
		/* a plain walk of packed lines: walk_lines32 is the per-lane kernel (below 4 GiB and 2^29 lines, not the record walk) */
		const bool l32 = tr.lines32_mean && in.packed() && in_bytes < ((uint64_t)1 << 32) && in.n < 0x1FFFFFF0ull && d->plan.layout != FSM_HIP_LAYOUT_SPARSE;
		hint.short_mean = payload / in.n < (uint64_t)pick_mean_of(d, l32);
	}
	return hint;
}

/* The host-pointer front of every walk: stage the batch, walk_device on the private stream, bring the outputs back */
static int walk_host(const fsm_hip_dfa *dc, const Inputs &in, const Outputs &out, const FrontTraits &tr)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(dc);
	const size_t n = in.n;
	size_t in_bytes = 0;
	uint64_t payload = 0;
	if (d == nullptr || check_host_inputs(in, &in_bytes, &payload) != 0) { errno = EINVAL; return -1; }
	if (n == 0) return 0;
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	HostCall hc(d);
	const size_t sets = n * fsm_hip_eager_words(d) * sizeof(uint64_t);
	/* +32: the generic kernel reads whole aligned 16-byte chunks */
	const int p_in = hc.add(HostCall::IN, in.base, nullptr, in_bytes, 32);
	const int p_len = in.len ? hc.add(HostCall::IN, in.len, nullptr, n * sizeof(uint32_t)) : -1;
	const int p_off = in.off ? hc.add(HostCall::IN, in.off, nullptr, (n + 1) * sizeof(uint64_t)) : -1;
	const int p_off32 = in.off32 ? hc.add(HostCall::IN, in.off32, nullptr, (n + 1) * sizeof(uint32_t)) : -1;
	const int p_st = hc.add(HostCall::INOUT, out.state_io, out.state_io, n * sizeof(uint32_t));
	const int p_eio = hc.add(HostCall::INOUT, out.eager_io, out.eager_io, sets);
	const int p_end = hc.add(HostCall::OUT, nullptr, out.end_out, n * sizeof(uint32_t));
	const int p_bm = hc.add(HostCall::OUT, nullptr, out.bitmap, ((n + 63) / 64) * sizeof(uint64_t));
	const int p_id = hc.add(HostCall::OUT, nullptr, out.id_out, n * sizeof(uint32_t));
	const int p_eo = hc.add(HostCall::OUT, nullptr, out.eager_out, sets);
	if (hc.begin() != 0) return -1;
	Inputs din = in;
	din.base = hc.dev<unsigned char>(p_in);
	din.len = hc.dev<uint32_t>(p_len);
	din.off = hc.dev<uint64_t>(p_off);
	din.off32 = hc.dev<uint32_t>(p_off32);
	Outputs dout = out;
	dout.state_io = hc.dev<uint32_t>(p_st);
	dout.eager_io = hc.dev<uint64_t>(p_eio);
	dout.end_out = hc.dev<uint32_t>(p_end);
	dout.bitmap = hc.dev<uint64_t>(p_bm);
	dout.id_out = hc.dev<uint32_t>(p_id);
	dout.eager_out = hc.dev<uint64_t>(p_eo);
	if (walk_device(d, din, dout, d->hs, host_hint(d, in, in_bytes, payload, tr), tr) != 0) return -1;
	return hc.end();
}

extern "C" int fsm_hip_exec_batch(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap)
{
	return walk_host(d, Inputs::rows_or_offsets(base, stride, len, nullptr, n), Outputs::ends(end_out, accept_bitmap), FRONT_ROWS);
}

extern "C" int fsm_hip_exec_batch_offsets(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_OFF64, base, off, n, &in)) { errno = EINVAL; return -1; }
	return walk_host(d, in, Outputs::ends(end_out, accept_bitmap), FRONT_PACKED);
}

extern "C" int fsm_hip_exec_batch_offsets32(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint32_t *off32, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_OFF32, base, off32, n, &in)) { errno = EINVAL; return -1; }
	return walk_host(d, in, Outputs::ends(end_out, accept_bitmap), FRONT_PACKED);
}

extern "C" int fsm_hip_exec_batch_lengths(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap)
{
	Inputs in;
	if (!Inputs::packed_by(FSM_HIP_META_LENGTHS, base, len, n, &in)) { errno = EINVAL; return -1; }
	return walk_host(d, in, Outputs::ends(end_out, accept_bitmap), FRONT_PACKED);
}

extern "C" double fsm_hip_lds_chain_probe_gbps(size_t table_bytes, int waves, int blocks_per_cu, size_t steps, void *d_scratch4, void *hip_stream)
{
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	DevEvent e0, e1;
	float ms = -1.f;
	if (d_scratch4 == nullptr || table_bytes < 2048 || table_bytes > 160u * 1024u || waves < 1 || waves > 16 || blocks_per_cu < 1 || steps < 16) { errno = EINVAL; return -1.0; }
	int dev = 0, ncu = 256;
	(void)hipGetDevice(&dev);
	(void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
	const uint32_t words = (uint32_t)(table_bytes / 4u);
	const unsigned grid = (unsigned)(ncu * blocks_per_cu);
	if (!HIP_OK(hipFuncSetAttribute((const void *)lds_chain_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)table_bytes))) return -1.0;
	for (int rep = 0; rep < 2; rep++) {   /* the second launch is the timed one */
		if (e0 == nullptr && (!HIP_OK(e0.create()) || !HIP_OK(e1.create()))) return -1.0;
		if (!HIP_OK(hipEventRecord(e0, s))) return -1.0;
		hipLaunchKernelGGL(lds_chain_probe_kernel, dim3(grid), dim3((unsigned)waves * 64u), table_bytes, s, words, (uint32_t)(steps / 16u * 16u), static_cast<uint32_t *>(d_scratch4));
		if (!HIP_OK(hipGetLastError())) return -1.0;
		if (!HIP_OK(hipEventRecord(e1, s))) return -1.0;
		if (!HIP_OK(hipEventSynchronize(e1))) return -1.0;
		if (!HIP_OK(hipEventElapsedTime(&ms, e0, e1))) return -1.0;
	}
	return (double)grid * waves * 64.0 * (double)(steps / 16u * 16u) / ((double)ms * 1e-3) / 1e9;
}

/* ------------------------------------------------------------------ */
/* info / tuning / end-ids                                            */
/* ------------------------------------------------------------------ */

extern "C" int fsm_hip_dfa_info(const struct fsm_hip_dfa *d, struct fsm_hip_dfa_info *out)
{
	if (d == nullptr || out == nullptr) { errno = EINVAL; return -1; }
	if (ensure_uploaded(d) != 0) return -1;
	memset(out, 0, sizeof *out);
	const Plan &p = d->plan;
	out->nstates = p.nstates;
	out->nclasses = p.C;
	out->layout = p.layout;
	out->nabsorbing = p.nabsorbing;
	/* the uploaded table's bytes; COMBSELF has always reported comb64[n] + rng16[n] + dsm[32] with neither padding nor the
	 * trailing smask[n], and keeps doing so */
	out->table_bytes = p.layout == FSM_HIP_LAYOUT_COMBSELF ? p.comb.size() * 10 + 256 : d->img.tab_size;
	LaunchCfg c = pick_cfg(d, true, 1024, 0);
	out->lds_bytes = c.lds;
	out->waves_per_block = (uint32_t)c.waves;
	out->device = (uint32_t)d->device;
	return 0;
}

extern "C" int fsm_hip_dfa_tune(struct fsm_hip_dfa *d, int knob, int value)
{
	if (d == nullptr) { errno = EINVAL; return -1; }
	if (ensure_uploaded(d) != 0) return -1;
	if (d->alt != nullptr) (void)fsm_hip_dfa_tune(d->alt, knob, value);   /* the knobs of the variable-length kernels live there */
	switch (knob) {
	case FSM_HIP_KNOB_INPUT_MODE: d->knob_input_mode = value; break;
	case FSM_HIP_KNOB_NB: d->knob_nb = value; break;
	case FSM_HIP_KNOB_ROWS: d->knob_rows = value; break;   /* the lazy walk's inputs per lane (2 / 3 / 4: A/B); the table walks have one */
	case FSM_HIP_KNOB_LAZY_DYN: d->knob_lazy_dyn = value != 0; break;
	case FSM_HIP_KNOB_LAZY_LINES: d->knob_lazy_lines = value != 0; break;
	case FSM_HIP_KNOB_MASK: break;   /* retired: exec-masking absorbing lanes cost more than it saved */
	case FSM_HIP_KNOB_SEG: d->knob_seg = value; break;
	case FSM_HIP_KNOB_PREFETCH: d->knob_prefetch = value; break;
	case FSM_HIP_KNOB_NT: d->knob_nt = value; break;
	case FSM_HIP_KNOB_PACK: d->knob_pack = value < 0 ? -1 : value != 0; break;
	case FSM_HIP_KNOB_HOT_BYTES:
		if (d->plan.layout != FSM_HIP_LAYOUT_GLOBAL || value < 0) { errno = EINVAL; return -1; }
		set_hot_bytes(d, (uint32_t)value);
		break;
	case FSM_HIP_KNOB_WAVES: d->knob_waves = value; break;
	case FSM_HIP_KNOB_BLOCKS_PER_CU: d->knob_blocks_per_cu = value; break;
	case FSM_HIP_KNOB_EARLY_RETIRE:
		/* bit 128 is round 4's resource bound, kept for the test that pins the range rule: it LOSES bytes.  Not for a stray value */
		if (value >= 0 && (value & 128) && getenv("FSM_HIP_TEST_KNOBS") == nullptr) { errno = EINVAL; return -1; }
		d->knob_early = value;
		break;
	case FSM_HIP_KNOB_NOSKIP: d->knob_noskip = value; break;
	case FSM_HIP_KNOB_RAGGED_ALIGN: break;   /* retired: segments start at the input's own first byte now */
	case FSM_HIP_KNOB_PK_RMIN:
	case FSM_HIP_KNOB_PK_RMAX:
	case FSM_HIP_KNOB_PK_DEBUG: break;   /* retired with walk_packed (round 4): accepted, ignored */
	case FSM_HIP_KNOB_SPARSE_FAST: d->knob_sparse_fast = value < 0 || value > 3 ? (d->d_lazy ? 3 : 1) : value; break;
	case FSM_HIP_KNOB_PICK_MEAN: if (value < -1) { errno = EINVAL; return -1; } d->knob_pick_mean = value; break;   /* -1: the defaults */
	case FSM_HIP_KNOB_DMA_BUFS: break;   /* retired: two DMA tiles per wave measured slower (profiles/r02m_ab_one_vs_two_dma_tiles.txt) */
	default: errno = EINVAL; return -1;
	}
	return 0;
}

extern "C" size_t fsm_hip_endid_count(const struct fsm_hip_dfa *d, uint32_t end_state)
{
	if (d == nullptr || end_state >= d->plan.nstates) return 0;
	return d->plan.endid_off[end_state + 1] - d->plan.endid_off[end_state];
}

extern "C" int fsm_hip_endid_get(const struct fsm_hip_dfa *d, uint32_t end_state,
	size_t id_buf_count, uint32_t *id_buf)
{
	if (d == nullptr || end_state >= d->plan.nstates) return 0;
	const uint32_t a = d->plan.endid_off[end_state], b = d->plan.endid_off[end_state + 1];
	if (b - a > id_buf_count) return 0; /* fsm_endid_get: 0 = buffer too small */
	for (uint32_t k = a; k < b; k++) id_buf[k - a] = d->plan.endids[k];
	return 1;
}

/* ------------------------------------------------------------------ */
/* plan inspection (no device needed; used by the CPU-side tests)      */
/* ------------------------------------------------------------------ */

struct fsm_hip_plan { Plan p; };

extern "C" struct fsm_hip_plan *fsm_hip_plan_create(const struct fsm_hip_dfa_desc *desc, unsigned flags, uint32_t lds_limit)
{
	fsm_hip_plan *pl = new (std::nothrow) fsm_hip_plan();
	if (pl == nullptr) { errno = ENOMEM; return nullptr; }
	int r = build_plan(desc, flags, lds_limit ? lds_limit : 160u * 1024u, pl->p);
	if (r != 0) { delete pl; errno = r; return nullptr; }
	return pl;
}

extern "C" void fsm_hip_plan_free(struct fsm_hip_plan *pl) { delete pl; }

extern "C" int fsm_hip_plan_get(const struct fsm_hip_plan *pl, int what, const void **data, size_t *count)
{
	if (pl == nullptr || data == nullptr || count == nullptr) { errno = EINVAL; return -1; }
	const Plan &p = pl->p;
	static thread_local uint32_t scalars[20];
	switch (what) {
	case FSM_HIP_PLAN_SCALARS:
		scalars[0] = p.nstates; scalars[1] = p.S1; scalars[2] = p.start; scalars[3] = p.C;
		scalars[4] = p.abs_min; scalars[5] = p.nabsorbing; scalars[6] = p.layout; scalars[7] = p.row_bytes;
		scalars[8] = p.comb_abs_min_off; scalars[9] = p.comb256_abs_min_off; scalars[10] = p.comb256_dflt;
		scalars[11] = p.eager_lo_end; scalars[12] = p.eager_hi_begin;
		scalars[13] = p.comb_eager_lo_off; scalars[14] = p.comb_eager_hi_off;
		scalars[15] = p.comb256_eager_lo_off; scalars[16] = p.comb256_eager_hi_off;
		*data = scalars; *count = 17; return 0;
	case FSM_HIP_PLAN_CLS: *data = p.cls; *count = 256; return 0;
	case FSM_HIP_PLAN_NEW2OLD: *data = p.new2old.data(); *count = p.new2old.size(); return 0;
	case FSM_HIP_PLAN_FIN: *data = p.fin.data(); *count = p.fin.size(); return 0;
	case FSM_HIP_PLAN_DENSE: *data = p.dense.data(); *count = p.dense.size(); return 0;
	case FSM_HIP_PLAN_TINY_COL: *data = p.tiny_col.data(); *count = p.tiny_col.size(); return 0;
	case FSM_HIP_PLAN_TINY5_COL: *data = p.tiny5_col.data(); *count = p.tiny5_col.size(); return 0;
	case FSM_HIP_PLAN_LDS_TAB: *data = p.lds_tab.data(); *count = p.lds_tab.size(); return 0;
	case FSM_HIP_PLAN_COMB: *data = p.comb.data(); *count = p.comb.size(); return 0;
	case FSM_HIP_PLAN_COMB_DFLT: *data = p.comb_dflt.data(); *count = p.comb_dflt.size(); return 0;
	case FSM_HIP_PLAN_COMB_OFF: *data = p.comb_off.data(); *count = p.comb_off.size(); return 0;
	case FSM_HIP_PLAN_COMB_FIN: *data = p.comb_fin.data(); *count = p.comb_fin.size(); return 0;
	case FSM_HIP_PLAN_GLOB_TAB: *data = p.glob_tab.data(); *count = p.glob_tab.size(); return 0;
	case FSM_HIP_PLAN_GLOB_TAB16: *data = p.glob_tab16.data(); *count = p.glob_tab16.size(); return 0;
	case FSM_HIP_PLAN_GLOB16_RANK: *data = p.glob16_rank.data(); *count = p.glob16_rank.size(); return 0;
	case FSM_HIP_PLAN_GLOB16_FIN: *data = p.glob16_fin.data(); *count = p.glob16_fin.size(); return 0;
	case FSM_HIP_PLAN_SPARSE: *data = p.sparse_img.data(); *count = p.sparse_img.size(); return 0;
	case FSM_HIP_PLAN_LAZY: *data = p.lazy_img.data(); *count = p.lazy_img.size(); return 0;
	case FSM_HIP_PLAN_COMB256: *data = p.comb256.data(); *count = p.comb256.size(); return 0;
	case FSM_HIP_PLAN_COMB256_OFF: *data = p.comb256_off.data(); *count = p.comb256_off.size(); return 0;
	case FSM_HIP_PLAN_COMB256_FIN: *data = p.comb256_fin.data(); *count = p.comb256_fin.size(); return 0;
	case FSM_HIP_PLAN_COMB_SMASK: *data = p.comb_smask.data(); *count = p.comb_smask.size(); return 0;
	case FSM_HIP_PLAN_COMB_RNG: *data = p.comb_rng.data(); *count = p.comb_rng.size(); return 0;
	case FSM_HIP_PLAN_EMASK: *data = p.emask.data(); *count = p.emask.size(); return 0;
	case FSM_HIP_PLAN_EAGER_IDS: *data = p.eager_ids.data(); *count = p.eager_ids.size(); return 0;
	case FSM_HIP_PLAN_EW_OFF: *data = p.ew_off.data(); *count = p.ew_off.size(); return 0;
	case FSM_HIP_PLAN_EW_WORD: *data = p.ew_word.data(); *count = p.ew_word.size(); return 0;
	case FSM_HIP_PLAN_EW_MASK: *data = p.ew_mask.data(); *count = p.ew_mask.size(); return 0;
	default: errno = EINVAL; return -1;
	}
}

/* ------------------------------------------------------------------ */
/* synthetic generator                                                */
/* ------------------------------------------------------------------ */

static int fill_gen(GenArgs &g, void *base, size_t stride, size_t n, uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *plant, unsigned plant_len, unsigned plant_every)
{
	memset(&g, 0, sizeof g);
	if (nalpha > 256 || plant_len > sizeof g.plant || (plant_len && (plant_every == 0 || plant_len > stride))) return -1;
	g.base = static_cast<unsigned char *>(base);
	g.stride = stride; g.n = n; g.first_index = first_index; g.seed = seed;
	g.nalpha = alphabet ? nalpha : 0;
	if (g.nalpha) memcpy(g.alphabet, alphabet, g.nalpha);
	g.plant_len = plant ? plant_len : 0;
	g.plant_every = plant_every;
	if (g.plant_len) memcpy(g.plant, plant, g.plant_len);
	return 0;
}

extern "C" int fsm_hip_gen_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *plant, unsigned plant_len, unsigned plant_every,
	void *hip_stream)
{
	GenArgs g;
	if (stride == 0 || stride % 8u != 0 || (reinterpret_cast<uintptr_t>(d_base) % 8u) != 0 ||
	    fill_gen(g, d_base, stride, n, first_index, seed, alphabet, nalpha, plant, plant_len, plant_every) != 0) {
		errno = EINVAL;
		return -1;
	}
	if (n == 0) return 0;
	uint64_t total = (uint64_t)n * (stride / 8u);
	uint64_t blocks = (total + 255) / 256;
	if (blocks > 256u * 64u) blocks = 256u * 64u;
	hipLaunchKernelGGL(gen_inputs_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), g);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) { errno = hip_errno(e); return -1; }
	return 0;
}

extern "C" void fsm_hip_gen_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *plant, unsigned plant_len, unsigned plant_every)
{
	GenArgs g;
	if (fill_gen(g, base, stride, n, first_index, seed, alphabet, nalpha, plant, plant_len, plant_every) != 0) return;
	for (size_t row = 0; row < n; row++) {
		const uint64_t gi = first_index + row;
		unsigned char *p = base + row * stride;
		for (size_t t = 0; t < stride; t += 8) {
			uint64_t v = gen_word(g, gi, t / 8);
			for (size_t k = 0; k < 8 && t + k < stride; k++) p[t + k] = (unsigned char)(v >> (8 * k));
		}
		if (g.plant_len != 0 && gi % g.plant_every == 0)
			memcpy(p + plant_offset(g, gi), g.plant, g.plant_len);
	}
}

extern "C" int fsm_hip_gen_pack_rows_device(const void *d_rows, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	size_t max_len, void *d_out, void *hip_stream)
{
	if (n == 0) return 0;
	if (d_rows == nullptr || d_len == nullptr || d_off == nullptr || d_out == nullptr || max_len > stride) { errno = EINVAL; return -1; }
	const uint64_t wpr = (max_len + 7u) / 8u;
	if (wpr == 0) return 0;
	uint64_t blocks = ((uint64_t)n * wpr + 255u) / 256u;
	if (blocks > 256u * 64u) blocks = 256u * 64u;
	hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
	                   static_cast<const unsigned char *>(d_rows), (uint64_t)stride, d_len, d_off, (uint64_t)n, wpr, static_cast<unsigned char *>(d_out));
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) { errno = hip_errno(e); return -1; }
	return 0;
}

/* ---- affix generator (see walk_kernels.h) ---- */

static int fill_affix(AffixArgs &x, const unsigned char *body, unsigned nbody, const unsigned char *body2, unsigned nbody2,
	unsigned npfx, unsigned nsfx, unsigned every)
{
	memset(&x, 0, sizeof x);
	if (body == nullptr || nbody == 0 || nbody > 256 || npfx == 0 || nsfx == 0 || every == 0 ||
	    nbody2 > sizeof x.body2 || (nbody2 != 0 && body2 == nullptr)) return -1;
	x.npfx = npfx; x.nsfx = nsfx; x.every = every; x.nbody = nbody; x.nbody2 = nbody2;
	memcpy(x.body, body, nbody);
	if (nbody2) memcpy(x.body2, body2, nbody2);
	return 0;
}

static int check_affixes(const unsigned char *t, unsigned n, size_t stride)
{
	if (t == nullptr) return -1;
	for (unsigned i = 0; i < n; i++) if (t[8 * i] > 7 || t[8 * i] > stride / 2) return -1;
	return 0;
}

extern "C" int fsm_hip_gen_affix2_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *body2, unsigned nbody2,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every, void *hip_stream)
{
	GenArgs g;
	AffixArgs x;
	DevBuf<unsigned char> d_tab;
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	if (stride == 0 || stride % 8u != 0 || (reinterpret_cast<uintptr_t>(d_base) % 8u) != 0 ||
	    fill_gen(g, d_base, stride, n, first_index, seed, alphabet, nalpha, nullptr, 0, 0) != 0 ||
	    fill_affix(x, body, nbody, body2, nbody2, npfx, nsfx, every) != 0 ||
	    check_affixes(prefixes, npfx, stride) != 0 || check_affixes(suffixes, nsfx, stride) != 0) {
		errno = EINVAL;
		return -1;
	}
	if (n == 0) return 0;
	if (!HIP_OK(d_tab.alloc(8u * ((size_t)npfx + nsfx)))) return -1;
	if (!HIP_OK(hipMemcpy(d_tab, prefixes, 8u * (size_t)npfx, hipMemcpyHostToDevice))) return -1;
	if (!HIP_OK(hipMemcpy(d_tab + 8u * (size_t)npfx, suffixes, 8u * (size_t)nsfx, hipMemcpyHostToDevice))) return -1;
	x.pfx = d_tab;
	x.sfx = d_tab + 8u * (size_t)npfx;
	{
		uint64_t total = (uint64_t)n * (stride / 8u);
		uint64_t blocks = (total + 255) / 256;
		if (blocks > 256u * 64u) blocks = 256u * 64u;
		hipLaunchKernelGGL(gen_affix_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, x);
		if (!HIP_OK(hipGetLastError())) return -1;
		if (!HIP_OK(hipStreamSynchronize(s))) return -1; /* the table goes with this call */
	}
	return 0;
}

extern "C" int fsm_hip_gen_affix_inputs_device(void *d_base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every, void *hip_stream)
{
	return fsm_hip_gen_affix2_inputs_device(d_base, stride, n, first_index, seed, alphabet, nalpha, body, nbody, nullptr, 0,
	                                        prefixes, npfx, suffixes, nsfx, every, hip_stream);
}

extern "C" void fsm_hip_gen_affix2_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *body2, unsigned nbody2,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every)
{
	GenArgs g;
	AffixArgs x;
	if (fill_gen(g, base, stride, n, first_index, seed, alphabet, nalpha, nullptr, 0, 0) != 0 ||
	    fill_affix(x, body, nbody, body2, nbody2, npfx, nsfx, every) != 0 ||
	    check_affixes(prefixes, npfx, stride) != 0 || check_affixes(suffixes, nsfx, stride) != 0) return;
	x.pfx = prefixes;
	x.sfx = suffixes;
	for (size_t row = 0; row < n; row++) {
		unsigned char *p = base + row * stride;
		for (size_t t = 0; t < stride; t += 8) {
			uint64_t v = affix_word(g, x, first_index + row, t / 8);
			for (size_t k = 0; k < 8 && t + k < stride; k++) p[t + k] = (unsigned char)(v >> (8 * k));
		}
	}
}

extern "C" void fsm_hip_gen_affix_inputs_host(unsigned char *base, size_t stride, size_t n,
	uint64_t first_index, uint64_t seed,
	const unsigned char *alphabet, unsigned nalpha,
	const unsigned char *body, unsigned nbody,
	const unsigned char *prefixes, unsigned npfx,
	const unsigned char *suffixes, unsigned nsfx,
	unsigned every)
{
	fsm_hip_gen_affix2_inputs_host(base, stride, n, first_index, seed, alphabet, nalpha, body, nbody, nullptr, 0,
	                               prefixes, npfx, suffixes, nsfx, every);
}

/* ---- HBM read-stream probe ---- */

extern "C" double fsm_hip_stream_read_probe_ms(const void *d_base, size_t bytes, void *d_scratch4, int reps, void *hip_stream)
{
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	DevEvent e0, e1;
	float ms = -1.f;
	if (d_base == nullptr || d_scratch4 == nullptr || bytes < 16 || reps <= 0 ||
	    (reinterpret_cast<uintptr_t>(d_base) % 16u) != 0) { errno = EINVAL; return -1.0; }
	int dev = 0, ncu = 256;
	(void)hipGetDevice(&dev);
	(void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
	if (!HIP_OK(e0.create())) return (double)ms;
	if (!HIP_OK(e1.create())) return (double)ms;
	for (int nt = 0; nt < 2; nt++) {   /* plain and nontemporal loads: the faster of the two is reported */
		void (*k)(const u32x4 *, uint64_t, uint32_t *) = nt ? stream_read_kernel<true> : stream_read_kernel<false>;
		float t = -1.f;
		hipLaunchKernelGGL(k, dim3((unsigned)ncu * 8u), dim3(256), 0, s,
		                   static_cast<const u32x4 *>(d_base), (uint64_t)(bytes / 16u), static_cast<uint32_t *>(d_scratch4));
		if (!HIP_OK(hipEventRecord(e0, s))) return (double)ms;
		for (int r = 0; r < reps; r++)
			hipLaunchKernelGGL(k, dim3((unsigned)ncu * 8u), dim3(256), 0, s,
			                   static_cast<const u32x4 *>(d_base), (uint64_t)(bytes / 16u), static_cast<uint32_t *>(d_scratch4));
		if (!HIP_OK(hipEventRecord(e1, s))) return (double)ms;
		if (!HIP_OK(hipEventSynchronize(e1))) return (double)ms;
		if (!HIP_OK(hipEventElapsedTime(&t, e0, e1))) return (double)ms;
		t /= (float)reps;
		if (ms < 0.f || t < ms) ms = t;
	}
	if (bytes >= ((size_t)64 << 20)) {
		/* third candidate: the walk's own input path without the walk -- LDS-DMA of 128-byte segments of
		 * 1 KiB rows into per-wave tiles (6.5-7.06 TB/s; a few waves per CU already saturate it) */
		const uint64_t stride = 1024, nrows = (bytes / stride) / 64u * 64u;
		for (int waves = 3; waves <= 12; waves *= 2) {   /* 3, 6, 12 waves per workgroup, two workgroups per CU */
			const size_t ldsb = (size_t)waves * 8192u;
			float t = -1.f;
			if (!HIP_OK(hipFuncSetAttribute((const void *)dma_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb))) return (double)ms;
			hipLaunchKernelGGL(dma_stream_kernel, dim3((unsigned)ncu * 2u), dim3((unsigned)waves * 64u), ldsb, s,
			                   static_cast<const uint8_t *>(d_base), nrows, stride, static_cast<uint32_t *>(d_scratch4));
			if (!HIP_OK(hipEventRecord(e0, s))) return (double)ms;
			for (int r = 0; r < reps; r++)
				hipLaunchKernelGGL(dma_stream_kernel, dim3((unsigned)ncu * 2u), dim3((unsigned)waves * 64u), ldsb, s,
				                   static_cast<const uint8_t *>(d_base), nrows, stride, static_cast<uint32_t *>(d_scratch4));
			if (!HIP_OK(hipEventRecord(e1, s))) return (double)ms;
			if (!HIP_OK(hipEventSynchronize(e1))) return (double)ms;
			if (!HIP_OK(hipEventElapsedTime(&t, e0, e1))) return (double)ms;
			t = t / (float)reps * (float)((double)bytes / (double)(nrows * stride));   /* normalise to `bytes` */
			if (t > 0.f && t < ms) ms = t;
		}
	}
	return (double)ms;
}

extern "C" double fsm_hip_gather_probe_ms(const void *d_base, size_t bytes, size_t ngathers, int vec_bytes, void *d_scratch4, void *hip_stream)
{
	hipStream_t s = static_cast<hipStream_t>(hip_stream);
	DevEvent e0, e1;
	float ms = -1.f;
	if (d_base == nullptr || d_scratch4 == nullptr || (vec_bytes != 4 && vec_bytes != 16) || bytes < 16 || ngathers == 0 ||
	    (reinterpret_cast<uintptr_t>(d_base) % 16u) != 0) { errno = EINVAL; return -1.0; }
	int dev = 0, ncu = 256;
	(void)hipGetDevice(&dev);
	(void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
	if (!HIP_OK(e0.create())) return (double)ms;
	if (!HIP_OK(e1.create())) return (double)ms;
	if (!HIP_OK(hipEventRecord(e0, s))) return (double)ms;
	if (vec_bytes == 16)
		hipLaunchKernelGGL(gather_probe_kernel<16>, dim3((unsigned)ncu * 8u), dim3(256), 0, s, static_cast<const unsigned char *>(d_base),
		                   (uint64_t)(bytes / 16u), (uint64_t)ngathers, static_cast<uint32_t *>(d_scratch4));
	else
		hipLaunchKernelGGL(gather_probe_kernel<4>, dim3((unsigned)ncu * 8u), dim3(256), 0, s, static_cast<const unsigned char *>(d_base),
		                   (uint64_t)(bytes / 4u), (uint64_t)ngathers, static_cast<uint32_t *>(d_scratch4));
	if (!HIP_OK(hipGetLastError())) return (double)ms;
	if (!HIP_OK(hipEventRecord(e1, s))) return (double)ms;
	if (!HIP_OK(hipEventSynchronize(e1))) return (double)ms;
	if (!HIP_OK(hipEventElapsedTime(&ms, e0, e1))) return (double)ms;
	return (double)ms;
}

/* ------------------------------------------------------------------ */
/* end-ids delivered by the device                                    */
/* ------------------------------------------------------------------ */

/* the per-encoded-state tables the kernel copies into id_out[] (image.cpp build_id_tables), once */
static int ensure_ids(fsm_hip_dfa *d)
{
	if (ensure_uploaded(d) != 0) return -1;
	DfaLock lk(d->mu);
	if (d->ids_ready) return 0;
	build_id_tables(d->plan, d->img, d->ids);
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (!HIP_OK(d->d_fin_earliest.upload(d->ids.earliest))) return -1;
	if (!HIP_OK(d->d_fin_ret.upload(d->ids.ret))) return -1;
	std::vector<uint32_t>().swap(d->ids.earliest);
	std::vector<uint32_t>().swap(d->ids.ret);
	d->ids_ready = true;
	return 0;
}

static Outputs ids_outputs(int mode, uint32_t *id_out)
{
	Outputs o;
	o.ids_mode = mode;
	o.id_out = id_out;
	return o;
}

extern "C" int fsm_hip_exec_batch_ids_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	int mode, uint32_t *d_id_out, void *hip_stream)
{
	if (d_id_out == nullptr) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, nullptr, n), ids_outputs(mode, d_id_out), hip_stream, BatchHint(), FRONT_IDS);
}

extern "C" int fsm_hip_exec_batch_ids_offsets_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint64_t *d_off, size_t n,
	int mode, uint32_t *d_id_out, void *hip_stream)
{
	if (d_id_out == nullptr || (n != 0 && d_off == nullptr)) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, 0, nullptr, d_off, n), ids_outputs(mode, d_id_out), hip_stream, BatchHint(), FRONT_IDS);
}

extern "C" int fsm_hip_exec_batch_ids(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	int mode, uint32_t *id_out)
{
	if (id_out == nullptr) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, stride, len, nullptr, n), ids_outputs(mode, id_out), FRONT_IDS);
}

extern "C" int fsm_hip_exec_batch_ids_offsets(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint64_t *off, size_t n,
	int mode, uint32_t *id_out)
{
	if (id_out == nullptr || (n != 0 && off == nullptr)) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, 0, nullptr, off, n), ids_outputs(mode, id_out), FRONT_IDS);
}

extern "C" int fsm_hip_ids_conflict(const struct fsm_hip_dfa *dc, fsm_state_t *state)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(dc);
	if (d == nullptr) { errno = EINVAL; return -1; }
	if (ensure_ids(d) != 0) return -1;
	if (d->ids.conflict == FSM_HIP_NO_MATCH) return 0;
	if (state != nullptr) *state = d->ids.conflict;
	return 1;
}

extern "C" size_t fsm_hip_ret_count(const struct fsm_hip_dfa *dc)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(dc);
	if (d == nullptr || ensure_ids(d) != 0) return 0;
	return d->ids.ret_off.size() - 1;
}

extern "C" int fsm_hip_ret_get(const struct fsm_hip_dfa *dc, uint32_t ret_index, const uint32_t **ids, size_t *count)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(dc);
	if (d == nullptr || ids == nullptr || count == nullptr || ensure_ids(d) != 0 || ret_index + 1 >= d->ids.ret_off.size()) {
		errno = EINVAL;
		return -1;
	}
	*ids = d->ids.ret_ids.data() + d->ids.ret_off[ret_index];
	*count = d->ids.ret_off[ret_index + 1] - d->ids.ret_off[ret_index];
	return 0;
}

/* ------------------------------------------------------------------ */
/* resume: start every input from a given state, return the state reached */
/* ------------------------------------------------------------------ */

static int ensure_resume(fsm_hip_dfa *d)
{
	if (ensure_uploaded(d) != 0) return -1;
	DfaLock lk(d->mu);
	if (d->resume_ready) return 0;
	ResumeTables t;
	build_resume_tables(d->plan, d->img, t);
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (!HIP_OK(d->d_enc_of.upload(t.enc_of))) return -1;
	if (!HIP_OK(d->d_orig_of.upload(t.orig_of))) return -1;
	d->resume_ready = true;
	return 0;
}

extern "C" int fsm_hip_state_is_absorbing(const struct fsm_hip_dfa *d, uint32_t state)
{
	if (d == nullptr) { errno = EINVAL; return -1; }
	if (state == FSMHIP_STATE_DEAD) return 1;
	if (state == FSMHIP_STATE_START) state = d->plan.new2old[d->plan.start];
	if (state >= d->plan.nstates) { errno = EINVAL; return -1; }
	return d->plan.old2new[state] >= d->plan.abs_min ? 1 : 0;
}

static Outputs resume_outputs(uint32_t *state_io, uint32_t *end_out, uint64_t *bitmap, uint64_t *eager_io)
{
	Outputs o = Outputs::ends(end_out, bitmap);
	o.state_io = state_io;
	o.eager_io = eager_io;
	return o;
}

extern "C" int fsm_hip_exec_batch_resume_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	if (d_state_io == nullptr) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, nullptr, n), resume_outputs(d_state_io, d_end_out, d_accept_bitmap, nullptr), hip_stream, BatchHint(), FRONT_RESUME);
}

extern "C" int fsm_hip_exec_batch_resume_offsets_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	if (d_state_io == nullptr || (n != 0 && d_off == nullptr)) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, 0, nullptr, d_off, n), resume_outputs(d_state_io, d_end_out, d_accept_bitmap, nullptr), hip_stream, BatchHint(), FRONT_RESUME);
}

/* resume over packed inputs whose metadata is u64 offsets, u32 offsets or lengths alone: the carry of fsm_vm_match_file
 * (src/libfsm/vm.c:188-216: the state survives from one buffer to the next) for batches in the compact forms */
extern "C" int fsm_hip_exec_batch_resume_packed_device(const struct fsm_hip_dfa *d,
	const void *d_base, int meta_form, const void *d_meta, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_accept_bitmap, void *hip_stream)
{
	Inputs in;
	if (d_state_io == nullptr || !Inputs::packed_by(meta_form, d_base, d_meta, n, &in)) { errno = EINVAL; return -1; }
	return walk_device(d, in, resume_outputs(d_state_io, d_end_out, d_accept_bitmap, nullptr), hip_stream, BatchHint(), FRONT_RESUME);
}

extern "C" int fsm_hip_exec_batch_resume(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *state_io, uint32_t *end_out)
{
	if (state_io == nullptr) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, stride, len, nullptr, n), resume_outputs(state_io, end_out, nullptr, nullptr), FRONT_RESUME);
}

extern "C" int fsm_hip_exec_batch_resume_offsets(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *state_io, uint32_t *end_out)
{
	if (state_io == nullptr || (n != 0 && off == nullptr)) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, 0, nullptr, off, n), resume_outputs(state_io, end_out, nullptr, nullptr), FRONT_RESUME);
}

extern "C" int fsm_hip_exec_batch_resume_packed(const struct fsm_hip_dfa *d,
	const unsigned char *base, int meta_form, const void *meta, size_t n,
	uint32_t *state_io, uint32_t *end_out)
{
	Inputs in;
	if (state_io == nullptr || !Inputs::packed_by(meta_form, base, meta, n, &in)) { errno = EINVAL; return -1; }
	return walk_host(d, in, resume_outputs(state_io, end_out, nullptr, nullptr), FRONT_RESUME);
}

/* resume + eager outputs: the carry of fsm_vm_match_file with fsm_exec's callback installed (exec.c:126-151) */
extern "C" int fsm_hip_exec_batch_eager_resume_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	uint32_t *d_state_io, uint32_t *d_end_out, uint64_t *d_eager_io, void *hip_stream)
{
	if (d_state_io == nullptr || d_eager_io == nullptr) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, d_off, n), resume_outputs(d_state_io, d_end_out, nullptr, d_eager_io), hip_stream, BatchHint(), FRONT_RESUME);
}

extern "C" int fsm_hip_exec_batch_eager_resume(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, const uint64_t *off, size_t n,
	uint32_t *state_io, uint32_t *end_out, uint64_t *eager_io)
{
	if (state_io == nullptr || eager_io == nullptr) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, stride, len, off, n), resume_outputs(state_io, end_out, nullptr, eager_io), FRONT_RESUME);
}

/* ------------------------------------------------------------------ */
/* eager outputs                                                      */
/* ------------------------------------------------------------------ */

extern "C" size_t fsm_hip_eager_id_count(const struct fsm_hip_dfa *d)
{
	return d == nullptr ? 0 : d->plan.eager_ids.size();
}

extern "C" size_t fsm_hip_eager_words(const struct fsm_hip_dfa *d)
{
	return d == nullptr || d->plan.eager_words == 0 ? 1 : d->plan.eager_words;
}

extern "C" uint32_t fsm_hip_eager_id(const struct fsm_hip_dfa *d, unsigned bit)
{
	if (d == nullptr || bit >= d->plan.eager_ids.size()) return FSM_HIP_NO_MATCH;
	return d->plan.eager_ids[bit];
}

static Outputs eager_outputs(uint32_t *end_out, uint64_t *eager_out)
{
	Outputs o = Outputs::ends(end_out, nullptr);
	o.eager_out = eager_out;
	return o;
}

extern "C" int fsm_hip_exec_batch_eager_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, size_t n,
	uint32_t *d_end_out, uint64_t *d_eager_out, void *hip_stream)
{
	if (d_eager_out == nullptr) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, nullptr, n), eager_outputs(d_end_out, d_eager_out), hip_stream, BatchHint(), FRONT_EAGER);
}

extern "C" int fsm_hip_exec_batch_eager_offsets_device(const struct fsm_hip_dfa *d,
	const void *d_base, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_eager_out, void *hip_stream)
{
	if (d_eager_out == nullptr || (n != 0 && d_off == nullptr)) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, 0, nullptr, d_off, n), eager_outputs(d_end_out, d_eager_out), hip_stream, BatchHint(), FRONT_EAGER);
}

extern "C" int fsm_hip_exec_batch_eager(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, size_t n,
	uint32_t *end_out, uint64_t *eager_out)
{
	if (eager_out == nullptr) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, stride, len, nullptr, n), eager_outputs(end_out, eager_out), FRONT_EAGER);
}

extern "C" int fsm_hip_exec_batch_eager_offsets(const struct fsm_hip_dfa *d,
	const unsigned char *base, const uint64_t *off, size_t n,
	uint32_t *end_out, uint64_t *eager_out)
{
	if (eager_out == nullptr || (n != 0 && off == nullptr)) { errno = EINVAL; return -1; }
	return walk_host(d, Inputs::rows_or_offsets(base, 0, nullptr, off, n), eager_outputs(end_out, eager_out), FRONT_EAGER);
}

static Outputs all_outputs(uint32_t *end_out, uint64_t *bitmap, int ids_mode, uint32_t *id_out, uint64_t *eager_out)
{
	Outputs o = Outputs::ends(end_out, bitmap);
	o.ids_mode = ids_mode;
	o.id_out = id_out;
	o.eager_out = eager_out;
	return o;
}

/* Every output of one batch from ONE walk: end states and / or the accept bitmap, device-side end-ids (ids_mode, d_id_out) and
 * eager sets (d_eager_out), whichever are asked for (the multi-device front used to launch one walk per output) */
extern "C" int fsm_hip_exec_batch_all_device(const struct fsm_hip_dfa *d,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream)
{
	if (d_off != nullptr && d_len != nullptr) { errno = EINVAL; return -1; }
	return walk_device(d, Inputs::rows_or_offsets(d_base, stride, d_len, d_off, n), all_outputs(d_end_out, d_accept_bitmap, ids_mode, d_id_out, d_eager_out), hip_stream, BatchHint(), FRONT_ALL);
}

/* the same over packed inputs whose metadata is u64 offsets, u32 offsets or lengths alone */
extern "C" int fsm_hip_exec_batch_packed_all_device(const struct fsm_hip_dfa *d,
	const void *d_base, int meta_form, const void *d_meta, size_t n,
	uint32_t *d_end_out, uint64_t *d_accept_bitmap, int ids_mode, uint32_t *d_id_out, uint64_t *d_eager_out, void *hip_stream)
{
	Inputs in;
	if (!Inputs::packed_by(meta_form, d_base, d_meta, n, &in)) { errno = EINVAL; return -1; }
	return walk_device(d, in, all_outputs(d_end_out, d_accept_bitmap, ids_mode, d_id_out, d_eager_out), hip_stream, BatchHint(), FRONT_ALL);
}

/* host pointers: the metadata is checked (non-decreasing offsets, the lengths' sum is the batch) */
extern "C" int fsm_hip_exec_batch_packed_all(const struct fsm_hip_dfa *d,
	const unsigned char *base, int meta_form, const void *meta, size_t n,
	uint32_t *end_out, uint64_t *accept_bitmap, int ids_mode, uint32_t *id_out, uint64_t *eager_out)
{
	Inputs in;
	if (!Inputs::packed_by(meta_form, base, meta, n, &in)) { errno = EINVAL; return -1; }
	return walk_host(d, in, all_outputs(end_out, accept_bitmap, ids_mode, id_out, eager_out), FRONT_ALL);
}

/* ---- the emission stream (order and repeats kept): trace_kernel.h ---- */

static int ensure_trace(fsm_hip_dfa *d)
{
	if (ensure_uploaded(d) != 0) return -1;
	DfaLock lk(d->mu);
	if (d->trace_ready) return 0;
	const Plan &p = d->plan;
	if (p.dense.size() != (size_t)p.S1 * p.C) { errno = ENOTSUP; return -1; }
	TraceTables t;
	build_trace_tables(p, t);
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	if (!HIP_OK(d->d_tr_dense.upload(p.dense))) return -1;
	if (!HIP_OK(d->d_tr_cls4.upload(t.cls4))) return -1;
	if (!HIP_OK(d->d_tr_eoff.upload(t.eoff))) return -1;
	if (!HIP_OK(d->d_tr_eids.upload(t.eids))) return -1;
	if (!HIP_OK(d->d_tr_fin.upload(p.fin))) return -1;
	d->trace_ready = true;
	return 0;
}

extern "C" int fsm_hip_exec_batch_eager_trace_device(const struct fsm_hip_dfa *cd,
	const void *d_base, size_t stride, const uint32_t *d_len, const uint64_t *d_off, size_t n, size_t cap,
	uint32_t *d_end_out, uint32_t *d_count_out, uint32_t *d_ids_out, uint32_t *d_pos_out, void *hip_stream)
{
	fsm_hip_dfa *d = const_cast<fsm_hip_dfa *>(cd);
	if (d == nullptr || d_count_out == nullptr || (cap != 0 && d_ids_out == nullptr) || cap > 0xFFFFFFFFu ||
	    (n != 0 && d_off == nullptr && d_base == nullptr && stride != 0)) { errno = EINVAL; return -1; }
	if (n == 0) return 0;
	if (ensure_trace(d) != 0) return -1;
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	TraceArgs a;
	a.base = static_cast<const uint8_t *>(d_base);
	a.stride = d_off ? 0 : stride;
	a.len = d_off ? nullptr : d_len;
	a.off = d_off;
	a.n = n;
	a.dense = d->d_tr_dense; a.cls4 = d->d_tr_cls4; a.eoff = d->d_tr_eoff; a.eids = d->d_tr_eids; a.fin = d->d_tr_fin;
	a.C = d->plan.C; a.start = d->plan.start; a.dead = d->plan.S1 - 1u;
	a.cap = (uint32_t)cap;
	a.end_out = d_end_out; a.count_out = d_count_out; a.ids_out = d_ids_out; a.pos_out = d_pos_out;
	const uint64_t blocks = (n + 255u) / 256u;
	if (blocks > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
	hipLaunchKernelGGL(eager_trace_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) { errno = hip_errno(e); return -1; }
	return 0;
}

extern "C" int fsm_hip_exec_batch_eager_trace(const struct fsm_hip_dfa *d,
	const unsigned char *base, size_t stride, const uint32_t *len, const uint64_t *off, size_t n, size_t cap,
	uint32_t *end_out, uint32_t *count_out, uint32_t *ids_out, uint32_t *pos_out)
{
	size_t in_bytes = 0;
	uint64_t payload = 0;
	if (d == nullptr || count_out == nullptr || (cap != 0 && ids_out == nullptr) || cap > 0xFFFFFFFFu ||
	    check_host_inputs(Inputs::rows_or_offsets(base, stride, len, off, n), &in_bytes, &payload) != 0) { errno = EINVAL; return -1; }
	if (n == 0) return 0;
	if (n > ((size_t)1 << 40) / (cap ? cap : 1)) { errno = EINVAL; return -1; }
	DevGuard dg(d->device);
	if (!dg.ok()) { errno = ENODEV; return -1; }
	HostCall hc(d);
	const int p_in = hc.add(HostCall::IN, base, nullptr, in_bytes, 32);
	const int p_len = len ? hc.add(HostCall::IN, len, nullptr, n * sizeof(uint32_t)) : -1;
	const int p_off = off ? hc.add(HostCall::IN, off, nullptr, (n + 1) * sizeof(uint64_t)) : -1;
	const int p_end = hc.add(HostCall::OUT, nullptr, end_out, n * sizeof(uint32_t));
	const int p_cnt = hc.add(HostCall::OUT, nullptr, count_out, n * sizeof(uint32_t));
	const int p_ids = hc.add(HostCall::OUT, nullptr, ids_out, n * cap * sizeof(uint32_t));
	const int p_pos = hc.add(HostCall::OUT, nullptr, pos_out, n * cap * sizeof(uint32_t));
	if (hc.begin() != 0) return -1;
	if (fsm_hip_exec_batch_eager_trace_device(d, hc.dev<unsigned char>(p_in), stride, hc.dev<uint32_t>(p_len), hc.dev<uint64_t>(p_off), n, cap,
	                                          hc.dev<uint32_t>(p_end), hc.dev<uint32_t>(p_cnt), hc.dev<uint32_t>(p_ids), hc.dev<uint32_t>(p_pos), hc.d->hs) != 0) return -1;
	return hc.end();
}
