/*
 * text_objects.h -- what the other units read of a text and of its hits (both made in text.hip): the two objects themselves, for
 * the tally's file groups and the distinct records of the hits, and the batch that the lines of a text, or of its hits, are for a
 * front.  Not part of the C ABI: the types are the library's own, their destructors are no exported symbols.  Host code only.
 */
#ifndef FSMHIP_CSRC_TEXT_OBJECTS_H
#define FSMHIP_CSRC_TEXT_OBJECTS_H

#include <initializer_list>
#include <optional>

#include "hip_host.h"
#include "line_batch.h"

#pragma GCC visibility push(hidden)

struct fsm_hip_text {
	int device = 0, delim = 0;
	size_t nbytes = 0, n = 0;
	const unsigned char *d_text = nullptr;   /* the caller's bytes (open_device) or `owned` */
	DevBuf<unsigned char> owned;
	DevBuf<uint64_t> d_off;                  /* n + 1 */
	DevBuf<uint64_t> d_cnt;                  /* per block: its delimiters, then their exclusive scan; + the 2 (files: 4) words of meta */
	DevEvent ev[4];                          /* around count + scan, around offsets; ev[3]: the offsets are there */
	/* a text of files (fsm_hip_text_open_files*): all NULL / 0 in a plain text */
	size_t nfiles = 0;
	const uint64_t *d_file_off = nullptr;    /* nfiles + 1: the caller's (open_files_device) or `owned_file_off` */
	DevBuf<uint64_t> owned_file_off;
	DevBuf<uint64_t> d_file_lines;           /* nfiles + 1 */
	DevBuf<uint64_t> d_plain;                /* the plain offsets the merge reads; the host form frees them once its stream is idle */
	DevBuf<uint64_t> d_frank;                /* per file end: (added ends before it in its block) << 1 | it adds one */
	DevBuf<uint64_t> d_fpairs;               /* per block of file ends: (added ends, invalid entries), then their exclusive scan */
	DevEvent fev[3];                         /* around mark + scan; fev[2]: the plain offsets are there, the merge runs to ev[3] */
	DevStream own;                           /* the host-pointer forms run here, never on the NULL stream (last: it goes first) */
};

struct fsm_hip_text_hits {
	int device = 0, delim = 0;                   /* delim: the text's */
	size_t m = 0, nbytes = 0;
	DevBuf<uint64_t> d_pairs;                /* per block of lines: (lines, bytes) selected, then their exclusive scan; + m and the bytes */
	DevBuf<uint64_t> d_lines;                /* m */
	DevBuf<uint64_t> d_off;                  /* m + 1 */
	DevBuf<uint64_t> d_src;                  /* m: where each selected line starts in the text */
	DevBuf<uint64_t> d_first;                /* per output block + 1: the rank of the line that covers its first byte */
	DevBuf<unsigned char> d_bytes;           /* nbytes, rounded up to whole blocks */
	DevEvent ev[6];                          /* around count + scan, emit, gather; ev[5]: all is there */
	size_t nfiles = 0;                       /* a text of files: its hits per file; 0 / NULL for a plain text */
	DevBuf<uint64_t> d_file_first;           /* nfiles + 1 */
	DevEvent fev[2];                         /* around hits_file_first, between emit and gather */
	/* hits with context (fsm_hip_text_hits_context*): all NULL / 0 in plain hits */
	bool context = false;
	size_t core_count = 0;
	DevBuf<uint64_t> d_wide;                 /* ceil(n / 64): W, the bitmap the select reads */
	DevBuf<uint64_t> d_fmap;                 /* ceil(n / 64): F, the file starts; NULL for a plain text */
	DevBuf<uint64_t> d_sum;                  /* per block of lines: its summary, then the carries; + the 2 words of d_cmeta */
	uint64_t *d_cmeta = nullptr;             /* inside d_sum: (core_count, groups), counted by atomics from 0 */
	DevBuf<uint64_t> d_core;                 /* ceil(m / 64) */
	DevBuf<uint64_t> d_group;                /* ceil(m / 64) */
	DevEvent cev[4];                         /* around the widening, around the marks */
};

/* The lines of a text, or (h != null) of its hits, as a batch for a front on stream s: every object of `devices` is on the
 * text's device, which *dg makes current for the caller; the stream waits for the hits' lines (and, behind them, the text's
 * offsets).  false + errno. */
inline bool text_batch(const struct fsm_hip_text *t, const struct fsm_hip_text_hits *h, std::initializer_list<int> devices, hipStream_t s,
	std::optional<DevGuard> *dg, fsmhip::LineBatch *in)
{
	for (int d : devices)
		if (d != t->device) { errno = EINVAL; return false; }
	if (h != nullptr && h->device != t->device) { errno = EINVAL; return false; }
	dg->emplace(t->device);
	if (!(*dg)->ok()) { errno = ENODEV; return false; }
	if (!HIP_OK(hipStreamWaitEvent(s, h != nullptr ? h->ev[5] : t->ev[3], 0))) return false;
	in->base = t->d_text;
	in->off = t->d_off;
	in->n = t->n;
	in->pick = h != nullptr ? h->d_lines.p : nullptr;
	in->m = h != nullptr ? h->m : t->n;
	in->limit = t->nbytes;
	in->has_limit = true;
	in->trim = t->delim;
	return true;
}

#pragma GCC visibility pop

#endif
