/*
 * examples/hipsed.c -- sed 's/pat/repl/g' for a union of rules over many files, spliced on the device: no host loop over bytes
 * and none over matches:
 *
 *     hipsed [-m | -t] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip REPL... -- FILE...
 *
 * The three tables are hipscan's (examples/hipscan.c): LINES selects the lines that hold a match, STARTS accepts anything followed
 * by the reversal of pat, ENDS accepts exactly pat and carries one end-id per rule.  The i-th REPL replaces every match of rule
 * i; a rule without a REPL, and a match whose state has no id, stay as they are.  fsm_hip_text_matches() finds every match of
 * EVERY line -- not only of the hits, so lines without one pass through unchanged --, fsm_hip_text_replace() builds the new text
 * on the device, and the files' text comes out on stdout, delimiters and a missing last newline as they were.
 *     -m         mask (FSM_HIP_REPL_MASK): a match keeps its length and is filled with its REPL, repeated; an empty REPL leaves it
 *     -t         template (fsm_hip_repl_create_template): every REPL is a sed replacement -- & is the match itself, \& and \\ are
 *                the literals & and \, a backslash before anything else stands for itself, a REPL may not end in one.
 *                s/[0-9]+/(&)/g, grep --color.  Not together with -m
 * Exit status: 0 if some line held a match (LINES), 1 if none did (the text is written all the same), 2 on error.  Plain C against
 * include/fsm_hip.h only.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

static struct fsm_hip_dfa_desc *
read_desc(const char *path)
{
	struct fsm_hip_dfa_desc *desc;
	FILE *f;

	f = fopen(path, "rb");
	if (f == NULL) {
		perror(path);
		exit(2);
	}
	desc = fsm_hip_desc_read(f);
	fclose(f);
	if (desc == NULL) {
		perror("fsm_hip_desc_read");
		exit(2);
	}
	return desc;
}

static struct fsm_hip_dfa *
read_dfa(const char *path)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;

	desc = read_desc(path);
	dfa = fsm_hip_dfa_create(desc, FSM_HIP_DEFER_UPLOAD);   /* planned only: the images are all that goes to the device */
	fsm_hip_desc_free(desc);
	if (dfa == NULL) {
		perror("fsm_hip_dfa_create");
		exit(2);
	}
	return dfa;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_pos_dfa *starts;
	struct fsm_hip_tok_dfa *ends;
	struct fsm_hip_repl *repl;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	struct fsm_hip_matches *matches;
	struct fsm_hip_replaced *replaced;
	unsigned char *buf = NULL, *rbytes = NULL, *out = NULL;
	uint64_t *file_off, *roff, *ioff = NULL, *ins = NULL, nout;
	size_t cap = 0, len = 0, got, nfiles, nrepl, j, k, rlen = 0, nhits;
	unsigned flags = 0;
	int a, sep, tmpl = 0;
	const char *arg;
	char **names;
	FILE *f;

	a = 1;
	while (a < argc && (strcmp(argv[a], "-m") == 0 || strcmp(argv[a], "-t") == 0)) {
		if (argv[a][1] == 'm') {
			flags = FSM_HIP_REPL_MASK;
		} else {
			tmpl = 1;
		}
		a++;
	}
	for (sep = a + 3; sep < argc && strcmp(argv[sep], "--") != 0; sep++) {
		;
	}
	if (a + 3 > argc || sep >= argc - 1 || (tmpl && flags != 0)) {
		fprintf(stderr, "usage: hipsed [-m | -t] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip REPL... -- FILE...\n");
		return 2;
	}
	desc = read_desc(argv[a]);
	ld = fsm_hip_lines_dfa_create(desc, '\n', 0);
	fsm_hip_desc_free(desc);
	if (ld == NULL) {
		perror("fsm_hip_lines_dfa_create");
		return 2;
	}
	dfa = read_dfa(argv[a + 1]);
	starts = fsm_hip_pos_dfa_create(dfa);
	fsm_hip_dfa_free(dfa);
	if (starts == NULL) {
		perror("fsm_hip_pos_dfa_create");
		return 2;
	}
	dfa = read_dfa(argv[a + 2]);
	ends = fsm_hip_tok_dfa_create(dfa, FSM_HIP_IDS_EARLIEST);
	fsm_hip_dfa_free(dfa);
	if (ends == NULL) {
		perror("fsm_hip_tok_dfa_create");
		return 2;
	}

	/* the table: R[i] = rbytes[roff[i], roff[i + 1]) */
	nrepl = (size_t)(sep - a - 3);
	roff = malloc((nrepl + 1) * sizeof *roff);
	for (j = 0; j < nrepl; j++) {
		rlen += strlen(argv[a + 3 + j]);
	}
	rbytes = malloc(rlen + 1);
	if (roff == NULL || rbytes == NULL) {
		perror("malloc");
		return 2;
	}
	roff[0] = 0;
	if (!tmpl) {
		for (j = 0; j < nrepl; j++) {
			memcpy(rbytes + roff[j], argv[a + 3 + j], strlen(argv[a + 3 + j]));
			roff[j + 1] = roff[j] + strlen(argv[a + 3 + j]);
		}
		repl = fsm_hip_repl_create(rbytes, roff, nrepl, flags);
	} else {
		/* -t: the literal bytes of every REPL, and per & the count of literal bytes in front of it (no REPL has more of
		 * either than it has bytes) */
		ioff = malloc((nrepl + 1) * sizeof *ioff);
		ins = malloc((rlen + 1) * sizeof *ins);
		if (ioff == NULL || ins == NULL) {
			perror("malloc");
			return 2;
		}
		ioff[0] = 0;
		for (j = 0; j < nrepl; j++) {
			arg = argv[a + 3 + j];
			roff[j + 1] = roff[j];
			ioff[j + 1] = ioff[j];
			for (k = 0; arg[k] != '\0'; k++) {
				if (arg[k] == '&') {
					ins[ioff[j + 1]++] = roff[j + 1] - roff[j];
					continue;
				}
				if (arg[k] == '\\' && arg[k + 1] == '\0') {
					fprintf(stderr, "hipsed: REPL %zu ends in a backslash\n", j + 1);
					return 2;
				}
				if (arg[k] == '\\' && (arg[k + 1] == '&' || arg[k + 1] == '\\')) {
					k++;
				}
				rbytes[roff[j + 1]++] = (unsigned char)arg[k];
			}
		}
		repl = fsm_hip_repl_create_template(rbytes, roff, nrepl, ins, ioff, 0);
	}
	if (repl == NULL) {
		perror(tmpl ? "fsm_hip_repl_create_template" : "fsm_hip_repl_create");
		return 2;
	}

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]); a line ends where its file ends */
	names = argv + sep + 1;
	nfiles = (size_t)(argc - sep - 1);
	file_off = malloc((nfiles + 1) * sizeof *file_off);
	if (file_off == NULL) {
		perror("malloc");
		return 2;
	}
	for (j = 0; j < nfiles; j++) {
		file_off[j] = len;
		f = fopen(names[j], "rb");
		if (f == NULL) {
			perror(names[j]);
			return 2;
		}
		for (;;) {
			if (cap - len < 65536) {
				cap = cap ? cap * 2 : 1 << 20;
				buf = realloc(buf, cap);
				if (buf == NULL) {
					perror("realloc");
					return 2;
				}
			}
			got = fread(buf + len, 1, cap - len, f);
			if (got == 0) {
				break;
			}
			len += got;
		}
		fclose(f);
	}
	file_off[nfiles] = len;

	text = fsm_hip_text_open_files(buf, len, '\n', file_off, nfiles);
	if (text == NULL) {
		perror("fsm_hip_text_open_files");
		return 2;
	}
	hits = fsm_hip_text_hits(ld, text, FSM_HIP_HITS_NO_BYTES);     /* for the exit status alone */
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	nhits = fsm_hip_text_hits_count(hits);
	matches = fsm_hip_text_matches(starts, ends, text, NULL, 0, NULL);   /* every match of every line; empty ones insert */
	if (matches == NULL) {
		perror("fsm_hip_text_matches");
		return 2;
	}
	replaced = fsm_hip_text_replace(matches, text, NULL, repl, NULL);     /* the new text, on the device */
	if (replaced == NULL) {
		perror("fsm_hip_text_replace");
		return 2;
	}
	nout = fsm_hip_replaced_nbytes(replaced);
	if (nout != 0) {
		out = malloc((size_t)nout);
		if (out == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_replaced_copy(replaced, NULL, out) != 0) {
			perror("fsm_hip_replaced_copy");
			return 2;
		}
		if (fwrite(out, 1, (size_t)nout, stdout) != (size_t)nout) {
			perror("stdout");
			return 2;
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_replaced_free(replaced);
	fsm_hip_matches_free(matches);
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_repl_free(repl);
	fsm_hip_tok_dfa_free(ends);
	fsm_hip_pos_dfa_free(starts);
	fsm_hip_lines_dfa_free(ld);
	free(file_off);
	free(roff);
	free(ioff);
	free(ins);
	free(rbytes);
	free(out);
	free(buf);
	return nhits != 0 ? 0 : 1;
}
