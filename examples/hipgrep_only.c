/*
 * examples/hipgrep_only.c -- the matching PARTS of the lines of many files: what grep -o prints, with no host loop over bytes:
 *
 *     hipgrep_only [-b] [-n] [-H] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...
 *
 * Three tables: LINES selects the lines (.*(pat).* -- fsm_hip_text_hits, as hipgrep_files.c), STARTS accepts anything followed
 * by the reversal of pat, ENDS accepts exactly pat.  fsm_hip_text_hits_spans() walks STARTS backward and ENDS forward over every
 * hit on the device and leaves the leftmost-longest match of each; fsm_hip_text_spans_next() moves every hit behind its match
 * and walks again.  The loop over ROUNDS is on the host, and it ends when fsm_hip_text_spans_count() says that no hit has a
 * match left; the rounds' spans are kept and printed hit by hit, so the output is in grep's order.
 *     (default)  every non-empty match on a line of its own
 *     -b         the 0-based byte offset of the match in its file before it
 *     -n         the number of its line in its file, from 1, before that
 *     -H         the file's name before everything
 * Exit status: 0 if a match was printed, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

static struct fsm_hip_dfa_desc *
read_table(const char *path)
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

static struct fsm_hip_pos_dfa *
read_image(const char *path)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_pos_dfa *pd;

	desc = read_table(path);
	dfa = fsm_hip_dfa_create(desc, FSM_HIP_DEFER_UPLOAD);   /* planned only: the image below is all that goes to the device */
	fsm_hip_desc_free(desc);
	if (dfa == NULL) {
		perror("fsm_hip_dfa_create");
		exit(2);
	}
	pd = fsm_hip_pos_dfa_create(dfa);
	fsm_hip_dfa_free(dfa);
	if (pd == NULL) {
		perror("fsm_hip_pos_dfa_create");
		exit(2);
	}
	return pd;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_pos_dfa *starts, *ends;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	struct fsm_hip_text_spans *spans;
	unsigned char *buf = NULL, *out = NULL;
	uint64_t *file_off, *file_lines, *file_first, *lines = NULL, *off = NULL, *text_off = NULL, **rs = NULL, **re = NULL;
	size_t cap = 0, len = 0, got, m, nfiles, j, k, r, rounds = 0, printed = 0;
	int bytes = 0, number = 0, name = 0, a;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-b") == 0) {
			bytes = 1;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else if (strcmp(argv[a], "-H") == 0) {
			name = 1;
		} else {
			a = argc;
		}
	}
	if (a + 4 > argc) {
		fprintf(stderr, "usage: hipgrep_only [-b] [-n] [-H] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...\n");
		return 2;
	}
	desc = read_table(argv[a]);
	ld = fsm_hip_lines_dfa_create(desc, '\n', 0);
	fsm_hip_desc_free(desc);
	if (ld == NULL) {
		perror("fsm_hip_lines_dfa_create");
		return 2;
	}
	starts = read_image(argv[a + 1]);
	ends = read_image(argv[a + 2]);

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]) */
	names = argv + a + 3;
	nfiles = (size_t)(argc - a - 3);
	file_off = malloc((nfiles + 1) * sizeof *file_off);
	file_first = malloc((nfiles + 1) * sizeof *file_first);
	file_lines = malloc((nfiles + 1) * sizeof *file_lines);
	if (file_off == NULL || file_first == NULL || file_lines == NULL) {
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
	hits = fsm_hip_text_hits(ld, text, 0);
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	m = fsm_hip_text_hits_count(hits);
	if (m != 0) {
		out = malloc(fsm_hip_text_hits_nbytes(hits));
		off = malloc((m + 1) * sizeof *off);
		lines = malloc(m * sizeof *lines);
		text_off = malloc((fsm_hip_text_lines(text) + 1) * sizeof *text_off);
		if (out == NULL || off == NULL || lines == NULL || text_off == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, off, out) != 0 || fsm_hip_text_hits_file_first(hits, file_first) != 0 ||
		    fsm_hip_text_file_lines(text, file_lines) != 0 || fsm_hip_text_offsets(text, text_off) != 0) {
			perror("fsm_hip_text_hits_copy");
			return 2;
		}
		/* the rounds: one match of every hit each, until no hit has one */
		spans = fsm_hip_text_hits_spans(hits, text, starts, ends, NULL);
		if (spans == NULL) {
			perror("fsm_hip_text_hits_spans");
			return 2;
		}
		while (fsm_hip_text_spans_count(spans) != 0) {
			rs = realloc(rs, (rounds + 1) * sizeof *rs);
			re = realloc(re, (rounds + 1) * sizeof *re);
			if (rs == NULL || re == NULL || (rs[rounds] = malloc(m * sizeof **rs)) == NULL || (re[rounds] = malloc(m * sizeof **re)) == NULL) {
				perror("malloc");
				return 2;
			}
			if (fsm_hip_text_spans_copy(spans, rs[rounds], re[rounds]) != 0 || fsm_hip_text_spans_next(spans) != 0) {
				perror("fsm_hip_text_spans_next");
				return 2;
			}
			rounds++;
		}
		fsm_hip_text_spans_free(spans);
		for (j = 0; j < nfiles; j++) {
			for (k = (size_t)file_first[j]; k < (size_t)file_first[j + 1]; k++) {
				for (r = 0; r < rounds && rs[r][k] != FSM_HIP_NO_POS; r++) {
					if (re[r][k] == rs[r][k]) {
						continue;                   /* an empty match: dropped, as grep does */
					}
					if (name) {
						printf("%s:", names[j]);
					}
					if (number) {
						printf("%llu:", (unsigned long long)(lines[k] - file_lines[j]) + 1);
					}
					if (bytes) {
						printf("%llu:", (unsigned long long)(text_off[lines[k]] - file_off[j] + rs[r][k]));
					}
					fwrite(out + off[k] + rs[r][k], 1, (size_t)(re[r][k] - rs[r][k]), stdout);
					putchar('\n');
					printed++;
				}
			}
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	for (r = 0; r < rounds; r++) {
		free(rs[r]);
		free(re[r]);
	}
	free(rs);
	free(re);
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_pos_dfa_free(starts);
	fsm_hip_pos_dfa_free(ends);
	fsm_hip_lines_dfa_free(ld);
	free(file_off);
	free(file_first);
	free(file_lines);
	free(lines);
	free(off);
	free(text_off);
	free(out);
	free(buf);
	return printed ? 0 : 1;
}
