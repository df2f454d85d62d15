/*
 * examples/hipgrep_print.c -- print the matching lines themselves, with no host loop over answers or offsets:
 *
 *     hipgrep_print [-v] [-c] [-n] TABLE.fsmhip < lines.txt
 *
 * The file is slurped and handed over as it is (hipgrep_text.c); fsm_hip_text_hits() walks it and leaves the selected lines'
 * numbers, output offsets and bytes packed on the device, fsm_hip_text_hits_copy() brings back what is printed.
 *     (default)  the matching lines' bytes, verbatim: one fwrite of the gathered buffer (a last line without '\n' gets none)
 *     -c         the number of matching lines (FSM_HIP_HITS_NO_BYTES: nothing is gathered)
 *     -n         every line prefixed with "<number>:", numbers from 1
 *     -v         the lines that do NOT match
 * Exit status as grep's: 0 if a line was selected, 1 if none, 2 on error.  Plain C against include/fsm_hip.h only.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	unsigned char *buf = NULL, *out = NULL;
	uint64_t *lines = NULL, *off = NULL;
	size_t cap = 0, len = 0, got, m, nbytes, k;
	unsigned flags = 0;
	int count = 0, number = 0, a;
	FILE *tf;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-v") == 0) {
			flags |= FSM_HIP_HITS_INVERT;
		} else if (strcmp(argv[a], "-c") == 0) {
			count = 1;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else {
			a = argc;
		}
	}
	if (a != argc - 1) {
		fprintf(stderr, "usage: hipgrep_print [-v] [-c] [-n] TABLE.fsmhip < records\n");
		return 2;
	}
	if (count) {
		flags |= FSM_HIP_HITS_NO_BYTES;
	}
	tf = fopen(argv[a], "rb");
	if (tf == NULL) {
		perror(argv[a]);
		return 2;
	}
	desc = fsm_hip_desc_read(tf);
	fclose(tf);
	if (desc == NULL) {
		perror("fsm_hip_desc_read");
		return 2;
	}
	ld = fsm_hip_lines_dfa_create(desc, '\n', 0);
	fsm_hip_desc_free(desc);
	if (ld == NULL) {
		perror("fsm_hip_lines_dfa_create");
		return 2;
	}

	/* slurp stdin */
	for (;;) {
		if (cap - len < 65536) {
			cap = cap ? cap * 2 : 1 << 20;
			buf = realloc(buf, cap);
			if (buf == NULL) {
				perror("realloc");
				return 2;
			}
		}
		got = fread(buf + len, 1, cap - len, stdin);
		if (got == 0) {
			break;
		}
		len += got;
	}
	text = fsm_hip_text_open(buf, len, '\n');
	if (text == NULL) {
		perror("fsm_hip_text_open");
		return 2;
	}
	hits = fsm_hip_text_hits(ld, text, flags);
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	m = fsm_hip_text_hits_count(hits);
	nbytes = fsm_hip_text_hits_nbytes(hits);
	if (count) {
		printf("%zu\n", m);
	} else if (m != 0) {
		out = malloc(nbytes);
		if (number) {
			lines = malloc(m * sizeof *lines);
			off = malloc((m + 1) * sizeof *off);
		}
		if (out == NULL || (number && (lines == NULL || off == NULL))) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, off, out) != 0) {
			perror("fsm_hip_text_hits_copy");
			return 2;
		}
		if (!number) {
			fwrite(out, 1, nbytes, stdout);
		} else {
			for (k = 0; k < m; k++) {
				printf("%llu:", (unsigned long long)lines[k] + 1);
				fwrite(out + off[k], 1, (size_t)(off[k + 1] - off[k]), stdout);
			}
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_lines_dfa_free(ld);
	free(lines);
	free(off);
	free(out);
	free(buf);
	return m ? 0 : 1;
}
