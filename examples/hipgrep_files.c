/*
 * examples/hipgrep_files.c -- many files in ONE text: what grep -H prints, with no host loop over bytes or over all lines:
 *
 *     hipgrep_files [-c | -l | -L] [-n] [-v] TABLE.fsmhip FILE...
 *
 * The files are read back to back into one buffer with nothing between them; fsm_hip_text_open_files() cuts the lines at every
 * delimiter AND at every file end (a file without a final '\n' does not glue its last line to the next file's first),
 * fsm_hip_text_hits() walks them and leaves the selected lines packed on the device, and file_first says which hits are whose:
 * the hits of file j are [file_first[j], file_first[j + 1]).  The host loop runs over files and hits only.
 *     (default)  FILE:line for every matching line (a line without '\n' gets one)
 *     -n         FILE:number:line, numbers from 1 in each file
 *     -c         FILE:count for every file (FSM_HIP_HITS_NO_BYTES: nothing is gathered)
 *     -l / -L    the names of the files with / without a selected line
 *     -v         select the lines that do NOT match
 * Exit status: 0 if a line was selected (-L: if a file was listed), 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
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
	uint64_t *file_off, *file_lines = NULL, *file_first, *lines = NULL, *off = NULL;
	size_t cap = 0, len = 0, got, m, nbytes, nfiles, j, k, listed = 0;
	unsigned flags = 0;
	int mode = 0, number = 0, a;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-v") == 0) {
			flags |= FSM_HIP_HITS_INVERT;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else if ((strcmp(argv[a], "-c") == 0 || strcmp(argv[a], "-l") == 0 || strcmp(argv[a], "-L") == 0) && mode == 0) {
			mode = argv[a][1];
		} else {
			a = argc;
		}
	}
	if (a + 2 > argc) {
		fprintf(stderr, "usage: hipgrep_files [-c | -l | -L] [-n] [-v] TABLE.fsmhip FILE...\n");
		return 2;
	}
	if (mode != 0) {
		flags |= FSM_HIP_HITS_NO_BYTES;
	}
	f = fopen(argv[a], "rb");
	if (f == NULL) {
		perror(argv[a]);
		return 2;
	}
	desc = fsm_hip_desc_read(f);
	fclose(f);
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

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]) */
	names = argv + a + 1;
	nfiles = (size_t)(argc - a - 1);
	file_off = malloc((nfiles + 1) * sizeof *file_off);
	file_first = malloc((nfiles + 1) * sizeof *file_first);
	if (file_off == NULL || file_first == NULL) {
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
	hits = fsm_hip_text_hits(ld, text, flags);
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	m = fsm_hip_text_hits_count(hits);
	nbytes = fsm_hip_text_hits_nbytes(hits);
	if (fsm_hip_text_hits_file_first(hits, file_first) != 0) {
		perror("fsm_hip_text_hits_file_first");
		return 2;
	}
	if (mode != 0) {
		for (j = 0; j < nfiles; j++) {
			const size_t c = (size_t)(file_first[j + 1] - file_first[j]);
			if (mode == 'c') {
				printf("%s:%zu\n", names[j], c);
			} else if ((c != 0) == (mode == 'l')) {
				printf("%s\n", names[j]);
				listed++;
			}
		}
	} else if (m != 0) {
		out = malloc(nbytes);
		off = malloc((m + 1) * sizeof *off);
		if (number) {
			lines = malloc(m * sizeof *lines);
			file_lines = malloc((nfiles + 1) * sizeof *file_lines);
		}
		if (out == NULL || off == NULL || (number && (lines == NULL || file_lines == NULL))) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, off, out) != 0 || (number && fsm_hip_text_file_lines(text, file_lines) != 0)) {
			perror("fsm_hip_text_hits_copy");
			return 2;
		}
		for (j = 0; j < nfiles; j++) {
			for (k = (size_t)file_first[j]; k < (size_t)file_first[j + 1]; k++) {
				fputs(names[j], stdout);
				if (number) {
					printf(":%llu", (unsigned long long)(lines[k] - file_lines[j]) + 1);
				}
				putchar(':');
				fwrite(out + off[k], 1, (size_t)(off[k + 1] - off[k]), stdout);
				if (out[off[k + 1] - 1] != '\n') {   /* a file's last line without a delimiter: every line has a byte */
					putchar('\n');
				}
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
	free(file_off);
	free(file_first);
	free(file_lines);
	free(lines);
	free(off);
	free(out);
	free(buf);
	if (mode == 'L') {
		return listed ? 0 : 1;
	}
	return m ? 0 : 1;
}
