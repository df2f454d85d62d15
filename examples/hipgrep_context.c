/*
 * examples/hipgrep_context.c -- the lines around a match: what grep -H prints with -A, -B or -C, with no host loop over all lines:
 *
 *     hipgrep_context [-A N] [-B N] [-C N] [-n] [-v] TABLE.fsmhip FILE...
 *
 * The files are one text (fsm_hip_text_open_files, as examples/hipgrep_files.c); fsm_hip_text_hits_context() walks it, widens
 * the selected lines by N lines before / after inside each file on the device, and leaves the hits with two marks:
 *     core   the hit is a selected line: NAME:line (NAME:number:line under -n); a context line gets '-' in place of ':'
 *     group  the hit is not the successor of the hit before it, or begins another file: "--" goes before it, except before the first
 * The host loop runs over files and hits only.  A line without a final '\n' gets one.
 *     -A N / -B N / -C N   N lines after / before / both (any N up to 2^64 - 1: "the whole file")
 *     -n                   line numbers from 1 in each file
 *     -v                   select the lines that do NOT match, then widen
 * Exit status: 0 if a line was selected, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

static int
number_of(const char *s, uint64_t *out)
{
	char *end;

	if (s == NULL || *s < '0' || *s > '9') {
		return -1;
	}
	errno = 0;
	*out = strtoull(s, &end, 10);
	return errno != 0 || *end != '\0' ? -1 : 0;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	unsigned char *buf = NULL, *out = NULL;
	uint64_t *file_off, *file_lines, *file_first, *lines = NULL, *off = NULL, *core = NULL, *group = NULL;
	uint64_t before = 0, after = 0, num;
	size_t cap = 0, len = 0, got, m, nbytes, nfiles, j, k;
	unsigned flags = 0;
	int number = 0, a;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-v") == 0) {
			flags |= FSM_HIP_HITS_INVERT;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else if ((strcmp(argv[a], "-A") == 0 || strcmp(argv[a], "-B") == 0 || strcmp(argv[a], "-C") == 0) &&
		           a + 1 < argc && number_of(argv[a + 1], &num) == 0) {
			if (argv[a][1] != 'B') {
				after = num;
			}
			if (argv[a][1] != 'A') {
				before = num;
			}
			a++;
		} else {
			a = argc;
		}
	}
	if (a + 2 > argc) {
		fprintf(stderr, "usage: hipgrep_context [-A N] [-B N] [-C N] [-n] [-v] TABLE.fsmhip FILE...\n");
		return 2;
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
	file_lines = malloc((nfiles + 1) * sizeof *file_lines);
	file_first = malloc((nfiles + 1) * sizeof *file_first);
	if (file_off == NULL || file_lines == NULL || file_first == NULL) {
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
	hits = fsm_hip_text_hits_context(ld, text, flags, before, after);
	if (hits == NULL) {
		perror("fsm_hip_text_hits_context");
		return 2;
	}
	m = fsm_hip_text_hits_count(hits);
	nbytes = fsm_hip_text_hits_nbytes(hits);
	if (m != 0) {
		out = malloc(nbytes);
		off = malloc((m + 1) * sizeof *off);
		lines = malloc(m * sizeof *lines);
		core = malloc((m + 63) / 64 * sizeof *core);
		group = malloc((m + 63) / 64 * sizeof *group);
		if (out == NULL || off == NULL || lines == NULL || core == NULL || group == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, off, out) != 0 || fsm_hip_text_hits_marks(hits, core, group) != 0 ||
		    fsm_hip_text_hits_file_first(hits, file_first) != 0 || fsm_hip_text_file_lines(text, file_lines) != 0) {
			perror("fsm_hip_text_hits_copy");
			return 2;
		}
		for (j = 0; j < nfiles; j++) {
			for (k = (size_t)file_first[j]; k < (size_t)file_first[j + 1]; k++) {
				const int sep = (core[k / 64] >> (k % 64) & 1) != 0 ? ':' : '-';
				if (k != 0 && (group[k / 64] >> (k % 64) & 1) != 0) {
					fputs("--\n", stdout);
				}
				fputs(names[j], stdout);
				putchar(sep);
				if (number) {
					printf("%llu%c", (unsigned long long)(lines[k] - file_lines[j]) + 1, sep);
				}
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
	free(file_lines);
	free(file_first);
	free(lines);
	free(off);
	free(core);
	free(group);
	free(out);
	free(buf);
	return m ? 0 : 1;
}
