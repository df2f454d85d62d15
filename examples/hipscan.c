/*
 * examples/hipscan.c -- every match of a union of rules in the lines of many files, and which rule it was, from ONE call: no
 * host loop over bytes and none over rounds (examples/hipgrep_only.c has that one):
 *
 *     hipscan [-e] [-b] [-n] [-H] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...
 *
 * Three tables: LINES selects the lines (.*(pat).* -- fsm_hip_text_hits, as hipgrep_files.c), STARTS accepts anything followed
 * by the reversal of pat, ENDS accepts exactly pat and carries one end-id per rule ("starts and ends with
 * end-ids").  fsm_hip_text_matches() walks STARTS backward once over every hit, then ENDS forward from mark to mark, and leaves
 * start, end and id of every match on the device.  One line of output per match:
 *     LINE:START-END:ID
 * LINE the number of the line in the whole input, from 1; START and END byte positions in the line; ID the lowest end-id of the
 * state the match ended in (a lower id is a higher rule priority), `-` for a state without one.
 *     -e         keep empty matches (by default FSM_HIP_MATCHES_DROP_EMPTY drops them, as grep does)
 *     -b         START and END are 0-based byte offsets in the file
 *     -n         LINE is the number of the line in its file
 *     -H         the file's name before everything
 * Exit status: 0 if a match was printed, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

static struct fsm_hip_dfa *
read_dfa(const char *path)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
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
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	struct fsm_hip_matches *matches;
	unsigned char *buf = NULL;
	uint64_t *file_off, *file_lines, *file_first, *lines = NULL, *text_off = NULL, *off = NULL, *start = NULL, *end = NULL, add;
	uint32_t *id = NULL;
	size_t cap = 0, len = 0, got, m, total, nfiles, j, k, t, printed = 0;
	unsigned flags = FSM_HIP_MATCHES_DROP_EMPTY;
	int bytes = 0, number = 0, name = 0, a;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-e") == 0) {
			flags = 0;
		} else if (strcmp(argv[a], "-b") == 0) {
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
		fprintf(stderr, "usage: hipscan [-e] [-b] [-n] [-H] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...\n");
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
	hits = fsm_hip_text_hits(ld, text, FSM_HIP_HITS_NO_BYTES);     /* the matches read the text itself */
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	matches = fsm_hip_text_matches(starts, ends, text, hits, flags, NULL);   /* every match of every hit: one call */
	if (matches == NULL) {
		perror("fsm_hip_text_matches");
		return 2;
	}
	m = fsm_hip_matches_count(matches);
	total = fsm_hip_matches_total(matches);
	if (total != 0) {
		lines = malloc(m * sizeof *lines);
		text_off = malloc((fsm_hip_text_lines(text) + 1) * sizeof *text_off);
		off = malloc((m + 1) * sizeof *off);
		start = malloc(total * sizeof *start);
		end = malloc(total * sizeof *end);
		id = malloc(total * sizeof *id);
		if (lines == NULL || text_off == NULL || off == NULL || start == NULL || end == NULL || id == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, NULL, NULL) != 0 || fsm_hip_text_hits_file_first(hits, file_first) != 0 ||
		    fsm_hip_text_file_lines(text, file_lines) != 0 || fsm_hip_text_offsets(text, text_off) != 0 ||
		    fsm_hip_matches_copy(matches, off, start, end, id) != 0) {
			perror("fsm_hip_matches_copy");
			return 2;
		}
		for (j = 0; j < nfiles; j++) {
			for (k = (size_t)file_first[j]; k < (size_t)file_first[j + 1]; k++) {
				add = bytes ? text_off[lines[k]] - file_off[j] : 0;
				for (t = (size_t)off[k]; t < (size_t)off[k + 1]; t++) {
					if (name) {
						printf("%s:", names[j]);
					}
					printf("%llu:%llu-%llu:", (unsigned long long)(lines[k] - (number ? file_lines[j] : 0)) + 1,
					       (unsigned long long)(start[t] + add), (unsigned long long)(end[t] + add));
					if (id[t] == FSM_HIP_NO_ID) {
						printf("-\n");
					} else {
						printf("%lu\n", (unsigned long)id[t]);
					}
					printed++;
				}
			}
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_matches_free(matches);
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_tok_dfa_free(ends);
	fsm_hip_pos_dfa_free(starts);
	fsm_hip_lines_dfa_free(ld);
	free(file_off);
	free(file_first);
	free(file_lines);
	free(lines);
	free(text_off);
	free(off);
	free(start);
	free(end);
	free(id);
	free(buf);
	return printed ? 0 : 1;
}
