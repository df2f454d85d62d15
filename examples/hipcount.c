/*
 * examples/hipcount.c -- how often every rule of a union matches in every file, and in how many lines, counted on the device: no
 * host loop over matches, and neither the matches' ids nor their offsets leave the device:
 *
 *     hipcount [-t] [-r NRULES] STARTS.fsmhip ENDS.fsmhip FILE...
 *
 * The two tables are hipscan's (examples/hipscan.c): STARTS accepts anything followed by the reversal of pat, ENDS accepts exactly
 * pat and carries one end-id per rule.  fsm_hip_text_matches() finds every non-empty match of every line in one call and
 * fsm_hip_matches_tally() counts them per file and per rule: the groups are the text's file_lines, the one array of nfiles + 1
 * entries that the host hands on.  Printed is
 *     file:rule:matches:lines
 * one line per file and rule with a match, in the order of the files and of the rules; `lines` is what grep -c prints for that
 * rule alone.  Matches whose state carries no id, or an id of NRULES or above, are the rule "other".
 *     -t         totals over all files: rule:matches:lines (a line counts once, a file's name is not printed)
 *     -r NRULES  the rules 0 .. NRULES - 1 have a column of their own; default: the largest end-id of ENDS + 1
 * Exit status: 0 if a match was counted, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
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

static void
print_rule(size_t c, size_t nrules)
{
	if (c < nrules) {
		printf("%zu", c);
	} else {
		printf("other");
	}
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_pos_dfa *starts;
	struct fsm_hip_tok_dfa *ends;
	struct fsm_hip_text *text;
	struct fsm_hip_matches *matches;
	unsigned char *buf = NULL;
	uint64_t *file_off, *file_lines, *count, *lines;
	size_t cap = 0, len = 0, got, nfiles, nrules = 0, ngroups, C, j, c, k;
	int totals = 0, have_rules = 0, any = 0, a;
	unsigned long v;
	char *end;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-t") == 0) {
			totals = 1;
		} else if (strcmp(argv[a], "-r") == 0 && a + 1 < argc) {
			errno = 0;
			v = strtoul(argv[++a], &end, 10);
			if (end == argv[a] || *end != '\0' || errno != 0 || v > 1000000ul) {
				fprintf(stderr, "hipcount: -r takes a number of rules\n");
				return 2;
			}
			nrules = (size_t)v;
			have_rules = 1;
		} else {
			a = argc;
		}
	}
	if (a + 3 > argc) {
		fprintf(stderr, "usage: hipcount [-t] [-r NRULES] STARTS.fsmhip ENDS.fsmhip FILE...\n");
		return 2;
	}
	desc = read_desc(argv[a]);
	dfa = fsm_hip_dfa_create(desc, FSM_HIP_DEFER_UPLOAD);   /* planned only: the images are all that goes to the device */
	fsm_hip_desc_free(desc);
	starts = dfa != NULL ? fsm_hip_pos_dfa_create(dfa) : NULL;
	fsm_hip_dfa_free(dfa);
	if (starts == NULL) {
		perror("fsm_hip_pos_dfa_create");
		return 2;
	}
	desc = read_desc(argv[a + 1]);
	if (!have_rules && desc->endid_off != NULL) {           /* over the description's ids, not over matches */
		for (k = 0; k < desc->endid_off[desc->nstates]; k++) {
			if ((size_t)desc->endids[k] + 1 > nrules) {
				nrules = (size_t)desc->endids[k] + 1;
			}
		}
	}
	dfa = fsm_hip_dfa_create(desc, FSM_HIP_DEFER_UPLOAD);
	fsm_hip_desc_free(desc);
	ends = dfa != NULL ? fsm_hip_tok_dfa_create(dfa, FSM_HIP_IDS_EARLIEST) : NULL;
	fsm_hip_dfa_free(dfa);
	if (ends == NULL) {
		perror("fsm_hip_tok_dfa_create");
		return 2;
	}

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]); a line ends where its file ends */
	names = argv + a + 2;
	nfiles = (size_t)(argc - a - 2);
	ngroups = totals ? 1 : nfiles;
	C = nrules + 1;
	file_off = malloc((nfiles + 1) * sizeof *file_off);
	file_lines = malloc((nfiles + 1) * sizeof *file_lines);
	count = malloc(ngroups * C * sizeof *count);
	lines = malloc(ngroups * C * sizeof *lines);
	if (file_off == NULL || file_lines == NULL || count == NULL || lines == NULL) {
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
	matches = fsm_hip_text_matches(starts, ends, text, NULL, FSM_HIP_MATCHES_DROP_EMPTY, NULL);   /* as grep: no empty match */
	if (matches == NULL) {
		perror("fsm_hip_text_matches");
		return 2;
	}
	if (fsm_hip_text_file_lines(text, file_lines) != 0) {
		perror("fsm_hip_text_file_lines");
		return 2;
	}
	/* the counting: one call, the tables of nfiles x (nrules + 1) entries are all that comes back */
	if (fsm_hip_matches_tally(matches, totals ? NULL : file_lines, ngroups, nrules, 0, count, lines) != 0) {
		perror("fsm_hip_matches_tally");
		return 2;
	}
	for (j = 0; j < ngroups; j++) {
		for (c = 0; c < C; c++) {
			if (count[j * C + c] == 0) {
				continue;
			}
			any = 1;
			if (!totals) {
				printf("%s:", names[j]);
			}
			print_rule(c, nrules);
			printf(":%llu:%llu\n", (unsigned long long)count[j * C + c], (unsigned long long)lines[j * C + c]);
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_matches_free(matches);
	fsm_hip_text_free(text);
	fsm_hip_tok_dfa_free(ends);
	fsm_hip_pos_dfa_free(starts);
	free(file_off);
	free(file_lines);
	free(count);
	free(lines);
	free(buf);
	return any ? 0 : 1;
}
