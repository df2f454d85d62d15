/*
 * examples/hipextract.c -- the matching PARTS of the lines of many files, what grep -o prints, gathered on the device: no host
 * loop over bytes and no host round per match:
 *
 *     hipextract [-b] [-n] [-H] [-r LIST] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...
 *
 * The three tables are hipscan's (examples/hipscan.c): LINES selects the lines that hold a match, STARTS accepts anything followed
 * by the reversal of pat, ENDS accepts exactly pat and carries one end-id per rule.  fsm_hip_text_matches() finds every non-empty
 * match of every hit in one call, fsm_hip_text_extract() packs the matched bytes, each followed by '\n', into one text on the
 * device, and that text is copied out and written with one fwrite.  (examples/hipgrep_only.c prints the same from the spans'
 * rounds, one host round per match.)
 *     -r LIST    keep the matches of these rules alone: numbers from 0, separated by commas; a match whose state has no id is
 *                not kept then
 *     -b         the 0-based byte offset of the match in its file before it
 *     -n         the number of its line in its file, from 1, before that
 *     -H         the file's name before everything
 * With a prefix the records are written one by one, from the same packed text; line[] and match[] of the extracted object say
 * where each came from.  Exit status: 0 if a match was printed, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
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

/* "0,3,17" -> the set's bitmap and *nrules = the largest number + 1 */
static unsigned char *
read_rules(const char *list, size_t *nrules)
{
	unsigned char *bits = NULL;
	size_t nbytes = 0, want;
	unsigned long v;
	char *end;

	*nrules = 0;
	while (*list != '\0') {
		errno = 0;
		v = strtoul(list, &end, 10);
		if (end == list || errno != 0 || v >= 0xFFFFFFFEul || (*end != ',' && *end != '\0')) {
			fprintf(stderr, "hipextract: -r takes numbers separated by commas\n");
			exit(2);
		}
		want = (size_t)v / 8 + 1;
		if (want > nbytes) {
			bits = realloc(bits, want);
			if (bits == NULL) {
				perror("realloc");
				exit(2);
			}
			memset(bits + nbytes, 0, want - nbytes);
			nbytes = want;
		}
		bits[v / 8] |= (unsigned char)(1u << (v % 8));
		if ((size_t)v + 1 > *nrules) {
			*nrules = (size_t)v + 1;
		}
		list = *end == ',' ? end + 1 : end;
	}
	return bits;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_pos_dfa *starts;
	struct fsm_hip_tok_dfa *ends;
	struct fsm_hip_rules *keep = NULL;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	struct fsm_hip_matches *matches;
	struct fsm_hip_extracted *extracted;
	unsigned char *buf = NULL, *out = NULL, *bits;
	uint64_t *file_off, *file_lines = NULL, *file_first = NULL, *lines = NULL, *text_off = NULL, *off = NULL, *rline = NULL, *rmatch = NULL,
	         *start = NULL, nout;
	size_t cap = 0, len = 0, got, nfiles, nrules, j, r, nrec, m, total;
	int bytes = 0, number = 0, name = 0, a;
	const char *rules = NULL;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-b") == 0) {
			bytes = 1;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else if (strcmp(argv[a], "-H") == 0) {
			name = 1;
		} else if (strcmp(argv[a], "-r") == 0 && a + 1 < argc) {
			rules = argv[++a];
		} else {
			a = argc;
		}
	}
	if (a + 4 > argc) {
		fprintf(stderr, "usage: hipextract [-b] [-n] [-H] [-r LIST] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...\n");
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
	if (rules != NULL) {
		bits = read_rules(rules, &nrules);
		keep = fsm_hip_rules_create(bits, nrules, 0);
		free(bits);
		if (keep == NULL) {
			perror("fsm_hip_rules_create");
			return 2;
		}
	}

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]); a line ends where its file ends */
	names = argv + a + 3;
	nfiles = (size_t)(argc - a - 3);
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
	hits = fsm_hip_text_hits(ld, text, FSM_HIP_HITS_NO_BYTES);      /* the lines' numbers alone: the text itself is read */
	if (hits == NULL) {
		perror("fsm_hip_text_hits");
		return 2;
	}
	matches = fsm_hip_text_matches(starts, ends, text, hits, FSM_HIP_MATCHES_DROP_EMPTY, NULL);   /* as grep: no empty match */
	if (matches == NULL) {
		perror("fsm_hip_text_matches");
		return 2;
	}
	extracted = fsm_hip_text_extract(matches, text, hits, keep, '\n', NULL);    /* the matched bytes, gathered on the device */
	if (extracted == NULL) {
		perror("fsm_hip_text_extract");
		return 2;
	}
	nrec = fsm_hip_extracted_count(extracted);
	nout = fsm_hip_extracted_nbytes(extracted);
	if (nrec != 0) {
		out = malloc((size_t)nout);
		if (out == NULL) {
			perror("malloc");
			return 2;
		}
		if (!name && !number && !bytes) {
			if (fsm_hip_extracted_copy(extracted, NULL, out, NULL, NULL) != 0) {
				perror("fsm_hip_extracted_copy");
				return 2;
			}
			if (fwrite(out, 1, (size_t)nout, stdout) != (size_t)nout) {
				perror("stdout");
				return 2;
			}
		} else {
			m = fsm_hip_text_hits_count(hits);
			total = fsm_hip_matches_total(matches);
			off = malloc((nrec + 1) * sizeof *off);
			rline = malloc(nrec * sizeof *rline);
			rmatch = malloc(nrec * sizeof *rmatch);
			start = malloc(total * sizeof *start);
			lines = malloc(m * sizeof *lines);
			text_off = malloc((fsm_hip_text_lines(text) + 1) * sizeof *text_off);
			file_first = malloc((nfiles + 1) * sizeof *file_first);
			file_lines = malloc((nfiles + 1) * sizeof *file_lines);
			if (off == NULL || rline == NULL || rmatch == NULL || start == NULL || lines == NULL || text_off == NULL || file_first == NULL ||
			    file_lines == NULL) {
				perror("malloc");
				return 2;
			}
			if (fsm_hip_extracted_copy(extracted, off, out, rline, rmatch) != 0 || fsm_hip_matches_copy(matches, NULL, start, NULL, NULL) != 0 ||
			    fsm_hip_text_hits_copy(hits, lines, NULL, NULL) != 0 || fsm_hip_text_hits_file_first(hits, file_first) != 0 ||
			    fsm_hip_text_file_lines(text, file_lines) != 0 || fsm_hip_text_offsets(text, text_off) != 0) {
				perror("fsm_hip_extracted_copy");
				return 2;
			}
			/* the records are in the order of the hits, and so are the files */
			for (r = 0, j = 0; r < nrec; r++) {
				while (j + 1 < nfiles && rline[r] >= file_first[j + 1]) {
					j++;
				}
				if (name) {
					printf("%s:", names[j]);
				}
				if (number) {
					printf("%llu:", (unsigned long long)(lines[rline[r]] - file_lines[j]) + 1);
				}
				if (bytes) {
					printf("%llu:", (unsigned long long)(text_off[lines[rline[r]]] - file_off[j] + start[rmatch[r]]));
				}
				fwrite(out + off[r], 1, (size_t)(off[r + 1] - off[r]), stdout);
			}
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_extracted_free(extracted);
	fsm_hip_matches_free(matches);
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_rules_free(keep);
	fsm_hip_tok_dfa_free(ends);
	fsm_hip_pos_dfa_free(starts);
	fsm_hip_lines_dfa_free(ld);
	free(file_off);
	free(file_first);
	free(file_lines);
	free(lines);
	free(text_off);
	free(off);
	free(rline);
	free(rmatch);
	free(start);
	free(out);
	free(buf);
	return nrec != 0 ? 0 : 1;
}
