/*
 * examples/hipuniq.c -- which values match, and how often: grep -o PATTERN FILE... | sort | uniq -c with neither the sort nor a host
 * pass over the matches.  The matches are found, extracted and made distinct on the device; what comes back is one entry per
 * DISTINCT value:
 *
 *     hipuniq [-c] [-s] [-l] [-r LIST] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...
 *
 * The three tables are hipscan's (examples/hipscan.c): LINES selects the lines that hold a match, STARTS accepts anything followed
 * by the reversal of pat, ENDS accepts exactly pat and carries one end-id per rule.  fsm_hip_text_matches() finds every non-empty
 * match of every hit, fsm_hip_text_extract() packs the matched bytes, fsm_hip_extracted_distinct() leaves every distinct value once,
 * with the number of its occurrences.  Printed is
 *     count<TAB>value
 * one line per distinct value, in the order of first appearance.
 *     -c         sorted by count, the most frequent first (ties in the order of first appearance): a host sort over the D
 *                distinct values, not over the matches
 *     -s         in byte order, as sort | uniq -c prints them: fsm_hip_keys_sort() sorts the distinct values on the device and
 *                its order[] and sorted text come back; with -c, by count first and in byte order among equal counts
 *                (FSM_HIP_SORT_BY_COUNT): uniq -c | sort -rn without a host sort
 *     -l         the records are the LINES that hold a match, not the matches: fsm_hip_text_hits_distinct()
 *     -r LIST    the matches of these rules alone: numbers from 0, separated by commas (not with -l)
 * Exit status: 0 if a value was printed, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
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
			fprintf(stderr, "hipuniq: -r takes numbers separated by commas\n");
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

static const uint64_t *sort_count;

/* by count, descending; equal counts by number, which is the order of first appearance */
static int
by_count(const void *a, const void *b)
{
	const size_t x = *(const size_t *)a, y = *(const size_t *)b;

	if (sort_count[x] != sort_count[y]) {
		return sort_count[x] > sort_count[y] ? -1 : 1;
	}
	return x < y ? -1 : x > y;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_dfa_desc *desc;
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_lines_dfa *ld;
	struct fsm_hip_pos_dfa *starts = NULL;
	struct fsm_hip_tok_dfa *ends = NULL;
	struct fsm_hip_rules *keep = NULL;
	struct fsm_hip_text *text;
	struct fsm_hip_text_hits *hits;
	struct fsm_hip_matches *matches = NULL;
	struct fsm_hip_extracted *extracted = NULL;
	struct fsm_hip_distinct *distinct;
	struct fsm_hip_sorted *by_key = NULL;
	unsigned char *buf = NULL, *keys = NULL, *bits;
	uint64_t *file_off, *count = NULL, *doff = NULL, *rec = NULL;
	size_t *order = NULL;
	size_t cap = 0, len = 0, got, nfiles, nrules, j, d, D;
	int by_lines = 0, sorted = 0, by_bytes = 0, a;
	const char *rules = NULL;
	char **names;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-c") == 0) {
			sorted = 1;
		} else if (strcmp(argv[a], "-s") == 0) {
			by_bytes = 1;
		} else if (strcmp(argv[a], "-l") == 0) {
			by_lines = 1;
		} else if (strcmp(argv[a], "-r") == 0 && a + 1 < argc) {
			rules = argv[++a];
		} else {
			a = argc;
		}
	}
	if (a + 4 > argc || (by_lines && rules != NULL)) {
		fprintf(stderr, "usage: hipuniq [-c] [-s] [-l] [-r LIST] LINES.fsmhip STARTS.fsmhip ENDS.fsmhip FILE...\n");
		return 2;
	}
	desc = read_desc(argv[a]);
	ld = fsm_hip_lines_dfa_create(desc, '\n', 0);
	fsm_hip_desc_free(desc);
	if (ld == NULL) {
		perror("fsm_hip_lines_dfa_create");
		return 2;
	}
	if (!by_lines) {
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
	if (by_lines) {
		hits = fsm_hip_text_hits(ld, text, 0);                      /* the lines' bytes, packed on the device */
		if (hits == NULL) {
			perror("fsm_hip_text_hits");
			return 2;
		}
		distinct = fsm_hip_text_hits_distinct(hits, '\n', 0, NULL);
	} else {
		hits = fsm_hip_text_hits(ld, text, FSM_HIP_HITS_NO_BYTES);  /* the lines' numbers alone: the text itself is read */
		if (hits == NULL) {
			perror("fsm_hip_text_hits");
			return 2;
		}
		matches = fsm_hip_text_matches(starts, ends, text, hits, FSM_HIP_MATCHES_DROP_EMPTY, NULL);   /* as grep: no empty match */
		if (matches == NULL) {
			perror("fsm_hip_text_matches");
			return 2;
		}
		extracted = fsm_hip_text_extract(matches, text, hits, keep, '\n', NULL);
		if (extracted == NULL) {
			perror("fsm_hip_text_extract");
			return 2;
		}
		distinct = fsm_hip_extracted_distinct(extracted, '\n', 0, NULL);
	}
	if (distinct == NULL) {
		perror("fsm_hip_distinct");
		return 2;
	}
	D = fsm_hip_distinct_count(distinct);
	if (D != 0) {
		count = malloc(D * sizeof *count);
		doff = malloc((D + 1) * sizeof *doff);
		order = malloc(D * sizeof *order);
		keys = malloc((size_t)fsm_hip_distinct_nbytes(distinct));
		if (count == NULL || doff == NULL || order == NULL || keys == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_distinct_copy(distinct, NULL, count, NULL, doff, keys) != 0) {
			perror("fsm_hip_distinct_copy");
			return 2;
		}
		for (d = 0; d < D; d++) {
			order[d] = d;
		}
		if (by_bytes) {
			/* the sort on the device: record p of its text is key order[p], so the keys and their offsets are replaced by the
			 * sorted ones and only the counts are looked up through order[] */
			by_key = fsm_hip_keys_sort(distinct, '\n', sorted ? FSM_HIP_SORT_BY_COUNT : 0, NULL);
			rec = malloc(D * sizeof *rec);
			if (by_key == NULL || rec == NULL) {
				perror("fsm_hip_keys_sort");
				return 2;
			}
			if (fsm_hip_sorted_copy(by_key, rec, NULL, doff, keys) != 0) {
				perror("fsm_hip_sorted_copy");
				return 2;
			}
			for (d = 0; d < D; d++) {
				printf("%llu\t", (unsigned long long)count[rec[d]]);
				fwrite(keys + doff[d], 1, (size_t)(doff[d + 1] - doff[d]), stdout);
			}
			fsm_hip_sorted_free(by_key);
		} else if (sorted) {
			sort_count = count;
			qsort(order, D, sizeof *order, by_count);
		}
		for (d = 0; d < D && !by_bytes; d++) {
			printf("%llu\t", (unsigned long long)count[order[d]]);
			fwrite(keys + doff[order[d]], 1, (size_t)(doff[order[d] + 1] - doff[order[d]]), stdout);   /* the key and its '\n' */
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_distinct_free(distinct);
	fsm_hip_extracted_free(extracted);
	fsm_hip_matches_free(matches);
	fsm_hip_text_hits_free(hits);
	fsm_hip_text_free(text);
	fsm_hip_rules_free(keep);
	fsm_hip_tok_dfa_free(ends);
	fsm_hip_pos_dfa_free(starts);
	fsm_hip_lines_dfa_free(ld);
	free(file_off);
	free(count);
	free(doff);
	free(order);
	free(rec);
	free(keys);
	free(buf);
	return D != 0 ? 0 : 1;
}
