/*
 * examples/hipfgrep.c -- the lines that equal a line of a list: grep -F -x -f LIST FILE... without an automaton.  The list's lines
 * become the keys of a distinct object, the files' lines are looked up among them on the device, and the bitmap of the lookup
 * selects the hits:
 *
 *     hipfgrep -f LIST [-v] [-c] [-n] FILE...
 *
 * fsm_hip_distinct() makes the dictionary of LIST's lines (trimmed by '\n'; only the table is kept: FSM_HIP_DISTINCT_NO_TEXT),
 * fsm_hip_text_open_files() cuts the files into lines, fsm_hip_keys_find_text() looks every line up -- no pick is needed:
 * FSM_HIP_FIND_NO_PICK -- and its bitmap goes, as it lies on the device, into fsm_hip_text_hits_device(); the hits' copy is what is
 * printed.  However long the list is, a line costs one hash and one walk of a chain.
 *     -v         the lines that equal NO line of LIST (FSM_HIP_HITS_INVERT)
 *     -c         the number of such lines per file instead of the lines
 *     -n         each line behind its number in its file, from 1
 * With more than one FILE every line is printed behind its file's name, as grep prints it.
 * Exit status: 0 if a line was selected, 1 if not, 2 on error.  Plain C against include/fsm_hip.h only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsm_hip.h"

/* the file's bytes behind buf[*len], which grows */
static unsigned char *
read_file(const char *path, unsigned char *buf, size_t *cap, size_t *len)
{
	size_t got;
	FILE *f;

	f = fopen(path, "rb");
	if (f == NULL) {
		perror(path);
		exit(2);
	}
	for (;;) {
		if (*cap - *len < 65536) {
			*cap = *cap ? *cap * 2 : 1 << 20;
			buf = realloc(buf, *cap);
			if (buf == NULL) {
				perror("realloc");
				exit(2);
			}
		}
		got = fread(buf + *len, 1, *cap - *len, f);
		if (got == 0) {
			break;
		}
		*len += got;
	}
	fclose(f);
	return buf;
}

int
main(int argc, char **argv)
{
	struct fsm_hip_distinct *keys;
	struct fsm_hip_text *text;
	struct fsm_hip_found *found;
	struct fsm_hip_text_hits *hits;
	unsigned char *list = NULL, *buf = NULL, *out = NULL;
	uint64_t *list_off, *file_off, *file_lines, *file_first, *lines = NULL, *out_off = NULL;
	size_t list_cap = 0, list_len = 0, cap = 0, len = 0, nkeys, nfiles, m, i, j, k;
	int invert = 0, count = 0, number = 0, a;
	const char *list_path = NULL;
	char **names;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-v") == 0) {
			invert = 1;
		} else if (strcmp(argv[a], "-c") == 0) {
			count = 1;
		} else if (strcmp(argv[a], "-n") == 0) {
			number = 1;
		} else if (strcmp(argv[a], "-f") == 0 && a + 1 < argc) {
			list_path = argv[++a];
		} else {
			a = argc;
		}
	}
	if (list_path == NULL || a >= argc) {
		fprintf(stderr, "usage: hipfgrep -f LIST [-v] [-c] [-n] FILE...\n");
		return 2;
	}

	/* the list as a packed text: a record is a line with its '\n', which the trim byte takes off again */
	list = read_file(list_path, list, &list_cap, &list_len);
	nkeys = 0;
	for (i = 0; i < list_len; i++) {
		nkeys += list[i] == '\n';
	}
	nkeys += list_len != 0 && list[list_len - 1] != '\n';
	list_off = malloc((nkeys + 1) * sizeof *list_off);
	if (list_off == NULL) {
		perror("malloc");
		return 2;
	}
	list_off[0] = 0;
	for (i = 0, k = 0; i < list_len; i++) {
		if (list[i] == '\n') {
			list_off[++k] = i + 1;
		}
	}
	list_off[nkeys] = list_len;
	keys = fsm_hip_distinct(list_off, list, nkeys, '\n', NULL, -1, FSM_HIP_DISTINCT_NO_TEXT);
	if (keys == NULL) {
		perror("fsm_hip_distinct");
		return 2;
	}

	/* the files back to back: file j is buf[file_off[j], file_off[j + 1]); a line ends where its file ends */
	names = argv + a;
	nfiles = (size_t)(argc - a);
	file_off = malloc((nfiles + 1) * sizeof *file_off);
	file_lines = malloc((nfiles + 1) * sizeof *file_lines);
	file_first = malloc((nfiles + 1) * sizeof *file_first);
	if (file_off == NULL || file_lines == NULL || file_first == NULL) {
		perror("malloc");
		return 2;
	}
	for (j = 0; j < nfiles; j++) {
		file_off[j] = len;
		buf = read_file(names[j], buf, &cap, &len);
	}
	file_off[nfiles] = len;
	text = fsm_hip_text_open_files(buf, len, '\n', file_off, nfiles);
	if (text == NULL) {
		perror("fsm_hip_text_open_files");
		return 2;
	}

	/* the lookup and the selection, one behind the other on the NULL stream; nothing comes to the host in between */
	found = fsm_hip_keys_find_text(keys, text, FSM_HIP_FIND_NO_PICK, NULL);
	if (found == NULL) {
		perror("fsm_hip_keys_find_text");
		return 2;
	}
	hits = fsm_hip_text_hits_device(text, fsm_hip_found_bitmap_device(found), (invert ? FSM_HIP_HITS_INVERT : 0) | (count ? FSM_HIP_HITS_NO_BYTES : 0), NULL);
	if (hits == NULL) {
		perror("fsm_hip_text_hits_device");
		return 2;
	}
	m = fsm_hip_text_hits_count(hits);
	if (fsm_hip_text_hits_file_first(hits, file_first) != 0 || fsm_hip_text_file_lines(text, file_lines) != 0) {
		perror("fsm_hip_text_hits_file_first");
		return 2;
	}
	if (count) {
		for (j = 0; j < nfiles; j++) {
			if (nfiles > 1) {
				printf("%s:", names[j]);
			}
			printf("%llu\n", (unsigned long long)(file_first[j + 1] - file_first[j]));
		}
	} else if (m != 0) {
		lines = malloc(m * sizeof *lines);
		out_off = malloc((m + 1) * sizeof *out_off);
		out = malloc(fsm_hip_text_hits_nbytes(hits) + 1);
		if (lines == NULL || out_off == NULL || out == NULL) {
			perror("malloc");
			return 2;
		}
		if (fsm_hip_text_hits_copy(hits, lines, out_off, out) != 0) {
			perror("fsm_hip_text_hits_copy");
			return 2;
		}
		for (j = 0; j < nfiles; j++) {
			for (k = (size_t)file_first[j]; k < (size_t)file_first[j + 1]; k++) {
				if (nfiles > 1) {
					printf("%s:", names[j]);
				}
				if (number) {
					printf("%llu:", (unsigned long long)(lines[k] - file_lines[j] + 1));
				}
				fwrite(out + out_off[k], 1, (size_t)(out_off[k + 1] - out_off[k]), stdout);
				if (out_off[k + 1] == out_off[k] || out[out_off[k + 1] - 1] != '\n') {
					putchar('\n');                                      /* a file's last line without its delimiter */
				}
			}
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_text_hits_free(hits);
	fsm_hip_found_free(found);                                          /* before the dictionary and the text it probed */
	fsm_hip_text_free(text);
	fsm_hip_distinct_free(keys);
	free(list_off);
	free(file_off);
	free(file_lines);
	free(file_first);
	free(lines);
	free(out_off);
	free(out);
	free(list);
	free(buf);
	return m != 0 ? 0 : 1;
}
