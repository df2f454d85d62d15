/*
 * examples/hipgrep_text.c -- hipgrep.c without its host loop over the bytes:
 *
 *     hipgrep_text TABLE.fsmhip < lines.txt
 *
 * Same command line and output as hipgrep.c ("<line-number>:<end-id>[,<end-id>...]" per accepted record).  The file is
 * slurped and handed over as it is: fsm_hip_text_open() finds the lines on the device, fsm_hip_lines_dfa_create() builds
 * the automaton in which '\n' is a self-loop of every state, and fsm_hip_text_exec() walks the untouched text -- nothing is
 * squeezed, no offsets are built on the host.  Plain C against include/fsm_hip.h only.
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
	const struct fsm_hip_dfa *dfa;
	struct fsm_hip_text *text;
	unsigned char *buf = NULL;
	uint32_t *end = NULL;
	size_t cap = 0, len = 0, n, i, got;
	FILE *tf;

	if (argc != 2) {
		fprintf(stderr, "usage: hipgrep_text TABLE.fsmhip < records\n");
		return 2;
	}
	tf = fopen(argv[1], "rb");
	if (tf == NULL) {
		perror(argv[1]);
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
	dfa = fsm_hip_lines_dfa_inner(ld);

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
	n = fsm_hip_text_lines(text);
	if (n == 0) {
		fsm_hip_text_free(text);
		fsm_hip_lines_dfa_free(ld);
		free(buf);
		return 1;
	}
	end = malloc(n * sizeof *end);
	if (end == NULL || fsm_hip_text_exec(ld, text, end, NULL, 0, NULL, NULL) != 0) {
		perror("fsm_hip_text_exec");
		return 2;
	}
	got = 0;
	for (i = 0; i < n; i++) {
		uint32_t ids[64];
		size_t c, k;
		if (end[i] == FSM_HIP_NO_MATCH) {
			continue;
		}
		got++;
		c = fsm_hip_endid_count(dfa, end[i]);
		printf("%zu:", i + 1);
		if (c <= 64 && fsm_hip_endid_get(dfa, end[i], c, ids)) {
			for (k = 0; k < c; k++) {
				printf(k ? ",%u" : "%u", ids[k]);
			}
		}
		putchar('\n');
	}
	fsm_hip_text_free(text);
	fsm_hip_lines_dfa_free(ld);
	free(end);
	free(buf);
	return got ? 0 : 1;
}
