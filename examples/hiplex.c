/*
 * examples/hiplex.c -- a text cut into tokens, every line in one launch: the loop around a DFA in a lexer, with no host loop
 * over bytes:
 *
 *     hiplex [-s] [-b] TABLE.fsmhip FILE
 *
 * TABLE is a lexer's automaton as the library writes it (fsm_hip_desc_write): a union of the token rules with one end-id per
 * rule, determinised, NOT anchored at the end ("a lexer's automaton from libfsm").  fsm_hip_text_open() cuts
 * FILE into lines on the device, fsm_hip_text_tokens() cuts every line into longest-match tokens.  One line of output per token:
 *     LINE:START-END:ID
 * LINE from 1, START and END byte positions in the line, ID the lowest end-id of the state the token was accepted in (a lower id
 * is a higher rule priority), `-` for a byte no token begins at.  By default a line stops at its first such byte.
 *     -s   go on behind such a byte (FSM_HIP_TOKENS_SKIP_BAD): it is printed as a one-byte token with id -
 *     -b   never return to an earlier accept (FSM_HIP_TOKENS_NO_BACKTRACK: what lx's generated lexers do)
 * Exit status: 0, or 2 on error.  Plain C against include/fsm_hip.h only.
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
	struct fsm_hip_dfa *dfa;
	struct fsm_hip_tok_dfa *td;
	struct fsm_hip_text *text;
	struct fsm_hip_tokens *tokens;
	unsigned char *buf = NULL;
	uint64_t *off, *end, p;
	uint32_t *id;
	size_t cap = 0, len = 0, got, m, total, i, k;
	unsigned flags = 0;
	int a;
	FILE *f;

	for (a = 1; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a++) {
		if (strcmp(argv[a], "-s") == 0) {
			flags |= FSM_HIP_TOKENS_SKIP_BAD;
		} else if (strcmp(argv[a], "-b") == 0) {
			flags |= FSM_HIP_TOKENS_NO_BACKTRACK;
		} else {
			a = argc;
		}
	}
	if (a + 2 != argc) {
		fprintf(stderr, "usage: hiplex [-s] [-b] TABLE.fsmhip FILE\n");
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
	dfa = fsm_hip_dfa_create(desc, FSM_HIP_DEFER_UPLOAD);   /* planned only: the image below is all that goes to the device */
	fsm_hip_desc_free(desc);
	if (dfa == NULL) {
		perror("fsm_hip_dfa_create");
		return 2;
	}
	td = fsm_hip_tok_dfa_create(dfa, FSM_HIP_IDS_EARLIEST);
	fsm_hip_dfa_free(dfa);
	if (td == NULL) {
		perror("fsm_hip_tok_dfa_create");
		return 2;
	}

	f = fopen(argv[a + 1], "rb");
	if (f == NULL) {
		perror(argv[a + 1]);
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

	text = fsm_hip_text_open(buf, len, '\n');
	if (text == NULL) {
		perror("fsm_hip_text_open");
		return 2;
	}
	tokens = fsm_hip_text_tokens(td, text, NULL, flags, NULL);
	if (tokens == NULL) {
		perror("fsm_hip_text_tokens");
		return 2;
	}
	m = fsm_hip_tokens_count(tokens);
	total = fsm_hip_tokens_total(tokens);
	off = malloc((m + 1) * sizeof *off);
	end = malloc((total + 1) * sizeof *end);
	id = malloc((total + 1) * sizeof *id);
	if (off == NULL || end == NULL || id == NULL) {
		perror("malloc");
		return 2;
	}
	if (fsm_hip_tokens_copy(tokens, off, end, id, NULL) != 0) {
		perror("fsm_hip_tokens_copy");
		return 2;
	}
	for (i = 0; i < m; i++) {
		p = 0;                                      /* a token starts where the one before it ended */
		for (k = (size_t)off[i]; k < (size_t)off[i + 1]; k++) {
			if (id[k] == FSM_HIP_NO_MATCH) {
				printf("%llu:%llu-%llu:-\n", (unsigned long long)i + 1, (unsigned long long)p, (unsigned long long)end[k]);
			} else {
				printf("%llu:%llu-%llu:%lu\n", (unsigned long long)i + 1, (unsigned long long)p, (unsigned long long)end[k], (unsigned long)id[k]);
			}
			p = end[k];
		}
	}
	if (fflush(stdout) != 0) {
		perror("stdout");
		return 2;
	}
	fsm_hip_tokens_free(tokens);
	fsm_hip_text_free(text);
	fsm_hip_tok_dfa_free(td);
	free(off);
	free(end);
	free(id);
	free(buf);
	return 0;
}
