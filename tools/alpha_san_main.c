/*
 * alpha_san_main.c -- robustness driver of the extended container parser and the ALPH decoder, meant
 * to be compiled together with the host sources under -fsanitize=address,undefined and run as a
 * program of its own (tests/test_alpha_host.py does that).
 *
 *   alpha_san <file.webp>...
 *
 * Each file is given to webp_parse_extended whole, truncated at every length, and with 2000 seeded
 * single-byte corruptions; its ALPH payload (if any) goes to vp8f_alpha_decode the same way.  Every
 * buffer handed to the library is an exact-size heap copy, so a read past the end is a report.
 * Prints one summary line per file; exit 0 unless a file cannot be read (the sanitizers end the
 * program themselves on a finding).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../webp-decoder_amd/host/vp8_front.h"

static uint64_t rng_state;
static uint32_t rng(void) { /* splitmix64 */
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int parse(const uint8_t* data, size_t n, WebPContainerX* c) {
	uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
	if (!copy) exit(3);
	memcpy(copy, data, n);
	ByteSpan s = {copy, n};
	const int rc = webp_parse_extended(s, c);
	free(copy);
	return rc;
}

static int decode(const uint8_t* alph, size_t n, uint32_t w, uint32_t h, uint8_t* residual) {
	uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
	if (!copy) exit(3);
	memcpy(copy, alph, n);
	uint32_t filter = 0;
	Vp8fAlphaStats st;
	const int rc = vp8f_alpha_decode(copy, n, w, h, residual, &filter, &st);
	if (rc == 0 && filter > 3) abort();
	free(copy);
	return rc;
}

int main(int argc, char** argv) {
	for (int a = 1; a < argc; a++) {
		FILE* f = fopen(argv[a], "rb");
		if (!f) return 2;
		uint8_t* data = (uint8_t*)malloc(1 << 20);
		const size_t n = fread(data, 1, 1 << 20, f);
		fclose(f);
		rng_state = 0x1234 + (uint64_t)n;
		WebPContainerX c, t;
		unsigned ok_parse = 0, ok_dec = 0, runs = 0;
		const int whole = parse(data, n, &c);
		for (size_t k = 0; k < n; k++) ok_parse += parse(data, k, &t) == 0;
		for (int k = 0; k < 2000 && n; k++) {
			const size_t at = rng() % n;
			const uint8_t old = data[at];
			data[at] ^= (uint8_t)(1u + rng() % 255u);
			ok_parse += parse(data, n, &t) == 0;
			data[at] = old;
		}
		if (whole == 0 && c.alph_chunk_offset) {
			const uint32_t w = c.canvas_width, h = c.canvas_height;
			uint8_t* alph = data + c.alph_chunk_offset;
			const size_t an = c.alph_chunk_size;
			uint8_t* residual = (uint8_t*)malloc((size_t)w * h);
			if (!residual) return 3;
			ok_dec += decode(alph, an, w, h, residual) == 0, runs++;
			for (size_t k = 0; k < an; k++) ok_dec += decode(alph, k, w, h, residual) == 0, runs++;
			for (int k = 0; k < 2000 && an; k++) {
				const size_t at = rng() % an;
				const uint8_t old = alph[at];
				alph[at] ^= (uint8_t)(1u + rng() % 255u);
				ok_dec += decode(alph, an, w, h, residual) == 0, runs++;
				alph[at] = old;
			}
			free(residual);
		}
		printf("%s: container %s, %u variants parsed; ALPH %u of %u variants decoded\n", argv[a], whole == 0 ? "ok" : "refused",
		       ok_parse, ok_dec, runs);
		free(data);
	}
	return 0;
}
