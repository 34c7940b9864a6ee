/*
 * lossless_san_main.c -- robustness driver of webp_parse_any and the lossless (VP8L) decoder, meant to be
 * compiled together with the host sources under -fsanitize=address,undefined and run as a program of
 * its own (tests/test_lossless_host.py does that).
 *
 *   lossless_san <file.webp>...
 *
 * Each file is given to webp_parse_any, and to webp_locate_still in each of its modes, whole, truncated (every length up to 2048 bytes, then 2048 evenly
 * spaced lengths) and with 500 seeded single-byte corruptions; its VP8L payload (if any) goes to
 * vp8f_lossless_decode the same way (errno cleared before each call: a failure must set EINVAL or ENOMEM itself),
 * and what decodes goes through vp8f_lossless_apply.  Every buffer
 * handed to the library is an exact-size heap copy, so a read past the end is a report.
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

static int parse(const uint8_t* data, size_t n, WebPContainerL* c) {
	uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
	if (!copy) exit(3);
	memcpy(copy, data, n);
	ByteSpan s = {copy, n};
	const int rc = webp_parse_any(s, c);
	if (rc == 0 && c->vp8l_chunk_offset && c->vp8l_chunk_offset + c->vp8l_chunk_size > n) abort();
	/* the walk under the parsers, in each of its modes: what it locates lies inside the file, and with everything
	 * accepted its verdict is webp_parse_any's */
	for (unsigned accept = 0; accept <= (WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS); accept++) {
		WebPStill st;
		const int got = webp_locate_still(s, accept, &st);
		if (accept == (WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS) && got != rc) abort();
		if (got != 0) continue;
		if (st.vp8_offset + st.vp8_size > n || st.alph_offset + st.alph_size > n || st.vp8l_offset + st.vp8l_size > n) abort();
		if (!st.vp8_offset == !st.vp8l_offset) abort(); /* (one image chunk, of one kind) */
	}
	free(copy);
	return rc;
}

static uint64_t sum; /* (keeps the results observable) */

static int decode(const uint8_t* vp8l, size_t n) {
	uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
	if (!copy) exit(3);
	memcpy(copy, vp8l, n);
	Vp8fLosslessImage im;
	Vp8fAlphaStats st;
	errno = 0;
	int rc = vp8f_lossless_decode(copy, n, &im, &st);
	const int e = errno;
	free(copy);
	if (rc != 0) {
		if (e != EINVAL && e != ENOMEM) abort(); /* (every failure sets errno itself) */
		if (im.argb || im.ntransforms) abort(); /* (a failed decode leaves nothing behind) */
		return rc;
	}
	uint32_t* argb = (uint32_t*)malloc((size_t)im.width * im.height * sizeof(uint32_t));
	if (!argb) exit(3);
	rc = vp8f_lossless_apply(&im, argb);
	if (rc == 0) sum += argb[0] + argb[(size_t)im.width * im.height - 1];
	free(argb);
	vp8f_lossless_free(&im);
	return rc;
}

int main(int argc, char** argv) {
	for (int a = 1; a < argc; a++) {
		FILE* f = fopen(argv[a], "rb");
		if (!f) return 2;
		uint8_t* data = (uint8_t*)malloc(1 << 20);
		const size_t n = fread(data, 1, 1 << 20, f);
		fclose(f);
		rng_state = 0x4321 + (uint64_t)n;
		WebPContainerL c, t;
		unsigned ok_parse = 0, ok_dec = 0, runs = 0;
		const int whole = parse(data, n, &c);
		for (size_t k = 0; k < n; k += k < 2048 ? 1 : 1 + n / 2048) ok_parse += parse(data, k, &t) == 0;
		for (int k = 0; k < 500 && n; k++) {
			const size_t at = rng() % n;
			const uint8_t old = data[at];
			data[at] ^= (uint8_t)(1u + rng() % 255u);
			ok_parse += parse(data, n, &t) == 0;
			data[at] = old;
		}
		if (whole == 0 && c.vp8l_chunk_offset) {
			uint8_t* p = data + c.vp8l_chunk_offset;
			const size_t pn = c.vp8l_chunk_size;
			ok_dec += decode(p, pn) == 0, runs++;
			for (size_t k = 0; k < pn; k += k < 2048 ? 1 : 1 + pn / 2048) ok_dec += decode(p, k) == 0, runs++;
			for (int k = 0; k < 500 && pn; k++) {
				const size_t at = rng() % pn;
				const uint8_t old = p[at];
				p[at] ^= (uint8_t)(1u + rng() % 255u);
				ok_dec += decode(p, pn) == 0, runs++;
				p[at] = old;
			}
		}
		printf("%s: container %s, %u variants parsed; VP8L %u of %u variants decoded (%llu)\n", argv[a], whole == 0 ? "ok" : "refused",
		       ok_parse, ok_dec, runs, (unsigned long long)sum);
		free(data);
	}
	return 0;
}
