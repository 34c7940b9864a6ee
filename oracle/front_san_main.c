/*
 * front_san_main.c -- TEST INFRASTRUCTURE: the host front end under AddressSanitizer + UBSan, in a
 * program of its own (`make -C oracle san` builds oracle/front_san from this file and the host sources; not
 * part of `all`, CPU only, never loaded into Python).
 *
 *   front_san <dir>      every *.webp of <dir> (tests/test_streams.py writes the directed streams there)
 *
 * Per file, vp8f_decode_memory, vp8f_decode_packed_memory (without and with VP8F_MULTI_PARTITION) and
 * vp8f_token_header_memory (likewise) run on
 *   - the intact stream;
 *   - every prefix of its first 64 payload bytes;
 *   - prefixes ending at and around (-2 .. +2 bytes) each partition boundary;
 *   - 300 seeded single-bit flips confined to the frame tag, the size fields, partition 0's first
 *     64 bytes and the partition-size table
 * (a prefix is the payload cut short with the container sizes rewritten, so that it reaches the VP8
 * parser; a mutation whose size fields give more than 1024 macroblocks is skipped to bound the run).
 * Checks: the entry points agree on success or failure (dense = packed = token header without the
 * flag; packed = token header with it; whatever parses without the flag parses with it), nothing is
 * left allocated on failure (every pointer of the outputs is NULL; LeakSanitizer at exit), and the
 * sanitizers stay silent (-fno-sanitize-recover: any report aborts).
 * Prints "front_san: OK ..." and exits 0, or the first disagreement and exits 1.
 */
#include <dirent.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../webp-decoder_amd/host/vp8_front.h"

static unsigned long g_runs, g_ok;

static int frame_clean(const Vp8DecodedFrame* f) {
	return !f->segment_id && !f->skip_coeff && !f->has_coeff && !f->ymode && !f->uv_mode && !f->bmode && !f->coeff_y2 &&
	       !f->coeff_y && !f->coeff_u && !f->coeff_v;
}

/* 0 ok, 1 a check failed (reported) */
static int run_one(const char* name, const char* what, long arg, const uint8_t* data, size_t size) {
	/* an exact-size heap copy: one byte past the end is an ASan report */
	uint8_t* d = (uint8_t*)malloc(size ? size : 1);
	if (!d) return 1;
	memcpy(d, data, size);
	int rc[5], bad = 0;
	Vp8KeyFrameHeader kf;
	Vp8DecodedFrame f;
	int stage;
	memset(&f, 0, sizeof(f));
	rc[0] = vp8f_decode_memory(d, size, &kf, &f, &stage);
	if (rc[0] != 0 && !frame_clean(&f)) bad = 1;
	if (rc[0] == 0) vp8_decoded_frame_free(&f);
	for (int multi = 0; multi < 2; multi++) {
		Vp8gPackedFrame p;
		memset(&p, 0, sizeof(p));
		rc[1 + multi] = vp8f_decode_packed_memory(d, size, &p, &stage, VP8F_PACK_HASH | (multi ? VP8F_MULTI_PARTITION : 0u));
		if (rc[1 + multi] != 0 && (!frame_clean(&p.f) || p.masks || p.mb_off || p.values)) bad = 1;
		if (rc[1 + multi] == 0) vp8f_packed_free(&p);
		Vp8DecodedFrame hdr;
		Vp8gTokFrame tf;
		uint64_t off = 0;
		uint32_t psize = 0;
		rc[3 + multi] = vp8f_token_header_memory(d, size, &kf, &hdr, &tf, &off, &psize, &stage, multi ? VP8F_MULTI_PARTITION : 0u);
		if (rc[3 + multi] == 0 && (off + psize > size || tf.p0_end > psize || tf.b_next > tf.p0_end || tf.nparts < 1 ||
		                           tf.nparts > 8 || tf.part_end[tf.nparts - 1] > psize))
			bad = 1;
	}
	free(d);
	g_runs++;
	g_ok += rc[2] == 0;
	const int agree = (rc[0] == 0) == (rc[1] == 0) && (rc[1] == 0) == (rc[3] == 0) && (rc[2] == 0) == (rc[4] == 0) &&
	                  (rc[1] != 0 || rc[2] == 0);
	if (bad || !agree) {
		printf("front_san: FAIL %s %s %ld: dense %d packed %d/%d header %d/%d%s\n", name, what, arg, rc[0], rc[1], rc[2], rc[3],
		       rc[4], bad ? " (output not clean)" : "");
		return 1;
	}
	return 0;
}

static void put_le32(uint8_t* p, uint32_t v) {
	for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

/* the stream with its payload cut to n bytes, container sizes rewritten */
static size_t make_prefix(const uint8_t* data, size_t n, uint8_t* out) {
	memcpy(out, data, 20 + n);
	out[20 + n] = 0;
	put_le32(out + 4, (uint32_t)(12 + n + (n & 1)));
	put_le32(out + 16, (uint32_t)n);
	return 20 + n + (n & 1);
}

static uint64_t xorshift(uint64_t* s) {
	uint64_t x = *s;
	x ^= x << 13, x ^= x >> 7, x ^= x << 17;
	return *s = x;
}

static int run_file(const char* name, const uint8_t* data, size_t size, uint64_t seed) {
	if (run_one(name, "intact", 0, data, size)) return 1;
	if (size < 30 || memcmp(data, "RIFF", 4) != 0) return 0;
	const size_t payload = (size_t)data[16] | (size_t)data[17] << 8 | (size_t)data[18] << 16 | (size_t)data[19] << 24;
	if (20 + payload > size) return 0;
	uint8_t* tmp = (uint8_t*)malloc(size + 2);
	if (!tmp) return 1;
	int fail = 0;
	for (size_t n = 0; n <= 64 && n <= payload && !fail; n++) fail = run_one(name, "prefix", (long)n, tmp, make_prefix(data, n, tmp));
	/* partition boundaries, found with the front end's own header parser on the intact stream */
	Vp8KeyFrameHeader kf;
	Vp8DecodedFrame hdr;
	Vp8gTokFrame tf;
	uint64_t off;
	uint32_t psize;
	int stage;
	uint32_t table = 0, nparts = 1;
	if (vp8f_token_header_memory(data, size, &kf, &hdr, &tf, &off, &psize, &stage, VP8F_MULTI_PARTITION) == 0) {
		nparts = tf.nparts;
		table = tf.p0_end;
		for (uint32_t p = 0; p <= nparts && !fail; p++) {
			const long edge = p == 0 ? (long)tf.p0_end : (long)tf.part_end[p - 1];
			for (long dlt = -2; dlt <= 2 && !fail; dlt++) {
				const long n = edge + dlt;
				if (n < 0 || (size_t)n > payload) continue;
				fail = run_one(name, "boundary", n, tmp, make_prefix(data, (size_t)n, tmp));
			}
		}
		if (!fail) fail = run_one(name, "boundary", (long)tf.part_off[0], tmp, make_prefix(data, tf.part_off[0], tmp));
	}
	/* bit flips: bytes 0..9 (frame tag, start code, size fields), partition 0's first 64 bytes, the size table */
	uint64_t rng = seed ? seed : 0x5EED;
	const size_t head = payload < 74 ? payload : 74, tab = table ? 3u * (nparts - 1u) : 0;
	for (int i = 0; i < 300 && !fail && head + tab > 0; i++) {
		size_t k = (size_t)(xorshift(&rng) % (head + tab));
		k = k < head ? k : table + (k - head);
		if (k >= payload) continue;
		memcpy(tmp, data, size);
		tmp[20 + k] ^= (uint8_t)(1u << (xorshift(&rng) & 7u));
		const uint32_t w = (uint32_t)(tmp[26] | tmp[27] << 8) & 0x3FFFu, h = (uint32_t)(tmp[28] | tmp[29] << 8) & 0x3FFFu;
		if ((uint64_t)((w + 15u) >> 4) * ((h + 15u) >> 4) > 1024u) continue;
		fail = run_one(name, "flip", (long)(k * 8), tmp, size);
	}
	free(tmp);
	return fail;
}

static int by_name(const void* a, const void* b) { return strcmp(*(char* const*)a, *(char* const*)b); }

int main(int argc, char** argv) {
	if (argc != 2) {
		fputs("usage: front_san <dir of .webp files>\n", stderr);
		return 2;
	}
	DIR* dir = opendir(argv[1]);
	if (!dir) {
		perror(argv[1]);
		return 2;
	}
	char* names[4096];
	size_t n = 0;
	for (struct dirent* e; (e = readdir(dir)) != NULL && n < 4096;) {
		const size_t l = strlen(e->d_name);
		if (l > 5 && !strcmp(e->d_name + l - 5, ".webp")) names[n++] = strdup(e->d_name);
	}
	closedir(dir);
	qsort(names, n, sizeof(names[0]), by_name);
	int fail = 0;
	for (size_t i = 0; i < n; i++) {
		char path[4096];
		snprintf(path, sizeof(path), "%s/%s", argv[1], names[i]);
		FILE* fp = fopen(path, "rb");
		if (!fp) {
			perror(path);
			fail = 1;
		} else {
			fseek(fp, 0, SEEK_END);
			const long sz = ftell(fp);
			fseek(fp, 0, SEEK_SET);
			uint8_t* buf = (uint8_t*)malloc(sz > 0 ? (size_t)sz : 1);
			if (!buf || fread(buf, 1, (size_t)sz, fp) != (size_t)sz) fail = 1;
			else if (!fail) fail = run_file(names[i], buf, (size_t)sz, 0x9E3779B97F4A7C15ull * (i + 1));
			free(buf);
			fclose(fp);
		}
		free(names[i]);
	}
	if (fail || n == 0) {
		printf("front_san: FAILED (%zu files)\n", n);
		return 1;
	}
	printf("front_san: OK %zu files, %lu inputs, %lu of them decodable\n", n, g_runs, g_ok);
	return 0;
}
