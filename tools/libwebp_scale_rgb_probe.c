/*
 * libwebp_scale_rgb_probe.c -- drives libwebp's own decoder into RGB with cropping / scaling, for
 * tests/golden/make_scale_rgb_golden.py (the goldens of libwebp's scaled RGB).
 * Links against libwebp only.
 *
 *   probe <in.webp> rgb|rgba left top cw ch sw sh <out.raw>
 *       WebPDecode in MODE_RGB / MODE_RGBA (not premultiplied) with use_cropping (cw > 0) and
 *       use_scaling (sw or sh > 0; a dimension of 0 is derived by libwebp); the loop filter is
 *       libwebp's own choice (bypass_filtering 0).  Prints "w h" of the output.
 *
 * Output: w * h tight pixels of 3 or 4 bytes, no header.  Exit 0 ok, 1 failure.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <webp/decode.h>

static uint8_t* slurp(const char* path, size_t* n) {
	FILE* f = fopen(path, "rb");
	if (!f) return NULL;
	fseek(f, 0, SEEK_END);
	long sz = ftell(f);
	fseek(f, 0, SEEK_SET);
	uint8_t* b = (uint8_t*)malloc(sz > 0 ? (size_t)sz : 1);
	if (b && fread(b, 1, (size_t)sz, f) != (size_t)sz) {
		free(b);
		b = NULL;
	}
	fclose(f);
	*n = (size_t)sz;
	return b;
}

int main(int argc, char** argv) {
	if (argc != 10 || (strcmp(argv[2], "rgb") && strcmp(argv[2], "rgba"))) {
		fputs("usage: probe in.webp rgb|rgba left top cw ch sw sh out.raw\n", stderr);
		return 2;
	}
	size_t n = 0;
	uint8_t* in = slurp(argv[1], &n);
	if (!in) return 1;
	WebPDecoderConfig cfg;
	if (!WebPInitDecoderConfig(&cfg)) return 1;
	const int bpp = argv[2][3] ? 4 : 3;
	const int cw = atoi(argv[5]), ch = atoi(argv[6]), sw = atoi(argv[7]), sh = atoi(argv[8]);
	if (cw > 0) {
		cfg.options.use_cropping = 1;
		cfg.options.crop_left = atoi(argv[3]), cfg.options.crop_top = atoi(argv[4]);
		cfg.options.crop_width = cw, cfg.options.crop_height = ch;
	}
	if (sw > 0 || sh > 0) {
		cfg.options.use_scaling = 1;
		cfg.options.scaled_width = sw, cfg.options.scaled_height = sh;
	}
	cfg.output.colorspace = bpp == 4 ? MODE_RGBA : MODE_RGB;
	const VP8StatusCode st = WebPDecode(in, n, &cfg);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPDecode: status %d\n", (int)st);
		return 1;
	}
	const WebPRGBABuffer* b = &cfg.output.u.RGBA;
	const int w = cfg.output.width, h = cfg.output.height;
	printf("%d %d\n", w, h);
	FILE* f = fopen(argv[9], "wb");
	if (!f) return 1;
	for (int r = 0; r < h; r++) fwrite(b->rgba + (size_t)r * b->stride, 1, (size_t)w * bpp, f);
	const int rc = fclose(f) != 0;
	WebPFreeDecBuffer(&cfg.output);
	free(in);
	return rc;
}
