/*
 * libwebp_argb_scale_probe.c -- libwebp's decoder with its crop / scale options into MODE_RGBA, for
 * tests/golden/make_lossless_scale_golden.py (the goldens of the scaled lossless path).
 * Links against libwebp only.
 *
 *   probe <in.webp> <out.rgba> left top crop_w crop_h scaled_w scaled_h
 *       crop_w = crop_h = 0: no cropping (use_cropping off); scaled_w = scaled_h = 0: no scaling
 *       (use_scaling off); one of scaled_w / scaled_h 0: libwebp derives it.
 *       Prints "w h" of the decoded picture.  Output: w*h R,G,B,A byte quadruples, no header.
 *
 * Exit 0 ok, 1 failure (libwebp refused the file or the options; its status goes to stderr).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <webp/decode.h>

int main(int argc, char** argv) {
	if (argc != 9) {
		fputs("usage: probe in.webp out.rgba left top crop_w crop_h scaled_w scaled_h\n", stderr);
		return 2;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 1;
	fseek(f, 0, SEEK_END);
	const long sz = ftell(f);
	fseek(f, 0, SEEK_SET);
	uint8_t* in = (uint8_t*)malloc(sz > 0 ? (size_t)sz : 1);
	if (!in || fread(in, 1, (size_t)sz, f) != (size_t)sz) return 1;
	fclose(f);
	WebPDecoderConfig cfg;
	if (!WebPInitDecoderConfig(&cfg)) return 1;
	const int v[6] = {atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8])};
	if (v[2] | v[3]) {
		cfg.options.use_cropping = 1;
		cfg.options.crop_left = v[0], cfg.options.crop_top = v[1], cfg.options.crop_width = v[2], cfg.options.crop_height = v[3];
	}
	if (v[4] | v[5]) {
		cfg.options.use_scaling = 1;
		cfg.options.scaled_width = v[4], cfg.options.scaled_height = v[5];
	}
	cfg.output.colorspace = MODE_RGBA;
	const VP8StatusCode st = WebPDecode(in, (size_t)sz, &cfg);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPDecode: status %d\n", (int)st);
		return 1;
	}
	const WebPRGBABuffer* o = &cfg.output.u.RGBA;
	const int w = cfg.output.width, h = cfg.output.height;
	printf("%d %d\n", w, h);
	f = fopen(argv[2], "wb");
	if (!f) return 1;
	for (int y = 0; y < h; y++) fwrite(o->rgba + (size_t)y * o->stride, 1, (size_t)w * 4, f);
	WebPFreeDecBuffer(&cfg.output);
	free(in);
	return fclose(f) != 0;
}
