/*
 * libwebp_lossless_probe.c -- drives libwebp's decoder and lossless encoder for
 * tests/golden/make_lossless_golden.py (the goldens of the lossless path).  Links against
 * libwebp only.
 *
 *   probe rgba <in.webp> <out.rgba>
 *       WebPDecodeRGBA; prints "w h has_alpha" (has_alpha as WebPGetFeatures reports it).
 *       Output: w*h R,G,B,A byte quadruples, no header.
 *   probe lossless W H <in.argb> method quality <out.webp>
 *       WebPEncode, lossless and exact, of W*H pixels stored as little-endian 0xAARRGGBB words
 *
 * Exit 0 ok, 1 failure (rgba: libwebp refused the file; its status goes to stderr).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <webp/decode.h>
#include <webp/encode.h>

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

static int cmd_rgba(char** a) {
	size_t n = 0;
	uint8_t* in = slurp(a[0], &n);
	if (!in) return 1;
	WebPBitstreamFeatures feat;
	VP8StatusCode st = WebPGetFeatures(in, n, &feat);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPGetFeatures: status %d\n", (int)st);
		return 1;
	}
	int w = 0, h = 0;
	uint8_t* px = WebPDecodeRGBA(in, n, &w, &h);
	if (!px) {
		fputs("WebPDecodeRGBA failed\n", stderr);
		return 1;
	}
	printf("%d %d %d\n", w, h, feat.has_alpha);
	FILE* f = fopen(a[1], "wb");
	if (!f) return 1;
	fwrite(px, 1, (size_t)w * h * 4, f);
	WebPFree(px);
	free(in);
	return fclose(f) != 0;
}

static int cmd_lossless(char** a) {
	const int W = atoi(a[0]), H = atoi(a[1]);
	size_t n = 0;
	uint8_t* in = slurp(a[2], &n);
	if (!in || n != (size_t)W * H * 4) return 1;
	WebPConfig cfg;
	WebPPicture pic;
	if (!WebPConfigInit(&cfg) || !WebPPictureInit(&pic)) return 1;
	cfg.lossless = 1, cfg.exact = 1;
	cfg.method = atoi(a[3]), cfg.quality = (float)atoi(a[4]);
	pic.use_argb = 1, pic.width = W, pic.height = H;
	if (!WebPPictureAlloc(&pic)) return 1;
	for (int y = 0; y < H; y++) memcpy(pic.argb + (size_t)y * pic.argb_stride, in + (size_t)y * W * 4, (size_t)W * 4);
	free(in);
	WebPMemoryWriter wr;
	WebPMemoryWriterInit(&wr);
	pic.writer = WebPMemoryWrite;
	pic.custom_ptr = &wr;
	if (!WebPValidateConfig(&cfg) || !WebPEncode(&cfg, &pic)) {
		fprintf(stderr, "WebPEncode: error %d\n", (int)pic.error_code);
		return 1;
	}
	FILE* f = fopen(a[5], "wb");
	if (!f) return 1;
	fwrite(wr.mem, 1, wr.size, f);
	WebPMemoryWriterClear(&wr);
	WebPPictureFree(&pic);
	return fclose(f) != 0;
}

int main(int argc, char** argv) {
	if (argc == 4 && !strcmp(argv[1], "rgba")) return cmd_rgba(argv + 2);
	if (argc == 8 && !strcmp(argv[1], "lossless")) return cmd_lossless(argv + 2);
	fputs("usage: probe rgba in.webp out.rgba | probe lossless W H in.argb method quality out.webp\n", stderr);
	return 2;
}
