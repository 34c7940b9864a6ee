/*
 * libwebp_scale_probe.c -- drives libwebp's own rescaler, for tests/golden/make_scale_golden.py
 * (the goldens of the crop + downscale path).  Links against libwebp only.
 *
 *   probe rescale W H w h <in.i420> <out.i420>
 *       WebPPictureRescale of a W x H 4:2:0 picture (Y, U, V tight in the file) to w x h
 *   probe decode <in.webp> bypass left top cw ch sw sh <out.i420>
 *       WebPDecode in MODE_YUV with use_cropping (cw > 0) / use_scaling (sw or sh > 0) and
 *       bypass_filtering; prints "w h" of the output
 *
 * Output: Y (w*h) then U then V (each ceil(w/2)*ceil(h/2)), no header.  Exit 0 ok, 1 failure.
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

static int dump(const char* path, const uint8_t* y, int ys, const uint8_t* u, const uint8_t* v, int uvs, int w, int h) {
	FILE* f = fopen(path, "wb");
	if (!f) return 1;
	const int cw = (w + 1) / 2, ch = (h + 1) / 2;
	for (int r = 0; r < h; r++) fwrite(y + (size_t)r * ys, 1, (size_t)w, f);
	for (int r = 0; r < ch; r++) fwrite(u + (size_t)r * uvs, 1, (size_t)cw, f);
	for (int r = 0; r < ch; r++) fwrite(v + (size_t)r * uvs, 1, (size_t)cw, f);
	return fclose(f) != 0;
}

static int cmd_rescale(char** a) {
	const int W = atoi(a[0]), H = atoi(a[1]), w = atoi(a[2]), h = atoi(a[3]);
	size_t n = 0;
	uint8_t* in = slurp(a[4], &n);
	const int CW = (W + 1) / 2, CH = (H + 1) / 2;
	if (!in || n != (size_t)W * H + 2 * (size_t)CW * CH) return 1;
	WebPPicture pic;
	if (!WebPPictureInit(&pic)) return 1;
	pic.use_argb = 0;
	pic.colorspace = WEBP_YUV420;
	pic.width = W, pic.height = H;
	if (!WebPPictureAlloc(&pic)) return 1;
	for (int r = 0; r < H; r++) memcpy(pic.y + (size_t)r * pic.y_stride, in + (size_t)r * W, (size_t)W);
	for (int r = 0; r < CH; r++) {
		memcpy(pic.u + (size_t)r * pic.uv_stride, in + (size_t)W * H + (size_t)r * CW, (size_t)CW);
		memcpy(pic.v + (size_t)r * pic.uv_stride, in + (size_t)W * H + (size_t)CW * CH + (size_t)r * CW, (size_t)CW);
	}
	if (!WebPPictureRescale(&pic, w, h) || pic.width != w || pic.height != h) return 1;
	const int rc = dump(a[5], pic.y, pic.y_stride, pic.u, pic.v, pic.uv_stride, w, h);
	WebPPictureFree(&pic);
	free(in);
	return rc;
}

static int cmd_decode(char** a) {
	size_t n = 0;
	uint8_t* in = slurp(a[0], &n);
	if (!in) return 1;
	WebPDecoderConfig cfg;
	if (!WebPInitDecoderConfig(&cfg)) return 1;
	cfg.options.bypass_filtering = atoi(a[1]);
	const int cw = atoi(a[4]), ch = atoi(a[5]), sw = atoi(a[6]), sh = atoi(a[7]);
	if (cw > 0) {
		cfg.options.use_cropping = 1;
		cfg.options.crop_left = atoi(a[2]), cfg.options.crop_top = atoi(a[3]);
		cfg.options.crop_width = cw, cfg.options.crop_height = ch;
	}
	if (sw > 0 || sh > 0) {
		cfg.options.use_scaling = 1;
		cfg.options.scaled_width = sw, cfg.options.scaled_height = sh;
	}
	cfg.output.colorspace = MODE_YUV;
	const VP8StatusCode st = WebPDecode(in, n, &cfg);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPDecode: status %d\n", (int)st);
		return 1;
	}
	const WebPYUVABuffer* b = &cfg.output.u.YUVA;
	printf("%d %d\n", cfg.output.width, cfg.output.height);
	const int rc = dump(a[8], b->y, b->y_stride, b->u, b->v, b->u_stride, cfg.output.width, cfg.output.height);
	WebPFreeDecBuffer(&cfg.output);
	free(in);
	return rc;
}

int main(int argc, char** argv) {
	if (argc == 8 && !strcmp(argv[1], "rescale")) return cmd_rescale(argv + 2);
	if (argc == 11 && !strcmp(argv[1], "decode")) return cmd_decode(argv + 2);
	fputs("usage: probe rescale W H w h in out | probe decode in.webp bypass left top cw ch sw sh out\n", stderr);
	return 2;
}
