/*
 * libwebp_alpha_probe.c -- drives libwebp's decoder and encoders for tests/golden/make_alpha_golden.py
 * (the goldens of the extended-container / alpha path).  Links against libwebp only.
 *
 *   probe decode <in.webp> left top cw ch sw sh <out.yuva>
 *       WebPDecode with use_cropping (cw > 0) / use_scaling (sw or sh > 0), in MODE_YUVA for the A plane
 *       and in MODE_YUV for Y, U, V; prints "w h has_alpha" (has_alpha as WebPGetFeatures reports it).
 *       Output: Y (w*h), U, V (each ceil(w/2)*ceil(h/2)), A (w*h), no header.
 *   probe lossless W H <in.argb> method quality <out.webp>
 *       WebPEncode, lossless and exact, of W*H pixels stored as little-endian 0xAARRGGBB words
 *   probe lossy W H <in.rgba> quality alpha_quality alpha_filtering alpha_compression <out.webp>
 *       WebPEncode, lossy, of W*H R,G,B,A byte quadruples
 *
 * Exit 0 ok, 1 failure (decode: libwebp refused the file; its status goes to stderr).
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

static void rows(FILE* f, const uint8_t* p, int stride, int w, int h) {
	for (int r = 0; r < h; r++) fwrite(p + (size_t)r * stride, 1, (size_t)w, f);
}

static int cmd_decode(char** a) {
	size_t n = 0;
	uint8_t* in = slurp(a[0], &n);
	if (!in) return 1;
	WebPDecoderConfig cfg;
	if (!WebPInitDecoderConfig(&cfg)) return 1;
	VP8StatusCode st = WebPGetFeatures(in, n, &cfg.input);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPGetFeatures: status %d\n", (int)st);
		return 1;
	}
	const int cw = atoi(a[3]), ch = atoi(a[4]), sw = atoi(a[5]), sh = atoi(a[6]);
	if (cw > 0) {
		cfg.options.use_cropping = 1;
		cfg.options.crop_left = atoi(a[1]), cfg.options.crop_top = atoi(a[2]);
		cfg.options.crop_width = cw, cfg.options.crop_height = ch;
	}
	if (sw > 0 || sh > 0) {
		cfg.options.use_scaling = 1;
		cfg.options.scaled_width = sw, cfg.options.scaled_height = sh;
	}
	cfg.output.colorspace = MODE_YUVA;
	st = WebPDecode(in, n, &cfg);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPDecode: status %d\n", (int)st);
		return 1;
	}
	/* Y, U, V come from a second decode in MODE_YUV (what `dwebp -yuv` writes): when it rescales a picture
	 * with alpha in MODE_YUVA, libwebp multiplies the luma by alpha before the rescaler and divides after */
	WebPDecoderConfig yuv = cfg;
	memset(&yuv.output, 0, sizeof(yuv.output));
	WebPInitDecBuffer(&yuv.output);
	yuv.output.colorspace = MODE_YUV;
	st = WebPDecode(in, n, &yuv);
	if (st != VP8_STATUS_OK) {
		fprintf(stderr, "WebPDecode (MODE_YUV): status %d\n", (int)st);
		return 1;
	}
	const WebPYUVABuffer* b = &cfg.output.u.YUVA;
	const WebPYUVABuffer* c = &yuv.output.u.YUVA;
	const int w = cfg.output.width, h = cfg.output.height;
	if (yuv.output.width != w || yuv.output.height != h) return 1;
	printf("%d %d %d\n", w, h, cfg.input.has_alpha);
	FILE* f = fopen(a[7], "wb");
	if (!f || !b->a) return 1;
	rows(f, c->y, c->y_stride, w, h);
	rows(f, c->u, c->u_stride, (w + 1) / 2, (h + 1) / 2);
	rows(f, c->v, c->v_stride, (w + 1) / 2, (h + 1) / 2);
	rows(f, b->a, b->a_stride, w, h);
	const int rc = fclose(f) != 0;
	WebPFreeDecBuffer(&cfg.output);
	WebPFreeDecBuffer(&yuv.output);
	free(in);
	return rc;
}

static int encode(WebPConfig* cfg, WebPPicture* pic, const char* out) {
	WebPMemoryWriter wr;
	WebPMemoryWriterInit(&wr);
	pic->writer = WebPMemoryWrite;
	pic->custom_ptr = &wr;
	if (!WebPValidateConfig(cfg) || !WebPEncode(cfg, pic)) {
		fprintf(stderr, "WebPEncode: error %d\n", (int)pic->error_code);
		return 1;
	}
	FILE* f = fopen(out, "wb");
	if (!f) return 1;
	fwrite(wr.mem, 1, wr.size, f);
	WebPMemoryWriterClear(&wr);
	WebPPictureFree(pic);
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
	return encode(&cfg, &pic, a[5]);
}

static int cmd_lossy(char** a) {
	const int W = atoi(a[0]), H = atoi(a[1]);
	size_t n = 0;
	uint8_t* in = slurp(a[2], &n);
	if (!in || n != (size_t)W * H * 4) return 1;
	WebPConfig cfg;
	WebPPicture pic;
	if (!WebPConfigInit(&cfg) || !WebPPictureInit(&pic)) return 1;
	cfg.quality = (float)atoi(a[3]);
	cfg.alpha_quality = atoi(a[4]), cfg.alpha_filtering = atoi(a[5]), cfg.alpha_compression = atoi(a[6]);
	pic.width = W, pic.height = H;
	if (!WebPPictureImportRGBA(&pic, in, W * 4)) return 1;
	free(in);
	return encode(&cfg, &pic, a[7]);
}

int main(int argc, char** argv) {
	if (argc == 10 && !strcmp(argv[1], "decode")) return cmd_decode(argv + 2);
	if (argc == 8 && !strcmp(argv[1], "lossless")) return cmd_lossless(argv + 2);
	if (argc == 10 && !strcmp(argv[1], "lossy")) return cmd_lossy(argv + 2);
	fputs("usage: probe decode in.webp left top cw ch sw sh out | probe lossless W H in.argb method quality out.webp |\n"
	      "       probe lossy W H in.rgba quality alpha_quality alpha_filtering alpha_compression out.webp\n", stderr);
	return 2;
}
