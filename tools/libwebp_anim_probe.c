/*
 * libwebp_anim_probe.c -- drives libwebp's WebPAnimDecoder and still decoder for tests/golden/make_anim_golden.py
 * (the goldens of the animation path).  Links against libwebpdemux (which brings its libwebp).
 *
 *   probe anim <in.webp> <out.rgba>
 *       WebPAnimDecoderNew (MODE_RGBA, default options) and WebPAnimDecoderGetNext until the last frame.
 *       Prints "w h frames loop_count bgcolor" and then one line per frame with its timestamp (the cumulative
 *       end time in ms).  Output: frames canvases of w*h R,G,B,A byte quadruples each, no header.
 *       Exit 1: WebPAnimDecoderNew refused the file; exit 3: a frame did not decode.
 *   probe rgba <in.webp> <out.rgba>
 *       WebPDecodeRGBA of a still file; prints "w h has_alpha".
 *   probe version
 *       prints the demux and decoder versions as hex.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <webp/decode.h>
#include <webp/demux.h>

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

static int cmd_anim(char** a) {
	WebPData data;
	uint8_t* in = slurp(a[0], &data.size);
	if (!in) return 2;
	data.bytes = in;
	WebPAnimDecoderOptions opt;
	if (!WebPAnimDecoderOptionsInit(&opt)) return 2;
	opt.color_mode = MODE_RGBA;
	WebPAnimDecoder* dec = WebPAnimDecoderNew(&data, &opt);
	if (!dec) {
		fputs("WebPAnimDecoderNew refused the file\n", stderr);
		return 1;
	}
	WebPAnimInfo info;
	if (!WebPAnimDecoderGetInfo(dec, &info)) return 2;
	printf("%u %u %u %u %u\n", info.canvas_width, info.canvas_height, info.frame_count, info.loop_count, info.bgcolor);
	FILE* f = fopen(a[1], "wb");
	if (!f) return 2;
	while (WebPAnimDecoderHasMoreFrames(dec)) {
		uint8_t* canvas;
		int ts;
		if (!WebPAnimDecoderGetNext(dec, &canvas, &ts)) {
			fputs("WebPAnimDecoderGetNext failed\n", stderr);
			return 3;
		}
		printf("%d\n", ts);
		fwrite(canvas, 1, (size_t)info.canvas_width * info.canvas_height * 4, f);
	}
	WebPAnimDecoderDelete(dec);
	free(in);
	return fclose(f) != 0 ? 2 : 0;
}

static int cmd_rgba(char** a) {
	size_t n = 0;
	uint8_t* in = slurp(a[0], &n);
	if (!in) return 2;
	WebPBitstreamFeatures feat;
	if (WebPGetFeatures(in, n, &feat) != VP8_STATUS_OK) return 1;
	int w = 0, h = 0;
	uint8_t* px = WebPDecodeRGBA(in, n, &w, &h);
	if (!px) return 1;
	printf("%d %d %d\n", w, h, feat.has_alpha);
	FILE* f = fopen(a[1], "wb");
	if (!f) return 2;
	fwrite(px, 1, (size_t)w * h * 4, f);
	WebPFree(px);
	free(in);
	return fclose(f) != 0 ? 2 : 0;
}

int main(int argc, char** argv) {
	if (argc == 4 && !strcmp(argv[1], "anim")) return cmd_anim(argv + 2);
	if (argc == 4 && !strcmp(argv[1], "rgba")) return cmd_rgba(argv + 2);
	if (argc == 2 && !strcmp(argv[1], "version")) {
		printf("%x %x\n", (unsigned)WebPGetDemuxVersion(), (unsigned)WebPGetDecoderVersion());
		return 0;
	}
	fputs("usage: probe anim in.webp out.rgba | probe rgba in.webp out.rgba | probe version\n", stderr);
	return 2;
}
