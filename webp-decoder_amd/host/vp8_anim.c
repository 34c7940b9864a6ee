/*
 * vp8_anim.c -- the compositor of an animated .webp, sequentially: libwebp's WebPAnimDecoder (MODE_RGBA, default
 * options) restated on 0xAARRGGBB dwords.  The authority the device kernel (csrc/vp8g_anim.hip) is
 * tested against, itself checked against libwebp's canvases for tests/golden/anim/ (tests/golden/anim.json).
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "vp8_front.h"

static int full(const Vp8fAnimFrame* f, uint32_t cw, uint32_t ch) { return f->width == cw && f->height == ch; }

int vp8f_anim_keyframes(uint32_t cw, uint32_t ch, Vp8fAnimFrame* frames, uint32_t n) {
	if (!frames || n == 0 || cw == 0 || ch == 0 || cw > 16383u || ch > 16383u) {
		errno = EINVAL;
		return -1;
	}
	for (uint32_t k = 0; k < n; k++) {
		Vp8fAnimFrame* f = &frames[k];
		if (f->width == 0 || f->height == 0 || f->x > cw || f->y > ch || f->width > cw - f->x || f->height > ch - f->y) {
			errno = EINVAL;
			return -1;
		}
		if (k == 0) {
			f->key = 1;
			continue;
		}
		const Vp8fAnimFrame* p = f - 1;
		f->key = ((!f->has_alpha || !f->blend) && full(f, cw, ch)) || (p->dispose && (full(p, cw, ch) || p->key));
	}
	return 0;
}

/* libwebp's non-premultiplied blend of one pixel over another (anim_decode.c: BlendPixelNonPremult, and the
 * shortcut of its row function for an opaque source) */
static uint32_t blend_pixel(uint32_t s, uint32_t d) {
	const uint32_t sa = s >> 24;
	if (sa == 255u) return s;
	if (sa == 0u) return d;
	const uint32_t dfa = ((d >> 24) * (256u - sa)) >> 8;
	const uint32_t ba = sa + dfa;
	const uint32_t scale = (1u << 24) / ba;
	uint32_t out = ba << 24;
	for (int sh = 0; sh < 24; sh += 8) out |= (((((s >> sh) & 255u) * sa + ((d >> sh) & 255u) * dfa) * scale) >> 24) << sh;
	return out;
}

int vp8f_anim_compose(uint32_t cw, uint32_t ch, const Vp8fAnimFrame* frames, uint32_t n, uint32_t* canvases) {
	if (!frames || !canvases || n == 0) {
		errno = EINVAL;
		return -1;
	}
	Vp8fAnimFrame* fr = (Vp8fAnimFrame*)malloc((size_t)n * sizeof(*fr));
	if (!fr) {
		errno = ENOMEM;
		return -1;
	}
	memcpy(fr, frames, (size_t)n * sizeof(*fr));
	int rc = vp8f_anim_keyframes(cw, ch, fr, n);
	for (uint32_t k = 0; rc == 0 && k < n; k++)
		if (!fr[k].argb) errno = EINVAL, rc = -1;
	const size_t px = (size_t)cw * ch;
	uint32_t* disposed = rc == 0 ? (uint32_t*)calloc(px, sizeof(uint32_t)) : NULL; /* the previous canvas after its disposal */
	if (rc == 0 && !disposed) errno = ENOMEM, rc = -1;
	for (uint32_t k = 0; rc == 0 && k < n; k++) {
		const Vp8fAnimFrame* f = &fr[k];
		const Vp8fAnimFrame* p = k ? f - 1 : f;
		uint32_t* cur = canvases + (size_t)k * px;
		if (f->key) memset(cur, 0, px * sizeof(uint32_t));
		else memcpy(cur, disposed, px * sizeof(uint32_t));
		const int blends = f->blend && !f->key;
		for (uint32_t y = 0; y < f->height; y++) {
			const uint32_t cy = f->y + y;
			const int prow = cy >= p->y && cy < p->y + p->height;
			for (uint32_t x = 0; x < f->width; x++) {
				const uint32_t cx = f->x + x;
				uint32_t s = f->argb[(size_t)y * f->width + x];
				/* (where the previous frame's disposal has just cleared the canvas, the source stands as it is) */
				const int cleared = p->dispose && prow && cx >= p->x && cx < p->x + p->width;
				if (blends && !cleared) s = blend_pixel(s, cur[(size_t)cy * cw + cx]);
				cur[(size_t)cy * cw + cx] = s;
			}
		}
		memcpy(disposed, cur, px * sizeof(uint32_t));
		if (f->dispose)
			for (uint32_t y = 0; y < f->height; y++) memset(disposed + (size_t)(f->y + y) * cw + f->x, 0, (size_t)f->width * sizeof(uint32_t));
	}
	free(disposed);
	free(fr);
	return rc;
}
