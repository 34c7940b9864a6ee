/*
 * vp8_scale.c -- crop + downscale of an I420 image, bit-exact to libwebp 1.2.2's rescaler
 * (the `use_cropping` / `use_scaling` decoder options, `dwebp -crop x y w h -scale w h`, and
 * WebPPictureRescale for 4:2:0 pictures).
 *
 * This is the sequential host restatement: the CPU path, and the checker of the device kernel
 * (csrc/vp8g_scale.hip, which evaluates the same sums in closed form).  It is written from the
 * rescaler's arithmetic as DESIGN.md §14 states it: per plane W x H -> w x h, every value a wrapping
 * uint32_t.  Shrinking (w <= W, h <= H):
 *
 *   fx = 2^32 / w, fy = 2^32 / h, fxy = (h * 2^32) / (W * H)   (0 when it does not fit 32 bits)
 *   MULT(x, y) = (x * y + 2^31) >> 32, FLOOR(x, y) = (x * y) >> 32       (64-bit products)
 *
 * a source row is imported into w horizontal sums (each source sample split between the two
 * outputs it straddles, the split carried through MULT(., fx)), imported rows accumulate, and an
 * output row is exported whenever the vertical accumulator runs out, the straddling row split
 * with FLOOR(., fy * remainder) and the total scaled by MULT(., fxy).
 *
 * Expanding (VP8G_SCALE_EXPAND; per plane and per axis, xe = W < w, ye = H < h) is libwebp's
 * bilinear path.  With xe, x_add = w - 1 and x_sub = W - 1 and a row is imported as
 * frow[k] = R * x_add + (L - R) * accum over the two source samples L, R that output k lies between
 * (fx unused; a shrinking y then uses fxy = (h * 2^32) / ((w - 1) * H)).  With ye, y_add = H - 1,
 * y_sub = h - 1, fy = 2^32 / x_add, nothing accumulates: irow and frow swap before every import so
 * that they hold the last two imported rows, and an output row is their blend
 * MULT((A * frow + B * irow + 2^31) >> 32, fy) with B = (-y_accum * 2^32) / y_sub, A = 2^32 - B
 * (MULT(frow, fy) when y_accum is 0).
 *
 * Luma is scaled from the (cropped) window to the target size, each chroma plane from
 * ceil(window / 2) to ceil(target / 2), independently, each with its own mode.  Without
 * VP8G_SCALE_EXPAND a target beyond the window in either dimension is EINVAL.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "vp8_front.h"

#define SCALE_MAX_DIM 16383u /* VP8's 14-bit frame size; keeps every product below 2^28 */

static uint32_t mult_fix(uint32_t x, uint32_t y) { return (uint32_t)(((uint64_t)x * y + (1ull << 31)) >> 32); }
static uint32_t mult_floor(uint32_t x, uint32_t y) { return (uint32_t)(((uint64_t)x * y) >> 32); }

/* snap: the window's origin is rounded down to even (I420), or taken as given (ARGB) */
static int resolve(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, Vp8fScaleGeom* g, int snap) {
	if (!opt || !g || width == 0 || height == 0 || width > SCALE_MAX_DIM || height > SCALE_MAX_DIM ||
	    (opt->flags & ~(VP8G_SCALE_DWEBP_FILTER | VP8G_SCALE_EXPAND)))
		goto bad;
	{
		const int expand = (opt->flags & VP8G_SCALE_EXPAND) != 0;
		uint32_t left = 0, top = 0, ww = width, wh = height;
		if (opt->crop_left | opt->crop_top | opt->crop_w | opt->crop_h) {
			/* libwebp's rules: the size as given, the origin snapped down to even (I420 only);
			 * the bounds are checked with the caller's own values */
			if (opt->crop_w == 0 || opt->crop_h == 0 || (uint64_t)opt->crop_left + opt->crop_w > width ||
			    (uint64_t)opt->crop_top + opt->crop_h > height)
				goto bad;
			left = snap ? opt->crop_left & ~1u : opt->crop_left, top = snap ? opt->crop_top & ~1u : opt->crop_top;
			ww = opt->crop_w, wh = opt->crop_h;
		}
		uint32_t ow = opt->scaled_w, oh = opt->scaled_h;
		if (ow == 0 && oh == 0) {
			ow = ww, oh = wh; /* crop only */
		} else if (ow == 0) {
			if (expand ? oh > SCALE_MAX_DIM : oh > wh) goto bad;
			ow = (uint32_t)(((uint64_t)ww * oh + wh - 1u) / wh);
		} else if (oh == 0) {
			if (expand ? ow > SCALE_MAX_DIM : ow > ww) goto bad;
			oh = (uint32_t)(((uint64_t)wh * ow + ww - 1u) / ww);
		}
		if (ow == 0 || oh == 0) goto bad;
		if (expand ? (ow > SCALE_MAX_DIM || oh > SCALE_MAX_DIM) : (ow > ww || oh > wh)) goto bad; /* downscale only */
		g->left = left, g->top = top, g->win_w = ww, g->win_h = wh, g->out_w = ow, g->out_h = oh;
		g->scaling = (opt->scaled_w | opt->scaled_h) != 0;
		return 0;
	}
bad:
	errno = EINVAL;
	return -1;
}

int vp8f_scale_resolve(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, Vp8fScaleGeom* g) {
	return resolve(width, height, opt, g, 1);
}

int vp8f_scale_resolve_argb(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, Vp8fScaleGeom* g) {
	return resolve(width, height, opt, g, 0);
}

int vp8f_scale_filtered(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, int filtered) {
	Vp8fScaleGeom g;
	if (!filtered) return 0;
	if (!opt || !(opt->flags & VP8G_SCALE_DWEBP_FILTER) || vp8f_scale_resolve(width, height, opt, &g) != 0 || !g.scaling)
		return 1;
	/* libwebp: the full picture size, integer products, strict inequalities */
	return !(g.out_w < width * 3u / 4u && g.out_h < height * 3u / 4u);
}

void vp8f_scale_factors(uint32_t W, uint32_t H, uint32_t w, uint32_t h, uint32_t* fx, uint32_t* fy, uint32_t* fxy) {
	const int xe = W < w, ye = H < h;
	const uint32_t x_add = xe ? w - 1u : W, x_sub = xe ? W - 1u : w;
	*fx = xe ? 0u : (uint32_t)((1ull << 32) / x_sub);
	if (ye) {
		*fy = (uint32_t)((1ull << 32) / x_add);
		*fxy = 0u;
	} else {
		const uint64_t ratio = ((uint64_t)h << 32) / ((uint64_t)x_add * H);
		*fy = (uint32_t)((1ull << 32) / h);
		*fxy = (ratio >> 32) ? 0u : (uint32_t)ratio;
	}
}

/* import: the horizontal sums of one source row (shrinking or identity) */
static void import_shrink(const uint8_t* src, uint32_t W, uint32_t w, uint32_t fx, uint32_t* frow) {
	uint32_t x_in = 0, sum = 0;
	int32_t accum = 0;
	for (uint32_t k = 0; k < w; k++) {
		uint32_t base = 0;
		accum += (int32_t)W;
		while (accum > 0) {
			accum -= (int32_t)w;
			base = src[x_in++];
			sum += base;
		}
		const uint32_t frac = base * (uint32_t)(-accum);
		frow[k] = sum * w - frac;
		sum = mult_fix(frac, fx);
	}
}

/* import: bilinear interpolation of one source row (W < w) */
static void import_expand(const uint8_t* src, uint32_t W, uint32_t w, uint32_t* frow) {
	const uint32_t x_add = w - 1u, x_sub = W - 1u;
	uint32_t x_in = 0, left = src[0], right = W > 1u ? src[1] : left;
	int32_t accum = (int32_t)x_add;
	x_in++;
	for (uint32_t k = 0;;) {
		frow[k] = right * x_add + (left - right) * (uint32_t)accum;
		if (++k >= w) break;
		accum -= (int32_t)x_sub;
		if (accum < 0) {
			left = right;
			right = src[++x_in];
			accum += (int32_t)x_add;
		}
	}
}

/* work: 2 * w words */
static void scale_plane(const uint8_t* s, uint32_t ss, uint32_t W, uint32_t H, uint8_t* d, uint32_t ds, uint32_t w,
                        uint32_t h, uint32_t* work) {
	uint32_t fx, fy, fxy;
	vp8f_scale_factors(W, H, w, h, &fx, &fy, &fxy);
	const int xe = W < w, ye = H < h;
	const uint32_t y_add = ye ? H - 1u : H, y_sub = ye ? h - 1u : h;
	uint32_t* irow = work;
	uint32_t* frow = work + w;
	memset(work, 0, (size_t)2 * w * sizeof(uint32_t));
	int32_t y_accum = (int32_t)(ye ? y_sub : y_add);
	uint32_t y = 0, dy = 0;
	while (dy < h) {
		while (y_accum > 0 && y < H) { /* import until an output row is due */
			if (ye) {
				uint32_t* const tmp = irow;
				irow = frow, frow = tmp;
			}
			if (xe) import_expand(s + (size_t)y * ss, W, w, frow);
			else import_shrink(s + (size_t)y * ss, W, w, fx, frow);
			if (!ye)
				for (uint32_t k = 0; k < w; k++) irow[k] += frow[k];
			y++;
			y_accum -= (int32_t)y_sub;
		}
		if (y_accum > 0) break; /* (never: the source rows run out with the last output row) */
		/* export one output row */
		uint8_t* dst = d + (size_t)dy * ds;
		if (ye) {
			if (y_accum == 0) {
				for (uint32_t k = 0; k < w; k++) {
					const int32_t v = (int32_t)mult_fix(frow[k], fy);
					dst[k] = v > 255 ? 255u : (uint8_t)v;
				}
			} else {
				const uint32_t B = (uint32_t)(((uint64_t)(uint32_t)(-y_accum) << 32) / y_sub);
				const uint32_t A = (uint32_t)((1ull << 32) - B);
				for (uint32_t k = 0; k < w; k++) {
					const uint64_t I = (uint64_t)A * frow[k] + (uint64_t)B * irow[k];
					const uint32_t J = (uint32_t)((I + (1ull << 31)) >> 32);
					const int32_t v = (int32_t)mult_fix(J, fy);
					dst[k] = v > 255 ? 255u : (uint8_t)v;
				}
			}
		} else {
			const uint32_t yscale = fy * (uint32_t)(-y_accum);
			if (fxy == 0) { /* x_add == 1 and h == H: the sums are the samples */
				for (uint32_t k = 0; k < w; k++) dst[k] = (uint8_t)irow[k], irow[k] = 0;
			} else if (yscale) {
				for (uint32_t k = 0; k < w; k++) {
					const uint32_t frac = mult_floor(frow[k], yscale);
					const int32_t v = (int32_t)mult_fix(irow[k] - frac, fxy);
					dst[k] = v > 255 ? 255u : (uint8_t)v;
					irow[k] = frac;
				}
			} else {
				for (uint32_t k = 0; k < w; k++) {
					const int32_t v = (int32_t)mult_fix(irow[k], fxy);
					dst[k] = v > 255 ? 255u : (uint8_t)v;
					irow[k] = 0;
				}
			}
		}
		y_accum += (int32_t)y_add;
		dy++;
	}
}

int vp8f_scale_i420(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t stride_y, uint32_t stride_uv,
                    uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint8_t* dy, uint8_t* du, uint8_t* dv,
                    uint32_t dstride_y, uint32_t dstride_uv) {
	Vp8fScaleGeom g;
	if (!y || !u || !v || !dy || !du || !dv || vp8f_scale_resolve(width, height, opt, &g) != 0 || stride_y < width ||
	    stride_uv < (width + 1u) / 2u || dstride_y < g.out_w || dstride_uv < (g.out_w + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	uint32_t* work = (uint32_t*)malloc((size_t)2 * g.out_w * sizeof(uint32_t));
	if (!work) {
		errno = ENOMEM;
		return -1;
	}
	const uint32_t cw = (g.win_w + 1u) / 2u, ch = (g.win_h + 1u) / 2u, ocw = (g.out_w + 1u) / 2u, och = (g.out_h + 1u) / 2u;
	const size_t co = (size_t)(g.top / 2u) * stride_uv + g.left / 2u;
	scale_plane(y + (size_t)g.top * stride_y + g.left, stride_y, g.win_w, g.win_h, dy, dstride_y, g.out_w, g.out_h, work);
	scale_plane(u + co, stride_uv, cw, ch, du, dstride_uv, ocw, och, work);
	scale_plane(v + co, stride_uv, cw, ch, dv, dstride_uv, ocw, och, work);
	free(work);
	return 0;
}

/* libwebp's scaled RGB of a lossy picture (WebPDecode with use_scaling into MODE_RGB / MODE_RGBA, dwebp -ppm -scale;
 * DESIGN.md §14.2): Y, U and V each go straight to the target size -- chroma from its own window, ceil(window / 2) at
 * (left / 2, top / 2), each axis shrinking or expanding as its own sizes say whatever VP8G_SCALE_EXPAND says of luma --
 * and the pixel is VP8YuvToRgb of the three samples; no upsampler. */
int vp8f_scale_yuv444(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t stride_y, uint32_t stride_uv,
                      uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint8_t* dy, uint8_t* du, uint8_t* dv) {
	Vp8fScaleGeom g;
	if (!y || !u || !v || !dy || !du || !dv || vp8f_scale_resolve(width, height, opt, &g) != 0 || !g.scaling || stride_y < width ||
	    stride_uv < (width + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	uint32_t* work = (uint32_t*)malloc((size_t)2 * g.out_w * sizeof(uint32_t));
	if (!work) {
		errno = ENOMEM;
		return -1;
	}
	const uint32_t cw = (g.win_w + 1u) / 2u, ch = (g.win_h + 1u) / 2u;
	const size_t co = (size_t)(g.top / 2u) * stride_uv + g.left / 2u;
	scale_plane(y + (size_t)g.top * stride_y + g.left, stride_y, g.win_w, g.win_h, dy, g.out_w, g.out_w, g.out_h, work);
	scale_plane(u + co, stride_uv, cw, ch, du, g.out_w, g.out_w, g.out_h, work);
	scale_plane(v + co, stride_uv, cw, ch, dv, g.out_w, g.out_w, g.out_h, work);
	free(work);
	return 0;
}

/* ---- ARGB pictures (lossless files): libwebp's 4-channel rescaler ------------------------------
 *
 * libwebp rescales the rows of a VP8L picture as four interleaved byte channels, each with exactly the
 * single-plane arithmetic above, between an alpha premultiply and its inverse.  The
 * window's origin is taken as given (no even rounding: there is no chroma to stay aligned with), and a
 * crop without a target size copies the window's pixels untouched. */

#define ARGB_MFIX 24
#define ARGB_HALF (1u << (ARGB_MFIX - 1))
#define ARGB_KINV_255 ((1u << ARGB_MFIX) / 255u) /* 65793 */

void vp8f_argb_mult_row(uint32_t* px, uint32_t n, int inverse) {
	for (uint32_t x = 0; x < n; x++) {
		const uint32_t p = px[x], a = p >> 24;
		if (a == 255u) continue;
		if (a == 0u) {
			px[x] = 0;
			continue;
		}
		const uint32_t scale = inverse ? (255u << ARGB_MFIX) / a : a * ARGB_KINV_255;
		uint32_t out = p & 0xFF000000u;
		for (int s = 0; s < 24; s += 8) {
			/* (premultiply: 255 * 255 * 65793 + 2^23 < 2^32; the inverse's product needs 64 bits in general) */
			const uint64_t v = ((uint64_t)((p >> s) & 255u) * scale + ARGB_HALF) >> ARGB_MFIX;
			out |= (uint32_t)(v & 255u) << s;
		}
		px[x] = out;
	}
}

int vp8f_argb_scale(const uint32_t* argb, uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint32_t* out) {
	Vp8fScaleGeom g;
	if (!argb || !out || vp8f_scale_resolve_argb(width, height, opt, &g) != 0) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t* win = argb + (size_t)g.top * width + g.left;
	if (!g.scaling) { /* crop only: libwebp emits the window's rows as they are */
		for (uint32_t y = 0; y < g.win_h; y++) memcpy(out + (size_t)y * g.win_w, win + (size_t)y * width, (size_t)g.win_w * 4u);
		return 0;
	}
	const size_t wsz = (size_t)g.win_w * g.win_h, osz = (size_t)g.out_w * g.out_h;
	uint32_t* row = (uint32_t*)malloc(((size_t)g.win_w + 2u * g.out_w) * sizeof(uint32_t));
	uint8_t* planes = (uint8_t*)malloc(4u * (wsz + osz));
	if (!row || !planes) {
		free(row), free(planes);
		errno = ENOMEM;
		return -1;
	}
	/* premultiply the window's rows; channel c of a pixel is byte c of the dword: B, G, R, A */
	for (uint32_t y = 0; y < g.win_h; y++) {
		memcpy(row, win + (size_t)y * width, (size_t)g.win_w * 4u);
		vp8f_argb_mult_row(row, g.win_w, 0);
		for (uint32_t x = 0; x < g.win_w; x++)
			for (uint32_t c = 0; c < 4u; c++) planes[c * wsz + (size_t)y * g.win_w + x] = (uint8_t)(row[x] >> (8u * c));
	}
	uint8_t* scaled = planes + 4u * wsz;
	for (uint32_t c = 0; c < 4u; c++)
		scale_plane(planes + c * wsz, g.win_w, g.win_w, g.win_h, scaled + c * osz, g.out_w, g.out_w, g.out_h, row + g.win_w);
	int ok = 1;
	for (uint32_t y = 0; y < g.out_h; y++) {
		uint32_t* o = out + (size_t)y * g.out_w;
		for (uint32_t x = 0; x < g.out_w; x++) {
			const size_t i = (size_t)y * g.out_w + x;
			const uint32_t b = scaled[i], gr = scaled[osz + i], r = scaled[2u * osz + i], a = scaled[3u * osz + i];
			/* every channel is the same monotone function of sums in which colour <= alpha holds termwise: the
			 * inverse below therefore stays within a byte */
			ok &= b <= a && gr <= a && r <= a;
			o[x] = a << 24 | r << 16 | gr << 8 | b;
		}
		vp8f_argb_mult_row(o, g.out_w, 1);
	}
	free(row), free(planes);
	if (!ok) { /* (never) */
		errno = ERANGE;
		return -1;
	}
	return 0;
}
