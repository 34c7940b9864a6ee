/*
 * vp8_alpha.c -- the ALPH chunk of an extended .webp (RFC 9649 2.7.1.2): header byte, raw or
 * lossless-compressed residual plane, and the sequential restatement of the un-prediction.
 *
 * Compression 1 is a complete decoder of the RFC's lossless image stream (3.4 - 3.7, 5) of implicit
 * size w x h: the four transforms (colour indexing with its 1/2/4/8-bit packing), normal and simple
 * prefix codes, the entropy image, LZ77 backward references with the short-distance map, and the
 * colour cache.  Written from the RFC text.  For ALPH only the green channel leaves: it is the residual
 * plane that the un-prediction (on the device: csrc/vp8g_alpha.hip) turns into alpha.
 *
 * The same decoder serves lossless main images (VP8L chunks) in two halves: vp8f_lossless_decode
 * (the 5-byte header, then the entropy half: the residual ARGB image and the transforms, nothing inverted) and
 * vp8f_lossless_apply (the inverse transforms, sequentially: the restatement of csrc/vp8g_lossless.hip).
 *
 * Reentrant: all state is on the stack or in allocations owned by the call.  Every read of the
 * stream is bounds-checked (a read past the end yields zero bits and marks the stream as ended,
 * which fails the decode); every allocation is bounded by the picture size (pixels, the entropy image,
 * one prefix-code group per entropy-image pixel at most) or by the symbols the stream has spelled out.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "vp8_front.h"

/* ---- bit reader (LSB first) -------------------------------------------------------------- */

typedef struct {
	const uint8_t* p;
	size_t size;
	uint64_t pos, nbits; /* in bits */
	int eos;
} BitRd;

static uint32_t br_peek(const BitRd* b) { /* the next 32 - 7 = 25 bits at least; zero beyond the end */
	const size_t byte = (size_t)(b->pos >> 3);
	uint64_t v = 0;
	if (byte < b->size) {
		const size_t avail = b->size - byte;
		memcpy(&v, b->p + byte, avail >= 8 ? 8 : avail);
	}
	return (uint32_t)(v >> (b->pos & 7u));
}

static void br_skip(BitRd* b, unsigned n) {
	if (b->pos + n > b->nbits) {
		b->eos = 1;
		b->pos = b->nbits;
	} else {
		b->pos += n;
	}
}

static uint32_t br_read(BitRd* b, unsigned n) { /* n <= 24 */
	if (n == 0) return 0;
	const uint32_t v = br_peek(b) & ((1u << n) - 1u);
	br_skip(b, n);
	return b->eos ? 0 : v;
}

/* ---- prefix codes ------------------------------------------------------------------------- */

#define MAX_LEN 15
#define LUT_BITS 8
#define ALPHABET_MAX (256 + 24 + 2048)

/* A canonical prefix code: the symbols in use sorted by (length, value) in sym[0 .. nsym), and a
 * table for codes of up to LUT_BITS bits (entry = length << 12 | symbol, 0 = a longer code). */
typedef struct {
	uint16_t count[MAX_LEN + 1];
	uint16_t lut[1 << LUT_BITS];
	uint32_t sym0; /* index of the code's first symbol in the symbol arena */
	uint32_t nsym;
} Code;

typedef struct {
	uint16_t* v;
	size_t n, cap;
	int fixed; /* v is the caller's array: never reallocated */
} SymArena;

typedef struct {
	Code c[5]; /* green + length + cache, red, blue, alpha, distance */
} Group;

static int arena_reserve(SymArena* a, size_t extra) {
	if (a->n + extra <= a->cap) return 0;
	if (a->fixed) {
		errno = EINVAL;
		return -1;
	}
	size_t cap = a->cap ? a->cap * 2 : 1024;
	while (cap < a->n + extra) cap *= 2;
	uint16_t* nv = (uint16_t*)realloc(a->v, cap * sizeof(uint16_t));
	if (!nv) {
		errno = ENOMEM;
		return -1;
	}
	a->v = nv, a->cap = cap;
	return 0;
}

/* Build the code of lengths len[0 .. n).  The tree must be complete, or hold one leaf (which then
 * costs no bits).  0, or -1 (errno set: EINVAL or ENOMEM). */
static int code_build(Code* c, const uint8_t* len, uint32_t n, SymArena* a) {
	memset(c, 0, sizeof(*c));
	uint32_t used = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (len[i] > MAX_LEN) goto bad;
		if (len[i]) c->count[len[i]]++, used++;
	}
	if (used == 0) goto bad;
	if (used > 1) {
		uint32_t kraft = 0;
		for (int l = 1; l <= MAX_LEN; l++) kraft += (uint32_t)c->count[l] << (MAX_LEN - l);
		if (kraft != 1u << MAX_LEN) goto bad;
	}
	if (arena_reserve(a, used) != 0) return -1;
	c->sym0 = (uint32_t)a->n, c->nsym = used;
	uint32_t offs[MAX_LEN + 2];
	offs[1] = 0;
	for (int l = 1; l <= MAX_LEN; l++) offs[l + 1] = offs[l] + c->count[l];
	uint16_t* sym = a->v + a->n;
	for (uint32_t i = 0; i < n; i++)
		if (len[i]) sym[offs[len[i]]++] = (uint16_t)i;
	a->n += used;
	if (used == 1) return 0;
	/* canonical codes in increasing order; the stream holds a code's most significant bit first */
	uint32_t code = 0, k = 0;
	for (int l = 1; l <= LUT_BITS; l++) {
		for (uint32_t j = 0; j < c->count[l]; j++, k++, code++) {
			uint32_t rev = 0;
			for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
			for (uint32_t hi = rev; hi < (1u << LUT_BITS); hi += 1u << l) c->lut[hi] = (uint16_t)((uint32_t)l << 12 | sym[k]);
		}
		code <<= 1;
	}
	return 0;
bad:
	errno = EINVAL;
	return -1;
}

static uint32_t code_read(const Code* c, const uint16_t* arena, BitRd* b) {
	const uint16_t* sym = arena + c->sym0;
	if (c->nsym == 1) return sym[0];
	const uint32_t bits = br_peek(b);
	const uint32_t e = c->lut[bits & ((1u << LUT_BITS) - 1u)];
	if (e) {
		br_skip(b, e >> 12);
		return e & 0xFFFu;
	}
	uint32_t code = 0, first = 0, index = 0;
	for (int l = 1; l <= MAX_LEN; l++) {
		code |= (bits >> (l - 1)) & 1u;
		const uint32_t cnt = c->count[l];
		if (code < first + cnt) {
			br_skip(b, (unsigned)l);
			return sym[index + (code - first)];
		}
		index += cnt, first = (first + cnt) << 1, code <<= 1;
	}
	b->eos = 1; /* (unreachable for a complete tree) */
	return 0;
}

static const uint8_t kCodeLengthOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

static int code_parse(Code* c, uint32_t alphabet, BitRd* b, SymArena* a, Vp8fAlphaStats* st) {
	uint8_t len[ALPHABET_MAX];
	memset(len, 0, alphabet);
	if (br_read(b, 1)) { /* simple */
		const uint32_t nsym = br_read(b, 1) + 1u;
		const uint32_t s0 = br_read(b, br_read(b, 1) ? 8 : 1);
		const uint32_t s1 = nsym == 2 ? br_read(b, 8) : s0;
		if (b->eos || s0 >= alphabet || s1 >= alphabet) goto bad;
		len[s0] = len[s1] = 1;
		st->simple_codes++;
	} else {
		uint8_t cl[19] = {0};
		const uint32_t ncl = 4u + br_read(b, 4);
		for (uint32_t i = 0; i < ncl; i++) cl[kCodeLengthOrder[i]] = (uint8_t)br_read(b, 3);
		if (b->eos) goto bad;
		Code cc;
		SymArena ca = {0};
		uint16_t cbuf[19];
		ca.v = cbuf, ca.cap = 19, ca.fixed = 1;
		if (code_build(&cc, cl, 19, &ca) != 0) return -1;
		uint32_t max_symbol = alphabet;
		if (br_read(b, 1)) {
			const uint32_t nb = 2u + 2u * br_read(b, 3);
			max_symbol = 2u + br_read(b, nb);
			if (max_symbol > alphabet) goto bad;
		}
		uint32_t s = 0, prev = 8;
		while (s < alphabet && max_symbol-- > 0) {
			const uint32_t v = code_read(&cc, cbuf, b);
			if (b->eos) goto bad;
			if (v < 16) {
				len[s++] = (uint8_t)v;
				if (v) prev = v;
				continue;
			}
			const uint32_t rep = v == 16 ? 3u + br_read(b, 2) : v == 17 ? 3u + br_read(b, 3) : 11u + br_read(b, 7);
			if (b->eos || s + rep > alphabet) goto bad;
			memset(len + s, v == 16 ? (int)prev : 0, rep);
			s += rep;
			st->repeat_codes[v - 16]++;
		}
		st->normal_codes++;
	}
	return code_build(c, len, alphabet, a);
bad:
	errno = EINVAL;
	return -1;
}

/* ---- entropy-coded image ------------------------------------------------------------------ */

static const int8_t kDistMap[120][2] = {
	{0, 1},  {1, 0},  {1, 1},  {-1, 1}, {0, 2},  {2, 0},  {1, 2},  {-1, 2}, {2, 1},  {-2, 1}, {2, 2},  {-2, 2}, {0, 3},  {3, 0},  {1, 3},
	{-1, 3}, {3, 1},  {-3, 1}, {2, 3},  {-2, 3}, {3, 2},  {-3, 2}, {0, 4},  {4, 0},  {1, 4},  {-1, 4}, {4, 1},  {-4, 1}, {3, 3},  {-3, 3},
	{2, 4},  {-2, 4}, {4, 2},  {-4, 2}, {0, 5},  {3, 4},  {-3, 4}, {4, 3},  {-4, 3}, {5, 0},  {1, 5},  {-1, 5}, {5, 1},  {-5, 1}, {2, 5},
	{-2, 5}, {5, 2},  {-5, 2}, {4, 4},  {-4, 4}, {3, 5},  {-3, 5}, {5, 3},  {-5, 3}, {0, 6},  {6, 0},  {1, 6},  {-1, 6}, {6, 1},  {-6, 1},
	{2, 6},  {-2, 6}, {6, 2},  {-6, 2}, {4, 5},  {-4, 5}, {5, 4},  {-5, 4}, {3, 6},  {-3, 6}, {6, 3},  {-6, 3}, {0, 7},  {7, 0},  {1, 7},
	{-1, 7}, {5, 5},  {-5, 5}, {7, 1},  {-7, 1}, {4, 6},  {-4, 6}, {6, 4},  {-6, 4}, {2, 7},  {-2, 7}, {7, 2},  {-7, 2}, {3, 7},  {-3, 7},
	{7, 3},  {-7, 3}, {5, 6},  {-5, 6}, {6, 5},  {-6, 5}, {8, 0},  {4, 7},  {-4, 7}, {7, 4},  {-7, 4}, {8, 1},  {8, 2},  {6, 6},  {-6, 6},
	{8, 3},  {5, 7},  {-5, 7}, {7, 5},  {-7, 5}, {8, 4},  {6, 7},  {-6, 7}, {7, 6},  {-7, 6}, {8, 5},  {7, 7},  {-7, 7}, {8, 6},  {8, 7},
};

static uint32_t div_up(uint32_t v, unsigned bits) { return (v + (1u << bits) - 1u) >> bits; }

/* LZ77 prefix coding (RFC 5.2.2): a length or distance from its prefix symbol */
static uint32_t prefix_value(uint32_t sym, BitRd* b) {
	if (sym < 4) return sym + 1u;
	const unsigned extra = (sym - 2u) >> 1;
	const uint32_t offset = (2u + (sym & 1u)) << extra;
	return offset + br_read(b, extra) + 1u;
}

/* One entropy-coded image of w x h pixels into a fresh allocation (*out; the caller frees it).
 * level0: the spatially-coded image's own pixels, which may carry an entropy image. */
static int image_decode(BitRd* b, uint32_t w, uint32_t h, int level0, uint32_t** out, Vp8fAlphaStats* st) {
	int rc = -1;
	uint32_t *pix = NULL, *meta = NULL, *cache = NULL;
	Group* groups = NULL;
	SymArena arena = {0};
	int32_t* gmap = NULL;
	uint32_t cache_bits = 0, meta_bits = 0, meta_w = 0, ngroups = 1, nkept = 0;
	*out = NULL;
	if (br_read(b, 1)) {
		cache_bits = br_read(b, 4);
		if (cache_bits < 1 || cache_bits > 11) goto bad;
	}
	if (level0 && br_read(b, 1)) {
		meta_bits = br_read(b, 3) + 2u;
		meta_w = div_up(w, meta_bits);
		const uint32_t meta_h = div_up(h, meta_bits);
		if (b->eos) goto bad;
		if (image_decode(b, meta_w, meta_h, 0, &meta, st) != 0) goto out;
		uint32_t top = 0;
		for (size_t i = 0; i < (size_t)meta_w * meta_h; i++) {
			meta[i] = (meta[i] >> 8) & 0xFFFFu;
			if (meta[i] > top) top = meta[i];
		}
		ngroups = top + 1u;
		if (ngroups > 1) st->multi_group++;
		/* only the groups the entropy image names are kept (at most one per pixel of it): gmap[g] = its
		 * slot, -1 for a group that is in the stream but never used, whose codes are parsed and dropped */
		gmap = (int32_t*)malloc((size_t)ngroups * sizeof(int32_t));
		if (!gmap) {
			errno = ENOMEM;
			goto out;
		}
		memset(gmap, 0xFF, (size_t)ngroups * sizeof(int32_t));
		for (size_t i = 0; i < (size_t)meta_w * meta_h; i++) {
			if (gmap[meta[i]] < 0) gmap[meta[i]] = (int32_t)nkept++;
			meta[i] = (uint32_t)gmap[meta[i]];
		}
	} else {
		nkept = 1;
	}
	if (b->eos) goto bad;
	/* a group takes at least 5 simple codes of 4 bits: more groups than that cannot be in the stream */
	if ((uint64_t)ngroups * 20u > b->nbits - b->pos) goto bad;
	groups = (Group*)malloc(((size_t)nkept + 1u) * sizeof(Group)); /* (+ 1: the slot unused groups are parsed into) */
	pix = (uint32_t*)malloc((size_t)w * h * sizeof(uint32_t));
	if (cache_bits) cache = (uint32_t*)calloc((size_t)1 << cache_bits, sizeof(uint32_t));
	if (!groups || !pix || (cache_bits && !cache)) {
		errno = ENOMEM;
		goto out;
	}
	const uint32_t cache_size = cache_bits ? 1u << cache_bits : 0u;
	for (uint32_t g = 0; g < ngroups; g++) {
		static const uint16_t kAlphabet[5] = {256 + 24, 256, 256, 256, 40};
		const int keep = !gmap || gmap[g] >= 0;
		Group* G = &groups[keep ? (gmap ? (uint32_t)gmap[g] : 0u) : nkept];
		const size_t mark = arena.n;
		for (int k = 0; k < 5; k++)
			if (code_parse(&G->c[k], kAlphabet[k] + (k == 0 ? cache_size : 0u), b, &arena, st) != 0) goto out;
		if (!keep) arena.n = mark;
	}
	const size_t n = (size_t)w * h;
	size_t pos = 0;
	uint32_t x = 0, y = 0;
	const unsigned cshift = 32u - cache_bits;
	while (pos < n) {
		const Group* G = &groups[meta ? meta[(size_t)(y >> meta_bits) * meta_w + (x >> meta_bits)] : 0u];
		const uint32_t s = code_read(&G->c[0], arena.v, b);
		if (s < 256u + 24u) {
			if (s < 256u) {
				const uint32_t r = code_read(&G->c[1], arena.v, b);
				const uint32_t bl = code_read(&G->c[2], arena.v, b);
				const uint32_t al = code_read(&G->c[3], arena.v, b);
				const uint32_t p = al << 24 | r << 16 | s << 8 | bl;
				pix[pos++] = p;
				if (cache) cache[(0x1e35a7bdu * p) >> cshift] = p;
				if (++x == w) x = 0, y++;
			} else {
				const uint32_t length = prefix_value(s - 256u, b);
				const uint32_t dsym = code_read(&G->c[4], arena.v, b);
				const uint32_t dcode = prefix_value(dsym, b);
				uint64_t dist;
				if (dcode > 120u) {
					dist = dcode - 120u;
				} else {
					const int64_t d = kDistMap[dcode - 1u][0] + (int64_t)kDistMap[dcode - 1u][1] * (int64_t)w;
					dist = d < 1 ? 1u : (uint64_t)d;
					st->short_dist++;
				}
				if (b->eos || dist > pos || length > n - pos) goto bad;
				for (uint32_t i = 0; i < length; i++, pos++) {
					const uint32_t p = pix[pos - dist];
					pix[pos] = p;
					if (cache) cache[(0x1e35a7bdu * p) >> cshift] = p;
				}
				x += length;
				while (x >= w) x -= w, y++;
				st->backrefs++;
			}
		} else {
			const uint32_t idx = s - (256u + 24u);
			if (idx >= cache_size) goto bad;
			/* every pixel enters the cache, one read from it too (as libwebp does): a no-op for a slot that was
			 * written, but the 0 of a slot never written goes to slot 0 and replaces what was there */
			const uint32_t p = cache[idx];
			pix[pos++] = p;
			cache[(0x1e35a7bdu * p) >> cshift] = p;
			if (++x == w) x = 0, y++;
			st->cache_hits++;
		}
		if (b->eos) goto bad;
	}
	*out = pix;
	pix = NULL;
	rc = 0;
	goto out;
bad:
	errno = EINVAL;
out:
	free(pix);
	free(meta);
	free(cache);
	free(groups);
	free(gmap);
	free(arena.v);
	return rc;
}

/* ---- transforms --------------------------------------------------------------------------- */

enum { T_PREDICTOR = VP8F_T_PREDICTOR, T_CROSS_COLOR = VP8F_T_CROSS_COLOR, T_SUBTRACT_GREEN = VP8F_T_SUBTRACT_GREEN, T_COLOR_INDEX = VP8F_T_COLOR_INDEX };

typedef Vp8fLosslessTransform Transform; /* (vp8_front.h) */

static uint32_t add_px(uint32_t a, uint32_t b) {
	return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
static uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
static int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static int iabs(int v) { return v < 0 ? -v : v; }
#define CH(p, s) ((int)(((p) >> (s)) & 0xFFu))

static uint32_t pred_select(uint32_t L, uint32_t T, uint32_t TL) {
	int pl = 0, pt = 0; /* distances of L + T - TL to L and to T */
	for (int s = 0; s < 32; s += 8) pl += iabs(CH(T, s) - CH(TL, s)), pt += iabs(CH(L, s) - CH(TL, s));
	return pl < pt ? L : T;
}
static uint32_t pred_clamp_full(uint32_t a, uint32_t b, uint32_t c) {
	uint32_t r = 0;
	for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255(CH(a, s) + CH(b, s) - CH(c, s)) << s;
	return r;
}
static uint32_t pred_clamp_half(uint32_t a, uint32_t b) {
	uint32_t r = 0;
	for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255(CH(a, s) + (CH(a, s) - CH(b, s)) / 2) << s;
	return r;
}

static void inv_predictor(const Transform* t, uint32_t* p, uint32_t h) {
	const uint32_t w = t->xsize, bw = div_up(w, t->bits);
	for (uint32_t y = 0; y < h; y++) {
		uint32_t* row = p + (size_t)y * w;
		const uint32_t* up = row - w; /* (read for y > 0 only) */
		for (uint32_t x = 0; x < w; x++) {
			uint32_t pred;
			if (y == 0) {
				pred = x == 0 ? 0xFF000000u : row[x - 1];
			} else if (x == 0) {
				pred = up[x];
			} else {
				const uint32_t L = row[x - 1], T = up[x], TL = up[x - 1];
				const uint32_t TR = up[x + 1]; /* (rightmost column: the row's first pixel, as the RFC says) */
				switch ((t->data[(size_t)(y >> t->bits) * bw + (x >> t->bits)] >> 8) & 15u) {
					case 1: pred = L; break;
					case 2: pred = T; break;
					case 3: pred = TR; break;
					case 4: pred = TL; break;
					case 5: pred = avg2(avg2(L, TR), T); break;
					case 6: pred = avg2(L, TL); break;
					case 7: pred = avg2(L, T); break;
					case 8: pred = avg2(TL, T); break;
					case 9: pred = avg2(T, TR); break;
					case 10: pred = avg2(avg2(L, TL), avg2(T, TR)); break;
					case 11: pred = pred_select(L, T, TL); break;
					case 12: pred = pred_clamp_full(L, T, TL); break;
					case 13: pred = pred_clamp_half(avg2(L, T), TL); break;
					default: pred = 0xFF000000u; break; /* 0, and 14 / 15 as libwebp reads them */
				}
			}
			row[x] = add_px(row[x], pred);
		}
	}
}

static int delta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }

static void inv_cross_color(const Transform* t, uint32_t* p, uint32_t h) {
	const uint32_t w = t->xsize, bw = div_up(w, t->bits);
	for (uint32_t y = 0; y < h; y++)
		for (uint32_t x = 0; x < w; x++) {
			const uint32_t e = t->data[(size_t)(y >> t->bits) * bw + (x >> t->bits)];
			const uint32_t g2r = e & 255u, g2b = (e >> 8) & 255u, r2b = (e >> 16) & 255u;
			const uint32_t v = p[(size_t)y * w + x], g = (v >> 8) & 255u;
			uint32_t r = (v >> 16) & 255u, b = v & 255u;
			r = (r + (uint32_t)delta(g2r, g)) & 255u;
			b = (b + (uint32_t)delta(g2b, g)) & 255u;
			b = (b + (uint32_t)delta(r2b, r)) & 255u;
			p[(size_t)y * w + x] = (v & 0xFF00FF00u) | r << 16 | b;
		}
}

static void inv_subtract_green(uint32_t* p, size_t n) {
	for (size_t i = 0; i < n; i++) {
		const uint32_t g = (p[i] >> 8) & 255u;
		p[i] = (p[i] & 0xFF00FF00u) | (((p[i] & 0x00FF00FFu) + (g << 16 | g)) & 0x00FF00FFu);
	}
}

/* src: packed pixels, div_up(w, bits) per row; dst: w per row (another buffer) */
static void inv_color_index(const Transform* t, const uint32_t* src, uint32_t* dst, uint32_t h) {
	const uint32_t w = t->xsize, pw = div_up(w, t->bits);
	const unsigned bpp = 8u >> t->bits;
	const uint32_t mask = (1u << bpp) - 1u, per = (1u << t->bits) - 1u;
	for (uint32_t y = 0; y < h; y++)
		for (uint32_t x = 0; x < w; x++) {
			const uint32_t packed = (src[(size_t)y * pw + (x >> t->bits)] >> 8) & 255u;
			const uint32_t idx = (packed >> ((x & per) * bpp)) & mask;
			dst[(size_t)y * w + x] = idx < t->ncolors ? t->data[idx] : 0u;
		}
}

/* The entropy half: the transforms' headers and data, then the spatially-coded image, of a stream
 * of implicit size w x h.  On failure *im is left for vp8f_lossless_free. */
static int lossless_entropy(const uint8_t* data, size_t size, uint32_t w, uint32_t h, Vp8fLosslessImage* im, Vp8fAlphaStats* st) {
	BitRd b = {data, size, 0, (uint64_t)size * 8u, 0};
	unsigned seen = 0;
	uint32_t xsize = w;
	im->width = w, im->height = h;
	while (br_read(&b, 1)) {
		const int type = (int)br_read(&b, 2);
		if (b.eos || (seen & (1u << type))) goto bad;
		seen |= 1u << type;
		Transform* t = &im->tr[im->ntransforms++];
		t->type = (uint32_t)type, t->xsize = xsize;
		if (type == T_PREDICTOR || type == T_CROSS_COLOR) {
			t->bits = br_read(&b, 3) + 2u;
			if (b.eos) goto bad;
			if (image_decode(&b, div_up(xsize, t->bits), div_up(h, t->bits), 0, &t->data, st) != 0) return -1;
			if (type == T_PREDICTOR) st->predictor++;
			else st->cross_color++;
		} else if (type == T_COLOR_INDEX) {
			t->ncolors = br_read(&b, 8) + 1u;
			t->bits = t->ncolors > 16 ? 0 : t->ncolors > 4 ? 1 : t->ncolors > 2 ? 2 : 3;
			if (b.eos) goto bad;
			if (image_decode(&b, t->ncolors, 1, 0, &t->data, st) != 0) return -1;
			for (uint32_t i = 1; i < t->ncolors; i++) t->data[i] = add_px(t->data[i], t->data[i - 1]);
			xsize = div_up(xsize, t->bits);
			st->color_index++;
			st->pack_bits[3 - t->bits]++;
		} else {
			st->subtract_green++;
		}
	}
	im->xsize = xsize;
	if (b.eos) goto bad;
	if (image_decode(&b, xsize, h, 1, &im->argb, st) != 0) return -1;
	st->lossless++;
	return 0;
bad:
	errno = EINVAL;
	return -1;
}

/* The inverse half, in place on pix (im->xsize x height on entry, a malloc'ed buffer that colour
 * indexing replaces); *out = the width x height result. */
static int lossless_inverse(const Vp8fLosslessImage* im, uint32_t* pix, uint32_t** out) {
	const uint32_t h = im->height;
	uint32_t xsize = im->xsize;
	*out = pix;
	for (int i = (int)im->ntransforms - 1; i >= 0; i--) {
		const Transform* t = &im->tr[i];
		/* (the width the transform works at: everything read after a colour indexing transform sees the
		 * packed width, which is that transform's input) */
		switch (t->type) {
			case T_PREDICTOR: inv_predictor(t, pix, h); break;
			case T_CROSS_COLOR: inv_cross_color(t, pix, h); break;
			case T_SUBTRACT_GREEN: inv_subtract_green(pix, (size_t)xsize * h); break;
			default: {
				uint32_t* wide = (uint32_t*)malloc((size_t)t->xsize * h * sizeof(uint32_t));
				if (!wide) {
					errno = ENOMEM;
					return -1;
				}
				inv_color_index(t, pix, wide, h);
				free(pix);
				*out = pix = wide;
				xsize = t->xsize;
				break;
			}
		}
	}
	return 0;
}

static int lossless_decode(const uint8_t* data, size_t size, uint32_t w, uint32_t h, uint8_t* residual, Vp8fAlphaStats* st) {
	Vp8fLosslessImage im;
	memset(&im, 0, sizeof(im));
	int rc = lossless_entropy(data, size, w, h, &im, st);
	if (rc == 0) {
		uint32_t* pix = im.argb;
		im.argb = NULL;
		rc = lossless_inverse(&im, pix, &pix);
		if (rc == 0)
			for (size_t i = 0; i < (size_t)w * h; i++) residual[i] = (uint8_t)(pix[i] >> 8);
		free(pix);
	}
	const int e = errno;
	vp8f_lossless_free(&im);
	errno = e;
	return rc;
}

/* ---- public ------------------------------------------------------------------------------- */

int vp8f_alpha_decode(const uint8_t* alph, size_t size, uint32_t w, uint32_t h, uint8_t* residual, uint32_t* filter,
                      Vp8fAlphaStats* stats) {
	Vp8fAlphaStats local;
	Vp8fAlphaStats* st = stats ? stats : &local;
	memset(st, 0, sizeof(*st));
	if (!alph || !residual || !filter || size < 1 || w == 0 || h == 0 || w > 16383 || h > 16383) {
		errno = EINVAL;
		return -1;
	}
	const unsigned compression = alph[0] & 3u;
	*filter = (alph[0] >> 2) & 3u; /* pre-processing (bits 4-5) and the reserved bits are ignored */
	if (compression == 0) {
		if (size - 1 < (size_t)w * h) {
			errno = EINVAL;
			return -1;
		}
		memcpy(residual, alph + 1, (size_t)w * h);
		st->raw++;
		return 0;
	}
	if (compression != 1) {
		errno = EINVAL;
		return -1;
	}
	return lossless_decode(alph + 1, size - 1, w, h, residual, st);
}

int vp8f_alpha_unfilter(const uint8_t* residual, uint32_t w, uint32_t h, uint32_t filter, uint8_t* out) {
	if (!residual || !out || w == 0 || h == 0 || filter > 3) {
		errno = EINVAL;
		return -1;
	}
	for (uint32_t y = 0; y < h; y++) {
		const uint8_t* r = residual + (size_t)y * w;
		uint8_t* o = out + (size_t)y * w;
		const uint8_t* up = o - w;
		for (uint32_t x = 0; x < w; x++) {
			int pred;
			if (filter == 0 || (x == 0 && y == 0)) pred = 0;
			else if (y == 0) pred = o[x - 1];
			else if (x == 0) pred = up[0];
			else if (filter == 1) pred = o[x - 1];
			else if (filter == 2) pred = up[x];
			else pred = clamp255((int)o[x - 1] + (int)up[x] - (int)up[x - 1]);
			o[x] = (uint8_t)(pred + r[x]);
		}
	}
	return 0;
}

void vp8f_lossless_free(Vp8fLosslessImage* im) {
	if (!im) return;
	for (int i = 0; i < 4; i++) free(im->tr[i].data);
	free(im->argb);
	memset(im, 0, sizeof(*im));
}

int vp8f_lossless_decode(const uint8_t* data, size_t size, Vp8fLosslessImage* out, Vp8fAlphaStats* stats) {
	Vp8fAlphaStats local;
	Vp8fAlphaStats* st = stats ? stats : &local;
	memset(st, 0, sizeof(*st));
	if (out) memset(out, 0, sizeof(*out));
	uint32_t w, h, hint;
	if (!out || vp8f_lossless_header(data, size, &w, &h, &hint) != 0) {
		errno = EINVAL;
		return -1;
	}
	if (w > 16383 || h > 16383) { /* (as every other entry point of the project) */
		errno = EINVAL;
		return -1;
	}
	out->alpha_hint = hint;
	if (lossless_entropy(data + 5, size - 5, w, h, out, st) != 0) {
		const int e = errno;
		vp8f_lossless_free(out);
		errno = e;
		return -1;
	}
	return 0;
}

int vp8f_lossless_apply(const Vp8fLosslessImage* im, uint32_t* argb) {
	if (!im || !argb || !im->argb || im->width == 0 || im->height == 0 || im->xsize == 0 || im->ntransforms > 4) {
		errno = EINVAL;
		return -1;
	}
	const size_t n = (size_t)im->xsize * im->height;
	uint32_t* pix = (uint32_t*)malloc(n * sizeof(uint32_t));
	if (!pix) {
		errno = ENOMEM;
		return -1;
	}
	memcpy(pix, im->argb, n * sizeof(uint32_t));
	const int rc = lossless_inverse(im, pix, &pix);
	if (rc == 0) memcpy(argb, pix, (size_t)im->width * im->height * sizeof(uint32_t));
	free(pix);
	return rc;
}
