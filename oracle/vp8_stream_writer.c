/*
 * vp8_stream_writer.c -- TEST INFRASTRUCTURE (oracle/libstreamw.so); never linked into the product.
 *
 * The inverse of m05: writes a Vp8DecodedFrame (header fields and arrays) as a complete simple-lossy
 * .webp -- RIFF, the `VP8 ` chunk, frame tag, start code, size fields, partition 0 and 1/2/4/8 token
 * partitions -- so that the entropy front ends (host/vp8_parse.c, csrc/vp8g_m05.hip) can be fed
 * streams no encoder in the corpus produces (tests/streams.py).
 *
 * Written from RFC 6386: 9.1 frame tag and size fields, 9.2 colour space / clamping, 9.3 segmentation,
 * 9.5 token partitions, 9.6 loop filter and quantiser, 9.10-9.11 entropy refresh and skip, 11.2-11.5
 * (19.3) per-macroblock header with the key-frame mode trees and sub-block contexts, 13.2-13.4 token
 * tree, categories, contexts and probability updates.  Tables: host/vp8_tables.inc.  Boolean
 * encoder: vp8_boolenc.h (7.3).
 *
 * What the frame's arrays do not determine comes from Vp8StreamParams.  What a decoder cannot
 * return is ignored on input: position 0 of the Y blocks and bmode[] of a non-B_PRED macroblock,
 * segment_id when no map is sent, has_coeff, skip_coeff (the skip policy decides; what was written
 * is returned in skip_written).  tests/streams.py canonical() restates these rules on the frame.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../webp-decoder_amd/host/vp8_front.h"
#include "vp8_boolenc.h"

#include "../webp-decoder_amd/host/vp8_tables.inc"

enum { SKIP_EMPTY = 0, SKIP_NONE = 1, SKIP_HALF = 2 };
enum { T_EOB = 0, T_ZERO, T_ONE, T_TWO, T_THREE, T_FOUR, T_CAT1, T_CAT2, T_CAT3, T_CAT4, T_CAT5, T_CAT6, T_KINDS };

/* 1112 bytes; mirrored by tests/streams.py StreamParams */
typedef struct {
	uint8_t color_space, clamp_type;        /* RFC 9.2 bits */
	uint8_t x_scale, y_scale;               /* RFC 9.1: the two upper bits of each size field */
	uint8_t update_mb_segmentation_map;     /* with segmentation on: send a map */
	uint8_t seg_tree_probs[3];              /* 255 = not sent */
	uint8_t update_segment_feature_data;    /* with segmentation on: send mode + 4 + 4 values */
	uint8_t lf_delta_update;                /* with lf_delta_enabled: send the 4 + 4 deltas */
	uint8_t log2_nparts;                    /* 0..3 */
	uint8_t refresh_entropy_probs;
	uint8_t use_skip, skip_prob;            /* mb_no_coeff_skip and its probability */
	uint8_t skip_policy;                    /* SKIP_*: which empty macroblocks are coded as skipped */
	uint8_t reserved;
	uint64_t skip_seed;                     /* SKIP_HALF: xorshift64 state (0 -> 0x5EED) */
	uint32_t cut[8];                        /* per token partition: trailing bytes left out of the stream
	                                           and of its declared size (>= its length: empty) */
	uint8_t coeff_probs[4][8][3][11];       /* sent exactly where it differs from the default */
} Vp8StreamParams;

/* 416 bytes; mirrored by tests/streams.py StreamCensus */
typedef struct {
	uint64_t tokens[T_KINDS];               /* tokens written per kind */
	uint64_t ymode[5], uv_mode[4], bmode[10], segment[4]; /* leaves taken per tree */
	uint64_t skip_bits[2];                  /* skip bools written per value */
	uint32_t max_magnitude;
	uint32_t nparts;
	uint32_t part0_size;                    /* first_partition_len */
	uint32_t part_off[8], part_end[8];      /* token partitions, payload offsets (as declared) */
	uint32_t part_off_mod4[8];
	uint32_t prob_updates;                  /* coefficient probabilities sent */
	uint32_t payload_size;
} Vp8StreamCensus;

static const uint8_t k_band[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};
static const uint8_t k_scan[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
static const uint8_t k_cat_probs[6][12] = {
    {159, 0}, {165, 145, 0}, {173, 148, 140, 0}, {176, 155, 140, 135, 0}, {180, 157, 141, 134, 130, 0},
    {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0},
};
static const int k_cat_base[7] = {5, 7, 11, 19, 35, 67, 2115};
static const int8_t k_kf_ymode_tree[8] = {-4, 2, 4, 6, -0, -1, -2, -3};
static const uint8_t k_kf_ymode_prob[4] = {145, 156, 163, 128};
static const int8_t k_uv_mode_tree[6] = {-0, 2, -1, 4, -2, -3};
static const uint8_t k_kf_uv_mode_prob[3] = {142, 114, 183};
static const int8_t k_bmode_tree[18] = {-0, 2, -1, 4, -2, 6, 8, 12, -3, 10, -5, -6, -4, 14, -7, 16, -8, -9};
static const int8_t k_segment_tree[6] = {2, 4, -0, -1, -2, -3};

static void enc_literal(BoolEnc* e, uint32_t v, int n) {
	while (n-- > 0) enc_bool(e, 128, (int)((v >> n) & 1u));
}

/* optional signed field: flag, magnitude, sign (RFC 9.3, 9.6) */
static void enc_opt_signed(BoolEnc* e, int v, int n) {
	enc_bool(e, 128, v != 0);
	if (!v) return;
	enc_literal(e, (uint32_t)(v < 0 ? -v : v), n);
	enc_bool(e, 128, v < 0);
}

/* trees as in host/vp8_bool.h: pairs of branches, entries <= 0 are leaves (-symbol) */
static int tree_has(const int8_t* tree, int node, int sym) {
	for (int bit = 0; bit < 2; bit++) {
		const int next = tree[node + bit];
		if (next <= 0 ? -next == sym : tree_has(tree, next, sym)) return 1;
	}
	return 0;
}

/* the tree walk proper: at each node take the branch whose subtree holds the symbol */
static void put_tree(BoolEnc* e, const int8_t* tree, const uint8_t* probs, int sym) {
	int node = 0;
	for (;;) {
		const int l = tree[node];
		const int left = l <= 0 ? -l == sym : tree_has(tree, l, sym);
		const int bit = left ? 0 : 1;
		enc_bool(e, probs[node >> 1], bit);
		const int next = tree[node + bit];
		if (next <= 0) return;
		node = next;
	}
}

typedef struct {
	const uint8_t (*probs)[8][3][11];
	Vp8StreamCensus* cs;
	uint32_t (*branch)[8][3][11][2]; /* may be NULL: per token-tree node, bools written per value */
} TokCtx;

/* One 4x4 block (natural order in, RFC 13 tokens out).  Returns 1 if a coded value is non-zero. */
static int put_block(TokCtx* t, BoolEnc* e, int type, int first, int ctx, const int16_t* blk) {
	const uint8_t(*P)[3][11] = t->probs[type];
	int last = -1;
	for (int i = first; i < 16; i++)
		if (blk[k_scan[i]]) last = i;
	int pos = first, skip_eob = 0;
	int band = k_band[pos];
#define NODE(n, bit)                                                \
	do {                                                            \
		const int bit_ = (bit) != 0;                                \
		enc_bool(e, P[band][ctx][n], bit_);                         \
		if (t->branch) t->branch[type][band][ctx][n][bit_]++;       \
	} while (0)
	while (pos < 16) {
		if (pos > last) { /* (after a ZERO pos <= last always holds: zeros are written only before a value) */
			NODE(0, 0);
			t->cs->tokens[T_EOB]++;
			break;
		}
		if (!skip_eob) NODE(0, 1);
		const int v = blk[k_scan[pos]];
		if (!v) {
			NODE(1, 0);
			t->cs->tokens[T_ZERO]++;
			pos++;
			band = k_band[pos], ctx = 0;
			skip_eob = 1;
			continue;
		}
		NODE(1, 1);
		const int mag = v < 0 ? -v : v;
		if ((uint32_t)mag > t->cs->max_magnitude) t->cs->max_magnitude = (uint32_t)mag;
		if (mag == 1) {
			NODE(2, 0);
			t->cs->tokens[T_ONE]++;
		} else {
			NODE(2, 1);
			if (mag <= 4) {
				NODE(3, 0);
				NODE(4, mag != 2);
				if (mag != 2) NODE(5, mag == 4);
				t->cs->tokens[T_TWO + mag - 2]++;
			} else {
				int cat = 0;
				while (mag >= k_cat_base[cat + 1]) cat++;
				NODE(3, 1);
				NODE(6, cat >= 2);
				if (cat < 2) {
					NODE(7, cat & 1);
				} else {
					NODE(8, cat >= 4);
					if (cat < 4) NODE(9, cat & 1);
					else NODE(10, cat & 1);
				}
				t->cs->tokens[T_CAT1 + cat]++;
				int n = 0;
				while (k_cat_probs[cat][n]) n++;
				const int extra = mag - k_cat_base[cat];
				for (int i = 0; i < n; i++) enc_bool(e, k_cat_probs[cat][i], (extra >> (n - 1 - i)) & 1);
			}
		}
		enc_bool(e, 128, v < 0);
		if (++pos == 16) break;
		band = k_band[pos], ctx = mag == 1 ? 1 : 2;
		skip_eob = 0;
	}
#undef NODE
	return last >= 0;
}

static int mb_empty(const Vp8DecodedFrame* f, uint32_t mb) {
	const int bp = f->ymode[mb] == 4;
	if (!bp)
		for (int i = 0; i < 16; i++)
			if (f->coeff_y2[(size_t)mb * 16 + i]) return 0;
	for (int b = 0; b < 16; b++)
		for (int i = bp ? 0 : 1; i < 16; i++)
			if (f->coeff_y[((size_t)mb * 16 + b) * 16 + i]) return 0;
	for (int i = 0; i < 64; i++)
		if (f->coeff_u[(size_t)mb * 64 + i] || f->coeff_v[(size_t)mb * 64 + i]) return 0;
	return 1;
}

static int representable(const Vp8DecodedFrame* f) {
	const size_t n = f->mb_total;
	for (size_t m = 0; m < n; m++) {
		if (f->ymode[m] > 4 || f->uv_mode[m] > 3) return 0;
		if (f->ymode[m] == 4)
			for (int i = 0; i < 16; i++)
				if (f->bmode[m * 16 + i] > 9) return 0;
	}
	const int16_t* arr[4] = {f->coeff_y2, f->coeff_y, f->coeff_u, f->coeff_v};
	const size_t per[4] = {16, 256, 64, 64};
	for (int a = 0; a < 4; a++)
		for (size_t i = 0; i < n * per[a]; i++) {
			/* (the ignored Y DC slots of Y2 macroblocks are not coded and may hold anything) */
			if (a == 1 && (i & 15) == 0 && f->ymode[i / 256] != 4) continue;
			if (arr[a][i] > 2114 || arr[a][i] < -2114) return 0;
		}
	return 1;
}

/* Writes the .webp of (kf, f, prm) into out (cap bytes).  Returns its size, or -1 + errno: EINVAL for
 * a frame the format cannot represent (|coefficient| > 2114, a mode out of range, a field beyond its
 * bit width, a partition 0 of 2^19 bytes or more, bad parameters), ENOSPC for a small buffer, ENOMEM.
 * census (may be NULL) and skip_written ([mb_total], may be NULL) report what was written;
 * branch_counts (uint32 [4][8][3][11][2], may be NULL) counts the token-tree bools per node and value
 * (what a probability table fitted to this frame is computed from). */
long vp8_stream_write(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* f, const Vp8StreamParams* prm, uint8_t* out,
                      size_t cap, Vp8StreamCensus* census, uint8_t* skip_written, uint32_t* branch_counts) {
	Vp8StreamCensus local;
	Vp8StreamCensus* cs = census ? census : &local;
	memset(cs, 0, sizeof(*cs));
	if (!kf || !f || !prm || !out || prm->log2_nparts > 3 || prm->x_scale > 3 || prm->y_scale > 3 || kf->width == 0 ||
	    kf->width > 16383 || kf->height == 0 || kf->height > 16383 || prm->skip_policy > SKIP_HALF) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t cols = (kf->width + 15u) >> 4, rows = (kf->height + 15u) >> 4, total = cols * rows;
	int ok = f->mb_cols == cols && f->mb_rows == rows && f->mb_total == total && f->segment_id && f->ymode && f->uv_mode &&
	         f->bmode && f->coeff_y2 && f->coeff_y && f->coeff_u && f->coeff_v && f->q_index <= 127 && f->lf_level <= 63 &&
	         f->lf_sharpness <= 7;
	const int8_t dq[5] = {f->y1_dc_delta_q, f->y2_dc_delta_q, f->y2_ac_delta_q, f->uv_dc_delta_q, f->uv_ac_delta_q};
	for (int i = 0; i < 5; i++) ok = ok && dq[i] >= -15 && dq[i] <= 15;
	for (int i = 0; i < 4; i++)
		ok = ok && f->seg_quant_idx[i] >= -127 && f->seg_lf_level[i] >= -63 && f->seg_lf_level[i] <= 63 &&
		     f->lf_ref_delta[i] >= -63 && f->lf_ref_delta[i] <= 63 && f->lf_mode_delta[i] >= -63 && f->lf_mode_delta[i] <= 63;
	if (!ok || !representable(f)) {
		errno = EINVAL;
		return -1;
	}
	const int seg = f->segmentation_enabled != 0;
	const int map = seg && prm->update_mb_segmentation_map;
	if (map)
		for (uint32_t m = 0; m < total; m++)
			if (f->segment_id[m] > 3) {
				errno = EINVAL;
				return -1;
			}

	const uint32_t k = 1u << prm->log2_nparts;
	BoolEnc p0, parts[8];
	enc_init(&p0);
	for (uint32_t p = 0; p < k; p++) enc_init(&parts[p]);

	/* ---- frame header (RFC 9.2-9.11, 13.4) ---- */
	enc_bool(&p0, 128, prm->color_space != 0);
	enc_bool(&p0, 128, prm->clamp_type != 0);
	enc_bool(&p0, 128, seg);
	if (seg) {
		enc_bool(&p0, 128, map);
		enc_bool(&p0, 128, prm->update_segment_feature_data != 0);
		if (prm->update_segment_feature_data) {
			enc_bool(&p0, 128, f->segmentation_abs != 0);
			for (int i = 0; i < 4; i++) enc_opt_signed(&p0, f->seg_quant_idx[i], 7);
			for (int i = 0; i < 4; i++) enc_opt_signed(&p0, f->seg_lf_level[i], 6);
		}
		if (map)
			for (int i = 0; i < 3; i++) {
				enc_bool(&p0, 128, prm->seg_tree_probs[i] != 255);
				if (prm->seg_tree_probs[i] != 255) enc_literal(&p0, prm->seg_tree_probs[i], 8);
			}
	}
	enc_bool(&p0, 128, f->lf_use_simple != 0);
	enc_literal(&p0, f->lf_level, 6);
	enc_literal(&p0, f->lf_sharpness, 3);
	enc_bool(&p0, 128, f->lf_delta_enabled != 0);
	if (f->lf_delta_enabled) {
		enc_bool(&p0, 128, prm->lf_delta_update != 0);
		if (prm->lf_delta_update) {
			for (int i = 0; i < 4; i++) enc_opt_signed(&p0, f->lf_ref_delta[i], 6);
			for (int i = 0; i < 4; i++) enc_opt_signed(&p0, f->lf_mode_delta[i], 6);
		}
	}
	enc_literal(&p0, prm->log2_nparts, 2);
	enc_literal(&p0, f->q_index, 7);
	for (int i = 0; i < 5; i++) enc_opt_signed(&p0, dq[i], 4);
	enc_bool(&p0, 128, prm->refresh_entropy_probs != 0);
	for (int i = 0; i < 4; i++)
		for (int j = 0; j < 8; j++)
			for (int c = 0; c < 3; c++)
				for (int l = 0; l < 11; l++) {
					const int upd = prm->coeff_probs[i][j][c][l] != vp8_default_coeff_probs[i][j][c][l];
					enc_bool(&p0, vp8_coeff_update_probs[i][j][c][l], upd);
					if (upd) enc_literal(&p0, prm->coeff_probs[i][j][c][l], 8);
					cs->prob_updates += (uint32_t)upd;
				}
	enc_bool(&p0, 128, prm->use_skip != 0);
	if (prm->use_skip) enc_literal(&p0, prm->skip_prob, 8);

	/* ---- per-macroblock headers (partition 0) and tokens (partition row % k) ---- */
	uint8_t* above_b = (uint8_t*)calloc((size_t)cols, 4);  /* above sub-block modes, B_DC = 0 */
	uint8_t* above = (uint8_t*)calloc((size_t)cols, 9);    /* per MB column: Y[4] U[2] V[2] Y2 */
	long result = -1;
	if (!above_b || !above) {
		errno = ENOMEM;
		goto done;
	}
	TokCtx tc = {prm->coeff_probs, cs, (uint32_t(*)[8][3][11][2])branch_counts};
	if (branch_counts) memset(branch_counts, 0, sizeof(uint32_t) * 4 * 8 * 3 * 11 * 2);
	uint64_t rng = prm->skip_seed ? prm->skip_seed : 0x5EED;
	const uint8_t seg_probs[3] = {prm->seg_tree_probs[0], prm->seg_tree_probs[1], prm->seg_tree_probs[2]};
	for (uint32_t r = 0; r < rows; r++) {
		BoolEnc* te = &parts[r % k];
		uint8_t left_b[4] = {0, 0, 0, 0};
		uint8_t left[9] = {0};
		for (uint32_t c = 0; c < cols; c++) {
			const uint32_t mb = r * cols + c;
			const int ym = f->ymode[mb];
			int skip = 0;
			if (map) {
				put_tree(&p0, k_segment_tree, seg_probs, f->segment_id[mb]);
				cs->segment[f->segment_id[mb]]++;
			}
			if (prm->use_skip) {
				if (mb_empty(f, mb)) {
					if (prm->skip_policy == SKIP_EMPTY) skip = 1;
					else if (prm->skip_policy == SKIP_HALF) {
						rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
						skip = (int)((rng >> 33) & 1u);
					}
				}
				enc_bool(&p0, prm->skip_prob, skip);
				cs->skip_bits[skip]++;
			}
			if (skip_written) skip_written[mb] = (uint8_t)skip;
			put_tree(&p0, k_kf_ymode_tree, k_kf_ymode_prob, ym);
			cs->ymode[ym]++;
			const uint8_t* bm = f->bmode + (size_t)mb * 16;
			uint8_t* ab = above_b + (size_t)c * 4;
			if (ym == 4) {
				for (int i = 0; i < 16; i++) {
					const int y = i >> 2, x = i & 3;
					const uint8_t a = y ? bm[i - 4] : ab[x];
					const uint8_t l = x ? bm[i - 1] : left_b[y];
					put_tree(&p0, k_bmode_tree, vp8_kf_bmode_prob[a][l], bm[i]);
					cs->bmode[bm[i]]++;
				}
				for (int i = 0; i < 4; i++) {
					ab[i] = bm[12 + i];
					left_b[i] = bm[4 * i + 3];
				}
			} else {
				static const uint8_t implied[4] = {0, 2, 3, 1}; /* DC->B_DC, V->B_VE, H->B_HE, TM->B_TM */
				memset(ab, implied[ym], 4);
				memset(left_b, implied[ym], 4);
			}
			put_tree(&p0, k_uv_mode_tree, k_kf_uv_mode_prob, f->uv_mode[mb]);
			cs->uv_mode[f->uv_mode[mb]]++;

			/* tokens (RFC 13): Y2 (if any), 16 Y, 4 U, 4 V; a skipped macroblock writes none and
			 * clears its contexts (the Y2 context only if it has a Y2 block) */
			uint8_t* abv = above + (size_t)c * 9;
			if (ym != 4) {
				int nz = 0;
				if (!skip) nz = put_block(&tc, te, 1, 0, left[8] + abv[8], f->coeff_y2 + (size_t)mb * 16);
				left[8] = abv[8] = (uint8_t)nz;
			}
			for (int by = 0; by < 4; by++)
				for (int bx = 0; bx < 4; bx++) {
					int nz = 0;
					if (!skip)
						nz = put_block(&tc, te, ym != 4 ? 0 : 3, ym != 4 ? 1 : 0, left[by] + abv[bx],
						               f->coeff_y + ((size_t)mb * 16 + (size_t)(by * 4 + bx)) * 16);
					left[by] = abv[bx] = (uint8_t)nz;
				}
			for (int pl = 0; pl < 2; pl++) {
				const int16_t* base = pl == 0 ? f->coeff_u : f->coeff_v;
				uint8_t* lc = left + 4 + 2 * pl;
				uint8_t* ac = abv + 4 + 2 * pl;
				for (int by = 0; by < 2; by++)
					for (int bx = 0; bx < 2; bx++) {
						int nz = 0;
						if (!skip) nz = put_block(&tc, te, 2, 0, lc[by] + ac[bx], base + ((size_t)mb * 4 + (size_t)(by * 2 + bx)) * 16);
						lc[by] = ac[bx] = (uint8_t)nz;
					}
			}
		}
	}
	enc_finish(&p0);
	int oom = p0.oom;
	size_t plen[8];
	size_t payload = 10 + p0.n + 3 * (k - 1);
	for (uint32_t p = 0; p < k; p++) {
		enc_finish(&parts[p]);
		oom |= parts[p].oom;
		plen[p] = parts[p].n - (prm->cut[p] < parts[p].n ? prm->cut[p] : parts[p].n);
		payload += plen[p];
	}
	if (oom) {
		errno = ENOMEM;
	} else if (p0.n >= (1u << 19) || payload > 0x7FFFFFF0u) {
		errno = EINVAL;
	} else if (20 + payload + (payload & 1) > cap) {
		errno = ENOSPC;
	} else {
		uint8_t* o = out;
		memcpy(o, "RIFF", 4);
		put_le(o + 4, (uint32_t)(12 + payload + (payload & 1)), 4);
		memcpy(o + 8, "WEBPVP8 ", 8);
		put_le(o + 16, (uint32_t)payload, 4);
		uint8_t* v = o + 20;
		/* RFC 9.1: key frame (0), version, show_frame, first partition size */
		put_le(v, ((uint32_t)(kf->profile & 7u) << 1) | ((uint32_t)(kf->show_frame != 0) << 4) | (uint32_t)p0.n << 5, 3);
		v[3] = 0x9d, v[4] = 0x01, v[5] = 0x2a;
		put_le(v + 6, (uint32_t)kf->width | (uint32_t)prm->x_scale << 14, 2);
		put_le(v + 8, (uint32_t)kf->height | (uint32_t)prm->y_scale << 14, 2);
		memcpy(v + 10, p0.buf, p0.n);
		uint8_t* q = v + 10 + p0.n;
		for (uint32_t p = 0; p + 1 < k; p++, q += 3) put_le(q, (uint32_t)plen[p], 3);
		for (uint32_t p = 0; p < k; p++) {
			cs->part_off[p] = (uint32_t)(q - v);
			cs->part_off_mod4[p] = cs->part_off[p] & 3u;
			memcpy(q, parts[p].buf, plen[p]);
			q += plen[p];
			cs->part_end[p] = (uint32_t)(q - v);
		}
		if (payload & 1) *q = 0;
		cs->nparts = k;
		cs->part0_size = (uint32_t)p0.n;
		cs->payload_size = (uint32_t)payload;
		result = (long)(20 + payload + (payload & 1));
	}
done:
	free(above_b);
	free(above);
	free(p0.buf);
	for (uint32_t p = 0; p < k; p++) free(parts[p].buf);
	return result;
}

/* the default token probabilities (RFC 13.5), [4][8][3][11], and layout checks for the Python mirror */
const uint8_t* vp8_stream_default_probs(void) { return &vp8_default_coeff_probs[0][0][0][0]; }
/* RFC 14.1 quantiser tables, [128] each (for the tests' restatement of the dequantisation factors) */
const int16_t* vp8_stream_dc_q(void) { return vp8_dc_qlookup; }
const int16_t* vp8_stream_ac_q(void) { return vp8_ac_qlookup; }
size_t vp8_stream_params_size(void) { return sizeof(Vp8StreamParams); }
size_t vp8_stream_census_size(void) { return sizeof(Vp8StreamCensus); }
