// vp8g_lossless.hip -- the inverse transforms of lossless (VP8L) images on the device
// (include/vp8g.h: vp8g_lossless_batch_device).  The sequential restatement, and the
// authority, is vp8f_lossless_apply (host/vp8_alpha.c).
//
// One 16-wave workgroup per image (images taken by a grid-stride loop).  The workgroup walks the
// image's transform list last to first; the image's own width x height dwords of the output buffer are
// the working buffer from the first pass on, and a workgroup barrier separates the passes.
//   cross colour, add green   pointwise, in place;
//   colour indexing           a gather that widens the rows; in place it runs from the last pixel back,
//                             1024 pixels a step, every step reading before a barrier and writing after it
//                             (an output pixel's index is never below the index of the packed pixel it reads);
//   predictor                 (x, y) needs L, T, TL and TR, so the only parallelism is a wavefront in which
//                             row y trails row y - 1 by TWO columns.  A wave takes a band of 64 rows, one row
//                             per lane: at step t lane l is at column t - 2 l, L is its own previous result, TR
//                             is lane l - 1's previous result (a DPP wave shift), T and TL are what TR was one and
//                             two steps earlier.  At the rightmost column TR is the row's own first pixel, kept
//                             in a register.  Band b trails band b - 1 by kDelay groups of kG steps and takes that
//                             band's bottom row from a ring in LDS; bands beyond the 16th wait for the next round
//                             of the same workgroup, and wave 15 hands its bottom row to wave 0 of the next round
//                             through a full-width row in LDS.  One workgroup barrier per group of kG steps paces
//                             the waves: no wave waits on another workgroup and nothing spins on memory.
//                             A lane fetches its mode once per block, and its residuals four pixels at a time
//                             (one 16-byte load a group ahead of their use; one 16-byte store).
// A cross-colour pass right before a predictor pass is applied on the predictor's load, an add-green pass
// right after it on its store.  For the stream order subtract green, predictor, cross colour -- the inverse
// runs last to first: cross colour -> predictor -> add green -- both apply and the image is read once and
// written once; libwebp 1.2.2 writes the two halves of it (predictor, cross colour / subtract green,
// predictor), each one pass as well.  The stream order predictor, cross colour, subtract green inverts as
// add green, then cross colour + predictor: two passes.
// Every global access is an index below the image's own sizes: x < width, y < height of the pass,
// block indices below the sub-image's div_up sizes, colour indices below ncolors.
#include <errno.h>
#include <string.h>

#include "vp8g_device.h"
#define VP8G_SKEW_HOST_ONLY  // (no wait sites here: the band hooks alone)
#define VP8G_SKEW_BANDS
#include "vp8g_skew.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))
#define DEV __device__ __forceinline__

namespace {

constexpr uint32_t kWaves = 16, kThreads = kWaves * 64, kMaxDim = 16383;
constexpr int kSkew = 2;                 // columns a row trails the row above
constexpr int kLag = 63 * kSkew;         // columns lane 63 trails lane 0
constexpr int kG = 64;                   // steps (columns of lane 0) per group: the tile step
constexpr int kDelay = 3;                // groups a band trails the band above
constexpr int kRing = 256;               // bottom-row ring of a wave, in pixels, indexed by the column
constexpr int kRingDwords = (int)kWaves * kRing;
constexpr int kFullCap = 16384 + 64;      // the full-width row at most, in pixels (what the launch may ask for)
// a reader's group reads columns up to kG (k + 1) of the row above; the writer's group k + kDelay - 1 has
// written up to kG (k + kDelay) - 1 - kLag; and the writer's group k + kDelay must not reuse their slots
static_assert(kDelay * kG >= kG + kLag + 1 && kRing >= kDelay * kG + kG - kLag && (kRing & (kRing - 1)) == 0 && kG % 4 == 0,
              "hand-over geometry");

typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

DEV uint32_t ldu(const uint8_t* p, size_t i) { return *(const u32u*)(p + 4 * i); }
DEV int div_up(int v, int bits) { return (v + (1 << bits) - 1) >> bits; }

DEV uint32_t add_px(uint32_t a, uint32_t b) {
	return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
DEV uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
DEV int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
DEV int ch(uint32_t p, int s) { return (int)((p >> s) & 0xFFu); }

DEV uint32_t pred_select(uint32_t L, uint32_t T, uint32_t TL) {
	// (sums of absolute byte differences: distances of L + T - TL to L and to T)
	const uint32_t pl = __builtin_amdgcn_sad_u8(T, TL, 0u), pt = __builtin_amdgcn_sad_u8(L, TL, 0u);
	return pl < pt ? L : T;
}
DEV uint32_t pred_clamp_full(uint32_t a, uint32_t b, uint32_t c) {
	uint32_t r = 0;
#pragma unroll
	for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255(ch(a, s) + ch(b, s) - ch(c, s)) << s;
	return r;
}
DEV uint32_t pred_clamp_half(uint32_t a, uint32_t b) {
	uint32_t r = 0;
#pragma unroll
	for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255(ch(a, s) + (ch(a, s) - ch(b, s)) / 2) << s;
	return r;
}

DEV uint32_t predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
	switch (mode) {
		case 1: return L;
		case 2: return T;
		case 3: return TR;
		case 4: return TL;
		case 5: return avg2(avg2(L, TR), T);
		case 6: return avg2(L, TL);
		case 7: return avg2(L, T);
		case 8: return avg2(TL, T);
		case 9: return avg2(T, TR);
		case 10: return avg2(avg2(L, TL), avg2(T, TR));
		case 11: return pred_select(L, T, TL);
		case 12: return pred_clamp_full(L, T, TL);
		case 13: return pred_clamp_half(avg2(L, T), TL);
		default: return 0xFF000000u;  // 0, and 14 / 15
	}
}

DEV int cc_delta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }
DEV uint32_t cross_color(uint32_t e, uint32_t v) {
	const uint32_t g2r = e & 255u, g2b = (e >> 8) & 255u, r2b = (e >> 16) & 255u, g = (v >> 8) & 255u;
	uint32_t r = (v >> 16) & 255u, b = v & 255u;
	r = (r + (uint32_t)cc_delta(g2r, g)) & 255u;
	b = (b + (uint32_t)cc_delta(g2b, g)) & 255u;
	b = (b + (uint32_t)cc_delta(r2b, r)) & 255u;
	return (v & 0xFF00FF00u) | r << 16 | b;
}
DEV uint32_t add_green(uint32_t v) {
	const uint32_t g = (v >> 8) & 255u;
	return (v & 0xFF00FF00u) | (((v & 0x00FF00FFu) + (g << 16 | g)) & 0x00FF00FFu);
}

// lane l <- lane l - 1 (lane 0 keeps its own value; it does not use the result)
DEV uint32_t from_lane_above(uint32_t v) {
	return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// pixels x .. x + 3 of a row of w pixels at `row` (any byte alignment); those outside it read as 0
DEV void load_px4(const uint8_t* row, int x, int w, bool rowok, uint32_t (&r)[4]) {
	if (rowok && x >= 0 && x + 4 <= w) {
		const u32x4u v = *(const u32x4u*)(row + 4 * (size_t)x);
		r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
		return;
	}
#pragma unroll
	for (int q = 0; q < 4; q++) r[q] = rowok && x + q >= 0 && x + q < w ? ldu(row, (size_t)(x + q)) : 0u;
}

DEV void store_px4(uint32_t* row, int x, int w, bool rowok, const uint32_t (&o)[4]) {
	if (rowok && x >= 0 && x + 4 <= w) {
		*(u32x4a*)(row + x) = u32x4a{o[0], o[1], o[2], o[3]};
		return;
	}
#pragma unroll
	for (int q = 0; q < 4; q++)
		if (rowok && x + q >= 0 && x + q < w) row[x + q] = o[q];
}

// The predictor pass over the w x h image at `in` (which may be the output itself) into out.  cc: a
// cross-colour transform applied to the residuals as they are loaded, or nullptr; green: add green to
// what is stored (the prediction runs on the pixels before it).
__device__ void predictor_pass(const uint8_t* in, uint32_t* out, int w, int h, const Vp8gLosslessTransform& pt,
                               const Vp8gLosslessTransform* cc, bool green, const uint8_t* src, uint32_t* smem, int lane, int wave) {
	const int nbands = (h + 63) >> 6, ngroups = (w + kLag + kG - 1) / kG;
	// (the skew build's mutants, csrc/vp8g_skew.h: in the shipped library mut is the constant 0)
	const uint32_t mut = VP8G_BAND_MUTANT();
	const int delay = kDelay - (mut == kBandMutDelay ? 1 : 0);
	const uint32_t ringmask = (uint32_t)(mut == kBandMutRing ? kRing / 2 : kRing) - 1u;
	// a round: every wave one band.  Wave j starts kDelay groups after wave j - 1; the next round starts
	// when wave 0 trails wave 15 by kDelay groups at least (16 kDelay) and no earlier than kDelay groups
	// after a band's last group, so that a wave's ring is not rewritten while the wave below reads it
	const int round_len =
	    (ngroups + delay > (int)kWaves * delay && mut != kBandMutNoLong ? ngroups + delay : (int)kWaves * delay) - (mut == kBandMutRound ? 1 : 0);
	const int rounds = (nbands + (int)kWaves - 1) / (int)kWaves;
	const int steps = (rounds - 1) * round_len + ((int)kWaves - 1) * delay + ngroups;
	uint32_t* const full = smem + kRingDwords;
	// bottom rows, indexed by the column (the full-width row holds every column: its mask changes nothing)
	uint32_t* const hw = wave == (int)kWaves - 1 ? full : smem + wave * kRing;
	const uint32_t* const hr = wave == 0 ? full : smem + (wave - 1) * kRing;
	const uint32_t wmask = wave == (int)kWaves - 1 ? 0x7FFFu : ringmask;
	const uint32_t rmask = wave == 0 ? 0x7FFFu : ringmask;
	const uint8_t* const modes = src + pt.data;
	const int pbits = (int)pt.bits, pbw = div_up(w, pbits), pmask = (1 << pbits) - 1;
	const uint8_t* const ccdata = cc ? src + cc->data : src;
	const int cbits = cc ? (int)cc->bits : 2, cbw = div_up(w, cbits), cmask = (1 << cbits) - 1;
	uint32_t cur = 0, T = 0, TL = 0, first = 0, mode = 0, cce = 0;
	for (int st = 0; st < steps; st++) {
		const int rel = st - delay * wave;
		const int p = rel >= 0 ? rel / round_len : rounds;
		const int k = rel - p * round_len;
		const int b = p * (int)kWaves + wave;
		const bool on = p < rounds && b < nbands && k < ngroups;  // (wave-uniform)
		if (on) {
			const int y = b * 64 + lane;
			const bool rowok = y < h;
			const uint8_t* const inrow = in + 4 * (size_t)(rowok ? y : 0) * (size_t)w;
			uint32_t* const outrow = out + (size_t)(rowok ? y : 0) * (size_t)w;
			if (k == 0) {
				cur = 0, TL = 0;
				T = b ? hr[0] : 0u;  // (lane 0: the pixel above column 0; the other lanes shift theirs in)
			}
			uint32_t nxt[4];
			load_px4(inrow, k * kG - kSkew * lane, w, rowok, nxt);
			for (int c = 0; c < kG / 4; c++) {
				const int x0 = k * kG + 4 * c - kSkew * lane;
				uint32_t r[4], o[4], top[4];
#pragma unroll
				for (int q = 0; q < 4; q++) r[q] = nxt[q], o[q] = 0;
				if (c + 1 < kG / 4) load_px4(inrow, x0 + 4, w, rowok, nxt);
				// lane 0 alone: the row above at columns x + 1 (band 0 has none: row 0 predicts from L)
#pragma unroll
				for (int q = 0; q < 4; q++) top[q] = 0;
				if (lane == 0 && b) {
#pragma unroll
					for (int q = 0; q < 4; q++) {
						const int xi = x0 + q + 1;  // (x0 >= 0 in lane 0; at xi >= w nothing is read: TR is then the row's first pixel)
						if (xi < w) top[q] = hr[(uint32_t)xi & rmask];
					}
				}
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const int x = x0 + q;
					const uint32_t up = from_lane_above(cur);
					uint32_t TR = lane == 0 ? top[q] : up;
					if (rowok && x >= 0 && x < w) {
						if ((x & pmask) == 0) mode = (ldu(modes, (size_t)(y >> pbits) * (size_t)pbw + (size_t)(x >> pbits)) >> 8) & 15u;
						uint32_t res = r[q];
						if (cc) {
							if ((x & cmask) == 0) cce = ldu(ccdata, (size_t)(y >> cbits) * (size_t)cbw + (size_t)(x >> cbits));
							res = cross_color(cce, res);
						}
						if (x == w - 1) TR = first;
						const uint32_t m = y == 0 ? (x == 0 ? 0u : 1u) : x == 0 ? 2u : mode;
						const uint32_t v = add_px(res, predict(m, cur, T, TL, TR));
						if (x == 0) first = v;
						cur = v;
						o[q] = green ? add_green(v) : v;
						if (lane == 63) hw[(uint32_t)x & wmask] = v;
					}
					TL = T, T = TR;
				}
				store_px4(outrow, x0, w, rowok, o);
			}
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(kThreads) void lossless_kernel(const Vp8gLosslessDesc* __restrict__ D, uint32_t n, const uint8_t* src,
                                                            uint8_t* dst) {
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	const int tid = (int)threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	for (uint32_t im = blockIdx.x; im < n; im += gridDim.x) {
		const Vp8gLosslessDesc& d = D[im];
		const int h = (int)d.height, ntr = (int)d.ntransforms;
		VP8G_BAND_POISON(smem, (uint32_t)kRingDwords + ((d.width + 64u) & ~63u));  // (no more than the launch's widest image asked for)
		uint32_t* const out = (uint32_t*)(dst + d.dst);
		const uint8_t* in = src + d.src;
		int cw = (int)d.width;  // the width of the image at `in`
		for (int i = 0; i < ntr; i++)
			if (d.tr[i].type == VP8G_L_COLOR_INDEX) cw = div_up(cw, (int)d.tr[i].bits);
		if (ntr == 0)
			for (int i = tid; i < cw * h; i += (int)kThreads) out[i] = ldu(in, (size_t)i);
		for (int i = ntr - 1; i >= 0; i--) {
			const Vp8gLosslessTransform* cc = nullptr;
			if (d.tr[i].type == VP8G_L_CROSS_COLOR && i > 0 && d.tr[i - 1].type == VP8G_L_PREDICTOR) cc = &d.tr[i--];
			const Vp8gLosslessTransform& t = d.tr[i];
			if (t.type == VP8G_L_PREDICTOR) {
				const bool green = i > 0 && d.tr[i - 1].type == VP8G_L_SUBTRACT_GREEN;
				predictor_pass(in, out, cw, h, t, cc, green, src, smem, lane, wave);
				if (green) i--;
			} else if (t.type == VP8G_L_CROSS_COLOR) {
				const uint8_t* const data = src + t.data;
				const int bits = (int)t.bits, bw = div_up(cw, bits);
				for (int j = tid; j < cw * h; j += (int)kThreads) {
					const int y = j / cw, x = j - y * cw;
					out[j] = cross_color(ldu(data, (size_t)(y >> bits) * (size_t)bw + (size_t)(x >> bits)), ldu(in, (size_t)j));
				}
			} else if (t.type == VP8G_L_SUBTRACT_GREEN) {
				for (int j = tid; j < cw * h; j += (int)kThreads) out[j] = add_green(ldu(in, (size_t)j));
			} else {
				const uint8_t* const table = src + t.data;
				const int w = (int)t.xsize, bits = (int)t.bits, pw = cw;
				const uint32_t bpp = 8u >> bits, mask = (1u << bpp) - 1u, per = (1u << bits) - 1u;
				const int total = w * h;
				for (int c0 = (total - 1) / (int)kThreads * (int)kThreads; c0 >= 0; c0 -= (int)kThreads) {
					const int j = c0 + tid;
					uint32_t v = 0;
					if (j < total) {
						const int y = j / w, x = j - y * w;
						const uint32_t packed = (ldu(in, (size_t)y * (size_t)pw + (size_t)(x >> bits)) >> 8) & 255u;
						const uint32_t idx = (packed >> (((uint32_t)x & per) * bpp)) & mask;
						v = idx < t.ncolors ? ldu(table, idx) : 0u;
					}
					__syncthreads();
					if (j < total) out[j] = v;
				}
				cw = w;
			}
			in = (const uint8_t*)out;
			__syncthreads();
		}
		__syncthreads();
	}
}

uint32_t ci_bits(uint32_t ncolors) { return ncolors > 16 ? 0u : ncolors > 4 ? 1u : ncolors > 2 ? 2u : 3u; }

bool desc_ok(const Vp8gLosslessDesc& d) {
	if (d.width < 1 || d.height < 1 || d.width > kMaxDim || d.height > kMaxDim || d.ntransforms > 4 || d.dst % 4u) return false;
	uint32_t xs = d.width, seen = 0;
	for (uint32_t i = 0; i < d.ntransforms; i++) {
		const Vp8gLosslessTransform& t = d.tr[i];
		if (t.type > VP8G_L_COLOR_INDEX || (seen & (1u << t.type)) || t.xsize != xs) return false;
		seen |= 1u << t.type;
		if (t.type == VP8G_L_PREDICTOR || t.type == VP8G_L_CROSS_COLOR) {
			if (t.bits < 2 || t.bits > 9) return false;
		} else if (t.type == VP8G_L_COLOR_INDEX) {
			if (t.ncolors < 1 || t.ncolors > 256 || t.bits != ci_bits(t.ncolors)) return false;
			xs = (xs + (1u << t.bits) - 1u) >> t.bits;
		}
	}
	return true;
}

}  // namespace

// (tests/test_gpu_lossless.py takes its boundary sizes from here, through vp8g.lossless_geometry())
VP8G_API void vp8g_lossless_geometry(uint32_t out[3]) { out[0] = (uint32_t)kG, out[1] = 64u, out[2] = kWaves; }

// (tests/bands.py states the hand-over geometry once more; tests/test_gpu_bands.py holds the two together)
VP8G_API void vp8g_lossless_handover(uint32_t out[4]) { out[0] = (uint32_t)kSkew, out[1] = (uint32_t)kDelay, out[2] = (uint32_t)kRing, out[3] = (uint32_t)kFullCap; }
VP8G_BAND_EXPORTS(lossless)

VP8G_API int vp8g_make_lossless_desc(uint32_t width, uint32_t height, uint64_t src, uint64_t dst, uint32_t ntransforms,
                                     const Vp8gLosslessTransform* tr, uint32_t task0, Vp8gLosslessDesc* out) {
	if (!out || ntransforms > 4 || (ntransforms && !tr)) {
		errno = EINVAL;
		return -1;
	}
	Vp8gLosslessDesc d;
	memset(&d, 0, sizeof(d));
	d.src = src, d.dst = dst, d.width = width, d.height = height, d.ntransforms = ntransforms, d.task0 = task0;
	for (uint32_t i = 0; i < ntransforms; i++) {
		d.tr[i].data = tr[i].data, d.tr[i].type = tr[i].type, d.tr[i].bits = tr[i].bits, d.tr[i].xsize = tr[i].xsize;
		d.tr[i].ncolors = tr[i].type == VP8G_L_COLOR_INDEX ? tr[i].ncolors : 0u;
	}
	if (!desc_ok(d)) {
		errno = EINVAL;
		return -1;
	}
	*out = d;
	return 0;
}

VP8G_API int vp8g_lossless_batch_device(const Vp8gLosslessDesc* h, const Vp8gLosslessDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                        uint8_t* d_dst, void* stream) {
	bool ok = h && d_descs && d_src && d_dst && n > 0 && n <= 0x7FFFFFFFu && (uintptr_t)d_dst % 4u == 0;
	uint32_t maxw = 0;
	for (uint32_t i = 0; ok && i < n; i++) {
		ok = desc_ok(h[i]) && h[i].task0 == i;
		if (ok && h[i].width > maxw) maxw = h[i].width;
	}
	if (!ok) return vp8g::fail(EINVAL);
	constexpr uint32_t kLdsMax = (uint32_t)(kRingDwords + kFullCap) * 4u;
	static const hipError_t attr =
	    hipFuncSetAttribute((const void*)lossless_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
	// the rings, and a full-width row as wide as the launch's widest image
	const uint32_t lds = (uint32_t)(kRingDwords + ((maxw + 64u) & ~63u)) * 4u;
	return vp8g::gated_launch(
	    (hipStream_t)stream, "lossless launch",
	    [&] {
		    hipLaunchKernelGGL(lossless_kernel, dim3(vp8g::grid_for(n, 1u)), dim3(kThreads), lds, (hipStream_t)stream, d_descs, n, d_src,
		                       d_dst);
		    return hipGetLastError();
	    },
	    attr);
}
