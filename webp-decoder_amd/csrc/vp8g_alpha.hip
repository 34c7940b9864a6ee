// vp8g_alpha.hip -- the un-prediction of ALPH residual planes on the device
// (include/vp8g.h: vp8g_alpha_unfilter_batch_device).
//
// One 16-wave workgroup per plane (planes taken by a grid-stride loop), one kernel for the four filters:
//   0  a copy;
//   1  column 0 is a scan down the plane (wave 0, into LDS), then every row is a scan (a wave per row,
//      256 bytes per step: four bytes per lane, a wave scan of the lane sums, a carry);
//   2  row 0 is a scan (wave 0, into LDS), then every column is a scan down the plane (four columns per
//      thread, the rows' loads coalesced across the lanes);
//   3  the gradient predictor clips, so it is not a scan: (x, y) needs (x-1, y), (x, y-1), (x-1, y-1), and the
//      only parallelism is the anti-diagonal.  A wave takes a band of 64 rows, one row per lane, lane l
//      running l columns behind lane l-1: at step t lane l is at column t - l, its left neighbour is its own
//      previous result, the pixel above is lane l-1's previous result (a DPP wave shift) and the one above
//      left is what that was a step earlier.  The residuals reach the lanes through LDS: per tile step
//      a wave loads 64 rows x 64 skewed columns (row l starts l columns earlier) with unaligned dword loads,
//      16 lanes to a row, reads them back one dword per lane per four steps (row pitch 17 dwords: the 64
//      rows of a column fall on distinct banks in each 32-lane half), leaves its results in the same
//      slots and stores the tile the way it was loaded.  Band b trails band b-1 by two tile steps and
//      takes that band's bottom row (lane 63's results) from a ring in LDS; bands beyond the 16th wait
//      for the next round of the same workgroup, and wave 15 hands its bottom row to wave 0 of the next
//      round through a full-width row in LDS.  The waves are paced by workgroup barriers only (three
//      per tile step): no wave waits on another workgroup and nothing spins on memory.
// Every global access is checked against the plane's own width x height bytes.
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
constexpr int kT = 64;                  // skewed columns per tile step
constexpr int kPitch32 = kT / 4 + 1;    // tile row pitch in dwords (odd)
constexpr int kDelay = 2;               // tile steps a band trails the band above: lane 63 is 63 columns behind lane 0
constexpr int kTileBytes = 64 * kPitch32 * 4;
constexpr int kRing = 256;              // bottom-row ring of a wave, indexed by its step t (four tiles)
constexpr int kFull = 16640;            // full-width row: wave 15 -> wave 0 of the next round (t < 16383 + 63 + 64 + 8);
                                        // also column 0 / row 0 of the scans
constexpr int kOffRing = (int)kWaves * kTileBytes;
constexpr int kOffFull = kOffRing + (int)kWaves * kRing;
constexpr int kLdsBytes = kOffFull + kFull;
static_assert(kDelay * kT >= kT + 63 && kRing >= (kDelay + 2) * kT && kFull >= 16383 + 63 + kT + 8, "hand-over geometry");

typedef uint32_t u32u __attribute__((aligned(1)));

// bytes x .. x + 3 of a row of w bytes (those outside it read as 0)
DEV uint32_t load4(const uint8_t* __restrict__ row, int x, int w) {
	if (x >= 0 && x + 4 <= w) return *(const u32u*)(row + x);
	uint32_t v = 0;
#pragma unroll
	for (int q = 0; q < 4; q++)
		if (x + q >= 0 && x + q < w) v |= (uint32_t)row[x + q] << (8 * q);
	return v;
}

DEV void store4(uint8_t* __restrict__ row, int x, int w, uint32_t v) {
	if (x >= 0 && x + 4 <= w) {
		*(u32u*)(row + x) = v;
		return;
	}
#pragma unroll
	for (int q = 0; q < 4; q++)
		if (x + q >= 0 && x + q < w) row[x + q] = (uint8_t)(v >> (8 * q));
}

DEV uint32_t wave_scan(uint32_t v, int lane) {  // inclusive sum over the lanes up to this one
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t)__shfl_up((int)v, d);
		if (lane >= d) v += o;
	}
	return v;
}

// lane l <- lane l - 1 (lane 0 keeps its own value; it does not use the result)
DEV uint32_t from_lane_above(uint32_t v) {
	return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// One chunk of a row scan: 256 bytes at x0 (four per lane), `first` replacing byte 0 of the row when x0 = 0
// (first < 0: keep it); returns the carry into the next chunk.
DEV uint32_t scan_chunk(const uint8_t* __restrict__ srow, uint8_t* __restrict__ drow, int x0, int w, int lane, uint32_t carry,
                        int first, uint32_t* __restrict__ keep32) {
	const int x = x0 + 4 * lane;
	uint32_t v = load4(srow, x, w);
	if (x == 0 && first >= 0) v = (v & ~255u) | (uint32_t)first;
	const uint32_t s0 = v & 255u, s1 = s0 + ((v >> 8) & 255u), s2 = s1 + ((v >> 16) & 255u), s3 = s2 + (v >> 24);
	const uint32_t inc = wave_scan(s3, lane);
	const uint32_t base = inc - s3 + carry;
	const uint32_t o = ((s0 + base) & 255u) | ((s1 + base) & 255u) << 8 | ((s2 + base) & 255u) << 16 | ((s3 + base) & 255u) << 24;
	store4(drow, x, w, o);
	if (keep32 && x < w) keep32[x >> 2] = o;
	return carry + (uint32_t)__shfl((int)inc, 63);
}

// full_off: where the full-width row sits in the launch's LDS (kOffFull; 0 in a launch without a gradient
// plane, which allocates that row alone and so fits several workgroups on a CU)
__global__ __launch_bounds__(kThreads) void alpha_kernel(const Vp8gAlphaDesc* __restrict__ D, uint32_t n, const uint8_t* __restrict__ src,
                                                         uint8_t* __restrict__ dst, uint32_t full_off) {
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int tid = (int)threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint8_t* const full8 = smem + full_off;
	uint32_t* const full32 = (uint32_t*)full8;
	for (uint32_t pl = blockIdx.x; pl < n; pl += gridDim.x) {
		const Vp8gAlphaDesc d = D[pl];
		VP8G_BAND_POISON((uint32_t*)smem, (full_off + (uint32_t)kFull) / 4u);  // (the launch's whole dynamic LDS, either way)
		const int w = (int)d.width, h = (int)d.height;
		const uint8_t* __restrict__ s = src + d.src;
		uint8_t* __restrict__ o = dst + d.dst;
		const size_t ss = d.src_stride, ds = d.dst_stride;
		const int nd = (w + 3) >> 2;  // dwords per row
		if (d.filter == 0) {
			for (int i = tid; i < h * nd; i += (int)kThreads) {
				const int y = i / nd, x = (i - y * nd) * 4;
				store4(o + (size_t)y * ds, x, w, load4(s + (size_t)y * ss, x, w));
			}
		} else if (d.filter == 1) {
			if (wave == 0) {  // column 0
				uint32_t carry = 0;
				for (int y0 = 0; y0 < h; y0 += 64) {
					const int y = y0 + lane;
					const uint32_t inc = wave_scan(y < h ? (uint32_t)s[(size_t)y * ss] : 0u, lane);
					if (y < h) full8[y] = (uint8_t)(inc + carry);
					carry += (uint32_t)__shfl((int)inc, 63);
				}
			}
			__syncthreads();
			for (int y = wave; y < h; y += (int)kWaves) {
				uint32_t carry = 0;
				const int first = full8[y];
				for (int x0 = 0; x0 < w; x0 += 256) carry = scan_chunk(s + (size_t)y * ss, o + (size_t)y * ds, x0, w, lane, carry, first, nullptr);
			}
		} else if (d.filter == 2) {
			if (wave == 0) {  // row 0
				uint32_t carry = 0;
				for (int x0 = 0; x0 < w; x0 += 256) carry = scan_chunk(s, o, x0, w, lane, carry, -1, full32);
			}
			__syncthreads();
			for (int g = tid; g < nd; g += (int)kThreads) {
				uint32_t acc = full32[g];
				for (int y = 1; y < h; y++) {
					const uint32_t v = load4(s + (size_t)y * ss, 4 * g, w);
					acc = (((acc & 0x00FF00FFu) + (v & 0x00FF00FFu)) & 0x00FF00FFu) | (((acc & 0xFF00FF00u) + (v & 0xFF00FF00u)) & 0xFF00FF00u);
					store4(o + (size_t)y * ds, 4 * g, w, acc);
				}
			}
		} else {
			const int nbands = (h + 63) >> 6, ntiles = (w + 63 + kT - 1) / kT;
			// (the skew build's mutants, csrc/vp8g_skew.h: in the shipped library mut is the constant 0)
			const uint32_t mut = VP8G_BAND_MUTANT();
			const int delay = kDelay - (mut == kBandMutDelay ? 1 : 0);
			const uint32_t ringmask = (uint32_t)(mut == kBandMutRing ? kRing / 2 : kRing) - 1u;
			// a round: every wave one band.  Wave j starts kDelay steps after wave j - 1; the next round starts
			// when wave 0 trails wave 15 by kDelay steps at least (16 kDelay) and no earlier than kDelay steps
			// after a band's last tile, so that a wave's ring is not rewritten while the wave below reads it
			const int round_len =
			    (ntiles + delay > (int)kWaves * delay && mut != kBandMutNoLong ? ntiles + delay : (int)kWaves * delay) - (mut == kBandMutRound ? 1 : 0);
			const int rounds = (nbands + (int)kWaves - 1) / (int)kWaves;
			const int steps = (rounds - 1) * round_len + ((int)kWaves - 1) * delay + ntiles;
			uint32_t* const tile32 = (uint32_t*)(smem + wave * kTileBytes);
			// bottom rows: written at the writer's t, read at the reader's t + 63
			uint32_t* const hw32 = wave == (int)kWaves - 1 ? full32 : (uint32_t*)(smem + kOffRing + wave * kRing);
			const uint32_t* const hr32 = wave == 0 ? full32 : (const uint32_t*)(smem + kOffRing + (wave - 1) * kRing);
			const uint32_t wmask = wave == (int)kWaves - 1 ? 0x7FFFu : ringmask;
			const uint32_t rmask = wave == 0 ? 0x7FFFu : ringmask;
			const int trow = lane >> 4, tcol = lane & 15;  // load / store mapping: 16 lanes to a row, 4 rows per access
			uint32_t cur = 0, ul = 0;
			for (int st = 0; st < steps; st++) {
				const int rel = st - delay * wave;
				const int p = rel >= 0 ? rel / round_len : rounds;
				const int k = rel - p * round_len;
				const int b = p * (int)kWaves + wave;
				const bool on = p < rounds && b < nbands && k < ntiles;  // (wave-uniform)
				if (on) {
#pragma unroll 4
					for (int i = 0; i < 16; i++) {
						const int r = i * 4 + trow, y = b * 64 + r;
						if (y < h) tile32[r * kPitch32 + tcol] = load4(s + (size_t)y * ss, k * kT + 4 * tcol - r, w);
					}
				}
				__syncthreads();
				if (on) {
					if (k == 0) cur = 0, ul = 0;
					for (int c = 0; c < kT / 4; c++) {
						const int t4 = k * kT + 4 * c;
						const uint32_t word = tile32[lane * kPitch32 + c];
						const uint32_t pos = (uint32_t)t4 + 60u;
						const uint32_t d0 = hr32[(pos & rmask) >> 2], d1 = hr32[((pos + 4u) & rmask) >> 2];
						const uint32_t top4 = b ? (d0 >> 24) | (d1 << 8) : 0u;  // (band 0: a row of zeros above gives the top row's rule)
						uint32_t outw = 0;
#pragma unroll
						for (int q = 0; q < 4; q++) {
							const uint32_t up = from_lane_above(cur);
							const uint32_t a = lane == 0 ? (top4 >> (8 * q)) & 255u : up;
							int g = (int)cur + (int)a - (int)ul;  // (x = 0: cur = ul = 0, so the prediction is the pixel above)
							g = g < 0 ? 0 : g > 255 ? 255 : g;
							const uint32_t v = ((uint32_t)g + ((word >> (8 * q)) & 255u)) & 255u;
							const bool act = t4 + q >= lane;  // x >= 0
							cur = act ? v : 0u;
							ul = act ? a : 0u;
							outw |= v << (8 * q);
						}
						tile32[lane * kPitch32 + c] = outw;
						if (lane == 63) hw32[((uint32_t)t4 & wmask) >> 2] = outw;
					}
				}
				__syncthreads();
				if (on) {
#pragma unroll 4
					for (int i = 0; i < 16; i++) {
						const int r = i * 4 + trow, y = b * 64 + r;
						if (y < h) store4(o + (size_t)y * ds, k * kT + 4 * tcol - r, w, tile32[r * kPitch32 + tcol]);
					}
				}
				__syncthreads();
			}
		}
		__syncthreads();
	}
}

bool desc_ok(const Vp8gAlphaDesc& d) {
	return d.width >= 1 && d.height >= 1 && d.width <= kMaxDim && d.height <= kMaxDim && d.filter <= 3 && d.src_stride >= d.width &&
	       d.dst_stride >= d.width && d.ntasks == 1;
}

}  // namespace

// (tests/bands.py states the hand-over geometry once more; tests/test_gpu_bands.py holds the two together)
VP8G_API void vp8g_alpha_handover(uint32_t out[4]) { out[0] = (uint32_t)kT, out[1] = (uint32_t)kDelay, out[2] = (uint32_t)kRing, out[3] = (uint32_t)kFull; }
VP8G_BAND_EXPORTS(alpha)

VP8G_API int vp8g_make_alpha_desc(uint32_t width, uint32_t height, uint32_t filter, uint64_t src, uint32_t src_stride, uint64_t dst,
                                  uint32_t dst_stride, uint32_t task0, Vp8gAlphaDesc* out) {
	if (!out) {
		errno = EINVAL;
		return -1;
	}
	Vp8gAlphaDesc d;
	memset(&d, 0, sizeof(d));
	d.src = src, d.dst = dst, d.width = width, d.height = height, d.src_stride = src_stride, d.dst_stride = dst_stride;
	d.filter = filter, d.task0 = task0, d.ntasks = 1;
	if (!desc_ok(d)) {
		errno = EINVAL;
		return -1;
	}
	*out = d;
	return 0;
}

VP8G_API int vp8g_alpha_unfilter_batch_device(const Vp8gAlphaDesc* h, const Vp8gAlphaDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                              uint8_t* d_dst, void* stream) {
	bool ok = h && d_descs && d_src && d_dst && n > 0 && n <= 0x7FFFFFFFu;
	bool gradient = false;
	for (uint32_t i = 0; ok && i < n; i++) ok = desc_ok(h[i]) && h[i].task0 == i, gradient |= h[i].filter == 3;
	if (!ok) return vp8g::fail(EINVAL);
	static const hipError_t attr =
	    hipFuncSetAttribute((const void*)alpha_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
	// the tiles and rings are the gradient's: a launch without one asks for the full-width row only, and two
	// 16-wave workgroups share a CU; with one, a workgroup's LDS fills more than half a CU's
	const uint32_t lds = gradient ? (uint32_t)kLdsBytes : (uint32_t)kFull, full_off = gradient ? (uint32_t)kOffFull : 0u;
	const uint32_t grid = vp8g::grid_for(n, gradient ? 1u : 2u);
	return vp8g::gated_launch(
	    (hipStream_t)stream, "alpha launch",
	    [&] {
		    hipLaunchKernelGGL(alpha_kernel, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, d_descs, n, d_src, d_dst, full_off);
		    return hipGetLastError();
	    },
	    attr);
}
