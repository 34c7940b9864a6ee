// vp8g_scale_argb_fused.hip -- crop + shrink of ARGB pictures straight into tensor elements, bit-exact to libwebp 1.2.2's
// decoder options on a picture with alpha (include/vp8g.h: vp8g_scale_argb_tensor_batch_device; host restatement
// vp8f_argb_scale in host/vp8_scale.c followed by the tensor arithmetic).
//
// The planar route (vp8g_scale_argb.hip) splits the window into four byte planes, rescales each, merges them and hands
// the picture to the tensor kernel: five launches, a work buffer twice the window's size, twelve bytes moved per window
// pixel.  Here one kernel does all of it for the pictures that shrink (or keep) both axes:
//
//   stage    a task's source rows go through LDS in blocks of block_rows row segments, one 16-byte load per four pixels
//            (the source is only dword-aligned and the window's origin may be odd: a segment starts 0, 4, 8 or 12 bytes
//            into its first 16-byte chunk); every pixel is alpha-premultiplied on its way into LDS (§17.7 step 3), and
//            the next block is in flight in registers while the current one is summed;
//   sum      the closed form at the head of vp8g_scale_device.h -- frow, irow, the boundary row of a run, `group` lanes per
//            output column combined by the lane butterfly -- for the four byte channels of a column together: a lane
//            reads a staged pixel once and adds its bytes to two registers of two 16-bit fields each (B | R and G | A;
//            a lane sums at most kMaxSeg / 64 + 1 pixels of a row, so a field never carries), and keeps four irows;
//   export   at every F(j + 1) boundary lane 0 of a column has the premultiplied pixel: it un-premultiplies it (§17.7
//            step 5), the lanes of four adjacent columns hand theirs to the first by lane exchange, and that lane
//            converts them (conv / conv_a of vp8g_tensor_device.h) and stores them as the compositor does: one run of
//            4 C elements (NHWC) or C runs of four (NCHW) through store_run, element by element at a row's ragged end
//            and where a wave holds fewer than four columns (group > 16).
//
// One launch takes pictures of mixed sizes, windows and targets; a workgroup task is tile_w = 256 / group output columns
// x run_h output rows of one picture, tasks numbered picture by picture.  No planes, no work buffer.  No workgroup waits
// on another and nothing spins on memory.
#include <errno.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../host/vp8_front.h"
#include "vp8g_device.h"
#include "vp8g_scale_device.h"
#include "vp8g_tensor_device.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))
#define DEV __device__ __forceinline__

namespace {

using namespace vp8g_tensor;
using namespace vp8g_scale;

constexpr uint32_t kBufBytes = 32768;                 // LDS staging: five workgroups to a CU's 160 KB
constexpr uint32_t kMaxSeg = (kBufBytes - 16u) / 4u;  // pixels of the longest row segment that can be staged (8188)
constexpr uint32_t kQuad = 4;                         // adjacent columns whose pixels one lane stores
static_assert(kBufBytes / 16u % kThreads == 0, "whole chunks per thread");
static_assert((kMaxSeg / 64u + 1u) * 255u < 65536u, "a lane's sum of one byte channel over a row fits 16 bits");
static_assert(sizeof(Vp8gScaleArgbTensorDesc) == 96, "descriptor layout (no padding: desc_ok compares byte for byte)");

struct FusedParams {
	float scale[3], bias[3];
};

// the four elements of pixel c (0xAARRGGBB) in the output's channel order
template <uint32_t DT, bool BGR>
DEV void elements(uint32_t c, const FusedParams& P, uint32_t (&e)[4]) {
	// (channel<> reads r | g << 8 | b << 16)
	const uint32_t rgb = ((c >> 16) & 255u) | (c & 0xFF00u) | ((c & 255u) << 16);
#pragma unroll
	for (int q = 0; q < 3; q++) e[q] = conv<DT>(channel<BGR>(rgb, q), P.scale[q], P.bias[q]);
	e[3] = conv_a<DT>(c >> 24);
}

template <uint32_t DT, bool PLANAR, bool BGR, int C>
__global__ __launch_bounds__(kThreads) void scale_argb_fused_kernel(const Vp8gScaleArgbTensorDesc* __restrict__ descs, uint32_t n,
                                                                    FusedParams P, const uint8_t* __restrict__ src,
                                                                    uint8_t* __restrict__ dst) {
	static_assert(C == 3 || C == 4, "RGB, or RGB and alpha");
	constexpr uint32_t EB = (uint32_t)elem_bytes(DT);
	__shared__ __attribute__((aligned(16))) uint8_t lds[kBufBytes];
	const uint32_t* const ldsw = (const uint32_t*)lds;
	const uint32_t task = blockIdx.x, tid = threadIdx.x;
	// the picture that owns this task (tasks are numbered picture by picture)
	const Vp8gScaleArgbTensorDesc& D = descs[task_owner<Vp8gScaleArgbTensorDesc, &Vp8gScaleArgbTensorDesc::task0>(descs, n, task)];
	const uint32_t t = task - D.task0;
	if (task < D.task0 || t >= D.ntasks) return;
	const uint32_t W = D.win_w, H = D.win_h, w = D.width, h = D.height;
	const uint32_t fx = D.fx, fxy = D.fxy;
	const uint32_t G = D.group, pitch = D.pitch, R = D.block_rows, sw = D.src_width;
	if (G == 0 || (G & (G - 1u)) || G > 64u || D.tile_w * G != kThreads || D.tiles_x == 0 || D.run_h == 0 || w > W || h > H) return;
	const uint32_t tx = t % D.tiles_x, ry = t / D.tiles_x;

	// -- columns: the tile's source segment [xs, xe) and this lane's footprint, in pixels of the window
	const uint32_t k0 = tx * D.tile_w, kend = min(k0 + D.tile_w, w);
	const uint32_t j0 = ry * D.run_h, j1 = min(j0 + D.run_h, h);
	if (k0 >= w || j0 >= h) return;
	const uint32_t xs = k0 ? ceil_div(k0 * W, w) - 1u : 0u;  // E(k0) - 1: the first column's carry pixel
	const uint32_t xe = ceil_div(kend * W, w);                // E(kend) <= W
	const uint32_t span = xe - xs;
	if (4u * span + 12u > pitch || (pitch & 15u) || R == 0 || (uint64_t)pitch * R > kBufBytes) return;  // (never: see make_desc)
	const uint32_t gi = tid & (G - 1u), col = tid / G, k = k0 + col;
	const ShrinkCol fp(k, kend, xs, W, w);
	ShrinkRows rows(j0, j1, H, h, D.fy);
	// (the window's first pixel; rows 4 src_width bytes apart)
	StagedRows<4, kBufBytes> stage(src, (uintptr_t)src + D.src + 4u * ((uintptr_t)D.crop_top * sw + D.crop_left), 4u * sw, W, H, xs, span,
	                               pitch, tid);

	uint32_t irow[4] = {0, 0, 0, 0};
	// the lane that stores a quad: lane 0 of the first of four adjacent columns, all four in this wave and in the picture
	const bool quads = kQuad * G <= 64u;
	const bool quad_head = quads && gi == 0 && (col & (kQuad - 1u)) == 0 && k + kQuad <= kend;
	const bool quad_tail = quads && k < kend && (k0 + (col & ~(kQuad - 1u))) + kQuad <= kend;  // its pixel goes out with a quad
	uint8_t* const out = dst + D.dst;
	const uint64_t plane = (uint64_t)w * h * EB;  // one NCHW plane of this picture
	const uint32_t y_last = rows.y_last;
	stage.load(rows.y_first, min(R, y_last - rows.y_first));
	for (uint32_t yb = rows.y_first; yb < y_last; yb += R) {
		const uint32_t nr = min(R, y_last - yb);
		__syncthreads();  // the previous block has been summed
		stage.store(lds, nr, [](uint32_t p) { return premultiply(p); });  // (§17.7 step 3)
		__syncthreads();
		if (yb + R < y_last) stage.load(yb + R, min(R, y_last - (yb + R)));  // in flight while this block is summed
		for (uint32_t r = 0; r < nr; r++) {
			const uint32_t y = yb + r;
			const uint32_t off = (stage.lds_offset(r, y) >> 2) - xs;  // ldsw[off + x] = premultiplied s[y][x] for x in [xs, xe)
			uint32_t br = 0, ga = 0;  // B | R << 16 and G | A << 16
			for (uint32_t x = fp.e0 + gi; x < fp.e1; x += G) {
				const uint32_t p = ldsw[off + x];
				br += p & 0x00FF00FFu, ga += (p >> 8) & 0x00FF00FFu;
			}
			uint32_t part[4] = {br & 0xFFFFu, ga & 0xFFFFu, br >> 16, ga >> 16};  // the dword's byte order: B, G, R, A
			for (uint32_t o = G >> 1; o; o >>= 1) {
#pragma unroll
				for (int c = 0; c < 4; c++) part[c] += __shfl_xor(part[c], (int)o);
			}
			uint32_t frow[4] = {0, 0, 0, 0};
			if (fp.active) {
				const uint32_t pc = fp.carry_in ? ldsw[off + fp.e0 - 1u] : 0u, pl = ldsw[off + fp.e1 - 1u];
#pragma unroll
				for (int c = 0; c < 4; c++) frow[c] = fp.frow((pc >> (8 * c)) & 255u, part[c], (pl >> (8 * c)) & 255u, w, fx);
			}
			if (rows.shared_row(y)) {  // the row shared with the run above: only its lower part
#pragma unroll
				for (int c = 0; c < 4; c++) irow[c] = rows.lower_part(frow[c]);
				continue;
			}
#pragma unroll
			for (int c = 0; c < 4; c++) irow[c] += frow[c];
			if (!rows.exports(y)) continue;
			uint32_t px = 0;
#pragma unroll
			for (int c = 0; c < 4; c++) px |= rows.sample(irow[c], frow[c], fxy) << (8 * c);
			px = unpremultiply(px);  // (§17.7 step 5)
			// (every lane of the wave takes part in the exchange: the row test above is the same for all of them)
			uint32_t q4[kQuad] = {px, 0u, 0u, 0u};
			if (quads) {
#pragma unroll
				for (uint32_t q = 1; q < kQuad; q++) q4[q] = (uint32_t)__shfl_down((int)px, q * G);
			}
			const size_t pix = (size_t)rows.j * w + k;
			if (quad_head) {
				uint32_t e[kQuad][4];
#pragma unroll
				for (uint32_t q = 0; q < kQuad; q++) elements<DT, BGR>(q4[q], P, e[q]);
				if constexpr (PLANAR) {
#pragma unroll
					for (int c = 0; c < C; c++) {
						const uint32_t run[kQuad] = {e[0][c], e[1][c], e[2][c], e[3][c]};
						store_run<DT, (int)kQuad>(out + (size_t)c * plane + pix * EB, run);
					}
				} else {
					uint32_t run[kQuad * C];
#pragma unroll
					for (int q = 0; q < (int)kQuad; q++)
#pragma unroll
						for (int c = 0; c < C; c++) run[C * q + c] = e[q][c];
					store_run<DT, (int)kQuad * C>(out + pix * C * EB, run);
				}
			} else if (fp.active && gi == 0 && !quad_tail) {  // a row's ragged end, or group > 16: element by element
				uint32_t e[4];
				elements<DT, BGR>(px, P, e);
#pragma unroll
				for (int c = 0; c < C; c++) {
					uint8_t* p = PLANAR ? out + (size_t)c * plane + pix * EB : out + (pix * C + (uint32_t)c) * EB;
					store_elem<DT>(p, e[c]);
				}
			}
			rows.next();
		}
	}
}

using KernelFn = void (*)(const Vp8gScaleArgbTensorDesc*, uint32_t, FusedParams, const uint8_t*, uint8_t*);
// [C - 3][dtype][layout][bgr]
#define VP8G_F_ROW(DT, C) \
	{ {scale_argb_fused_kernel<DT, false, false, C>, scale_argb_fused_kernel<DT, false, true, C>}, \
	  {scale_argb_fused_kernel<DT, true, false, C>, scale_argb_fused_kernel<DT, true, true, C>} }
const KernelFn kKernels[2][4][2][2] = {{VP8G_F_ROW(VP8G_T_U8, 3), VP8G_F_ROW(VP8G_T_F16, 3), VP8G_F_ROW(VP8G_T_BF16, 3), VP8G_F_ROW(VP8G_T_F32, 3)},
                                       {VP8G_F_ROW(VP8G_T_U8, 4), VP8G_F_ROW(VP8G_T_F16, 4), VP8G_F_ROW(VP8G_T_BF16, 4), VP8G_F_ROW(VP8G_T_F32, 4)}};
#undef VP8G_F_ROW

// 0; -1 + EINVAL (options that do not fit, a misaligned source); -1 + ENOTSUP (valid, but not this kernel's)
int make_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t dst, uint32_t task0,
              Vp8gScaleArgbTensorDesc* out) {
	Vp8fScaleGeom g;
	if (!out || vp8f_scale_resolve_argb(width, height, opt, &g) != 0 || src % 4u) return vp8g::fail(EINVAL);
	if (!g.scaling || g.out_w > g.win_w || g.out_h > g.win_h) return vp8g::fail(ENOTSUP);  // a plain copy; an axis that expands
	const uint32_t W = g.win_w, H = g.win_h, w = g.out_w, h = g.out_h;
	Vp8gScaleArgbTensorDesc d;
	memset(&d, 0, sizeof(d));
	d.src = src, d.dst = dst;
	d.width = w, d.height = h, d.src_width = width, d.src_height = height;
	d.crop_left = g.left, d.crop_top = g.top, d.win_w = W, d.win_h = H;
	vp8f_scale_factors(W, H, w, h, &d.fx, &d.fy, &d.fxy);
	const ShrinkTiling t = shrink_tiling(W, H, w, h, 4u, kBufBytes);
	d.group = t.group, d.tile_w = t.tile_w, d.tiles_x = t.tiles_x, d.run_h = t.run_h;
	if (t.ntasks + task0 > 0x7FFFFFFFu) return vp8g::fail(EINVAL);
	d.task0 = task0, d.ntasks = (uint32_t)t.ntasks;
	if (t.span > kMaxSeg) return vp8g::fail(ENOTSUP);  // (four columns of 64 lanes each: only where W / w exceeds 2046)
	d.pitch = t.pitch, d.block_rows = t.block_rows;
	*out = d;
	return 0;
}

// exactly what make_desc gives for the picture, window and target the descriptor names
bool desc_ok(const Vp8gScaleArgbTensorDesc& d) {
	const Vp8gScaleOpt o = {d.crop_left, d.crop_top, d.win_w, d.win_h, d.width, d.height, 0u};
	Vp8gScaleArgbTensorDesc m;
	return make_desc(d.src_width, d.src_height, d.src, &o, d.dst, d.task0, &m) == 0 && memcmp(&m, &d, sizeof(d)) == 0;
}

}  // namespace

// (tests/test_gpu_anim_scale.py takes its boundary sizes from here, through vp8g.scale_argb_fused_geometry())
VP8G_API void vp8g_scale_argb_fused_geometry(uint32_t out[3]) { out[0] = 4u, out[1] = kMaxSeg, out[2] = kRunSrcRows; }

VP8G_API int vp8g_make_scale_argb_tensor_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                                              uint32_t task0, Vp8gScaleArgbTensorDesc* out) {
	return make_desc(width, height, src, opt, dst_offset, task0, out);
}

VP8G_API int vp8g_scale_argb_tensor_batch_device(const Vp8gScaleArgbTensorDesc* h, const Vp8gScaleArgbTensorDesc* d_descs, uint32_t n,
                                                 const Vp8gTensorOpt* t, uint32_t channels, const uint8_t* d_src, void* d_dst, void* stream) {
	if (!h || !d_descs || !d_src || !d_dst || n == 0 || (channels != 3 && channels != 4) || !vp8g_tensor_slot_size(t) ||
	    (uintptr_t)d_src % 4u || (uintptr_t)d_descs % 8u)
		return vp8g::fail(EINVAL);
	const uint32_t eb = (uint32_t)elem_bytes(t->dtype);
	if ((uintptr_t)d_dst % eb) return vp8g::fail(EINVAL);
	uint64_t total = 0;
	try {
		std::vector<uint32_t> by_dst(n);
		for (uint32_t i = 0; i < n; i++) {
			const Vp8gScaleArgbTensorDesc& d = h[i];
			if (d.task0 != total || d.dst % eb || !desc_ok(d)) return vp8g::fail(EINVAL);  // tasks must be numbered picture by picture
			total += d.ntasks;
			if (total > 0x7FFFFFFFu) return vp8g::fail(EINVAL);
			by_dst[i] = i;
		}
		// no two pictures' slots may share bytes
		std::sort(by_dst.begin(), by_dst.end(), [&](uint32_t a, uint32_t b) { return h[a].dst < h[b].dst; });
		for (uint32_t q = 1; q < n; q++) {
			const Vp8gScaleArgbTensorDesc& p = h[by_dst[q - 1]];
			if (p.dst + (uint64_t)channels * p.width * p.height * eb > h[by_dst[q]].dst) return vp8g::fail(EINVAL);
		}
	} catch (const std::bad_alloc&) {
		return vp8g::fail(ENOMEM);
	}
	FusedParams P;
	for (int c = 0; c < 3; c++) P.scale[c] = t->scale[c], P.bias[c] = t->bias[c];
	hipStream_t s = (hipStream_t)stream;
	return vp8g::gated_launch(s, "argb fused scale launch", [&] {
		hipLaunchKernelGGL(kKernels[channels == 4u][t->dtype][t->layout][t->flags & VP8G_T_BGR], dim3((uint32_t)total), dim3(kThreads), 0, s,
		                   d_descs, n, P, d_src, (uint8_t*)d_dst);
		return hipGetLastError();
	});
}
