// vp8g_tensor.hip -- device-resident I420 (and an alpha plane), or ARGB, -> one dense RGB / RGBA tensor, in
// the form a model reads (include/vp8g.h: vp8g_tensor_batch_device, _a, _argb).
//
// The pixels are those of the file encoder (vp8g_rgb.hip: "fancy" 4:2:0 upsampling, libwebp's
// VP8YuvToRgb; both go through vp8g_rgb_device.h), but the unit of work is a run of pixels of one
// row, not a span of a file: a thread takes one chunk of 12 pixels of a row (six pixel pairs; one
// unaligned 8-byte load per chroma row and plane, one 12-byte luma load), converts them to the
// element type -- out = u8 * scale[c] + bias[c], a rounded multiply and then a rounded add -- and
// stores them:
//   NHWC  one run of 12 C elements;
//   NCHW  C runs of 12 elements, one per plane; neighbouring lanes hold neighbouring chunks of
//         the row, so each plane's stores are contiguous across the lanes of a wave.
// C = 3, or 4 with alpha as the fourth channel (the byte, or a / 255; scale and bias never touch it): one
// kernel, tensor_kernel<.., C>, whose alpha parts sit under `if constexpr (C == 4)`.
// A run whose address is dword-aligned goes out as 16- / 8- / 4-byte stores; runs of a row that
// starts off a dword boundary (an odd slot start, an odd width) go out element by element, as do
// the pixels of a row's last, partial chunk and of images narrower than 15 pixels (chroma rows
// shorter than the 8-byte load).  Every store lies inside the image's own C * w * h elements.
// No LDS and no barriers.  A workgroup task is 256 consecutive chunks of one image; the dtype,
// layout, channel order and channel count are template parameters picked on the host.
// Three planes of the picture's own size (vp8g_tensor_batch_device_444: libwebp's scaled RGB, whose chroma the rescaler
// has already taken to the luma target) are a source mode of the same kernel, tensor_kernel_444: a whole
// chunk is one unaligned 12-byte load per plane and VP8YuvToRgb per pixel, and everything from the colour on is shared.
// ARGB sources (lossless images) have a kernel of their own further down; the entry points share
// one host path, launch_tensor.
#include <errno.h>
#include <string.h>

#include <cmath>

#include <hip/hip_fp16.h>

#include "vp8g_device.h"
#include "vp8g_rgb_device.h"
#include "vp8g_tensor_device.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))
#define DEV __device__ __forceinline__

namespace {

using namespace vp8g_rgb;
using namespace vp8g_tensor;  // conv, conv_a, channel, store_run, ...: shared with vp8g_anim.hip

constexpr uint32_t kThreads = 256;  // chunks per workgroup task
constexpr uint32_t kMaxDim = 16383;

struct TensorParams {
	uint32_t w, h, cw, ch;
	uint32_t cpr;          // chunks per row
	uint32_t chunks;       // chunks per image (cpr * h)
	uint32_t tpi;          // workgroup tasks per image
	uint32_t reserved;
	uint64_t plane;        // bytes of one NCHW plane (w * h * element size)
	float scale[3], bias[3];
};

// S444: the source is three planes of the picture's own size (libwebp's scaled RGB; stride_uv is then the
// stride of full-width U and V planes): the pixel is VP8YuvToRgb of its own three samples, no upsampler.  Everything
// after the colours -- alpha, elements, stores -- is the one code below.
template <uint32_t DT, bool PLANAR, bool BGR, int C, bool S444>
DEV void tensor_body(const Vp8gTensorDesc* __restrict__ D, const Vp8gTensorAlpha* __restrict__ A, uint32_t total, const TensorParams& P,
                     const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
	static_assert(C == 3 || C == 4, "RGB, or RGB and alpha");
	constexpr uint32_t EB = (uint32_t)elem_bytes(DT);
	const uint32_t tid = threadIdx.x, W = P.w;
	for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
		const uint32_t img = g / P.tpi;  // (every image has P.tpi tasks, numbered image by image)
		const uint32_t gc = (g - img * P.tpi) * kThreads + tid;
		if (gc >= P.chunks) continue;
		const Vp8gTensorDesc& d = D[img];
		const uint32_t y = gc / P.cpr, x0 = (gc - y * P.cpr) * kChunk;
		// chroma rows (as vp8g_rgb.hip): row 0 uses row 0 twice; row y sits between a = (y-1)/2 and
		// b = min(a+1, ch-1), nearer a when y is odd
		// (S444: both "chroma rows" are the pixel row's own)
		const uint32_t a = S444 ? y : y ? (y - 1u) >> 1 : 0u, b = S444 ? y : y ? min(a + 1u, P.ch - 1u) : 0u;
		const bool near_a = y == 0 || (y & 1u);
		const uint8_t* yrow = src + d.src_y + (size_t)y * d.stride_y;
		const uint8_t* ua = src + d.src_u + (size_t)a * d.stride_uv;
		const uint8_t* ub = src + d.src_u + (size_t)b * d.stride_uv;
		const uint8_t* va = src + d.src_v + (size_t)a * d.stride_uv;
		const uint8_t* vb = src + d.src_v + (size_t)b * d.stride_uv;
		// C == 4: the alpha bytes of a chunk are read one by one (a plane of any stride and alignment), where
		// their elements are stored; an opaque image reads none.  C == 3 never reads A.
		[[maybe_unused]] bool opaque = true;
		[[maybe_unused]] const uint8_t* arow = src;
		if constexpr (C == 4) {
			const Vp8gTensorAlpha al = A[img];
			opaque = al.src_a == VP8G_T_OPAQUE;
			if (!opaque) arow = src + al.src_a + (size_t)y * al.stride_a;
		}
		[[maybe_unused]] auto alpha = [&](uint32_t x) { return conv_a<DT>(opaque ? 255u : (uint32_t)arow[x]); };
		uint8_t* out = dst + d.dst;
		const size_t pix = (size_t)y * W + x0;  // the chunk's first pixel in the image
		if (x0 + kChunk <= W && (S444 || P.cw >= 8u)) {
			uint32_t c[kChunk];
			if constexpr (S444) chunk_yuv444(yrow, ua, va, x0, c);
			else chunk_rgb(yrow, ua, ub, va, vb, x0, (int)P.cw, near_a, c);
			if constexpr (PLANAR) {
#pragma unroll
				for (int ch = 0; ch < C; ch++) {
					uint32_t e[kChunk];
#pragma unroll
					for (int i = 0; i < (int)kChunk; i++)
						e[i] = ch < 3 ? conv<DT>(channel<BGR>(c[i], ch), P.scale[ch % 3], P.bias[ch % 3]) : alpha(x0 + (uint32_t)i);
					store_run<DT, (int)kChunk>(out + (size_t)ch * P.plane + pix * EB, e);
				}
			} else if constexpr (C == 3 && DT == VP8G_T_U8) {
				// 12 pixels -> 36 bytes -> 9 dwords (4 pixels = 3 dwords), as the file encoder packs them
				uint8_t* p = out + pix * 3u;
				if (BGR) {
#pragma unroll
					for (int i = 0; i < (int)kChunk; i++) c[i] = (c[i] & 0xFF00u) | (c[i] >> 16) | ((c[i] & 0xFFu) << 16);
				}
				if (((uintptr_t)p & 3u) == 0) {
					uint32_t dw[9];
#pragma unroll
					for (int k = 0; k < 3; k++) {
						dw[3 * k + 0] = c[4 * k] | (c[4 * k + 1] << 24);
						dw[3 * k + 1] = (c[4 * k + 1] >> 8) | (c[4 * k + 2] << 16);
						dw[3 * k + 2] = (c[4 * k + 2] >> 16) | (c[4 * k + 3] << 8);
					}
					store_dwords<9>(p, dw);
				} else {
#pragma unroll
					for (int i = 0; i < 3 * (int)kChunk; i++) p[i] = (uint8_t)(c[i / 3] >> (8 * (i % 3)));
				}
			} else {
				uint32_t e[C * kChunk];
#pragma unroll
				for (int i = 0; i < (int)kChunk; i++) {
#pragma unroll
					for (int ch = 0; ch < 3; ch++) e[C * i + ch] = conv<DT>(channel<BGR>(c[i], ch), P.scale[ch], P.bias[ch]);
					if constexpr (C == 4) e[4 * i + 3] = alpha(x0 + (uint32_t)i);
				}
				store_run<DT, C * (int)kChunk>(out + pix * (uint32_t)C * EB, e);
			}
			continue;
		}
		// generic chunk (a row's last, partial chunk; 4:2:0 images narrower than 15 pixels): pixel by pixel
		const uint32_t xe = min(x0 + kChunk, W);
		for (uint32_t x = x0; x < xe; x++) {
			const uint32_t col = S444 ? yuv_rgb(yrow[x], ua[x], va[x]) : pixel_rgb(yrow, ua, ub, va, vb, x, P.cw, near_a);
			const size_t px = (size_t)y * W + x;
#pragma unroll
			for (int ch = 0; ch < C; ch++) {
				uint8_t* p = PLANAR ? out + (size_t)ch * P.plane + px * EB : out + (px * (uint32_t)C + (uint32_t)ch) * EB;
				store_elem<DT>(p, ch < 3 ? conv<DT>(channel<BGR>(col, ch), P.scale[ch % 3], P.bias[ch % 3]) : alpha(x));
			}
		}
	}
}

template <uint32_t DT, bool PLANAR, bool BGR, int C>
__global__ __launch_bounds__(kThreads) void tensor_kernel(const Vp8gTensorDesc* __restrict__ D, const Vp8gTensorAlpha* __restrict__ A,
                                                          uint32_t total, TensorParams P, const uint8_t* __restrict__ src,
                                                          uint8_t* __restrict__ dst) {
	tensor_body<DT, PLANAR, BGR, C, false>(D, A, total, P, src, dst);
}

template <uint32_t DT, bool PLANAR, bool BGR, int C>
__global__ __launch_bounds__(kThreads) void tensor_kernel_444(const Vp8gTensorDesc* __restrict__ D, const Vp8gTensorAlpha* __restrict__ A,
                                                              uint32_t total, TensorParams P, const uint8_t* __restrict__ src,
                                                              uint8_t* __restrict__ dst) {
	tensor_body<DT, PLANAR, BGR, C, true>(D, A, total, P, src, dst);
}

// ---- ARGB sources (vp8g_tensor_batch_device_argb) ------------------------------

// Tight 0xAARRGGBB dwords, as the lossless kernel leaves them.  Source and NHWC destination are both
// flat in the pixel index, so a thread takes four consecutive pixels of the image (one 16-byte load;
// NHWC: one run of 4 C elements, NCHW: a run of four per plane), and a workgroup task 1024 of them; the
// last pixels of an image whose size is no multiple of four go element by element.  The arithmetic on
// R, G and B is conv<>, that on A conv_a<>.
constexpr uint32_t kArgbPx = 4;

template <uint32_t DT, bool PLANAR, bool BGR, int C>
__global__ __launch_bounds__(kThreads) void tensor_kernel_argb(const Vp8gTensorArgbDesc* __restrict__ D, uint32_t total, TensorParams P,
                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
	constexpr uint32_t EB = (uint32_t)elem_bytes(DT);
	const uint32_t npx = P.w * P.h;
	for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
		const uint32_t img = g / P.tpi;
		const uint32_t p0 = ((g - img * P.tpi) * kThreads + threadIdx.x) * kArgbPx;
		if (p0 >= npx) continue;
		const Vp8gTensorArgbDesc& d = D[img];
		const uint32_t* in = (const uint32_t*)(src + d.src);
		uint8_t* out = dst + d.dst;
		uint32_t c[kArgbPx], e[kArgbPx][4];
		const uint32_t cnt = min(kArgbPx, npx - p0);
		if (cnt == kArgbPx) {
			const u32x4a v = *(const u32x4a*)(in + p0);
			c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
		} else {
#pragma unroll
			for (int i = 0; i < (int)kArgbPx; i++) c[i] = (uint32_t)i < cnt ? in[p0 + i] : 0u;
		}
#pragma unroll
		for (int i = 0; i < (int)kArgbPx; i++) {
			// (channel<> reads r | g << 8 | b << 16)
			const uint32_t rgb = ((c[i] >> 16) & 255u) | (c[i] & 0xFF00u) | ((c[i] & 255u) << 16);
#pragma unroll
			for (int k = 0; k < 3; k++) e[i][k] = conv<DT>(channel<BGR>(rgb, k), P.scale[k], P.bias[k]);
			e[i][3] = conv_a<DT>(c[i] >> 24);
		}
		if (cnt == kArgbPx) {
			if constexpr (PLANAR) {
#pragma unroll
				for (int k = 0; k < C; k++) {
					const uint32_t r[kArgbPx] = {e[0][k], e[1][k], e[2][k], e[3][k]};
					store_run<DT, (int)kArgbPx>(out + (size_t)k * P.plane + (size_t)p0 * EB, r);
				}
			} else {
				uint32_t r[kArgbPx * C];
#pragma unroll
				for (int i = 0; i < (int)kArgbPx; i++)
#pragma unroll
					for (int k = 0; k < C; k++) r[C * i + k] = e[i][k];
				store_run<DT, (int)kArgbPx * C>(out + (size_t)p0 * C * EB, r);
			}
			continue;
		}
		for (uint32_t i = 0; i < cnt; i++)
#pragma unroll
			for (int k = 0; k < C; k++) {
				const size_t px = (size_t)p0 + i;
				uint8_t* p = PLANAR ? out + (size_t)k * P.plane + px * EB : out + (px * C + (uint32_t)k) * EB;
				store_elem<DT>(p, i == 0 ? e[0][k] : i == 1 ? e[1][k] : e[2][k]);
			}
	}
}

using KernelFnArgb = void (*)(const Vp8gTensorArgbDesc*, uint32_t, TensorParams, const uint8_t*, uint8_t*);
using KernelFn = void (*)(const Vp8gTensorDesc*, const Vp8gTensorAlpha*, uint32_t, TensorParams, const uint8_t*, uint8_t*);
// [C - 3][dtype][layout][bgr]
#define VP8G_T_ROW(K, DT, C) { {K<DT, false, false, C>, K<DT, false, true, C>}, {K<DT, true, false, C>, K<DT, true, true, C>} }
#define VP8G_T_TABLE(K) \
	{ {VP8G_T_ROW(K, VP8G_T_U8, 3), VP8G_T_ROW(K, VP8G_T_F16, 3), VP8G_T_ROW(K, VP8G_T_BF16, 3), VP8G_T_ROW(K, VP8G_T_F32, 3)}, \
	  {VP8G_T_ROW(K, VP8G_T_U8, 4), VP8G_T_ROW(K, VP8G_T_F16, 4), VP8G_T_ROW(K, VP8G_T_BF16, 4), VP8G_T_ROW(K, VP8G_T_F32, 4)} }
const KernelFn kKernels[2][4][2][2] = VP8G_T_TABLE(tensor_kernel);
const KernelFn kKernels444[2][4][2][2] = VP8G_T_TABLE(tensor_kernel_444);
const KernelFnArgb kKernelsArgb[2][4][2][2] = VP8G_T_TABLE(tensor_kernel_argb);
#undef VP8G_T_TABLE
#undef VP8G_T_ROW

bool opt_ok(const Vp8gTensorOpt* t) {
	if (!t || t->width == 0 || t->height == 0 || t->width > kMaxDim || t->height > kMaxDim || t->dtype > VP8G_T_F32 ||
	    t->layout > VP8G_T_NCHW || (t->flags & ~VP8G_T_BGR))
		return false;
	if (t->dtype != VP8G_T_U8)
		for (int c = 0; c < 3; c++)
			if (!std::isfinite(t->scale[c]) || !std::isfinite(t->bias[c])) return false;
	return true;
}

uint32_t tasks_per_image(const Vp8gTensorOpt& t) {
	const uint32_t chunks = ((t.width + kChunk - 1u) / kChunk) * t.height;
	return (chunks + kThreads - 1u) / kThreads;
}

uint32_t argb_tasks_per_image(const Vp8gTensorOpt& t) {
	const uint32_t per = kThreads * kArgbPx;
	return (t.width * t.height + per - 1u) / per;
}

uint64_t slot_size(const Vp8gTensorOpt* t, uint64_t channels) {
	if (!opt_ok(t)) {
		errno = EINVAL;
		return 0;
	}
	return channels * t->width * t->height * (uint64_t)elem_bytes(t->dtype);
}

// What the three entry points share.  ptrs_ok: the caller's own pointer and argument checks.  The option and the
// tensor's base are checked here, then every descriptor: tasks numbered image by image, tpi(*t) each, the slot on an
// element boundary, and desc_ok(i), the entry point's own conditions.  table is [dtype][layout][bgr];
// args... are the kernel's leading (descriptor) arguments.  (P.cw .. P.chunks describe the I420 kernel's chunks; the
// ARGB kernel does not read them.)
template <class Desc, class Ok, class Kernel, class... Args>
int launch_tensor(bool ptrs_ok, const Desc* h, uint32_t n, const Vp8gTensorOpt* t, uint32_t (*tpi_of)(const Vp8gTensorOpt&),
                  const uint8_t* d_src, void* d_dst, void* stream, Ok&& desc_ok, const Kernel (&table)[4][2][2], Args... args) {
	if (!ptrs_ok || !h || !d_src || !d_dst || n == 0 || !opt_ok(t)) return vp8g::fail(EINVAL);
	const uint32_t eb = (uint32_t)elem_bytes(t->dtype), tpi = tpi_of(*t);
	uint64_t total = 0;
	bool ok = (uintptr_t)d_dst % eb == 0;
	for (uint32_t i = 0; ok && i < n; i++) {  // tasks must be numbered image by image
		ok = h[i].task0 == total && h[i].ntasks == tpi && h[i].dst % eb == 0 && desc_ok(i);
		total += tpi;
		if (total > 0x7FFFFFFFu) ok = false;
	}
	if (!ok) return vp8g::fail(EINVAL);
	TensorParams P;
	memset(&P, 0, sizeof(P));
	P.w = t->width, P.h = t->height, P.cw = (t->width + 1u) / 2u, P.ch = (t->height + 1u) / 2u;
	P.cpr = (t->width + kChunk - 1u) / kChunk, P.chunks = P.cpr * t->height, P.tpi = tpi;
	P.plane = (uint64_t)t->width * t->height * eb;
	for (int c = 0; c < 3; c++) P.scale[c] = t->scale[c], P.bias[c] = t->bias[c];
	return vp8g::gated_launch((hipStream_t)stream, "tensor launch", [&] {
		hipLaunchKernelGGL(table[t->dtype][t->layout][t->flags & VP8G_T_BGR], dim3(vp8g::grid_for(total, 16u)), dim3(kThreads), 0,
		                   (hipStream_t)stream, args..., (uint32_t)total, P, d_src, (uint8_t*)d_dst);
		return hipGetLastError();
	});
}

bool strides_ok(const Vp8gTensorDesc& d, const Vp8gTensorOpt& t) { return d.stride_y >= t.width && d.stride_uv >= (t.width + 1u) / 2u; }
bool strides_ok_444(const Vp8gTensorDesc& d, const Vp8gTensorOpt& t) { return d.stride_y >= t.width && d.stride_uv >= t.width; }

}  // namespace

VP8G_API uint64_t vp8g_tensor_slot_size(const Vp8gTensorOpt* t) { return slot_size(t, 3); }

VP8G_API uint64_t vp8g_tensor_slot_size_a(const Vp8gTensorOpt* t) { return slot_size(t, 4); }

VP8G_API int vp8g_make_tensor_desc(const Vp8gTensorOpt* t, uint64_t src_y, uint64_t src_u, uint64_t src_v, uint32_t stride_y,
                                   uint32_t stride_uv, uint64_t dst_offset, uint32_t task0, Vp8gTensorDesc* d) {
	if (!d || !opt_ok(t) || stride_y < t->width || stride_uv < (t->width + 1u) / 2u || dst_offset % (uint64_t)elem_bytes(t->dtype))
		return vp8g::fail(EINVAL);
	memset(d, 0, sizeof(*d));
	d->src_y = src_y, d->src_u = src_u, d->src_v = src_v, d->dst = dst_offset;
	d->stride_y = stride_y, d->stride_uv = stride_uv;
	d->task0 = task0, d->ntasks = tasks_per_image(*t);
	return 0;
}

VP8G_API int vp8g_tensor_batch_device(const Vp8gTensorDesc* h, const Vp8gTensorDesc* d_descs, uint32_t n, const Vp8gTensorOpt* t,
                                      const uint8_t* d_src, void* d_dst, void* stream) {
	return launch_tensor(
	    d_descs != nullptr, h, n, t, tasks_per_image, d_src, d_dst, stream, [&](uint32_t i) { return strides_ok(h[i], *t); }, kKernels[0],
	    d_descs, (const Vp8gTensorAlpha*)nullptr);
}

VP8G_API int vp8g_tensor_batch_device_a(const Vp8gTensorDesc* h, const Vp8gTensorDesc* d_descs, const Vp8gTensorAlpha* ha,
                                        const Vp8gTensorAlpha* d_alpha, uint32_t n, const Vp8gTensorOpt* t, const uint8_t* d_src,
                                        void* d_dst, void* stream) {
	return launch_tensor(
	    d_descs && ha && d_alpha, h, n, t, tasks_per_image, d_src, d_dst, stream,
	    [&](uint32_t i) { return strides_ok(h[i], *t) && (ha[i].src_a == VP8G_T_OPAQUE || ha[i].stride_a >= t->width); },
	    kKernels[1], d_descs, d_alpha);
}

// 4:4:4 planes (vp8g_make_scale_desc_444's output): the descriptor is vp8g_make_tensor_desc's but for the chroma stride
VP8G_API int vp8g_make_tensor_desc_444(const Vp8gTensorOpt* t, uint64_t src_y, uint64_t src_u, uint64_t src_v, uint32_t stride_y,
                                       uint32_t stride_uv, uint64_t dst_offset, uint32_t task0, Vp8gTensorDesc* d) {
	if (!opt_ok(t) || stride_uv < t->width) return vp8g::fail(EINVAL);
	return vp8g_make_tensor_desc(t, src_y, src_u, src_v, stride_y, stride_uv, dst_offset, task0, d);
}

VP8G_API int vp8g_tensor_batch_device_444(const Vp8gTensorDesc* h, const Vp8gTensorDesc* d_descs, const Vp8gTensorAlpha* ha,
                                          const Vp8gTensorAlpha* d_alpha, uint32_t n, const Vp8gTensorOpt* t, uint32_t channels,
                                          const uint8_t* d_src, void* d_dst, void* stream) {
	const bool with_a = channels == 4u;  // (3: both alpha arrays NULL; 4: both given)
	return launch_tensor(
	    d_descs && (channels == 3u || with_a) && (ha != nullptr) == with_a && (d_alpha != nullptr) == with_a, h, n, t, tasks_per_image, d_src,
	    d_dst, stream,
	    [&](uint32_t i) { return strides_ok_444(h[i], *t) && (!with_a || ha[i].src_a == VP8G_T_OPAQUE || ha[i].stride_a >= t->width); },
	    kKernels444[with_a], d_descs, d_alpha);
}

VP8G_API int vp8g_make_tensor_argb_desc(const Vp8gTensorOpt* t, uint32_t channels, uint64_t src, uint64_t dst_offset, uint32_t task0,
                                        Vp8gTensorArgbDesc* d) {
	if (!d || !opt_ok(t) || (channels != 3 && channels != 4) || src % 4u || dst_offset % (uint64_t)elem_bytes(t->dtype))
		return vp8g::fail(EINVAL);
	memset(d, 0, sizeof(*d));
	d->src = src, d->dst = dst_offset, d->task0 = task0, d->ntasks = argb_tasks_per_image(*t);
	return 0;
}

VP8G_API int vp8g_tensor_batch_device_argb(const Vp8gTensorArgbDesc* h, const Vp8gTensorArgbDesc* d_descs, uint32_t n,
                                           const Vp8gTensorOpt* t, uint32_t channels, const uint8_t* d_src, void* d_dst, void* stream) {
	return launch_tensor(
	    d_descs && (channels == 3 || channels == 4) && (uintptr_t)d_src % 4u == 0, h, n, t, argb_tasks_per_image, d_src, d_dst, stream,
	    [&](uint32_t i) { return h[i].src % 4u == 0; }, kKernelsArgb[channels == 4u], d_descs);
}
