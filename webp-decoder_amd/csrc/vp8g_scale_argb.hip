// vp8g_scale_argb.hip -- crop + rescale of ARGB pictures (lossless files) on the device, bit-exact to libwebp 1.2.2's
// decoder options on a VP8L image (include/vp8g.h: vp8g_scale_argb_batch_device; host restatement vp8f_argb_scale in
// host/vp8_scale.c).
//
// libwebp rescales such a picture as four interleaved byte channels, each with exactly the arithmetic of the
// single-plane rescaler (vp8g_scale.hip), between an alpha premultiply and its inverse.  So the picture takes the
// planar route through that rescaler, and the two kernels here are the passes around it:
//
//   split   the window of the ARGB source -> four byte planes (B, G, R, A: the dword's byte order) in the work buffer,
//           premultiplied on the way.  A thread takes four consecutive window pixels: one 16-byte load (the source is
//           only dword-aligned: the window's origin may be odd), one dword store per plane.  The last group of a row
//           loads its pixels one by one, and its dwords' spare bytes fall into the row's padding (the plane stride is a
//           multiple of 16, so that the rescaler's 16-byte staging loads are aligned).
//   scale   vp8g_scale_batch_device over four single-plane descriptors per picture (vp8g_make_scale_desc_plane's kind:
//           scale_kernel, and expand_kernel for a plane that grows), work buffer -> work buffer.  Those kernels read
//           their descriptors as one array, so the first task of every picture's split copies the picture's four to the
//           head of the work buffer.
//   merge   four scaled planes -> 0xAARRGGBB, un-premultiplied: a dword load per plane, one 16-byte store of four pixels.
//
// A crop without a target size is libwebp's plain copy of the window (no premultiply round trip): the split
// kernel writes such a picture's pixels straight to the output, and it has no planes and no other tasks.
// Tasks are numbered picture by picture, as in the rescaler; a task is kTaskGroups groups of four pixels.
#include <errno.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../host/vp8_front.h"
#include "vp8g_device.h"
#include "vp8g_scale_device.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vp8g_scale;  // premultiply, unpremultiply, task_owner (vp8g_scale_device.h)

constexpr uint32_t kPerThread = 4;                       // groups of four pixels per thread
constexpr uint32_t kTaskGroups = kThreads * kPerThread;  // ... and per task
constexpr uint32_t kPlaneDwords = 4u * sizeof(Vp8gScaleDesc) / 4u;
// (no padding: desc_ok compares descriptors byte for byte)
static_assert(sizeof(Vp8gScaleArgbDesc) == 4 * 8 + 20 * 4 + 4 * sizeof(Vp8gScaleDesc) && sizeof(Vp8gScaleDesc) == 272, "descriptor layout");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));  // four pixels at a dword-aligned address

__global__ __launch_bounds__(kThreads) void argb_split_kernel(const Vp8gScaleArgbDesc* __restrict__ descs, uint32_t n,
                                                              const uint8_t* __restrict__ src, uint8_t* __restrict__ work,
                                                              uint8_t* __restrict__ dst) {
	const uint32_t task = blockIdx.x, tid = threadIdx.x;
	const uint32_t im = task_owner<Vp8gScaleArgbDesc, &Vp8gScaleArgbDesc::split_task0>(descs, n, task);
	const Vp8gScaleArgbDesc& D = descs[im];
	const uint32_t t = task - D.split_task0;
	if (task < D.split_task0 || t >= D.split_ntasks) return;
	if (t == 0 && D.nplanes) {  // the rescaler's descriptors of this picture, to their place in the array it reads
		const uint32_t* const s = (const uint32_t*)D.plane;
		uint32_t* const d = (uint32_t*)work + (size_t)D.plane0 * (sizeof(Vp8gScaleDesc) / 4u);
		for (uint32_t k = tid; k < kPlaneDwords; k += kThreads) d[k] = s[k];
	}
	const uint32_t W = D.win_w, gpr = (W + 3u) >> 2, total = gpr * D.win_h;  // groups per row; of the window (< 2^26)
	const uint32_t* const win = (const uint32_t*)(src + D.src) + (size_t)D.crop_top * D.src_width + D.crop_left;
	uint32_t p[kPerThread][4], gy[kPerThread], gx[kPerThread];
#pragma unroll
	for (uint32_t it = 0; it < kPerThread; it++) {  // every load first: they are in flight together
		const uint32_t g = (t * kPerThread + it) * kThreads + tid;
		gy[it] = g / gpr, gx[it] = (g - gy[it] * gpr) << 2;
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++) p[it][q] = 0u;
		if (g >= total) continue;
		const uint32_t* const in = win + (size_t)gy[it] * D.src_width + gx[it];  // (row < win_h, columns < win_w: inside the window)
		if (gx[it] + 4u <= W) {
			const u32x4 v = *(const u32x4*)in;
			p[it][0] = v.x, p[it][1] = v.y, p[it][2] = v.z, p[it][3] = v.w;
		} else {
#pragma unroll
			for (uint32_t q = 0; q < 3u; q++)
				if (gx[it] + q < W) p[it][q] = in[q];
		}
	}
	const uint64_t pbytes = (uint64_t)D.plane_stride * D.win_h;
#pragma unroll
	for (uint32_t it = 0; it < kPerThread; it++) {
		const uint32_t g = (t * kPerThread + it) * kThreads + tid;
		if (g >= total) continue;
		if (!D.nplanes) {  // crop only: the window's pixels as they are
			uint32_t* const o = (uint32_t*)(dst + D.dst) + (size_t)gy[it] * W + gx[it];
			if (gx[it] + 4u <= W) {
				*(u32x4*)o = u32x4{p[it][0], p[it][1], p[it][2], p[it][3]};
			} else {
#pragma unroll
				for (uint32_t q = 0; q < 3u; q++)
					if (gx[it] + q < W) o[q] = p[it][q];
			}
			continue;
		}
		uint32_t m[4];
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++) m[q] = premultiply(p[it][q]);
		// (gx + 3 < plane_stride: the stride is win_w rounded up to 16)
		uint8_t* const o = work + D.work + (size_t)gy[it] * D.plane_stride + gx[it];
#pragma unroll
		for (uint32_t c = 0; c < 4u; c++) {
			const uint32_t s = 8u * c;
			*(uint32_t*)(o + c * pbytes) =
			    ((m[0] >> s) & 255u) | ((m[1] >> s) & 255u) << 8 | ((m[2] >> s) & 255u) << 16 | ((m[3] >> s) & 255u) << 24;
		}
	}
}

__global__ __launch_bounds__(kThreads) void argb_merge_kernel(const Vp8gScaleArgbDesc* __restrict__ descs, uint32_t n,
                                                              const uint8_t* __restrict__ work, uint8_t* __restrict__ dst) {
	const uint32_t task = blockIdx.x, tid = threadIdx.x;
	const uint32_t im = task_owner<Vp8gScaleArgbDesc, &Vp8gScaleArgbDesc::merge_task0>(descs, n, task);
	const Vp8gScaleArgbDesc& D = descs[im];
	const uint32_t t = task - D.merge_task0;
	if (task < D.merge_task0 || t >= D.merge_ntasks) return;
	const uint32_t w = D.width, gpr = (w + 3u) >> 2, total = gpr * D.height;
	const uint64_t obytes = (uint64_t)D.out_stride * D.height;
	const uint8_t* const planes = work + D.work + 4u * (uint64_t)D.plane_stride * D.win_h;
	uint32_t c[kPerThread][4], gy[kPerThread], gx[kPerThread];
#pragma unroll
	for (uint32_t it = 0; it < kPerThread; it++) {
		const uint32_t g = (t * kPerThread + it) * kThreads + tid;
		gy[it] = g / gpr, gx[it] = (g - gy[it] * gpr) << 2;
#pragma unroll
		for (uint32_t ch = 0; ch < 4u; ch++) c[it][ch] = 0u;
		if (g >= total) continue;
		// (gx + 3 < out_stride: a row's last dword may end in the row's padding, whose bytes no pixel below uses)
		const uint8_t* const in = planes + (size_t)gy[it] * D.out_stride + gx[it];
#pragma unroll
		for (uint32_t ch = 0; ch < 4u; ch++) c[it][ch] = *(const uint32_t*)(in + ch * obytes);
	}
#pragma unroll
	for (uint32_t it = 0; it < kPerThread; it++) {
		const uint32_t g = (t * kPerThread + it) * kThreads + tid;
		if (g >= total) continue;
		uint32_t px[4];
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++) {
			const uint32_t s = 8u * q;
			px[q] = unpremultiply(((c[it][0] >> s) & 255u) | ((c[it][1] >> s) & 255u) << 8 | ((c[it][2] >> s) & 255u) << 16 |
			                      ((c[it][3] >> s) & 255u) << 24);
		}
		uint32_t* const o = (uint32_t*)(dst + D.dst) + (size_t)gy[it] * w + gx[it];
		if (gx[it] + 4u <= w) {
			*(u32x4*)o = u32x4{px[0], px[1], px[2], px[3]};
		} else {
#pragma unroll
			for (uint32_t q = 0; q < 3u; q++)
				if (gx[it] + q < w) o[q] = px[q];
		}
	}
}

inline uint32_t al16(uint32_t v) { return (v + 15u) & ~15u; }
inline uint32_t tasks_of(uint32_t w, uint32_t h) { return (((w + 3u) >> 2) * h + kTaskGroups - 1u) / kTaskGroups; }

// bytes of the work buffer a resolved picture needs: four window planes, four scaled planes (0: crop only)
uint64_t work_bytes(const Vp8fScaleGeom& g) {
	return g.scaling ? 4u * ((uint64_t)al16(g.win_w) * g.win_h + (uint64_t)al16(g.out_w) * g.out_h) : 0u;
}

int make_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t work, uint64_t dst, uint32_t plane0,
              uint32_t split_task0, uint32_t scale_task0, uint32_t merge_task0, Vp8gScaleArgbDesc* out) {
	Vp8fScaleGeom g;
	if (!out || vp8f_scale_resolve_argb(width, height, opt, &g) != 0 || src % 4u || work % 16u || dst % 4u) return vp8g::fail(EINVAL);
	Vp8gScaleArgbDesc d;
	memset(&d, 0, sizeof(d));
	d.src = src, d.work = work, d.dst = dst;
	d.width = g.out_w, d.height = g.out_h, d.src_width = width, d.src_height = height;
	d.crop_left = g.left, d.crop_top = g.top, d.win_w = g.win_w, d.win_h = g.win_h;
	d.plane0 = plane0, d.split_task0 = split_task0, d.scale_task0 = scale_task0, d.merge_task0 = merge_task0;
	d.split_ntasks = tasks_of(g.win_w, g.win_h);
	if (g.scaling) {
		d.nplanes = 4;
		d.plane_stride = al16(g.win_w), d.out_stride = al16(g.out_w);
		d.merge_ntasks = tasks_of(g.out_w, g.out_h);
		const uint64_t pb = (uint64_t)d.plane_stride * g.win_h, ob = (uint64_t)d.out_stride * g.out_h;
		const Vp8gScaleOpt whole = {0, 0, 0, 0, g.out_w, g.out_h, VP8G_SCALE_EXPAND};  // the plane is the window already
		for (uint32_t c = 0; c < 4u; c++) {
			if (vp8g_make_scale_desc_plane(g.win_w, g.win_h, work + c * pb, d.plane_stride, &whole, work + 4u * pb + c * ob,
			                               scale_task0 + d.scale_ntasks, &d.plane[c]) != 0)
				return -1;  // (never: the target was resolved above)
			d.plane[c].p[0].dst_stride = d.out_stride;
			d.scale_ntasks += d.plane[c].ntasks;
		}
	}
	d.work_bytes = work_bytes(g);
	*out = d;
	return 0;
}

// exactly what make_desc gives for the picture, window and target the descriptor names
bool desc_ok(const Vp8gScaleArgbDesc& d) {
	if (d.nplanes != 0 && d.nplanes != 4) return false;
	const Vp8gScaleOpt o = {d.crop_left, d.crop_top, d.win_w, d.win_h, d.nplanes ? d.width : 0u, d.nplanes ? d.height : 0u,
	                        VP8G_SCALE_EXPAND};
	Vp8gScaleArgbDesc m;
	return make_desc(d.src_width, d.src_height, d.src, &o, d.work, d.dst, d.plane0, d.split_task0, d.scale_task0, d.merge_task0, &m) == 0 &&
	       memcmp(&m, &d, sizeof(d)) == 0;
}

}  // namespace

VP8G_API uint64_t vp8g_scale_argb_work_size(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt) {
	Vp8fScaleGeom g;
	if (vp8f_scale_resolve_argb(width, height, opt, &g) != 0) return errno = EINVAL, 0u;
	return work_bytes(g);
}

VP8G_API uint64_t vp8g_scale_argb_head_size(uint32_t n) { return ((uint64_t)n * 4u * sizeof(Vp8gScaleDesc) + 255u) & ~(uint64_t)255u; }

VP8G_API int vp8g_make_scale_argb_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t work_offset,
                                       uint64_t dst_offset, uint32_t plane0, uint32_t split_task0, uint32_t scale_task0,
                                       uint32_t merge_task0, Vp8gScaleArgbDesc* out) {
	return make_desc(width, height, src, opt, work_offset, dst_offset, plane0, split_task0, scale_task0, merge_task0, out);
}

VP8G_API int vp8g_scale_argb_batch_device(const Vp8gScaleArgbDesc* h, const Vp8gScaleArgbDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                          uint8_t* d_work, uint8_t* d_dst, void* stream) {
	if (!h || !d_descs || !d_src || !d_work || !d_dst || n == 0 || n > 0x7FFFFFFFu / 4u || (uintptr_t)d_src % 4u || (uintptr_t)d_work % 16u ||
	    (uintptr_t)d_dst % 4u)
		return vp8g::fail(EINVAL);
	uint64_t planes = 0, split = 0, scale = 0, merge = 0;
	const uint64_t head = vp8g_scale_argb_head_size(n);
	std::vector<Vp8gScaleDesc> sd;  // the rescaler's host copies
	try {
		std::vector<uint32_t> by_work;
		for (uint32_t i = 0; i < n; i++) {
			const Vp8gScaleArgbDesc& d = h[i];
			if (d.plane0 != planes || d.split_task0 != split || d.scale_task0 != scale || d.merge_task0 != merge || !desc_ok(d) ||
			    (d.nplanes && d.work < head))  // tasks and planes must be numbered picture by picture
				return vp8g::fail(EINVAL);
			planes += d.nplanes, split += d.split_ntasks, scale += d.scale_ntasks, merge += d.merge_ntasks;
			if (split > 0x7FFFFFFFu || scale > 0x7FFFFFFFu || merge > 0x7FFFFFFFu) return vp8g::fail(EINVAL);
			if (d.nplanes) sd.insert(sd.end(), d.plane, d.plane + 4), by_work.push_back(i);
		}
		// no two pictures' planes may share bytes of the work buffer
		std::sort(by_work.begin(), by_work.end(), [&](uint32_t a, uint32_t b) { return h[a].work < h[b].work; });
		for (size_t k = 1; k < by_work.size(); k++)
			if (h[by_work[k - 1]].work + h[by_work[k - 1]].work_bytes > h[by_work[k]].work) return vp8g::fail(EINVAL);
	} catch (const std::bad_alloc&) {
		return vp8g::fail(ENOMEM);
	}
	hipStream_t s = (hipStream_t)stream;
	int rc = vp8g::gated_launch(s, "argb split launch", [&] {
		hipLaunchKernelGGL(argb_split_kernel, dim3((uint32_t)split), dim3(kThreads), 0, s, d_descs, n, d_src, d_work, d_dst);
		return hipGetLastError();
	});
	if (rc != 0 || planes == 0) return rc;
	rc = vp8g_scale_batch_device(sd.data(), (const Vp8gScaleDesc*)d_work, (uint32_t)planes, d_work, d_work, s);
	if (rc != 0) return rc;
	return vp8g::gated_launch(s, "argb merge launch", [&] {
		hipLaunchKernelGGL(argb_merge_kernel, dim3((uint32_t)merge), dim3(kThreads), 0, s, d_descs, n, (const uint8_t*)d_work, d_dst);
		return hipGetLastError();
	});
}
