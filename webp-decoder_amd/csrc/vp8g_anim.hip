// vp8g_anim.hip -- the compositor of animated files: frames (tight 0xAARRGGBB pictures on the device) -> every
// canvas of every animation, as elements of a dense tensor (include/vp8g.h: vp8g_anim_compose_batch_device and
// the end-to-end vp8g_decode_webp_anim_tensor and vp8g_decode_webp_anim_tensor_scaled, which composes at full size
// into a staging buffer and rescales from there: vp8g_scale_argb_fused.hip).  The rules are
// libwebp's WebPAnimDecoder, restated sequentially in host/vp8_anim.c.
//
// Frames depend on each other, pixels do not.  A thread owns kPx adjacent pixels of one canvas row and keeps their
// canvas values in registers while it walks a segment -- the frames from one key frame (an empty canvas) up to the
// next: per frame it reads its pixels of the frame's rectangle (one 16-byte load when all four lie inside), blends
// or overwrites, converts the four pixels to the element type (conv / conv_a of vp8g_tensor_device.h, only when one
// of them changed) and stores them into that frame's canvas, then clears what the frame's disposal clears.  The
// canvas itself is never in memory: F frames on a W x H canvas read every frame pixel once and write F * W * H
// pixels once.
// A workgroup task is (segment, tile): 256 consecutive four-pixel pieces of the canvas in row-major order, for one
// segment; segments are independent, so a long animation on a small canvas still spreads over the device.  The
// frame records are the same for every thread of a task and are read with wave-uniform addresses (scalar loads).
// No LDS, no barriers, no workgroup waits on another, nothing spins on memory.
#include <errno.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "vp8g_argb_batch.h"
#include "vp8g_device.h"
#include "vp8g_tensor_device.h"
#include "../host/vp8_front.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))
#define DEV __device__ __forceinline__

namespace {

using namespace vp8g_tensor;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPx = 4;  // adjacent pixels of a row per thread
constexpr uint32_t kMaxDim = 16383;
constexpr uint32_t kInFlags = VP8G_ANIM_BLEND | VP8G_ANIM_DISPOSE | VP8G_ANIM_HAS_ALPHA;

struct AnimParams {
	float scale[3], bias[3];
};

// libwebp's non-premultiplied blend of source pixel s over canvas pixel d (host/vp8_anim.c: blend_pixel)
DEV uint32_t blend_pixel(uint32_t s, uint32_t d) {
	const uint32_t sa = s >> 24;
	if (sa == 255u) return s;
	if (sa == 0u) return d;
	const uint32_t dfa = ((d >> 24) * (256u - sa)) >> 8;
	const uint32_t ba = sa + dfa;  // 1 .. 255
	const uint32_t scale = (1u << 24) / ba;
	uint32_t out = ba << 24;
#pragma unroll
	for (int sh = 0; sh < 24; sh += 8) out |= (((((s >> sh) & 255u) * sa + ((d >> sh) & 255u) * dfa) * scale) >> 24) << sh;
	return out;
}

template <uint32_t DT, bool PLANAR, bool BGR, int C>
__global__ __launch_bounds__(kThreads) void anim_kernel(const Vp8gAnimDesc* __restrict__ D, uint32_t n, uint32_t total, AnimParams P,
                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
	static_assert(C == 3 || C == 4, "RGB, or RGB and alpha");
	constexpr uint32_t EB = (uint32_t)elem_bytes(DT);
	const uint32_t tid = threadIdx.x;
	for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
		// the animation of task g: the last one whose task0 is not beyond it (tasks are numbered animation by animation)
		uint32_t lo = 0, hi = n;
		while (hi - lo > 1u) {
			const uint32_t mid = (lo + hi) >> 1;
			if (D[mid].task0 <= g) lo = mid;
			else hi = mid;
		}
		const Vp8gAnimDesc& d = D[lo];
		const uint32_t W = d.width, H = d.height;
		const uint32_t cpr = (W + kPx - 1u) / kPx, pieces = cpr * H, tpc = (pieces + kThreads - 1u) / kThreads;
		const uint32_t t = g - d.task0, seg = t / tpc;
		const uint32_t gc = (t - seg * tpc) * kThreads + tid;
		if (gc >= pieces) continue;
		const uint32_t y = gc / cpr, x0 = (gc - y * cpr) * kPx;
		const uint32_t cnt = min(kPx, W - x0);
		const Vp8gAnimFrame* const R = (const Vp8gAnimFrame*)(src + d.frames);
		const uint32_t f0 = R[seg].seg_first, f1 = R[seg].seg_end;
		const uint64_t plane = (uint64_t)W * H * EB;  // one NCHW plane; a canvas is C of them
		const size_t pix = (size_t)y * W + x0;        // the piece's first pixel in the canvas
		uint32_t c[kPx] = {0u, 0u, 0u, 0u};           // the canvas under this thread, after the last frame's disposal
		uint32_t e[kPx][4];
		uint32_t cleared = 0;  // bit j: the previous frame's disposal has just cleared pixel j
		for (uint32_t k = f0; k < f1; k++) {
			const Vp8gAnimFrame& r = R[k];
			const uint32_t ry = y - r.y, rx = x0 - r.x;  // (unsigned: a pixel left of / above the rectangle compares as beyond it)
			uint32_t m = 0;  // bit j: pixel j lies in the frame's rectangle
			if (ry < r.height) {
#pragma unroll
				for (uint32_t j = 0; j < kPx; j++) m |= (rx + j < r.width ? 1u : 0u) << j;
			}
			if (m) {
				const uint32_t* const row = (const uint32_t*)(src + r.src) + (size_t)ry * r.width;
				uint32_t s[kPx] = {0u, 0u, 0u, 0u};
				if (m == 15u) {
					const u32x4a v = *(const u32x4a*)(row + rx);
					s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
				} else {
#pragma unroll
					for (uint32_t j = 0; j < kPx; j++)
						if ((m >> j) & 1u) s[j] = row[rx + j];
				}
				// blended only where the frame blends, is no key frame (k != f0: a segment starts at its only key frame)
				// and the canvas below was not just cleared
				const bool blends = (r.flags & VP8G_ANIM_BLEND) && k != f0;
#pragma unroll
				for (uint32_t j = 0; j < kPx; j++)
					if ((m >> j) & 1u) c[j] = (blends && !((cleared >> j) & 1u)) ? blend_pixel(s[j], c[j]) : s[j];
			}
			if (k == f0 || m || cleared) {
#pragma unroll
				for (uint32_t j = 0; j < kPx; j++) {
					// (channel<> reads r | g << 8 | b << 16)
					const uint32_t rgb = ((c[j] >> 16) & 255u) | (c[j] & 0xFF00u) | ((c[j] & 255u) << 16);
#pragma unroll
					for (int q = 0; q < 3; q++) e[j][q] = conv<DT>(channel<BGR>(rgb, q), P.scale[q], P.bias[q]);
					e[j][3] = conv_a<DT>(c[j] >> 24);
				}
			}
			uint8_t* const out = dst + d.dst + (uint64_t)k * C * plane;
			if (cnt == kPx) {
				if constexpr (PLANAR) {
#pragma unroll
					for (int q = 0; q < C; q++) {
						const uint32_t run[kPx] = {e[0][q], e[1][q], e[2][q], e[3][q]};
						store_run<DT, (int)kPx>(out + (size_t)q * plane + pix * EB, run);
					}
				} else {
					uint32_t run[kPx * C];
#pragma unroll
					for (int j = 0; j < (int)kPx; j++)
#pragma unroll
						for (int q = 0; q < C; q++) run[C * j + q] = e[j][q];
					store_run<DT, (int)kPx * C>(out + pix * C * EB, run);
				}
			} else {
				// a row's last, partial piece: element by element
#pragma unroll
				for (uint32_t j = 0; j < kPx - 1u; j++)
					if (j < cnt)
#pragma unroll
						for (int q = 0; q < C; q++) {
							uint8_t* p = PLANAR ? out + (size_t)q * plane + (pix + j) * EB : out + ((pix + j) * C + (uint32_t)q) * EB;
							store_elem<DT>(p, e[j][q]);
						}
			}
			cleared = (r.flags & VP8G_ANIM_DISPOSE) ? m : 0u;
#pragma unroll
			for (uint32_t j = 0; j < kPx; j++)
				if ((cleared >> j) & 1u) c[j] = 0u;
		}
	}
}

using KernelFn = void (*)(const Vp8gAnimDesc*, uint32_t, uint32_t, AnimParams, const uint8_t*, uint8_t*);
// [C - 3][dtype][layout][bgr]
#define VP8G_A_ROW(DT, C) { {anim_kernel<DT, false, false, C>, anim_kernel<DT, false, true, C>}, {anim_kernel<DT, true, false, C>, anim_kernel<DT, true, true, C>} }
const KernelFn kKernels[2][4][2][2] = {{VP8G_A_ROW(VP8G_T_U8, 3), VP8G_A_ROW(VP8G_T_F16, 3), VP8G_A_ROW(VP8G_T_BF16, 3), VP8G_A_ROW(VP8G_T_F32, 3)},
                                       {VP8G_A_ROW(VP8G_T_U8, 4), VP8G_A_ROW(VP8G_T_F16, 4), VP8G_A_ROW(VP8G_T_BF16, 4), VP8G_A_ROW(VP8G_T_F32, 4)}};
#undef VP8G_A_ROW

uint32_t tiles_of(uint32_t w, uint32_t h) { return (((w + kPx - 1u) / kPx) * h + kThreads - 1u) / kThreads; }

bool full(const Vp8gAnimFrame& f, uint32_t w, uint32_t h) { return f.width == w && f.height == h; }

// libwebp's key-frame rule for frame k, given the frames before it with their VP8G_ANIM_KEY set
bool is_key(const Vp8gAnimFrame* f, uint32_t k, uint32_t w, uint32_t h) {
	if (k == 0) return true;
	const Vp8gAnimFrame &c = f[k], &p = f[k - 1];
	if ((!(c.flags & VP8G_ANIM_HAS_ALPHA) || !(c.flags & VP8G_ANIM_BLEND)) && full(c, w, h)) return true;
	return (p.flags & VP8G_ANIM_DISPOSE) && (full(p, w, h) || (p.flags & VP8G_ANIM_KEY));
}

bool rect_ok(const Vp8gAnimFrame& f, uint32_t w, uint32_t h) {
	return f.width >= 1 && f.height >= 1 && f.x <= w && f.y <= h && f.width <= w - f.x && f.height <= h - f.y && !(f.x & 1u) && !(f.y & 1u) &&
	       f.src % 4u == 0;
}

// A descriptor and its host records as vp8g_make_anim_desc leaves them.
bool desc_ok(const Vp8gAnimDesc& d) {
	if (!d.h_frames || d.width < 1 || d.height < 1 || d.width > kMaxDim || d.height > kMaxDim || d.nframes < 1 || d.frames % 8u) return false;
	const Vp8gAnimFrame* f = d.h_frames;
	uint32_t segs = 0;
	for (uint32_t k = 0; k < d.nframes; k++) {
		if (!rect_ok(f[k], d.width, d.height) || (f[k].flags & ~(kInFlags | VP8G_ANIM_KEY))) return false;
		const bool key = is_key(f, k, d.width, d.height);
		if (key != ((f[k].flags & VP8G_ANIM_KEY) != 0)) return false;
		if (key) {
			if (segs && f[segs - 1].seg_end != k) return false;
			if (f[segs].seg_first != k) return false;
			segs++;
		}
	}
	return f[segs - 1].seg_end == d.nframes && d.nsegs == segs && (uint64_t)segs * tiles_of(d.width, d.height) == d.ntasks;
}

}  // namespace

// (tests/test_gpu_anim.py takes its boundary sizes from here, through vp8g.anim_geometry())
VP8G_API void vp8g_anim_geometry(uint32_t out[3]) { out[0] = kPx, out[1] = kPx * kThreads, out[2] = 0u; }

VP8G_API int vp8g_make_anim_desc(uint32_t width, uint32_t height, Vp8gAnimFrame* frames, uint32_t nframes, uint64_t frames_offset,
                                 uint64_t dst_offset, uint32_t task0, Vp8gAnimDesc* out) {
	if (!out || !frames || nframes == 0 || width < 1 || height < 1 || width > kMaxDim || height > kMaxDim || frames_offset % 8u)
		return vp8g::fail(EINVAL);
	for (uint32_t k = 0; k < nframes; k++)
		if (!rect_ok(frames[k], width, height) || (frames[k].flags & ~kInFlags)) return vp8g::fail(EINVAL);
	uint32_t segs = 0;
	for (uint32_t k = 0; k < nframes; k++) {
		frames[k].seg_first = frames[k].seg_end = frames[k].reserved = 0;
		if (!is_key(frames, k, width, height)) continue;
		frames[k].flags |= VP8G_ANIM_KEY;
		if (segs) frames[segs - 1].seg_end = k;  // (record s < k is complete by now: s <= its segment's first frame)
		frames[segs++].seg_first = k;
	}
	frames[segs - 1].seg_end = nframes;
	const uint64_t ntasks = (uint64_t)segs * tiles_of(width, height);
	if (ntasks + task0 > 0x7FFFFFFFu) return vp8g::fail(EINVAL);
	memset(out, 0, sizeof(*out));
	out->frames = frames_offset, out->h_frames = frames, out->dst = dst_offset;
	out->width = width, out->height = height, out->nframes = nframes, out->nsegs = segs;
	out->task0 = task0, out->ntasks = (uint32_t)ntasks;
	return 0;
}

VP8G_API int vp8g_anim_compose_batch_device(const Vp8gAnimDesc* h, const Vp8gAnimDesc* d_descs, uint32_t n, const Vp8gTensorOpt* t,
                                            uint32_t channels, const uint8_t* d_src, void* d_dst, void* stream) {
	if (!h || !d_descs || !d_src || !d_dst || n == 0 || (channels != 3 && channels != 4) || !vp8g_tensor_slot_size(t) ||
	    (uintptr_t)d_src % 8u)
		return vp8g::fail(EINVAL);
	const uint32_t eb = (uint32_t)elem_bytes(t->dtype);
	uint64_t total = 0, dst_end = 0;
	bool ok = (uintptr_t)d_dst % eb == 0;
	for (uint32_t i = 0; ok && i < n; i++) {  // tasks numbered animation by animation, canvases laid out in order
		ok = desc_ok(h[i]) && h[i].task0 == total && h[i].dst % eb == 0 && h[i].dst >= dst_end;
		total += h[i].ntasks;
		dst_end = h[i].dst + (uint64_t)h[i].nframes * channels * h[i].width * h[i].height * eb;
		if (total > 0x7FFFFFFFu) ok = false;
	}
	if (!ok) return vp8g::fail(EINVAL);
	AnimParams P;
	for (int c = 0; c < 3; c++) P.scale[c] = t->scale[c], P.bias[c] = t->bias[c];
	return vp8g::gated_launch((hipStream_t)stream, "anim launch", [&] {
		hipLaunchKernelGGL(kKernels[channels == 4u][t->dtype][t->layout][t->flags & VP8G_T_BGR], dim3(vp8g::grid_for(total, 8u)), dim3(kThreads), 0,
		                   (hipStream_t)stream, d_descs, n, (uint32_t)total, P, d_src, (uint8_t*)d_dst);
		return hipGetLastError();
	});
}

// ---- end to end ------------------------------------------------------------------------------

namespace {

using vp8g::al256;
using vp8g::ArgbScaleBatch;
using vp8g::Status;

// One frame as the still picture the pipeline decodes: its payloads where webp_parse_anim located them.
WebPStill still_of(const uint8_t* file, const WebPAnimFrame& f) {
	const auto chunk = [](uint32_t payload) { return 8u + (size_t)payload + (payload & 1u); };
	WebPStill s;
	memset(&s, 0, sizeof(s));
	s.data = file;
	s.vp8_offset = f.vp8_offset, s.vp8_size = f.vp8_size, s.alph_offset = f.alph_offset, s.alph_size = f.alph_size;
	s.vp8l_offset = f.vp8l_offset, s.vp8l_size = f.vp8l_size;
	s.width = f.width, s.height = f.height;
	// the planner's price: the frame as a file of its own -- RIFF header, VP8X chunk in front of an ALPH, the frame's chunks
	s.size = 12u + (f.alph_offset ? 18u + chunk(f.alph_size) : 0u) + chunk(f.vp8l_offset ? f.vp8l_size : f.vp8_size);
	return s;
}

int fail_all(int* status, uint32_t n, int e) {
	for (uint32_t i = 0; status && i < n; i++) status[i] = e;
	return vp8g::fail(e);
}

// How a file's canvases reach the tensor (vp8g_decode_webp_anim_tensor_scaled).
enum Route {
	kDirect,  // composed straight into the tensor: the identity on a canvas of the tensor's size
	kFused,   // composed into the staging buffer, then vp8g_scale_argb_tensor_batch_device
	kPlanar,  // ... then vp8g_scale_argb_batch_device and vp8g_tensor_batch_device_argb (what the fused maker answers ENOTSUP for)
};

constexpr uint64_t kStageDefault = 256ull << 20;  // canvas bytes per staging group when the caller gives 0

// The route of a cw x ch canvas under `o` into t's size, or -1 (EINVAL): an option that does not fit the canvas or
// whose result is not the tensor's size.
int route_of(uint32_t cw, uint32_t ch, const Vp8gScaleOpt& o, const Vp8gTensorOpt& t) {
	Vp8fScaleGeom g;
	if (vp8f_scale_resolve_argb(cw, ch, &o, &g) != 0 || g.out_w != t.width || g.out_h != t.height) return -1;
	if (!g.scaling && g.left == 0 && g.top == 0 && g.win_w == cw && g.win_h == ch) return kDirect;
	Vp8gScaleArgbTensorDesc d;
	if (vp8g_make_scale_argb_tensor_desc(cw, ch, 0, &o, 0, 0, &d) == 0) return kFused;
	return errno == ENOTSUP ? kPlanar : -1;
}

// A tensor of tight 0xAARRGGBB pictures: B, G, R, A bytes.
Vp8gTensorOpt argb_tensor(uint32_t w, uint32_t h) {
	Vp8gTensorOpt o;
	memset(&o, 0, sizeof(o));
	o.width = w, o.height = h, o.dtype = VP8G_T_U8, o.layout = VP8G_T_NHWC, o.flags = VP8G_T_BGR;
	return o;
}

// One call of vp8g_decode_webp_anim_tensor_scaled (n_opts = 0: of vp8g_decode_webp_anim_tensor, every file kDirect and no
// staging) and the stages it goes through, in the order of run().  It owns the call's host tables and device buffers, and
// everything it enqueues goes onto the null stream.  A stage returns 0 or the errno with which the call fails as a
// whole -- a refused descriptor, a device error; a C++ exception passes through to the entry point -- and every one of
// these leaves, like a finished call, through the destructor.
struct AnimCall {
	const ByteSpan* files;
	uint32_t n;
	int filtered;
	uint32_t threads, flags;
	const Vp8gScaleOpt* opts;
	uint32_t n_opts;
	uint64_t stage_bytes;
	const Vp8gTensorOpt* t;
	uint32_t channels;
	uint8_t* d_out;
	uint32_t* timestamps;

	struct File {
		WebPAnimInfo info;
		std::vector<WebPAnimFrame> fr;
		uint32_t first = 0;  // its first slot
		uint32_t ref0 = 0;   // its first frame in `refs` (files that parsed and have a route)
		uint32_t rec0 = 0;   // its first record in `recs` (files whose frames all decoded)
		int err = 0;
		int route = kDirect;
		Vp8gScaleOpt opt;    // (routes other than kDirect)
	};
	struct Ref {
		uint32_t file, frame;
		uint64_t src;  // of its picture in `buf`
	};
	struct Group {  // whole animations that share the staging buffer
		uint32_t q0, q1;  // its files: by_route[q0 .. q1)
		uint32_t nf, np;  // its canvases on the fused and on the planar route
		uint64_t o_fd, o_pd, o_td, o_sc, o_work, bytes;  // offsets in the staging buffer; canvases from 0
	};
	uint64_t slot = 0;                    // bytes per slot of the tensor
	std::vector<File> fs;
	std::vector<Ref> refs;                // every frame of the files still standing after parse_files ...
	std::vector<uint32_t> order;          // ... and their indices sorted by frame size: one decode call per size
	uint64_t rec_off = 0, desc_off = 0;   // `buf`: the frames' pictures from 0, then the records, then the descriptors
	std::vector<Vp8gAnimFrame> recs;
	std::vector<uint32_t> by_route;       // the files that compose: descriptor q belongs to file by_route[q], direct files first
	uint32_t ndirect = 0;
	std::vector<Vp8gAnimDesc> descs;
	std::vector<Group> groups;
	std::vector<Vp8gScaleArgbTensorDesc> fd;  // the group under way: its fused descriptors ...
	ArgbScaleBatch planar;              // ... and its planar batch
	uint8_t* buf = nullptr;               // device: frames, records, descriptors
	uint8_t* stg = nullptr;               // device: one group's full-size canvases, descriptors, scaled pictures, work area

	// The only way out.  The order matters: first the stream -- uploads from the vectors above and kernels on the two buffers
	// may still be in flight, whichever stage the call left from --, then the device buffers, and only after this body
	// the members, the host vectors among them.
	~AnimCall() {
		(void)hipStreamSynchronize(nullptr);
		if (stg) (void)hipFree(stg);
		if (buf) (void)hipFree(buf);
	}

	// 0, or EIO with the failed step recorded for vp8g_last_error
	static int io(const Status& s) {
		if (s.ok()) return 0;
		vp8g::set_error_text(s.where, s.he);
		return EIO;
	}
	static int dev_alloc(uint8_t** p, uint64_t bytes) {
		const hipError_t e = hipMalloc((void**)p, bytes);
		if (e == hipSuccess) return 0;
		(void)hipGetLastError();
		return e == hipErrorOutOfMemory ? ENOMEM : EIO;
	}
	Status upload(uint8_t* dst, const void* src, size_t bytes) const {
		return Status{hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, nullptr), "upload"};
	}
	const WebPAnimFrame& frame_of(uint32_t q) const { return fs[refs[q].file].fr[refs[q].frame]; }
	uint64_t size_of(uint32_t q) const { return ((uint64_t)frame_of(q).width << 32) | frame_of(q).height; }
	uint64_t canvas_bytes(const File& f) const { return 4ull * f.info.canvas_width * f.info.canvas_height; }
	Vp8gAnimDesc* d_descs() const { return (Vp8gAnimDesc*)(buf + desc_off); }

	// Parses the files, picks each one's route, writes the timestamps and numbers the slots; then lists the frames of the
	// files still standing.  A file that is no animation, or whose option or canvas does not suit the tensor, fails alone.
	int parse_files() {
		fs.resize(n);
		uint32_t slots = 0;
		for (uint32_t i = 0; i < n; i++) {
			File& f = fs[i];
			f.first = slots;
			if (webp_parse_anim(files[i], &f.info, nullptr, 0) != 0) {
				f.err = EINVAL;
				continue;
			}
			f.fr.resize(f.info.nframes);
			if (webp_parse_anim(files[i], &f.info, f.fr.data(), f.info.nframes) != 0) return EINVAL;  // (cannot differ)
			if (n_opts) {
				f.opt = opts[n_opts == 1u ? 0u : i];
				f.route = route_of(f.info.canvas_width, f.info.canvas_height, f.opt, *t);
				if (f.route < 0) f.err = EINVAL;
			} else if (f.info.canvas_width != t->width || f.info.canvas_height != t->height) {
				f.err = EINVAL;
			}
			uint32_t ts = 0;
			for (uint32_t k = 0; timestamps && k < f.info.nframes; k++) timestamps[slots + k] = ts += f.fr[k].duration;
			if ((uint64_t)slots + f.info.nframes > 0x7FFFFFFFu) return EINVAL;
			slots += f.info.nframes;
		}
		for (uint32_t i = 0; i < n; i++) {
			if (fs[i].err) continue;
			fs[i].ref0 = (uint32_t)refs.size();
			for (uint32_t k = 0; k < fs[i].info.nframes; k++) refs.push_back({i, k, 0});
		}
		return 0;
	}
	// The frames' place in `buf`: grouped by frame size, a group's pictures back to back (the slots of its decode call's
	// tensor); behind them the records and the descriptors.
	void layout_frames() {
		order.resize(refs.size());
		for (uint32_t q = 0; q < order.size(); q++) order[q] = q;
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return size_of(a) < size_of(b); });
		uint64_t stage = 0;
		for (size_t a = 0; a < order.size(); a++) {
			if (a && size_of(order[a]) != size_of(order[a - 1])) stage = al256(stage);
			refs[order[a]].src = stage;
			stage += 4ull * frame_of(order[a]).width * frame_of(order[a]).height;
		}
		rec_off = al256(stage), desc_off = al256(rec_off + refs.size() * sizeof(Vp8gAnimFrame));
	}
	// Every frame as a still picture of its own, one run of the still pipeline (vp8g::decode_located_tensor) per frame size,
	// into `buf`.  A frame
	// that does not decode fails its file; a call that fails without naming a frame, or for every frame with EIO, fails
	// this call.
	int decode_frames() {
		if (refs.empty()) return 0;
		if (int e = dev_alloc(&buf, desc_off + n * sizeof(Vp8gAnimDesc))) return e;
		for (size_t a = 0, b = 0; a < order.size(); a = b) {
			while (b < order.size() && size_of(order[b]) == size_of(order[a])) b++;
			std::vector<WebPStill> pics;
			for (size_t q = a; q < b; q++) pics.push_back(still_of(files[refs[order[q]].file].data, frame_of(order[q])));
			const Vp8gTensorOpt st = argb_tensor(frame_of(order[a]).width, frame_of(order[a]).height);
			std::vector<int> err(b - a, 0);
			const int rc = vp8g::decode_located_tensor(pics.data(), (uint32_t)(b - a), filtered, threads, flags, &st, VP8G_X_ALPHA | VP8G_X_LOSSLESS,
			                                           buf + refs[order[a]].src, err.data());
			const int en = errno;
			bool any = false, all_io = true;
			for (int e : err) any |= e != 0, all_io &= e == EIO;
			if (rc != 0 && (!any || all_io)) return en == EINVAL || en == ENOMEM ? en : EIO;
			for (size_t q = a; q < b; q++)
				if (err[q - a] && !fs[refs[order[q]].file].err) fs[refs[order[q]].file].err = err[q - a];
		}
		return 0;
	}
	// Descriptor q, of file by_route[q] on a w x h canvas: vp8g_make_anim_desc, which also completes the file's records.
	int make_desc(uint32_t q, uint32_t w, uint32_t h, uint64_t dst, uint32_t task0) {
		const File& f = fs[by_route[q]];
		return vp8g_make_anim_desc(w, h, recs.data() + f.rec0, f.info.nframes, rec_off + f.rec0 * sizeof(Vp8gAnimFrame), dst, task0, &descs[q]);
	}
	// The files whose frames all decoded: their records, their order in the descriptor array (the files composed straight
	// into the tensor first, then the others in file order) and the direct files' descriptors.
	int describe() {
		for (File& f : fs) {
			if (f.err) continue;
			f.rec0 = (uint32_t)recs.size();
			for (uint32_t k = 0; k < f.info.nframes; k++) {
				const WebPAnimFrame& a = f.fr[k];
				Vp8gAnimFrame r;
				memset(&r, 0, sizeof(r));
				r.src = refs[f.ref0 + k].src, r.x = a.x, r.y = a.y, r.width = a.width, r.height = a.height;
				r.flags = (a.blend ? VP8G_ANIM_BLEND : 0u) | (a.dispose ? VP8G_ANIM_DISPOSE : 0u) | (a.has_alpha ? VP8G_ANIM_HAS_ALPHA : 0u);
				recs.push_back(r);
			}
		}
		for (uint32_t i = 0; i < n; i++)
			if (!fs[i].err && fs[i].route == kDirect) by_route.push_back(i);
		ndirect = (uint32_t)by_route.size();
		for (uint32_t i = 0; i < n; i++)
			if (!fs[i].err && fs[i].route != kDirect) by_route.push_back(i);
		descs.resize(by_route.size());  // (recs no longer moves: the descriptors point into it)
		uint32_t task0 = 0;
		for (uint32_t q = 0; q < ndirect; q++) {
			if (make_desc(q, t->width, t->height, (uint64_t)fs[by_route[q]].first * slot, task0) != 0) return EINVAL;
			task0 += descs[q].ntasks;
		}
		return 0;
	}
	// The scaled files compose at full size into the staging buffer, group by group: whole animations, canvas bytes up to the
	// cap (one animation at least).  Their descriptors -- every one is made before the records are uploaded, since the maker
	// completes them -- and each group's layout, the planar batch priced as ArgbScaleBatch will build it.
	int plan_groups() {
		const uint64_t cap = stage_bytes ? stage_bytes : kStageDefault;
		for (uint32_t q = ndirect; q < by_route.size();) {
			Group g = {q, q, 0, 0, 0, 0, 0, 0, 0, 0};
			uint64_t cb = 0, off = 0, work = 0, scaled = 0;
			uint32_t task0 = 0;
			for (; g.q1 < by_route.size(); g.q1++) {
				const File& f = fs[by_route[g.q1]];
				const uint64_t b = canvas_bytes(f) * f.info.nframes;
				if (g.q1 > g.q0 && cb + b > cap) break;
				if (make_desc(g.q1, f.info.canvas_width, f.info.canvas_height, off, task0) != 0) return EINVAL;
				task0 += descs[g.q1].ntasks;
				cb += b, off = al256(off + b);
				if (f.route == kFused) {
					g.nf += f.info.nframes;
					continue;
				}
				const ArgbScaleBatch::Need nd = ArgbScaleBatch::need(f.info.canvas_width, f.info.canvas_height, &f.opt);
				g.np += f.info.nframes, work += f.info.nframes * nd.work, scaled += f.info.nframes * nd.scaled;
			}
			g.o_fd = off;
			g.o_pd = al256(g.o_fd + g.nf * sizeof(Vp8gScaleArgbTensorDesc));
			g.o_td = al256(g.o_pd + g.np * sizeof(Vp8gScaleArgbDesc));
			g.o_sc = al256(g.o_td + g.np * sizeof(Vp8gTensorArgbDesc));
			g.o_work = al256(g.o_sc + scaled);
			g.bytes = g.o_work + ArgbScaleBatch::head_bytes(g.np) + work;
			groups.push_back(g);
			q = g.q1;
		}
		return 0;
	}
	// Zeroes the slots of the failed files, uploads the records and composes the direct files into the tensor.
	int launch_direct() {
		Status st;
		for (uint32_t i = 0; st.ok() && i < n; i++)
			if (fs[i].err && !fs[i].fr.empty())
				st = Status{hipMemsetAsync(d_out + (uint64_t)fs[i].first * slot, 0, (uint64_t)fs[i].info.nframes * slot, nullptr), "memset"};
		if (st.ok() && !descs.empty()) st = upload(buf + rec_off, recs.data(), recs.size() * sizeof(Vp8gAnimFrame));
		if (st.ok() && ndirect) st = upload((uint8_t*)d_descs(), descs.data(), ndirect * sizeof(Vp8gAnimDesc));
		if (!st.ok()) return io(st);
		if (ndirect && vp8g_anim_compose_batch_device(descs.data(), d_descs(), ndirect, t, channels, buf, d_out, nullptr) != 0) return errno;
		return 0;
	}
	int alloc_staging() {
		uint64_t most = 0;
		for (const Group& g : groups) most = std::max(most, g.bytes);
		return groups.empty() ? 0 : dev_alloc(&stg, most);
	}
	// The rescale descriptors of a group's canvases, canvas k of a file from its k-th staged canvas into slot first + k.
	int describe_group(const Group& g) {
		fd.clear();
		planar.begin(g.np, g.o_sc);
		uint32_t f_task = 0;
		for (uint32_t q = g.q0; q < g.q1; q++) {
			const File& f = fs[by_route[q]];
			const uint32_t cw = f.info.canvas_width, ch = f.info.canvas_height;
			for (uint32_t k = 0; k < f.info.nframes; k++) {
				const uint64_t src = descs[q].dst + k * canvas_bytes(f), dst = (uint64_t)(f.first + k) * slot;
				if (f.route == kPlanar) {
					if (planar.add(cw, ch, src, &f.opt, t, channels, dst) != 0) return EINVAL;
					continue;
				}
				Vp8gScaleArgbTensorDesc d;
				if (vp8g_make_scale_argb_tensor_desc(cw, ch, src, &f.opt, dst, f_task, &d) != 0) return EINVAL;
				f_task += d.ntasks;
				fd.push_back(d);
			}
		}
		return 0;
	}
	// One group: composed into the staging buffer, then the fused launch, then the planar launches.  The synchronisation at
	// the end is the group's own: the next group reuses the staging buffer, `fd` and `planar`.  A launch entry point that
	// fails leaves the call's errno (EINVAL / ENOMEM before it launched anything, or EIO) and its own text.
	int run_group(const Group& g) {
		if (int e = describe_group(g)) return e;
		const uint32_t cnt = g.q1 - g.q0;
		const Vp8gTensorOpt st = argb_tensor(1, 1);  // the staging canvases (width and height are not read)
		if (Status s = upload((uint8_t*)(d_descs() + g.q0), descs.data() + g.q0, cnt * sizeof(Vp8gAnimDesc)); !s.ok()) return io(s);
		if (vp8g_anim_compose_batch_device(descs.data() + g.q0, d_descs() + g.q0, cnt, &st, 4, buf, stg, nullptr) != 0) return errno;
		if (g.nf) {
			if (Status s = upload(stg + g.o_fd, fd.data(), g.nf * sizeof(fd[0])); !s.ok()) return io(s);
			if (vp8g_scale_argb_tensor_batch_device(fd.data(), (const Vp8gScaleArgbTensorDesc*)(stg + g.o_fd), g.nf, t, channels, stg, d_out, nullptr) != 0)
				return errno;
		}
		if (g.np) {
			Status s = upload(stg + g.o_pd, planar.scale.data(), g.np * sizeof(Vp8gScaleArgbDesc));
			if (s.ok()) s = upload(stg + g.o_td, planar.tensor.data(), g.np * sizeof(Vp8gTensorArgbDesc));
			if (!s.ok()) return io(s);
			if (!planar.launch((const Vp8gScaleArgbDesc*)(stg + g.o_pd), (const Vp8gTensorArgbDesc*)(stg + g.o_td), stg, stg + g.o_work, t, channels,
			                   d_out, nullptr).ok())
				return errno;
		}
		return io(Status{hipStreamSynchronize(nullptr), "sync"});
	}
	// Every stage but the last; 0 when the tensor is complete.
	int run() {
		slot = channels == 4u ? vp8g_tensor_slot_size_a(t) : vp8g_tensor_slot_size(t);
		if (int e = parse_files()) return e;
		layout_frames();
		if (int e = decode_frames()) return e;
		if (int e = describe()) return e;
		if (int e = plan_groups()) return e;
		if (int e = launch_direct()) return e;
		if (int e = alloc_staging()) return e;
		for (const Group& g : groups)
			if (int e = run_group(g)) return e;
		return io(Status{hipStreamSynchronize(nullptr), "sync"});
	}
	// The per-file status of a call that ran; the first error in index order, or 0.
	int finish(int* status) const {
		int first = 0;
		for (uint32_t i = 0; i < n; i++) {
			if (status) status[i] = fs[i].err;
			if (fs[i].err && !first) first = fs[i].err;
		}
		return first;
	}
};

}  // namespace

VP8G_API int vp8g_anim_info(const ByteSpan* files, uint32_t n, uint32_t* canvas_w, uint32_t* canvas_h, uint32_t* nframes, uint32_t* loop_count,
                            int* status) {
	if (!files || !nframes || n == 0) return vp8g::fail(EINVAL);
	int first = 0;
	for (uint32_t i = 0; i < n; i++) {
		WebPAnimInfo info;
		const int e = webp_parse_anim(files[i], &info, nullptr, 0) == 0 ? 0 : EINVAL;  // (a refused file: info is zero)
		if (canvas_w) canvas_w[i] = info.canvas_width;
		if (canvas_h) canvas_h[i] = info.canvas_height;
		nframes[i] = info.nframes;
		if (loop_count) loop_count[i] = info.loop_count;
		if (status) status[i] = e;
		if (e && !first) first = e;
	}
	return first ? vp8g::fail(first) : 0;
}

VP8G_API int vp8g_decode_webp_anim_tensor_scaled(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                                 const Vp8gScaleOpt* opts, uint32_t n_opts, uint64_t stage_bytes, const Vp8gTensorOpt* t,
                                                 uint32_t channels, void* d_out, uint32_t* timestamps, int* status) {
	if (!files || n == 0 || !d_out || (channels != 3 && channels != 4) || !vp8g_tensor_slot_size(t) ||
	    (uintptr_t)d_out % (uint32_t)elem_bytes(t->dtype) || (flags & ~(VP8G_BATCH_DEVICE_M05 | VP8G_BATCH_MULTI_PARTITION)) ||
	    (n_opts != 0 && n_opts != 1 && n_opts != n) || (n_opts && !opts))
		return vp8g::fail(EINVAL);
	int whole = 0, first = 0;  // the errno of a call that fails as a whole; else of the first file that failed
	try {
		AnimCall c{files, n, filtered, threads, flags, opts, n_opts, stage_bytes, t, channels, (uint8_t*)d_out, timestamps};
		whole = c.run();
		if (!whole) first = c.finish(status);
	} catch (const std::bad_alloc&) {
		whole = ENOMEM;
	}
	// (~AnimCall has run: nothing of the call is in flight, and errno is set after it)
	if (whole) return fail_all(status, n, whole);
	return first ? vp8g::fail(first) : 0;
}

VP8G_API int vp8g_decode_webp_anim_tensor(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                          const Vp8gTensorOpt* t, uint32_t channels, void* d_out, uint32_t* timestamps, int* status) {
	return vp8g_decode_webp_anim_tensor_scaled(files, n, filtered, threads, flags, nullptr, 0, 0, t, channels, d_out, timestamps, status);
}
