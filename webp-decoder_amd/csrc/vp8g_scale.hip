// vp8g_scale.hip -- crop + rescale of I420 on the device, bit-exact to libwebp 1.2.2's rescaler
// (include/vp8g.h: vp8g_scale_batch_device, yuv420_rescale; host restatement host/vp8_scale.c;
// DESIGN.md §14).
//
// The closed form of libwebp's rescaler, the column footprint, the row walk of a run and the staging of a tile's rows
// through LDS are stated once, in vp8g_scale_device.h; scale_kernel below is that walk for one byte plane.  One launch
// scales a batch of images of mixed sizes; a workgroup task is one plane's tile of tile_w output columns x run_h
// output rows.
//
// Planes that expand in x or in y (VP8G_SCALE_EXPAND; libwebp's bilinear path) belong to a second
// kernel, expand_kernel below, launched on the same stream only when a batch has such a plane.  The
// two kernels share the task numbering (image by image, then plane by plane); a plane's `group`
// field says whose it is (0 = expand_kernel), and each kernel returns at once from the other's tasks.
#include <errno.h>
#include <string.h>

#include <mutex>

#include "../host/vp8_front.h"
#include "vp8g_device.h"
#include "vp8g_scale_device.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vp8g_scale;

constexpr uint32_t kBufBytes = 16448;  // LDS staging: one 16383-sample row segment at any alignment
constexpr uint32_t kMaxDim = 16383;
static_assert(kBufBytes % 16 == 0 && kBufBytes >= kMaxDim + 30, "staging buffer");

__global__ __launch_bounds__(kThreads) void scale_kernel(const Vp8gScaleDesc* __restrict__ descs, uint32_t n,
                                                         const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
	__shared__ __attribute__((aligned(16))) uint8_t lds[kBufBytes];
	const uint32_t task = blockIdx.x, tid = threadIdx.x;
	// the image that owns this task (tasks are numbered image by image), then its plane
	const Vp8gScaleDesc& D = descs[task_owner<Vp8gScaleDesc, &Vp8gScaleDesc::task0>(descs, n, task)];
	uint32_t t = task - D.task0;
	if (task < D.task0 || t >= D.ntasks) return;
	uint32_t pi = 0;
	while (pi < 2u && t >= D.p[pi].ntasks) t -= D.p[pi].ntasks, pi++;
	const Vp8gScalePlane& P = D.p[pi];
	const uint32_t W = P.src_w, H = P.src_h, w = P.dst_w, h = P.dst_h;
	const uint32_t fx = P.fx, fxy = P.fxy;
	const uint32_t G = P.group, pitch = P.pitch, R = P.block_rows;
	if (t >= P.ntasks || G == 0 || (G & (G - 1u)) || G > 64u || P.tile_w * G != kThreads || P.tiles_x == 0) return;
	const uint32_t tx = t % P.tiles_x, ry = t / P.tiles_x;

	// -- columns: the tile's source segment [xs, xe) and this lane's footprint
	const uint32_t k0 = tx * P.tile_w, kend = min(k0 + P.tile_w, w);
	const uint32_t j0 = ry * P.run_h, j1 = min(j0 + P.run_h, h);
	if (k0 >= w || j0 >= h) return;
	const uint32_t xs = k0 ? ceil_div(k0 * W, w) - 1u : 0u;  // E(k0) - 1: the first column's carry sample
	const uint32_t xe = ceil_div(kend * W, w);                // E(kend) <= W
	const uint32_t span = xe - xs;
	if (span + 15u > pitch || (pitch & 15u) || R == 0 || (uint64_t)pitch * R > kBufBytes) return;  // (never: see make_plane)
	const uint32_t gi = tid & (G - 1u), k = k0 + tid / G;
	const ShrinkCol col(k, kend, xs, W, w);
	ShrinkRows rows(j0, j1, H, h, P.fy);
	StagedRows<1, kBufBytes> stage(src, (uintptr_t)src + P.src, P.src_stride, W, H, xs, span, pitch, tid);  // (+ P.src: the window's first sample)

	uint32_t irow = 0;
	uint8_t* out = dst + P.dst + k;
	const uint32_t y_last = rows.y_last;
	stage.load(rows.y_first, min(R, y_last - rows.y_first));
	for (uint32_t yb = rows.y_first; yb < y_last; yb += R) {
		const uint32_t nr = min(R, y_last - yb);
		__syncthreads();  // the previous block has been summed
		stage.store(lds, nr, [](uint32_t v) { return v; });
		__syncthreads();
		if (yb + R < y_last) stage.load(yb + R, min(R, y_last - (yb + R)));  // in flight while this block is summed
		for (uint32_t r = 0; r < nr; r++) {
			const uint32_t y = yb + r;
			const uint8_t* row = lds + stage.lds_offset(r, y) - xs;  // row[x] = s[y][x] for x in [xs, xe)
			uint32_t part = 0;
			for (uint32_t x = col.e0 + gi; x < col.e1; x += G) part += row[x];
			for (uint32_t o = G >> 1; o; o >>= 1) part += __shfl_xor(part, (int)o);
			const uint32_t frow = col.active ? col.frow(col.carry_in ? row[col.e0 - 1u] : 0u, part, row[col.e1 - 1u], w, fx) : 0u;
			if (rows.shared_row(y)) {  // the row shared with the run above: only its lower part
				irow = rows.lower_part(frow);
				continue;
			}
			irow += frow;
			if (!rows.exports(y)) continue;
			const uint32_t v = rows.sample(irow, frow, fxy);
			if (col.active && gi == 0) out[(size_t)rows.j * P.dst_stride] = (uint8_t)v;
			rows.next();
		}
	}
}


// ---- expanding planes -------------------------------------------------------------------------
//
// libwebp's expand path has a closed form too.  With xe = W < w (x_add = w - 1, x_sub = W - 1):
//
//   frow(y, k) = R (w - 1) + (L - R) acc      i = max(0, ceil(k (W-1) / (w-1)) - 1), L = s[y][i], R = s[y][i+1]
//                                             acc = (i + 1)(w - 1) - k (W - 1)           (W == 1: R = L)
//
// and with ye = H < h output row j is a blend of the last two imported rows, cur = m - 1 and prev = m - 2:
//
//   m = 1 + ceil(j (H-1) / (h-1)), r = (m - 1)(h - 1) - j (H - 1), B = r 2^32 / (h - 1), A = 2^32 - B
//   out(j, k) = MULT((A frow(cur, k) + B frow(prev, k) + 2^31) >> 32, fy)     (r == 0: MULT(frow(cur, k), fy))
//
// An axis that does not expand keeps the shrink arithmetic above (footprint sums; accumulate / export).
//
// ye (x either way): a task is tile_w output columns x run_h output rows.  A horizontal pass, one lane
// per column, turns the source rows the run touches, m(j0) - 2 ... m(j1 - 1) - 1 (at most run_h + 1),
// into rows of u32 sums in LDS; a vertical pass, four adjacent columns per lane and 256 / (tile_w / 4)
// output rows at a time, blends two LDS rows per output row and stores a dword where the address
// allows.  B and the LDS row of every output row of the run are computed once, into LDS.  When x
// shrinks here, a lane sums its footprint with a plain loop (a 1000:1 shrink beside an expansion is
// not a performance target).
// xe and not ye: one lane per output column walks the run's source rows with its irow in a register,
// the row walk of vp8g_scale_device.h as scale_kernel does it with group = 1 (and its run height); the
// four lanes of an aligned dword combine their samples by lane exchange and one of them stores it.
// Source samples are read straight from global memory (two taps per sum; the rows are re-read from
// L1 / L2 by the neighbouring columns).
constexpr uint32_t kXLdsBytes = 32768;                        // rows of horizontal sums
constexpr uint32_t kXMinTile = 64, kXMaxTile = 256;           // output columns per task (ye)
constexpr uint32_t kXMaxRows = kXLdsBytes / (4u * kXMinTile);  // 128 LDS rows at the narrowest tile

__global__ __launch_bounds__(kThreads) void expand_kernel(const Vp8gScaleDesc* __restrict__ descs, uint32_t n,
                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
	__shared__ __attribute__((aligned(16))) uint32_t sums[kXLdsBytes / 4u];
	__shared__ uint32_t row_b[kXMaxRows], row_cur[kXMaxRows];
	const uint32_t task = blockIdx.x, tid = threadIdx.x;
	const Vp8gScaleDesc& D = descs[task_owner<Vp8gScaleDesc, &Vp8gScaleDesc::task0>(descs, n, task)];
	uint32_t t = task - D.task0;
	if (task < D.task0 || t >= D.ntasks) return;
	uint32_t pi = 0;
	while (pi < 2u && t >= D.p[pi].ntasks) t -= D.p[pi].ntasks, pi++;
	const Vp8gScalePlane& P = D.p[pi];
	const uint32_t W = P.src_w, H = P.src_h, w = P.dst_w, h = P.dst_h;
	const bool xexp = W < w, yexp = H < h;
	if (P.group != 0 || !(xexp || yexp) || t >= P.ntasks || P.tiles_x == 0 || P.run_h == 0) return;  // (scale_kernel's plane)
	const uint32_t fx = P.fx, fy = P.fy, fxy = P.fxy, tw = P.tile_w, sstride = P.src_stride;
	if (tw < kXMinTile || tw > kXMaxTile || (tw & (tw - 1u))) return;  // (never: see make_plane)
	const uint32_t tx = t % P.tiles_x, ry = t / P.tiles_x;
	const uint32_t k0 = tx * tw, kend = min(k0 + tw, w);
	const uint32_t j0 = ry * P.run_h, j1 = min(j0 + P.run_h, h);
	if (k0 >= w || j0 >= h) return;

	// -- this lane's column of the horizontal pass: the two taps (xe) or the footprint [e0, e1)
	const uint32_t c = tid & (tw - 1u), k = k0 + c;
	const bool colok = k < kend;
	uint32_t i0 = 0, acc = 0;
	if (colok && xexp) {
		const uint32_t up = ceil_div(k * (W - 1u), w - 1u);
		i0 = up ? up - 1u : 0u;
		acc = (i0 + 1u) * (w - 1u) - k * (W - 1u);
	}
	const ShrinkCol col(k, xexp ? 0u : kend, 0u, W, w);  // (xe: no footprint)
	const uint8_t* sbase = src + P.src;  // the window's first sample; every load below is row y < H, column < W
	// four source rows at a time, so that their loads are in flight together
	auto hsum4 = [&](const uint32_t (&y)[4], uint32_t (&f)[4]) {
		const uint8_t* row[4];
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++) row[q] = sbase + (size_t)y[q] * sstride;
		if (xexp) {
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) {
				const uint32_t L = row[q][i0], R = W > 1u ? row[q][i0 + 1u] : L;
				f[q] = R * (w - 1u) + (L - R) * acc;
			}
			return;
		}
		uint32_t sum[4] = {0, 0, 0, 0}, last[4] = {0, 0, 0, 0}, cs[4] = {0, 0, 0, 0};
		if (col.carry_in) {
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) cs[q] = row[q][col.e0 - 1u];
		}
		for (uint32_t x = col.e0; x < col.e1; x++) {  // (e1 > e0: W >= w)
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) last[q] = row[q][x], sum[q] += last[q];
		}
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++) f[q] = col.frow(cs[q], sum[q], last[q], w, fx);
	};

	if (yexp) {
		const uint32_t rows = P.block_rows;
		if (P.pitch != 4u * tw || rows != kXLdsBytes / P.pitch || P.run_h + 1u > rows) return;  // (never)
		auto m_of = [&](uint32_t j) { return H > 1u ? 1u + ceil_div(j * (H - 1u), h - 1u) : 1u; };
		const uint32_t m0 = m_of(j0), y_first = m0 >= 2u ? m0 - 2u : 0u, y_last = m_of(j1 - 1u);
		const uint32_t nrows = y_last - y_first, nout = j1 - j0;
		if (nrows > rows) return;  // (never: H < h, so a run of run_h rows touches at most run_h + 1)
		for (uint32_t jj = tid; jj < nout; jj += kThreads) {
			const uint32_t j = j0 + jj, m = m_of(j), r = (m - 1u) * (h - 1u) - j * (H - 1u), d = h - 1u;
			// B = floor(r 2^32 / d) in two 16-bit steps (r < d < 2^14)
			const uint32_t q1 = (r << 16) / d, r1 = (r << 16) - q1 * d;
			row_b[jj] = (q1 << 16) + (r1 << 16) / d;
			row_cur[jj] = m - 1u - y_first;
		}
		const uint32_t rstep = kThreads / tw;
		for (uint32_t r = tid / tw; r < nrows; r += 4u * rstep) {
			uint32_t y[4], f[4] = {0, 0, 0, 0};
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) y[q] = y_first + min(r + q * rstep, nrows - 1u);  // (past the run: a row again, dropped)
			if (colok) hsum4(y, f);
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++)
				if (r + q * rstep < nrows) sums[(r + q * rstep) * tw + c] = f[q];
		}
		__syncthreads();
		const uint32_t lanes_x = tw >> 2, cx = (tid & (lanes_x - 1u)) << 2, kk = k0 + cx;
		if (kk >= kend) return;
		for (uint32_t jj = tid / lanes_x; jj < nout; jj += kThreads / lanes_x) {
			const uint32_t B = row_b[jj], cur = row_cur[jj];
			const uint4 cv = *(const uint4*)&sums[cur * tw + cx];
			uint32_t f[4] = {cv.x, cv.y, cv.z, cv.w};
			if (B) {
				const uint4 pv = *(const uint4*)&sums[(cur - 1u) * tw + cx];  // (B != 0 only with m >= 2)
				const uint32_t g[4] = {pv.x, pv.y, pv.z, pv.w};
				const uint32_t A = 0u - B;
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++)
					f[q] = (uint32_t)(((uint64_t)A * f[q] + (uint64_t)B * g[q] + (1ull << 31)) >> 32);
			}
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) f[q] = clamp_u8(mult_fix(f[q], fy));
			uint8_t* o = dst + P.dst + (size_t)(j0 + jj) * P.dst_stride + kk;
			if (kk + 3u < kend && !((uintptr_t)o & 3u)) {
				*(uint32_t*)o = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
			} else {
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++)
					if (kk + q < kend) o[q] = (uint8_t)f[q];
			}
		}
		return;
	}

	// -- xe and not ye: scale_kernel's row walk (tile_w = 256: c == tid), the sums from the two taps
	if (tw != kThreads || !xexp) return;  // (never)
	auto hsum = [&](uint32_t y) -> uint32_t {
		const uint8_t* row = sbase + (size_t)y * sstride;
		const uint32_t L = row[i0], R = W > 1u ? row[i0 + 1u] : L;
		return R * (w - 1u) + (L - R) * acc;
	};
	ShrinkRows rows(j0, j1, H, h, fy);
	uint32_t irow = 0;
	uint8_t* out = dst + P.dst + k;
	const uint32_t lane = tid & 63u;
	for (uint32_t y = rows.y_first; y < rows.y_last; y++) {
		const uint32_t frow = colok ? hsum(y) : 0u;
		if (rows.shared_row(y)) {
			irow = rows.lower_part(frow);
			continue;
		}
		irow += frow;
		if (!rows.exports(y)) continue;
		const uint32_t v = rows.sample(irow, frow, fxy);
		// the lane whose byte starts an aligned dword stores it for the three lanes after it
		const uint32_t pk = v | ((uint32_t)__shfl_down((int)v, 1) << 8) | ((uint32_t)__shfl_down((int)v, 2) << 16) |
		                    ((uint32_t)__shfl_down((int)v, 3) << 24);
		uint8_t* o = out + (size_t)rows.j * P.dst_stride;
		const uint32_t a = (uint32_t)((uintptr_t)o & 3u);
		if (colok) {
			if (lane >= a && lane - a <= 60u && k - a + 3u < kend) {
				if (a == 0) *(uint32_t*)o = pk;
			} else {
				*o = (uint8_t)v;
			}
		}
		rows.next();
	}
}

// One plane's descriptor: factors and tiling.
void make_plane(Vp8gScalePlane* p, uint64_t src, uint32_t sstride, uint32_t W, uint32_t H, uint64_t dst, uint32_t w,
                uint32_t h) {
	memset(p, 0, sizeof(*p));
	p->src = src, p->dst = dst, p->src_stride = sstride, p->dst_stride = w;
	p->src_w = W, p->src_h = H, p->dst_w = w, p->dst_h = h;
	vp8f_scale_factors(W, H, w, h, &p->fx, &p->fy, &p->fxy);
	if (W < w || H < h) {  // expand_kernel's plane: group = 0 (include/vp8g.h)
		if (H < h) {
			p->tile_w = kXMinTile;
			while (p->tile_w < kXMaxTile && p->tile_w < w) p->tile_w *= 2u;
			p->pitch = 4u * p->tile_w;
			p->block_rows = kXLdsBytes / p->pitch;
			p->run_h = p->block_rows - 1u;
		} else {
			p->tile_w = kThreads;
			p->run_h = shrink_run_h(H, h);
		}
		p->tiles_x = (w + p->tile_w - 1u) / p->tile_w;
		p->ntasks = p->tiles_x * ((h + p->run_h - 1u) / p->run_h);
		return;
	}
	const ShrinkTiling t = shrink_tiling(W, H, w, h, 1u, kBufBytes);
	p->group = t.group, p->tile_w = t.tile_w, p->tiles_x = t.tiles_x, p->run_h = t.run_h;
	p->ntasks = (uint32_t)t.ntasks;  // (< 2^28: both sizes <= kMaxDim)
	p->pitch = t.pitch, p->block_rows = t.block_rows;
}

bool expands(const Vp8gScalePlane& p) { return p.src_w < p.dst_w || p.src_h < p.dst_h; }

// a chroma slot of a single-plane descriptor (vp8g_make_scale_desc_plane): no size, no tasks
bool plane_empty(const Vp8gScalePlane& p) { return !p.ntasks && !p.src_w && !p.src_h && !p.dst_w && !p.dst_h; }

bool plane_ok(const Vp8gScalePlane& p) {
	if (p.src_w && p.src_h && expands(p)) {  // expand_kernel's plane: exactly what make_plane gives
		uint32_t fx, fy, fxy, tw = kThreads;
		if (p.dst_w > kMaxDim || p.dst_h > kMaxDim || p.src_w > kMaxDim || p.src_h > kMaxDim || p.src_stride < p.src_w ||
		    p.dst_stride < p.dst_w || p.group != 0)
			return false;
		vp8f_scale_factors(p.src_w, p.src_h, p.dst_w, p.dst_h, &fx, &fy, &fxy);
		if (p.fx != fx || p.fy != fy || p.fxy != fxy) return false;
		if (p.src_h < p.dst_h) {
			for (tw = kXMinTile; tw < kXMaxTile && tw < p.dst_w;) tw *= 2u;
			if (p.pitch != 4u * tw || p.block_rows != kXLdsBytes / p.pitch || p.run_h != p.block_rows - 1u) return false;
		} else {
			if (p.pitch != 0 || p.block_rows != 0 || p.run_h != shrink_run_h(p.src_h, p.dst_h)) return false;
		}
		return p.tile_w == tw && p.tiles_x == (p.dst_w + tw - 1u) / tw &&
		       p.ntasks == p.tiles_x * ((p.dst_h + p.run_h - 1u) / p.run_h);
	}
	return p.src_w && p.src_h && p.dst_w && p.dst_h && p.dst_w <= p.src_w && p.dst_h <= p.src_h && p.src_w <= kMaxDim &&
	       p.src_h <= kMaxDim && p.src_stride >= p.src_w && p.dst_stride >= p.dst_w && p.group && !(p.group & (p.group - 1u)) &&
	       p.group <= 64u && p.tile_w * p.group == kThreads && p.run_h && p.tiles_x == (p.dst_w + p.tile_w - 1u) / p.tile_w &&
	       p.ntasks == p.tiles_x * ((p.dst_h + p.run_h - 1u) / p.run_h) && !(p.pitch & 15u) && p.block_rows &&
	       (uint64_t)p.pitch * p.block_rows <= kBufBytes &&
	       (((uint64_t)p.tile_w * p.src_w + p.dst_w - 1u) / p.dst_w + 2u + 15u <= p.pitch || p.src_w + 15u <= p.pitch);
}

}  // namespace

VP8G_API int vp8g_scaled_size(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint32_t* out_w, uint32_t* out_h) {
	Vp8fScaleGeom g;
	if (!out_w || !out_h) {
		errno = EINVAL;
		return -1;
	}
	if (vp8f_scale_resolve(width, height, opt, &g) != 0) return -1;
	*out_w = g.out_w, *out_h = g.out_h;
	return 0;
}

VP8G_API int vp8g_make_scale_desc(uint32_t width, uint32_t height, uint64_t src_y, uint64_t src_u, uint64_t src_v,
                                  uint32_t stride_y, uint32_t stride_uv, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                                  uint32_t task0, Vp8gScaleDesc* d) {
	Vp8fScaleGeom g;
	if (!d || vp8f_scale_resolve(width, height, opt, &g) != 0 || stride_y < width || stride_uv < (width + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	memset(d, 0, sizeof(*d));
	d->width = g.out_w, d->height = g.out_h;
	d->src_width = width, d->src_height = height, d->crop_left = g.left, d->crop_top = g.top;
	const uint32_t cw = (g.win_w + 1u) / 2u, ch = (g.win_h + 1u) / 2u, ocw = (g.out_w + 1u) / 2u, och = (g.out_h + 1u) / 2u;
	const uint64_t co = (uint64_t)(g.top / 2u) * stride_uv + g.left / 2u;
	const uint64_t ysz = (uint64_t)g.out_w * g.out_h, csz = (uint64_t)ocw * och;
	make_plane(&d->p[0], src_y + (uint64_t)g.top * stride_y + g.left, stride_y, g.win_w, g.win_h, dst_offset, g.out_w, g.out_h);
	make_plane(&d->p[1], src_u + co, stride_uv, cw, ch, dst_offset + ysz, ocw, och);
	make_plane(&d->p[2], src_v + co, stride_uv, cw, ch, dst_offset + ysz + csz, ocw, och);
	d->task0 = task0;
	d->ntasks = d->p[0].ntasks + d->p[1].ntasks + d->p[2].ntasks;
	return 0;
}

// libwebp's scaled RGB: chroma goes from its own window straight to the luma target, so the three planes
// are w x h each, back to back; a chroma plane that grows in an axis is the expand kernel's, whatever the option says
// of luma.  The tensor kernel's 4:4:4 mode reads them (vp8g_tensor_batch_device_444).
VP8G_API int vp8g_make_scale_desc_444(uint32_t width, uint32_t height, uint64_t src_y, uint64_t src_u, uint64_t src_v,
                                      uint32_t stride_y, uint32_t stride_uv, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                                      uint32_t task0, Vp8gScaleDesc* d) {
	Vp8fScaleGeom g;
	if (!d || vp8f_scale_resolve(width, height, opt, &g) != 0 || !g.scaling || stride_y < width || stride_uv < (width + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	memset(d, 0, sizeof(*d));
	d->width = g.out_w, d->height = g.out_h;
	d->src_width = width, d->src_height = height, d->crop_left = g.left, d->crop_top = g.top;
	const uint32_t cw = (g.win_w + 1u) / 2u, ch = (g.win_h + 1u) / 2u;
	const uint64_t co = (uint64_t)(g.top / 2u) * stride_uv + g.left / 2u;
	const uint64_t sz = (uint64_t)g.out_w * g.out_h;
	make_plane(&d->p[0], src_y + (uint64_t)g.top * stride_y + g.left, stride_y, g.win_w, g.win_h, dst_offset, g.out_w, g.out_h);
	make_plane(&d->p[1], src_u + co, stride_uv, cw, ch, dst_offset + sz, g.out_w, g.out_h);
	make_plane(&d->p[2], src_v + co, stride_uv, cw, ch, dst_offset + 2u * sz, g.out_w, g.out_h);
	d->task0 = task0;
	d->ntasks = d->p[0].ntasks + d->p[1].ntasks + d->p[2].ntasks;
	return 0;
}

// One plane scaled as luma (the A plane of an extended picture: libwebp rescales it with the luma
// arithmetic, window and target); p[1] and p[2] stay empty (no tasks).
VP8G_API int vp8g_make_scale_desc_plane(uint32_t width, uint32_t height, uint64_t src, uint32_t stride, const Vp8gScaleOpt* opt,
                                        uint64_t dst_offset, uint32_t task0, Vp8gScaleDesc* d) {
	Vp8fScaleGeom g;
	if (!d || vp8f_scale_resolve(width, height, opt, &g) != 0 || stride < width) {
		errno = EINVAL;
		return -1;
	}
	memset(d, 0, sizeof(*d));
	d->width = g.out_w, d->height = g.out_h;
	d->src_width = width, d->src_height = height, d->crop_left = g.left, d->crop_top = g.top;
	make_plane(&d->p[0], src + (uint64_t)g.top * stride + g.left, stride, g.win_w, g.win_h, dst_offset, g.out_w, g.out_h);
	d->task0 = task0;
	d->ntasks = d->p[0].ntasks;
	return 0;
}

VP8G_API int vp8g_scale_batch_device(const Vp8gScaleDesc* h, const Vp8gScaleDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                     uint8_t* d_dst, void* stream) {
	if (!h || !d_descs || !d_src || !d_dst || n == 0) return vp8g::fail(EINVAL);
	uint64_t total = 0;
	bool any_shrink = false, any_expand = false;
	for (uint32_t i = 0; i < n; i++) {
		const Vp8gScaleDesc& d = h[i];
		if (d.task0 != total || d.ntasks == 0 || d.ntasks != (uint64_t)d.p[0].ntasks + d.p[1].ntasks + d.p[2].ntasks ||
		    !plane_ok(d.p[0]) || !(plane_ok(d.p[1]) || plane_empty(d.p[1])) ||
		    !(plane_ok(d.p[2]) || plane_empty(d.p[2])))  // tasks must be numbered image by image
			return vp8g::fail(EINVAL);
		for (uint32_t pi = 0; pi < 3u; pi++)
			if (d.p[pi].ntasks) (expands(d.p[pi]) ? any_expand : any_shrink) = true;
		total += d.ntasks;
		if (total > 0x7FFFFFFFu) return vp8g::fail(EINVAL);
	}
	return vp8g::gated_launch((hipStream_t)stream, "scale launch", [&] {
		hipError_t e = hipSuccess;
		if (any_shrink) {
			hipLaunchKernelGGL(scale_kernel, dim3((uint32_t)total), dim3(kThreads), 0, (hipStream_t)stream, d_descs, n, d_src, d_dst);
			e = hipGetLastError();
		}
		if (e == hipSuccess && any_expand) {  // same grid, same numbering: each kernel returns from the other's tasks
			hipLaunchKernelGGL(expand_kernel, dim3((uint32_t)total), dim3(kThreads), 0, (hipStream_t)stream, d_descs, n, d_src, d_dst);
			e = hipGetLastError();
		}
		return e;
	});
}

VP8G_API int yuv420_rescale(const Yuv420Image* img, const Vp8gScaleOpt* opt, Yuv420Image* out) {
	if (!img || !opt || !out || !img->y || !img->u || !img->v || img->width == 0 || img->height == 0 ||
	    img->stride_y < img->width || img->stride_uv < (img->width + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t w = img->width, h = img->height, cw = (w + 1u) / 2u, ch = (h + 1u) / 2u;
	const uint64_t ysz = (uint64_t)w * h, csz = (uint64_t)cw * ch;
	const uint64_t o_desc = (ysz + 2 * csz + 255u) & ~255ull, o_out = o_desc + 512u;
	Vp8gScaleDesc desc;
	if (vp8g_make_scale_desc(w, h, 0, ysz, ysz + csz, w, cw, opt, o_out, 0, &desc) != 0) return -1;
	memset(out, 0, sizeof(*out));
	if (vp8g::alloc_planes(out, desc.width, desc.height, false) != 0) return -1;
	const uint32_t ow = desc.width, oh = desc.height, ocw = (ow + 1u) / 2u, och = (oh + 1u) / 2u;
	const uint64_t oysz = (uint64_t)ow * oh, ocsz = (uint64_t)ocw * och;
	hipStream_t s = nullptr;
	uint8_t* b = nullptr;
	const char* where = "stream";
	hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	if (e == hipSuccess) where = "hipMalloc", e = hipMalloc((void**)&b, o_out + oysz + 2 * ocsz + 16u);
	if (e == hipSuccess) {
		where = "H2D";
		if ((e = hipMemcpy2DAsync(b, w, img->y, img->stride_y, w, h, hipMemcpyHostToDevice, s)) == hipSuccess &&
		    (e = hipMemcpy2DAsync(b + ysz, cw, img->u, img->stride_uv, cw, ch, hipMemcpyHostToDevice, s)) == hipSuccess &&
		    (e = hipMemcpy2DAsync(b + ysz + csz, cw, img->v, img->stride_uv, cw, ch, hipMemcpyHostToDevice, s)) == hipSuccess)
			e = hipMemcpyAsync(b + o_desc, &desc, sizeof(desc), hipMemcpyHostToDevice, s);
	}
	int rc = 0;
	if (e == hipSuccess) rc = vp8g_scale_batch_device(&desc, (const Vp8gScaleDesc*)(b + o_desc), 1, b, b, s);
	if (e == hipSuccess && rc == 0) {
		where = "D2H";
		if ((e = hipMemcpyAsync(out->y, b + o_out, oysz, hipMemcpyDeviceToHost, s)) == hipSuccess &&
		    (e = hipMemcpyAsync(out->u, b + o_out + oysz, ocsz, hipMemcpyDeviceToHost, s)) == hipSuccess &&
		    (e = hipMemcpyAsync(out->v, b + o_out + oysz + ocsz, ocsz, hipMemcpyDeviceToHost, s)) == hipSuccess)
			where = "sync", e = hipStreamSynchronize(s);
	}
	if (s && e != hipSuccess) (void)hipStreamSynchronize(s);
	if (b) (void)hipFree(b);
	if (s) (void)hipStreamDestroy(s);
	if (e != hipSuccess || rc != 0) {
		const int en = e != hipSuccess ? EIO : errno;
		if (e != hipSuccess) vp8g::set_error_text(where, e);
		yuv420_free(out);
		errno = en;
		return -1;
	}
	return 0;
}

// libwebp's scaled RGB of one picture: upload, the three planes to the target size
// (vp8g_make_scale_desc_444), the tensor kernel's 4:4:4 mode into uint8 RGB triples, download.
VP8G_API int yuv420_rescale_rgb(const Yuv420Image* img, const Vp8gScaleOpt* opt, uint8_t** rgb, uint32_t* out_w, uint32_t* out_h) {
	if (!img || !opt || !rgb || !out_w || !out_h || !img->y || !img->u || !img->v || img->width == 0 || img->height == 0 ||
	    img->stride_y < img->width || img->stride_uv < (img->width + 1u) / 2u) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t w = img->width, h = img->height, cw = (w + 1u) / 2u, ch = (h + 1u) / 2u;
	const uint64_t ysz = (uint64_t)w * h, csz = (uint64_t)cw * ch;
	const uint64_t o_desc = (ysz + 2 * csz + 255u) & ~255ull, o_planes = o_desc + 512u;
	Vp8gScaleDesc desc;
	if (vp8g_make_scale_desc_444(w, h, 0, ysz, ysz + csz, w, cw, opt, o_planes, 0, &desc) != 0) return -1;
	const uint32_t ow = desc.width, oh = desc.height;
	const uint64_t osz = (uint64_t)ow * oh, o_rgb = (o_planes + 3u * osz + 255u) & ~255ull;
	Vp8gTensorOpt topt;
	memset(&topt, 0, sizeof(topt));
	topt.width = ow, topt.height = oh, topt.dtype = VP8G_T_U8, topt.layout = VP8G_T_NHWC;
	Vp8gTensorDesc tdesc;
	if (vp8g_make_tensor_desc_444(&topt, o_planes, o_planes + osz, o_planes + 2u * osz, ow, ow, 0, 0, &tdesc) != 0) return -1;
	static_assert(sizeof(Vp8gScaleDesc) + sizeof(Vp8gTensorDesc) <= 512u, "the two descriptors' room");
	uint8_t* host = (uint8_t*)malloc(3u * osz);
	if (!host) {
		errno = ENOMEM;
		return -1;
	}
	hipStream_t s = nullptr;
	uint8_t* b = nullptr;
	const char* where = "stream";
	hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	if (e == hipSuccess) where = "hipMalloc", e = hipMalloc((void**)&b, o_rgb + 3u * osz + 16u);
	if (e == hipSuccess) {
		where = "H2D";
		if ((e = hipMemcpy2DAsync(b, w, img->y, img->stride_y, w, h, hipMemcpyHostToDevice, s)) == hipSuccess &&
		    (e = hipMemcpy2DAsync(b + ysz, cw, img->u, img->stride_uv, cw, ch, hipMemcpyHostToDevice, s)) == hipSuccess &&
		    (e = hipMemcpy2DAsync(b + ysz + csz, cw, img->v, img->stride_uv, cw, ch, hipMemcpyHostToDevice, s)) == hipSuccess &&
		    (e = hipMemcpyAsync(b + o_desc, &desc, sizeof(desc), hipMemcpyHostToDevice, s)) == hipSuccess)
			e = hipMemcpyAsync(b + o_desc + sizeof(desc), &tdesc, sizeof(tdesc), hipMemcpyHostToDevice, s);
	}
	int rc = 0;
	if (e == hipSuccess) rc = vp8g_scale_batch_device(&desc, (const Vp8gScaleDesc*)(b + o_desc), 1, b, b, s);
	if (e == hipSuccess && rc == 0)
		rc = vp8g_tensor_batch_device_444(&tdesc, (const Vp8gTensorDesc*)(b + o_desc + sizeof(desc)), nullptr, nullptr, 1, &topt, 3, b,
		                                  b + o_rgb, s);
	if (e == hipSuccess && rc == 0) {
		where = "D2H";
		if ((e = hipMemcpyAsync(host, b + o_rgb, 3u * osz, hipMemcpyDeviceToHost, s)) == hipSuccess) where = "sync", e = hipStreamSynchronize(s);
	}
	if (s && e != hipSuccess) (void)hipStreamSynchronize(s);
	if (b) (void)hipFree(b);
	if (s) (void)hipStreamDestroy(s);
	if (e != hipSuccess || rc != 0) {
		const int en = e != hipSuccess ? EIO : errno;
		if (e != hipSuccess) vp8g::set_error_text(where, e);
		free(host);
		errno = en;
		return -1;
	}
	*rgb = host, *out_w = ow, *out_h = oh;
	return 0;
}
