// vp8g_scale_device.h -- the shrink rescaler, stated once: libwebp 1.2.2's import / export loop as a closed form, the
// pieces of a kernel that walks it, and the tiling its descriptors carry.  Used by scale_kernel and expand_kernel
// (vp8g_scale.hip), the split and merge passes (vp8g_scale_argb.hip) and the fused ARGB kernel
// (vp8g_scale_argb_fused.hip); host restatement host/vp8_scale.c; DESIGN.md §14, §14.1.
//
// libwebp's rescaler is a sequential import/export loop, but its result has a closed form: with
// E(k) = ceil(k W / w) and F(j) = ceil(j H / h) (all values wrapping u32),
//
//   frow(y, k) = (carry + sum of s[y][x], x in [E(k), E(k+1))) * w - s[y][E(k+1)-1] * (E(k+1) w - (k+1) W)
//                carry = k > 0 ? MULT(s[y][E(k)-1] * (E(k) w - k W), fx) : 0
//   out(j, k)  = MULT(irow - FLOOR(frow(F(j+1)-1, k), ys), fxy)        ys = fy * (F(j+1) h - (j+1) H)
//                irow = FLOOR(frow(F(j)-1, k), ys0) + sum of frow(y, k), y in [F(j), F(j+1))
//
// so every output sample depends only on its own source footprint plus one boundary row and column.
//
// A workgroup task is a tile of tile_w output columns x run_h output rows.  It walks the source rows of its run top to
// bottom (one extra row above when the run does not start the picture: the boundary row F(j0) - 1), staged through LDS
// in blocks of block_rows row segments loaded with 16-byte loads (the next block is in flight in registers while the
// current one is summed).  `group` lanes share an output column (each sums every group-th sample of the footprint,
// combined by a butterfly of lane exchanges), so a 17:1 and a 16383:1 reduction keep the lanes as busy as a 1:1 one;
// each lane keeps its column's irow in a register and lane 0 of the group emits a sample at every F(j+1) boundary.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp8g_scale {

#define VP8G_S_DEV __device__ __forceinline__

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRunSrcRows = 64;  // source rows per task (about): 1 / 64 of the rows is read twice
constexpr uint32_t kLanePerCol = 12;  // footprint samples per lane before another lane joins the column

VP8G_S_DEV uint32_t mult_fix(uint32_t x, uint32_t y) { return __umulhi(x, y) + ((x * y) >> 31); }
VP8G_S_DEV uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
VP8G_S_DEV uint32_t clamp_u8(uint32_t v) { return (int32_t)v > 255 ? 255u : v & 255u; }

// the descriptor that owns task `task` of a launch whose descriptors number their tasks one after another from the
// member T0 (the caller still checks that the task is inside that descriptor's range)
template <typename Desc, uint32_t Desc::*T0>
VP8G_S_DEV uint32_t task_owner(const Desc* descs, uint32_t n, uint32_t task) {
	uint32_t lo = 0, hi = n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (descs[mid].*T0 <= task) lo = mid;
		else hi = mid - 1u;
	}
	return lo;
}

// Output column k of a tile that ends at kend and whose staged segment starts at source column xs: the footprint
// [e0, e1) = [E(k), E(k+1)) and the weights a0 = E(k) w - k W, a1 = E(k+1) w - (k+1) W of its two edge samples.
// A lane past the tile is not active and has an empty footprint at xs.
struct ShrinkCol {
	uint32_t e0, e1, a0, a1;
	bool active, carry_in;
	VP8G_S_DEV ShrinkCol(uint32_t k, uint32_t kend, uint32_t xs, uint32_t W, uint32_t w) {
		active = k < kend;
		e0 = xs, e1 = xs, a0 = 0, a1 = 0;
		if (active) {
			e0 = ceil_div(k * W, w), e1 = ceil_div((k + 1u) * W, w);
			a0 = e0 * w - k * W, a1 = e1 * w - (k + 1u) * W;
		}
		carry_in = active && k > 0;
	}
	// frow of an active column: carry_sample = s[y][e0 - 1] (anything without carry_in), part = the footprint's sum,
	// last_sample = s[y][e1 - 1]
	VP8G_S_DEV uint32_t frow(uint32_t carry_sample, uint32_t part, uint32_t last_sample, uint32_t w, uint32_t fx) const {
		// (24-bit multiplies: samples < 2^8, a0 / a1 / w < 2^14, a row sum < 2^22)
		const uint32_t carry = carry_in ? mult_fix(__umul24(carry_sample, a0), fx) : 0u;
		return __umul24(carry + part, w) - __umul24(last_sample, a1);
	}
};

// The source rows [y_first, y_last) of the run of output rows [j0, j1); with j0 > 0 the first one is the boundary row
// F(j0) - 1, shared with the run above.  A kernel walks them as
//
//   if (rows.shared_row(y)) { irow = rows.lower_part(frow); continue; }
//   irow += frow;
//   if (!rows.exports(y)) continue;
//   v = rows.sample(irow, frow, fxy);  ... store v at output row rows.j ...
//   rows.next();
struct ShrinkRows {
	uint32_t y_first, y_last, ys0, qH, rH, h, fy, j, nextF, ya;
	bool boundary;
	VP8G_S_DEV ShrinkRows(uint32_t j0, uint32_t j1, uint32_t H, uint32_t h_, uint32_t fy_) {
		h = h_, fy = fy_;
		boundary = j0 > 0;
		const uint32_t Fj0 = ceil_div(j0 * H, h);
		y_first = boundary ? Fj0 - 1u : 0u, y_last = ceil_div(j1 * H, h);
		ys0 = fy * (Fj0 * h - j0 * H);
		// F(j+1) and ya = F(j+1) h - (j+1) H step without a divide: H = qH h + rH, and from one output row to
		// the next F grows by qH (+ 1 when rH exceeds what the last row left over)
		qH = H / h, rH = H - qH * h;
		j = j0, nextF = ceil_div((j0 + 1u) * H, h);
		ya = nextF * h - (j0 + 1u) * H;
	}
	VP8G_S_DEV bool shared_row(uint32_t y) const { return boundary && y == y_first; }
	VP8G_S_DEV uint32_t lower_part(uint32_t frow) const { return ys0 ? __umulhi(frow, ys0) : 0u; }  // (ys0 == 0: none of it)
	VP8G_S_DEV bool exports(uint32_t y) const { return y + 1u == nextF; }
	// output row j's sample of the column whose sums are irow, at the row that exports it (frow: that row's own);
	// leaves in irow the part of that row that belongs to output row j + 1
	VP8G_S_DEV uint32_t sample(uint32_t& irow, uint32_t frow, uint32_t fxy) const {
		const uint32_t ys = fy * ya;
		const uint32_t frac = ys ? __umulhi(frow, ys) : 0u;
		// (fxy == 0: x_add == 1 and h == H, the sums are the samples: W == 1, or the two taps' w == 2)
		const uint32_t v = fxy ? clamp_u8(mult_fix(irow - frac, fxy)) : irow & 255u;
		irow = frac;
		return v;
	}
	VP8G_S_DEV void next() {
		j++;
		if (rH > ya) nextF += qH + 1u, ya = h - (rH - ya);
		else nextF += qH, ya -= rH;
	}
};

// libwebp's WebPMultARGBRow and its inverse, one pixel 0xAARRGGBB (vp8f_argb_mult_row).  The premultiply needs no special
// cases: with a = 255 the scale is 2^24 - 1 and (x (2^24 - 1) + 2^23) >> 24 = x, with a = 0 it is 0 and so is the pixel.
VP8G_S_DEV uint32_t premultiply(uint32_t p) {
	const uint32_t a = p >> 24;
	const uint32_t scale = __umul24(a, 65793u);  // (2^24 / 255; 255 * 255 * 65793 + 2^23 < 2^32)
	uint32_t out = p & 0xFF000000u;
#pragma unroll
	for (uint32_t s = 0; s < 24u; s += 8u) out |= ((__umul24((p >> s) & 255u, scale) + (1u << 23)) >> 24) << s;
	return out;
}
VP8G_S_DEV uint32_t unpremultiply(uint32_t p) {
	const uint32_t a = p >> 24;
	if (a == 255u) return p;
	if (a == 0u) return 0u;
	const uint32_t scale = (255u << 24) / a;
	uint32_t out = p & 0xFF000000u;
#pragma unroll
	for (uint32_t s = 0; s < 24u; s += 8u) {
		const uint64_t v = ((uint64_t)((p >> s) & 255u) * scale + (1u << 23)) >> 24;  // (<= 255: colour <= alpha in a rescaled pixel)
		out |= ((uint32_t)v & 255u) << s;
	}
	return out;
}

// The staging of a tile's row segments: samples of SB bytes (1: a byte plane, 4: ARGB pixels), columns [xs, xs + span)
// of a window of W x H samples whose first sample is at address `base` and whose rows are `stride` bytes apart, through
// an LDS buffer of BUF bytes in blocks of rows.  Row r of a block sits at r * pitch, its segment starting at byte
// (address & 15); a thread owns the same 16-byte chunks (row ch_r, chunk ch_c) of every block, loads them into registers
// (load) and writes them to LDS a block later (store).  Only the window's own bytes are read.
template <uint32_t SB, uint32_t BUF>
struct StagedRows {
	static_assert((SB == 1u || SB == 4u) && BUF % 16u == 0, "bytes or dwords, whole chunks");
	static constexpr uint32_t kMaxChunks = (BUF / 16u + kThreads - 1u) / kThreads;  // 16-B loads per thread and block
	const uint8_t* src;
	uintptr_t base, ok_lo, ok_hi;
	uint32_t stride, xs, span, pitch;
	uint32_t ch_r[kMaxChunks], ch_c[kMaxChunks];
	uint4 pre[kMaxChunks];

	VP8G_S_DEV StagedRows(const uint8_t* src_, uintptr_t base_, uint32_t stride_, uint32_t W, uint32_t H, uint32_t xs_, uint32_t span_,
	                      uint32_t pitch_, uint32_t tid)
	    : src(src_), base(base_), ok_lo(base_), ok_hi(base_ + (uintptr_t)(H - 1u) * stride_ + SB * W), stride(stride_), xs(xs_),
	      span(span_), pitch(pitch_) {
		const uint32_t cpr = pitch >> 4;
#pragma unroll
		for (uint32_t m = 0; m < kMaxChunks; m++) {
			const uint32_t q = tid + m * kThreads;
			ch_r[m] = q / cpr, ch_c[m] = q % cpr;
		}
	}
	VP8G_S_DEV uintptr_t row_address(uint32_t y) const { return base + (uintptr_t)y * stride + SB * xs; }  // first wanted byte
	// LDS byte of sample xs of source row y, row r of the staged block
	VP8G_S_DEV uint32_t lds_offset(uint32_t r, uint32_t y) const { return r * pitch + (uint32_t)(row_address(y) & 15u); }
	VP8G_S_DEV void load(uint32_t yb, uint32_t nr) {
#pragma unroll
		for (uint32_t m = 0; m < kMaxChunks; m++) {
			pre[m] = make_uint4(0, 0, 0, 0);
			if (ch_r[m] >= nr) continue;
			const uintptr_t row = row_address(yb + ch_r[m]);
			const uintptr_t a = (row & ~(uintptr_t)15) + 16u * ch_c[m];
			if (a >= row + SB * span) continue;  // past the segment
			const uint8_t* const pa = src + (ptrdiff_t)(a - (uintptr_t)src);  // (an offset from the kernel's pointer: a global load)
			if (a >= ok_lo && a + 16u <= ok_hi) {
				pre[m] = *(const uint4*)pa;
			} else {  // a chunk that straddles the window's first or last sample: only the samples inside
				uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
				for (uint32_t b = 0; b < 16u; b += SB) {
					if (a + b < ok_lo || a + b >= ok_hi) continue;
					if constexpr (SB == 4u) v[b >> 2] = *(const uint32_t*)(pa + b);
					else v[b >> 2] |= (uint32_t)pa[b] << (8u * (b & 3u));
				}
				pre[m] = make_uint4(v[0], v[1], v[2], v[3]);
			}
		}
	}
	// xform: what becomes of a loaded dword on its way into LDS
	template <typename X>
	VP8G_S_DEV void store(uint8_t* lds, uint32_t nr, X xform) const {
#pragma unroll
		for (uint32_t m = 0; m < kMaxChunks; m++)
			if (ch_r[m] < nr)
				*(uint4*)(lds + ch_r[m] * pitch + 16u * ch_c[m]) = make_uint4(xform(pre[m].x), xform(pre[m].y), xform(pre[m].z), xform(pre[m].w));
	}
};

#undef VP8G_S_DEV

// ---- host: the tiling a descriptor carries -----------------------------------------------------------------------

// output rows per task: about kRunSrcRows source rows
inline uint32_t shrink_run_h(uint32_t H, uint32_t h) {
	const uint32_t rh = (uint32_t)((uint64_t)kRunSrcRows * h / H);
	return rh ? rh : 1u;
}

struct ShrinkTiling {
	uint32_t group, tile_w, tiles_x, run_h, span, pitch, block_rows;
	uint64_t ntasks;
};

// W x H samples of sample_bytes each shrunk to w x h (w <= W, h <= H) through a staging buffer of buf_bytes
inline ShrinkTiling shrink_tiling(uint32_t W, uint32_t H, uint32_t w, uint32_t h, uint32_t sample_bytes, uint32_t buf_bytes) {
	ShrinkTiling t;
	t.group = 1;
	while (t.group < 64u && (uint64_t)W > (uint64_t)kLanePerCol * t.group * w) t.group *= 2u;
	t.tile_w = kThreads / t.group;
	t.tiles_x = (w + t.tile_w - 1u) / t.tile_w;
	t.run_h = shrink_run_h(H, h);
	t.ntasks = (uint64_t)t.tiles_x * ((h + t.run_h - 1u) / t.run_h);
	// a tile's source segment: E(k0 + tile_w) - E(k0) + 1 <= ceil(tile_w W / w) + 1 samples, at most W
	const uint64_t sp = ((uint64_t)t.tile_w * W + w - 1u) / w + 2u;
	t.span = sp < W ? (uint32_t)sp : W;
	// + up to 16 - sample_bytes bytes of misalignment, in whole 16-B chunks
	t.pitch = (sample_bytes * t.span + (16u - sample_bytes) + 15u) & ~15u;
	t.block_rows = buf_bytes / t.pitch;
	return t;
}

}  // namespace vp8g_scale
