// vp8g_rgb_device.h -- the device arithmetic of m08: "fancy" 4:2:0 upsampling and libwebp's
// VP8YuvToRgb, shared by the file encoder (vp8g_rgb.hip) and the tensor writer (vp8g_tensor.hip).
// Both produce the same RGB bytes because both go through pair_rgb / yuv_rgb below.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp8g_rgb {

#define VP8G_RGB_DEV __device__ __forceinline__

constexpr uint32_t kChunk = 12;          // pixels of a row per thread and iteration
constexpr uint32_t kUnits = kChunk / 2;  // pixel-pair units m .. m + kUnits touched by a chunk

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));

// reference yuv2rgb_ppm.c:19-42: libwebp VP8YuvToRgb (14-bit fixed point, clip of v >> 6)
// Clamp before the shift (same result as clip(v >> 6)): the shift-then-clamp form of two
// neighbouring channels is selected as v_ashr_pk_u8_i32, whose result here kept the old upper 16
// bits of its destination register, which then leaked into the packed colour word.
VP8G_RGB_DEV uint32_t clip6(int v) { return (uint32_t)min(max(v, 0), 16383) >> 6; }
VP8G_RGB_DEV uint32_t yuv_rgb(int y, int u, int v) {  // packed r | g << 8 | b << 16
	const int yy = (y * 19077) >> 8;
	const uint32_t r = clip6(yy + ((v * 26149) >> 8) - 14234);
	const uint32_t g = clip6(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708);
	const uint32_t b = clip6(yy + ((u * 33050) >> 8) - 17685);
	return r | (g << 8) | (b << 16);
}

// One unit = pixels {2k-1, 2k} of a row (reference yuv2rgb_ppm.c:44-121): it blends chroma columns
// k-1 and k of the two chroma rows around the pixel row (at the edges both columns are one, which
// gives the 3:1 edge formula exactly).  (tl, t) = row a, (l, u) = row b; near_a = the pixel row is
// nearer row a.  Returns the two pixels' colours.
VP8G_RGB_DEV void pair_rgb(bool near_a, int tlu, int tu, int lu, int uu, int tlv, int tv, int lv, int uv, int y_odd,
                           int y_even, uint32_t& c_odd, uint32_t& c_even) {
	const int au = tlu + tu + lu + uu + 8, av = tlv + tv + lv + uv + 8;
	const int d12u = (au + 2 * (tu + lu)) >> 3, d03u = (au + 2 * (tlu + uu)) >> 3;
	const int d12v = (av + 2 * (tv + lv)) >> 3, d03v = (av + 2 * (tlv + uv)) >> 3;
	c_odd = yuv_rgb(y_odd, near_a ? (d12u + tlu) >> 1 : (d03u + lu) >> 1, near_a ? (d12v + tlv) >> 1 : (d03v + lv) >> 1);
	c_even = yuv_rgb(y_even, near_a ? (d03u + tu) >> 1 : (d12u + uu) >> 1, near_a ? (d03v + tv) >> 1 : (d12v + uv) >> 1);
}

VP8G_RGB_DEV uint32_t byte_of3(u32x3 v, int i) { return ((i < 4 ? v.x : (i < 8 ? v.y : v.z)) >> (8 * (i & 3))) & 255u; }

// 8 chroma samples, columns m1 .. m1 + 7 of one row (m1 >= -1), with the edge rule of the
// upsampler (reference yuv2rgb_ppm.c:44-121: column -1 reads column 0, columns >= cw read cw - 1):
// one unaligned 8-byte load inside the row, then the missing edge bytes replicated.  cw >= 8.
VP8G_RGB_DEV uint64_t chroma8(const uint8_t* row, int m1, int cw) {
	const int s = min(max(m1, 0), cw - 8);
	uint64_t v = *(const uint64_t*)(row + s);  // unaligned: gfx950 runs in unaligned mode (tools/ubench/unaligned.hip)
	const int dl = m1 - s;                     // -1 (left edge), 0 (inside), 1..7 (right edge)
	if (dl < 0) v = (v << 8) | (v & 0xFFu);
	if (dl > 0) v = (v >> (8 * dl)) | (((v >> 56) * 0x0101010101010101ull) << (64 - 8 * dl));
	return v;
}
VP8G_RGB_DEV uint32_t byte8(uint64_t v, int i) { return (uint32_t)(v >> (8 * i)) & 255u; }

// The kChunk colours of the whole chunk [x0, x0 + kChunk) of row y (x0 even, x0 + kChunk <= the
// width, cw >= 8): units m .. m+6 (unit k = pixels 2k-1, 2k) over chroma columns m-1 .. m+6 of the
// chroma rows a and b; pixel x0 + 2i is the even pixel of unit m+i, x0 + 2i - 1 the odd pixel of
// unit m+i.  One unaligned 8-byte load per chroma row and plane, one 12-byte luma load.
VP8G_RGB_DEV void chunk_rgb(const uint8_t* yrow, const uint8_t* ua_row, const uint8_t* ub_row, const uint8_t* va_row,
                            const uint8_t* vb_row, uint32_t x0, int cw, bool near_a, uint32_t (&c)[kChunk]) {
	const int m1 = (int)(x0 >> 1) - 1;
	const uint64_t ua = chroma8(ua_row, m1, cw), ub = chroma8(ub_row, m1, cw);
	const uint64_t va = chroma8(va_row, m1, cw), vb = chroma8(vb_row, m1, cw);
	const u32x3 yl = *(const u32x3*)(yrow + x0);
#pragma unroll
	for (int i = 0; i <= (int)kUnits; i++) {
		uint32_t c_odd, c_even;
		const int yo = i ? (int)byte_of3(yl, 2 * i - 1) : 0, ye = i < (int)kUnits ? (int)byte_of3(yl, 2 * i) : 0;
		pair_rgb(near_a, (int)byte8(ua, i), (int)byte8(ua, i + 1), (int)byte8(ub, i), (int)byte8(ub, i + 1), (int)byte8(va, i),
		         (int)byte8(va, i + 1), (int)byte8(vb, i), (int)byte8(vb, i + 1), yo, ye, c_odd, c_even);
		if (i) c[2 * i - 1] = c_odd;
		if (i < (int)kUnits) c[2 * i] = c_even;
	}
}

// The kChunk colours of the whole chunk [x0, x0 + kChunk) of a row of 4:4:4 planes (x0 + kChunk <= the width; the
// planes of libwebp's scaled RGB, which has no upsampler: DESIGN.md §14.2): one 12-byte load per plane, at whatever
// address the row and x0 give (u32x3u says so to the compiler; gfx950 runs global loads in unaligned mode,
// tools/ubench/unaligned.hip), then VP8YuvToRgb per pixel.
typedef uint32_t u32x3u __attribute__((ext_vector_type(3), aligned(1)));
VP8G_RGB_DEV void chunk_yuv444(const uint8_t* yrow, const uint8_t* urow, const uint8_t* vrow, uint32_t x0, uint32_t (&c)[kChunk]) {
	const u32x3 yl = *(const u32x3u*)(yrow + x0), ul = *(const u32x3u*)(urow + x0), vl = *(const u32x3u*)(vrow + x0);
#pragma unroll
	for (int i = 0; i < (int)kChunk; i++) c[i] = yuv_rgb((int)byte_of3(yl, i), (int)byte_of3(ul, i), (int)byte_of3(vl, i));
}

// The colour of pixel x of a row (the generic path: a row's last, partial chunk; images narrower
// than 15 pixels, whose chroma rows are shorter than the 8-byte load).
VP8G_RGB_DEV uint32_t pixel_rgb(const uint8_t* yrow, const uint8_t* ua_row, const uint8_t* ub_row, const uint8_t* va_row,
                                const uint8_t* vb_row, uint32_t x, uint32_t cw, bool near_a) {
	const uint32_t k = (x + 1u) >> 1;  // unit: pixels 2k-1 (odd x) and 2k (even x)
	const uint32_t cl = k ? k - 1u : 0u, cr = min(k, cw - 1u);
	uint32_t c_odd, c_even;
	const int yv = yrow[x];
	pair_rgb(near_a, ua_row[cl], ua_row[cr], ub_row[cl], ub_row[cr], va_row[cl], va_row[cr], vb_row[cl], vb_row[cr], yv, yv, c_odd,
	         c_even);
	return (x & 1u) ? c_odd : c_even;
}

}  // namespace vp8g_rgb
