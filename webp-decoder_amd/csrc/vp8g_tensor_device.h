// vp8g_tensor_device.h -- the element arithmetic and the stores of the tensor writers: 8-bit channel -> element
// (conv: a rounded multiply, then a rounded add, never fused), alpha byte -> element (conv_a: a correctly rounded
// a / 255), and runs of elements stored as wide as their alignment allows.  Shared by the tensor kernels
// (vp8g_tensor.hip) and the animation compositor (vp8g_anim.hip): both write the same elements because both go
// through conv / conv_a below.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "vp8g.h"

namespace vp8g_tensor {

#define VP8G_T_DEV __device__ __forceinline__

// (dword-aligned, not 16- / 8-byte aligned: a run starts wherever its row does)
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2a __attribute__((ext_vector_type(2), aligned(4)));

constexpr int elem_bytes(uint32_t dt) { return dt == VP8G_T_U8 ? 1 : dt == VP8G_T_F32 ? 4 : 2; }

// The element (its bits, in the low bytes) of the 8-bit value v.
template <uint32_t DT>
VP8G_T_DEV uint32_t conv(uint32_t v, float s, float b) {
	if constexpr (DT == VP8G_T_U8) {
		return v;
	} else {
		// A rounded multiply, then a rounded add: hipcc contracts a * b + c into a fused multiply-add
		// by default (and __fmul_rn / __fadd_rn are plain operators to it), so contraction is
		// switched off for these two operations.
#pragma clang fp contract(off)
		const float m = (float)v * s;
		const float f = m + b;
		const uint32_t u = __float_as_uint(f);
		if constexpr (DT == VP8G_T_F32) return u;
		else if constexpr (DT == VP8G_T_F16) return (uint32_t)__half_as_ushort(__float2half_rn(f));
		else return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;  // bfloat16, nearest-even (f is finite or infinite, never NaN)
	}
}

// channel ch of the output order out of a packed r | g << 8 | b << 16
template <bool BGR>
VP8G_T_DEV uint32_t channel(uint32_t c, int ch) {
	return (c >> (8 * (BGR ? 2 - ch : ch))) & 255u;
}

template <uint32_t DT>
VP8G_T_DEV void store_elem(uint8_t* p, uint32_t e) {
	if constexpr (DT == VP8G_T_U8) *p = (uint8_t)e;
	else if constexpr (DT == VP8G_T_F32) *(uint32_t*)p = e;
	else *(uint16_t*)p = (uint16_t)e;
}

// ND dwords to a dword-aligned address: 16-byte stores, then what is left
template <int ND>
VP8G_T_DEV void store_dwords(uint8_t* p, const uint32_t (&dw)[ND]) {
	int k = 0;
#pragma unroll
	for (; k + 4 <= ND; k += 4) *(u32x4a*)(p + 4 * k) = u32x4a{dw[k], dw[k + 1], dw[k + 2], dw[k + 3]};
	if constexpr (ND % 4 >= 2) {
		*(u32x2a*)(p + 4 * k) = u32x2a{dw[k], dw[k + 1]};
		k += 2;
	}
	if constexpr (ND % 2 == 1) *(uint32_t*)(p + 4 * k) = dw[k];
}

// A run of R elements (R * element size a multiple of 4) to p: wide stores when p is dword-aligned,
// else element by element.  p is element-aligned, so a float run is always dword-aligned.
template <uint32_t DT, int R>
VP8G_T_DEV void store_run(uint8_t* p, const uint32_t (&e)[R]) {
	constexpr int EB = elem_bytes(DT), PER = 4 / EB, ND = R / PER;
	static_assert(R % PER == 0, "whole dwords");
	uint32_t dw[ND];
#pragma unroll
	for (int j = 0; j < ND; j++) {
		uint32_t v = 0;
#pragma unroll
		for (int q = 0; q < PER; q++) v |= e[PER * j + q] << (8 * EB * q);
		dw[j] = v;
	}
	if (EB == 4 || ((uintptr_t)p & 3u) == 0) {
		store_dwords<ND>(p, dw);
		return;
	}
	if constexpr (EB < 4) {
#pragma unroll
		for (int i = 0; i < R; i++) store_elem<DT>(p + EB * i, e[i]);
	}
}

// The element of the alpha byte a: the byte, or the float nearest to a / 255 (a correctly rounded
// division, not a multiply by a rounded reciprocal), rounded once more for the 16-bit types.
template <uint32_t DT>
VP8G_T_DEV uint32_t conv_a(uint32_t a) {
	if constexpr (DT == VP8G_T_U8) {
		return a;
	} else {
		const float f = __fdiv_rn((float)a, 255.0f);
		const uint32_t u = __float_as_uint(f);
		if constexpr (DT == VP8G_T_F32) return u;
		else if constexpr (DT == VP8G_T_F16) return (uint32_t)__half_as_ushort(__float2half_rn(f));
		else return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
	}
}

}  // namespace vp8g_tensor
