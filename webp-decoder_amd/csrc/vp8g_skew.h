// vp8g_skew.h -- hooks of the skew build (lib/diag/libvp8g_skew.so, -DVP8G_TEST_SKEW; DESIGN.md §3.2.1,
// tests/test_gpu_skew.py).  Without the flag every macro below expands to nothing (or to the constant
// 0): the shipped library's code does not change.
//
// The hand-offs between waves are progress words and flags that a producer publishes and a consumer
// polls.  Under the natural schedule the producer runs well ahead, so a threshold one step too small
// still reads finished data.  The skew build
//   * sleeps right after a publish (a quarter of them, in runs of four steps, chosen by a hash of seed,
//     site, workgroup, unit and step): for that long, what was published is all a consumer can rely on;
//   * counts, per wait site, how often the wait was entered satisfied and how often it had to spin;
//   * fills the hand-off buffers with 0xA5 before every launch (vp8g_shim.hip), so that context read
//     too early is not the previous launch's (correct) bytes;
//   * can lower one wait's threshold by one step (`early_site`): the mutants the tests must catch.
#ifndef VP8G_SKEW_H
#define VP8G_SKEW_H

#include <stdint.h>

// wait sites (census index; the first five are also the `early_site` values)
enum : int {
	kSkQNeed = 0,   // quad: per-step context of the row above, progress >= min(t + 8, Tprev)
	kSkQRing0 = 1,  // quad: ring-0 fill before the first step, progress >= min(8, Tprev)
	kSkFWg = 2,     // frame_kernel: the pair above in this workgroup, t + 4
	kSkFPart = 3,   // frame_kernel: the pair above in another part (mailbox), t + 5
	kSkQFlag = 4,   // quad, mirror split: the top segment's flag of this epoch
	kSkQStart = 5,  // quad: the unit before this one has started (+1)
	kSkQSlot = 6,   // quad: the last quad of frame j - 2 / j - 4 before its table slot is overwritten
	kSkMRing = 7,   // m05 modes wave: less than kRing MBs ahead of the slowest token wave
	kSkMProd = 8,   // m05 token wave: the modes wave past MB m
	kSkMUp = 9,     // m05 token wave: the row above past column c
	kSkSites = 10,
	kSkMutants = 5
};
// publish sites (an input of the delay hash)
enum : int { kSkPubQStep = 0, kSkPubQEnd = 1, kSkPubFrame = 2, kSkPubModes = 3, kSkPubTokens = 4 };

#ifdef VP8G_TEST_SKEW
#include <hip/hip_runtime.h>
#define VP8G_SKEW_POISON(ptr, bytes, stream) ((ptr) && (bytes) ? hipMemsetAsync(ptr, 0xA5, bytes, stream) : hipSuccess)
#endif

#if defined(VP8G_TEST_SKEW) && !defined(VP8G_SKEW_HOST_ONLY)  // (HOST_ONLY: a unit without kernels, the poison fill alone)

// s_sleep(127) is 127 * 64 shader clocks: 128 of them are 1.04 M clocks, under 20 ms -- a hundredth of
// the 2 s wait bound (VP8G_WAIT_TICKS, counted in the constant 100 MHz clock) -- at any shader clock
// above 52 MHz, idle clocks included.  Lengths above it are refused (vp8g_skew_set_*), and the scaled
// delay is clamped to it.
#define VP8G_SKEW_MAX_LEN 128u

namespace vp8g_skew {
// one copy per translation unit that has kernels (set and read through that unit's exports below)
static __device__ uint32_t g_cfg[4];  // seed, delay length (s_sleep(127) count, 0 = none), early_site + 1
static __device__ unsigned int g_census[2 * kSkSites];  // per site: entered satisfied, had to spin

// `scale`: the quad's end-of-unit publish hands over to the waits at a unit's start (the unit before has
// started, the table slot is free), which a free wave reaches some 50 to 120 steps early; every step of
// the producers is stretched by the per-step delays too, so only a delay of many steps' worth lets the
// wave arrive late for once.
__device__ __forceinline__ void delay(uint32_t site, uint32_t unit, uint32_t step, uint32_t scale = 1u) {
	const uint32_t len = min((uint32_t)__builtin_amdgcn_readfirstlane((int)g_cfg[1]) * scale, VP8G_SKEW_MAX_LEN);
	if (len == 0) return;
	uint32_t h = g_cfg[0] ^ (site * 0x9E3779B1u) ^ ((uint32_t)blockIdx.x * 0x85EBCA77u) ^ (unit * 0xC2B2AE3Du) ^ ((step >> 2) * 0x27D4EB2Fu);
	h ^= h >> 15, h *= 0x2C1B3C6Du, h ^= h >> 12, h *= 0x297A2D39u, h ^= h >> 15;
	h = (uint32_t)__builtin_amdgcn_readfirstlane((int)h);
	if ((h & 3u) == 0)
		for (uint32_t i = 0; i < len; i++) __builtin_amdgcn_s_sleep(127);
}
__device__ __forceinline__ void census(int site, bool satisfied) {
	if ((threadIdx.x & 63u) == 0) atomicAdd(&g_census[2 * site + (satisfied ? 0 : 1)], 1u);
}
// (m05's ring wait: the slowest token wave's progress, as the wait itself takes it)
template <class P>
__device__ __forceinline__ uint32_t min_of(P words, uint32_t n) {
	uint32_t lo = 0xFFFFFFFFu;
	for (uint32_t w = 0; w < n; w++) lo = min(lo, (uint32_t)__builtin_amdgcn_readfirstlane(words[w]));
	return lo;
}
__device__ __forceinline__ uint32_t early(int site) {
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)g_cfg[2]) == (uint32_t)site + 1u ? 1u : 0u;
}
}  // namespace vp8g_skew

#define VP8G_SKEW_DELAY(site, unit, step) vp8g_skew::delay((uint32_t)(site), (uint32_t)(unit), (uint32_t)(step))
#define VP8G_SKEW_DELAY_LONG(site, unit, step) vp8g_skew::delay((uint32_t)(site), (uint32_t)(unit), (uint32_t)(step), 16u)
#define VP8G_SKEW_CENSUS(site, satisfied) vp8g_skew::census(site, satisfied)
#define VP8G_SKEW_EARLY(site) vp8g_skew::early(site)
// Diag-only exports of a translation unit (not in include/vp8g.h): the settings, and the census
// (out[2 * kSkSites]; reset != 0 zeroes it).  Synchronous copies: call between launches.
#define VP8G_SKEW_EXPORTS(tag)                                                                                                  \
	extern "C" __attribute__((visibility("default"))) int vp8g_skew_set_##tag(uint32_t seed, uint32_t len, int early_site) {    \
		if (len > VP8G_SKEW_MAX_LEN || early_site < -1 || early_site >= kSkMutants) return -1;                                  \
		const uint32_t c[4] = {seed, len, (uint32_t)(early_site + 1), 0u};                                                      \
		return hipMemcpyToSymbol(HIP_SYMBOL(vp8g_skew::g_cfg), c, sizeof(c)) == hipSuccess ? 0 : -1;                            \
	}                                                                                                                           \
	extern "C" __attribute__((visibility("default"))) int vp8g_skew_census_##tag(unsigned int* out, int reset) {                \
		if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vp8g_skew::g_census), sizeof(unsigned int) * 2 * kSkSites) != hipSuccess)       \
			return -1;                                                                                                          \
		if (reset) {                                                                                                            \
			const unsigned int z[2 * kSkSites] = {0};                                                                           \
			if (hipMemcpyToSymbol(HIP_SYMBOL(vp8g_skew::g_census), z, sizeof(z)) != hipSuccess) return -1;                      \
		}                                                                                                                       \
		return 0;                                                                                                               \
	}
#else
#define VP8G_SKEW_DELAY(site, unit, step) \
	do {                                  \
	} while (0)
#define VP8G_SKEW_DELAY_LONG(site, unit, step) \
	do {                                       \
	} while (0)
#define VP8G_SKEW_CENSUS(site, satisfied) \
	do {                                  \
	} while (0)
#define VP8G_SKEW_EARLY(site) 0u
#define VP8G_SKEW_EXPORTS(tag)
#endif
#ifndef VP8G_SKEW_POISON
#define VP8G_SKEW_POISON(ptr, bytes, stream) hipSuccess
#endif

// ---- The banded wavefront kernels (vp8g_lossless.hip, vp8g_alpha.hip) --------
// A unit defines VP8G_SKEW_BANDS (and VP8G_SKEW_HOST_ONLY: it has no wait sites) before the include.
// These kernels are paced by workgroup barriers alone, so there is nothing to delay and nothing to count;
// the skew build
//   * fills the LDS of a workgroup with 0xA5 before every image, so that a bottom row read too early is
//     not the previous launch's (correct) row;
//   * can alter one term of the schedule (`mutant`, below): the mutants tests/test_gpu_bands.py must catch.
// A mutant changes only values that every thread of the workgroup computes alike (the band delay, the
// round length, a ring's mask): every thread still reaches the same barriers, every LDS index stays
// masked, and (band, group, lane) stay within the image -- wrong pixels, never another address.
enum : unsigned {
	kBandMutNone = 0,
	kBandMutDelay = 1,     // a band trails the band above by kDelay - 1
	kBandMutRound = 2,     // a round is one step shorter
	kBandMutRing = 3,      // the ring's mask halved
	kBandMutNoLong = 4,    // the long-round branch dropped: round_len = 16 kDelay whatever the width
	kBandMutants = 5
};
#if defined(VP8G_TEST_SKEW) && defined(VP8G_SKEW_BANDS)
namespace vp8g_skew {
static __device__ uint32_t g_band_mutant;
__device__ __forceinline__ uint32_t band_mutant() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)g_band_mutant); }
// (dwords < the workgroup's dynamic LDS; all threads of the workgroup)
__device__ __forceinline__ void band_poison(uint32_t* lds, uint32_t dwords) {
	for (uint32_t i = threadIdx.x; i < dwords; i += blockDim.x) lds[i] = 0xA5A5A5A5u;
	__syncthreads();
}
}  // namespace vp8g_skew
#define VP8G_BAND_MUTANT() vp8g_skew::band_mutant()
#define VP8G_BAND_POISON(lds, dwords) vp8g_skew::band_poison(lds, dwords)
// Diag-only export of the unit: the mutant of its kernel (0: none).  A synchronous copy: call between launches.
#define VP8G_BAND_EXPORTS(tag)                                                                                \
	extern "C" __attribute__((visibility("default"))) int vp8g_band_mutant_##tag(uint32_t mutant) {           \
		if (mutant >= kBandMutants) return -1;                                                                \
		return hipMemcpyToSymbol(HIP_SYMBOL(vp8g_skew::g_band_mutant), &mutant, sizeof(mutant)) == hipSuccess ? 0 : -1; \
	}
#else
#define VP8G_BAND_MUTANT() 0u
#define VP8G_BAND_POISON(lds, dwords) \
	do {                              \
	} while (0)
#define VP8G_BAND_EXPORTS(tag)
#endif

#endif
