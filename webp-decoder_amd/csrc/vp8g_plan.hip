// vp8g_plan.hip -- which recon kernel a batch runs on (host code only; declarations and the table's
// prose in vp8g_device.h).  plan_launch is pure: it reads its arguments and nothing
// else -- no HIP call, no environment -- so the whole table is tested on the CPU
// (tests/test_launch_plan.py through vp8g_plan_launch).  knobs_from_env is the one place that reads
// the six VP8G_* launch switches.
#include <errno.h>
#include <stdlib.h>

#include "vp8g_device.h"

namespace vp8g {

// Compile-time defaults of the knobs (A/B builds, tools/build_ab.sh: -DVP8G_CHAIN_DEFAULT=0,
// -DVP8G_SPLITCHAIN_DEFAULT=0 / 1, -DVP8G_CHAIN_IL_DEFAULT=0; diagnostic builds: -DVP8G_NO_ORDER,
// batch order always; -DVP8G_FORCE_GCTX, the column context in device memory for every frame).
#ifndef VP8G_CHAIN_DEFAULT
#define VP8G_CHAIN_DEFAULT -1
#endif
#ifndef VP8G_SPLITCHAIN_DEFAULT
#define VP8G_SPLITCHAIN_DEFAULT -1
#endif
#ifndef VP8G_CHAIN_IL_DEFAULT
#define VP8G_CHAIN_IL_DEFAULT -1
#endif
#ifdef VP8G_NO_ORDER
constexpr bool kOrderDefault = false;
#else
constexpr bool kOrderDefault = true;
#endif
#ifdef VP8G_FORCE_GCTX
constexpr bool kForceGctx = true;
#else
constexpr bool kForceGctx = false;
#endif
const Knobs kDefaultKnobs = {0u, 0u, VP8G_CHAIN_DEFAULT, VP8G_SPLITCHAIN_DEFAULT, VP8G_CHAIN_IL_DEFAULT, kOrderDefault, kForceGctx};

Knobs knobs_from_env() {
	Knobs k = kDefaultKnobs;
	if (const char* e = getenv("VP8G_SPLIT")) k.split = (uint32_t)strtoul(e, nullptr, 10);
	if (const char* e = getenv("VP8G_WAVES")) k.waves = (uint32_t)strtoul(e, nullptr, 10);
	if (const char* e = getenv("VP8G_CHAIN")) k.chain = atoi(e);
	if (const char* e = getenv("VP8G_SPLITCHAIN")) k.splitchain = atoi(e);
	if (const char* e = getenv("VP8G_CHAIN_IL")) k.chain_il = atoi(e);
	if (const char* e = getenv("VP8G_ORDER")) k.order = k.order && e[0] != '0';
	return k;
}

namespace {

// Waves per frame workgroup: the hint if non-zero, else 8 (two frames per CU) when the batch fills
// the chip and 16 for at most one frame per CU (twice the MB row pairs in flight); no more than MB
// row pairs, rounded down to a supported count.
uint32_t pick_waves(uint32_t waves_hint, uint32_t max_mb_rows, uint32_t n_frames, int n_cus) {
	static const uint32_t kSupported[] = {1, 2, 4, 8, 12, 16};
	uint32_t want = waves_hint ? waves_hint : (n_cus > 0 && n_frames <= (uint32_t)n_cus ? 16u : 8u);
	const uint32_t pairs = (max_mb_rows + 1) / 2;
	if (want > pairs) want = pairs;
	uint32_t nw = 1;
	for (uint32_t s : kSupported)
		if (s <= want) nw = s;
	return nw;
}

// Workgroups per frame: split_hint if non-zero, else CUs / frames, capped at kMaxSplit and at one
// part per CU overall (all parts must be co-resident), 1 if not possible.
uint32_t pick_split(uint32_t split_hint, uint32_t n_frames, uint32_t nw, uint32_t max_mb_rows, int n_cus) {
	if (nw != 8 && nw != 16) return 1;  // split kernels exist for these only
	const uint32_t pairs = (max_mb_rows + 1) / 2;
	uint32_t k = split_hint ? split_hint : (n_cus > 0 ? (uint32_t)n_cus / n_frames : 1u);
	if (k > kMaxSplit) k = kMaxSplit;
	while (k > 1 && (k - 1) * nw >= pairs) k--;  // every part gets at least one pair
	if (n_cus <= 0 || (uint64_t)n_frames * k > (uint64_t)n_cus) k = 1;
	return k ? k : 1;
}

// Cost-balanced placement of an unsplit launch: F = the CU count when that is worth it (more frames
// than CUs, classes differ), else 0 (a uniform batch: the order would be the identity).
uint32_t pick_order(const Vp8gFrameDesc* h_descs, uint32_t n_frames, int n_cus, bool on) {
	if (!on || n_cus <= 0 || n_frames <= (uint32_t)n_cus) return 0;
	const uint32_t c0 = cost_class(h_descs[0]);
	for (uint32_t i = 1; i < n_frames; i++)
		if (cost_class(h_descs[i]) != c0) return (uint32_t)n_cus;
	return 0;
}

// Chain mode: the workgroup count (0 = not applicable: too few frames, a loop-filter-only frame in
// the batch -- the quad kernel has no such path --, more than 1024 MB columns, or chain = 0), and
// whether the frames are placed by cost class (needs the sort scratch to fit the wave areas).
uint32_t pick_chain(const Vp8gFrameDesc* h_descs, uint32_t n_frames, uint32_t ctx_cols, int n_cus, const Knobs& kn, bool* ordered) {
	*ordered = false;
	if (kn.chain == 0 || n_cus <= 0 || (kn.chain < 0 && n_frames <= (uint32_t)n_cus)) return 0;
	for (uint32_t i = 0; i < n_frames; i++)
		if (h_descs[i].mb_cols != 0 && h_descs[i].mb_rows != 0 && (h_descs[i].flags & VP8G_F_LF_ONLY)) return 0;
	const uint32_t wg = n_frames < (uint32_t)n_cus ? n_frames : (uint32_t)n_cus;
	const uint32_t list_max = (n_frames + wg - 1) / wg;
	if (ctx_cols > 1024 || chain_lds_bytes(list_max) > (size_t)kMaxLds) return 0;
	*ordered = (size_t)4 * (kCostClasses + n_frames) <= kChainScratch && pick_order(h_descs, n_frames, n_cus, kn.order) != 0;
	return wg;
}

// Mirror split: worth it for ordered batches of at most two frames per workgroup (splitchain = 0 / 1
// forces it off / on), and the doubled list must fit.
bool pick_chain_split(uint32_t n_frames, uint32_t workgroups, bool ordered, int mode) {
	if (mode == 0 || workgroups == 0) return false;
	const uint32_t list_max = (n_frames + workgroups - 1) / workgroups;
	if (chain_lds_bytes(2 * list_max) > (size_t)kMaxLds) return false;
	return mode > 0 || (ordered && list_max <= 2);
}

// Two-frame interleave: every frame of the batch the same size, at least two per workgroup and no
// mirror split (chain_il = 0 forces it off).
bool pick_chain_interleave(const Vp8gFrameDesc* h_descs, uint32_t n_frames, uint32_t workgroups, bool split, int mode) {
	if (mode == 0 || split || workgroups == 0 || n_frames < 2 * workgroups) return false;
	for (uint32_t i = 1; i < n_frames; i++)
		if (h_descs[i].mb_cols != h_descs[0].mb_cols || h_descs[i].mb_rows != h_descs[0].mb_rows) return false;
	if (h_descs[0].mb_rows < 2) return false;
	const uint32_t list_max = (n_frames + workgroups - 1) / workgroups;
	return chain_lds_bytes(list_max) <= (size_t)kMaxLds;
}

// Every 16-B luma / 8-B chroma row piece inside its frame and aligned (relative to the output base).
bool whole_pieces(const Vp8gFrameDesc* h_descs, uint32_t n_frames) {
	for (uint32_t i = 0; i < n_frames; i++) {
		const Vp8gFrameDesc& d = h_descs[i];
		if (d.mb_cols == 0 || d.mb_rows == 0) continue;
		if (d.width != 16u * d.mb_cols || ((d.out_y | d.stride_y) & 15u) != 0 || ((d.out_u | d.stride_uv | (d.out_v - d.out_u)) & 7u) != 0)
			return false;
	}
	return true;
}

Launch frames_launch(uint32_t n, uint32_t ctx_cols, uint32_t waves, bool gctx, uint32_t parts, uint32_t ord_first) {
	Launch L = {};
	L.waves = waves;
	L.gctx = gctx;
	L.parts = parts;
	L.workgroups = n * parts;
	L.ord_first = ord_first;
	L.lds = (uint32_t)lds_bytes((int)waves, ctx_cols, gctx);
	L.mode = parts > 1 ? VP8G_MODE_SPLIT_PARTS : 0u;
	return L;
}

Launch chain_launch(uint32_t n, uint32_t wg, bool ordered, bool split, bool interleave, bool whole) {
	Launch L = {};
	L.quad = true;
	L.waves = 16;
	L.parts = 1;
	L.workgroups = wg;
	L.ordered = ordered, L.split = split, L.interleave = interleave, L.whole = whole;
	const uint32_t list_max = (n + wg - 1) / wg;
	L.lds = (uint32_t)chain_lds_bytes(split ? 2 * list_max : list_max);
	L.mode = VP8G_MODE_CHAIN | VP8G_MODE_QUAD | (split ? VP8G_MODE_MIRROR_SPLIT : 0u) | (interleave ? VP8G_MODE_INTERLEAVE : 0u);
	return L;
}

}  // namespace

LaunchPlan plan_launch(const Vp8gFrameDesc* h_descs, uint32_t n, int n_cus, bool out_aligned, uint32_t waves_hint, const Knobs& knobs,
                       const LaunchPolicy& pol) {
	LaunchPlan P = {};
	P.n = n;
	if (n == 0) return P;  // (nothing to launch: launch() returns at once)
	for (uint32_t i = 0; i < n; i++) {
		if (h_descs[i].mb_cols > P.ctx_cols) P.ctx_cols = h_descs[i].mb_cols;
		if (h_descs[i].mb_rows > P.max_rows) P.max_rows = h_descs[i].mb_rows;
	}
	const uint32_t cols = P.ctx_cols, rows = P.max_rows;
	const uint32_t hint = !waves_hint && pol.env_geometry ? knobs.waves : waves_hint;
	const uint32_t env = pol.env_geometry ? knobs.split : 0u;
	const bool plain = hint && pol.hint_plain;
	const uint32_t nw = pick_waves(hint, rows, n, n_cus);
	// small batches: 8-wave parts, up to kMaxSplit per frame (measured on one 4K frame: 8 waves x 8
	// parts 3.9 ms per call, 16 waves x 1..8 parts 8.1..4.7 ms)
	const bool try_split = (pol.may_split || env > 1) && env != 1 && !plain;
	const uint32_t nw_split = try_split && pick_split(env, n, 8, rows, n_cus) > 1 ? 8u : nw;
	const uint32_t nw_whole = pol.split_waves_stay ? nw_split : nw;  // (unsplit launches)
	const bool big = (pol.env_geometry && knobs.force_gctx) || lds_bytes((int)nw_whole, cols, false) > (size_t)kMaxLds;
	const bool big_split = lds_bytes((int)nw_split, cols, false) > (size_t)kMaxLds;
	const uint32_t parts = !big_split && try_split ? pick_split(env, n, nw_split, rows, n_cus) : 1u;
	bool ordered = false;
	const uint32_t wg = !big && !plain ? pick_chain(h_descs, n, cols, n_cus, knobs, &ordered) : 0u;
	const bool split = wg && pol.chain_extras && pick_chain_split(n, wg, ordered, knobs.splitchain);
	const bool whole = wg && whole_pieces(h_descs, n) && out_aligned;
	// (the interleave depends on whether the gate lets the mirror split through: one answer per outcome)
	auto chain = [&](bool sp) {
		return chain_launch(n, wg, ordered, sp, pol.chain_extras && pick_chain_interleave(h_descs, n, wg, sp, knobs.chain_il), whole);
	};
	P.shut = wg ? chain(false) : frames_launch(n, cols, nw_whole, big, 1, pol.placement ? pick_order(h_descs, n, n_cus, knobs.order) : 0u);
	P.open = parts > 1 ? frames_launch(n, cols, nw_split, false, parts, 0) : (split ? chain(true) : P.shut);

	// what the launches of either outcome read and write beside the batch itself
	const size_t ctx = (size_t)n * cols * kCtxBytesPerCol;
	P.gctx_bytes = big || (wg && pol.snap_in_gctx) ? ctx : 0;
	P.snap_bytes = wg && !pol.snap_in_gctx ? ctx : 0;
	P.mbox_bytes = parts > 1 ? (size_t)parts * ctx : 0;
	P.gprog_bytes = parts > 1 ? (size_t)n * parts * sizeof(uint32_t) : 0;
	P.flags_bytes = split ? (size_t)n * sizeof(uint32_t) : 0;
	return P;
}

}  // namespace vp8g

#define VP8G_API extern "C" __attribute__((visibility("default")))

VP8G_API int vp8g_plan_launch(const Vp8gFrameDesc* descs, uint32_t n, uint32_t cus, uint32_t waves_hint, uint32_t split, uint32_t waves,
                              int32_t chain, int32_t splitchain, int32_t chain_il, int32_t order, uint32_t policy, int may_cross,
                              Vp8gLaunchPlan* out) {
	if ((!descs && n) || !out || policy > (VP8G_PLAN_PIPELINE | VP8G_PLAN_NO_SPLIT)) {
		errno = EINVAL;
		return -1;
	}
	for (uint32_t i = 0; i < n; i++)  // (what vp8g_decode_batch_device accepts)
		if (descs[i].mb_cols > 1024 || descs[i].mb_rows > 1024 || (!descs[i].mb_cols != !descs[i].mb_rows)) {
			errno = EINVAL;
			return -1;
		}
	vp8g::Knobs kn = vp8g::kDefaultKnobs;
	kn.split = split, kn.waves = waves, kn.chain = chain, kn.splitchain = splitchain, kn.chain_il = chain_il, kn.order = order != 0;
	vp8g::LaunchPolicy pol = policy & VP8G_PLAN_PIPELINE ? vp8g::kPipelinePolicy : vp8g::kReferencePolicy;
	pol.may_split = !(policy & VP8G_PLAN_NO_SPLIT);
	const vp8g::LaunchPlan P = vp8g::plan_launch(descs, n, (int)cus, true, waves_hint, kn, pol);
	const vp8g::Launch& L = P.resolve(may_cross != 0);
	*out = Vp8gLaunchPlan{L.quad, L.waves, L.gctx, L.parts, L.workgroups, L.ordered, L.split, L.interleave, L.whole, L.ord_first, L.lds, L.mode,
	                      P.gctx_bytes, P.mbox_bytes + P.gprog_bytes, P.snap_bytes, P.flags_bytes};
	return 0;
}
