// vp8g_device.h -- internal interface between the C-ABI shim and the gfx950 kernels.
#pragma once

#include <errno.h>

#include <hip/hip_runtime.h>

#include "vp8g.h"

struct WebPStill;  // host/vp8_front.h

namespace vp8g {

// Per-half-wave LDS scratch (bytes).  A wave works on two macroblocks at once, one per 32-lane
// half; each half owns one of these areas.  16-B aligned where a 16-B access is made.
// Filter tiles (luma 20 rows, chroma 12 rows, one pitch: the horizontal-edge pass reads every
// plane's lines with one set of immediate row offsets), each row a ring of two MB columns (slot =
// mb_col & 1).  Their placement sets the LDS bank conflicts of the loop filter's byte gathers
// (tools/lds_banks.py): 32 lines per 32-lane half -- 16 luma, 8 U and 8 V rows in the vertical-edge
// pass -- should spread over the 32 banks.  With the chroma tile 4 bytes off 8-B alignment the
// chroma 8-B pieces are accessed as two dwords (kC8).
#ifndef VP8G_TP
#define VP8G_TP 40
#endif
#ifndef VP8G_UV
#define VP8G_UV 804
#endif
#ifndef VP8G_CV
#define VP8G_CV 64
#endif
constexpr int kTP = VP8G_TP;    // tile row pitch
constexpr int kLfY = 0;         // luma filter tile: 20 rows x kTP (4 rows above + 16 MB rows; two MB
                                // columns as a ring at +0 / +16)
constexpr int kLfUV = VP8G_UV;  // chroma tile: 12 rows x kTP (4 above + 8 MB rows); per row U at +0,
constexpr int kCV = VP8G_CV;    // V at +kCV, each a ring of two 8-B MB columns
constexpr bool kC8 = kLfUV % 8 == 0 && kTP % 8 == 0 && kCV % 8 == 0;  // chroma 8-B pieces 8-B aligned
// V rows may sit rows away from their U rows (kCV >= kTP: V row r shares a physical row with U row
// r + kCV / kTP, in bytes kCV % kTP ..+16): with kCV = 64 at pitch 40 (V at 24..39 of the next row)
// the 32 rows a vertical-edge gather touches -- 16 luma, 8 U, 8 V -- fall on 32 distinct banks
// (tools/lds_banks.py), where U and V side by side (kCV = 16) met two rows per bank.
static_assert(kLfUV >= 20 * kTP && kCV % kTP >= 16 && kCV % kTP + 16 <= kTP, "tile layout");
constexpr int kUVBytes = 12 * kTP > kCV + 11 * kTP + 16 ? 12 * kTP : kCV + 11 * kTP + 16;  // chroma tile span
constexpr int kAbY = (kLfUV + kUVBytes + 15) & ~15;  // luma above row: [15] corner P, [16..31] A, [32..35] above-right
constexpr int kAbUV = kAbY + 48;   // chroma above rows: U P@7 A@8..15, V P@23 A@24..31
constexpr int kColY = kAbUV + 32;  // B_PRED: luma columns 11, 7, 3 of the MB (16 B each, in that order),
                                   // so that the left column of sub-block column j is at kLeft - 16 j
constexpr int kLeft = kColY + 48;  // unfiltered left columns: Y 0..15, U 16..23, V 24..31
constexpr int kResid = kLeft + 32;  // luma residual of the MB (for B_PRED): 16 blocks x 16 int16
constexpr int kWht = kResid + 512;  // 16 int16 luma DCs out of the inverse WHT
constexpr int kHalfBytes = kWht + 32;
constexpr int kWaveBytes = 2 * kHalfBytes;

// Workgroup header.
constexpr int kProgress = 0;      // 16 x u32 progress words (one per wave)
constexpr int kBpTable = 64;      // B_PRED predictor table: 11 modes x 16 px x {perm selectors, byte
                                  // mask, dot weights, bias}
constexpr int kBpModes = 11;      // modes 0..9 + one constant-128 entry for out-of-range modes
constexpr int kBpEntry = 16;      // bytes per (mode, pixel) entry
constexpr int kDqTable = kBpTable + kBpModes * 16 * kBpEntry;  // 4 segments x 6 int16 dequant factors
constexpr int kLfTable = kDqTable + 48;                 // 4 segments x 2 (B_PRED?) x {E, I, T, 0}
constexpr int kTabStride = 80;                          // per frame slot (chain mode: two slots, four interleaved)
constexpr int kTabSlots = 4;
constexpr int kMisc = kDqTable + kTabSlots * kTabStride;  // chain mode: list length
constexpr int kRoleTab = kMisc + 16;                    // whole-block predictor lane roles: 32 lanes x 8 B
constexpr int kHdrBytes = kRoleTab + 256;

// Shared per-MB-column context (one frame per workgroup).
constexpr int kCtxRecBytes = 32;   // unfiltered bottom row: Y 16, U 8, V 8 (intra prediction)
constexpr int kCtxLfBytes = 128;   // bottom 4 rows, filter state: Y 4x16, U 4x8, V 4x8 (loop filter)
constexpr int kCtxBytesPerCol = kCtxRecBytes + kCtxLfBytes;

constexpr int kMaxLds = 163840;

// Launch order (cost-balanced placement).  A frame's time is set by its size and by how much its
// loop filter filters (profiles/r02b_wave_placement.json: 4K frames at filter level 2 take 11.2 ms,
// at 40-63 14.8 ms); workgroups b and b + CUs share a CU.  cost_class is a coarse log2 of
// MBs x (64 + the frame's largest MB-edge limit 2E + I, halved for the simple filter): 4 classes
// per octave, 0..127, higher = heavier.
constexpr uint32_t kCostClasses = 128;
__host__ __device__ inline uint32_t cost_class(const Vp8gFrameDesc& d) {
	uint32_t s = 0;
	if (d.flags & VP8G_F_LOOPFILTER) {
		for (int g = 0; g < 4; g++)
			for (int b = 0; b < 2; b++) {
				const uint32_t v = 2u * d.lf[g][b][0] + d.lf[g][b][1];
				s = v > s ? v : s;
			}
		if (d.flags & VP8G_F_SIMPLE) s >>= 1;
	}
	const uint64_t cost = (uint64_t)d.mb_cols * d.mb_rows * (64u + s);  // < 2^27 for valid frames
	if (cost < 4u) return 0u;  // an empty (all-zero) descriptor: a no-op slot, the lightest class
	if (cost >= (1ull << 31)) return kCostClasses - 1u;
	const uint32_t lg = 63u - (uint32_t)__builtin_clzll(cost);
	return 4u * lg + (uint32_t)((cost >> (lg - 2u)) & 3u);
}

inline size_t lds_bytes(int waves, uint32_t ctx_cols, bool global_ctx) {
	return (size_t)kHdrBytes + (size_t)waves * kWaveBytes + (global_ctx ? 0 : (size_t)ctx_cols * kCtxBytesPerCol);
}
// Chain mode (batches of more frames than CUs): one 16-wave workgroup per CU decodes a list of frames,
// four MB rows per wave (the quad chain kernel, vp8g_quad.inc).  A wave's LDS is four
// quarter areas (the half layout without the iWHT scratch) and four 3-column context rings; the
// context between waves lives in device memory (the snapshot buffer, one region per frame), so the
// chain's LDS does not depend on the frame width.
constexpr int kQuarterBytes = kWht;                          // tile, borders, B_PRED buffers, residual park
constexpr int kRingBytes = 3 * kCtxBytesPerCol;              // three MB columns of context
constexpr int kQRings = kHdrBytes + 4 * kQuarterBytes;       // wave-relative: ring h at + h * kRingBytes
constexpr int kQWaveBytes = 4 * kQuarterBytes + 4 * kRingBytes;
constexpr int kQList = kHdrBytes + 16 * kQWaveBytes;         // the chain list (after 16 wave areas)
constexpr size_t kChainScratch = (size_t)16 * kQWaveBytes;  // the cost sort's scratch: the wave areas
inline size_t chain_lds_bytes(uint32_t list_max) { return (size_t)kQList + 4 * (size_t)list_max; }

// Record a HIP failure for vp8g_last_error() (calling thread).
void set_error_text(const char* where, hipError_t e);
inline int fail(int e) { return errno = e, -1; }

// What a stage of an end-to-end call returns: hipSuccess, or the HIP error and the step that met it (vp8g_last_error's
// text).  capi_status: of one of the library's C entry points, which leave HIP's error, if there was one, behind their
// -1; errno stays what the entry point left, for a caller that passes it on.
struct Status {
	hipError_t he = hipSuccess;
	const char* where = nullptr;
	bool ok() const { return he == hipSuccess; }
};
inline Status capi_status(int rc, const char* where) {
	if (rc == 0) return Status{};
	const int en = errno;
	const hipError_t e = hipGetLastError();
	errno = en;
	return Status{e == hipSuccess ? hipErrorInvalidValue : e, where};
}

// Offsets inside the device buffers of the end-to-end calls: every region starts on 256 bytes.
inline uint64_t al256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

int device_cus();  // the device's CU count; 0 = unknown
// The grid of a launch whose workgroups loop over `tasks`: per_cu workgroups for every CU, no more than there are tasks.
inline uint32_t grid_for(uint64_t tasks, uint32_t per_cu) {
	const int cus = device_cus();
	const uint64_t cap = (uint64_t)(cus > 0 ? cus : 256) * per_cu;
	return (uint32_t)(tasks < cap ? tasks : cap);
}

// Process-wide launch gate (vp8g_shim.hip).  Launch modes whose workgroups wait on each other across
// CUs -- split parts (Launch::parts > 1) and the chain's mirror split -- need every
// workgroup of the launch resident at once.  Beside another kernel of this library (an earlier
// asynchronous batch on another stream, a pipeline chunk, a device-m05 or writer kernel) some of
// them could wait for CUs that the others hold while they spin; two such launches side by side
// would both run into the bounded wait and fail with VP8G_ERR_TIMEOUT.  So every kernel launch of
// the library is enqueued inside a GateScope, which holds one process-wide mutex from the decision
// to the last enqueue:
//   * the scope's stream is first ordered after a cross-workgroup launch still in flight on
//     another stream (hipStreamWaitEvent), so nothing starts beside one;
//   * may_cross() is true only when no launch of the library is in flight on any other stream
//     (hipEventQuery of each stream's last recorded launch), so a cross-workgroup launch never
//     starts beside another kernel;
//   * done(crossed) records the launch's completion event for the next caller.
// Kernels launched by the caller's own code on other streams are outside the gate.
class GateScope {
   public:
	explicit GateScope(hipStream_t s);
	~GateScope();
	GateScope(const GateScope&) = delete;
	GateScope& operator=(const GateScope&) = delete;
	hipError_t status() const { return err_; }
	bool may_cross() const { return may_cross_; }
	hipError_t done(bool crossed);

   private:
	hipStream_t s_;
	hipError_t err_ = hipSuccess;
	bool may_cross_ = false;
};

// The rule above has one implementation for every launch that does not cross workgroups (the sink stages, device m05,
// the digests): `enqueue` (hipError_t(): each launch followed by hipGetLastError(), stopping at the first failure) runs
// inside a GateScope on `stream` -- gate status, the enqueues, the completion event.  `before` carries an error found ahead
// of the gate: the scope is still entered, nothing is enqueued, no event recorded.  0, or -1 with errno = EIO and
// `where` recorded for vp8g_last_error.  The launches that may cross (run_locked in the shim, Pipeline::launch_recon)
// read may_cross() and hold their own scope.
template <class F>
int gated_launch(hipStream_t stream, const char* where, F&& enqueue, hipError_t before = hipSuccess) {
	hipError_t e;
	{
		GateScope gate(stream);
		e = before != hipSuccess ? before : gate.status();
		if (e == hipSuccess) e = enqueue();
		if (e == hipSuccess) e = gate.done(false);
	}
	if (e == hipSuccess) return 0;
	set_error_text(where, e);
	return fail(EIO);
}

// ---- Which kernel a batch runs on (vp8g_plan.hip) --------------------------------
// The launch switches.  knobs_from_env reads all six from the environment on every call (so a
// process may change them between calls: tests/test_gpu_split.py), over the compile-time defaults
// (vp8g_plan.hip: VP8G_CHAIN_DEFAULT, VP8G_SPLITCHAIN_DEFAULT, VP8G_CHAIN_IL_DEFAULT, VP8G_NO_ORDER,
// VP8G_FORCE_GCTX).
struct Knobs {
	uint32_t split;   // VP8G_SPLIT=<k>: workgroups per frame (1 = never split; 0 / unset: automatic)
	uint32_t waves;   // VP8G_WAVES=<w>: waves per frame workgroup where the caller gives no hint
	int chain;        // VP8G_CHAIN=0: never the chain; 1: also for batches of at most the CU count; -1: automatic
	int splitchain;   // VP8G_SPLITCHAIN=0 / 1: the mirror split never / wherever it fits; -1: automatic
	int chain_il;     // VP8G_CHAIN_IL=0: the two-frame interleave never; else wherever it fits
	bool order;       // VP8G_ORDER=0 clears it: launch in batch order, no cost-class placement
	bool force_gctx;  // (build switch only) the frame kernel's column context in device memory always
};
extern const Knobs kDefaultKnobs;
Knobs knobs_from_env();

// What the two callers of plan_launch do differently (DESIGN.md §3.3 has the history of each).
struct LaunchPolicy {
	bool may_split;         // split parts without VP8G_SPLIT > 1: the call is synchronous (the host APIs) / the call's only chunk
	bool hint_plain;        // a non-zero wave hint means exactly that: no split parts, no chain
	bool env_geometry;      // honours Knobs::split, waves and force_gctx
	bool split_waves_stay;  // the gate refuses split parts: the whole-frame launch keeps their 8 waves
	bool placement;         // whole-frame launches of more frames than CUs are placed by cost class
	bool chain_extras;      // the chain may take the mirror split or the interleave
	bool snap_in_gctx;      // the chain's snapshots live in the global-context buffer (no buffer of their own)
};
constexpr LaunchPolicy kReferencePolicy = {true, true, true, false, true, true, false};   // vp8g_shim.hip (may_split: see run_locked)
constexpr LaunchPolicy kPipelinePolicy = {true, true, false, true, false, false, true};   // vp8g_pipeline.hip

// One launch: frame_kernel<waves, gctx, parts > 1> over `workgroups` = n * parts workgroups, or the
// quad chain kernel (vp8g_quad.inc) over one 16-wave workgroup per CU.
struct Launch {
	bool quad;        // the quad chain kernel, else the frame kernel
	bool gctx;        // frame kernel: the variant whose per-column context lives in device memory (frames too wide for LDS)
	bool ordered, split, interleave;  // chain: placed by cost class; mirror split (kSegTop); two frames interleaved
	bool whole;       // chain: every frame has whole, aligned 16-B / 8-B row pieces -- the lean instantiation (the
	                  // general one adds a byte path for pieces cut by the right edge or unaligned planes)
	uint32_t waves;   // per workgroup
	uint32_t parts;   // frame kernel: workgroups per frame, handing off through mailboxes (8 or 16 waves, LDS context only)
	uint32_t workgroups;
	// ord_first = F != 0 (whole-frame launches of more than F frames): workgroup w decodes the frame at
	// position p(w) of the batch sorted by descending cost_class (stable): the first F workgroups the F
	// heaviest frames, the next S = min(n - F, F) the S lightest in reverse (so the heaviest frame
	// shares its CU with the lightest), the rest the middle positions heaviest first.  F = the CU count.
	uint32_t ord_first;
	uint32_t lds;     // dynamic LDS bytes
	uint32_t mode;    // VP8G_MODE_* (vp8g_last_launch_mode)
	bool crosses() const { return parts > 1 || split; }  // workgroups wait on each other across CUs (GateScope)
};
// Both outcomes of the launch gate, decided before it (so nothing is allocated inside it), and the
// bytes the auxiliary buffers must hold for either.  Inside the gate, resolve() is all that is left.
struct LaunchPlan {
	uint32_t n, ctx_cols, max_rows;  // frames; the largest MB columns / rows of the batch
	Launch open, shut;               // the gate allows a cross-workgroup launch / does not
	size_t gctx_bytes;   // every frame's column context (n * ctx_cols * kCtxBytesPerCol)
	size_t mbox_bytes;   // split parts: parts mailboxes per frame, each one frame's column context ...
	size_t gprog_bytes;  // ... and one progress word per part, zeroed before the launch
	size_t snap_bytes;   // chain: every frame's context between waves, and with it the mirror split's snapshots
	size_t flags_bytes;  // mirror split: one word per frame, none equal to the launch's epoch before it
	const Launch& resolve(bool may_cross) const { return may_cross ? open : shut; }
};
// Pure: no HIP call, no environment.  n_cus: the device's CU count (device_cus(); 0 = unknown: eight
// waves, no chain, no split).  out_aligned: the output base is 16-byte aligned (else no `whole`).
LaunchPlan plan_launch(const Vp8gFrameDesc* h_descs, uint32_t n, int n_cus, bool out_aligned, uint32_t waves_hint, const Knobs& knobs,
                       const LaunchPolicy& policy);

constexpr uint32_t kMaxSplit = 8;

// The buffers a launch may use (device pointers; those the plan sized as 0 bytes may be null).
struct LaunchBuffers {
	uint8_t* gctx;
	uint8_t* mbox;
	uint32_t* gprog;
	uint8_t* snap;  // (LaunchPolicy::snap_in_gctx: the caller passes its global-context buffer here as well)
	uint32_t* flags;
	uint32_t epoch;  // mirror split: this launch's counter value for `flags`
};
// Enqueue launch L of plan P (inside a GateScope).
hipError_t launch(const LaunchPlan& P, const Launch& L, const Vp8gFrameDesc* d_descs, const Vp8gBatchArrays& arrays, uint8_t* d_out,
                  const LaunchBuffers& b, hipStream_t stream);

// vp8g_make_frame_desc; dense_coeffs = false skips the check of the coeff_* pointers (packed
// frames: the coefficients reach the device through the expansion kernel).
int make_desc(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* d, int filtered, uint64_t mb_offset, uint64_t out_offset,
              Vp8gFrameDesc* out, bool dense_coeffs);

// Planes in the yuv420_alloc layout; init = false leaves them uninitialised (outputs a D2H
// overwrites completely).
int alloc_planes(Yuv420Image* img, uint32_t width, uint32_t height, bool init);

// The end-to-end pipeline (vp8g_pipeline.hip) over pictures that are already located in their files (WebPStill,
// host/vp8_front.h; every one a good record, its `size` what the batch planner prices it at): otherwise
// vp8g_decode_webp_batch_tensor_any without options, xflags VP8G_X_ALPHA | VP8G_X_LOSSLESS.  Not exported.
int decode_located_tensor(const WebPStill* pics, uint32_t n, int filtered, uint32_t threads, uint32_t flags, const Vp8gTensorOpt* t,
                          uint32_t xflags, void* d_out, int* status);

}  // namespace vp8g
