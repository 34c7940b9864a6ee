// vp8g_pipeline.hip -- end-to-end batch decode: .webp bytes in host memory -> I420 images in host memory, or
// pictures in the caller's device tensor (vp8g_decode_webp_batch and its kin, include/vp8g.h).
//
//   decode_batch     locates every file's payloads once (webp_locate_still, host/vp8_front.h) in the mode the entry
//                    point implies; every stage below reads that record, or the errno of the refusal
//   worker threads   key-frame header + m05 (host/vp8_parse.c, reentrant) into the packed wire format (and
//                    the ALPH chunk's entropy decode, if alpha is asked for), frames handed out in order from an
//                    atomic counter and kept at most a window ahead of the device
//   this thread      groups finished frames into chunks and takes each through the stages of Pipeline: H2D of the
//                    side arrays, block masks and non-zero values (~5x less than dense int16), expansion to the dense
//                    SoA, the fused recon(+LF) kernel, then the call's sinks -- crop / rescale, alpha un-prediction, the
//                    tensor kernel -- and D2H of what the caller gets in host memory.  Chunk slots alternate (two per
//                    chunk kind), so one chunk's device work and copies overlap the entropy decoding of the next ones.
//
// With VP8G_BATCH_DEVICE_M05 the workers only parse the frame header and the first partition's
// frame-level fields (vp8f_token_header); the chunk uploads the compressed VP8 payloads themselves and m05 runs
// on the device (vp8g_m05.hip, one workgroup per frame) straight into the dense SoA -- except for the heaviest frames,
// which plan_frames leaves to the host threads.
// The reference decodes one file per process (src/main.c:591-705: m01..m05 then m06/m07); its
// m05 keeps global state (vp8_tokens.c:382, :625), which is why it cannot be threaded as is.
#include <errno.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../host/vp8_front.h"
#include "vp8g_argb_batch.h"
#include "vp8g_device.h"

#define VP8G_API extern "C" __attribute__((visibility("default")))

namespace {

using vp8g::al256;
using vp8g::ArgbScaleBatch;
using vp8g::capi_status;
using vp8g::Status;

constexpr uint32_t kChunkFrames = 32;          // frames per host-m05 chunk (at most; tools/chunk_sweep.py: 32 shortens the tail)
constexpr uint64_t kChunkMbs = 2u << 20;       // macroblocks per chunk (at most, unless one frame is bigger)
// device m05: one workgroup per frame and a chunk's m05 time is its slowest frame's, so a chunk
// wants as many frames as the chip runs at once (~1500 at full scalar-unit load): 1024 4K frames,
// ~1.2 KB of device buffers per MB (coefficients, side arrays, I420 out) = ~41 GB per slot
constexpr uint32_t kTokChunkFrames = 1024;
constexpr uint64_t kTokChunkMbs = 34u << 20;
constexpr uint32_t kNb = VP8G_PK_BLOCKS;

// Packed -> dense coefficients.  32 lanes per MB; lane b < 25 owns block b (Y 0..15, U 0..3,
// V 0..3, Y2).  Its values start at the MB's offset plus the popcounts of the blocks before it
// (a 32-lane inclusive scan); position i takes value rank popcount(mask & ((1 << i) - 1)).
__global__ __launch_bounds__(256) void expand_kernel(const uint16_t* __restrict__ masks, const uint32_t* __restrict__ mb_off,
                                                     const int16_t* __restrict__ vals, uint32_t n_mb, int16_t* __restrict__ cy,
                                                     int16_t* __restrict__ cu, int16_t* __restrict__ cv,
                                                     int16_t* __restrict__ cy2) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	const uint32_t mb = t >> 5, b = t & 31u;
	if (mb >= n_mb) return;  // whole 32-lane groups leave together
	const uint32_t m = b < kNb ? masks[(size_t)mb * kNb + b] : 0u;
	const uint32_t cnt = __popc(m);
	uint32_t incl = cnt;
#pragma unroll
	for (int d = 1; d < 32; d <<= 1) {
		const uint32_t v = __shfl_up(incl, (unsigned)d, 32);
		if (b >= (uint32_t)d) incl += v;
	}
	if (b >= kNb) return;
	const int16_t* src = vals + mb_off[mb] + (incl - cnt);
	uint32_t w[8];
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const uint32_t k0 = 2 * i, k1 = 2 * i + 1;
		uint32_t lo = 0, hi = 0;
		if ((m >> k0) & 1u) lo = (uint16_t)src[__popc(m & ((1u << k0) - 1u))];
		if ((m >> k1) & 1u) hi = (uint16_t)src[__popc(m & ((1u << k1) - 1u))];
		w[i] = lo | (hi << 16);
	}
	int16_t* dst = b < 16u   ? cy + ((size_t)mb * 16u + b) * 16u
	               : b < 20u ? cu + ((size_t)mb * 4u + (b - 16u)) * 16u
	               : b < 24u ? cv + ((size_t)mb * 4u + (b - 20u)) * 16u
	                         : cy2 + (size_t)mb * 16u;
	uint4* d4 = (uint4*)dst;
	d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
	d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// bitstream slot of a payload: 16-B aligned start, >= 512 bytes of slack (the device bool
// decoder loads its 256-byte windows one ahead, up to 512 bytes past a partition's end)
inline uint64_t bits_slot(uint32_t psize) { return ((uint64_t)psize + 512u + 15u) & ~(uint64_t)15u; }

// Host half of a device-m05 frame.
struct TokJob {
	Vp8KeyFrameHeader kf;
	Vp8DecodedFrame hdr;  // header fields only (no arrays)
	Vp8gTokFrame tf;
};

// The library's one background releaser of host frames (the last chunks' packed frames, freed
// after a call returns: see defer_release).  Owned, and joined when the library is unloaded or
// the process exits, so no thread runs library code after that.
struct Freer {
	std::mutex mu;
	std::condition_variable cv;
	std::vector<std::vector<Vp8gPackedFrame>> q;
	std::vector<std::vector<Vp8fLosslessImage>> ql;  // lossless frames' residual images and transform data
	bool stop = false;
	std::thread th;
	void post(std::vector<Vp8gPackedFrame>&& v) {
		std::lock_guard<std::mutex> lk(mu);
		if (!th.joinable()) th = std::thread([this] { run(); });
		q.push_back(std::move(v));
		cv.notify_one();
	}
	void post(std::vector<Vp8fLosslessImage>&& v) {
		std::lock_guard<std::mutex> lk(mu);
		if (!th.joinable()) th = std::thread([this] { run(); });
		ql.push_back(std::move(v));
		cv.notify_one();
	}
	void run() {
		std::unique_lock<std::mutex> lk(mu);
		for (;;) {
			cv.wait(lk, [this] { return stop || !q.empty() || !ql.empty(); });
			if (q.empty() && ql.empty()) return;  // (stop with nothing queued)
			std::vector<Vp8gPackedFrame> v;
			std::vector<Vp8fLosslessImage> vl;
			if (!q.empty()) v = std::move(q.back()), q.pop_back();
			else vl = std::move(ql.back()), ql.pop_back();
			lk.unlock();
			for (Vp8gPackedFrame& p : v) vp8f_packed_free(&p);
			for (Vp8fLosslessImage& im : vl) vp8f_lossless_free(&im);
			lk.lock();
		}
	}
	~Freer() {
		{
			std::lock_guard<std::mutex> lk(mu);
			stop = true;
		}
		cv.notify_one();
		if (th.joinable()) th.join();
	}
};
Freer g_freer;

uint32_t default_threads() {
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0) {
		const int n = CPU_COUNT(&set);
		if (n > 0) return (uint32_t)n;
	}
	const unsigned h = std::thread::hardware_concurrency();
	return h ? h : 1u;
}

// Frames handed from the workers to the device thread, in the order `order` (positions), each
// either decoded on the host into the packed format or only header-parsed for device m05 (dev[i]).
struct Feed {
	const WebPStill* pics = nullptr;  // the located pictures ...
	const int* refused = nullptr;     // ... or (not NULL, not 0) the errno with which a file's container was refused
	uint32_t n = 0;
	std::vector<uint8_t> dev;       // frame i: m05 on the device (workers fill tj[i], else pk[i])
	std::vector<uint32_t> order;    // position -> frame index
	unsigned fflags = 0;  // front-end flags (VP8F_MULTI_PARTITION)
	bool alpha = false;             // also entropy-decode the ALPH chunk, if there is one (VP8G_X_ALPHA): ares[i] = the residual plane
	std::vector<uint8_t*> ares;     // (malloc; NULL = no alpha; freed with the frame's host data)
	std::vector<uint32_t> afilter;
	std::vector<uint8_t> is_ll;     // frame i is lossless (VP8G_X_LOSSLESS; it has no kf / pk / tj; it rides in the chunk its position falls in)
	std::vector<Vp8fLosslessImage> ll;  // (freed with the frame's host data)
	std::vector<Vp8gPackedFrame> pk;
	std::vector<TokJob> tj;
	std::vector<int> err;
	std::unique_ptr<uint8_t[]> ready;
	std::atomic<uint32_t> next{0};
	uint32_t limit = 0;  // workers may start positions < limit (guarded by mu)
	bool abort = false;
	std::mutex mu;
	std::condition_variable cv_ready, cv_limit;

	void work() {
		for (;;) {
			const uint32_t pos = next.fetch_add(1);
			if (pos >= n) return;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_limit.wait(lk, [&] { return pos < limit || abort; });
				if (abort) return;
			}
			const uint32_t i = order[pos];
			const int e = decode(i);
			{
				std::lock_guard<std::mutex> lk(mu);
				err[i] = e;
				ready[i] = 1;
			}
			cv_ready.notify_all();
		}
	}
	// The host's share of picture i, from its located payloads: 0, or the errno with which the picture fails.
	int decode(uint32_t i) {
		const WebPStill& p = pics[i];
		if (refused && refused[i]) return refused[i];
		if (p.vp8l_offset) {
			is_ll[i] = 1;
			return vp8f_lossless_decode(p.data + p.vp8l_offset, p.vp8l_size, &ll[i], nullptr) == 0 ? 0 : errno ? errno : EINVAL;
		}
		const ByteSpan payload = {p.data + p.vp8_offset, p.vp8_size};
		if (dev[i] && p.vp8_size > 0xFFFFFFF0u) return EFBIG;  // (a payload's bitstream slot is sized in 32 bits)
		if (dev[i] ? vp8f_token_header(payload, &tj[i].kf, &tj[i].hdr, &tj[i].tf, fflags) : vp8f_decode_packed(payload, &pk[i], fflags))
			return errno ? errno : EINVAL;
		if (!alpha || !p.alph_offset) return 0;
		const Vp8KeyFrameHeader& kf = dev[i] ? tj[i].kf : pk[i].kf;
		ares[i] = (uint8_t*)malloc((size_t)kf.width * kf.height);
		if (!ares[i]) return ENOMEM;
		if (vp8f_alpha_decode(p.data + p.alph_offset, p.alph_size, kf.width, kf.height, ares[i], &afilter[i], nullptr) == 0) return 0;
		const int e = errno ? errno : EINVAL;  // a picture whose ALPH does not decode fails as a whole, as in libwebp
		free(ares[i]);
		ares[i] = nullptr;
		return e;
	}
	void wait_ready(uint32_t i) {
		std::unique_lock<std::mutex> lk(mu);
		cv_ready.wait(lk, [&] { return ready[i] != 0; });
	}
	void set_limit(uint32_t l) {
		{
			std::lock_guard<std::mutex> lk(mu);
			if (l > limit) limit = l;
		}
		cv_limit.notify_all();
	}
	void stop() {
		{
			std::lock_guard<std::mutex> lk(mu);
			abort = true;
		}
		cv_limit.notify_all();
	}
};

// One chunk's device buffer and the host state that must live until its copies are done.
struct D2H {
	void* dst;
	const void* src;
	size_t bytes;
};
struct Slot {
	uint8_t* buf = nullptr;
	size_t cap = 0;
	hipEvent_t done = nullptr;     // the chunk's D2H finished (copy stream)
	hipEvent_t kdone = nullptr;    // the chunk's kernels finished (compute stream)
	bool busy = false;
	std::vector<uint32_t> frames;  // frame indices of the chunk (packed data freed when the slot is reused)
	std::vector<Vp8gFrameDesc> descs;
	std::vector<Vp8gScaleDesc> sdescs;  // scaled decode: one per frame of the chunk
	std::vector<Vp8gTensorDesc> tdescs;  // tensor sink: one per frame of the chunk
	std::vector<Vp8gAlphaDesc> adescs;   // alpha sink: the chunk's frames that have an ALPH plane
	std::vector<Vp8gScaleDesc> asdescs;  //   their alpha planes through the rescaler
	std::vector<Vp8gTensorAlpha> talpha; //   one per tensor descriptor
	std::vector<Vp8gTensorDesc> tdescs444;   // libwebp's scaled RGB (Sinks::rgb_scale): the frames whose planes are 4:4:4,
	std::vector<Vp8gTensorAlpha> talpha444;  //   a launch of their own
	std::vector<Vp8gLosslessDesc> ldescs;     // lossless sink: the chunk's lossless frames
	ArgbScaleBatch lbatch;                    //   their way into the tensor, cropped / rescaled (VP8G_X_LOSSLESS_SCALE) or as they are
	std::vector<Vp8gTokFrame> jobs;  // device m05
	uint32_t status = 0;
	std::vector<D2H> d2h;          // the chunk's downloads (issued by a Copier)
	bool issued = false;           // the Copier has issued them and recorded `done` (guarded by its mutex)
	hipError_t copy_err = hipSuccess;
};

// Downloads into the callers' images are pageable-memory copies, which HIP completes
// synchronously in the calling thread -- after waiting for the chunk's kernels.  Issued from
// the thread that launches chunks, one long device-m05 chunk's download would hold up every
// later launch (host-m05 chunks that are ready, the next device chunk).  Each Copier owns a
// thread and a stream and issues the downloads of the chunks queued to it, in order.
struct Copier {
	std::thread th;
	std::mutex mu;
	std::condition_variable cv;
	std::vector<Slot*> q;
	size_t head = 0;
	bool quit = false;
	hipStream_t stream = nullptr;

	void run() {
		for (;;) {
			Slot* s;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return head < q.size() || quit; });
				if (quit) return;
				s = q[head++];
			}
			// fresh output images fault their pages in during the copy, one 4-KB page at a time in
			// this thread; populate them first, while the chunk's kernels still run
			for (const D2H& c : s->d2h) prefault(c.dst, c.bytes);
			hipError_t e = hipStreamWaitEvent(stream, s->kdone, 0);
			for (const D2H& c : s->d2h)
				if (e == hipSuccess) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream);
			if (e == hipSuccess) e = hipEventRecord(s->done, stream);
			{
				std::lock_guard<std::mutex> lk(mu);
				s->issued = true;
				s->copy_err = e;
			}
			cv.notify_all();
		}
	}
	static void prefault(void* p, size_t bytes) {
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
		static const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
		const uintptr_t a = ((uintptr_t)p + pg - 1) & ~(pg - 1), e = ((uintptr_t)p + bytes) & ~(pg - 1);
		if (e > a) (void)madvise((void*)a, e - a, MADV_POPULATE_WRITE);  // (best effort: older kernels say EINVAL)
	}
	void push(Slot* s) {
		{
			std::lock_guard<std::mutex> lk(mu);
			s->issued = false;
			q.push_back(s);
		}
		cv.notify_all();
	}
	hipError_t wait_issued(Slot* s) {
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&] { return s->issued; });
		return s->copy_err;
	}
	void stop() {
		{
			std::lock_guard<std::mutex> lk(mu);
			quit = true;
		}
		cv.notify_all();
		if (th.joinable()) th.join();
	}
};

struct ChunkLayout {
	uint64_t ym, uvm, seg, hasc, bm, masks, mboff, vals, cy, cu, cv, cy2, bits, jobs, desc, status, gctx, mbox, gprog, out,
	    sdesc, sout, tdesc, ares, aout, asout, adesc, asdesc, talpha, lsrc, lout, ldesc, ltdesc, lswork, lsout,
	    lsdesc, total;
};

hipError_t grow(Slot& s, size_t need) {
	if (need <= s.cap) return hipSuccess;
	if (s.buf) (void)hipFree(s.buf);
	s.buf = nullptr;
	s.cap = 0;
	const size_t n = need + need / 4;
	hipError_t e = hipMalloc((void**)&s.buf, n);
	if (e == hipSuccess) s.cap = n;
	return e;
}

// A batch's files located, each once, under `accept` (webp_locate_still): the records, and per file 0 or the errno with
// which its container was refused.
struct LocatedFiles {
	std::vector<WebPStill> pics;
	std::vector<int> refused;
	LocatedFiles(const ByteSpan* files, uint32_t n, unsigned accept) : pics(n), refused(n, 0) {
		for (uint32_t i = 0; i < n; i++)
			if (webp_locate_still(files[i], accept, &pics[i]) != 0) refused[i] = errno ? errno : EINVAL;
	}
};

// Which frames run m05 on the device and in which order the workers take them.  Without
// VP8G_BATCH_DEVICE_M05 every frame is decoded on the host, in index order.  With it the device
// runs m05 as one workgroup per frame, so the device part lasts as long as its heaviest frame
// (latency ~ kDevNsPerByte x payload bytes) plus the download of all its images, while the host
// threads would otherwise only parse headers.  So the heaviest frames go to the host threads
// (~ kHostNsPerByte x bytes each, `threads` at a time): the k heaviest, for the k that minimises
// max(host time, device time) (VP8G_HYBRID=0 turns this off).  Device frames come
// first, so their chunk launches while the host threads decode the heavy ones.
constexpr double kDevNsPerByte = 850.0;    // device m05 latency per payload byte, 4K fixtures
constexpr double kHostNsPerByte = 50.0;    // host m05 into the packed format, per payload byte and thread
constexpr double kD2HNsPerByte = 0.085;    // download into fresh pageable images (~12 GB/s)
// (rates measured on the box: tools/e2e_probe.py chunk traces, tools/hybrid_sweep.py; profiles/r02_hybrid.json)
// download = false (the tensor sink: the pictures stay on the device) prices no download.
// A file is priced by its size (pics[i].size, whatever became of its container) and its picture's I420 bytes.
void plan_frames(const WebPStill* pics, const int* refused, uint32_t n, bool tok, uint32_t threads, std::vector<uint8_t>& dev,
                 std::vector<uint32_t>& order, bool download) {
	dev.assign(n, tok ? 1 : 0);
	order.resize(n);
	for (uint32_t i = 0; i < n; i++) order[i] = i;
	const char* hv = getenv("VP8G_HYBRID");
	if (!tok || (hv && atoi(hv) == 0)) return;
	double dev_per_b = kDevNsPerByte, host_per_b = kHostNsPerByte, d2h_per_b = kD2HNsPerByte;
	if (const char* e = getenv("VP8G_DEV_NS_PER_BYTE")) dev_per_b = atof(e);  // calibration knobs
	if (const char* e = getenv("VP8G_HOST_NS_PER_BYTE")) host_per_b = atof(e);
	if (const char* e = getenv("VP8G_D2H_NS_PER_BYTE")) d2h_per_b = atof(e);
	if (!download) d2h_per_b = 0.0;
	std::vector<double> outb(n, 0.0);  // I420 bytes (0 for a file whose header does not parse: it fails anyway)
	for (uint32_t i = 0; i < n; i++)
		if (!(refused && refused[i]) && pics[i].vp8_offset && pics[i].width)  // (0 x 0: the simple layout with a bad frame header)
			outb[i] = (double)vp8g_i420_size(pics[i].width, pics[i].height);
	const auto size_of = [&](uint32_t i) { return (double)pics[i].size; };
	std::vector<uint32_t> by_size(order);
	std::stable_sort(by_size.begin(), by_size.end(), [&](uint32_t x, uint32_t y) { return pics[x].size > pics[y].size; });
	double dev_out = 0;
	for (uint32_t i = 0; i < n; i++) dev_out += outb[i];
	const double thr = threads ? (double)threads : 1.0;
	double host_ns = 0, best = dev_per_b * size_of(by_size[0]) + d2h_per_b * dev_out;
	uint32_t best_k = 0;
	for (uint32_t k = 1; k <= n; k++) {  // the k heaviest on the host
		const uint32_t f = by_size[k - 1];
		host_ns += host_per_b * size_of(f) / thr;
		dev_out -= outb[f];
		const double dev_ns = (k < n ? dev_per_b * size_of(by_size[k]) : 0.0) + d2h_per_b * dev_out;
		const double t = host_ns > dev_ns ? host_ns : dev_ns;
		if (t < best) best = t, best_k = k;
	}
	for (uint32_t k = 0; k < best_k; k++) dev[by_size[k]] = 0;
	uint32_t p = 0;
	for (uint32_t i = 0; i < n; i++)
		if (dev[i]) order[p++] = i;
	for (uint32_t k = 0; k < n; k++)
		if (!dev[by_size[k]]) order[p++] = by_size[k];
}

// Where a call's pictures go, and what happens to them on the way (one per entry point).
struct Sinks {
	const Vp8gScaleOpt* opts = nullptr;   // crop / rescale on the device (vp8g_scale.hip): one for all frames or one each
	uint32_t n_opts = 0;
	Yuv420Image* outs = nullptr;          // I420 images in host memory, or (outs = NULL) ...
	const Vp8gTensorOpt* topt = nullptr;  // ... the slots of the caller's device tensor (vp8g_tensor.hip)
	uint8_t* d_tensor = nullptr;
	bool extended = false;                // the extended container (VP8X) in front
	bool alpha = false;                   // VP8G_X_ALPHA: ALPH planes become the tensor's fourth channel
	bool lossless = false;                // VP8G_X_LOSSLESS: lossless files decode as well (vp8g_lossless.hip)
	bool lossless_scale = false;          // VP8G_X_LOSSLESS_SCALE: ... and are cropped / rescaled (vp8g_scale_argb.hip)
	bool rgb_scale = false;               // vp8g_decode_webp_batch_tensor_rgb: a lossy frame with a target size gets libwebp's RGB
	uint64_t tslot = 0;                   // bytes per tensor slot (decode_batch fills it in)
	const Vp8gScaleOpt* opt_of(uint32_t i) const { return opts ? &opts[n_opts == 1 ? 0 : i] : nullptr; }
	// Whether lossy frame i is rescaled as libwebp rescales for RGB output: Y, U and V each to the target
	// size (vp8g_make_scale_desc_444), for the tensor kernel's 4:4:4 mode.  Only with a target size: a crop alone is the
	// fancy upsampler on the window in libwebp too, the 4:2:0 route.
	bool yuv444(uint32_t i) const { return rgb_scale && opts && (opt_of(i)->scaled_w | opt_of(i)->scaled_h) != 0; }
};

// Device bytes per macroblock at which the memory budget prices a chunk.  Either kind holds per MB (ChunkLayout) ymode,
// uv_mode, segment_id, has_coeff (4 bytes), bmode (16), the dense coefficients cy, cu, cv, cy2 (512 + 128 + 128 + 32) and
// the I420 output (384): 1204 bytes.  A host-m05 chunk adds the block masks (kNb * 2 = 50), mb_off (4) and its packed
// values, priced at 278 bytes (139 values); a device-m05 chunk adds its payloads' bitstream slots, priced at 127 bytes.
constexpr uint64_t kPkBytesPerMb = 1536, kTokBytesPerMb = 1331;
// what a frame holds beyond that (a scaled picture larger than the frame, alpha planes), in MBs of the chunk budget
inline uint64_t extra_mbs(uint64_t bytes) { return (bytes + kPkBytesPerMb - 1) / kPkBytesPerMb; }

// Macroblocks per chunk (at most), by kind: [0] host m05, [1] device m05.  Four chunk slots, two per kind, stay
// within ~3/8 of the free device memory, so a device shared with other work gets smaller chunks instead of a failed
// allocation (EIO for every frame); the device-m05 slots get what the (small) host-m05 slots leave.
struct MbCaps { uint64_t mbs[2]; };
MbCaps chunk_budget(size_t free_bytes) {
	MbCaps c{{kChunkMbs, kTokChunkMbs}};
	if (!free_bytes) return c;  // (unknown: the defaults)
	const uint64_t budget = (uint64_t)free_bytes / 8u * 3u;
	const uint64_t floor_mbs = 1u << 15;  // one 4K frame and change
	const uint64_t cap_pk = budget / (4u * kPkBytesPerMb);
	if (cap_pk < c.mbs[0]) c.mbs[0] = cap_pk > floor_mbs ? cap_pk : floor_mbs;
	const uint64_t pk_bytes = 2u * c.mbs[0] * kPkBytesPerMb;
	const uint64_t cap_tok = budget > pk_bytes ? (budget - pk_bytes) / (2u * kTokBytesPerMb) : 0u;
	if (cap_tok < c.mbs[1]) c.mbs[1] = cap_tok > floor_mbs ? cap_tok : floor_mbs;
	return c;
}

// What a chunk's frames add up to: the sizes its buffer is laid out from.
struct ChunkShape {
	uint32_t nf = 0, max_cols = 0, max_rows = 0;
	uint64_t mbs = 0, vals = 0, bitsb = 0;          // macroblocks; packed values (host m05); bitstream slots (device m05)
	uint64_t outb = 0, soutb = 0, ab = 0, asb = 0;  // bytes of I420, scaled I420 (or 4:4:4 planes: 3 w h), alpha planes, scaled alpha planes
	uint32_t nl = 0;                                // lossless frames
	uint64_t lsrcb = 0, loutb = 0;                  // bytes of their residual images + transform data, of their ARGB pictures
	uint32_t nls = 0;                               // those of them that are cropped / rescaled
	uint64_t lsworkb = 0, lsoutb = 0;               // bytes of their planes in the rescaler's work buffer, of their scaled pictures
};

ChunkLayout make_layout(const ChunkShape& sh, bool tok, const Sinks& sk, const vp8g::LaunchPlan& plan) {
	const uint64_t mbs = sh.mbs, nf = sh.nf;
	ChunkLayout L;
	uint64_t o = 0;
	L.ym = o, o = al256(o + mbs);
	L.uvm = o, o = al256(o + mbs);
	L.seg = o, o = al256(o + mbs);
	L.hasc = o, o = al256(o + mbs);
	L.bm = o, o = al256(o + mbs * 16);
	L.masks = o, o = al256(o + (tok ? 0 : mbs * kNb * 2));
	L.mboff = o, o = al256(o + (tok ? 0 : mbs * 4));
	L.vals = o, o = al256(o + (tok ? 0 : sh.vals * 2 + 64));  // +64: the expansion may address one past the end
	L.cy = o, o = al256(o + mbs * 512);
	L.cu = o, o = al256(o + mbs * 128);
	L.cv = o, o = al256(o + mbs * 128);
	L.cy2 = o, o = al256(o + mbs * 32);
	L.bits = o, o = al256(o + sh.bitsb);
	L.jobs = o, o = al256(o + (tok ? nf * sizeof(Vp8gTokFrame) : 0));
	L.desc = o, o = al256(o + nf * sizeof(Vp8gFrameDesc));
	L.status = o, o = al256(o + 4);
	// (every frame's column context: the global-context variant for frames too wide for LDS, and
	// the quad chain kernel, whose rows hand over through device memory)
	L.gctx = o, o = al256(o + nf * sh.max_cols * vp8g::kCtxBytesPerCol);
	L.mbox = o, o = al256(o + plan.mbox_bytes);
	L.gprog = o, o = al256(o + plan.gprog_bytes);
	L.out = o, o = al256(o + sh.outb);
	L.sdesc = o, o = al256(o + (sk.opts ? nf * sizeof(Vp8gScaleDesc) : 0));
	L.sout = o, o = al256(o + sh.soutb);
	L.tdesc = o, o = al256(o + (sk.topt ? nf * sizeof(Vp8gTensorDesc) : 0));
	L.ares = o, o = al256(o + sh.ab);
	L.aout = o, o = al256(o + sh.ab);
	L.asout = o, o = al256(o + sh.asb);
	L.adesc = o, o = al256(o + (sk.alpha ? nf * sizeof(Vp8gAlphaDesc) : 0));
	L.asdesc = o, o = al256(o + (sk.alpha ? nf * sizeof(Vp8gScaleDesc) : 0));
	L.talpha = o, o = al256(o + (sk.alpha ? nf * sizeof(Vp8gTensorAlpha) : 0));
	L.lsrc = o, o = al256(o + sh.lsrcb);
	L.lout = o, o = al256(o + sh.loutb);
	L.ldesc = o, o = al256(o + sh.nl * sizeof(Vp8gLosslessDesc));
	L.ltdesc = o, o = al256(o + sh.nl * sizeof(Vp8gTensorArgbDesc));
	L.lswork = o, o = al256(o + ArgbScaleBatch::head_bytes(sh.nls) + sh.lsworkb);
	L.lsout = o, o = al256(o + sh.lsoutb);
	L.lsdesc = o, o = al256(o + sh.nls * sizeof(Vp8gScaleArgbDesc));
	L.total = o;
	return L;
}

// One chunk on its way through the stages: the positions [a, b) of the feed's order, all of one kind, of which
// idx are the frames that decode (chunk position j = frame idx[j]), in slot `s` on its stream.
struct Chunk {
	bool tok;  // device m05
	uint32_t a, b;
	Slot& s;
	hipStream_t stream;
	std::vector<uint32_t> idx;
	std::vector<uint32_t> lidx;  // the chunk's lossless frames (not in idx: they have no macroblocks and skip every stage but their own)
	ChunkShape sh;
	vp8g::LaunchPlan plan = {};  // the recon launch, for either outcome of the launch gate
	ChunkLayout L;
	std::vector<uint32_t> sj;             // chunk position of each scale descriptor
	std::vector<uint8_t> s444;            //   ... and whether it is a 4:4:4 one (Sinks::yuv444)
	std::vector<Vp8gTensorAlpha> aplane;  // per chunk position: where the tensor kernel finds the frame's alpha
	hipError_t up_err = hipSuccess;
	// H2D onto the chunk's stream, to an offset of its buffer; after a failure the rest are skipped.  false: up_status
	bool up(uint64_t off, const void* src, size_t bytes) {
		if (up_err == hipSuccess) up_err = hipMemcpyAsync(s.buf + off, src, bytes, hipMemcpyHostToDevice, stream);
		return up_err == hipSuccess;
	}
	Status up_status() const { return Status{up_err, "H2D"}; }
	template <class T>  // ... of a whole descriptor array
	bool up(uint64_t off, const std::vector<T>& v) { return up(off, v.data(), v.size() * sizeof(T)); }
};

// One call's resources and the stages its chunks go through; a finished call, a device failure and a C++ exception
// all leave through the destructor.  Uploads and kernels run on one stream per chunk slot, downloads by the Copiers:
// chunk k's D2H overlaps chunk k+1's kernels.  Slots 0/1 alternate between device-m05 chunks, 2/3 between host-m05
// chunks, so a hybrid batch's host chunks never wait for the (long) device-m05 chunk's slot.
struct Pipeline {
	const WebPStill* pics = nullptr;  // located by the caller (decode_batch); Feed has the refusals
	uint32_t n = 0;
	int filtered = 0;
	Sinks sk;
	uint32_t chunk_frames[2] = {kChunkFrames, kTokChunkFrames};  // per chunk (at most), by kind like caps.mbs: [tok]
	MbCaps caps{{kChunkMbs, kTokChunkMbs}};
	uint32_t window = 0;    // positions the workers may run ahead of the last launched chunk
	uint32_t released = 0;  // positions whose chunks are launched (all below this one)
	bool trace = false;     // VP8G_PIPE_TRACE=1: one stderr line per chunk (kind, frames, MBs, launch / retire times; diagnostics)
	std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
	Feed feed;
	std::vector<std::thread> pool;
	hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};
	Copier copiers[2];  // downloads of host-m05 chunks / device-m05 chunks
	Slot slots[4];
	uint32_t nchunk[2] = {0, 0};  // chunks so far per kind (host, device)
	std::vector<uint8_t> live;    // frame i has its output (an allocated image; a slot of the tensor)
	// The host frames of the last chunks are released by the background freer (g_freer) once the
	// call has its results: freeing them is when glibc trims the heap those frames grew (GBs of packed data,
	// ~0.3 s at 1024 4K frames), work the caller need not wait for.
	bool defer_release = false;
	std::vector<Vp8gPackedFrame> late;
	std::vector<Vp8fLosslessImage> late_ll;  // (the same for lossless frames: 4 bytes per pixel of residuals each)
	bool finished = false;  // every chunk retired (set by the caller); else the destructor takes the failure path,
	Status failure;         //   with the device failure if that is why
	~Pipeline() {
		if (!finished) feed.stop();            // workers waiting for their window leave
		for (std::thread& t : pool) t.join();  // (before the device buffers they feed are freed)
		for (Copier& c : copiers) c.stop();
		const hipStream_t all[6] = {streams[0], streams[1], streams[2], streams[3], copiers[0].stream, copiers[1].stream};
		if (!finished) {
			for (Vp8gPackedFrame& p : late) vp8f_packed_free(&p);  // (inline: there is no result to hurry back with)
			late.clear();
			for (Vp8fLosslessImage& im : late_ll) vp8f_lossless_free(&im);
			late_ll.clear();
			for (hipStream_t st : all)
				if (st) (void)hipStreamSynchronize(st);
			if (!failure.ok()) vp8g::set_error_text(failure.where ? failure.where : "pipeline", failure.he);
		}
		for (Slot& s : slots) {
			if (s.done) (void)hipEventDestroy(s.done);
			if (s.kdone) (void)hipEventDestroy(s.kdone);
			if (s.buf) (void)hipFree(s.buf);
		}
		for (hipStream_t st : all)
			if (st) (void)hipStreamDestroy(st);
		if (trace && finished) fprintf(stderr, "[pipe] buffers freed at %.1f ms\n", ms_now());
		try {  // (started last: its heap trimming would contend with the device-memory frees above)
			if (!late.empty()) g_freer.post(std::move(late));
		} catch (...) {  // (no thread, no memory: `late` is untouched)
			for (Vp8gPackedFrame& p : late) vp8f_packed_free(&p);
		}
		try {
			if (!late_ll.empty()) g_freer.post(std::move(late_ll));
		} catch (...) {
			for (Vp8fLosslessImage& im : late_ll) vp8f_lossless_free(&im);
		}
		for (size_t i = 0; i < feed.dev.size(); i++) {  // failed frames (the others were freed per chunk)
			if (!feed.dev[i]) vp8f_packed_free(&feed.pk[i]);
			free(feed.ares[i]);
			vp8f_lossless_free(&feed.ll[i]);
		}
	}
	double ms_now() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); }
	const Vp8KeyFrameHeader& kf_of(uint32_t i) const { return feed.dev[i] ? feed.tj[i].kf : feed.pk[i].kf; }
	const Vp8DecodedFrame& f_of(uint32_t i) const { return feed.dev[i] ? feed.tj[i].hdr : feed.pk[i].f; }
	// scaled decode: the loop filter per frame (VP8G_SCALE_DWEBP_FILTER), the output image at the scaled size
	int filtered_of(uint32_t i) const {
		return sk.opts ? vp8f_scale_filtered(kf_of(i).width, kf_of(i).height, sk.opt_of(i), filtered) : filtered;
	}
	int alloc_out(uint32_t i, uint32_t w, uint32_t h) {
		if (sk.opts && vp8g_scaled_size(w, h, sk.opt_of(i), &w, &h) != 0) return -1;
		if (!sk.topt && vp8g::alloc_planes(&sk.outs[i], w, h, false) != 0) return -1;
		live[i] = 1;
		return 0;
	}
	// Plans the batch, starts the workers, creates the device objects.  (No constructor: an exception on the way must
	// leave a complete object, whose destructor joins the threads that did start.)
	Status start(const WebPStill* pics_, const int* refused, uint32_t n_, int filtered_, uint32_t threads, uint32_t flags, const Sinks& sinks) {
		pics = pics_, n = n_, filtered = filtered_, sk = sinks;
		const bool tok = (flags & VP8G_BATCH_DEVICE_M05) != 0;
		const long knob = getenv("VP8G_CHUNK_FRAMES") ? atol(getenv("VP8G_CHUNK_FRAMES")) : 0;  // test knob: smaller chunks
		for (uint32_t& cf : chunk_frames)
			if (knob > 0 && (uint64_t)knob < cf) cf = (uint32_t)knob;
		size_t fr = 0, tot = 0;
		caps = chunk_budget(hipMemGetInfo(&fr, &tot) == hipSuccess ? fr : 0);
		live.assign(n, 0);
		if (!threads) threads = default_threads();
		if (threads > n) threads = n;
		feed.pics = pics, feed.refused = refused, feed.n = n;
		feed.fflags = (flags & VP8G_BATCH_MULTI_PARTITION) ? VP8F_MULTI_PARTITION : 0u;
		feed.pk.assign(n, Vp8gPackedFrame{});
		if (tok) feed.tj.assign(n, TokJob{});
		feed.err.assign(n, 0);
		feed.alpha = sk.alpha;
		feed.ares = std::vector<uint8_t*>(n, nullptr);
		feed.afilter.resize(n);
		feed.is_ll.assign(n, 0);
		feed.ll.assign(n, Vp8fLosslessImage{});
		feed.ready.reset(new uint8_t[n]());
		plan_frames(pics, refused, n, tok, threads, feed.dev, feed.order, sk.topt == nullptr);
		trace = getenv("VP8G_PIPE_TRACE") && atoi(getenv("VP8G_PIPE_TRACE")) != 0;
		if (trace) {
			uint32_t nd = 0;
			for (uint32_t i = 0; i < n; i++) nd += feed.dev[i];
			fprintf(stderr, "[pipe] n=%u threads=%u device_frames=%u host_frames=%u chunk_mbs_tok=%llu chunk_mbs_pk=%llu\n", n,
			        threads, nd, n - nd, (unsigned long long)caps.mbs[1], (unsigned long long)caps.mbs[0]);
		}
		const uint32_t cf = chunk_frames[tok];
		window = 2 * cf > 4 * threads ? 2 * cf : 4 * threads;
		feed.limit = window;
		pool.reserve(threads);
		for (uint32_t t = 0; t < threads; t++) pool.emplace_back([this] { feed.work(); });
		// The device-m05 slots' streams (0, 1) at the lowest stream priority, the others at the default:
		// HIP keeps a pool of hardware queues per priority, so a host-m05 chunk never sits in one hardware
		// queue behind a device-m05 kernel (~0.5-1.5 s, one frame's serial bool decoding) -- streams
		// beyond GPU_MAX_HW_QUEUES share queues, and work on a shared queue runs in order.
		int least = 0, greatest = 0;
		if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
		hipError_t e = hipSuccess;
		for (int i = 0; i < 4 && e == hipSuccess; i++)
			e = i < 2 ? hipStreamCreateWithPriority(&streams[i], hipStreamNonBlocking, least)
			          : hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking);
		for (Copier& c : copiers) {
			if (e == hipSuccess) e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
			if (e == hipSuccess) c.th = std::thread([&c] { c.run(); });
		}
		if (e != hipSuccess) return Status{e, "stream"};
		for (Slot& s : slots) {
			if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
			if (e == hipSuccess) e = hipEventCreateWithFlags(&s.kdone, hipEventDisableTiming);
		}
		return Status{e, "event"};
	}
	void release(Slot& s) {
		for (uint32_t i : s.frames) {
			free(feed.ares[i]);
			feed.ares[i] = nullptr;
			if (feed.is_ll[i]) {
				if (defer_release) late_ll.push_back(feed.ll[i]), memset(&feed.ll[i], 0, sizeof(feed.ll[i]));
				else vp8f_lossless_free(&feed.ll[i]);
				continue;
			}
			if (feed.dev[i]) continue;
			if (defer_release) late.push_back(feed.pk[i]), memset(&feed.pk[i], 0, sizeof(feed.pk[i]));
			else vp8f_packed_free(&feed.pk[i]);
		}
		s.frames.clear();
	}
	// Waits for a slot's chunk, if it has one, and frees the chunk's host data.
	Status finish_slot(Slot& s) {
		if (!s.busy) return Status{};
		s.busy = false;
		const int si = (int)(&s - slots);
		const double tw = trace ? ms_now() : 0.0;
		if (hipError_t e = copiers[si < 2 ? 1 : 0].wait_issued(&s); e != hipSuccess) return Status{e, "D2H"};
		if (hipError_t e = hipEventSynchronize(s.done); e != hipSuccess) return Status{e, "sync"};
		if (trace) fprintf(stderr, "[pipe] slot %d retired at %.1f ms (waited %.1f ms)\n", si, ms_now(), ms_now() - tw);
		const double tr = trace ? ms_now() : 0.0;
		release(s);
		if (trace) fprintf(stderr, "[pipe] slot %d host data freed in %.1f ms\n", si, ms_now() - tr);
		return s.status != 0 ? Status{hipErrorLaunchFailure, "kernel status"} : Status{};
	}
	// The next chunk's frames and shape: consecutive positions of one kind from c.a, in order, as they finish.  A frame
	// whose options or size do not suit the sinks fails here (feed.err) and stays out of idx; the others still decode.
	void gather_chunk(Chunk& c) {
		ChunkShape& sh = c.sh;
		uint64_t xmbs = 0;  // what the frames hold beyond their MBs' share (extra_mbs)
		for (; c.b < n && c.b - c.a < chunk_frames[c.tok] && (feed.dev[feed.order[c.b]] != 0) == c.tok; c.b++) {
			const uint32_t fi = feed.order[c.b];
			feed.wait_ready(fi);
			if (feed.err[fi]) continue;
			if (feed.is_ll[fi]) {
				const uint64_t srcb = lossless_src_bytes(feed.ll[fi]), outb = 4ull * feed.ll[fi].width * feed.ll[fi].height;
				if (int e = lossless_fits(fi)) {
					feed.err[fi] = e;
					continue;
				}
				// a frame that is cropped / rescaled also holds its planes and its scaled picture
				Vp8fScaleGeom g;
				const bool scaled = !lossless_whole(fi, &g);
				const ArgbScaleBatch::Need nd = scaled ? ArgbScaleBatch::need(feed.ll[fi].width, feed.ll[fi].height, sk.opt_of(fi)) : ArgbScaleBatch::Need{0, 0, 0};
				const uint64_t fx = extra_mbs(al256(srcb) + al256(outb) + nd.work + nd.scaled + nd.descs);
				if (!(c.idx.empty() && c.lidx.empty()) && sh.mbs + xmbs + fx > caps.mbs[c.tok]) break;
				xmbs += fx;
				sh.lsrcb = al256(sh.lsrcb + srcb), sh.loutb = al256(sh.loutb + outb);
				if (scaled) sh.nls++, sh.lsworkb += nd.work, sh.lsoutb += nd.scaled;
				c.lidx.push_back(fi);
				continue;
			}
			const uint32_t w = kf_of(fi).width, h = kf_of(fi).height;
			uint32_t sw = w, sh_ = h;  // the picture's size at the sink
			if (sk.opts && vp8g_scaled_size(w, h, sk.opt_of(fi), &sw, &sh_) != 0) feed.err[fi] = EINVAL;  // options that do not fit it
			else if (sk.topt && (sw != sk.topt->width || sh_ != sk.topt->height)) feed.err[fi] = EINVAL;  // not the tensor's size
			if (feed.err[fi]) continue;
			const Vp8DecodedFrame& f = f_of(fi);
			const uint64_t ownb = vp8g_i420_size(w, h), sclb = scaled_bytes(fi, sw, sh_);
			uint64_t fx = sclb > ownb ? extra_mbs(sclb - ownb) : 0u;  // (0 unless VP8G_SCALE_EXPAND grows it, or 4:4:4 planes of a mild shrink)
			// alpha planes count against the chunk's memory budget: residual + un-predicted (+ scaled)
			const uint64_t apl = feed.ares[fi] ? (uint64_t)w * h : 0u;
			const uint64_t aspl = apl && sk.opts ? (uint64_t)sw * sh_ : 0u;
			fx += extra_mbs(2u * apl + aspl);
			if (!(c.idx.empty() && c.lidx.empty()) && sh.mbs + xmbs + f.mb_total + fx > caps.mbs[c.tok]) break;
			xmbs += fx;
			if (sk.opts) sh.soutb = al256(sh.soutb + sclb);
			if (apl) sh.ab = al256(sh.ab + apl), sh.asb = al256(sh.asb + aspl);
			c.idx.push_back(fi);
			sh.mbs += f.mb_total;
			if (c.tok) sh.bitsb += bits_slot(pics[fi].vp8_size);
			else sh.vals += feed.pk[fi].n_values;
			sh.outb = al256(sh.outb + ownb);
			if (f.mb_cols > sh.max_cols) sh.max_cols = f.mb_cols;
			if (f.mb_rows > sh.max_rows) sh.max_rows = f.mb_rows;
		}
		sh.nf = (uint32_t)c.idx.size();
		sh.nl = (uint32_t)c.lidx.size();
	}
	// bytes of lossy frame fi's scaled planes in the chunk's small buffer
	uint64_t scaled_bytes(uint32_t fi, uint32_t sw, uint32_t sh_) const {
		return !sk.opts ? 0u : sk.yuv444(fi) ? 3ull * sw * sh_ : vp8g_i420_size(sw, sh_);
	}
	// a lossless frame's upload: the residual image and every transform's data, each padded to a dword count
	static uint64_t lossless_tr_dwords(const Vp8fLosslessImage& im, uint32_t k) {
		const Vp8fLosslessTransform& t = im.tr[k];
		if (t.type == VP8F_T_COLOR_INDEX) return t.ncolors;
		if (t.type == VP8F_T_SUBTRACT_GREEN) return 0;
		const uint64_t r = (1u << t.bits) - 1u;
		return ((t.xsize + r) >> t.bits) * ((im.height + r) >> t.bits);
	}
	static uint64_t lossless_src_bytes(const Vp8fLosslessImage& im) {
		uint64_t dw = (uint64_t)im.xsize * im.height;
		for (uint32_t k = 0; k < im.ntransforms; k++) dw += lossless_tr_dwords(im, k);
		return 4u * dw;
	}
	// Whether a lossless frame goes to the tensor as it is: without VP8G_X_LOSSLESS_SCALE always (lossless_fits has let
	// only identities pass); with it when there is no option, or one that resolves (*g, libwebp's rules for such a file:
	// the window's origin as given) to the whole picture and no target size -- a target equal to the picture's size still
	// takes libwebp's premultiply, rescale, un-premultiply.  An option that does not fit: true.
	bool lossless_whole(uint32_t fi, Vp8fScaleGeom* g) const {
		const uint32_t w = feed.ll[fi].width, h = feed.ll[fi].height;
		if (!sk.opts || !sk.lossless_scale || vp8f_scale_resolve_argb(w, h, sk.opt_of(fi), g) != 0) return true;
		return !g->scaling && g->win_w == w && g->win_h == h;
	}
	// 0, or why a lossless frame cannot go to the sink: without VP8G_X_LOSSLESS_SCALE scaling it is not supported (ENOTSUP
	// for any option that is not the identity); with it the option must fit the frame; and the result must have the
	// tensor's size
	int lossless_fits(uint32_t fi) const {
		uint32_t w = feed.ll[fi].width, h = feed.ll[fi].height;
		if (sk.opts && sk.lossless_scale) {
			Vp8fScaleGeom g;
			if (vp8f_scale_resolve_argb(w, h, sk.opt_of(fi), &g) != 0) return EINVAL;
			w = g.out_w, h = g.out_h;
		} else if (sk.opts) {
			const Vp8gScaleOpt& o = *sk.opt_of(fi);
			uint32_t sw = 0, sh_ = 0;
			if (vp8g_scaled_size(w, h, &o, &sw, &sh_) != 0) return EINVAL;
			const bool whole = (o.crop_left | o.crop_top | o.crop_w | o.crop_h) == 0 ||
			                   (o.crop_left == 0 && o.crop_top == 0 && o.crop_w == w && o.crop_h == h);
			if (!whole || sw != w || sh_ != h) return ENOTSUP;
		}
		return sk.topt && w == sk.topt->width && h == sk.topt->height ? 0 : EINVAL;
	}
	// Frame descriptors and output images of the chunk's frames.
	void describe_chunk(Chunk& c) {
		Slot& s = c.s;
		s.descs.assign(c.sh.nf, Vp8gFrameDesc{});
		uint64_t mo = 0, oo = 0;  // offsets in the chunk: MBs, output bytes
		for (uint32_t j = 0; j < c.sh.nf; j++) {
			const uint32_t fi = c.idx[j];
			const Vp8KeyFrameHeader& kf = kf_of(fi);
			if (vp8g::make_desc(&kf, &f_of(fi), filtered_of(fi), mo, oo, &s.descs[j], false) != 0 || alloc_out(fi, kf.width, kf.height) != 0) {
				feed.err[fi] = errno ? errno : EINVAL;  // (cannot happen for a frame the host front end accepted)
				s.descs[j].flags = 0;
			}
			mo += f_of(fi).mb_total;
			oo = al256(oo + vp8g_i420_size(kf.width, kf.height));
		}
	}
	// The recon launch (vp8g_plan.hip, kPipelinePolicy).  Split mode (a frame over several co-resident workgroups that
	// spin on each other) only for a call's only chunk: other slots' streams could hold the CUs a part is waiting for.
	void plan_launch(Chunk& c) const {
		vp8g::LaunchPolicy pol = vp8g::kPipelinePolicy;
		pol.may_split = c.a == 0 && c.b == n;
		c.plan = vp8g::plan_launch(c.s.descs.data(), c.sh.nf, vp8g::device_cus(), true, 0, vp8g::knobs_from_env(), pol);
	}
	// The chunk's input onto its stream (a device-m05 chunk's payloads and m05 jobs, a host-m05 one's side arrays, block
	// masks and packed values); then the descriptors and a zero status word.
	Status upload_chunk(Chunk& c) {
		Slot& s = c.s;
		const ChunkLayout& L = c.L;
		if (c.tok) s.jobs.resize(c.sh.nf);
		uint64_t mo = 0, po = 0;  // offsets in the chunk: MBs, payload (bitstream bytes / packed values)
		for (uint32_t j = 0; j < c.sh.nf && c.up_err == hipSuccess; j++) {
			const uint32_t fi = c.idx[j];
			const uint64_t mt = f_of(fi).mb_total;
			if (c.tok) {
				const WebPStill& pic = pics[fi];
				s.jobs[j] = feed.tj[fi].tf;
				s.jobs[j].data = po;
				s.jobs[j].mb_offset = mo;
				c.up(L.bits + po, pic.data + pic.vp8_offset, pic.vp8_size);
				po += bits_slot(pic.vp8_size);
			} else {
				Vp8gPackedFrame& p = feed.pk[fi];
				for (uint32_t m = 0; po && m < mt; m++) p.mb_off[m] += (uint32_t)po;  // chunk-relative value offsets
				c.up(L.ym + mo, p.f.ymode, mt);
				c.up(L.uvm + mo, p.f.uv_mode, mt);
				c.up(L.seg + mo, p.f.segment_id, mt);
				c.up(L.hasc + mo, p.f.has_coeff, mt);
				c.up(L.bm + mo * 16, p.f.bmode, mt * 16);
				c.up(L.masks + mo * kNb * 2, p.masks, mt * kNb * 2);
				c.up(L.mboff + mo * 4, p.mb_off, mt * 4);
				if (p.n_values) c.up(L.vals + po * 2, p.values, p.n_values * 2);
				po += p.n_values;
			}
			mo += mt;
		}
		if (c.tok) c.up(L.jobs, s.jobs);
		if (c.up_err != hipSuccess) return c.up_status();
		s.frames = c.idx;
		if (trace)
			fprintf(stderr, "[pipe] chunk %s slot %u frames=%u mbs=%llu launched at %.1f ms\n", c.tok ? "device-m05" : "host-m05",
			        (uint32_t)(&s - slots), c.sh.nf, (unsigned long long)c.sh.mbs, ms_now());
		if (!c.up(L.desc, s.descs)) return c.up_status();
		return Status{hipMemsetAsync(s.buf + L.status, 0, 4, c.stream), "memset"};
	}
	// Expansion (or device m05) + recon(+LF), inside the process-wide launch gate (vp8g_device.h): the split mode only
	// when no other launch of the library is in flight.
	Status launch_recon(Chunk& c) {
		const ChunkLayout& L = c.L;
		const uint32_t nf = c.sh.nf;
		uint8_t* d = c.s.buf;
		hipStream_t stream = c.stream;
		vp8g::GateScope gate(stream);
		if (gate.status() != hipSuccess) return Status{gate.status(), "hipStreamWaitEvent(gate)"};
		const vp8g::Launch& run = c.plan.resolve(gate.may_cross());
		if (run.parts > 1)
			if (hipError_t e = hipMemsetAsync(d + L.gprog, 0, c.plan.gprog_bytes, stream); e != hipSuccess) return Status{e, "memset"};
		Vp8gBatchArrays arr{(const int16_t*)(d + L.cy), (const int16_t*)(d + L.cu), (const int16_t*)(d + L.cv), (const int16_t*)(d + L.cy2),
		                    d + L.ym, d + L.uvm, d + L.seg, d + L.hasc, d + L.bm, /*src=*/nullptr, (uint32_t*)(d + L.status)};
		if (c.tok) {
			if (hipError_t e = hipMemsetAsync(d + L.cy, 0, L.cy2 + c.sh.mbs * 32 - L.cy, stream); e != hipSuccess) return Status{e, "memset"};
			const int rc = vp8g_m05_batch_device(c.s.jobs.data(), (const Vp8gTokFrame*)(d + L.jobs), nf, d + L.bits, &arr, stream);
			if (rc != 0) return capi_status(rc, "m05 launch");
		} else {
			const uint64_t threads_x = c.sh.mbs * 32;
			hipLaunchKernelGGL(expand_kernel, dim3((uint32_t)((threads_x + 255) / 256)), dim3(256), 0, stream,
			                   (const uint16_t*)(d + L.masks), (const uint32_t*)(d + L.mboff), (const int16_t*)(d + L.vals),
			                   (uint32_t)c.sh.mbs, (int16_t*)(d + L.cy), (int16_t*)(d + L.cu), (int16_t*)(d + L.cv), (int16_t*)(d + L.cy2));
			if (hipError_t e = hipGetLastError(); e != hipSuccess) return Status{e, "expand launch"};
		}
		// (the gctx region holds the frame kernel's global context or the chain's context between waves: never both)
		const vp8g::LaunchBuffers bufs = {d + L.gctx, d + L.mbox, (uint32_t*)(d + L.gprog), d + L.gctx, nullptr, 0};
		if (hipError_t e = vp8g::launch(c.plan, run, (const Vp8gFrameDesc*)(d + L.desc), arr, d + L.out, bufs, stream); e != hipSuccess)
			return Status{e, "recon launch"};
		return Status{gate.done(run.crosses()), "hipEventRecord(gate)"};
	}
	// A batch of scale descriptors (the frames', the alpha planes') to `off` of the chunk's buffer and through the rescaler.
	Status scale_batch(Chunk& c, const std::vector<Vp8gScaleDesc>& v, uint64_t off, const char* where) {
		if (v.empty()) return Status{};
		if (!c.up(off, v)) return c.up_status();
		uint8_t* d = c.s.buf;
		return capi_status(vp8g_scale_batch_device(v.data(), (const Vp8gScaleDesc*)(d + off), (uint32_t)v.size(), d, d, c.stream), where);
	}
	// Scaled decode: crop / rescale the chunk's frames into the small buffer (same stream).
	Status launch_scale(Chunk& c) {
		Slot& s = c.s;
		s.sdescs.clear();
		uint64_t so = 0;
		uint32_t task0 = 0;
		for (uint32_t j = 0; sk.opts && j < c.sh.nf; j++) {
			const Vp8gFrameDesc& fd = s.descs[j];
			if (!live[c.idx[j]]) continue;  // (a frame that failed above)
			Vp8gScaleDesc sd;
			const bool y444 = sk.yuv444(c.idx[j]);
			if ((y444 ? vp8g_make_scale_desc_444 : vp8g_make_scale_desc)(fd.width, fd.height, c.L.out + fd.out_y, c.L.out + fd.out_u,
			                                                             c.L.out + fd.out_v, fd.stride_y, fd.stride_uv, sk.opt_of(c.idx[j]),
			                                                             c.L.sout + so, task0, &sd) != 0) {
				feed.err[c.idx[j]] = EINVAL;  // (cannot happen: the options were resolved when the chunk was gathered)
				continue;
			}
			s.sdescs.push_back(sd);
			c.sj.push_back(j);
			c.s444.push_back(y444);
			task0 += sd.ntasks;
			so = al256(so + scaled_bytes(c.idx[j], sd.width, sd.height));
		}
		return scale_batch(c, s.sdescs, c.L.sdesc, "scale launch");
	}
	// Alpha sink: the residual planes of the chunk's frames that have one are uploaded, un-predicted (vp8g_alpha.hip) and,
	// with opts, cropped / rescaled as luma (same stream); c.aplane = where each frame's alpha ends up (opaque if none).
	Status launch_alpha(Chunk& c) {
		Slot& s = c.s;
		const ChunkLayout& L = c.L;
		uint8_t* d = s.buf;
		s.adescs.clear();
		s.asdescs.clear();
		c.aplane.assign(c.sh.nf, Vp8gTensorAlpha{VP8G_T_OPAQUE, 0, 0});
		uint64_t ao = 0, aso = 0;
		uint32_t atask = 0;
		for (uint32_t j = 0; sk.alpha && j < c.sh.nf && c.up_err == hipSuccess; j++) {
			const uint32_t fi = c.idx[j];
			if (!feed.ares[fi] || !live[fi]) continue;
			const uint32_t w = kf_of(fi).width, h = kf_of(fi).height;
			Vp8gAlphaDesc ad;
			if (vp8g_make_alpha_desc(w, h, feed.afilter[fi], L.ares + ao, w, L.aout + ao, w, (uint32_t)s.adescs.size(), &ad) != 0) {
				feed.err[fi] = EINVAL;  // (cannot happen: the decoder returns filters 0..3 for sizes it accepted)
				continue;
			}
			c.up(L.ares + ao, feed.ares[fi], (size_t)w * h);
			c.aplane[j] = Vp8gTensorAlpha{L.aout + ao, w, 0};
			if (sk.opts) {
				Vp8gScaleDesc sd;
				if (vp8g_make_scale_desc_plane(w, h, L.aout + ao, w, sk.opt_of(fi), L.asout + aso, atask, &sd) != 0) {
					feed.err[fi] = EINVAL;  // (cannot happen: the options were resolved when the chunk was gathered)
					continue;
				}
				s.asdescs.push_back(sd);
				atask += sd.ntasks;
				c.aplane[j] = Vp8gTensorAlpha{L.asout + aso, sd.width, 0};
				aso = al256(aso + (uint64_t)sd.width * sd.height);
			}
			s.adescs.push_back(ad);
			ao = al256(ao + (uint64_t)w * h);
		}
		if (s.adescs.empty() || !c.up(L.adesc, s.adescs)) return c.up_status();  // (no plane: no scale descriptor either)
		const int rc = vp8g_alpha_unfilter_batch_device(s.adescs.data(), (const Vp8gAlphaDesc*)(d + L.adesc), (uint32_t)s.adescs.size(), d, d,
		                                                c.stream);
		if (rc != 0) return capi_status(rc, "alpha launch");
		return scale_batch(c, s.asdescs, L.asdesc, "alpha scale launch");
	}
	// One frame of the chunk (position j, its planes at offsets of the chunk's buffer) into its slot of the tensor.
	// y444: the planes are 4:4:4 (launch_scale made them with vp8g_make_scale_desc_444); those frames have a launch of their own.
	void add_tensor_desc(Chunk& c, uint32_t j, uint64_t y, uint64_t u, uint64_t v, uint32_t sy, uint32_t suv, bool y444 = false) {
		const uint32_t fi = c.idx[j];
		if (feed.err[fi]) return;  // (a frame whose alpha stage failed above)
		Vp8gTensorDesc td;
		if ((y444 ? vp8g_make_tensor_desc_444 : vp8g_make_tensor_desc)(sk.topt, y, u, v, sy, suv, (uint64_t)fi * sk.tslot, 0, &td) != 0) {
			feed.err[fi] = EINVAL;  // (cannot happen: the size was checked when the chunk was gathered)
			return;
		}
		std::vector<Vp8gTensorDesc>& descs = y444 ? c.s.tdescs444 : c.s.tdescs;
		td.task0 = (uint32_t)descs.size() * td.ntasks;  // (every image of a tensor has the same task count)
		descs.push_back(td);
		(y444 ? c.s.talpha444 : c.s.talpha).push_back(c.aplane[j]);
	}
	// Tensor sink: the chunk's frames (scaled or as reconstructed) into their slots of the caller's tensor (same stream).
	// A chunk may hold 4:2:0 frames and 4:4:4 ones (Sinks::yuv444): one launch each, the second's descriptors behind the
	// first's in the chunk's buffer; each launch writes only its own frames' slots.
	Status launch_tensor(Chunk& c) {
		Slot& s = c.s;
		const ChunkLayout& L = c.L;
		uint8_t* d = s.buf;
		s.tdescs.clear();
		s.talpha.clear();
		s.tdescs444.clear();
		s.talpha444.clear();
		for (size_t q = 0; sk.topt && sk.opts && q < s.sdescs.size(); q++) {
			const Vp8gScaleDesc& sd = s.sdescs[q];
			add_tensor_desc(c, c.sj[q], sd.p[0].dst, sd.p[1].dst, sd.p[2].dst, sd.p[0].dst_stride, sd.p[1].dst_stride, c.s444[q] != 0);
		}
		for (uint32_t j = 0; sk.topt && !sk.opts && j < c.sh.nf; j++) {
			const Vp8gFrameDesc& fd = s.descs[j];
			if (live[c.idx[j]]) add_tensor_desc(c, j, L.out + fd.out_y, L.out + fd.out_u, L.out + fd.out_v, fd.stride_y, fd.stride_uv);
		}
		const uint32_t nt = (uint32_t)s.tdescs.size(), nt444 = (uint32_t)s.tdescs444.size();
		if (nt) {
			if (!c.up(L.tdesc, s.tdescs) || (sk.alpha && !c.up(L.talpha, s.talpha))) return c.up_status();
			const Status st = capi_status(
			    sk.alpha ? vp8g_tensor_batch_device_a(s.tdescs.data(), (const Vp8gTensorDesc*)(d + L.tdesc), s.talpha.data(),
			                                          (const Vp8gTensorAlpha*)(d + L.talpha), nt, sk.topt, d, sk.d_tensor, c.stream)
			             : vp8g_tensor_batch_device(s.tdescs.data(), (const Vp8gTensorDesc*)(d + L.tdesc), nt, sk.topt, d, sk.d_tensor, c.stream),
			    "tensor launch");
			if (!st.ok()) return st;
		}
		if (!nt444) return Status{};
		const uint64_t o_desc = L.tdesc + nt * sizeof(Vp8gTensorDesc), o_alpha = L.talpha + nt * sizeof(Vp8gTensorAlpha);  // (both regions hold nf entries)
		if (!c.up(o_desc, s.tdescs444) || (sk.alpha && !c.up(o_alpha, s.talpha444))) return c.up_status();
		return capi_status(vp8g_tensor_batch_device_444(s.tdescs444.data(), (const Vp8gTensorDesc*)(d + o_desc), sk.alpha ? s.talpha444.data() : nullptr,
		                                                sk.alpha ? (const Vp8gTensorAlpha*)(d + o_alpha) : nullptr, nt444, sk.topt,
		                                                sk.alpha ? 4u : 3u, d, sk.d_tensor, c.stream),
		                   "tensor launch (4:4:4)");
	}
	// Lossless sink: the residual images and transform data of the chunk's lossless frames are uploaded, the transforms
	// inverted (vp8g_lossless.hip) and the ARGB pictures written to their slots of the tensor (same stream); with
	// VP8G_X_LOSSLESS_SCALE the pictures whose option is not the identity pass through vp8g_scale_argb_batch_device between
	// the two, and the tensor kernel reads their scaled copies (ArgbScaleBatch, vp8g_argb_batch.h, keeps the offsets and
	// counters of those two launches).
	Status launch_lossless(Chunk& c) {
		Slot& s = c.s;
		const ChunkLayout& L = c.L;
		uint8_t* d = s.buf;
		s.ldescs.clear();
		s.lbatch.begin(c.sh.nls, L.lsout);
		s.frames.insert(s.frames.end(), c.lidx.begin(), c.lidx.end());  // (their host data lives until the slot retires)
		const uint32_t channels = sk.alpha ? 4u : 3u;
		uint64_t so = 0, oo = 0;
		for (uint32_t fi : c.lidx) {
			const Vp8fLosslessImage& im = feed.ll[fi];
			Vp8gLosslessTransform tr[4];
			const uint64_t src = L.lsrc + so;
			c.up(src, im.argb, 4u * (size_t)im.xsize * im.height);
			so += 4u * (uint64_t)im.xsize * im.height;
			for (uint32_t k = 0; k < im.ntransforms; k++) {
				const uint64_t bytes = 4u * lossless_tr_dwords(im, k);
				tr[k] = Vp8gLosslessTransform{L.lsrc + so, im.tr[k].type, im.tr[k].bits, im.tr[k].xsize, im.tr[k].ncolors};
				if (bytes) c.up(L.lsrc + so, im.tr[k].data, bytes);
				so += bytes;
			}
			so = al256(so);
			Vp8gLosslessDesc ld;
			Vp8fScaleGeom g;
			const uint64_t pic = L.lout + oo, dst = (uint64_t)fi * sk.tslot;  // the transform kernel's picture; the frame's slot
			if (vp8g_make_lossless_desc(im.width, im.height, src, pic, im.ntransforms, tr, (uint32_t)s.ldescs.size(), &ld) != 0 ||
			    (lossless_whole(fi, &g) ? s.lbatch.add_whole(sk.topt, channels, pic, dst)
			                            : s.lbatch.add(im.width, im.height, pic, sk.opt_of(fi), sk.topt, channels, dst)) != 0) {
				feed.err[fi] = EINVAL;  // (cannot happen for a stream the host decoder accepted and a size checked when gathered)
				continue;
			}
			oo = al256(oo + 4u * (uint64_t)im.width * im.height);
			s.ldescs.push_back(ld);
			live[fi] = 1;
		}
		if (s.ldescs.empty()) return c.up_status();
		if (!c.up(L.ldesc, s.ldescs) || !c.up(L.ltdesc, s.lbatch.tensor) || !(s.lbatch.scale.empty() || c.up(L.lsdesc, s.lbatch.scale)))
			return c.up_status();
		const uint32_t nl = (uint32_t)s.ldescs.size();
		if (int rc = vp8g_lossless_batch_device(s.ldescs.data(), (const Vp8gLosslessDesc*)(d + L.ldesc), nl, d, d, c.stream); rc != 0)
			return capi_status(rc, "lossless launch");
		return s.lbatch.launch((const Vp8gScaleArgbDesc*)(d + L.lsdesc), (const Vp8gTensorArgbDesc*)(d + L.ltdesc), d, d + L.lswork, sk.topt, channels,
		                       sk.d_tensor, c.stream);
	}
	// D2H into the callers' images (and of the status word, whatever the sink), by this kind's Copier once the
	// kernels are done; then the workers may run a window ahead of this chunk.
	void queue_downloads(Chunk& c) {
		Slot& s = c.s;
		uint8_t* d = s.buf;
		s.d2h.clear();
		for (size_t q = 0; q < s.sdescs.size() && !sk.topt; q++) {
			const Vp8gScaleDesc& sd = s.sdescs[q];
			Yuv420Image& img = sk.outs[c.idx[c.sj[q]]];
			const size_t ysz = (size_t)sd.width * sd.height, uvsz = (size_t)sd.p[1].dst_w * sd.p[1].dst_h;
			s.d2h.insert(s.d2h.end(), {{img.y, d + sd.p[0].dst, ysz}, {img.u, d + sd.p[1].dst, uvsz}, {img.v, d + sd.p[2].dst, uvsz}});
		}
		for (uint32_t j = 0; j < c.sh.nf && !sk.opts && !sk.topt; j++) {
			const Vp8gFrameDesc& fd = s.descs[j];
			Yuv420Image& img = sk.outs[c.idx[j]];
			if (!img.y) continue;
			const uint8_t* o = d + c.L.out;
			const size_t ysz = (size_t)fd.stride_y * fd.height, uvsz = (size_t)fd.stride_uv * ((fd.height + 1) / 2);
			s.d2h.insert(s.d2h.end(), {{img.y, o + fd.out_y, ysz}, {img.u, o + fd.out_u, uvsz}, {img.v, o + fd.out_v, uvsz}});
		}
		s.d2h.push_back({&s.status, d + c.L.status, 4});
		copiers[c.tok ? 1 : 0].push(&s);
		s.busy = true;
		released = c.b;
		feed.set_limit(released + window);
	}
	// A gathered chunk (with at least one frame) through its slot's buffer and stream, every stage in enqueue order.
	Status launch_chunk(Chunk& c) {
		const bool lossy = !c.idx.empty();  // (else only lossless frames: no recon launch, c.plan stays empty)
		if (lossy) {
			describe_chunk(c);
			plan_launch(c);
		}
		c.L = make_layout(c.sh, c.tok, sk, c.plan);
		const double tg = trace ? ms_now() : 0.0;
		if (hipError_t e = grow(c.s, c.L.total); e != hipSuccess) return Status{e, "hipMalloc(chunk)"};
		const uint32_t si = (uint32_t)(&c.s - slots);
		if (trace) fprintf(stderr, "[pipe] slot %u buffer %.1f GB ready at %.1f ms (%.1f ms)\n", si, c.L.total / 1e9, ms_now(), ms_now() - tg);
		Status st = lossy ? upload_chunk(c) : Status{hipMemsetAsync(c.s.buf + c.L.status, 0, 4, c.stream), "memset"};
		if (!lossy) c.s.descs.clear(), c.s.sdescs.clear();
		if (st.ok() && lossy) st = launch_recon(c);
		// (the scale, alpha and tensor entry points take the launch gate themselves: outside launch_recon's scope)
		if (st.ok() && lossy) st = launch_scale(c);
		if (st.ok() && lossy) st = launch_alpha(c);
		if (st.ok() && lossy) st = launch_tensor(c);
		if (st.ok()) st = launch_lossless(c);
		if (st.ok()) st = Status{hipEventRecord(c.s.kdone, c.stream), "event"};
		if (st.ok()) queue_downloads(c);
		return st;
	}
	// Every chunk of the batch, then the slots' last chunks.
	Status run() {
		for (uint32_t a = 0; a < n;) {
			const bool tok = feed.dev[feed.order[a]] != 0;  // this chunk's kind
			const uint32_t si = (tok ? 0u : 2u) + (nchunk[tok ? 1 : 0]++ & 1u);
			Chunk c{tok, a, a, slots[si], streams[si]};
			gather_chunk(c);
			if (Status st = finish_slot(c.s); !st.ok()) return st;
			if (!c.idx.empty() || !c.lidx.empty())  // (else every frame of it failed)
				if (Status st = launch_chunk(c); !st.ok()) return st;
			a = c.b;
		}
		defer_release = true;
		for (Slot& s : slots)
			if (Status st = finish_slot(s); !st.ok()) return st;
		defer_release = false;
		bool any = false;
		for (uint32_t i = 0; sk.topt && i < n; i++) {  // tensor sink: the slot of every failed frame reads as zero bytes
			if (!feed.err[i]) continue;
			if (hipError_t e = hipMemsetAsync(sk.d_tensor + (uint64_t)i * sk.tslot, 0, sk.tslot, streams[2]); e != hipSuccess)
				return Status{e, "memset"};
			any = true;
		}
		return any ? Status{hipStreamSynchronize(streams[2]), "sync"} : Status{};
	}
};

bool opts_ok(const Vp8gScaleOpt* opts, uint32_t n_opts, uint32_t n) { return opts ? n_opts == 1 || n_opts == n : n_opts == 0; }
// a valid option (vp8g_tensor_slot_size: 0 for a NULL or invalid one) and a tensor that starts on an element boundary
bool tensor_ok(const Vp8gTensorOpt* t, const void* d_out) {
	return t && d_out && vp8g_tensor_slot_size(t) && (uintptr_t)d_out % (vp8g_tensor_slot_size(t) / (3ull * t->width * t->height)) == 0;
}
using vp8g::fail;
// A call that fails as a whole: no output survives, every frame reports `e`.
int fail_all(Yuv420Image* outs, uint32_t n, int* status, int e) {
	for (uint32_t i = 0; i < n; i++) {
		if (outs) yuv420_free(&outs[i]);
		if (status) status[i] = e;
	}
	return fail(e);
}

// The body of every end-to-end entry point: the files, each located here, once, in the mode the sinks imply
// (webp_locate_still: a refused file keeps the errno as its status), or (files = NULL) pictures already located, all of
// them good.  0, or -1 with errno = the first failed frame's error in index order and
// status[i] per frame (a failed frame's image is freed, its tensor slot zero).  After a device failure every status is EIO
// and every output freed; a C++ exception (no memory, no thread) unwinds through ~Pipeline and ends the call alike.
int decode_batch(const ByteSpan* files, const WebPStill* located, uint32_t n, int filtered, uint32_t threads, uint32_t flags, Sinks sk,
                 int* status) {
	sk.tslot = sk.topt ? (sk.alpha ? vp8g_tensor_slot_size_a(sk.topt) : vp8g_tensor_slot_size(sk.topt)) : 0;
	if ((!files && !located) || (sk.topt ? !sk.d_tensor || !sk.tslot || sk.outs : !sk.outs) || n == 0 || (sk.alpha && !(sk.topt && sk.extended)) ||
	    (sk.lossless && !(sk.topt && sk.extended)) ||
	    (flags & ~(VP8G_BATCH_DEVICE_M05 | VP8G_BATCH_MULTI_PARTITION)))
		return fail(EINVAL);
	for (uint32_t i = 0; sk.outs && i < n; i++) memset(&sk.outs[i], 0, sizeof(sk.outs[i]));
	std::vector<int> err;  // per frame, once every chunk has retired
	try {
		const unsigned accept = !sk.extended ? 0u : sk.lossless ? WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS : WEBP_ACCEPT_EXTENDED;
		const LocatedFiles lf(files, files ? n : 0, accept);  // (outlives the Pipeline, whose workers read the records)
		Pipeline p;
		p.failure = p.start(files ? lf.pics.data() : located, files ? lf.refused.data() : nullptr, n, filtered, threads, flags, sk);
		if (p.failure.ok()) p.failure = p.run();
		p.finished = p.failure.ok();
		if (p.finished && p.trace) fprintf(stderr, "[pipe] all chunks retired at %.1f ms\n", p.ms_now());
		if (p.finished) err.swap(p.feed.err);
	} catch (const std::bad_alloc&) {  // (~Pipeline has run: no copy into `outs` is in flight)
		return fail_all(sk.outs, n, status, ENOMEM);
	} catch (const std::system_error& e) {
		return fail_all(sk.outs, n, status, e.code().value() ? e.code().value() : EAGAIN);
	}
	if (err.empty()) return fail_all(sk.outs, n, status, EIO);
	int first = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (status) status[i] = err[i];
		if (err[i] && !first) first = err[i];
		if (err[i] && sk.outs) yuv420_free(&sk.outs[i]);
	}
	return first ? fail(first) : 0;
}

}  // namespace

VP8G_API int vp8g_plan_batch(const ByteSpan* files, uint32_t n, uint32_t threads, uint32_t flags, uint8_t* dev,
                             uint32_t* order) {
	if (!files || !dev || !order || n == 0 || (flags & ~(VP8G_BATCH_DEVICE_M05 | VP8G_BATCH_MULTI_PARTITION))) return fail(EINVAL);
	uint32_t thr = threads ? threads : default_threads();
	if (thr > n) thr = n;  // (as vp8g_decode_webp_batch_ex)
	std::vector<uint8_t> d;
	std::vector<uint32_t> o;
	try {
		const LocatedFiles lf(files, n, 0);  // (as vp8g_decode_webp_batch_ex locates them)
		plan_frames(lf.pics.data(), lf.refused.data(), n, (flags & VP8G_BATCH_DEVICE_M05) != 0, thr, d, o, true);
	} catch (const std::bad_alloc&) {
		return fail(ENOMEM);
	}
	memcpy(dev, d.data(), n);
	memcpy(order, o.data(), n * sizeof(uint32_t));
	return 0;
}

VP8G_API int vp8g_decode_webp_batch_ex(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                       Yuv420Image* outs, int* status) {
	return decode_batch(files, nullptr, n, filtered, threads, flags, Sinks{nullptr, 0, outs}, status);
}

// With `opts` (n_opts = 1 or n) each chunk's frames are cropped / rescaled on the device (vp8g_scale.hip) into a second
// buffer (small, unless VP8G_SCALE_EXPAND grows them: that counts against the chunk's budget); only that is downloaded.
VP8G_API int vp8g_decode_webp_batch_scaled(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                           const Vp8gScaleOpt* opts, uint32_t n_opts, Yuv420Image* outs, int* status) {
	if (!opts || !opts_ok(opts, n_opts, n)) return fail(EINVAL);
	return decode_batch(files, nullptr, n, filtered, threads, flags, Sinks{opts, n_opts, outs}, status);
}

// The sink is the caller's device tensor: each chunk's frames, scaled or not, are written to their slots of d_out
// by the tensor kernel (vp8g_tensor.hip) on the chunk's stream, and only the chunk's status word is downloaded.
VP8G_API int vp8g_decode_webp_batch_tensor(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                           const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, void* d_out,
                                           int* status) {
	if (!tensor_ok(t, d_out) || !opts_ok(opts, n_opts, n)) return fail(EINVAL);
	return decode_batch(files, nullptr, n, filtered, threads, flags, Sinks{opts, n_opts, nullptr, t, (uint8_t*)d_out}, status);
}

// The extended container (WEBP_ACCEPT_EXTENDED) in front of the same pipeline: VP8X files decode, alpha
// is ignored.
VP8G_API int vp8g_decode_webp_batch_x(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                      const Vp8gScaleOpt* opts, uint32_t n_opts, Yuv420Image* outs, int* status) {
	if (!opts_ok(opts, n_opts, n)) return fail(EINVAL);
	return decode_batch(files, nullptr, n, filtered, threads, flags, Sinks{opts, n_opts, outs, nullptr, nullptr, /*extended=*/true}, status);
}

// ... and with VP8G_X_ALPHA the ALPH planes as the tensor's fourth channel.
VP8G_API int vp8g_decode_webp_batch_tensor_x(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                             const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                             void* d_out, int* status) {
	if ((xflags & ~VP8G_X_ALPHA) || !tensor_ok(t, d_out) || !opts_ok(opts, n_opts, n)) return fail(EINVAL);
	const Sinks sk{opts, n_opts, nullptr, t, (uint8_t*)d_out, /*extended=*/true, /*alpha=*/(xflags & VP8G_X_ALPHA) != 0};
	return decode_batch(files, nullptr, n, filtered, threads, flags, sk, status);
}

// ... and with VP8G_X_LOSSLESS lossless files beside the lossy ones.
VP8G_API int vp8g_decode_webp_batch_tensor_any(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                               const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                               void* d_out, int* status) {
	if ((xflags & ~(VP8G_X_ALPHA | VP8G_X_LOSSLESS | VP8G_X_LOSSLESS_SCALE)) ||
	    ((xflags & VP8G_X_LOSSLESS_SCALE) && !(xflags & VP8G_X_LOSSLESS)) || !tensor_ok(t, d_out) || !opts_ok(opts, n_opts, n))
		return fail(EINVAL);
	const Sinks sk{opts,  n_opts, nullptr, t, (uint8_t*)d_out, /*extended=*/true, /*alpha=*/(xflags & VP8G_X_ALPHA) != 0,
	               /*lossless=*/(xflags & VP8G_X_LOSSLESS) != 0, /*lossless_scale=*/(xflags & VP8G_X_LOSSLESS_SCALE) != 0};
	return decode_batch(files, nullptr, n, filtered, threads, flags, sk, status);
}

// ... and with libwebp's own RGB for a lossy frame that is rescaled: chroma straight to the target size,
// VP8YuvToRgb per pixel, no upsampler.
VP8G_API int vp8g_decode_webp_batch_tensor_rgb(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                               const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                               void* d_out, int* status) {
	if ((xflags & ~(VP8G_X_ALPHA | VP8G_X_LOSSLESS | VP8G_X_LOSSLESS_SCALE)) ||
	    ((xflags & VP8G_X_LOSSLESS_SCALE) && !(xflags & VP8G_X_LOSSLESS)) || !tensor_ok(t, d_out) || !opts_ok(opts, n_opts, n))
		return fail(EINVAL);
	const Sinks sk{opts,  n_opts, nullptr, t, (uint8_t*)d_out, /*extended=*/true, /*alpha=*/(xflags & VP8G_X_ALPHA) != 0,
	               /*lossless=*/(xflags & VP8G_X_LOSSLESS) != 0, /*lossless_scale=*/(xflags & VP8G_X_LOSSLESS_SCALE) != 0, /*rgb_scale=*/true};
	return decode_batch(files, nullptr, n, filtered, threads, flags, sk, status);
}

// vp8g_decode_webp_batch_tensor_any without options, over pictures located by the caller (vp8g_device.h): the animation
// path's frames, which its parser has located already.
int vp8g::decode_located_tensor(const WebPStill* pics, uint32_t n, int filtered, uint32_t threads, uint32_t flags, const Vp8gTensorOpt* t,
                                uint32_t xflags, void* d_out, int* status) {
	if ((xflags & ~(VP8G_X_ALPHA | VP8G_X_LOSSLESS)) || !tensor_ok(t, d_out)) return fail(EINVAL);
	const Sinks sk{nullptr, 0, nullptr, t, (uint8_t*)d_out, /*extended=*/true, /*alpha=*/(xflags & VP8G_X_ALPHA) != 0,
	               /*lossless=*/(xflags & VP8G_X_LOSSLESS) != 0};
	return decode_batch(nullptr, pics, n, filtered, threads, flags, sk, status);
}

VP8G_API int vp8g_decode_webp_batch(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, Yuv420Image* outs,
                                    int* status) {
	return vp8g_decode_webp_batch_ex(files, n, filtered, threads, 0, outs, status);
}
