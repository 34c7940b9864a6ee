// vp8g_quad.inc -- the chain kernel, FOUR MB rows per wave (every batch of more frames than CUs,
// pick_chain; included by vp8g_kernels.hip inside namespace vp8g::{anonymous}, after frame_kernel,
// whose helpers and tables it uses).  DESIGN.md §3.1 (verdict r04 #1).  Reference: the per-MB raster loops of
// src/m06_recon/vp8_recon.c:444-684 and src/m07_loopfilter/vp8_loopfilter.c:214-280.
//
// The chain.  ONE workgroup of 16 waves per CU decodes a list of frames as one continuous chain of
// quads (four MB rows) -- global quad g of the list (the frames' quads one after another) belongs
// to wave g % 16 -- so no wave idles at a frame's end while another frame of the CU still has rows,
// and a heavy frame never runs alone on half the CU.  Two frames are in flight at once: frame j of
// the list uses table slot j & 1 (its dequant / loop-filter tables); quad 0 of frame j waits until
// frame j - 2, the slot's previous user, has finished its last quad (which implies all of its
// quads: a quad's last steps wait for the quad above to complete).  The list of workgroup b: the
// frames at positions b, 2W-1-b, 2W+b, 4W-1-b, ... of the batch sorted by descending cost class
// (snake order: every CU gets one of the heaviest and one of the lightest frames per two rounds),
// sorted in the prologue by wave 0 (stable counting sort over the cost classes, its scratch in the
// wave areas).  Progress words encode global quad * 2048 + steps done (kProgShift).
// Mirror split (ord_first bit 1, batches of at most two frames per workgroup): each frame is cut at
// quad h = ceil(quads / 2) into a top segment (quads [0, h), decoded by the frame's own workgroup,
// first in its list) and a bottom segment (quads [h, quads), decoded LAST by the mirror workgroup
// W-1-b).  Every workgroup thus decodes half of its own frames and half of its mirror's, which
// evens out the pairing of heavy and light frames (two 4K frames per CU cannot balance four fixture
// kinds).  The top segment's last quad stores the launch's epoch in the frame's flag after its last
// publish (its context row is in device memory already); the bottom segment's first quad waits for
// that flag.  Tops never wait across workgroups and bottoms come after every top of their list, so
// no cycle exists, and a top finishes in the first half of its workgroup's work, long before its
// bottom starts.
// Interleave (ord_first bit 2, same-size frames): list entries 2m, 2m + 1 form group m, whose 2P
// global quads alternate between them (quad k of frame 2m + e is global quad m * 2P + 2k + (e ^ (m & 1)),
// its quad above two global quads back, i.e. two waves back); an odd last entry runs alone.  2P is
// even, so a wave keeps its parity's role in every group: the swap on odd groups hands the even and
// the odd waves the snake's heavy and light list positions in turn.  Frame j uses table slot j & 3:
// its first quad waits for frame j - 4's last quad.
//
// Lanes 16h .. 16h + 15 ("quarter" h) work on MB(4k + h, t - 2h) at step t of quad k: the rows of a
// quad run two columns apart, as the two halves of a pair do in frame_kernel.  Every lane takes the
// roles of TWO lanes of frame_kernel's 32-lane half -- ln = l and ln = l + 16 (l = lane & 15) -- so
// the per-role tables (border setup, predictor roles, loop-filter lines, flush pieces) are the same;
// per step each phase does its work for both roles (B_PRED: both sub-block groups of the wavefront).
// Per step and wave the fixed costs (side-info permutes, dependency wait, publish, loop control,
// the wave-uniform shortcut ballots) now serve four MBs instead of two.
//
// Context.  Between the rows of a quad: three-column rings in the wave's LDS (ring h + 1 is written
// by quarter h -- rec[c] at step c + 2h, lf[c - 1] at the same step -- and read by quarter h + 1 two
// steps later).  Between quads (waves): quarter 3's entries go to device memory (one region of
// ctx_cols x 160 B per frame, the snapshot buffer; write-through stores), and quarter 0's lanes
// 0..9 load the entries of the row above (L1-bypassing loads) into ring 0 early in the step that
// uses them, right after its side info.
// Progress t means steps < t are visible.  Step t publishes it right after issuing the next step's
// prefetch, behind `s_waitcnt vmcnt(5)`: only those five loads may be pending, so every older
// operation -- step t - 1's context stores among them -- is acknowledged.  After the last step:
// vmcnt(0) and T.
// The quad below needs rec[t + 1] and lf[t] of this quad's quarter 3 (written at step t + 7) when it
// issues its loads early in step t, so it waits for progress >= t + 8.
// Frames: loop-filtered or unfiltered, with whole 16-B / 8-B row pieces (frame_kernel's fl_fast
// condition) or not (the general instantiation's byte path); no loop-filter-only frames (pick_chain
// on the host keeps such batches out).
// The placements and layouts that were measured against these (publish and context-load timing,
// prefetch depth, LDS bank shift, B_PRED register hand-off, store pairing and cache policy) are in
// DESIGN.md §3.2, "Retired experiment code".

// Loop filter of one lane's luma line and chroma line (quads: role 0 is always luma, role 1 always
// chroma, so each runs only its own edges -- frame_kernel's lanes mix both and the chroma lanes issue
// the two luma-only edges masked -- and a chroma line gathers its 12 bytes, not 20).
template <int kA, int kB>
DEV void gather12(const uint8_t* a, const uint8_t* b, int* px) {
	const uint32_t la = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)a;
	const uint32_t lb = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)b;
	asm volatile(
	    "ds_read_u8 %0, %12\n"
	    "ds_read_u8 %1, %12 offset:%14\n"
	    "ds_read_u8 %2, %12 offset:%15\n"
	    "ds_read_u8 %3, %12 offset:%16\n"
	    "ds_read_u8 %4, %13\n"
	    "ds_read_u8 %5, %13 offset:%17\n"
	    "ds_read_u8 %6, %13 offset:%18\n"
	    "ds_read_u8 %7, %13 offset:%19\n"
	    "ds_read_u8 %8, %13 offset:%20\n"
	    "ds_read_u8 %9, %13 offset:%21\n"
	    "ds_read_u8 %10, %13 offset:%22\n"
	    "ds_read_u8 %11, %13 offset:%23\n"
	    "s_waitcnt lgkmcnt(0)"
	    : "=&v"(px[0]), "=&v"(px[1]), "=&v"(px[2]), "=&v"(px[3]), "=&v"(px[4]), "=&v"(px[5]), "=&v"(px[6]), "=&v"(px[7]), "=&v"(px[8]),
	      "=&v"(px[9]), "=&v"(px[10]), "=&v"(px[11])
	    : "v"(la), "v"(lb), "i"(kA), "i"(2 * kA), "i"(3 * kA), "i"(kB), "i"(2 * kB), "i"(3 * kB), "i"(4 * kB), "i"(5 * kB), "i"(6 * kB),
	      "i"(7 * kB)
	    : "memory");
#pragma unroll
	for (int i = 0; i < 12; i++) __builtin_assume((uint32_t)px[i] < 256u);
}
template <bool kSimple>
DEV void lf_mb_luma(const LfLine& L, bool en, bool mb_v, bool mb_h, bool inner, int E, int I, int T) {
	int px[20];
	uint8_t* const Lp = L.Lp;
	uint8_t* const Mp = L.Mp;
	PRIO_AFTER(8, 5);
	gather20<1, 1>(Lp, Mp, px);
	PRIO_AFTER(9, 8);
	lf_line<kSimple>(px, en && mb_v, en && inner, true, E, I, T);
	if (en) {
		st32(Lp, pack4b(px[0], px[1], px[2], px[3]));
		st32(Mp, pack4b(px[4], px[5], px[6], px[7]));
		st32(Mp + 4, pack4b(px[8], px[9], px[10], px[11]));
		st32(Mp + 8, pack4b(px[12], px[13], px[14], px[15]));
		st32(Mp + 12, pack4b(px[16], px[17], px[18], px[19]));
	}
	wave_lds_sync();
	uint8_t* const colp = L.colp;
	PRIO_AFTER(8, 9);
	gather20<kTP, kTP>(colp, colp + 4 * kTP, px);
	PRIO_AFTER(9, 8);
	lf_line<kSimple>(px, en && mb_h, en && inner, true, E, I, T);
	if (en) {
#pragma unroll
		for (int i = 1; i < 18; i++) stb(colp + kTP * i, px[i]);
	}
	wave_lds_sync();
}
DEV void lf_mb_chroma(const LfLine& L, bool en, bool mb_v, bool mb_h, bool inner, int E, int I, int T) {  // normal filter only
	int px[12];
	uint8_t* const Lp = L.Lp;
	uint8_t* const Mp = L.Mp;
	PRIO_AFTER(8, 5);
	gather12<1, 1>(Lp, Mp, px);
	PRIO_AFTER(9, 8);
	lf_mb_edge(px + 0, en && mb_v, 2 * (E + 2) + I, I, T);
	lf_sub_edge(px + 4, en && inner, 2 * E + I, I, T);
	if (en) {
		st32(Lp, pack4b(px[0], px[1], px[2], px[3]));
		st32(Mp, pack4b(px[4], px[5], px[6], px[7]));
		st32(Mp + 4, pack4b(px[8], px[9], px[10], px[11]));
	}
	wave_lds_sync();
	uint8_t* const colp = L.colp;
	PRIO_AFTER(8, 9);
	gather12<kTP, kTP>(colp, colp + 4 * kTP, px);
	PRIO_AFTER(9, 8);
	lf_mb_edge(px + 0, en && mb_h, 2 * (E + 2) + I, I, T);
	lf_sub_edge(px + 4, en && inner, 2 * E + I, I, T);
	if (en) {
#pragma unroll
		for (int i = 1; i < 10; i++) stb(colp + kTP * i, px[i]);
	}
	wave_lds_sync();
}

// Paired pixel stores (role 0's luma rows and both roles' chroma rows, in both instantiations): a
// lane keeps its piece of an even MB column for one step and stores at the odd column.  Luma (16-B
// pieces, the most a lane stores): the lanes l and l ^ 1 (same piece column) trade halves, so that
// one store instruction writes each of the two rows as two adjacent pieces -- 32 B from two lanes
// instead of two 16-B pieces a step apart.  Chroma (8-B pieces): the kept piece and the current one
// are 16 adjacent bytes of the lane's own row and go out as one 16-B store, with no exchange.
//
// A step's vector-memory operations, in issue order (vmcnt counts in issue order, and the step loop's
// `s_waitcnt vmcnt(N)` are written against this list): the context load (1, after the side info), the
// next step's prefetch (5, after the residual), the pixel stores (5: role 0's luma as two paired
// stores, role 1's luma, one chroma store per role) and quarter 3's context stores (3): 14 in all.
// The single stores of a last column come on top, in few steps; more operations in flight only make
// a wait stricter than it has to be.
constexpr int kQPrefLoads = 5;
constexpr int kQStoresPerStep = 5 + 3;
// Cache policy of the pixel stores: write-through (sc1).  With 32-B luma / 16-B chroma pieces a
// write-back L2 still refilled the partly written lines from HBM (1 564 B read per MB against 820);
// sc1 writes them straight through (DESIGN.md §3.1, r05p2).
constexpr int kQStoreCpol = kCpolSc1;
DEV uint32_t opq_u(uint32_t v) {  // (opaque to the optimiser: keeps bit arithmetic from becoming compares)
	asm("" : "+v"(v));
	return v;
}
// The pair exchange of a piece, as VOP2 DPP selects (quad_perm [1,0,3,2]: the partner lane l ^ 1):
// dA = even lanes' held, odd lanes' partner's cur; dB = odd lanes' cur, even lanes' partner's held.
// (One s_nop covers the VALU-write -> DPP-read hazard the compiler does not see inside asm.  s_not_b64
// writes SCC: without "scc" among the clobbers the compiler may keep a comparison's SCC across the
// block -- round 6, a rescheduled build lost the even last column's single stores that way.)
constexpr uint64_t kEvenLanes = 0x5555555555555555ull;
#define VP8G_SELSWAP(d, keep, other) "v_cndmask_b32_dpp " d ", " other ", " keep ", vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
DEV void pair_swap(const u32x4& held, const u32x4& cur, u32x4& dA, u32x4& dB) {
	asm("s_mov_b64 vcc, %16\n\ts_nop 1\n\t"
	    VP8G_SELSWAP("%0", "%8", "%12") VP8G_SELSWAP("%1", "%9", "%13") VP8G_SELSWAP("%2", "%10", "%14") VP8G_SELSWAP("%3", "%11", "%15")
	    "s_not_b64 vcc, vcc\n\t"
	    VP8G_SELSWAP("%4", "%12", "%8") VP8G_SELSWAP("%5", "%13", "%9") VP8G_SELSWAP("%6", "%14", "%10") VP8G_SELSWAP("%7", "%15", "%11")
	    : "=&v"(dA.x), "=&v"(dA.y), "=&v"(dA.z), "=&v"(dA.w), "=&v"(dB.x), "=&v"(dB.y), "=&v"(dB.z), "=&v"(dB.w)
	    : "v"(held.x), "v"(held.y), "v"(held.z), "v"(held.w), "v"(cur.x), "v"(cur.y), "v"(cur.z), "v"(cur.w), "s"(kEvenLanes)
	    : "vcc", "scc");
}
#undef VP8G_SELSWAP
DEV void qst128(Rsrc r, uint32_t off, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)off, 0, kQStoreCpol); }
DEV void qst64(Rsrc r, uint32_t off, u32x2 v) { __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)off, 0, kQStoreCpol); }

constexpr uint32_t kSegTop = 1u, kSegBottom = 2u, kSegMask = 0x3FFFFFFFu;  // list entry: frame | tag << 30 (mirror split)

// kWP: every frame of the batch has whole row pieces (the bench's batches); the general instantiation
// adds the byte path for pieces cut by the right edge or unaligned planes (+1 % when used for
// whole-piece batches: the extra frame state costs SGPRs, r05q18).
template <int NW, bool kWP>
__global__ __launch_bounds__(NW * 64, min_waves_per_simd<NW>()) void quad_kernel(const Vp8gFrameDesc* __restrict__ descs, Vp8gBatchArrays A,
                                                                                 uint8_t* __restrict__ out, uint32_t ctx_cols,
                                                                                 uint8_t* __restrict__ gctx, uint32_t epoch,
                                                                                 uint32_t* __restrict__ gflags, uint32_t ord_first,
                                                                                 uint32_t n_chain) {
	static_assert(NW == 16, "the quad kernel's LDS layout is sized for 16 waves");
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int lane0 = (int)(threadIdx.x & 63);
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const bool il = (ord_first & 4u) != 0;
	uint32_t* const chain_list = (uint32_t*)(smem + kQList);
	auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
	auto quads_of = [&](uint32_t fi) { return (descs[fi].mb_rows + 3u) >> 2; };

	// ---- this workgroup's frame list (see the top of the file); ord_first bit 0: cost-sorted positions
	{
		const uint32_t Wg = gridDim.x, b = blockIdx.x, n = n_chain;
		if (wave == 0) {
			uint32_t* const hist = (uint32_t*)(smem + kHdrBytes);
			uint32_t* const sorted = hist + kCostClasses;
			const uint64_t lt = (1ull << lane0) - 1ull;
			if (ord_first & 1u) {
				for (int i = lane0; i < (int)kCostClasses; i += 64) hist[i] = 0u;
				wave_lds_sync();
				for (int pass = 0; pass < 2; pass++) {
					for (uint32_t c0 = 0; c0 < n; c0 += 64) {
						const uint32_t i = c0 + (uint32_t)lane0;
						const bool valid = i < n;
						const uint32_t cls = valid ? cost_class(descs[i]) : 0u;
						uint64_t rem = __ballot(valid);
						while (rem) {  // one distinct class per iteration (peeled by its first lane)
							const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cls, (int)__builtin_ctzll(rem));
							const uint64_t mk = __ballot(valid && cls == c);
							const uint32_t base = hist[c];
							wave_lds_sync();
							if (pass == 1 && ((mk >> lane0) & 1ull)) sorted[base + (uint32_t)__popcll(mk & lt)] = i;
							if (lane0 == (int)__builtin_ctzll(mk)) hist[c] = base + (uint32_t)__popcll(mk);
							wave_lds_sync();
							rem &= ~mk;
						}
					}
					if (pass == 0) {  // counts -> start positions, heaviest class first
						if (lane0 == 0) {
							uint32_t acc = 0;
							for (int c = (int)kCostClasses - 1; c >= 0; c--) {
								const uint32_t h = hist[c];
								hist[c] = acc;
								acc += h;
							}
						}
						wave_lds_sync();
					}
				}
			}
			// snake positions of workgroup b (increasing in j), empty descriptors left out.  Mirror
			// split: workgroup b decodes the top halves of its own frames, then the bottom halves of
			// workgroup W-1-b's frames (entry tags, kSegTop / kSegBottom)
			uint32_t cnt = 0;
			auto add_list = [&](uint32_t bb, uint32_t tag) {
				for (uint32_t j0 = 0;; j0 += 64) {
					const uint32_t j = j0 + (uint32_t)lane0;
					const uint32_t pos = j * Wg + ((j & 1u) ? Wg - 1u - bb : bb);
					const bool valid = pos < n;
					if (__ballot(valid) == 0ull) break;
					const uint32_t fi = valid ? ((ord_first & 1u) ? sorted[pos] : pos) : 0u;
					const bool keep = valid && descs[fi].mb_cols != 0 && descs[fi].mb_rows != 0 && (tag != kSegBottom || descs[fi].mb_rows > 4u);
					const uint64_t mk = __ballot(keep);
					if (keep) chain_list[cnt + (uint32_t)__popcll(mk & lt)] = fi | (tag << 30);
					cnt += (uint32_t)__popcll(mk);
				}
			};
			const bool split = (ord_first & 2u) != 0;
			add_list(b, split ? kSegTop : 0u);
			if (split) add_list(Wg - 1u - b, kSegBottom);
			if (lane0 == 0) *(uint32_t*)(smem + kMisc) = cnt;
		}
		__syncthreads();
	}
	const uint32_t m_chain = uni(*(const uint32_t*)(smem + kMisc));

	for (int i = (int)threadIdx.x; i < kBpModes * 16 * (kBpEntry / 4); i += NW * 64) ((uint32_t*)(smem + kBpTable))[i] = kBpTab.v[i];
	if (threadIdx.x < 64) ((uint32_t*)(smem + kRoleTab))[threadIdx.x] = kPredRoleTab.v[threadIdx.x];
	uint32_t bt0 = kBorderTab.v[lane0 & 15], bt1 = kBorderTab.v[(lane0 & 15) + 16];  // the two border roles
	auto put_tables = [&](const Vp8gFrameDesc& Df, uint32_t tabo_, int l) {
		if (l < 24) {
			const int sg = l / 6, kk = l % 6, cl = kk >> 1;
			((int16_t*)(smem + kDqTable + tabo_))[(cl * 4 + sg) * 2 + (kk & 1)] = Df.dq[sg][kk];
		}
		if (l < 32) smem[kLfTable + tabo_ + l] = Df.lf[l >> 3][(l >> 2) & 1][l & 3];
	};
	if (threadIdx.x < 16) ((uint32_t*)(smem + kProgress))[threadIdx.x] = 0;
	__syncthreads();
	if (m_chain == 0) return;

	// ---- the current frame
	const Vp8gFrameDesc* Dp;
	uint32_t C, R, flags, W, H, CW, CH, sy, suv, vofs, nq, tabo;
	bool wp;  // whole row pieces: every 16-B luma / 8-B chroma piece inside the frame and aligned
	uint64_t mb0;
	uint8_t* outY;
	uint8_t* outU;
	uint8_t* gq;
	auto set_frame = [&](uint32_t fi, uint32_t slot) {
		Dp = descs + fi;
		const Vp8gFrameDesc& D = *Dp;
		C = D.mb_cols, R = D.mb_rows;
		flags = D.flags;
		mb0 = D.mb_offset;
		outY = out + D.out_y;
		outU = out + D.out_u;
		W = D.width, H = D.height, CW = (D.width + 1) >> 1, CH = (D.height + 1) >> 1;
		sy = D.stride_y, suv = D.stride_uv;
		vofs = (uint32_t)(D.out_v - D.out_u);
		gq = gctx + (size_t)fi * ctx_cols * kCtxBytesPerCol;
		wp = kWP || (W == 16u * C && CW == 8u * C);
		nq = (R + 3u) >> 2;
		tabo = slot * (uint32_t)kTabStride;
	};
	uint32_t* const prog = (uint32_t*)(smem + kProgress);
	bool dead = false;
#ifdef VP8G_STAMPS
	// phases as frame_kernel's (bench.py names them); 4 = the rec capture
	uint64_t st_acc[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint64_t st_prev = __builtin_amdgcn_s_memtime();
	const uint64_t st_t0 = __builtin_amdgcn_s_memrealtime();
#endif
	auto wait_prog = [&](uint32_t pw, uint32_t need) {
		uint32_t spins = 0;
		uint64_t t0 = 0;
		while (__hip_atomic_load(prog + pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) {
			__builtin_amdgcn_s_sleep(VP8G_WAIT_SLEEP);
			if ((++spins & 1023u) == 0) {
				const uint64_t now = __builtin_amdgcn_s_memrealtime();
				if (t0 == 0) t0 = now;
				else if (now - t0 > (uint64_t)VP8G_WAIT_TICKS) {
					if (lane0 == 0) atomicOr(A.status, VP8G_ERR_TIMEOUT);
					dead = true;
					break;
				}
			}
		}
		asm volatile("" ::: "memory");
	};
	auto wait_flag = [&](uint32_t* flag, uint32_t ep) {
		uint32_t spins = 0;
		uint64_t t0 = 0;
		// (skew build, early_site = kSkQFlag: the previous epoch's flag accepted too.  Memory-safe: the
		// bottom segment then only loads the same context entries of `gq` sooner -- pixel bytes that feed
		// prediction and filter arithmetic, never an address)
		while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ep &&
		       !(VP8G_SKEW_EARLY(kSkQFlag) && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ep - 1u)) {
			__builtin_amdgcn_s_sleep(2);
			if ((++spins & 255u) == 0) {
				const uint64_t now = __builtin_amdgcn_s_memrealtime();
				if (t0 == 0) t0 = now;
				else if (now - t0 > (uint64_t)VP8G_WAIT_TICKS) {
					if (lane0 == 0) atomicOr(A.status, VP8G_ERR_TIMEOUT);
					dead = true;
					break;
				}
			}
		}
		asm volatile("" ::: "memory");
	};
	auto seg_k0 = [&](uint32_t e) { return (e >> 30) == kSegBottom ? (quads_of(e & kSegMask) + 1u) >> 1 : 0u; };
	auto seg_units = [&](uint32_t e) {
		const uint32_t nn = quads_of(e & kSegMask), tag = e >> 30;
		return tag == 0u ? nn : (tag == kSegTop ? (nn + 1u) >> 1 : nn >> 1);
	};
	auto steps_of = [](uint32_t Cc, uint32_t Rr, uint32_t kq) { return Cc + 2u * (min(4u, Rr - 4u * kq) - 1u); };
	uint32_t jf = 0, gbase = 0, ecur = uni(chain_list[0]), np_c = seg_units(ecur);
	const uint32_t ilP = il ? uni(quads_of(ecur & kSegMask)) : 0u;
	uint32_t flags_l = 0;

	for (uint32_t g = (uint32_t)wave;; g += NW) {
		// (diagnostic VP8G_ABLATE & 32: only the first four rounds of units -- the tail's price is the time
		// beyond 64 / 68 of the whole; units wait only on earlier ones, so dropping the last is safe)
		if constexpr ((VP8G_ABLATE & 32) != 0) {
			if (g >= 4u * (uint32_t)NW) break;
		}
		uint32_t k;
		bool has_pred, from_snap = false, snap_out = false;
		uint32_t fcur, dg = 1;
		if (il) {
			const uint32_t gp = 2u * ilP, m = g / gp, off = g - m * gp;
			if (m >= (m_chain >> 1)) {
				if (m > (m_chain >> 1) || !(m_chain & 1u) || off >= ilP) break;
				jf = 2u * m, k = off, dg = 1u;
			} else {
				jf = 2u * m + ((off ^ m) & 1u), k = off >> 1, dg = 2u;
			}
			jf = uni(jf), k = uni(k), dg = uni(dg);
			ecur = uni(chain_list[jf]);
			fcur = ecur & kSegMask;
			set_frame(fcur, jf & 3u);
			has_pred = k > 0;
			if (k == 0) {
				if (jf >= 4u && !dead) {
					const uint32_t j4 = jf - 4u, last4 = (j4 >> 1) * gp + 2u * (ilP - 1u) + ((j4 ^ (j4 >> 1)) & 1u);
					VP8G_SKEW_CENSUS(kSkQSlot, __hip_atomic_load(prog + last4 % NW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >=
					                               (last4 << kProgShift) + steps_of(C, R, ilP - 1u));
					wait_prog(last4 % NW, (last4 << kProgShift) + steps_of(C, R, ilP - 1u));
				}
				put_tables(*Dp, tabo, lane0);
				wave_lds_sync();
			} else if (!dead) {
				VP8G_SKEW_CENSUS(kSkQStart, __hip_atomic_load(prog + (wave + NW - (int)dg) % NW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >=
				                                ((g - dg) << kProgShift) + 1u);
				wait_prog((uint32_t)((wave + NW - (int)dg) % NW), ((g - dg) << kProgShift) + 1u);
			}
		} else {
			while (g >= gbase + np_c) {
				gbase += np_c;
				if (++jf >= m_chain) break;
				ecur = uni(chain_list[jf]);
				np_c = seg_units(ecur);
			}
			if (jf >= m_chain) break;
			jf = uni(jf), gbase = uni(gbase), ecur = uni(ecur);
			fcur = ecur & kSegMask;
			set_frame(fcur, jf & 1u);
			const uint32_t tag = ecur >> 30, k0 = seg_k0(ecur);
			k = k0 + (g - gbase);
			has_pred = g > gbase;
			snap_out = tag == kSegTop && g + 1u == gbase + np_c && np_c < nq;
			if (g == gbase) {
				if (jf >= 2 && !dead) {
					const uint32_t e2 = uni(chain_list[jf - 2u]), f2 = e2 & kSegMask;
					const uint32_t last2 = gbase - seg_units(uni(chain_list[jf - 1u])) - 1u;
					const uint32_t kl2 = seg_k0(e2) + seg_units(e2) - 1u;
					VP8G_SKEW_CENSUS(kSkQSlot, __hip_atomic_load(prog + last2 % NW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >=
					                               (last2 << kProgShift) + steps_of(descs[f2].mb_cols, descs[f2].mb_rows, kl2));
					wait_prog(last2 % NW, (last2 << kProgShift) + steps_of(descs[f2].mb_cols, descs[f2].mb_rows, kl2));
				}
				if (tag == kSegBottom) {  // the row above: the top segment's last quad, in device memory
					if (!dead) {
						VP8G_SKEW_CENSUS(kSkQFlag, __hip_atomic_load(gflags + fcur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch);
						wait_flag(gflags + fcur, epoch);
					}
					from_snap = true;
				}
				put_tables(*Dp, tabo, lane0);
				wave_lds_sync();
			} else if (!dead) {
				VP8G_SKEW_CENSUS(kSkQStart, __hip_atomic_load(prog + (wave + NW - 1) % NW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >=
				                                ((g - 1u) << kProgShift) + 1u);
				wait_prog((uint32_t)((wave + NW - 1) % NW), ((g - 1u) << kProgShift) + 1u);
			}
		}
		const Rsrc rY = plane_rsrc(outY, sy * H), rC = plane_rsrc(outU, vofs + suv * CH);
		const Rsrc rQ = plane_rsrc(gq, C * (uint32_t)kCtxBytesPerCol);
		const bool has_hbm = has_pred || from_snap;
		const uint32_t rA = 4u * k, nrows = min(4u, R - rA), T = C + 2u * (nrows - 1u);
		const uint32_t Tprev = C + 6u;  // (the quad above is a full one)
		const uint32_t pw = (uint32_t)((wave + NW - (int)dg) % NW), gprev = g - dg;
		uint8_t* const wq = smem + wave * kQWaveBytes;

		// ---- per-lane words of this quad (two roles: ln = l, l + 16)
		uint64_t cb0, cb1, sbase;
		uint32_t csh1;
		{
			const int h = lane0 >> 4, l = lane0 & 15;
			const uint64_t mrow = mb0 + __umul24(min(rA + (uint32_t)h, R - 1u), C);
			cb0 = (uint64_t)A.coeff_y + (mrow << 9) + (uint32_t)l * 32u;
			const int ln = l + 16;
			const bool isb = ln == 25;
			const uint32_t sh = ln < 24 ? 7u : (isb ? 4u : 5u);
			const uint32_t boff = ln < 24 ? (uint32_t)(ln & 3) * 32u : 0u;
			const uint64_t base = vsel(ln < 20, (uint64_t)A.coeff_u, vsel(ln < 24, (uint64_t)A.coeff_v, vsel(isb, (uint64_t)A.bmode, (uint64_t)A.coeff_y2)));
			cb1 = base + (mrow << sh) + boff;
			csh1 = sh;
			const int q = ln & 3;
			sbase = vsel(q == 2, (uint64_t)A.ymode, vsel(q == 3, (uint64_t)A.uv_mode, vsel(q == 0, (uint64_t)A.segment_id, (uint64_t)A.has_coeff))) + mrow;
		}
		uint32_t lf_vp0, lf_hp0, lf_vp1, lf_hp1;
		auto lf_words = [&](int ln, uint32_t& vp, uint32_t& hp) {
			const int h = lane0 >> 4;
			const bool isy = ln < 16;
			const uint32_t cp = (uint32_t)(ln >> 3) & 1u, hb = (uint32_t)(kHdrBytes + h * kQuarterBytes);
			const uint32_t rowp = hb + (isy ? (uint32_t)(kLfY + (4 + ln) * kTP) : (uint32_t)kLfUV + (4u + (uint32_t)(ln & 7)) * kTP + cp * kCV);
			const uint32_t col = hb + (isy ? (uint32_t)(kLfY + ln) : (uint32_t)kLfUV + cp * kCV + (uint32_t)(ln & 7));
			const uint32_t d = isy ? 16u : 8u;
			vp = rowp | ((rowp + d) << 16);
			hp = col | ((col + d) << 16);
		};
		lf_words(lane0 & 15, lf_vp0, lf_hp0);
		lf_words((lane0 & 15) + 16, lf_vp1, lf_hp1);
		// flush words of a role (whole-piece frames): output offsets with the lane's column shift folded
		// in (kNoStore: never stored to the planes this quad), the context-entry offset of the rows the
		// next MB row still filters (luma < 2^30, chroma | 2^30, none ~0), tile sources by slot
		uint32_t fY0, fC0, lfo0, sY0, sC0, fY1, fC1, lfo1, sY1, sC1;
		auto fl_words = [&](int ln, uint32_t& oY, uint32_t& oC, uint32_t& lfo, uint32_t& sYw, uint32_t& sCw) {
			const int h = lane0 >> 4;
			const uint32_t rr = rA + (uint32_t)h;
			const bool row_ok = (uint32_t)h < nrows;
			const uint32_t prowY = rr * 16u + (uint32_t)ln - 4u;
			const int pc = ln >= 12 ? 1 : 0, kc = ln - 12 * pc;
			const uint32_t prowC = rr * 8u + (uint32_t)kc - 4u;
			const bool nlast = rr + 1u < R;
			const bool visY = row_ok && ln < 20 && prowY < H, ctxY = ln >= 16 && nlast;
			const bool visC = row_ok && ln < 24 && prowC < CH, ctxC = kc >= 8 && nlast;
			const bool topY = ln < 4, topC = kc < 4;
			const uint32_t shy = 2u * (uint32_t)h + (topY ? 0u : 1u), shc = 2u * (uint32_t)h + (topC ? 0u : 1u);
			const uint32_t hb = (uint32_t)(kHdrBytes + h * kQuarterBytes);
			const uint32_t sY = hb + kLfY + (uint32_t)ln * kTP, sC = hb + kLfUV + (uint32_t)(pc * kCV + kc * kTP);
			sYw = (sY + (topY ? 0u : 16u)) | ((sY + (topY ? 16u : 0u)) << 16);
			sCw = (sC + (topC ? 0u : 8u)) | ((sC + (topC ? 8u : 0u)) << 16);
			oY = visY && !ctxY ? __umul24(prowY, sy) - shy * 16u : kNoStore;
			oC = visC && !ctxC ? (pc ? vofs : 0u) + __umul24(prowC, suv) - shc * 8u : kNoStore;
			lfo = visY && ctxY ? (uint32_t)(ln - 16) * 16u
			                   : (visC && ctxC ? (0x40000000u | (64u + (uint32_t)pc * 32u + (uint32_t)(kc - 8) * 8u)) : ~0u);
		};
		fl_words(lane0 & 15, fY0, fC0, lfo0, sY0, sC0);
		fl_words((lane0 & 15) + 16, fY1, fC1, lfo1, sY1, sC1);

		// ring 0 <- rec[0], lf[0], rec[1] of the row above (quarter 0's lanes 0..11)
		if (has_hbm) {
			// (skew build, early_site = kSkQRing0: one step less.  Memory-safe: the load below reads the same
			// three context entries of `gq` whatever they hold; they are pixel bytes, stored to LDS as such)
			if (has_pred && !dead) {
				VP8G_SKEW_CENSUS(kSkQRing0, __hip_atomic_load(prog + pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >=
				                                (gprev << kProgShift) + min(8u, Tprev) - VP8G_SKEW_EARLY(kSkQRing0));
				wait_prog(pw, (gprev << kProgShift) + min(8u, Tprev) - VP8G_SKEW_EARLY(kSkQRing0));
			}
			const uint32_t l = (uint32_t)lane0;
			const uint32_t col = l < 10u ? 0u : 1u, o = l < 10u ? 16u * l : 16u * (l - 10u);
			const bool ok = l < 12u && col < C;
			const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rQ, (int)(ok ? col * (uint32_t)kCtxBytesPerCol + o : kNoStore), 0, kCpolSc1);
			if (ok) st128(wq + kQRings + col * kCtxBytesPerCol + o, v);
			wave_lds_sync();
		}

		// the step's coefficients, one step ahead: role 0 = Y block l, role 1 = U / V block (l < 8),
		// Y2 (8, 10..15), the 16 B_PRED modes (9); side bytes in lanes l = 10..13
		struct QPref {
			u32x4 a0, b0, a1, b1;
			uint32_t side;
		};
		auto qprefetch = [&](int lane, int tt) -> QPref {
			QPref p;
			const int h = lane >> 4, l = lane & 15;
			const uint32_t cn = (uint32_t)min(max(tt - 2 * h, 0), (int)C - 1);
			const gu32x4* s0 = (const gu32x4*)(cb0 + ((uint64_t)cn << 9));
			const gu32x4* s1 = (const gu32x4*)(cb1 + ((uint64_t)cn << csh1));
			// (the side byte first, the B_PRED modes second: vmcnt counts in issue order, so the side-info
			// permutes wait for one load, the modes' for two, and the coefficients have until the
			// dequantisation)
			p.side = ((const __attribute__((address_space(1))) uint8_t*)sbase)[cn];
			p.a1 = *s1;  // (the B_PRED modes' permutes come next)
			p.a0 = s0[0];
			p.b0 = s0[1];
			p.b1 = *(l == 9 ? s1 : s1 + 1);
			return p;
		};
		// (the loop's per-lane words are made live here, before the prefetch: reloaded from scratch at
		// the end of the setup instead, those loads came after the prefetch and the first use in the loop
		// waited for them with vmcnt(0) -- at the top of every step)
		asm volatile("" : "+v"(bt0), "+v"(bt1), "+v"(fY0), "+v"(fC0), "+v"(lfo0), "+v"(sY0), "+v"(sC0));
		asm volatile("" : "+v"(fY1), "+v"(fC1), "+v"(lfo1), "+v"(sY1), "+v"(sC1), "+v"(lf_vp0), "+v"(lf_hp0), "+v"(lf_vp1), "+v"(lf_hp1));
		asm volatile("" : "+v"(cb0), "+v"(cb1), "+v"(sbase), "+v"(csh1));
		QPref cur = qprefetch(lane0, 0);
		// Everything of the setup drained before the step loop (once per quad): with nothing outstanding
		// on entry, the waits the compiler places in the loop are set by its back edge alone -- vmcnt(12)
		// and (11) for the side byte and the modes at the top (the rest of the prefetch and the previous
		// step's eight stores are younger), vmcnt(9) and (8) for the coefficients (the context load is
		// younger too); the context load itself is covered by the publish's wait.  (Dummy operations to
		// match the back edge's count were fragile: the compiler merged identical ones and placed scratch
		// reloads after them, and the loop then waited vmcnt(0) -- every store of the previous step -- at
		// the top of each step.)
		u32x4 mbx = u32x4{0u, 0u, 0u, 0u};
		u32x4 hY0 = mbx;  // (paired stores: the pieces kept from the even column)
		u32x2 hC0 = u32x2{0u, 0u}, hC1 = hC0;
		__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
		flags_l = (uint32_t)__builtin_amdgcn_readfirstlane((int)flags);

		auto load_dq4 = [&](int ln_) -> u32x4 { return *(const u32x4*)(smem + kDqTable + tabo + 16 * (ln_ < 16 ? 0 : (ln_ < 24 ? 1 : 2))); };
		auto pick_dq = [&](const u32x4& dq4, int seg_) -> uint32_t {
			const uint64_t m1 = __builtin_amdgcn_ballot_w64((seg_ & 1) != 0), m2 = __builtin_amdgcn_ballot_w64((seg_ & 2) != 0);
			uint32_t lo, hi, r;
			asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(lo) : "v"(dq4.x), "v"(dq4.y), "s"(m1));
			asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(hi) : "v"(dq4.z), "v"(dq4.w), "s"(m1));
			asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(lo), "v"(hi), "s"(m2));
			return r;
		};

		for (uint32_t t = 0; t < T; t++) {
			int lane = lane0;
			asm volatile("" : "+v"(lane));
			asm volatile("" : "+v"(bt0), "+v"(bt1), "+s"(flags_l));
			asm volatile("" : "+v"(fY0), "+v"(fC0), "+v"(lfo0), "+v"(sY0), "+v"(sC0));
			asm volatile("" : "+v"(fY1), "+v"(fC1), "+v"(lfo1), "+v"(sY1), "+v"(sC1));
			asm volatile("" : "+v"(lf_vp0), "+v"(lf_hp0), "+v"(lf_vp1), "+v"(lf_hp1));
			const bool lf_on = (flags_l & VP8G_F_LOOPFILTER) != 0;
			const bool simple = (flags_l & VP8G_F_SIMPLE) != 0;
			const int h = lane >> 4, l = lane & 15;
			const uint32_t r = rA + (uint32_t)h;
			const int c = (int)t - 2 * h;
			const bool act = (uint32_t)h < nrows && c >= 0 && c < (int)C;
			const uint32_t cu = (uint32_t)c;
			const int slot = c & 1;
			uint8_t* const hv = wq + kHdrBytes + __umul24((uint32_t)h, (uint32_t)kQuarterBytes);  // this quarter's area (24-bit multiply: h comes from a laundered lane id)
			uint8_t* const tY = hv + kLfY;
			uint8_t* const tC = hv + kLfUV;
			uint8_t* const abY = hv + kAbY;
			uint8_t* const left = hv + kLeft;
			uint8_t* const rin = wq + kQRings + __umul24((uint32_t)h, (uint32_t)kRingBytes);  // ring h: the row above this quarter
			uint8_t* const rout = rin + kRingBytes;               // ring h + 1 (quarters 0..2)
			// ring slots: column c mod 3 (c = t - 2h == t + h mod 3), c + 1, c - 1
			uint32_t m0 = t % 3u + (uint32_t)h;
			m0 = m0 >= 3u ? m0 - 3u : m0;
			const uint32_t m1 = m0 == 2u ? 0u : m0 + 1u, mm = m0 == 0u ? 2u : m0 - 1u;
#ifdef VP8G_STAMPS
			// (this step's prefetch complete: only the previous step's stores, issued after it, may be pending)
			asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kQStoresPerStep) : "memory");
			STAMP(13);
#endif
			// (the progress word of the quad above read ahead of the side info: the poll's LDS round trip
			// overlaps the side-info permutes)
			uint32_t p_early = 0xFFFFFFFFu;
			if (t > 0 && has_pred && !dead) p_early = __hip_atomic_load(prog + pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);

			// ---------------------------------------------- side info (quarter's lanes 9..13)
			const u32x4 dq4a = load_dq4(l), dq4b = load_dq4(l + 16);
			const int sdl = (16 * h + 10) * 4, bml = (16 * h + 9) * 4;
			const int ymode = __builtin_amdgcn_ds_bpermute(sdl, (int)cur.side);
			const int uvmode = __builtin_amdgcn_ds_bpermute(sdl + 4, (int)cur.side);
			const int seg = __builtin_amdgcn_ds_bpermute(sdl + 8, (int)cur.side) & 3;
			const int hasc = __builtin_amdgcn_ds_bpermute(sdl + 12, (int)cur.side);
			const u32x4 bmw = u32x4{(uint32_t)__builtin_amdgcn_ds_bpermute(bml, (int)cur.a1.x), (uint32_t)__builtin_amdgcn_ds_bpermute(bml, (int)cur.a1.y),
			                        (uint32_t)__builtin_amdgcn_ds_bpermute(bml, (int)cur.a1.z), (uint32_t)__builtin_amdgcn_ds_bpermute(bml, (int)cur.a1.w)};
			const bool bpred = ymode == 4;
			const uint32_t y0 = r * 16, cy0 = r * 8;
			// The row above's context for this step (rec[t + 1], lf[t] of the quad above's quarter 3): the
			// wait for progress >= t + 8 (the spin entered only if the value read above is short), then the
			// load -- an L2 hit, hidden behind the residual, put into ring 0 after it.  (Stamps builds count
			// this wait as side info.)
			if (t > 0) {
				// (skew build, early_site = kSkQNeed: t + 7.  Memory-safe: the load below takes its address from
				// t and the lane alone, so the same entries of `gq` are read, only sooner; their bytes are pixels
				// that go through ring 0 into prediction and filter arithmetic)
				const uint32_t need = (gprev << kProgShift) + min(t + 8u, Tprev) - VP8G_SKEW_EARLY(kSkQNeed);
				if (has_pred && !dead && !(VP8G_ABLATE & 8)) VP8G_SKEW_CENSUS(kSkQNeed, p_early >= need);
				if (has_pred && !dead && !(VP8G_ABLATE & 8) && p_early < need) wait_prog(pw, need);
				asm volatile("" ::: "memory");
				const uint32_t lcol = lane < 2 ? t + 1u : t;
				const bool ok = has_hbm && lane < 10 && lcol < C;
				mbx = __builtin_amdgcn_raw_buffer_load_b128(rQ, (int)(ok ? __umul24(lcol, (uint32_t)kCtxBytesPerCol) + 16u * (uint32_t)lane : kNoStore), 0, kCpolSc1);
			} else {
				mbx = __builtin_amdgcn_raw_buffer_load_b128(rQ, (int)kNoStore, 0, kCpolSc1);  // (a step issues it every time: the waits count it)
			}
			STAMP(10);

			// ---------------------------------------------- residual, both roles
			PRIO(0);
			uint32_t rs0[8], rs1[4];  // (chroma: this lane's two rows of the block)
			{
				const uint32_t fd0 = pick_dq(dq4a, seg), fa0 = __builtin_amdgcn_perm(fd0, fd0, 0x03020302u);
				const uint32_t fd1 = pick_dq(dq4b, seg), fa1 = __builtin_amdgcn_perm(fd1, fd1, 0x03020302u);
				uint32_t w0[8] = {pk_mul(cur.a0.x, fd0), pk_mul(cur.a0.y, fa0), pk_mul(cur.a0.z, fa0), pk_mul(cur.a0.w, fa0),
				                  pk_mul(cur.b0.x, fa0), pk_mul(cur.b0.y, fa0), pk_mul(cur.b0.z, fa0), pk_mul(cur.b0.w, fa0)};
				const uint32_t w1[8] = {pk_mul(cur.a1.x, fd1), pk_mul(cur.a1.y, fa1), pk_mul(cur.a1.z, fa1), pk_mul(cur.a1.w, fa1),
				                        pk_mul(cur.b1.x, fa1), pk_mul(cur.b1.y, fa1), pk_mul(cur.b1.z, fa1), pk_mul(cur.b1.w, fa1)};
				const bool anyac0 = ((w0[0] >> 16) | w0[1] | w0[2] | w0[3] | w0[4] | w0[5] | w0[6] | w0[7]) != 0u;
				const bool anyac1 = ((w1[0] >> 16) | w1[1] | w1[2] | w1[3] | w1[4] | w1[5] | w1[6] | w1[7]) != 0u;
				// Y2 (non-B_PRED): inverse WHT in role-1 lanes 10..13 (frame_kernel's 26..29) through the
				// quarter's residual park, which is written only after it
				if (__ballot(act && !bpred) != 0ull) {
					PRIO(10);
					uint8_t* const wh = hv + kResid;
					{
						const int hp = l & 1;
						const uint32_t q0 = hp ? w1[1] : w1[0], q1 = hp ? w1[3] : w1[2], q2 = hp ? w1[5] : w1[4], q3 = hp ? w1[7] : w1[6];
						const uint32_t a1 = pk_add(q0, q3), b1 = pk_add(q1, q2), c1 = pk_sub(q1, q2), d1 = pk_sub(q0, q3);
						if (l == 10 || l == 11) {
							uint8_t* const q = wh + 4 * hp;
							st32(q, pk_add(a1, b1));
							st32(q + 8, pk_add(c1, d1));
							st32(q + 16, pk_sub(a1, b1));
							st32(q + 24, pk_sub(d1, c1));
						}
					}
					wave_lds_sync();
					if (l >= 10 && l < 14) {
						uint8_t* const q = wh + 8 * (l - 10);
						const u32x2 tw = ld64(q);
						const int x0 = lo_s16(tw.x), x1 = hi_s16(tw.x), x2 = lo_s16(tw.y), x3 = hi_s16(tw.y);
						const int a1 = x0 + x3 + 3, b1 = x1 + x2, c1 = x1 - x2, d1 = x0 - x3 + 3;
						st64(q, u32x2{pack2((a1 + b1) >> 3, (c1 + d1) >> 3), pack2((a1 - b1) >> 3, (d1 - c1) >> 3)});
					}
					wave_lds_sync();
					if (!bpred) w0[0] = (w0[0] & 0xFFFF0000u) | *(const uint16_t*)(wh + 2 * l);
					PRIO(0);
				}
				STAMP(11);
				// inverse DCT of both blocks (frame_kernel's three wave-uniform forms, chosen per role)
				auto vpass = [&](uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, uint32_t* o) {
					const uint32_t a1 = pk_add(q0, q2), b1 = pk_sub(q0, q2);
					const uint32_t c1 = pk_sub(mul_s2(q1), mul_c2(q3)), d1 = pk_add(mul_c2(q1), mul_s2(q3));
					o[0] = pk_add(a1, d1);
					o[3] = pk_sub(a1, d1);
					o[1] = pk_add(b1, c1);
					o[2] = pk_sub(b1, c1);
				};
				auto idct = [&](const uint32_t* w, uint32_t* rs, uint64_t mac, uint64_t m23) {
					if (mac == 0ull) {
						const int d = (lo_s16(w[0]) + 4) >> 3;
#pragma unroll
						for (int i = 0; i < 8; i++) rs[i] = pack2(d, d);
					} else if (m23 == 0ull) {
						uint32_t oh[4];
						vpass(w[0], w[2], w[4], w[6], oh);
						int c1[4], d1[4];
#pragma unroll
						for (int rr = 0; rr < 4; rr++) {
							const int x1 = hi_s16(oh[rr]);
							c1[rr] = mul_s(x1), d1[rr] = mul_c(x1);
						}
#pragma unroll
						for (int rr = 0; rr < 4; rr++) {
							const int x0 = lo_s16(oh[rr]) + 4;
							rs[2 * rr] = pack2((x0 + d1[rr]) >> 3, (x0 + c1[rr]) >> 3);
							rs[2 * rr + 1] = pack2((x0 - c1[rr]) >> 3, (x0 - d1[rr]) >> 3);
						}
					} else {
						uint32_t o[8];
#pragma unroll
						for (int hp = 0; hp < 2; hp++) {
							uint32_t oh[4];
							vpass(w[hp], w[2 + hp], w[4 + hp], w[6 + hp], oh);
#pragma unroll
							for (int rr = 0; rr < 4; rr++) o[2 * rr + hp] = oh[rr];
						}
						int c1[4], d1[4];
#pragma unroll
						for (int rr = 0; rr < 4; rr++) {
							const int x1 = hi_s16(o[2 * rr]), x3 = hi_s16(o[2 * rr + 1]);
							c1[rr] = mul_s(x1) - mul_c(x3), d1[rr] = mul_c(x1) + mul_s(x3);
						}
#pragma unroll
						for (int rr = 0; rr < 4; rr++) {
							const int x0 = lo_s16(o[2 * rr]), x2 = lo_s16(o[2 * rr + 1]);
							const int a1 = x0 + x2 + 4, b1 = x0 - x2 + 4;
							rs[2 * rr] = pack2((a1 + d1[rr]) >> 3, (b1 + c1[rr]) >> 3);
							rs[2 * rr + 1] = pack2((b1 - c1[rr]) >> 3, (a1 - d1[rr]) >> 3);
						}
					}
				};
				idct(w0, rs0, __ballot(anyac0 && act), __ballot(act && (w0[1] | w0[3] | w0[5] | w0[7]) != 0u));
				// Chroma (role 1): blocks sit in lanes l < 8 only, the lanes l + 8 hold the Y2 / mode / side
				// roles, idle in the iDCT.  In the full form a block's work is split over the lane pair
				// (l, l + 8) -- DPP row_ror:8 exchanges within a quarter's 16-lane row: lane l + 8 takes the
				// block's column pair 1 in the vertical pass and rows 2..3 in the row pass.  Every form leaves
				// a lane its own two rows in rs1[0..3] (l: 0, 1; l + 8: 2, 3), as the chroma predictor wants them.
				const uint64_t mac1 = __ballot(anyac1 && l < 8 && act), m23_1 = __ballot(act && l < 8 && (w1[1] | w1[3] | w1[5] | w1[7]) != 0u);
				auto ror8 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x128, 0xF, 0xF, false); };
				if (mac1 != 0ull && m23_1 != 0ull) {
					const bool hi = (l & 8) != 0;
					uint32_t q[4], oh[4];
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const uint32_t odd = ror8(w1[2 * k + 1]);  // (lane l + 8: the block's column pair 1)
						q[k] = hi ? odd : w1[2 * k];
					}
					vpass(q[0], q[1], q[2], q[3], oh);
					const uint32_t r0 = ror8(hi ? oh[0] : oh[2]), r1 = ror8(hi ? oh[1] : oh[3]);
					// this lane's two rows (l: 0, 1; l + 8: 2, 3) as (columns 0-1, columns 2-3) words
					const uint32_t A[2] = {hi ? r0 : oh[0], hi ? r1 : oh[1]}, B[2] = {hi ? oh[2] : r0, hi ? oh[3] : r1};
					uint32_t rr2[4];
#pragma unroll
					for (int rr = 0; rr < 2; rr++) {
						const int x1 = hi_s16(A[rr]), x3 = hi_s16(B[rr]);
						const int c1 = mul_s(x1) - mul_c(x3), d1 = mul_c(x1) + mul_s(x3);
						const int x0 = lo_s16(A[rr]), x2 = lo_s16(B[rr]);
						const int a1 = x0 + x2 + 4, b1 = x0 - x2 + 4;
						rr2[2 * rr] = pack2((a1 + d1) >> 3, (b1 + c1) >> 3);
						rr2[2 * rr + 1] = pack2((b1 - c1) >> 3, (a1 - d1) >> 3);
					}
#pragma unroll
					for (int k = 0; k < 4; k++) rs1[k] = rr2[k];
				} else {
					// the other two forms, this lane's rows only
					const bool hi = (l & 8) != 0;  // (per arm on purpose: one shared definition changes the generated code)
					if (mac1 == 0ull) {  // DC only: the block's DC from lane l
						const uint32_t w0p = ror8(w1[0]);
						const int d = (lo_s16(hi ? w0p : w1[0]) + 4) >> 3;
#pragma unroll
						for (int k = 0; k < 4; k++) rs1[k] = pack2(d, d);
					} else {  // columns 2, 3 zero: lane l's vertical pass, rows 2, 3 of it to lane l + 8
						uint32_t oh[4];
						vpass(w1[0], w1[2], w1[4], w1[6], oh);
						const uint32_t r2 = ror8(oh[2]), r3 = ror8(oh[3]);
						const uint32_t A[2] = {hi ? r2 : oh[0], hi ? r3 : oh[1]};
#pragma unroll
						for (int rr = 0; rr < 2; rr++) {
							const int x1 = hi_s16(A[rr]);
							const int c1 = mul_s(x1), d1 = mul_c(x1);
							const int x0 = lo_s16(A[rr]) + 4;
							rs1[2 * rr] = pack2((x0 + d1) >> 3, (x0 + c1) >> 3);
							rs1[2 * rr + 1] = pack2((x0 - c1) >> 3, (x0 - d1) >> 3);
						}
					}
				}
				if (bpred) {  // the luma residual for the B_PRED pixel lanes
					uint8_t* rp = hv + kResid + l * 32;
					st128(rp, u32x4{rs0[0], rs0[1], rs0[2], rs0[3]});
					st128(rp + 16, u32x4{rs0[4], rs0[5], rs0[6], rs0[7]});
				}
			}
			// (issued right after the dequantisation instead, the iDCT's time earlier: ±0, r05p5)
			cur = qprefetch(lane, (int)t + 1);
			// Publish progress t (steps < t visible).  Only the prefetch just issued may be pending: this
			// step's context load and every store of step t - 1 are older, so they are acknowledged.
			asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kQPrefLoads) : "memory");
			if (lane == 0 && wave != VP8G_TEST_STALL_WAVE)
				__hip_atomic_store(prog + wave, (g << kProgShift) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			VP8G_SKEW_DELAY(kSkPubQStep, g, t);
			STAMP(0);

			// ---------------------------------------------- row above: ring 0 fill
			PRIO(1);
			if (has_hbm && t > 0 && lane < 10) {  // rec[t + 1] (lanes 0, 1) and lf[t] (2..9), loaded after this step's side info
				const uint32_t col = lane < 2 ? t + 1u : t;
				// (the slot chosen first and scaled by a 24-bit multiply: selecting between two scaled scalars
				// was folded into a select and a quarter-rate v_mul_lo_u32)
				const uint32_t s3o = __umul24(lane < 2 ? uni((t + 1u) % 3u) : uni(t % 3u), (uint32_t)kCtxBytesPerCol);
				if (col < C) st128(wq + kQRings + s3o + 16u * (uint32_t)lane, mbx);
			}
			wave_lds_sync();
			STAMP(1);

			// ---------------------------------------------- borders + loop-filter top strip
			PRIO_AFTER(2, 1);
			const u32x2 prole0 = ld64(smem + kRoleTab + 8 * l), prole1 = ld64(smem + kRoleTab + 8 * ((l & 7) + 16));
			if (act) {
				const bool top = r == 0;
				const uint8_t* const rec0 = rin + __umul24(m0, (uint32_t)kCtxBytesPerCol);
				const uint8_t* const rec1 = rin + __umul24(m1, (uint32_t)kCtxBytesPerCol);
				// (both roles' loads before either role's stores: the corner roles read the old above row,
				// which the above-row roles replace -- in frame_kernel they were lanes of one instruction)
				auto border = [&](int ln, uint32_t bt) -> uint32_t {
					const bool clampc = ln == 4 && cu + 1 == C;
					const uint8_t* const rb = (ln == 4 && !clampc) ? rec1 : rec0;
					const uint32_t ldv = ld32(rb + (clampc ? 12u : ((bt >> 12) & 0xFFu)));
					const uint32_t kind = (bt >> 20) & 3u;
					const uint32_t vabove = top ? 0x7F7F7F7Fu : (clampc ? __builtin_amdgcn_perm(ldv, ldv, 0x03030303u) : ldv);
					const uint32_t oldb = hv[(bt & 0xFFFu) + ((bt >> 12) & 0xFFu)];
					const uint32_t vcorner = c == 0 ? (top ? 0x7F000000u : 0x81000000u) : oldb << 24;
					return kind == 0 ? vabove : (kind == 1 ? 0x81818181u : vcorner);
				};
				const uint32_t v0 = border(l, bt0), v1 = border(l + 16, bt1);
				wave_lds_sync();
				if ((((bt0 >> 20) & 3u) != 1u || c == 0)) st32(hv + (bt0 & 0xFFFu), v0);
				if (l < 4 && (((bt1 >> 20) & 3u) != 1u || c == 0)) st32(hv + (bt1 & 0xFFFu), v1);
				if (lf_on && !top && l >= 4) {  // roles 20..31: the MB above's filter-state rows
					const bool ly = (bt1 >> 22) & 1u;
					const uint8_t* const lo = rec0 + ((bt1 >> 12) & 0xFFu);
					uint8_t* const td = hv + (bt1 & 0xFFFu) + (slot ? (ly ? 16u : 8u) : 0u);
					const u32x2 s0 = ld64(lo), s1 = ld64(lo + 8);
					if (ly) st64(td, s0), st64(td + 8, s1);
					else stc64(td, s0);
				}
			}
			wave_lds_sync();
			STAMP(2);

			// ---------------------------------------------- prediction + reconstruction
			PRIO(3);
			// luma (role 0: every lane a luma block): the mode's masks and constant from bits of the
			// mode (0 DC, 1 V, 2 H, 3 TM) instead of compares and selects
			if (act && !bpred) {
				const u32x2 prole = prole0;
				const uint8_t* ab = hv + (prole.x & 0x7FFu);
				const uint8_t* lc = hv + (prole.y & 0x7FFu);
				const int mode = ymode > 4 ? 0 : ymode;
				const u32x2 a01 = ld64(ab), a23 = ld64(ab + 8), l01 = ld64(lc), l23 = ld64(lc + 8);
				const uint32_t aw = ld32(hv + __builtin_amdgcn_ubfe(prole.x, 11u, 11u));
				const uint32_t lw = ld32(lc + 4u * __builtin_amdgcn_ubfe(prole.y, 22u, 2u));
				const int P = (int)ab[-1];
				const uint32_t sa4 = __builtin_amdgcn_sad_u8(a23.y, 0u, __builtin_amdgcn_sad_u8(a23.x, 0u, __builtin_amdgcn_sad_u8(a01.y, 0u, __builtin_amdgcn_sad_u8(a01.x, 0u, 0u))));
				const uint32_t sl4 = __builtin_amdgcn_sad_u8(l23.y, 0u, __builtin_amdgcn_sad_u8(l23.x, 0u, __builtin_amdgcn_sad_u8(l01.y, 0u, __builtin_amdgcn_sad_u8(l01.x, 0u, 0u))));
				const bool ha = r > 0, hl = c > 0;
				const uint32_t sum = (ha ? sa4 : 0u) + (hl ? sl4 : 0u);
				const int shift = 3 + (ha ? 1 : 0) + (hl ? 1 : 0);
				int dcv;
				asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(dcv) : "v"(128), "v"((int)((sum + (1u << (shift - 1))) >> shift)),
				    "s"(__builtin_amdgcn_ballot_w64(ha || hl)));
				const uint32_t mb = opq_u((uint32_t)mode);
				const uint32_t mA = (0u - ((0xAu >> mb) & 1u)) & 0x00FF00FFu;  // V, TM: the above row
				const uint32_t mL = (0u - ((0xCu >> mb) & 1u)) & 0x00FF00FFu;  // H, TM: the left column
				const int K = (int)((0u - (uint32_t)P) & (0u - ((0x8u >> mb) & 1u))) + (int)((uint32_t)dcv & (0u - (0x1u & ~mb & ~(mb >> 1))));
				const uint32_t K2 = __builtin_amdgcn_perm((uint32_t)K, (uint32_t)K, 0x05040100u);
				uint8_t* dst = hv + __builtin_amdgcn_ubfe(prole.y, 11u, 11u) + (slot ? 16u : 0u);
				const uint32_t A01 = pk_add(__builtin_amdgcn_perm(aw, aw, 0x0C010C00u) & mA, K2);
				const uint32_t A23 = pk_add(__builtin_amdgcn_perm(aw, aw, 0x0C030C02u) & mA, K2);
				uint32_t wv[4];
				auto pack_row = [&](uint32_t q01, uint32_t q23) -> uint32_t { return sat_pk(q01) | (sat_pk(q23) << 16); };
				if (__ballot(mode == 3) != 0ull) {
#pragma unroll
					for (int rr = 0; rr < 4; rr++) {
						const uint32_t L2 = __builtin_amdgcn_perm(lw, lw, 0x0C000C00u + 0x00010001u * rr) & mL;
						wv[rr] = pack_row(pk_add(pk_clamp255(pk_add(L2, A01)), rs0[2 * rr]), pk_add(pk_clamp255(pk_add(L2, A23)), rs0[2 * rr + 1]));
					}
				} else {
#pragma unroll
					for (int rr = 0; rr < 4; rr++) {
						const uint32_t L2 = __builtin_amdgcn_perm(lw, lw, 0x0C000C00u + 0x00010001u * rr) & mL;
						wv[rr] = pack_row(pk_add(pk_add(L2, A01), rs0[2 * rr]), pk_add(pk_add(L2, A23), rs0[2 * rr + 1]));
					}
				}
#pragma unroll
				for (int rr = 0; rr < 4; rr++) st32(dst + rr * kTP, wv[rr]);
				if ((prole.x >> 24) & 1u) {  // right column -> the next MB's left column
					const uint32_t c01 = __builtin_amdgcn_perm(wv[1], wv[0], 0x0C0C0703u);
					const uint32_t c23 = __builtin_amdgcn_perm(wv[3], wv[2], 0x0C0C0703u);
					st32(const_cast<uint8_t*>(lc) + 4u * __builtin_amdgcn_ubfe(prole.y, 22u, 2u), __builtin_amdgcn_perm(c23, c01, 0x05040100u));
				}
			}
			// chroma: the block of lane l & 7, rows 0, 1 in lane l < 8 and rows 2, 3 in lane l + 8 (the
			// residual rows are where the split iDCT leaves them)
			if (act) {
				const u32x2 prole = prole1;
				const uint8_t* ab = hv + (prole.x & 0x7FFu);
				const uint8_t* lc = hv + (prole.y & 0x7FFu);
				const int mode = uvmode > 3 ? 0 : uvmode;
				const u32x2 a01 = ld64(ab), l01 = ld64(lc);
				const uint32_t aw = ld32(hv + __builtin_amdgcn_ubfe(prole.x, 11u, 11u));
				const uint32_t lw = ld32(lc + 4u * __builtin_amdgcn_ubfe(prole.y, 22u, 2u));
				const int P = (int)ab[-1];
				const uint32_t sa2 = __builtin_amdgcn_sad_u8(a01.y, 0u, __builtin_amdgcn_sad_u8(a01.x, 0u, 0u));
				const uint32_t sl2 = __builtin_amdgcn_sad_u8(l01.y, 0u, __builtin_amdgcn_sad_u8(l01.x, 0u, 0u));
				const bool ha = r > 0, hl = c > 0;
				const uint32_t sum = (ha ? sa2 : 0u) + (hl ? sl2 : 0u);
				const int shift = 2 + (ha ? 1 : 0) + (hl ? 1 : 0);
				int dcv;
				asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(dcv) : "v"(128), "v"((int)((sum + (1u << (shift - 1))) >> shift)),
				    "s"(__builtin_amdgcn_ballot_w64(ha || hl)));
				const uint32_t mA = (mode == 1 || mode == 3) ? 0x00FF00FFu : 0u;
				const uint32_t mL = (mode == 2 || mode == 3) ? 0x00FF00FFu : 0u;
				const int K = (mode == 3 ? -P : 0) + (mode == 0 ? dcv : 0);
				const uint32_t K2 = __builtin_amdgcn_perm((uint32_t)K, (uint32_t)K, 0x05040100u);
				const uint32_t rb = (uint32_t)(l & 8) >> 2;  // first row of this lane: 0 or 2
				uint8_t* dst = hv + __builtin_amdgcn_ubfe(prole.y, 11u, 11u) + (slot ? 8u : 0u) + rb * kTP;
				const uint32_t A01 = pk_add(__builtin_amdgcn_perm(aw, aw, 0x0C010C00u) & mA, K2);
				const uint32_t A23 = pk_add(__builtin_amdgcn_perm(aw, aw, 0x0C030C02u) & mA, K2);
				const uint32_t lsel = 0x0C000C00u + 0x00010001u * rb;
				uint32_t wv[2];
				auto pack_row = [&](uint32_t q01, uint32_t q23) -> uint32_t { return sat_pk(q01) | (sat_pk(q23) << 16); };
				if (__ballot(mode == 3) != 0ull) {
#pragma unroll
					for (int k = 0; k < 2; k++) {
						const uint32_t L2 = __builtin_amdgcn_perm(lw, lw, lsel + 0x00010001u * k) & mL;
						wv[k] = pack_row(pk_add(pk_clamp255(pk_add(L2, A01)), rs1[2 * k]), pk_add(pk_clamp255(pk_add(L2, A23)), rs1[2 * k + 1]));
					}
				} else {
#pragma unroll
					for (int k = 0; k < 2; k++) {
						const uint32_t L2 = __builtin_amdgcn_perm(lw, lw, lsel + 0x00010001u * k) & mL;
						wv[k] = pack_row(pk_add(pk_add(L2, A01), rs1[2 * k]), pk_add(pk_add(L2, A23), rs1[2 * k + 1]));
					}
				}
				st32(dst, wv[0]);
				st32(dst + kTP, wv[1]);
				if ((prole.x >> 24) & 1u) {  // right column -> the next MB's left column (this lane's two bytes)
					const uint32_t c01 = __builtin_amdgcn_perm(wv[1], wv[0], 0x0C0C0703u);
					*(uint16_t*)(const_cast<uint8_t*>(lc) + 4u * __builtin_amdgcn_ubfe(prole.y, 22u, 2u) + rb) = (uint16_t)c01;
				}
			}
			wave_lds_sync();
			STAMP(12);
			const bool bp_lane = act && bpred;
			const uint64_t bpb = __ballot(bp_lane);
			if (bpb != 0ull && !(VP8G_ABLATE & 2)) {
				PRIO_AFTER(4, 3);
				// B_PRED wavefront (frame_kernel's): group g's sub-block at wavefront step s is
				// (i0 + g, s - 2 i0 - 2 g), pixel (rr, cc) = l.  Quarters with a B_PRED MB: bit h of qm.
				const uint32_t qm = (uint32_t)((bpb & 1ull) | ((bpb >> 15) & 2ull) | ((bpb >> 30) & 4ull) | ((bpb >> 45) & 8ull));
				const int rr = l >> 2, cc = l & 3;
				const bool col3 = cc == 3;
				const u32x4* const tabp = (const u32x4*)(smem + kBpTable) + l * (kBpEntry / 16);
				if (__builtin_popcount(qm) <= 2) {
					// At most two B_PRED MBs: one group per lane, as in frame_kernel -- quarters 0 / 1 of the wave
					// take groups 0 / 1 of the first such MB, quarters 2 / 3 those of the second -- so the
					// wavefront costs what it costs for two MBs, whatever quarters they sit in.
					const uint32_t qa = (uint32_t)__builtin_ctz(qm), qrest = qm & (qm - 1u);
					const uint32_t qb = qrest ? (uint32_t)__builtin_ctz(qrest) : qa;
					const uint32_t q = h < 2 ? qa : qb;
					const bool on = h < 2 || qrest != 0u;
					const int g = h & 1;
					uint8_t* const hq = wq + kHdrBytes + q * kQuarterBytes;
					uint8_t* const tYq = hq + kLfY;
					const uint8_t* const abq = hq + kAbY;
					uint8_t* const leftq = hq + kLeft;
					// (the target quarter's modes: every lane of a quarter holds them)
					const int bsrc = (int)(16u * q) * 4;
					const u32x4 bmq = u32x4{(uint32_t)__builtin_amdgcn_ds_bpermute(bsrc, (int)bmw.x), (uint32_t)__builtin_amdgcn_ds_bpermute(bsrc, (int)bmw.y),
					                        (uint32_t)__builtin_amdgcn_ds_bpermute(bsrc, (int)bmw.z), (uint32_t)__builtin_amdgcn_ds_bpermute(bsrc, (int)bmw.w)};
					uint8_t* const tpix = tYq + slot * 16 + 4 * kTP + kBS * g + kTP * rr + cc;
					const uint8_t* const tA = tYq + slot * 16 + 3 * kTP + kBS * g;
					const uint8_t* const aE = g ? tA : abq + 16;
					uint8_t* const lB = leftq + 36 * g;
					const int16_t* const rsp = (const int16_t*)(hq + kResid) + l + 32 * g;
					if (on) {
#pragma unroll
						for (int s = 0; s < 10; s++) {
							const int i0 = s <= 3 ? 0 : (s - 2) >> 1;
							const int j0 = s - 2 * i0;
							const bool v0 = j0 <= 3, v1 = i0 + 1 <= 3 && j0 >= 2;
							const bool valid = g ? v1 : v0;
							if (valid) {
								const int b0 = 4 * i0 + j0;
								const int mb0_ = v0 ? (int)((bmq[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu) : 0;
								const int mb1_ = v1 ? (int)((bmq[(b0 + 2) >> 2] >> (8 * ((b0 + 2) & 3))) & 0xFFu) : 0;
								const int mode = min(g ? mb1_ : mb0_, kBpModes - 1);
								const uint8_t* const arow = i0 == 0 ? aE + 4 * s : tA + kBS * i0 + 4 * s;
								const bool r3_0 = j0 == 3, r3_1 = j0 == 5;
								const uint8_t* const a47p = (r3_0 || r3_1) ? ((g ? r3_1 : r3_0) ? abq + 32 : arow + 4) : arow + 4;
								uint8_t* const lb = lB + 36 * i0 - 16 * s;
								const uint8_t* const pp = i0 == 0 ? (g ? lb - 1 : arow - 1) : lb - 1;
								const uint32_t a03 = ld32(arow), a47 = ld32(a47p), lw = ld32(lb);
								const uint32_t ey = ld32(pp - 3);  // E[4..7]: the corner on top of three bytes no tap weighs (make_bptab)
								const u32x4 tb = tabp[16 * (kBpEntry / 16) * mode];
								const int rv = rsp[16 * b0];
								const uint32_t lo = __builtin_amdgcn_perm(ey, lw, tb.x);
								const uint32_t hi = __builtin_amdgcn_perm(a47, a03, tb.x);
								const uint32_t x3 = (hi & tb.y) | (lo & ~tb.y);
								const int vdir = sat8(__builtin_amdgcn_sdot4((int)(x3 ^ 0x00808080u), (int)tb.z, (int)tb.w, false) >> 2);
								const int vdc = (int)((__builtin_amdgcn_sad_u8(a03, 0u, __builtin_amdgcn_sad_u8(lw, 0u, 4u))) >> 3);
								const int pred = mode == 0 ? vdc : vdir;
								const int px = sat8(pred + rv);
								tpix[kBS * i0 + 4 * s] = (uint8_t)px;
								const bool j3 = g ? j0 == 5 : j0 == 3;
								if (col3) (j3 ? leftq + 4 * (i0 + g) + rr : lb - 16 + rr)[0] = (uint8_t)px;
							}
							wave_lds_sync();
						}
					}
				} else if (bp_lane) {
					// three or four: both groups in every B_PRED quarter.  Sub-steps 0, 1, 8, 9 hold one sub-block
					// (group 0's): one pixel per lane, pixel (rr, cc) = l.  Sub-steps 2..7 hold two, and one
					// instruction stream serves both: lanes 0..7 take group 0's sub-block, lanes 8..15 group 1's,
					// each lane the pixel pair (r2, 2 c2), (r2, 2 c2 + 1) -- a sub-block's pixels depend on its
					// edges alone, so its edge loads, corner word, DC value and mode are a lane's once, and only
					// the table row, the perms and the dot product run per pixel.  The group-dependent offsets
					// are per-lane bases, computed here.  (ey: the dword that ends at the corner, as above.)
					static_assert(kBS % 8 == 0 && kBpEntry == 16, "the paired mapping's bases");
					const uint32_t g8 = (uint32_t)l & 8u, r2 = __builtin_amdgcn_ubfe((uint32_t)l, 1u, 2u), c2 = (uint32_t)l & 1u;  // l = 8 g + 2 r2 + c2
					const bool grp1 = g8 != 0u;
					const u32x4* const tabp2 = (const u32x4*)(smem + kBpTable + (((uint32_t)l & 7u) << 5));  // pixel 4 r2 + 2 c2
					const uint8_t* const tA2 = tY + slot * 16 + 3 * kTP + __umul24(g8, (uint32_t)(kBS / 8));
					const uint8_t* const aE2 = grp1 ? tA2 : abY + 16;
					uint8_t* const tpix2 = const_cast<uint8_t*>(tA2) + kTP + __umul24(r2, (uint32_t)kTP) + 2u * c2;
					uint8_t* const lB2 = left + (grp1 ? 36 : 0);
					uint8_t* const rc2 = lB2 + r2;               // right column -> the left column of sub-block column j + 1 ...
					uint8_t* const rc2m = rc2 + (grp1 ? 0 : 64);  // ... and, from group 0's column 3, the next MB's
					const int16_t* const rsp2 = (const int16_t*)(hv + kResid + (((uint32_t)l + g8) << 2));  // 16 (2 g) + 4 r2 + 2 c2
					const int16_t* const rsp = (const int16_t*)(hv + kResid) + l;
#pragma unroll
					for (int s = 0; s < 10; s++) {
						const int i0 = s <= 3 ? 0 : (s - 2) >> 1;
						const int j0 = s - 2 * i0;
						const bool vg1 = i0 + 1 <= 3 && j0 >= 2;  // (group 0 is valid in every sub-step, in column 3 when j0 == 3)
						const int b0 = 4 * i0 + j0;
						const bool r3 = j0 == 3;
						if (vg1) {
							const int b1 = b0 + 2;  // group 1's sub-block
							const uint32_t mraw = grp1 ? (bmw[b1 >> 2] >> (8 * (b1 & 3))) & 0xFFu : (bmw[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu;
							const int mode = min((int)mraw, kBpModes - 1);
							const uint8_t* const arow = i0 == 0 ? aE2 + 4 * s : tA2 + kBS * i0 + 4 * s;
							// (group 0 in column 3 takes the MB's above-right; in sub-block row 0 that is arow + 4 itself)
							const uint8_t* const a47p = r3 && i0 > 0 && !grp1 ? abY + 32 : arow + 4;
							const uint8_t* const lb = lB2 + 36 * i0 - 16 * s;
							const uint8_t* const pp = i0 == 0 && !grp1 ? arow - 1 : lb - 1;
							const uint32_t a03 = ld32(arow), a47 = ld32(a47p), lw = ld32(lb);
							const uint32_t ey = ld32(pp - 3);
							const u32x4* const tp = tabp2 + 16 * (kBpEntry / 16) * mode;
							const u32x4 tb0 = tp[0], tb1 = tp[kBpEntry / 16];
							const uint32_t rv2 = *(const uint32_t*)(rsp2 + 16 * b0);  // the pair's residuals: adjacent int16
							const int vdc = (int)((__builtin_amdgcn_sad_u8(a03, 0u, __builtin_amdgcn_sad_u8(lw, 0u, 4u))) >> 3);
							auto pixel = [&](const u32x4& tb, int rv) -> uint32_t {
								const uint32_t lo = __builtin_amdgcn_perm(ey, lw, tb.x);
								const uint32_t hi = __builtin_amdgcn_perm(a47, a03, tb.x);
								const uint32_t x3 = (hi & tb.y) | (lo & ~tb.y);
								const int vdir = sat8(__builtin_amdgcn_sdot4((int)(x3 ^ 0x00808080u), (int)tb.z, (int)tb.w, false) >> 2);
								return (uint32_t)sat8((mode == 0 ? vdc : vdir) + rv);
							};
							const uint32_t px0 = pixel(tb0, (int)(int16_t)rv2), px1 = pixel(tb1, (int)rv2 >> 16);
							*(uint16_t*)(tpix2 + kBS * i0 + 4 * s) = (uint16_t)(px0 | (px1 << 8));
							if (c2) (r3 ? rc2m : rc2)[36 * i0 - 16 * s - 16] = (uint8_t)px1;
						} else {
							const int md = min((int)((bmw[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu), kBpModes - 1);
							const uint8_t* const tA = tY + slot * 16 + 3 * kTP;
							const uint8_t* const arow = i0 == 0 ? abY + 16 + 4 * s : tA + kBS * i0 + 4 * s;
							const uint8_t* const a47p = r3 ? abY + 32 : arow + 4;
							uint8_t* const lb = left + 36 * i0 - 16 * s;
							const uint8_t* const pp = i0 == 0 ? arow - 1 : lb - 1;
							const uint32_t a03 = ld32(arow), a47 = ld32(a47p), lw = ld32(lb);
							const uint32_t ey = ld32(pp - 3);
							const u32x4 tb = tabp[16 * (kBpEntry / 16) * md];
							const int rv = rsp[16 * b0];
							const uint32_t lo = __builtin_amdgcn_perm(ey, lw, tb.x);
							const uint32_t hi = __builtin_amdgcn_perm(a47, a03, tb.x);
							const uint32_t x3 = (hi & tb.y) | (lo & ~tb.y);
							const int vdir = sat8(__builtin_amdgcn_sdot4((int)(x3 ^ 0x00808080u), (int)tb.z, (int)tb.w, false) >> 2);
							const int vdc = (int)((__builtin_amdgcn_sad_u8(a03, 0u, __builtin_amdgcn_sad_u8(lw, 0u, 4u))) >> 3);
							const int px = sat8((md == 0 ? vdc : vdir) + rv);
							(tY + slot * 16 + 4 * kTP + kTP * rr + cc)[kBS * i0 + 4 * s] = (uint8_t)px;
							if (col3) (r3 ? left + 4 * i0 + rr : lb - 16 + rr)[0] = (uint8_t)px;
						}
						wave_lds_sync();
					}
				}
			}
			wave_lds_sync();
			STAMP(3);
			// the MB's unfiltered bottom row (tile rows 19 / 11, before the loop filter) -> rec[c]: lanes
			// 0..3 = luma bytes 0..7, 8..15, U, V (ring h + 1; quarter 3: device memory, stored below)
			u32x2 recv;
			{
				const uint8_t* const src = l < 2 ? tY + 19 * kTP + slot * 16 + 8 * l : tC + (l == 3 ? kCV : 0) + 11 * kTP + slot * 8;
				recv = l < 2 ? ld64(src) : ldc64(src);
				if (act && l < 4 && h < 3) st64(rout + __umul24(m0, (uint32_t)kCtxBytesPerCol) + 8 * l, recv);
			}
			STAMP(4);

			// ---------------------------------------------- loop filter MB(r, c), both roles
			// (diagnostic VP8G_ABLATE & 64: the same filter run after the flush instead of before it --
			// output wrong, instruction stream the same: what overlapping the stores with the filter is worth)
#if VP8G_ABLATE & 64
			auto lf_phase = [&]() {
#endif
			PRIO(5);
			if (lf_on && !(VP8G_ABLATE & 1)) {
				const uint8_t* lp = smem + kLfTable + tabo + seg * 8 + (bpred ? 4 : 0);
				const int E = lp[0], I = lp[1], Tt = lp[2];
				const bool en = act && E != 0;
				if (__ballot(en) != 0ull) {
					const bool inner = hasc != 0 || bpred;
					const uint32_t sl16 = (t & 1u) << 4;
					LfLine L0, L1;
					L0.Mp = wq + __builtin_amdgcn_ubfe(lf_vp0, sl16, 16u);
					L0.Lp = L0.Mp + (slot ? -4 : 28);
					L0.colp = wq + __builtin_amdgcn_ubfe(lf_hp0, sl16, 16u);
					L1.Mp = wq + __builtin_amdgcn_ubfe(lf_vp1, sl16, 16u);
					L1.Lp = L1.Mp + (slot ? -4 : 12);
					L1.colp = wq + __builtin_amdgcn_ubfe(lf_hp1, sl16, 16u);
					if (simple) {
						lf_mb_luma<true>(L0, en, c > 0, r > 0, inner, E, I, Tt);  // (the simple filter leaves chroma alone)
					} else {
						// (round 5: both lines' gathers issued before one wait and the two filters interleaved:
						// ±0 / +0.5 %, r05q12 -- the loop filter is not latency-bound here)
						lf_mb_luma<false>(L0, en, c > 0, r > 0, inner, E, I, Tt);
						lf_mb_chroma(L1, en, c > 0, r > 0, inner, E, I, Tt);
					}
				}
			}
#if VP8G_ABLATE & 64
			};
#endif

			STAMP(5);
			// ---------------------------------------------- store final pixels and context
			PRIO(6);
			uint32_t oY0 = kNoStore, oY1 = kNoStore, oC0 = kNoStore, oC1 = kNoStore;
			u32x2 ya0 = u32x2{0u, 0u}, yb0 = ya0, ya1 = ya0, yb1 = ya0, cv0 = ya0, cv1 = ya0;
			uint32_t qY = kNoStore, qC = kNoStore;  // quarter 3: context rows -> device memory
			u32x2 qCv = ya0;
			// (frames without whole pieces: each piece's column and tile source, for the byte path below)
			const uint8_t *sy0 = tY, *sy1 = tY, *sc0 = tC, *sc1 = tC;
			uint32_t cY0 = cu, cY1 = cu, cC0 = cu, cC1 = cu;
			if (!lf_on) {
				// unfiltered: MB(r, c) is final once reconstructed; role 0 stores luma row l, role 1 chroma
				// row l & 7 of plane l >> 3
				const uint8_t* const srcY = tY + (4 + l) * kTP + slot * 16;
				ya0 = ld64(srcY), yb0 = ld64(srcY + 8);
				const int p = l >> 3, row = l & 7;
				cv1 = ldc64(tC + p * kCV + (4 + row) * kTP + slot * 8);
				sy0 = srcY, sc1 = tC + p * kCV + (4 + row) * kTP + slot * 8;
				const uint32_t prow = y0 + (uint32_t)l, prc = cy0 + (uint32_t)row;
				oY0 = act && prow < H ? __umul24(prow, sy) + cu * 16u : kNoStore;
				oC1 = act && prc < CH ? (p ? vofs : 0u) + __umul24(prc, suv) + cu * 8u : kNoStore;
			} else {
				const uint32_t sl16 = (t & 1u) << 4;
				auto role = [&](int ln, uint32_t fY, uint32_t fC, uint32_t lfo, uint32_t sYw, uint32_t sCw, uint32_t& oY, uint32_t& oC,
				                u32x2& ya, u32x2& yb, u32x2& cv, const uint8_t*& srcY, const uint8_t*& srcC) {
					const bool okc = act && (ln < 4 || c > 0);
					srcY = wq + __builtin_amdgcn_ubfe(sYw, sl16, 16u);
					ya = ld64(srcY), yb = ld64(srcY + 8);
					oY = okc ? fY + t * 16u : kNoStore;
					const int kr = ln < 12 ? ln : ln - 12;
					const bool okcc = act && (kr < 4 || c > 0);
					srcC = wq + __builtin_amdgcn_ubfe(sCw, sl16, 16u);
					cv = ldc64(srcC);
					oC = okcc ? fC + t * 8u : kNoStore;
					// the rows the next MB row still filters (lf[c - 1]): ring h + 1 (quarters 0..2)
					const uint32_t mmo = __umul24(mm, (uint32_t)kCtxBytesPerCol) + kCtxRecBytes;
					if (okc && lfo < 0x40000000u && h < 3) st128(rout + mmo + lfo, u32x4{ya.x, ya.y, yb.x, yb.y});
					if (okcc && (int)lfo > 0x3FFFFFFF && h < 3) stc64(rout + mmo + (lfo & 0xFFFFu), cv);
				};
				role(l, fY0, fC0, lfo0, sY0, sC0, oY0, oC0, ya0, yb0, cv0, sy0, sc0);
				role(l + 16, fY1, fC1, lfo1, sY1, sC1, oY1, oC1, ya1, yb1, cv1, sy1, sc1);
				// (a piece's column: this MB's for the top strip -- luma tile rows 0..3, chroma 0..3 of U
				// (l < 4) and of V (role 0's l >= 12) --, the left MB's for the rest)
				cY0 = cu - (l < 4 ? 0u : 1u), cC0 = cu - ((l < 4 || l >= 12) ? 0u : 1u);
				cY1 = cu - 1u, cC1 = cu - 1u;
				// quarter 3: luma context rows from role 1 (l < 4), chroma from role 0 (l 8..11) or role 1 (l 4..7)
				const uint32_t lc = __umul24(cu - 1u, (uint32_t)kCtxBytesPerCol) + kCtxRecBytes;  // (used only where c > 0)
				qY = h == 3 && act && c > 0 && lfo1 < 0x40000000u ? lc + lfo1 : kNoStore;
				const uint32_t lfoC = l >= 8 ? lfo0 : lfo1;
				qC = h == 3 && act && c > 0 && (int)lfoC > 0x3FFFFFFF ? lc + (lfoC & 0xFFFFu) : kNoStore;
				qCv = l >= 8 ? cv0 : cv1;
			}
			if (VP8G_ABLATE & 4) oY0 = oY1 = oC0 = oC1 = kNoStore;
			// Frames without whole pieces (frame-uniform branch): a piece cut by the right edge goes byte
			// by byte after the piece stores (which then drop it), as in frame_kernel.  Unaligned pieces
			// keep their vector stores: the device runs in the unaligned access mode that the compiler
			// itself assumes for gfx950 / HSA (a 1-byte-aligned 16-B store compiles to one
			// global_store_dwordx4), and every such frame is checked against the oracle by the tests.
			uint32_t nY0 = 0, nY1 = 0, nC0 = 0, nC1 = 0, bY0 = 0, bY1 = 0, bC0 = 0, bC1 = 0;
			if (!kWP && !wp) {
				auto cutY = [&](uint32_t& o, uint32_t col, uint32_t& n, uint32_t& b) {
					const uint32_t colpx = col * 16u;
					if (o >= 0x80000000u || colpx + 16u <= W) return;
					n = colpx < W ? min(W - colpx, 16u) : 0u, b = o, o = kNoStore;
				};
				auto cutC = [&](uint32_t& o, uint32_t col, uint32_t& n, uint32_t& b) {
					const uint32_t colpx = col * 8u;
					if (o >= 0x80000000u || colpx + 8u <= CW) return;
					n = colpx < CW ? min(CW - colpx, 8u) : 0u, b = o, o = kNoStore;
				};
				cutY(oY0, cY0, nY0, bY0), cutY(oY1, cY1, nY1, bY1);
				cutC(oC0, cC0, nC0, bC0), cutC(oC1, cC1, nC1, bC1);
			}
			{
				// The pixel stores, paired over two MB columns (luma: pair_swap above; chroma: the lane's own
				// two pieces).
				// piece columns and the last column a role stores itself (the last MB's rows below its top
				// strip go out with its own stores below)
				// (general instantiation: a last column cut by the right edge goes byte by byte, so the
				// column before it is the last one paired; pieces bound for the byte path carry kNoStore,
				// and every store built from such an offset drops out)
				const uint32_t cutY = kWP ? 0u : (W < 16u * C ? 1u : 0u), cutC = kWP ? 0u : (CW < 8u * C ? 1u : 0u);
				const uint32_t lastAy = C - 1u - cutY, lastAc = C - 1u - cutC;
				const uint32_t lastBy = lf_on ? C - 2u : lastAy, lastBc = lf_on ? C - 2u : lastAc;
				const uint32_t lY0 = lf_on && l >= 4 ? lastBy : lastAy, lC0 = lf_on && l >= 4 && l < 12 ? lastBc : lastAc, lC1 = lastBc;
				const bool isE = (lane0 & 1) == 0;
				auto swp = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false); };
				uint32_t sgl = 0;  // bit per piece: an even last column, stored alone
				const bool near_end = __ballot(act && cu + 2u >= C) != 0ull;  // (wave-uniform: most steps skip the test)
				// (held = the previous step's piece: at an odd column that is the even column's; luma: A stores
				// the even lane's row -- its kept piece, then the odd lane's current one --, B the odd lane's)
				// (bit selects, not branches: the column parity differs between the lanes of a role)
				auto single = [&](uint32_t o, uint32_t col, uint32_t lastc, uint32_t odd, uint32_t bit) {
					if (near_end) sgl |= (col == lastc ? ~odd & bit : 0u) & (o < kNoStore ? bit : 0u);
				};
				{  // role 0's luma row
					const u32x4 cur = u32x4{ya0.x, ya0.y, yb0.x, yb0.y};
					u32x4 dA, dB;
					pair_swap(hY0, cur, dA, dB);
					const uint32_t oP = swp(oY0), odd = 0u - (cY0 & 1u);
					const uint32_t e = isE ? oY0 - 16u : oP, f = isE ? oP - 16u : oY0;
					single(oY0, cY0, lY0, odd, 1u);
					hY0 = cur;
					qst128(rY, (e & odd) | (kNoStore & ~odd), dA);
					qst128(rY, (f & odd) | (kNoStore & ~odd), dB);
				}
				qst128(rY, oY1, u32x4{ya1.x, ya1.y, yb1.x, yb1.y});
				// both roles' chroma rows: the kept piece and the current one, from the lane that owns them
				auto own = [&](uint32_t o, uint32_t col, uint32_t lastc, const u32x2& cur, u32x2& held, uint32_t bit) {
					const uint32_t odd = 0u - (col & 1u);
					single(o, col, lastc, odd, bit);
					qst128(rC, ((o - 8u) & odd) | (kNoStore & ~odd), u32x4{held.x, held.y, cur.x, cur.y});
					held = cur;
				};
				own(oC0, cC0, lC0, cv0, hC0, 2u);
				own(oC1, cC1, lC1, cv1, hC1, 4u);
				if (near_end && __ballot(sgl != 0u) != 0ull) {  // (a quarter at its last column: rare)
					qst128(rY, (sgl & 1u) ? oY0 : kNoStore, u32x4{ya0.x, ya0.y, yb0.x, yb0.y});
					qst64(rC, (sgl & 2u) ? oC0 : kNoStore, cv0);
					qst64(rC, (sgl & 4u) ? oC1 : kNoStore, cv1);
				}
			}
			// quarter 3's context -> device memory (issued every step: the waits count them)
			__builtin_amdgcn_raw_buffer_store_b128(u32x4{ya1.x, ya1.y, yb1.x, yb1.y}, rQ, (int)qY, 0, kCpolSc1);
			__builtin_amdgcn_raw_buffer_store_b64(qCv, rQ, (int)qC, 0, kCpolSc1);
			__builtin_amdgcn_raw_buffer_store_b64(recv, rQ, (int)(h == 3 && act && l < 4 ? __umul24(cu, (uint32_t)kCtxBytesPerCol) + 8u * (uint32_t)l : kNoStore), 0, kCpolSc1);
			if (!kWP && !wp && __ballot((nY0 | nY1 | nC0 | nC1) != 0u) != 0ull) {
				for (uint32_t q = 0; q < nY0; q++) outY[bY0 + q] = sy0[q];
				for (uint32_t q = 0; q < nY1; q++) outY[bY1 + q] = sy1[q];
				for (uint32_t q = 0; q < nC0; q++) outU[bC0 + q] = sc0[q];
				for (uint32_t q = 0; q < nC1; q++) outU[bC1 + q] = sc1[q];
			}
			if (lf_on && __ballot(act && cu + 1 == C) != 0ull) {
				// last column: its own rows are final too (role 0: luma tile row 4 + l, chroma plane l >> 3
				// tile row 4 + (l & 7)); the bottom ones go to the context unless this is the last MB row
				const bool own = act && cu + 1 == C;
				const bool last_row = r + 1 == R;
				{
					const int trow = 4 + l;
					const uint8_t* const src = tY + trow * kTP + slot * 16;
					const u32x2 lo = ld64(src), hi = ld64(src + 8);
					const bool to_ctx = own && trow >= 16 && !last_row;
					const uint32_t eo = kCtxRecBytes + (uint32_t)(trow - 16) * 16u;
					if (to_ctx && h < 3) st128(rout + __umul24(m0, (uint32_t)kCtxBytesPerCol) + eo, u32x4{lo.x, lo.y, hi.x, hi.y});
					__builtin_amdgcn_raw_buffer_store_b128(u32x4{lo.x, lo.y, hi.x, hi.y}, rQ,
					                                       (int)(to_ctx && h == 3 ? __umul24(cu, (uint32_t)kCtxBytesPerCol) + eo : kNoStore), 0, kCpolSc1);
					const uint32_t prow = y0 + (uint32_t)trow - 4u, off = __umul24(prow, sy) + cu * 16u;
					const bool vis = own && !to_ctx && prow < H;
					const bool full = cu * 16u + 16u <= W;
					qst128(rY, vis && (kWP || full) ? off : kNoStore, u32x4{lo.x, lo.y, hi.x, hi.y});
					if (!kWP && !wp && vis && !full)
						for (uint32_t q = 0, n = min(W - cu * 16u, 16u); q < n; q++) outY[off + q] = src[q];
				}
				{
					const int p = l >> 3, trow = 4 + (l & 7);
					const uint8_t* const src = tC + p * kCV + trow * kTP + slot * 8;
					const u32x2 lo = ldc64(src);
					const bool to_ctx = own && trow >= 8 && !last_row;
					const uint32_t eo = kCtxRecBytes + 64u + (uint32_t)p * 32u + (uint32_t)(trow - 8) * 8u;
					if (to_ctx && h < 3) stc64(rout + __umul24(m0, (uint32_t)kCtxBytesPerCol) + eo, lo);
					__builtin_amdgcn_raw_buffer_store_b64(lo, rQ, (int)(to_ctx && h == 3 ? __umul24(cu, (uint32_t)kCtxBytesPerCol) + eo : kNoStore), 0, kCpolSc1);
					const uint32_t prow = cy0 + (uint32_t)trow - 4u, off = (p ? vofs : 0u) + __umul24(prow, suv) + cu * 8u;
					const bool vis = own && !to_ctx && prow < CH;
					const bool full = cu * 8u + 8u <= CW;
					qst64(rC, vis && (kWP || full) ? off : kNoStore, lo);
					if (!kWP && !wp && vis && !full)
						for (uint32_t q = 0, n = min(CW - cu * 8u, 8u); q < n; q++) outU[off + q] = src[q];
				}
			}
			wave_lds_sync();
#if VP8G_ABLATE & 64
			lf_phase();
#endif
			STAMP(6);

			// ---------------------------------------------- end of the step
			// (its progress was published after the prefetch, above: the step's stores are left in flight,
			// and the next step's publish waits for them)
			PRIO_AFTER(7, 6);
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			STAMP(7);
		}
		// end of the quad: every store acknowledged, then all T steps
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (lane0 == 0 && wave != VP8G_TEST_STALL_WAVE)
			__hip_atomic_store(prog + wave, (g << kProgShift) + T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (snap_out && lane0 == 0) __hip_atomic_store(gflags + fcur, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		VP8G_SKEW_DELAY_LONG(kSkPubQEnd, g, 0);
	}
#ifdef VP8G_STAMPS
	if (lane0 == 0)
		for (int i = 0; i < 14; i++)
			if (i != 8 && i != 9) atomicAdd(&g_vp8g_stamps[i], (unsigned long long)st_acc[i]);
	if (blockIdx.x < 512 && lane0 == 0) {
		uint32_t hw, xcc;
		asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
		asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
		g_vp8g_wave_info[2 * (blockIdx.x * 16 + wave)] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
		g_vp8g_wave_info[2 * (blockIdx.x * 16 + wave) + 1] = __builtin_amdgcn_s_memrealtime() - st_t0;
	}
#endif
}
