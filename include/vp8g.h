/*
 * vp8g.h -- C ABI of the MI355X-native VP8 keyframe reconstruction + loop-filter path.
 *
 * This header is the drop-in boundary.  The first half re-declares, layout-identically, the
 * reference decoder's types and the five entry points of its m06/m07 hot path, so the
 * reference's own callers (src/main.c:591, :665, :742, :811, :881; src/main_ultra.c:43)
 * link against libvp8g.so unchanged.  The second half is an additive batch API used by the
 * batch/multi-GPU driver and the benchmark (device-resident frames, one launch per batch).
 *
 * Plain C: no HIP or torch types appear in any signature.  Streams are passed as void*.
 */
#ifndef VP8G_H
#define VP8G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Reference types (layout-identical) ------------------------------------------------ */

/* reference: src/common/os.h:6-9 */
#ifndef VP8G_NO_BYTESPAN
typedef struct {
	const uint8_t* data;
	size_t size;
} ByteSpan;
#endif

/* reference: src/m02_vp8_header/vp8_header.h:7-18 (28 bytes; width @20, height @22) */
typedef struct {
	int is_key_frame;
	uint8_t profile;
	int show_frame;
	uint32_t first_partition_len;
	int start_code_ok;
	uint16_t width;
	uint16_t height;
	uint8_t x_scale;
	uint8_t y_scale;
} Vp8KeyFrameHeader;

/* reference: src/m05_tokens/vp8_tokens.h:7-50 (200 bytes) */
typedef struct {
	uint32_t mb_cols;
	uint32_t mb_rows;
	uint32_t mb_total;
	uint32_t part0_size_bytes;
	uint32_t part0_bytes_used;
	uint8_t part0_overread;
	uint32_t part0_overread_bytes;
	uint32_t token_part_size_bytes;
	uint32_t token_part_bytes_used;
	uint8_t token_overread;
	uint32_t token_overread_bytes;
	uint32_t token_overread_mb_index;
	uint32_t token_overread_plane;
	uint32_t token_overread_block_index;
	uint32_t token_overread_coeff_i;
	uint32_t token_overread_stage;
	uint32_t mb_skip_coeff;
	uint32_t mb_b_pred;
	uint32_t ymode_counts[5];
	uint32_t uv_mode_counts[4];
	uint32_t bmode_counts[10];
	uint32_t blocks_total_y2;
	uint32_t blocks_total_y;
	uint32_t blocks_total_u;
	uint32_t blocks_total_v;
	uint32_t blocks_nonzero_y2;
	uint32_t blocks_nonzero_y;
	uint32_t blocks_nonzero_u;
	uint32_t blocks_nonzero_v;
	uint32_t coeff_nonzero_total;
	uint32_t coeff_eob_tokens;
	uint32_t coeff_abs_max;
	uint64_t coeff_hash_fnv1a64;
} Vp8CoeffStats;

/* reference: src/m05_tokens/vp8_tokens.h:52-99 (320 bytes).  The hot path's input:
 * per-MB modes + dense int16 coefficients in natural (de-zigzagged) order. */
typedef struct {
	uint32_t mb_cols;
	uint32_t mb_rows;
	uint32_t mb_total;
	uint8_t q_index;
	int8_t y1_dc_delta_q;
	int8_t y2_dc_delta_q;
	int8_t y2_ac_delta_q;
	int8_t uv_dc_delta_q;
	int8_t uv_ac_delta_q;
	uint8_t segmentation_enabled;
	uint8_t segmentation_abs;
	int8_t seg_quant_idx[4];
	int8_t seg_lf_level[4];
	uint8_t lf_use_simple;
	uint8_t lf_level;
	uint8_t lf_sharpness;
	uint8_t lf_delta_enabled;
	int8_t lf_ref_delta[4];
	int8_t lf_mode_delta[4];
	uint8_t* segment_id; /* [mb_total] 0..3 */
	uint8_t* skip_coeff; /* [mb_total] */
	uint8_t* has_coeff;  /* [mb_total] (may be NULL: treated as all zero) */
	uint8_t* ymode;      /* [mb_total] 0..4 = DC,V,H,TM,B_PRED */
	uint8_t* uv_mode;    /* [mb_total] 0..3 */
	uint8_t* bmode;      /* [mb_total*16] 0..9 */
	int16_t* coeff_y2;   /* [mb_total*16] */
	int16_t* coeff_y;    /* [mb_total*256] */
	int16_t* coeff_u;    /* [mb_total*64] */
	int16_t* coeff_v;    /* [mb_total*64] */
	Vp8CoeffStats stats;
} Vp8DecodedFrame;

/* reference: src/m06_recon/vp8_recon.h:10-18 (40 bytes). Planes are malloc()ed host memory. */
typedef struct {
	uint32_t width;
	uint32_t height;
	uint32_t stride_y;
	uint32_t stride_uv;
	uint8_t* y;
	uint8_t* u;
	uint8_t* v;
} Yuv420Image;

/* ---- Reference entry points (exact signatures) ----------------------------------------- */

/* replaces src/m06_recon/vp8_recon.c:360 (decl vp8_recon.h:20).  Y zeroed, U/V = 128;
 * stride_y = width, stride_uv = (width+1)/2.  0 / -1 + errno (EINVAL, ENOMEM). */
int yuv420_alloc(Yuv420Image* img, uint32_t width, uint32_t height);

/* replaces src/m06_recon/vp8_recon.c:387 (decl vp8_recon.h:21).  Plain free() of the planes. */
void yuv420_free(Yuv420Image* img);

/* replaces src/m06_recon/vp8_recon.c:714 (decl vp8_recon.h:25): recon only (decoder -yuv). */
int vp8_reconstruct_keyframe_yuv(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* decoded, Yuv420Image* out);

/* replaces src/m06_recon/vp8_recon.c:718 (decl vp8_recon.h:28): recon + loop filter (-yuvf). */
int vp8_reconstruct_keyframe_yuv_filtered(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* decoded,
                                          Yuv420Image* out);

/* replaces src/m07_loopfilter/vp8_loopfilter.c:201 (decl vp8_loopfilter.h:14): in-place filter of a
 * macroblock-aligned frame (width == mb_cols*16, height == mb_rows*16, else EINVAL). */
int vp8_loopfilter_apply_keyframe(Yuv420Image* padded_img, const Vp8DecodedFrame* decoded);

/* ---- Batch API (build-only, additive) --------------------------------------------------- */

/* Per-frame launch descriptor (host computes it once per frame: geometry, output placement,
 * dequant factors per segment (RFC 6386 14.1, reference vp8_recon.c:57-76) and loop-filter
 * parameters per (segment, is_B_PRED) (reference vp8_loopfilter.c:166-199)). 176 bytes. */
typedef struct {
	uint32_t mb_cols, mb_rows;
	uint32_t width, height;       /* crop (visible) size written to the output */
	uint32_t stride_y, stride_uv; /* output strides in bytes */
	uint64_t mb_offset;           /* index of this frame's first MB in the batch SoA arrays */
	uint64_t out_y, out_u, out_v; /* byte offsets of the three planes in the output buffer */
	uint64_t src_y, src_u, src_v; /* (loop-filter-only mode) byte offsets of the padded input */
	uint32_t flags;               /* VP8G_F_* */
	uint32_t src_stride_y, src_stride_uv;
	uint32_t reserved;
	int16_t dq[4][6];  /* [segment][Y1dc, Y1ac, UVdc, UVac, Y2dc, Y2ac] */
	uint8_t lf[4][2][4]; /* [segment][is_bpred] = {level(E), interior I, hev T, 0}; level 0 = skip */
} Vp8gFrameDesc;

#define VP8G_F_LOOPFILTER 1u /* apply m07 (some MB has a non-zero level) */
#define VP8G_F_SIMPLE 2u     /* simple filter (luma only) instead of normal */
#define VP8G_F_LF_ONLY 4u    /* loop-filter-only: pixels come from src_* instead of recon */

/* Device pointers of a batch, concatenated over frames in the exact per-array layout of
 * Vp8DecodedFrame (so a frame uploads with nine plain memcpys).  MB index m of frame f is
 * desc.mb_offset + m. */
typedef struct {
	const int16_t* coeff_y;  /* [MB*256] */
	const int16_t* coeff_u;  /* [MB*64] */
	const int16_t* coeff_v;  /* [MB*64] */
	const int16_t* coeff_y2; /* [MB*16] */
	const uint8_t* ymode;    /* [MB] */
	const uint8_t* uv_mode;  /* [MB] */
	const uint8_t* segment_id; /* [MB] */
	const uint8_t* has_coeff;  /* [MB] */
	const uint8_t* bmode;      /* [MB*16] */
	const uint8_t* src;        /* LF-only mode input pixels (else NULL) */
	uint32_t* status;          /* device word: 0 ok, else VP8G_ERR_* (kernel-detected) */
} Vp8gBatchArrays;

#define VP8G_ERR_TIMEOUT 1u /* a wavefront dependency wait exceeded its bound */

/* Fill a descriptor for one frame.  kf may be NULL in LF-only mode.  Returns 0 / -1+errno. */
int vp8g_make_frame_desc(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* decoded, int filtered,
                         uint64_t mb_offset, uint64_t out_offset, Vp8gFrameDesc* out);

/* Bytes of cropped I420 output for a w x h frame (Y + 2 * ceil(w/2)*ceil(h/2)). */
uint64_t vp8g_i420_size(uint32_t width, uint32_t height);

/* Launch the fused recon(+LF) kernel over n frames on `hip_stream` (NULL = default stream).
 * h_descs: host copy (launch geometry); d_descs: the same array in device memory.
 * All pointers in `arrays` and d_out are device pointers.  Asynchronous; returns 0 or -1+errno.
 * `waves_per_frame` 0 = default. */
int vp8g_decode_batch_device(const Vp8gFrameDesc* h_descs, const Vp8gFrameDesc* d_descs, uint32_t n_frames,
                             const Vp8gBatchArrays* arrays, uint8_t* d_out, void* hip_stream,
                             uint32_t waves_per_frame);

/* Per-frame 64-bit digests of a device-resident batch's outputs (parity without copying pixels
 * back): d_digests[i] = digest of frame i's cropped I420 bytes (Y, U, V at stride = row width, the
 * file the reference CLI writes): D = L*K + sum_i mix(w_i + (i+1)*K) mod 2^64 over the bytes as
 * little-endian u64 words w_i (last one zero-padded), K = 0x9E3779B97F4A7C15, mix = splitmix64's
 * finaliser.  Descriptors must have the contiguous layout vp8g_make_frame_desc
 * builds (else EINVAL).  Asynchronous on `hip_stream`; 0 or -1 + errno. */
int vp8g_frame_digests(const Vp8gFrameDesc* h_descs, const Vp8gFrameDesc* d_descs, uint32_t n_frames,
                       const uint8_t* d_out, uint64_t* d_digests, void* hip_stream);

/* Host-side batch: upload n decoded frames, run one launch, download into n freshly
 * yuv420_alloc()ed images.  Returns 0 / -1+errno (EIO on a HIP failure). */
int vp8g_reconstruct_batch(const Vp8KeyFrameHeader* const* kfs, const Vp8DecodedFrame* const* frames, uint32_t n,
                           int filtered, Yuv420Image* outs);

/* ---- End-to-end batch path: .webp bytes -> I420 (SURVEY §8(f1) step 1 + §8(f2)) ---------- */

/* Packed m05 output, the host -> device wire format.  Per MB the 25 blocks (Y 0..15, U 0..3,
 * V 0..3, Y2) each leave a 16-bit mask of the natural positions holding a non-zero coefficient;
 * the values follow block by block, natural order within a block.  A 4K frame of the bench
 * fixtures packs to ~2.5-5 MB instead of the 26.6 MB of dense int16 arrays. */
#define VP8G_PK_BLOCKS 25
typedef struct {
	Vp8KeyFrameHeader kf;
	Vp8DecodedFrame f;  /* header fields, side arrays and stats; coeff_* are NULL */
	uint16_t* masks;    /* [mb_total * 25] */
	uint32_t* mb_off;   /* [mb_total] index of the MB's first value in values[] */
	int16_t* values;    /* [n_values] */
	uint64_t n_values;
} Vp8gPackedFrame;

/* Device m05 job of one frame: the host parses the frame header and the
 * first partition's frame-level fields (RFC 6386 9.2-9.11, 13.4); the device decodes the
 * per-macroblock modes (partition 0, from the saved bool-decoder state) and the coefficient
 * tokens (the token partitions) into the batch SoA of Vp8gBatchArrays.  1296 bytes. */
typedef struct {
	uint64_t data;       /* byte offset of the VP8 payload in the device bitstream buffer (caller) */
	uint64_t mb_offset;  /* first MB of the frame in the batch arrays (caller) */
	uint64_t b_value;    /* partition-0 bool decoder at the first MB header: value window, */
	int32_t b_bits;      /*   bits below the 8-bit comparison window, */
	uint32_t b_range;    /*   range (128..255), */
	uint32_t b_next;     /*   payload offset of the next byte to load */
	uint32_t p0_end;     /* payload offset one past the first partition (bytes beyond read as 0) */
	uint32_t tok_off, tok_end; /* the (first) token partition [tok_off, tok_end) of the payload */
	uint32_t mb_cols, mb_rows;
	uint8_t seg_enabled, seg_map_update, use_skip, skip_prob;
	uint8_t seg_probs[3], reserved;
	uint8_t coeff_probs[4][8][3][12]; /* RFC 13.4 after this frame's updates; rows padded to 12 */
	uint32_t nparts;                  /* token partitions (1, 2, 4, 8; > 1 only with VP8F_MULTI_PARTITION) */
	uint32_t part_off[8], part_end[8]; /* partition p = [part_off[p], part_end[p]) (RFC 9.5); MB row r
	                                      reads partition r % nparts */
	uint32_t reserved2[3];
} Vp8gTokFrame;

/* Decode n .webp file images end to end: container/header/m05 on `threads` host threads (0 = the
 * CPUs this process may run on) into the packed format, chunks of frames uploaded packed,
 * expanded and reconstructed (+ loop filter when `filtered`) on the device while the next chunk
 * is being entropy-decoded, I420 downloaded into outs[i] (yuv420_alloc layout; the caller frees
 * each with yuv420_free).  status[i] (may be NULL) = 0 or the errno of frame i's failure (its
 * image is left zeroed).  Returns 0 when every frame decoded, else -1 + errno of the first
 * failing frame (EIO for a device failure, in which case no image is returned). */
int vp8g_decode_webp_batch(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, Yuv420Image* outs,
                           int* status);

/* vp8g_decode_webp_batch with options.  VP8G_BATCH_DEVICE_M05: the host threads only parse the
 * container and the frame headers; the compressed payloads are uploaded and m05 runs on the
 * device (vp8g_m05_batch_device), one wavefront per frame.  Same outputs and errors. */
#define VP8G_BATCH_DEVICE_M05 1u
/* also accept multi-partition token streams (which the reference rejects, ENOTSUP), in either
 * mode; on the device each partition gets its own wave */
#define VP8G_BATCH_MULTI_PARTITION 2u
int vp8g_decode_webp_batch_ex(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                              Yuv420Image* outs, int* status);

/* The schedule vp8g_decode_webp_batch_ex uses for `flags` (host code only, no device call; for
 * tests and tools): dev[i] = 1 if frame i's m05 runs on the device, 0 on the host threads;
 * order[] = the order the worker threads take the frames (device frames first).  In device-m05
 * mode the k heaviest payloads go to the host threads, k minimising max(host time, device
 * time) under the library's cost model (VP8G_HYBRID=0 in the environment keeps
 * every frame on the device).  0, or -1 + EINVAL. */
int vp8g_plan_batch(const ByteSpan* files, uint32_t n, uint32_t threads, uint32_t flags, uint8_t* dev, uint32_t* order);

/* The recon launch the library would make for a batch of descriptors (host code only, no device call,
 * the environment is not read; for tests and tools): a device of `cus` compute units, the wave hint
 * of vp8g_decode_batch_device (0 = none), the six launch switches as values (what VP8G_SPLIT,
 * VP8G_WAVES, VP8G_CHAIN, VP8G_SPLITCHAIN, VP8G_CHAIN_IL and VP8G_ORDER would say: 0 / 0 / -1 / -1 /
 * -1 / 1 when unset), the caller (`policy`) and whether the launch gate finds the device free of the
 * library's other launches (may_cross).  The output base counts as 16-byte aligned.  0, or -1 + EINVAL. */
#define VP8G_PLAN_REFERENCE 0u /* the reference entry points and vp8g_reconstruct_batch ... */
#define VP8G_PLAN_PIPELINE 1u  /* ... or a chunk of the end-to-end batch path */
#define VP8G_PLAN_NO_SPLIT 2u  /* | vp8g_decode_batch_device (asynchronous); a chunk that is not its call's only one */
typedef struct {
	uint32_t quad;       /* 1: the quad chain kernel; 0: the frame kernel, one (or `parts`) workgroups per frame */
	uint32_t waves;      /* per workgroup */
	uint32_t global_ctx; /* frame kernel: the per-column context in device memory */
	uint32_t parts;      /* frame kernel: workgroups per frame */
	uint32_t workgroups; /* the grid */
	uint32_t ordered, mirror_split, interleave, whole; /* chain: cost-class placement; the modes; the lean instantiation */
	uint32_t ord_first;  /* frame kernel: cost-balanced placement over this many CUs (0 = batch order) */
	uint32_t lds_bytes;  /* dynamic LDS per workgroup */
	uint32_t mode;       /* VP8G_MODE_* as vp8g_last_launch_mode reports it */
	/* bytes the auxiliary buffers hold for either outcome of the gate: global context, mailboxes + progress
	 * words, the chain's snapshots, the mirror split's flags */
	uint64_t gctx_bytes, mbox_bytes, snap_bytes, flags_bytes;
} Vp8gLaunchPlan;
int vp8g_plan_launch(const Vp8gFrameDesc* descs, uint32_t n, uint32_t cus, uint32_t waves_hint, uint32_t split, uint32_t waves,
                     int32_t chain, int32_t splitchain, int32_t chain_il, int32_t order, uint32_t policy, int may_cross,
                     Vp8gLaunchPlan* out);

/* Device m05 over n frames on `hip_stream`: h_jobs / d_jobs host and device copies of the jobs
 * (data = payload offset in d_bits, 4-aligned, with >= 512 readable bytes after the payload;
 * mb_offset = first MB in the arrays).  Writes ymode, uv_mode, segment_id, has_coeff, bmode and
 * the non-zero coefficients of `arrays` (the caller zeroes the four coefficient arrays first);
 * arrays->status (required) gets VP8G_ERR_TIMEOUT if the two waves of a frame lose each other.
 * Asynchronous; 0 or -1 + errno (EINVAL for an inconsistent job, EIO on a launch failure). */
int vp8g_m05_batch_device(const Vp8gTokFrame* h_jobs, const Vp8gTokFrame* d_jobs, uint32_t n, const uint8_t* d_bits,
                          const Vp8gBatchArrays* arrays, void* hip_stream);

/* ---- m08 / m09 boundary: I420 -> RGB24 ("fancy" 4:2:0 upsampling) and the file writers -- */

/* replaces src/m08_yuv2rgb_ppm/yuv2rgb_ppm.c:123 (decl yuv2rgb_ppm.h:10): binary PPM (P6) of img
 * to fd, full-range Rec.601 as libwebp's VP8YuvToRgb.  0, or -1 + errno (EINVAL bad arguments or
 * zero size, ENOMEM, EIO on a HIP failure, or write(2)'s errno). */
int yuv420_write_ppm_fd(int fd, const Yuv420Image* img);

/* replaces src/m09_png/yuv2rgb_png.c:208 (decl yuv2rgb_png.h:10): 8-bit RGB PNG, filter 0 on every
 * scanline, one IDAT holding a zlib stream of stored blocks (<= 65535 bytes each); EFBIG when the
 * raw scanline stream exceeds 2^31 - 1 bytes.  Same errors as yuv420_write_ppm_fd otherwise. */
int yuv420_write_png_fd(int fd, const Yuv420Image* img);

#define VP8G_ENC_RGB 0u /* RGB24 rows, no header: w*h*3 bytes */
#define VP8G_ENC_PPM 1u /* the file yuv420_write_ppm_fd writes */
#define VP8G_ENC_PNG 2u /* the file yuv420_write_png_fd writes */
#define VP8G_ENC_SPAN 32768u /* output bytes per workgroup task */

/* Per-image descriptor of the encoder kernels (built by vp8g_make_enc_desc).  1432 bytes. */
typedef struct {
	uint32_t width, height;
	uint32_t stride_y, stride_uv;  /* source plane strides */
	uint64_t src_y, src_u, src_v;  /* byte offsets of the source planes in the source buffer */
	uint64_t out;                  /* byte offset of the file in the output buffer (16-B aligned) */
	uint64_t file_len;             /* bytes of the file */
	uint32_t format;               /* VP8G_ENC_* */
	uint32_t prefix_len;           /* bytes before the first pixel byte (PNG: signature, IHDR, IDAT
	                                  header, zlib header = 43) */
	uint32_t row_bytes;            /* bytes per row of the pixel stream (3w; PNG 1 + 3w) */
	uint32_t raw_len;              /* pixel stream bytes (height * row_bytes) */
	uint32_t span0, nspans;        /* this image's VP8G_ENC_SPAN-byte tasks in the launch */
	uint32_t zend;                 /* PNG: file offset just past the zlib stream (Adler-32 ends here) */
	uint32_t crc_init;             /* PNG: CRC-32 correction for the 0xFFFFFFFF initial value */
	uint8_t prefix[48];
	uint32_t reserved[4];
	uint32_t crc_ops[10][32];      /* PNG: GF(2) operators (columns) of the checksum combine */
} Vp8gEncDesc;

/* Fill the descriptor of one w x h image whose planes sit at src_* (strides stride_*) in the
 * source buffer, encoded as `format` at out_offset (16-B aligned) of the output buffer; its tasks
 * start at span0.  Returns the image's task count (> 0), or 0 + errno (EINVAL, EFBIG). */
uint32_t vp8g_make_enc_desc(uint32_t width, uint32_t height, uint32_t format, uint64_t src_y, uint64_t src_u,
                            uint64_t src_v, uint32_t stride_y, uint32_t stride_uv, uint64_t out_offset,
                            uint32_t span0, Vp8gEncDesc* out);

/* Encoded file size (0 for a bad format / size). */
uint64_t vp8g_encoded_size(uint32_t format, uint32_t width, uint32_t height);

/* Device workspace bytes for a launch of `total_spans` tasks. */
uint64_t vp8g_encode_workspace_size(uint32_t total_spans);

/* Encode n images (device-resident source planes -> files in d_out) on `hip_stream`: one launch
 * over all tasks (pixels, layout, per-task checksum partials) plus, when some image is a PNG, one
 * that finishes the Adler-32 / CRC-32 fields.  h_descs / d_descs: host and device copies of the
 * descriptors; d_work: vp8g_encode_workspace_size() bytes.  Asynchronous; 0 or -1 + errno. */
int vp8g_encode_batch_device(const Vp8gEncDesc* h_descs, const Vp8gEncDesc* d_descs, uint32_t n, const uint8_t* d_src,
                             uint8_t* d_out, uint8_t* d_work, void* hip_stream);

/* ---- Decode to a target size: crop + rescale of I420 on the device ----------------------- */

/* libwebp's `use_cropping` / `use_scaling` decoder options (dwebp -crop x y w h -scale w h), bit-exact
 * to libwebp 1.2.2's rescaler.  All-zero = identity.
 *   crop    (crop_left, crop_top, crop_w, crop_h), all 0 = the full picture; else w, h >= 1,
 *           left + w <= width, top + h <= height; left and top are rounded down to even for I420
 *           (libwebp keeps the window aligned with chroma) -- but NOT for an ARGB picture of a lossless
 *           file, whose window starts where it is given (vp8g_scale_argb_batch_device).
 *   scale   scaled_w x scaled_h; one of them 0 = derived from the other with a ceiling
 *           (h = (src_h * w + src_w - 1) / src_w over the cropped size); both 0 = crop only.
 * Without VP8G_SCALE_EXPAND, DOWNSCALE ONLY: scaled_w <= the (cropped) width and scaled_h <= the
 * (cropped) height, else EINVAL.  With it a target dimension may be anything up to 16383: a plane
 * that grows in x or in y takes libwebp's bilinear expand path in that axis (per plane and per
 * axis: 500 x 200 -> 224 x 224 shrinks x and expands y; 5 -> 6 expands luma while chroma 3 -> 3 is a
 * copy), bit-exact as well.
 * The output is I420: luma scaled to the target, each chroma plane independently from
 * ceil(window / 2) to ceil(target / 2).  RGB of a scaled picture has two definitions:
 *   this library's   the encoder (vp8g_encode_batch_device, fancy upsampling) run on that scaled I420;
 *                    vp8g_decode_webp_batch_tensor (below) is the on-device route to it, scaled I420 ->
 *                    RGB tensor with no host copy;
 *   libwebp's        `dwebp -ppm -scale`, WebPDecode with use_scaling into MODE_RGB / MODE_RGBA: chroma is
 *                    rescaled straight to luma resolution and the fancy upsampler is skipped.  That is
 *                    vp8g_make_scale_desc_444, vp8g_tensor_batch_device_444 and
 *                    vp8g_decode_webp_batch_tensor_rgb (below), bit-exact to libwebp. */
typedef struct {
	uint32_t crop_left, crop_top, crop_w, crop_h;
	uint32_t scaled_w, scaled_h;
	uint32_t flags; /* VP8G_SCALE_* */
} Vp8gScaleOpt;

/* A `filtered` request follows libwebp's rule per frame: when scaling, the loop filter is skipped
 * if scaled_w < width * 3 / 4 and scaled_h < height * 3 / 4 (integer products, the full picture
 * size), so the output equals `dwebp -yuv -scale`.  Without the flag, filtered means filtered. */
#define VP8G_SCALE_DWEBP_FILTER 1u
/* Allow a target larger than the (cropped) source in either dimension (libwebp's expand path).
 * Bit 2 and every bit above 4 are unknown: EINVAL. */
#define VP8G_SCALE_EXPAND 4u

/* One plane of a scale descriptor: W x H source window -> w x h, and how the launch tiles it (a
 * workgroup task = tile_w output columns x run_h output rows). 80 bytes.
 * A plane that expands (src_w < dst_w or src_h < dst_h) belongs to the expand kernel, marked by
 * group = 0; its fields then mean:
 *   fx, fy, fxy   libwebp's values for the plane's mode (vp8f_scale_factors; unused ones 0)
 *   src_h < dst_h:  tile_w = 64, 128 or 256 (the smallest that holds dst_w, else 256), pitch = 4 * tile_w
 *                   (bytes of one row of horizontal sums in LDS), block_rows = 32768 / pitch (rows the
 *                   LDS holds), run_h = block_rows - 1 (a run never needs more source rows than
 *                   run_h + 1)
 *   else:           tile_w = 256 (one output column per lane), run_h = max(1, 64 * dst_h / src_h),
 *                   pitch = block_rows = 0 (no LDS)
 *   tiles_x, ntasks as below. */
typedef struct {
	uint64_t src;                    /* byte offset of the window's first sample in the source buffer */
	uint64_t dst;                    /* byte offset of the plane in the output buffer */
	uint32_t src_stride, dst_stride;
	uint32_t src_w, src_h, dst_w, dst_h;
	uint32_t fx, fy, fxy;            /* 2^32 / w, 2^32 / h, h * 2^32 / (W * H) (0 if >= 2^32) */
	uint32_t group;                  /* lanes sharing one output column (power of two, <= 64); 0 = expanding plane */
	uint32_t tile_w, run_h;          /* output columns (256 / group) and output rows per task */
	uint32_t tiles_x, ntasks;        /* tasks per row of tiles; tasks of the plane */
	uint32_t pitch, block_rows;      /* LDS staging: bytes per source row segment, rows per block */
} Vp8gScalePlane;

/* Per-image descriptor of the scale kernel (built by vp8g_make_scale_desc).  272 bytes. */
typedef struct {
	uint32_t width, height;          /* output size */
	uint32_t task0, ntasks;          /* this image's workgroup tasks in the launch */
	uint32_t src_width, src_height;  /* the picture the options were resolved against */
	uint32_t crop_left, crop_top;    /* resolved (even) window origin */
	Vp8gScalePlane p[3];             /* Y, U, V */
} Vp8gScaleDesc;

/* The output size `opt` gives for a width x height picture.  0, or -1 + EINVAL (NULL argument,
 * bad crop, upscale in either dimension without VP8G_SCALE_EXPAND, a target beyond 16383 with it,
 * unknown flag bit, picture beyond 16383 x 16383). */
int vp8g_scaled_size(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint32_t* out_w, uint32_t* out_h);

/* Fill the descriptor of one width x height image whose planes sit at src_* (strides stride_*) in
 * the source buffer; the scaled I420 (Y, U, V back to back, strides = row widths) goes to
 * dst_offset of the output buffer, its tasks start at task0.  0, or -1 + EINVAL. */
int vp8g_make_scale_desc(uint32_t width, uint32_t height, uint64_t src_y, uint64_t src_u, uint64_t src_v,
                         uint32_t stride_y, uint32_t stride_uv, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                         uint32_t task0, Vp8gScaleDesc* out);

/* Scale n images of mixed sizes (device-resident source planes -> scaled I420 in d_dst) in one
 * launch on `hip_stream`, plus a second launch (the expand kernel) on the same stream when some
 * plane of the batch expands; each kernel leaves the other's tasks alone.  h_descs / d_descs: host and device copies of the descriptors (tasks
 * numbered image by image).  Writes only the images' own bytes.  Asynchronous; 0 or -1 + errno
 * (EINVAL for inconsistent descriptors, EIO on a launch failure).  d_dst may feed
 * vp8g_encode_batch_device on the same stream with no host copy in between. */
int vp8g_scale_batch_device(const Vp8gScaleDesc* h_descs, const Vp8gScaleDesc* d_descs, uint32_t n, const uint8_t* d_src,
                            uint8_t* d_dst, void* hip_stream);

/* Single image: upload src, scale on the device, download into *out (yuv420_alloc layout; the
 * caller frees it with yuv420_free).  0, or -1 + errno (EINVAL, ENOMEM, EIO). */
int yuv420_rescale(const Yuv420Image* src, const Vp8gScaleOpt* opt, Yuv420Image* out);

/* vp8g_decode_webp_batch_ex to a target size: each chunk is reconstructed as there, scaled on the
 * device into a second, small buffer, and only that is downloaded; outs[i] has the scaled size.
 * opts: n_opts = 1 (one option for every frame) or n (opts[i] for frame i).  `filtered` is applied
 * per frame (VP8G_SCALE_DWEBP_FILTER).  A frame whose options are invalid for its size gets
 * status[i] = EINVAL; the others still decode. */
int vp8g_decode_webp_batch_scaled(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                  const Vp8gScaleOpt* opts, uint32_t n_opts, Yuv420Image* outs, int* status);

/* ---- Decode into device-resident RGB tensors ------------------------------ */

/* One dense tensor for a batch of same-size pictures, left on the device in the form a model reads.
 *   RGB     exactly the bytes of VP8G_ENC_RGB (fancy 4:2:0 upsampling, libwebp's VP8YuvToRgb);
 *           VP8G_T_BGR swaps the channel order.
 *   dtype   VP8G_T_U8: those bytes (scale and bias ignored).  VP8G_T_F32: (float)u8 * scale[c] + bias[c],
 *           a round-to-nearest multiply and then a round-to-nearest add (never fused); c is the OUTPUT
 *           channel (with VP8G_T_BGR, scale[0] applies to B).  VP8G_T_F16 / VP8G_T_BF16: that float
 *           rounded once, to nearest-even.
 *   layout  VP8G_T_NHWC (pixel-interleaved) or VP8G_T_NCHW (three planes per picture).
 * Picture i of a batch starts at byte i * vp8g_tensor_slot_size() of the tensor; a slot start is in
 * general not 16-byte aligned (3 x 3 uint8: 27-byte slots), only the base must be element-aligned. */
#define VP8G_T_U8 0u
#define VP8G_T_F16 1u
#define VP8G_T_BF16 2u
#define VP8G_T_F32 3u
#define VP8G_T_NHWC 0u
#define VP8G_T_NCHW 1u
#define VP8G_T_BGR 1u /* flags */
typedef struct {
	uint32_t width, height;  /* of every picture of the tensor, 1 .. 16383 */
	uint32_t dtype;          /* VP8G_T_U8 / F16 / BF16 / F32 */
	uint32_t layout;         /* VP8G_T_NHWC / VP8G_T_NCHW */
	uint32_t flags;          /* VP8G_T_BGR */
	float scale[3], bias[3]; /* per output channel; finite (float dtypes) */
} Vp8gTensorOpt;

/* Per-image descriptor of the tensor kernel (built by vp8g_make_tensor_desc).  48 bytes. */
typedef struct {
	uint64_t src_y, src_u, src_v;  /* byte offsets of the source planes in the source buffer */
	uint64_t dst;                  /* byte offset of the picture's slot in the output buffer */
	uint32_t stride_y, stride_uv;  /* source plane strides */
	uint32_t task0, ntasks;        /* this image's workgroup tasks in the launch */
} Vp8gTensorDesc;

/* Bytes of one picture of the tensor: 3 * width * height * element size.  0 + EINVAL for a NULL or
 * invalid option (size 0 or beyond 16383, unknown dtype / layout / flag bit, non-finite scale or bias
 * with a float dtype). */
uint64_t vp8g_tensor_slot_size(const Vp8gTensorOpt* opt);

/* Fill the descriptor of one opt->width x opt->height I420 image whose planes sit at src_* (strides
 * stride_*) in the source buffer; its pixels go to dst_offset (a multiple of the element size; slot i
 * of a dense tensor = i * vp8g_tensor_slot_size()) of the output buffer, its tasks start at task0.
 * 0, or -1 + EINVAL. */
int vp8g_make_tensor_desc(const Vp8gTensorOpt* opt, uint64_t src_y, uint64_t src_u, uint64_t src_v, uint32_t stride_y,
                          uint32_t stride_uv, uint64_t dst_offset, uint32_t task0, Vp8gTensorDesc* out);

/* Convert n device-resident I420 images to their slots of d_dst in one launch on `hip_stream`.
 * h_descs / d_descs: host and device copies of the descriptors (tasks numbered image by image).
 * Writes only the images' own slot bytes.  Asynchronous; 0 or -1 + errno (EINVAL: NULL pointer,
 * invalid option, d_dst not aligned to the element size, inconsistent descriptors; EIO on a launch
 * failure).  d_src may be the output of vp8g_scale_batch_device or of the reconstruction on the same
 * stream, with no host copy in between. */
int vp8g_tensor_batch_device(const Vp8gTensorDesc* h_descs, const Vp8gTensorDesc* d_descs, uint32_t n,
                             const Vp8gTensorOpt* opt, const uint8_t* d_src, void* d_dst, void* hip_stream);

/* vp8g_decode_webp_batch_ex / _scaled with the tensor as the sink: each chunk is reconstructed,
 * scaled on the same stream when opts is given (n_opts = 1 or n; NULL / 0 = no scaling), and written
 * to slot i of d_out (device memory, n slots) by the tensor kernel; only the chunks' status words
 * come back to the host.  Returns after all device work is complete (the tensor is then usable from
 * any stream).  A frame whose decoded (or scaled) size is not t->width x t->height, or whose scale
 * options are invalid for it, gets status[i] = EINVAL; a frame that does not parse gets its errno;
 * the slot of every failed frame is filled with zero bytes and the others still decode.  -1 + EINVAL
 * for bad arguments (nothing is launched), -1 + EIO for a device failure. */
int vp8g_decode_webp_batch_tensor(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                  const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, void* d_out,
                                  int* status);

/* ---- Alpha of extended (VP8X) files --------------------------------------- */

/* The ALPH chunk entropy-decodes on the host (vp8f_alpha_decode, host/vp8_front.h) into a plane of
 * residuals; turning those into alpha is a prediction that runs on the device:
 *   alpha(x, y) = (pred + residual(x, y)) & 255, with pred = 0 at (0, 0), the left neighbour on the top
 *   row and the neighbour above in the left column for every filter != 0, and otherwise
 *   filter 1 left, 2 above, 3 clip255(left + above - aboveleft); filter 0: alpha = residual.
 * Per-plane descriptor (built by vp8g_make_alpha_desc).  48 bytes. */
typedef struct {
	uint64_t src;                    /* byte offset of the residual plane in the source buffer */
	uint64_t dst;                    /* byte offset of the alpha plane in the output buffer */
	uint32_t width, height;          /* 1 .. 16383 */
	uint32_t src_stride, dst_stride; /* >= width */
	uint32_t filter;                 /* 0 .. 3 */
	uint32_t task0, ntasks;          /* this plane's workgroup tasks in the launch (one per plane) */
	uint32_t reserved;
} Vp8gAlphaDesc;

/* 0, or -1 + EINVAL (NULL, a size of 0 or beyond 16383, filter > 3, a stride below the width). */
int vp8g_make_alpha_desc(uint32_t width, uint32_t height, uint32_t filter, uint64_t src, uint32_t src_stride, uint64_t dst,
                         uint32_t dst_stride, uint32_t task0, Vp8gAlphaDesc* out);

/* The hand-over between the gradient filter's bands, for the tests' model of its schedule (tests/bands.py): out[0] =
 * skewed columns per tile step, out[1] = tile steps a band trails the band above, out[2] = bytes of a wave's ring of
 * bottom-row results, out[3] = bytes of the full-width row between two rounds. */
void vp8g_alpha_handover(uint32_t out[4]);

/* Un-predict n planes of mixed sizes and filters in one launch on `hip_stream`.  h_descs / d_descs:
 * host and device copies of the descriptors (tasks numbered plane by plane).  Writes only each plane's
 * own width x height bytes.  Asynchronous; 0 or -1 + errno (EINVAL: NULL pointer, n = 0, an invalid or
 * inconsistent descriptor; EIO on a launch failure).  No workgroup waits on another and nothing
 * spins on memory: the kernel has no timeout path. */
int vp8g_alpha_unfilter_batch_device(const Vp8gAlphaDesc* h_descs, const Vp8gAlphaDesc* d_descs, uint32_t n,
                                     const uint8_t* d_src, uint8_t* d_dst, void* hip_stream);

/* vp8g_make_scale_desc for ONE plane scaled as luma -- the A plane: libwebp rescales it with the luma
 * arithmetic, the same window (origin snapped to even) and the same target.  p[0] is that plane (src:
 * its byte offset, stride >= width; output tight at dst_offset); p[1] and p[2] carry no tasks.
 * vp8g_scale_batch_device takes such descriptors beside three-plane ones.  0, or -1 + EINVAL. */
int vp8g_make_scale_desc_plane(uint32_t width, uint32_t height, uint64_t src, uint32_t stride, const Vp8gScaleOpt* opt,
                               uint64_t dst_offset, uint32_t task0, Vp8gScaleDesc* out);

/* The alpha plane of one image of the 4-channel tensor kernel: src_a = byte offset of the plane in
 * the source buffer (stride_a >= width), or VP8G_T_OPAQUE for a picture without alpha. */
typedef struct {
	uint64_t src_a;
	uint32_t stride_a;
	uint32_t reserved;
} Vp8gTensorAlpha;
#define VP8G_T_OPAQUE UINT64_MAX

/* vp8g_tensor_slot_size for the 4-channel tensor: 4 * width * height * element size. */
uint64_t vp8g_tensor_slot_size_a(const Vp8gTensorOpt* opt);

/* vp8g_tensor_batch_device with alpha as a fourth channel: [N,H,W,4] / [N,4,H,W], channels R,G,B,A
 * (B,G,R,A with VP8G_T_BGR); descriptors from vp8g_make_tensor_desc, whose dst offset is then the start
 * of the picture's 4-channel slot (slot i of a dense tensor = i * vp8g_tensor_slot_size_a()).  The
 * three colour channels are exactly those of the 3-channel kernel (scale and bias have three
 * entries and never touch A).  A for VP8G_T_U8 is the alpha byte; for VP8G_T_F32 the float nearest to
 * a / 255 (an IEEE division: 255 -> 1.0f exactly); for F16 / BF16 that float rounded once to
 * nearest-even.  Not premultiplied.  h_alpha / d_alpha: host and device copies of the n alpha entries
 * (stride_a >= width unless opaque, else EINVAL). */
int vp8g_tensor_batch_device_a(const Vp8gTensorDesc* h_descs, const Vp8gTensorDesc* d_descs, const Vp8gTensorAlpha* h_alpha,
                               const Vp8gTensorAlpha* d_alpha, uint32_t n, const Vp8gTensorOpt* opt, const uint8_t* d_src,
                               void* d_dst, void* hip_stream);

/* vp8g_decode_webp_batch_ex / _scaled (opts NULL, n_opts 0: no scaling) with the extended container in
 * front: simple files as before, VP8X files too (ICC / EXIF / XMP and unknown chunks skipped); alpha is
 * ignored, as `dwebp -yuv` ignores it.  A file the extended parser refuses gets its errno in status[i]
 * (ENOTSUP: animation, a lossless main image). */
int vp8g_decode_webp_batch_x(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                             const Vp8gScaleOpt* opts, uint32_t n_opts, Yuv420Image* outs, int* status);

/* vp8g_decode_webp_batch_tensor with the extended container in front.  xflags (other bits EINVAL):
 *   0              the 3-channel tensor, alpha ignored;
 *   VP8G_X_ALPHA   the 4-channel tensor (n slots of vp8g_tensor_slot_size_a bytes, as vp8g_tensor_batch_device_a
 *                  writes them).  A worker thread entropy-decodes a frame's ALPH chunk (vp8f_alpha_decode, in
 *                  both m05 modes); the residual plane is uploaded into the chunk buffer, un-predicted, cropped /
 *                  rescaled with the frame's opts as luma, and read by the tensor kernel, all on the chunk's
 *                  stream.  A frame without alpha gets opaque A.  A frame whose ALPH does not decode gets
 *                  status[i] = EINVAL and a zero slot, as libwebp fails the whole picture; the others still
 *                  decode.  VP8G_SCALE_DWEBP_FILTER and the loop filter do not concern A.  Alpha planes count
 *                  against the chunk memory budget; vp8g_plan_batch does not price ALPH bytes. */
#define VP8G_X_ALPHA 1u
int vp8g_decode_webp_batch_tensor_x(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                    const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                    void* d_out, int* status);

/* ---- Lossless (VP8L) images ----------------------------------------------- */

/* A VP8L stream entropy-decodes on the host (vp8f_lossless_decode, host/vp8_front.h) into an ARGB
 * residual image and a list of up to four transforms; inverting those runs on the device.  One
 * transform of an image, as the stream spells it (RFC 9649 4): */
#define VP8G_L_PREDICTOR 0u
#define VP8G_L_CROSS_COLOR 1u
#define VP8G_L_SUBTRACT_GREEN 2u
#define VP8G_L_COLOR_INDEX 3u
typedef struct {
	uint64_t data;    /* byte offset in the source buffer of the sub-image (predictor, cross colour: div_up(xsize, bits) x
	                   * div_up(height, bits) dwords) or of the colour table (ncolors dwords, prefix-summed); any alignment */
	uint32_t type;    /* VP8G_L_* */
	uint32_t bits;    /* predictor, cross colour: 2 .. 9; colour index: 3 / 2 / 1 / 0 for up to 2 / 4 / 16 / 256 colours */
	uint32_t xsize;   /* the image's width when the transform was read */
	uint32_t ncolors; /* colour index: 1 .. 256 */
} Vp8gLosslessTransform;

/* Per-image descriptor (built by vp8g_make_lossless_desc).  128 bytes. */
typedef struct {
	uint64_t src;            /* byte offset of the residual image in the source buffer (any alignment): tight dwords,
	                          * height rows of the last transform's input width (the packed width after colour indexing) */
	uint64_t dst;            /* byte offset (a multiple of 4) of the tight width x height 0xAARRGGBB output */
	uint32_t width, height;  /* 1 .. 16383 */
	uint32_t ntransforms;    /* 0 .. 4, in stream order; inverted last to first */
	uint32_t task0;          /* this image's workgroup task in the launch (one per image) */
	Vp8gLosslessTransform tr[4];
} Vp8gLosslessDesc;

/* 0, or -1 + EINVAL: NULL, a size of 0 or beyond 16383, more than four transforms, a type twice, bits
 * or ncolors out of range, an xsize that is not the width the stream would have at that point, dst
 * not a multiple of 4. */
int vp8g_make_lossless_desc(uint32_t width, uint32_t height, uint64_t src, uint64_t dst, uint32_t ntransforms,
                            const Vp8gLosslessTransform* tr, uint32_t task0, Vp8gLosslessDesc* out);

/* The kernel's geometry, for tests that aim at its boundaries: out[0] = columns per barrier group (the tile step),
 * out[1] = rows per wave (a band), out[2] = bands per workgroup round. */
void vp8g_lossless_geometry(uint32_t out[3]);

/* The hand-over between the predictor's bands, for the tests' model of its schedule (tests/bands.py): out[0] = columns a
 * row trails the row above, out[1] = groups a band trails the band above, out[2] = a wave's ring of bottom-row pixels,
 * out[3] = pixels of the full-width row between two rounds that a launch may ask for at most. */
void vp8g_lossless_handover(uint32_t out[4]);

/* Invert the transforms of n images of mixed sizes and transform lists in one launch on `hip_stream`.
 * One 16-wave workgroup per image; the predictor runs as a skewed wavefront (a row per lane, each row
 * two columns behind the row above), paced by workgroup barriers only: no workgroup waits on another,
 * nothing spins on memory, there is no timeout path.  Writes only each image's own width x height
 * dwords (which also serve as its working buffer).  Asynchronous; 0 or -1 + errno (EINVAL: NULL pointer,
 * n = 0, d_dst not dword-aligned, an invalid or inconsistent descriptor -- checked before any launch;
 * EIO on a launch failure). */
int vp8g_lossless_batch_device(const Vp8gLosslessDesc* h_descs, const Vp8gLosslessDesc* d_descs, uint32_t n,
                               const uint8_t* d_src, uint8_t* d_dst, void* hip_stream);

/* One image of the ARGB tensor kernel: src = byte offset (a multiple of 4) of tight width x height
 * 0xAARRGGBB dwords, as vp8g_lossless_batch_device leaves them; dst = byte offset of the picture's slot. */
typedef struct {
	uint64_t src, dst;
	uint32_t task0, ntasks;
} Vp8gTensorArgbDesc;

/* channels = 3 or 4.  0, or -1 + EINVAL. */
int vp8g_make_tensor_argb_desc(const Vp8gTensorOpt* opt, uint32_t channels, uint64_t src, uint64_t dst_offset, uint32_t task0,
                               Vp8gTensorArgbDesc* out);

/* vp8g_tensor_batch_device / _a for ARGB sources: channels = 3 writes slots of vp8g_tensor_slot_size
 * bytes (alpha dropped, as `dwebp -ppm` drops it), channels = 4 slots of vp8g_tensor_slot_size_a bytes.
 * R, G, B: the arithmetic of vp8g_tensor_batch_device; A: that of vp8g_tensor_batch_device_a. */
int vp8g_tensor_batch_device_argb(const Vp8gTensorArgbDesc* h_descs, const Vp8gTensorArgbDesc* d_descs, uint32_t n,
                                  const Vp8gTensorOpt* opt, uint32_t channels, const uint8_t* d_src, void* d_dst,
                                  void* hip_stream);

/* ---- Crop + rescale of ARGB pictures (lossless files), exact to libwebp ---- */

/* libwebp applies a Vp8gScaleOpt to a lossless picture as follows, and so does this: the window is taken as
 * given (NO even rounding of its origin; see Vp8gScaleOpt); its pixels are alpha-premultiplied; each of the
 * four byte channels is rescaled exactly as a luma plane of vp8g_scale_batch_device (shrinking and, with
 * VP8G_SCALE_EXPAND, expanding, per axis); the output pixels are un-premultiplied.  A crop without a target size
 * copies the window's pixels untouched.  VP8G_SCALE_DWEBP_FILTER means nothing here and is ignored.
 * Per-picture descriptor (built by vp8g_make_scale_argb_desc).  1200 bytes. */
typedef struct {
	uint64_t src;                        /* byte offset (a multiple of 4) of the tight src_width x src_height 0xAARRGGBB picture */
	uint64_t work;                       /* byte offset (a multiple of 16) of this picture's planes in the work buffer */
	uint64_t dst;                        /* byte offset (a multiple of 4) of the tight width x height 0xAARRGGBB output */
	uint64_t work_bytes;                 /* bytes at `work`: four window planes, then four scaled planes (0: crop only) */
	uint32_t width, height;              /* output size */
	uint32_t src_width, src_height;      /* the picture the options were resolved against */
	uint32_t crop_left, crop_top, win_w, win_h;  /* the resolved window, origin as given */
	uint32_t plane_stride, out_stride;   /* bytes per row of a window plane / a scaled plane: win_w / width rounded up to 16 */
	uint32_t nplanes, plane0;            /* 4, or 0 for a crop without a target size; this picture's first plane descriptor in the launch */
	uint32_t split_task0, split_ntasks;  /* this picture's workgroup tasks in the split launch, ... */
	uint32_t scale_task0, scale_ntasks;  /* ... in the rescaler's (the sum over its planes), ... */
	uint32_t merge_task0, merge_ntasks;  /* ... and in the merge launch */
	uint32_t reserved[2];
	Vp8gScaleDesc plane[4];              /* B, G, R, A as vp8g_make_scale_desc_plane makes them: work buffer -> work buffer */
} Vp8gScaleArgbDesc;

/* Bytes of the work buffer one picture's planes need (a multiple of 16; 0 for a crop without a target size), or
 * 0 + EINVAL for options that do not fit the picture (as vp8g_scaled_size). */
uint64_t vp8g_scale_argb_work_size(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt);

/* Bytes at the START of the work buffer that a launch of n pictures keeps for itself (the rescaler's plane
 * descriptors); every picture's work_offset lies at or beyond it. */
uint64_t vp8g_scale_argb_head_size(uint32_t n);

/* Fill the descriptor of one width x height ARGB picture at `src` of the source buffer; its planes go to work_offset
 * of the work buffer (vp8g_scale_argb_work_size bytes), the scaled picture to dst_offset of the output buffer.  The
 * four counters are the launch's running totals before this picture: planes (out->nplanes each), split tasks, rescaler
 * tasks, merge tasks (out->*_ntasks each).  0, or -1 + EINVAL (NULL, options that do not fit, a misaligned offset). */
int vp8g_make_scale_argb_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t work_offset,
                              uint64_t dst_offset, uint32_t plane0, uint32_t split_task0, uint32_t scale_task0,
                              uint32_t merge_task0, Vp8gScaleArgbDesc* out);

/* Crop + rescale n device-resident ARGB pictures of mixed sizes and options on `hip_stream`: the split launch, the
 * rescaler's one or two launches (vp8g_scale_batch_device over the planes), the merge launch.  h_descs / d_descs: host
 * and device copies of the descriptors.  d_src and d_dst dword-aligned, d_work 16-byte aligned.  Reads only the
 * windows' pixels; writes only the pictures' own output dwords, their work regions and the head of d_work.
 * Asynchronous; 0 or -1 + errno.  The host copies are checked before anything is launched -- EINVAL: NULL or
 * misaligned pointer, n = 0, a descriptor that is not what vp8g_make_scale_argb_desc gives (a window outside the
 * picture, ...), counters that do not number the pictures in order, a work region inside the head or overlapping
 * another's; ENOMEM.  EIO on a launch failure.  d_dst may feed vp8g_tensor_batch_device_argb on the same stream with
 * no host copy in between, and d_src may be the output of vp8g_lossless_batch_device. */
int vp8g_scale_argb_batch_device(const Vp8gScaleArgbDesc* h_descs, const Vp8gScaleArgbDesc* d_descs, uint32_t n,
                                 const uint8_t* d_src, uint8_t* d_work, uint8_t* d_dst, void* hip_stream);

/* vp8g_decode_webp_batch_tensor_x, which with VP8G_X_LOSSLESS also decodes lossless files (a simple
 * 'VP8L' file, or VP8X + 'VP8L'): lossy and lossless files may share a batch and a tensor.  A worker
 * thread entropy-decodes a lossless frame (vp8f_lossless_decode); its residual image and transform data
 * are uploaded into the chunk buffer and go through vp8g_lossless_batch_device and
 * vp8g_tensor_batch_device_argb on the chunk's stream (3 channels without VP8G_X_ALPHA, 4 with).
 * Without VP8G_X_LOSSLESS_SCALE a lossless frame is not scaled: one whose resolved scale option is not the
 * identity gets status[i] = ENOTSUP and a zero slot.  A size mismatch with the tensor or a stream that does not
 * decode is EINVAL.  Without VP8G_X_LOSSLESS: vp8g_decode_webp_batch_tensor_x.  Other xflags bits: EINVAL.
 * The lossless buffers count against the chunk memory budget; vp8g_plan_batch does not price them.
 *   VP8G_X_LOSSLESS_SCALE (needs VP8G_X_LOSSLESS, else EINVAL)  a lossless frame's option is applied as libwebp
 *                  applies it to such a file (vp8g_scale_argb_batch_device above: the window's origin as given,
 *                  bit-exact RGBA): the transform kernel's picture goes through vp8g_scale_argb_batch_device and
 *                  then the tensor kernel on the chunk's stream; a frame whose option is the identity goes as
 *                  without the flag.  An option that does not fit the frame, or whose result is not the tensor's
 *                  size, is EINVAL.  The planes and the scaled picture count against the chunk memory budget.
 *                  Lossy frames of the batch are scaled as ever (their window's origin rounded down to even). */
#define VP8G_X_LOSSLESS 2u
#define VP8G_X_LOSSLESS_SCALE 16u
int vp8g_decode_webp_batch_tensor_any(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                      const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                      void* d_out, int* status);

/* ---- Scaled RGB exact to libwebp's (dwebp -ppm -scale) -------------------- */

/* libwebp asked for a scaled RGB picture of a lossy file rescales Y, U and V EACH straight to the target size and
 * converts pixel by pixel (VP8YuvToRgb); no upsampler runs.  An option with a target size (scaled_w or scaled_h not 0,
 * a target equal to the window included) resolves as for I420 (window origin snapped down to even, a derived dimension
 * by the ceiling, VP8G_SCALE_EXPAND deciding only whether the target may exceed the LUMA window), and then
 *   Y     window win_w x win_h -> w x h;
 *   U, V  origin (left / 2, top / 2), ceil(win_w / 2) x ceil(win_h / 2) -> the same w x h; each axis shrinks or expands
 *         as its own sizes say (128 -> 100 shrinks luma and expands chroma 64 -> 100);
 *   A     as luma (vp8g_make_scale_desc_plane); the A byte is not premultiplied (MODE_RGBA, not MODE_rgbA).
 * With VP8G_SCALE_DWEBP_FILTER and a filtered request the result is libwebp's.
 *
 * vp8g_make_scale_desc for that: the three planes w x h each, back to back at dst_offset, stride w.  0, or -1 + EINVAL
 * as vp8g_make_scale_desc, and for an option WITHOUT a target size (libwebp then runs the fancy upsampler on the window:
 * the I420 route).  vp8g_scale_batch_device takes such descriptors beside the others. */
int vp8g_make_scale_desc_444(uint32_t width, uint32_t height, uint64_t src_y, uint64_t src_u, uint64_t src_v,
                             uint32_t stride_y, uint32_t stride_uv, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                             uint32_t task0, Vp8gScaleDesc* out);

/* vp8g_make_tensor_desc for three planes of opt->width x opt->height each: stride_uv is the stride of the (full-width)
 * U and V planes, >= opt->width.  The planes may start at any byte. */
int vp8g_make_tensor_desc_444(const Vp8gTensorOpt* opt, uint64_t src_y, uint64_t src_u, uint64_t src_v, uint32_t stride_y,
                              uint32_t stride_uv, uint64_t dst_offset, uint32_t task0, Vp8gTensorDesc* out);

/* vp8g_tensor_batch_device / _a for such planes: pixel = VP8YuvToRgb(Y, U, V) of its own three samples; the element
 * for a colour byte, the layouts, VP8G_T_BGR and alpha are exactly those of the 4:2:0 kernel.  channels = 3: h_alpha and
 * d_alpha NULL, slots of vp8g_tensor_slot_size; channels = 4: both given, slots of vp8g_tensor_slot_size_a.  Anything
 * else, a stride below the width, tasks out of order or a slot off the element size: -1 + EINVAL.  Writes only the
 * images' own slot bytes; no LDS, no barrier, no wait on another workgroup.  Asynchronous. */
int vp8g_tensor_batch_device_444(const Vp8gTensorDesc* h_descs, const Vp8gTensorDesc* d_descs, const Vp8gTensorAlpha* h_alpha,
                                 const Vp8gTensorAlpha* d_alpha, uint32_t n, const Vp8gTensorOpt* opt, uint32_t channels,
                                 const uint8_t* d_src, void* d_dst, void* hip_stream);

/* Single image: upload src, the three planes to the target size, the 4:4:4 tensor kernel, download: *rgb = out_w * out_h
 * tight R, G, B triples (malloc; the caller frees it) -- libwebp's MODE_RGB bytes, the payload of `dwebp -ppm -scale`.
 * 0, or -1 + errno (EINVAL, also for an option without a target size; ENOMEM; EIO). */
int yuv420_rescale_rgb(const Yuv420Image* src, const Vp8gScaleOpt* opt, uint8_t** rgb, uint32_t* out_w, uint32_t* out_h);

/* vp8g_decode_webp_batch_tensor_any (same arguments, same xflags) with one difference: a lossy frame whose option has a
 * target size gets libwebp's RGB as above (vp8g_make_scale_desc_444, then vp8g_tensor_batch_device_444 on the chunk's
 * stream; the intermediate is 3 * w * h bytes of the chunk buffer).  Frames without a target size (no option, crop only)
 * take the 4:2:0 route, which is what libwebp computes for them; lossless frames take their ARGB route; statuses, zero
 * slots of failed frames and the size check against the tensor are those of _any. */
int vp8g_decode_webp_batch_tensor_rgb(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                      const Vp8gScaleOpt* opts, uint32_t n_opts, const Vp8gTensorOpt* t, uint32_t xflags,
                                      void* d_out, int* status);

/* ---- Crop + shrink of ARGB pictures straight into a tensor: the fused route ---- */

/* What vp8g_scale_argb_batch_device followed by vp8g_tensor_batch_device_argb computes, in ONE launch and without a work
 * buffer, for the pictures that expand in neither axis (win_w >= width and win_h >= height, equality included): each
 * window pixel is read once, premultiplied into LDS, the four byte channels are rescaled together, and the result is
 * un-premultiplied, converted (R, G, B: scale and bias; A: a / 255) and stored as elements of the picture's slot.
 * Per-picture descriptor (built by vp8g_make_scale_argb_tensor_desc).  96 bytes. */
typedef struct {
	uint64_t src;                    /* byte offset (a multiple of 4) of the tight src_width x src_height 0xAARRGGBB picture */
	uint64_t dst;                    /* byte offset (a multiple of the element size) of the picture's slot in the output */
	uint32_t width, height;          /* output size: the slot is channels x width x height elements */
	uint32_t src_width, src_height;  /* the picture the options were resolved against */
	uint32_t crop_left, crop_top, win_w, win_h;  /* the resolved window, origin as given */
	uint32_t fx, fy, fxy;            /* as Vp8gScalePlane */
	uint32_t group;                  /* lanes sharing one output column (power of two, <= 64) */
	uint32_t tile_w, run_h;          /* output columns (256 / group) and output rows per task */
	uint32_t tiles_x;                /* tasks per row of tiles */
	uint32_t pitch, block_rows;      /* LDS staging: bytes per source row segment (a multiple of 16), rows per block */
	uint32_t task0, ntasks;          /* this picture's workgroup tasks in the launch */
	uint32_t reserved;
} Vp8gScaleArgbTensorDesc;

/* The fused kernel's geometry, for tests that aim at its boundaries: out[0] = pixels per 16-byte load, out[1] = pixels of
 * the longest row segment a task can stage (a picture whose tiles need more is not this kernel's), out[2] = source rows
 * per run (about: a task takes max(1, out[2] * height / win_h) output rows). */
void vp8g_scale_argb_fused_geometry(uint32_t out[3]);

/* Fill the descriptor of one width x height ARGB picture at `src` of the source buffer, scaled by `opt` (resolved as
 * vp8g_make_scale_argb_desc resolves it: the window's origin as given, VP8G_SCALE_DWEBP_FILTER ignored) into the slot at
 * dst_offset of the output; its tasks start at task0.  0, or -1 + errno: EINVAL as vp8g_make_scale_argb_desc (NULL,
 * options that do not fit the picture, src not a multiple of 4); ENOTSUP for valid options that are not the fused
 * kernel's -- an axis that expands, a crop without a target size (a plain copy), a tile whose row segment is longer than
 * vp8g_scale_argb_fused_geometry's out[1] (only where win_w exceeds 2046 x width) -- which is how a caller chooses between
 * this route and the planar one. */
int vp8g_make_scale_argb_tensor_desc(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, uint64_t dst_offset,
                                     uint32_t task0, Vp8gScaleArgbTensorDesc* out);

/* Crop + shrink n device-resident ARGB pictures of mixed sizes, windows and targets into their slots of d_dst in one
 * launch on `hip_stream`.  opt gives the element type, layout, channel order, scale and bias (its width and height are
 * not read: every picture has its output size in its descriptor); channels = 3 (alpha dropped after the un-premultiply,
 * as MODE_RGB drops it) or 4.  Every element is the one vp8g_tensor_batch_device_argb writes for the picture
 * vp8g_scale_argb_batch_device makes.  h_descs / d_descs: host and device copies of the descriptors (d_descs 8-byte
 * aligned).  Reads only the windows' pixels and writes only the pictures' own slots.  No workgroup waits on another,
 * nothing spins on memory.  Asynchronous; 0 or -1 + errno.  The host copies are checked before anything is launched --
 * EINVAL: NULL or misaligned pointer (d_src to 4 bytes, d_dst to the element size), n = 0, channels, an invalid option,
 * a descriptor that is not byte for byte what vp8g_make_scale_argb_tensor_desc gives, tasks that do not number the
 * pictures in order, a dst offset off the element size, slots that overlap; ENOMEM.  EIO on a launch failure.  d_src may
 * be the uint8 / NHWC / BGR 4-channel tensor of vp8g_anim_compose_batch_device or the output of
 * vp8g_lossless_batch_device, on the same stream with no host copy between. */
int vp8g_scale_argb_tensor_batch_device(const Vp8gScaleArgbTensorDesc* h_descs, const Vp8gScaleArgbTensorDesc* d_descs, uint32_t n,
                                        const Vp8gTensorOpt* opt, uint32_t channels, const uint8_t* d_src, void* d_dst,
                                        void* hip_stream);

/* ---- Animated files (ANIM / ANMF), composited on the device --------------- */

/* An animation is a list of frames, each a rectangle of the canvas with a blend and a disposal rule; what is
 * shown for frame k -- canvas k -- is what libwebp's WebPAnimDecoder (MODE_RGBA) composes (the rules:
 * vp8f_anim_compose, host/vp8_front.h).  Frames depend on each other, pixels do not: a thread of the compositor
 * keeps a few pixels of the canvas in registers and walks the frame list, reading each frame's pixels once and
 * writing every canvas's elements once, already in the tensor's dtype and layout; the canvas never touches memory.
 * A key frame starts from an empty canvas, so the frames from one key frame to the next -- a segment -- are
 * composed independently of the others.
 * One frame (vp8g_make_anim_desc completes it).  40 bytes. */
#define VP8G_ANIM_BLEND 1u     /* alpha-blend over the canvas (else overwrite) */
#define VP8G_ANIM_DISPOSE 2u   /* the rectangle is cleared to transparent after the frame */
#define VP8G_ANIM_HAS_ALPHA 4u /* the frame's bitstream carries alpha (key-frame rule only) */
#define VP8G_ANIM_KEY 8u       /* set by vp8g_make_anim_desc */
typedef struct {
	uint64_t src;                 /* byte offset (a multiple of 4) in the source buffer of the frame's tight width x height
	                               * 0xAARRGGBB dwords, not premultiplied */
	uint32_t x, y, width, height; /* its rectangle on the canvas; x and y even */
	uint32_t flags;               /* VP8G_ANIM_* */
	uint32_t seg_first, seg_end;  /* in record s of an animation: segment s is frames [seg_first, seg_end) (s < nsegs) */
	uint32_t reserved;
} Vp8gAnimFrame;

/* Per-animation descriptor (built by vp8g_make_anim_desc).  48 bytes. */
typedef struct {
	uint64_t frames;                /* byte offset (a multiple of 8) in the source buffer of the device copy of the records */
	const Vp8gAnimFrame* h_frames;  /* their host copy, which the entry point checks before it launches (the kernel never
	                                 * reads this field); it must stay valid until vp8g_anim_compose_batch_device returns */
	uint64_t dst;                   /* byte offset of canvas 0 in the output buffer; canvas k follows k canvas sizes later */
	uint32_t width, height;         /* the canvas, 1 .. 16383 */
	uint32_t nframes, nsegs;
	uint32_t task0, ntasks;         /* this animation's workgroup tasks in the launch: nsegs x tiles of the canvas */
} Vp8gAnimDesc;

/* The kernel's geometry, for tests that aim at its boundaries: out[0] = adjacent pixels of a canvas row per thread,
 * out[1] = pixels per task (a tile: 256 threads' pixels in row-major order), out[2] = the most frames a task walks
 * (0: no limit -- the records are read through the scalar cache as the walk reaches them, not staged). */
void vp8g_anim_geometry(uint32_t out[3]);

/* Complete the nframes records of one animation (in: src, the rectangle, BLEND / DISPOSE / HAS_ALPHA; out: VP8G_ANIM_KEY
 * by libwebp's rule and the segment table) and fill its descriptor: records at frames_offset of the source buffer,
 * canvas k at dst_offset + k * channels * width * height * element size, tasks from task0.  0, or -1 + EINVAL: NULL,
 * no frames, a canvas or rectangle of 0 or beyond 16383, a rectangle outside the canvas, an odd x or y, an unknown flag
 * bit (VP8G_ANIM_KEY included), src not a multiple of 4, frames_offset not a multiple of 8, more than 2^31 tasks. */
int vp8g_make_anim_desc(uint32_t width, uint32_t height, Vp8gAnimFrame* frames, uint32_t nframes, uint64_t frames_offset,
                        uint64_t dst_offset, uint32_t task0, Vp8gAnimDesc* out);

/* Compose n animations of mixed canvas sizes and frame counts in one launch on `hip_stream`.  opt gives the element
 * type, layout, channel order, scale and bias (its width and height are not read: every animation has its canvas size
 * in its descriptor); channels = 3 (alpha dropped after compositing) or 4.  R, G, B and A of every element are those
 * vp8g_tensor_batch_device_argb writes for the composed canvas.  For animations of one canvas size, canvas k of
 * animation i lands in slot first[i] + k of a dense [N, ...] tensor when dst = first[i] * the slot size.
 * h_descs / d_descs: host and device copies of the descriptors (tasks numbered animation by animation, a task per
 * segment and tile).  No workgroup waits on another, nothing spins on memory, there is no timeout path.  Writes only
 * the animations' own canvases.  Asynchronous; 0 or -1 + errno.  The host copies are checked before anything is
 * launched -- EINVAL: NULL pointer, n = 0, channels, an invalid option, d_src not 8-byte aligned, d_dst or a dst
 * offset off the element size, a descriptor or record that is not what vp8g_make_anim_desc gives (a rectangle
 * outside the canvas, an odd offset, a key flag or segment table that does not follow the rule, ...), task counters
 * that do not number the animations in order, canvases that are not laid out in order without overlap.  EIO on a
 * launch failure.  d_src may be the output of vp8g_lossless_batch_device, or the uint8 / NHWC / BGR 4-channel tensor
 * of vp8g_tensor_batch_device_a / _argb (whose bytes are these dwords), on the same stream with no host copy between. */
int vp8g_anim_compose_batch_device(const Vp8gAnimDesc* h_descs, const Vp8gAnimDesc* d_descs, uint32_t n,
                                   const Vp8gTensorOpt* opt, uint32_t channels, const uint8_t* d_src, void* d_dst,
                                   void* hip_stream);

/* Canvas size, frame count and loop count (0 = forever) of n files, so that a caller can size the tensor: a file
 * that webp_parse_anim refuses (a still picture included) has nframes[i] = 0 and status[i] = EINVAL.  Any output
 * array but nframes may be NULL.  0, or -1 + errno (EINVAL: NULL arguments, n = 0; else the first refused file's). */
int vp8g_anim_info(const ByteSpan* files, uint32_t n, uint32_t* canvas_w, uint32_t* canvas_h, uint32_t* nframes,
                   uint32_t* loop_count, int* status);

/* Decode n animated files into a dense tensor of canvases: file i owns the nframes[i] slots (of vp8g_tensor_slot_size
 * bytes for channels = 3, vp8g_tensor_slot_size_a for 4) from slot first[i] = nframes[0] + ... + nframes[i - 1] on, in
 * frame order; d_out holds the sum of all nframes slots.  Every frame's payload is wrapped in memory as a file of its
 * own ('VP8 ' alone, VP8X + ALPH + 'VP8 ', or 'VP8L') and decoded by vp8g_decode_webp_batch_tensor_any (filtered, threads
 * and flags as there; VP8G_X_ALPHA | VP8G_X_LOSSLESS) into a uint8 / NHWC / BGR 4-channel staging tensor, one call per
 * distinct frame size; then one launch of vp8g_anim_compose_batch_device composes every file.  Nothing is scaled here
 * (vp8g_decode_webp_anim_tensor_scaled below decodes to a target size).
 * timestamps (may be NULL; one per slot): the cumulative end time of each frame in ms, as WebPAnimDecoderGetNext
 * returns it.  status[i]: 0; EINVAL for a file that is no animation (no slots), whose canvas is not t->width x
 * t->height, or one of whose frames does not decode (its errno) -- all slots of such a file are zero bytes and the
 * other files still decode.  Returns after all device work is complete.  0, or -1 + errno: the first failed file's;
 * EINVAL for bad arguments (nothing is launched); ENOMEM; EIO for a device failure (every status EIO). */
int vp8g_decode_webp_anim_tensor(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                 const Vp8gTensorOpt* t, uint32_t channels, void* d_out, uint32_t* timestamps, int* status);

/* vp8g_decode_webp_anim_tensor to a target size.  Scaled canvas k of a file is canvas k exactly as
 * above (the frames are never scaled before compositing: blending does not commute with rescaling), cropped and rescaled
 * as libwebp crops and rescales an RGBA picture that has alpha (vp8g_scale_argb_batch_device: the window's origin as
 * given, premultiply, the plane rescaler per byte channel, un-premultiply; a crop without a target size copies pixels
 * untouched; a target equal to the window is NOT the identity on translucent pixels; VP8G_SCALE_EXPAND for a larger
 * target; VP8G_SCALE_DWEBP_FILTER ignored); with 3 channels alpha is dropped after the un-premultiply.
 * opts: n_opts = 0 (the identity), 1 (one option for every file) or n; file i's option is resolved against its own canvas
 * and must give t->width x t->height, so canvases of different sizes may share one tensor.  An option that does not fit the
 * canvas, or whose result is not the tensor's size, is status[i] = EINVAL.  Slots, timestamps, the zero slots and errno of
 * a failed file, and the return value are those of vp8g_decode_webp_anim_tensor.
 * The frames decode as there.  A file whose option is the identity on a canvas of the tensor's size is composed straight
 * into d_out.  The others are composed at full size into a device staging buffer (uint8 / NHWC / BGR / 4 channels: the
 * ARGB dwords) and rescaled from there into d_out: by vp8g_scale_argb_tensor_batch_device, or -- the options its maker
 * answers ENOTSUP for -- by vp8g_scale_argb_batch_device and vp8g_tensor_batch_device_argb.  The canvases are staged in
 * groups of whole animations in file order: a group's canvas bytes (4 x canvas x frames per file) stay within stage_bytes
 * (0 = 256 MiB), but a group always holds at least one animation -- ONE ANIMATION'S CANVASES ARE ALWAYS STAGED TOGETHER,
 * whatever they take.  The grouping does not change a byte of the output.  A staging allocation that fails is ENOMEM
 * (every status ENOMEM). */
int vp8g_decode_webp_anim_tensor_scaled(const ByteSpan* files, uint32_t n, int filtered, uint32_t threads, uint32_t flags,
                                        const Vp8gScaleOpt* opts, uint32_t n_opts, uint64_t stage_bytes, const Vp8gTensorOpt* t,
                                        uint32_t channels, void* d_out, uint32_t* timestamps, int* status);

/* Name of the last HIP error seen by this library in the calling thread ("" if none). */
const char* vp8g_last_error(void);

/* How the calling thread's last reconstruction launch through vp8g_decode_batch_device or the
 * reference entry points ran: VP8G_MODE_* bits, 0 = one workgroup per frame (also after a call that
 * failed before its launch).  The end-to-end batch path (vp8g_decode_webp_batch[_ex]) does not set
 * it.  Diagnostics and tests. */
#define VP8G_MODE_CHAIN 1u        /* one 16-wave workgroup per CU decodes a chain of frames */
#define VP8G_MODE_MIRROR_SPLIT 2u /* frames split between a workgroup and its mirror */
#define VP8G_MODE_INTERLEAVE 4u   /* two frames of a chain interleaved */
#define VP8G_MODE_QUAD 8u         /* four MB rows per wave: set on every chain launch */
#define VP8G_MODE_SPLIT_PARTS 16u /* each frame over several workgroups */
uint32_t vp8g_last_launch_mode(void);

/* ABI version of this header (bumped on any layout change; the scale and tensor APIs above are
 * purely additive -- new symbols and structures, no existing layout touched -- and keep 5). */
#define VP8G_ABI_VERSION 5
uint32_t vp8g_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* VP8G_H */
