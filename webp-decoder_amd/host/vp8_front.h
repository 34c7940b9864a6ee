/*
 * vp8_front.h -- C11 host front end (container, frame header, bool decoder, modes, tokens).
 *
 * This is the producer of the hot path's input (Vp8DecodedFrame).  It is NOT on the GPU path
 * (serial entropy decode), but the CLI and the GPU-box tests need it,
 * so it is written here from RFC 6386 with the reference's exact output semantics and the same
 * public names as the reference modules it stands in for:
 *   webp_parse_simple_lossy    <- src/m01_container/webp_container.c:19  (a view of webp_locate_still, below)
 *   vp8_parse_keyframe_header  <- src/m02_vp8_header/vp8_header.c:13
 *   vp8_decode_decoded_frame   <- src/m05_tokens/vp8_tokens.c:673
 *   vp8_decoded_frame_free     <- src/m05_tokens/vp8_tokens.c:658
 * Unlike the reference (global g_coeff_probs, vp8_tokens.c:625) the decoder keeps all state
 * on the stack, so frames can be decoded concurrently from several threads.
 */
#ifndef VP8_FRONT_H
#define VP8_FRONT_H

#include "../../include/vp8g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* reference: src/m01_container/webp_container.h:8-15 */
typedef struct {
	uint32_t riff_size;
	size_t actual_size;
	size_t vp8_chunk_offset;
	uint32_t vp8_chunk_size;
} WebPContainer;

int webp_parse_simple_lossy(ByteSpan file, WebPContainer* out);
int vp8_parse_keyframe_header(ByteSpan vp8_payload, Vp8KeyFrameHeader* out);
int vp8_decode_decoded_frame(ByteSpan vp8_payload, Vp8DecodedFrame* out);
void vp8_decoded_frame_free(Vp8DecodedFrame* f);

/* Convenience for tools/tests: read a .webp file, parse container + key-frame header and
 * decode the macroblock data.  Returns 0, or -1 with errno and a stage code in *stage
 * (1 = open/read, 2 = container, 3 = key-frame header, 4 = macroblock/token decode). */
int vp8f_decode_file(const char* path, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* out, int* stage);

/* Same for an in-memory file image. */
int vp8f_decode_memory(const uint8_t* data, size_t size, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* out, int* stage);

/* m05 into the packed wire format (Vp8gPackedFrame, include/vp8g.h): same
 * decode, side arrays and stats as vp8_decode_decoded_frame, but each 4x4 block leaves only its
 * non-zero mask and values (no dense coefficient arrays).  The FNV coefficient hash is computed
 * only with VP8F_PACK_HASH (stats.coeff_hash_fnv1a64 = 0 otherwise).  Reentrant. */
#define VP8F_PACK_HASH 1u
/* also accept 2/4/8 token partitions (RFC 6386 9.5), which the reference rejects with ENOTSUP
 * (vp8_tokens.c:357-360); SURVEY §8(f4) */
#define VP8F_MULTI_PARTITION 2u
/* (the _memory forms only) read the container by webp_parse_extended's rules instead of
 * webp_parse_simple_lossy's: VP8X files decode, their ALPH chunk is not looked at */
#define VP8F_EXTENDED 4u
int vp8f_decode_packed(ByteSpan vp8_payload, Vp8gPackedFrame* out, unsigned flags);
/* container + key-frame header + vp8f_decode_packed; stage codes as vp8f_decode_file */
int vp8f_decode_packed_memory(const uint8_t* data, size_t size, Vp8gPackedFrame* out, int* stage, unsigned flags);
void vp8f_packed_free(Vp8gPackedFrame* p);
/* RFC 6386 9.5 token partition bounds [off[p], end[p]) within the VP8 payload (off / end may be
 * NULL to validate only).  0, or -1 + EINVAL when the size table or a partition overruns. */
int vp8f_partition_table(ByteSpan vp8_payload, uint32_t first_partition_len, unsigned nparts, uint32_t* off,
                         uint32_t* end);

/* Host half of the device m05 (Vp8gTokFrame, include/vp8g.h): key-frame header + the first
 * partition's frame-level fields; hdr receives those fields (no arrays), tf the device job
 * (data / mb_offset left 0 for the caller).  flags: VP8F_MULTI_PARTITION accepts 2/4/8 token
 * partitions.  0, or -1 + errno (EINVAL, ENOTSUP). */
int vp8f_token_header(ByteSpan vp8_payload, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* hdr, Vp8gTokFrame* tf,
                      unsigned flags);
/* container + vp8f_token_header; *payload_off / *payload_size locate the VP8 payload in data.
 * Stage codes as vp8f_decode_file (2 container, 3 not a key frame / bad frame header, 4 first
 * partition or unsupported partitioning). */
int vp8f_token_header_memory(const uint8_t* data, size_t size, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* hdr,
                             Vp8gTokFrame* tf, uint64_t* payload_off, uint32_t* payload_size, int* stage,
                             unsigned flags);

/* Seeded synthetic Vp8DecodedFrame (build-defined generator, see vp8_synth.c header for the
 * exact distribution).  profile 0 = "measured-like" statistics, 1 = stress (full-range coeffs,
 * all modes uniformly, random LF/segment parameters).  kf receives width/height. */
int vp8f_synth_frame(uint32_t width, uint32_t height, uint64_t seed, int profile, Vp8KeyFrameHeader* kf,
                     Vp8DecodedFrame* out);

/* ---- crop + rescale of I420, bit-exact to libwebp's rescaler (vp8_scale.c) --------------- */

/* A Vp8gScaleOpt (include/vp8g.h) resolved against a width x height picture: the luma window
 * (origin snapped down to even) and the output size.  The chroma window starts at
 * (left / 2, top / 2) and is ceil(win / 2) in size; chroma is scaled to ceil(out / 2). */
typedef struct {
	uint32_t left, top, win_w, win_h;
	uint32_t out_w, out_h;
	uint32_t scaling; /* a target size was given (else crop only) */
} Vp8fScaleGeom;

/* libwebp's rules: a crop needs w, h >= 1 and left + w <= width, top + h <= height (with the
 * caller's values); a target dimension of 0 is derived from the other with a ceiling
 * (h = (win_h * w + win_w - 1) / win_w), both 0 = no scaling.  Without VP8G_SCALE_EXPAND downscale
 * only: a target larger than the window in either dimension is -1 + EINVAL; with it a target
 * dimension (given or derived) may be up to 16383.  A picture beyond 16383 x 16383, unknown flags
 * or a NULL argument give -1 + EINVAL. */
int vp8f_scale_resolve(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, Vp8fScaleGeom* g);

/* Whether a `filtered` request runs the loop filter for this picture.  With
 * VP8G_SCALE_DWEBP_FILTER libwebp's rule applies: when scaling, the filter is skipped if
 * out_w < width * 3 / 4 and out_h < height * 3 / 4 (the full picture, not the crop). */
int vp8f_scale_filtered(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, int filtered);

/* The rescaler's three fixed-point factors of one plane W x H -> w x h, for the plane's mode per
 * axis (libwebp's values: fx = 0 when W < w, where it is unused; H < h: fy = 2^32 / x_add and
 * fxy = 0, unused). */
void vp8f_scale_factors(uint32_t W, uint32_t H, uint32_t w, uint32_t h, uint32_t* fx, uint32_t* fy, uint32_t* fxy);

/* Crop + rescale a width x height I420 image (plane pointers and strides) into the
 * destination planes, which must hold the resolved output size.  Sequential; reentrant.
 * 0, or -1 + errno (EINVAL, ENOMEM). */
int vp8f_scale_i420(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t stride_y, uint32_t stride_uv,
                    uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint8_t* dy, uint8_t* du, uint8_t* dv,
                    uint32_t dstride_y, uint32_t dstride_uv);

/* The three planes of libwebp's scaled RGB of a lossy picture: an option WITH a target size resolved
 * as above; Y from the luma window, U and V from the chroma window (ceil(win / 2) at (left / 2, top / 2)), every plane to
 * the same out_w x out_h with the plane arithmetic of vp8f_scale_i420 -- each axis of a plane shrinks or expands as its own
 * sizes say (128 -> 100 shrinks luma and expands chroma 64 -> 100), whatever VP8G_SCALE_EXPAND says of the luma target.
 * dy, du, dv: tight out_w x out_h planes.  The pixel is then VP8YuvToRgb(Y, U, V): no upsampler.  0, or -1 + errno
 * (EINVAL as vp8f_scale_resolve, and for an option without a target size; ENOMEM). */
int vp8f_scale_yuv444(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t stride_y, uint32_t stride_uv,
                      uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint8_t* dy, uint8_t* du, uint8_t* dv);

/* vp8f_scale_resolve for an ARGB picture (a lossless file): the same rules, but the window's origin is
 * taken as given -- libwebp rounds it down to even only where there is chroma to stay aligned with. */
int vp8f_scale_resolve_argb(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, Vp8fScaleGeom* g);

/* libwebp's alpha premultiply of n 0xAARRGGBB pixels in place (inverse = 0), or its inverse (1).  A is
 * kept; a == 255 leaves the pixel, a == 0 makes the whole pixel 0; otherwise each of R, G, B becomes
 * (x * scale + 2^23) >> 24 with scale = a * 65793 (65793 = 2^24 / 255), or (255 << 24) / a for the inverse. */
void vp8f_argb_mult_row(uint32_t* px, uint32_t n, int inverse);

/* Crop + rescale a tight width x height 0xAARRGGBB picture into `out` (tight, the resolved output size),
 * bit-exact to libwebp's decoder options on a lossless file: the window's rows are premultiplied, each of
 * the four byte channels is rescaled exactly as a luma plane above, and the output rows are
 * un-premultiplied.  Without a target size (crop only) the window's pixels are copied untouched.
 * VP8G_SCALE_DWEBP_FILTER means nothing here and is ignored.  Sequential; reentrant.  0, or -1 + errno
 * (EINVAL as vp8f_scale_resolve_argb, ENOMEM). */
int vp8f_argb_scale(const uint32_t* argb, uint32_t width, uint32_t height, const Vp8gScaleOpt* opt, uint32_t* out);

/* ---- a still picture located in its file -------------------------------- */

/* Where a file's payloads are: the one record of a still picture's container, read in one walk of its chunks.
 * Offsets are payload offsets from `data`, 0 = no such chunk; the image is 'VP8 ' (with or without an ALPH)
 * or 'VP8L', never both. */
typedef struct WebPStill {
	const uint8_t* data;
	size_t size;                                 /* of the file: what the batch planner prices it at */
	size_t vp8_offset, alph_offset, vp8l_offset;
	uint32_t vp8_size, alph_size, vp8l_size;
	uint32_t width, height;                      /* the canvas of a VP8X file, else the bitstream's size (0 x 0: a
	                                                simple lossy file whose frame header does not parse) */
	uint32_t riff_size;
	uint32_t extended;                           /* the file starts with a VP8X chunk */
	uint32_t vp8x_flags;                         /* its flag byte (ICC 0x20, alpha 0x10, EXIF 0x08, XMP 0x04, animation 0x02) */
} WebPStill;

/* What webp_locate_still accepts beyond the simple lossy layout, which is strict (RIFF size + 8 == file size, one
 * 'VP8 ' chunk with its pad byte, nothing behind it; the frame header is not looked at): */
#define WEBP_ACCEPT_EXTENDED 1u /* VP8X files, by the rules stated at webp_parse_extended */
#define WEBP_ACCEPT_LOSSLESS 2u /* (with WEBP_ACCEPT_EXTENDED) a 'VP8L' image too, by those at webp_parse_any */

/* The one walk.  `accept` picks whose verdict it gives: 0 webp_parse_simple_lossy's, WEBP_ACCEPT_EXTENDED
 * webp_parse_extended's, with WEBP_ACCEPT_LOSSLESS webp_parse_any's -- those three fill their structs from this
 * record.  0, or -1 + errno (EINVAL, ENOTSUP) with out->data / out->size set and the rest unspecified. */
int webp_locate_still(ByteSpan file, unsigned accept, WebPStill* out);

/* ---- extended container (VP8X) and the ALPH chunk (RFC 9649 2.7) ----------- */

/* What webp_parse_extended found.  alph_chunk_offset = 0: no alpha. */
typedef struct {
	uint32_t riff_size;
	size_t actual_size;
	size_t vp8_chunk_offset;
	uint32_t vp8_chunk_size;
	size_t alph_chunk_offset;
	uint32_t alph_chunk_size;
	uint32_t extended;       /* the file starts with a VP8X chunk */
	uint32_t vp8x_flags;     /* its flag byte (ICC 0x20, alpha 0x10, EXIF 0x08, XMP 0x04, animation 0x02) */
	uint32_t canvas_width, canvas_height;
} WebPContainerX;

/* webp_locate_still(WEBP_ACCEPT_EXTENDED) as a WebPContainerX (canvas 0 x 0 without VP8X).
 * The simple layout as webp_parse_simple_lossy reads it, or a VP8X file: the 10-byte VP8X chunk
 * first, then chunks up to the first 'VP8 ' chunk, which ends the parse as it does in libwebp (what
 * follows the image -- EXIF, XMP, a late ALPH -- is not looked at).  ICCP, EXIF, 'XMP ' and unknown
 * chunks are skipped (odd sizes padded); of several ALPH chunks before the image the last counts
 * (an empty one too: it then fails to decode); an ALPH chunk counts whether or not the VP8X alpha
 * flag is set, and the flag without a chunk means no alpha (an opaque picture).
 * riff_size may be smaller than the file (the rest is ignored); a riff_size beyond
 * the file, a chunk that overruns it, a missing image chunk or a canvas that differs from the VP8
 * frame size are -1 + EINVAL; the animation flag, ANIM / ANMF and a 'VP8L' image are -1 + ENOTSUP. */
int webp_parse_extended(ByteSpan file, WebPContainerX* out);

/* Which features of the format an ALPH stream used (tests and the golden script read it). */
typedef struct {
	uint32_t raw, lossless;          /* compression 0 / 1 */
	uint32_t predictor, cross_color, subtract_green, color_index; /* transforms */
	uint32_t pack_bits[4];           /* colour indexing at 1, 2, 4, 8 bits per pixel */
	uint32_t multi_group;            /* an entropy image with more than one prefix-code group */
	uint32_t backrefs, short_dist;   /* LZ77 copies; those through the 120-entry distance map */
	uint32_t cache_hits;             /* colour cache symbols */
	uint32_t simple_codes, normal_codes;
	uint32_t repeat_codes[3];        /* code-length codes 16, 17, 18 */
} Vp8fAlphaStats;

/* Entropy-decode an ALPH chunk payload (header byte + data) of a w x h picture into residual[w * h]
 * and *filter (0 none, 1 horizontal, 2 vertical, 3 gradient).  Compression 0 (raw) and 1 (the
 * RFC's lossless image stream, green channel); pre-processing and reserved bits are ignored.
 * stats may be NULL.  Reentrant.  0, or -1 + errno: EINVAL for a NULL argument, a size of 0 or beyond
 * 16383, an unknown compression, a malformed or truncated stream (never an over-read); ENOMEM. */
int vp8f_alpha_decode(const uint8_t* alph, size_t size, uint32_t w, uint32_t h, uint8_t* residual, uint32_t* filter,
                      Vp8fAlphaStats* stats);

/* The un-prediction, sequentially (tight planes): alpha = (pred + residual) & 255 with pred = 0 at
 * (0, 0), the left neighbour on the top row and the neighbour above in the left column for every
 * filter != 0, else left / above / clip255(left + above - aboveleft) for filters 1 / 2 / 3; filter 0
 * copies.  0, or -1 + EINVAL. */
int vp8f_alpha_unfilter(const uint8_t* residual, uint32_t w, uint32_t h, uint32_t filter, uint8_t* out);

/* ---- lossless (VP8L) main images (RFC 9649 3) ------------------------------ */

/* webp_parse_extended plus the lossless image chunk.  vp8l_chunk_offset = 0: a lossy file, whose
 * other fields are those of WebPContainerX; otherwise the image is the 'VP8L' chunk named here and
 * the vp8 / alph fields are 0 (an ALPH chunk beside a VP8L image is ignored, as libwebp ignores it). */
typedef struct {
	uint32_t riff_size;
	size_t actual_size;
	size_t vp8_chunk_offset;
	uint32_t vp8_chunk_size;
	size_t alph_chunk_offset;
	uint32_t alph_chunk_size;
	uint32_t extended;
	uint32_t vp8x_flags;
	uint32_t canvas_width, canvas_height;
	size_t vp8l_chunk_offset;
	uint32_t vp8l_chunk_size;
} WebPContainerL;

/* webp_locate_still(WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS) as a WebPContainerL:
 * webp_parse_extended, which also accepts a simple RIFF/WEBP/VP8L file (the chunk must lie inside
 * the file and the RIFF payload; what follows it is ignored) and a VP8X file whose image chunk is
 * 'VP8L'.  Animation stays -1 + ENOTSUP; a VP8X canvas that differs from the VP8L header's size, or
 * a VP8L header that does not parse, is -1 + EINVAL. */
int webp_parse_any(ByteSpan file, WebPContainerL* out);

/* The 5-byte header of a VP8L chunk payload: signature 0x2f, 14 + 14 bits of width - 1 and
 * height - 1, the alpha hint, a 3-bit version.  0, or -1 + EINVAL (NULL, fewer than 5 bytes, a wrong
 * signature, a non-zero version). */
int vp8f_lossless_header(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* alpha_hint);

enum { VP8F_T_PREDICTOR = 0, VP8F_T_CROSS_COLOR = 1, VP8F_T_SUBTRACT_GREEN = 2, VP8F_T_COLOR_INDEX = 3 };

typedef struct {
	uint32_t type;    /* VP8F_T_* */
	uint32_t bits;    /* block size (predictor, cross colour) or pixels per packed pixel (colour index), log2 */
	uint32_t xsize;   /* image width when the transform was read (its output width) */
	uint32_t ncolors; /* colour index: entries of the table */
	uint32_t* data;   /* sub-image of div_up(xsize, bits) x div_up(height, bits), or the colour table, prefix-summed */
} Vp8fLosslessTransform;

/* What the entropy half leaves: the ARGB residual image (xsize x height: the packed width when a
 * colour-indexing transform is present, else the width) and the transforms in stream order. */
typedef struct {
	uint32_t width, height, alpha_hint;
	uint32_t xsize;
	uint32_t ntransforms;
	uint32_t reserved;
	uint32_t* argb;
	Vp8fLosslessTransform tr[4];
} Vp8fLosslessImage;

/* Entropy-decode a VP8L chunk payload (header + stream) into *out; no inverse transform is applied.
 * stats may be NULL.  Reentrant.  0, or -1 + errno as vp8f_alpha_decode (EINVAL for a malformed or
 * truncated stream, never an over-read; ENOMEM), with *out zeroed.  vp8f_lossless_free releases *out. */
int vp8f_lossless_decode(const uint8_t* data, size_t size, Vp8fLosslessImage* out, Vp8fAlphaStats* stats);
void vp8f_lossless_free(Vp8fLosslessImage* img);

/* The inverse transforms, sequentially, last to first: argb[width * height] = 0xAARRGGBB.  The
 * authority the device kernel (csrc/vp8g_lossless.hip) is tested against.  0, or -1 + EINVAL / ENOMEM. */
int vp8f_lossless_apply(const Vp8fLosslessImage* img, uint32_t* argb);

/* ---- animation (ANIM / ANMF chunks, RFC 9649 2.7.1.1) ---------------------- */

/* What webp_parse_anim found in the file as a whole. */
typedef struct {
	uint32_t canvas_width, canvas_height;
	uint32_t bgcolor;    /* the ANIM chunk's background colour as stored; the compositor ignores it, as libwebp's does */
	uint32_t loop_count; /* 0 = forever */
	uint32_t nframes;    /* frames of the file (which may be more than the caller had room for) */
	uint32_t vp8x_flags;
} WebPAnimInfo;

/* One ANMF chunk.  The rectangle's size is that of the frame's bitstream, whatever the ANMF header names (libwebp's reading).
 * Spans are payload offsets in the file and payload sizes; a size of 0 = no such sub-chunk.  An image is
 * 'VP8 ' (with an optional 'ALPH' in front) or 'VP8L'.  80 bytes. */
typedef struct {
	size_t offset;                               /* the ANMF payload (its 16 header bytes first) */
	size_t alph_offset, vp8_offset, vp8l_offset;
	uint32_t size, alph_size, vp8_size, vp8l_size;
	uint32_t x, y, width, height;                /* x, y even */
	uint32_t duration;                           /* ms */
	uint32_t blend;                              /* 1: alpha-blend over the canvas, 0: overwrite */
	uint32_t dispose;                            /* 1: the rectangle is cleared to transparent after the frame */
	uint32_t has_alpha;                          /* an ALPH chunk, or the alpha bit of the VP8L header */
} WebPAnimFrame;

/* The animated layout: 'VP8X' with the animation flag, one 'ANIM', then 'ANMF' chunks (metadata and unknown
 * chunks between them skipped; a second ANIM ignored).  *info is always filled on success; frames (may be NULL
 * with max_frames = 0: count only) receives the first max_frames frames in file order.  The verdict is that of
 * libwebp's WebPAnimDecoderNew (tests/golden/anim.json records it for the directed files): -1 + EINVAL for a file
 * that is not an animation (a still picture, the flag without frames, ANMF without the flag), a reserved VP8X flag
 * bit, a canvas beyond 16383 in either dimension (this decoder's limit, not libwebp's), a RIFF payload beyond
 * the file, a chunk that overruns it, an ANMF before ANIM or shorter than its header, a top-level image chunk,
 * an ALPH without an image, behind its image or in front of a VP8L, a frame whose bitstream header does not parse,
 * or whose rectangle (the bitstream's size at the ANMF's offset) leaves the canvas.  libwebp reads what follows a frame's
 * image inside the ANMF as chunks of the top level, and so does this: unknown chunks there are skipped, an image there
 * is refused, and an ANMF in which nothing recognised comes first is no frame at all (it is dropped where its content
 * passes as top-level chunks, refused where an image follows or where it ends the file). */
int webp_parse_anim(ByteSpan file, WebPAnimInfo* info, WebPAnimFrame* frames, uint32_t max_frames);

/* One frame as the compositor sees it: a tight width x height 0xAARRGGBB picture (not premultiplied: the bytes
 * WebPDecodeRGBA gives) and where it goes.  key is filled by vp8f_anim_keyframes. */
typedef struct {
	const uint32_t* argb;
	uint32_t x, y, width, height;
	uint32_t blend, dispose, has_alpha;
	uint32_t key;
} Vp8fAnimFrame;

/* libwebp's key-frame rule (WebPAnimDecoder): frame 0 is a key frame; frame k is one if it covers the canvas and
 * has no alpha or does not blend, or if frame k - 1 disposes to background and covered the canvas or was a key
 * frame.  Sets frames[k].key.  0, or -1 + EINVAL (NULL, n = 0, a canvas of 0 or beyond 16383, an empty rectangle
 * or one outside the canvas). */
int vp8f_anim_keyframes(uint32_t canvas_w, uint32_t canvas_h, Vp8fAnimFrame* frames, uint32_t n);

/* The n canvases of an animation, sequentially, as WebPAnimDecoder (MODE_RGBA) composes them: canvases[k] (tight
 * canvas_w x canvas_h dwords each, 0xAARRGGBB) is what is shown for frame k.  A key frame starts from an all-zero
 * canvas, any other from the previous canvas after its disposal; the frame's pixels overwrite its rectangle, except
 * that a pixel is blended over the canvas below (non-premultiplied, libwebp's fixed-point formula; source alpha 255
 * keeps the source, 0 keeps the canvas pixel whole) when the frame blends, is no key frame, and the canvas pixel was
 * not just cleared by the previous frame's disposal.  The key flags are computed here (frames[k].key is not read).
 * The authority the device kernel (csrc/vp8g_anim.hip) is tested against.  0, or -1 + EINVAL / ENOMEM. */
int vp8f_anim_compose(uint32_t canvas_w, uint32_t canvas_h, const Vp8fAnimFrame* frames, uint32_t n, uint32_t* canvases);

/* FNV-1a 64 over a byte buffer (same constants as reference vp8_tokens.c:15-27). */
uint64_t vp8f_fnv1a64(const void* data, size_t n, uint64_t h);

#ifdef __cplusplus
}
#endif

#endif
