/*
 * webp_riff.c -- the RIFF/WEBP container (RFC 9649) and the VP8 frame tag / key-frame header (RFC 6386 9.1).
 *   container: one chunk iterator (riff_chunk) under two walks: a still picture's (webp_locate_still, of which
 *              webp_parse_simple_lossy, webp_parse_extended and webp_parse_any are views) and an animation's
 *              (webp_parse_anim).  The simple lossy layout keeps the reference's acceptance rules: 'RIFF' <size>
 *              'WEBP' then exactly one 'VP8 ' chunk, RIFF size + 8 == file size, nothing after the (even-padded)
 *              chunk  (reference src/m01_container/webp_container.c:19-89); the others libwebp's.
 *   header:    key frame, start code 9d 01 2a, 14-bit non-zero width/height, first partition
 *              fits in the payload  (reference src/m02_vp8_header/vp8_header.c:13-66)
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vp8_front.h"

static uint32_t rd_le32(const uint8_t* p) {
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static uint32_t rd_le24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

typedef struct {
	const uint8_t* tag; /* four bytes */
	uint32_t size;      /* of the payload, which starts 8 bytes behind the tag */
	size_t padded;      /* ... rounded up to even: the next chunk is 8 + padded on */
} RiffChunk;

static int tagged(const RiffChunk* c, const char* tag) { return memcmp(c->tag, tag, 4) == 0; }

/* The chunk at pos of a RIFF payload that ends at `end` (pos <= end): the one statement of a chunk header's bounds.
 * 0 = refused: no room for a header, or a size beyond 0xFFFFFFF6 or beyond the payload.  1 = the chunk and its pad
 * byte lie inside.  2 = the chunk does, its pad byte is missing: a still picture's image chunk may end so, no other. */
static int riff_chunk(const uint8_t* data, size_t pos, size_t end, RiffChunk* c) {
	if (end - pos < 8u) return 0;
	c->tag = data + pos;
	c->size = rd_le32(data + pos + 4);
	c->padded = (size_t)c->size + (c->size & 1u);
	if (c->size > 0xFFFFFFF6u || (size_t)c->size > end - pos - 8u) return 0;
	return c->padded > end - pos - 8u ? 2 : 1;
}

/* The end of a RIFF payload of at least `least` bytes that must lie inside the file (bytes after it are ignored), or 0. */
static size_t riff_end(ByteSpan file, uint32_t least) {
	const uint32_t riff_size = rd_le32(file.data + 4);
	if (riff_size < least || riff_size > 0xFFFFFFF6u || (size_t)riff_size > file.size - 8u) return 0;
	return 8u + (size_t)riff_size;
}

static int refuse(int e) {
	errno = e;
	return -1;
}

/* RFC 9649 2.5 - 2.7, with libwebp's reading where the RFC leaves a choice (tests/golden/alpha.json and lossless.json
 * record its verdict on the directed containers). */
int webp_locate_still(ByteSpan file, unsigned accept, WebPStill* out) {
	if (!out) return -1;
	memset(out, 0, sizeof(*out));
	out->data = file.data, out->size = file.size;
	const uint8_t* d = file.data;
	const int ext = (accept & WEBP_ACCEPT_EXTENDED) != 0, lossless = ext && (accept & WEBP_ACCEPT_LOSSLESS);
	if (!d || file.size < 12 || memcmp(d, "RIFF", 4) != 0) return refuse(EINVAL);
	out->riff_size = rd_le32(d + 4);
	if (file.size < 20 || memcmp(d + 8, "WEBP", 4) != 0) return refuse(EINVAL);
	const int vp8x = ext && memcmp(d + 12, "VP8X", 4) == 0;
	const int simple_vp8l = ext && memcmp(d + 12, "VP8L", 4) == 0;
	if (simple_vp8l && !lossless) return refuse(ENOTSUP);
	size_t pos = 12, end = file.size;
	if (vp8x || simple_vp8l) {
		if ((end = riff_end(file, 12)) == 0) return refuse(EINVAL);
	} else if ((size_t)out->riff_size + 8u != file.size) { /* the simple lossy layout is strict */
		return refuse(EINVAL);
	}
	if (vp8x) {
		if (end < 30u || rd_le32(d + 16) != 10u) return refuse(EINVAL);
		out->extended = 1;
		out->vp8x_flags = d[20];
		out->width = 1u + rd_le24(d + 24), out->height = 1u + rd_le24(d + 27);
		if (out->vp8x_flags & 0x02u) return refuse(ENOTSUP);
		pos = 30;
	}
	RiffChunk c;
	for (;;) { /* up to the image chunk */
		const int got = riff_chunk(d, pos, end, &c);
		if (!got) return refuse(EINVAL); /* (also: no image chunk) */
		const int is_vp8 = tagged(&c, "VP8 "), is_vp8l = tagged(&c, "VP8L");
		if (!vp8x) { /* a simple layout: the image chunk and, for the lossy one, nothing behind it */
			if (simple_vp8l ? !is_vp8l : (!is_vp8 || pos + 8u + c.padded != end)) return refuse(EINVAL);
		} else if ((is_vp8l && !lossless) || tagged(&c, "ANIM") || tagged(&c, "ANMF")) {
			return refuse(ENOTSUP);
		}
		if (is_vp8) out->vp8_offset = pos + 8u, out->vp8_size = c.size;
		if (is_vp8l) { /* (an ALPH chunk beside a VP8L image is ignored, as libwebp ignores it) */
			out->vp8l_offset = pos + 8u, out->vp8l_size = c.size;
			out->alph_offset = 0, out->alph_size = 0;
		}
		if (is_vp8 || is_vp8l) break;
		if (tagged(&c, "ALPH")) out->alph_offset = pos + 8u, out->alph_size = c.size;
		if (got != 1) return refuse(EINVAL);
		pos += 8u + c.padded;
	}
	/* the bitstream's size: in a VP8X file it must be the canvas; in the simple lossy layout a frame header that does
	 * not parse is not the container's business (0 x 0) */
	uint32_t w = 0, h = 0, hint;
	Vp8KeyFrameHeader kf;
	if (out->vp8l_offset) {
		if (vp8f_lossless_header(d + out->vp8l_offset, out->vp8l_size, &w, &h, &hint) != 0) return -1;
	} else {
		const ByteSpan payload = {d + out->vp8_offset, out->vp8_size};
		if (vp8_parse_keyframe_header(payload, &kf) == 0) w = kf.width, h = kf.height;
		else if (vp8x) return -1;
	}
	if (vp8x && (w != out->width || h != out->height)) return refuse(EINVAL);
	out->width = w, out->height = h;
	return 0;
}

/* ---- the three parsers: views of a WebPStill ----------------------------------------------- */

int webp_parse_simple_lossy(ByteSpan file, WebPContainer* out) {
	if (!out) return -1;
	WebPStill s;
	const int rc = webp_locate_still(file, 0, &s);
	memset(out, 0, sizeof(*out));
	out->riff_size = s.riff_size, out->actual_size = file.size;
	out->vp8_chunk_offset = s.vp8_offset, out->vp8_chunk_size = s.vp8_size;
	return rc;
}

int webp_parse_any(ByteSpan file, WebPContainerL* out) {
	if (!out) return -1;
	WebPStill s;
	const int rc = webp_locate_still(file, WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS, &s);
	memset(out, 0, sizeof(*out));
	out->riff_size = s.riff_size, out->actual_size = file.size;
	out->vp8_chunk_offset = s.vp8_offset, out->vp8_chunk_size = s.vp8_size;
	out->alph_chunk_offset = s.alph_offset, out->alph_chunk_size = s.alph_size;
	out->vp8l_chunk_offset = s.vp8l_offset, out->vp8l_chunk_size = s.vp8l_size;
	out->extended = s.extended, out->vp8x_flags = s.vp8x_flags;
	if (s.extended || s.vp8l_offset) out->canvas_width = s.width, out->canvas_height = s.height; /* (a simple lossy file names none) */
	return rc;
}

int webp_parse_extended(ByteSpan file, WebPContainerX* out) {
	if (!out) return -1;
	WebPStill s;
	const int rc = webp_locate_still(file, WEBP_ACCEPT_EXTENDED, &s);
	memset(out, 0, sizeof(*out));
	out->riff_size = s.riff_size, out->actual_size = file.size;
	out->vp8_chunk_offset = s.vp8_offset, out->vp8_chunk_size = s.vp8_size;
	out->alph_chunk_offset = s.alph_offset, out->alph_chunk_size = s.alph_size;
	out->extended = s.extended, out->vp8x_flags = s.vp8x_flags;
	if (s.extended) out->canvas_width = s.width, out->canvas_height = s.height;
	return rc;
}

int vp8f_lossless_header(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* alpha_hint) {
	if (!data || !width || !height || !alpha_hint || size < 5 || data[0] != 0x2f) return refuse(EINVAL);
	const uint32_t v = rd_le32(data + 1);
	if (v >> 29) return refuse(EINVAL); /* version */
	*width = (v & 0x3FFFu) + 1u, *height = ((v >> 14) & 0x3FFFu) + 1u, *alpha_hint = (v >> 28) & 1u;
	return 0;
}

/* The sub-chunks of one frame from *pos on, in a RIFF payload that ends at `end`, as libwebp's demuxer walks them: an
 * optional ALPH, then 'VP8 ' or 'VP8L'; the walk stops in front of the first chunk that is neither (or a second of
 * either kind) and leaves *pos there.  1 = a frame, 0 = nothing it recognises came first (libwebp drops such a frame
 * without a word), -1 = refused. */
static int anim_frame_chunks(const uint8_t* data, size_t* at, size_t end, WebPAnimFrame* f) {
	uint32_t bw = 0, bh = 0, hint = 0;
	size_t pos = *at;
	for (;;) {
		RiffChunk c; /* (a frame's walk needs a chunk header to look at, and one after each chunk it took) */
		if (riff_chunk(data, pos, end, &c) != 1) return -1;
		const int is_vp8 = tagged(&c, "VP8 "), is_vp8l = tagged(&c, "VP8L");
		if (tagged(&c, "ALPH")) {
			if (f->alph_offset) break;
			f->alph_offset = pos + 8u, f->alph_size = c.size;
		} else if (is_vp8 || is_vp8l) {
			if (is_vp8l && f->alph_offset) return -1;
			if (f->vp8_offset || f->vp8l_offset) break;
			if (is_vp8) {
				Vp8KeyFrameHeader kf;
				ByteSpan payload = {c.tag + 8, c.size};
				if (vp8_parse_keyframe_header(payload, &kf) != 0) return -1;
				bw = kf.width, bh = kf.height;
				f->vp8_offset = pos + 8u, f->vp8_size = c.size;
			} else {
				if (vp8f_lossless_header(c.tag + 8, c.size, &bw, &bh, &hint) != 0) return -1;
				f->vp8l_offset = pos + 8u, f->vp8l_size = c.size;
			}
			f->width = bw, f->height = bh; /* (the bitstream's size counts, whatever the ANMF header names: as in libwebp) */
		} else {
			break;
		}
		pos += 8u + c.padded;
		if (pos == end) break;
	}
	*at = pos;
	if (!f->alph_offset && !f->vp8_offset && !f->vp8l_offset) return 0;
	/* an ALPH alone, or one behind its image */
	if (!f->vp8_offset && !f->vp8l_offset) return -1;
	if (f->alph_offset && f->alph_offset > (f->vp8_offset ? f->vp8_offset : f->vp8l_offset)) return -1;
	f->has_alpha = f->alph_offset ? 1u : hint;
	return 1;
}

static int parse_anim(ByteSpan file, WebPAnimInfo* info, WebPAnimFrame* frames, uint32_t max_frames) {
	if (!file.data || file.size < 20 || memcmp(file.data, "RIFF", 4) != 0 || memcmp(file.data + 8, "WEBP", 4) != 0) return -1;
	const size_t end = riff_end(file, 22); /* (a VP8X chunk at the least) */
	RiffChunk c;
	if (!end || riff_chunk(file.data, 12, end, &c) != 1 || !tagged(&c, "VP8X") || c.size < 10u) return -1; /* (not VP8X: a still picture) */
	info->vp8x_flags = file.data[20];
	info->canvas_width = 1u + rd_le24(file.data + 24), info->canvas_height = 1u + rd_le24(file.data + 27);
	/* (libwebp's limit is the canvas area; this decoder's is the size of a tensor's picture) */
	if (info->canvas_width > 16383u || info->canvas_height > 16383u) return -1;
	if (!(info->vp8x_flags & 0x02u) || (info->vp8x_flags & ~0x3Eu)) return -1;
	size_t pos = 20u + c.padded;
	uint32_t anims = 0, n = 0;
	while (pos != end) {
		if (riff_chunk(file.data, pos, end, &c) != 1) return -1;
		if (tagged(&c, "VP8X") || tagged(&c, "VP8 ") || tagged(&c, "VP8L") || tagged(&c, "ALPH")) return -1;
		const uint8_t* p = c.tag + 8;
		if (tagged(&c, "ANIM")) {
			if (c.padded < 6u) return -1;
			if (anims++ == 0) info->bgcolor = rd_le32(p), info->loop_count = (uint32_t)p[4] | (uint32_t)p[5] << 8;
		} else if (tagged(&c, "ANMF")) {
			if (anims == 0 || c.padded < 16u) return -1;
			WebPAnimFrame f;
			memset(&f, 0, sizeof(f));
			f.offset = pos + 8u, f.size = c.size;
			f.x = 2u * rd_le24(p), f.y = 2u * rd_le24(p + 3), f.width = 1u + rd_le24(p + 6), f.height = 1u + rd_le24(p + 9);
			f.duration = rd_le24(p + 12);
			f.dispose = p[15] & 1u, f.blend = (p[15] & 2u) ? 0u : 1u;
			size_t at = pos + 24u;
			const int got = anim_frame_chunks(file.data, &at, end, &f);
			if (got < 0 || at > pos + 8u + c.padded) return -1; /* (a sub-chunk that runs past the ANMF's own end) */
			if (got > 0) {
				if ((uint64_t)f.x + f.width > info->canvas_width || (uint64_t)f.y + f.height > info->canvas_height) return -1;
				if (n < max_frames) frames[n] = f;
				if (++n == 0) return -1;
			}
			/* libwebp goes on from where the frame's walk stopped, not from the ANMF's end: what follows the image
			 * inside the ANMF is read as chunks of the top level (an unknown one is skipped, an image refused) */
			pos = at;
			continue;
		}
		pos += 8u + c.padded;
	}
	if (n == 0) return -1;
	info->nframes = n;
	return 0;
}

int webp_parse_anim(ByteSpan file, WebPAnimInfo* info, WebPAnimFrame* frames, uint32_t max_frames) {
	if (info) memset(info, 0, sizeof(*info));
	if (!info || (max_frames && !frames) || parse_anim(file, info, frames, max_frames) != 0) {
		if (info) memset(info, 0, sizeof(*info));
		errno = EINVAL; /* (every refusal is this one) */
		return -1;
	}
	return 0;
}

int vp8_parse_keyframe_header(ByteSpan p, Vp8KeyFrameHeader* out) {
	if (!out) return -1;
	memset(out, 0, sizeof(*out));
	if (!p.data || p.size < 10) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t tag = (uint32_t)p.data[0] | ((uint32_t)p.data[1] << 8) | ((uint32_t)p.data[2] << 16);
	out->is_key_frame = (tag & 1u) == 0;
	out->profile = (uint8_t)((tag >> 1) & 7u);
	out->show_frame = (int)((tag >> 4) & 1u);
	out->first_partition_len = tag >> 5;
	if (!out->is_key_frame) {
		errno = EINVAL;
		return -1;
	}
	out->start_code_ok = p.data[3] == 0x9d && p.data[4] == 0x01 && p.data[5] == 0x2a;
	if (!out->start_code_ok) {
		errno = EINVAL;
		return -1;
	}
	const uint16_t w = (uint16_t)(p.data[6] | (p.data[7] << 8));
	const uint16_t h = (uint16_t)(p.data[8] | (p.data[9] << 8));
	out->width = w & 0x3FFF;
	out->x_scale = (uint8_t)(w >> 14);
	out->height = h & 0x3FFF;
	out->y_scale = (uint8_t)(h >> 14);
	if (out->width == 0 || out->height == 0 || out->first_partition_len > p.size - 10) {
		errno = EINVAL;
		return -1;
	}
	return 0;
}

/* the VP8 payload of a file: the simple layout, or with VP8F_EXTENDED the extended one as well */
static int locate_vp8(const uint8_t* data, size_t size, unsigned flags, ByteSpan* payload, size_t* offset) {
	WebPStill s;
	const ByteSpan file = {data, size};
	if (webp_locate_still(file, (flags & VP8F_EXTENDED) ? WEBP_ACCEPT_EXTENDED : 0u, &s) != 0) return -1;
	payload->data = data + s.vp8_offset, payload->size = s.vp8_size;
	if (offset) *offset = s.vp8_offset;
	return 0;
}

int vp8f_decode_memory(const uint8_t* data, size_t size, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* out, int* stage) {
	int st = 0, rc = -1;
	ByteSpan payload;
	if (locate_vp8(data, size, 0, &payload, NULL) != 0) st = 2;
	else if (vp8_parse_keyframe_header(payload, kf) != 0 || !kf->is_key_frame) st = 3;
	else if (vp8_decode_decoded_frame(payload, out) != 0) st = 4;
	else rc = 0;
	if (stage) *stage = st;
	return rc;
}

int vp8f_decode_packed_memory(const uint8_t* data, size_t size, Vp8gPackedFrame* out, int* stage, unsigned flags) {
	int st = 0, rc = -1;
	ByteSpan payload;
	if (out) memset(out, 0, sizeof(*out));
	if (!out) {
		errno = EINVAL;
		st = 4;
	} else if (locate_vp8(data, size, flags, &payload, NULL) != 0) {
		st = 2;
	} else {
		if (vp8_parse_keyframe_header(payload, &out->kf) != 0 || !out->kf.is_key_frame) st = 3;
		else if (vp8f_decode_packed(payload, out, flags & ~VP8F_EXTENDED) != 0) st = 4;
		else rc = 0;
	}
	if (stage) *stage = st;
	return rc;
}

int vp8f_token_header_memory(const uint8_t* data, size_t size, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* hdr,
                             Vp8gTokFrame* tf, uint64_t* payload_off, uint32_t* payload_size, int* stage,
                             unsigned flags) {
	int st = 0, rc = -1;
	ByteSpan payload;
	size_t off;
	if (!kf || !hdr || !tf || !payload_off || !payload_size) {
		errno = EINVAL;
		st = 4;
	} else if (locate_vp8(data, size, flags, &payload, &off) != 0) {
		st = 2;
	} else if (payload.size > 0xFFFFFFF0u) {
		errno = EFBIG;
		st = 4;
	} else {
		if (vp8_parse_keyframe_header(payload, kf) != 0 || !kf->is_key_frame) {
			errno = EINVAL;
			st = 3;
		} else if (vp8f_token_header(payload, kf, hdr, tf, flags & ~VP8F_EXTENDED) != 0) {
			st = 4;
		} else {
			*payload_off = off;
			*payload_size = (uint32_t)payload.size;
			rc = 0;
		}
	}
	if (stage) *stage = st;
	return rc;
}

int vp8f_decode_file(const char* path, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* out, int* stage) {
	FILE* fp = fopen(path, "rb");
	if (!fp) {
		if (stage) *stage = 1;
		return -1;
	}
	uint8_t* buf = NULL;
	size_t cap = 0, n = 0;
	for (;;) {
		if (n == cap) {
			cap = cap ? cap * 2 : (1u << 16);
			uint8_t* nb = (uint8_t*)realloc(buf, cap);
			if (!nb) {
				free(buf);
				fclose(fp);
				errno = ENOMEM;
				if (stage) *stage = 1;
				return -1;
			}
			buf = nb;
		}
		size_t got = fread(buf + n, 1, cap - n, fp);
		n += got;
		if (got == 0) break;
	}
	int err = ferror(fp);
	fclose(fp);
	if (err) {
		free(buf);
		errno = EIO;
		if (stage) *stage = 1;
		return -1;
	}
	int rc = vp8f_decode_memory(buf, n, kf, out, stage);
	int e = errno;
	free(buf);
	errno = e;
	return rc;
}
