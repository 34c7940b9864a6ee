/*
 * webp_riff.c -- RIFF/WEBP container (RFC 9649 simple lossy layout) and the VP8 frame tag /
 * key-frame header (RFC 6386 9.1), with the reference's acceptance rules:
 *   container: 'RIFF' <size> 'WEBP' then exactly one 'VP8 ' chunk, RIFF size + 8 == file size,
 *              nothing after the (even-padded) chunk  (reference src/m01_container/webp_container.c:19-89)
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

int webp_parse_simple_lossy(ByteSpan file, WebPContainer* out) {
	if (!out) return -1;
	memset(out, 0, sizeof(*out));
	out->actual_size = file.size;
	if (!file.data || file.size < 12 || memcmp(file.data, "RIFF", 4) != 0) {
		errno = EINVAL;
		return -1;
	}
	out->riff_size = rd_le32(file.data + 4);
	if (memcmp(file.data + 8, "WEBP", 4) != 0 || (size_t)out->riff_size + 8u != file.size || file.size < 20) {
		errno = EINVAL;
		return -1;
	}
	const uint8_t* chunk = file.data + 12;
	const uint32_t csize = rd_le32(chunk + 4);
	if (memcmp(chunk, "VP8 ", 4) != 0 || csize > file.size - 20) {
		errno = EINVAL;
		return -1;
	}
	size_t end = 20u + (size_t)csize;
	end += end & 1u; /* chunks are padded to even length */
	if (end != file.size) {
		errno = EINVAL;
		return -1;
	}
	out->vp8_chunk_offset = 20;
	out->vp8_chunk_size = csize;
	return 0;
}

/* RFC 9649 2.7 (extended file format), with libwebp's reading where the RFC leaves a choice
 * (tests/golden/alpha.json records its verdict on the directed containers). */
int webp_parse_extended(ByteSpan file, WebPContainerX* out) {
	if (!out) return -1;
	memset(out, 0, sizeof(*out));
	out->actual_size = file.size;
	if (!file.data || file.size < 20 || memcmp(file.data, "RIFF", 4) != 0 || memcmp(file.data + 8, "WEBP", 4) != 0) {
		errno = EINVAL;
		return -1;
	}
	if (memcmp(file.data + 12, "VP8X", 4) != 0) {
		WebPContainer c;
		if (memcmp(file.data + 12, "VP8L", 4) == 0) {
			errno = ENOTSUP;
			return -1;
		}
		if (webp_parse_simple_lossy(file, &c) != 0) return -1;
		out->riff_size = c.riff_size;
		out->vp8_chunk_offset = c.vp8_chunk_offset, out->vp8_chunk_size = c.vp8_chunk_size;
		return 0;
	}
	out->riff_size = rd_le32(file.data + 4);
	/* the RIFF payload must lie inside the file; bytes after it are ignored */
	if (out->riff_size > 0xFFFFFFF6u || (size_t)out->riff_size > file.size - 8u || out->riff_size < 12u) {
		errno = EINVAL;
		return -1;
	}
	const size_t end = 8u + (size_t)out->riff_size;
	if (end < 30u || rd_le32(file.data + 16) != 10u) {
		errno = EINVAL;
		return -1;
	}
	out->extended = 1;
	out->vp8x_flags = file.data[20];
	out->canvas_width = 1u + ((uint32_t)file.data[24] | (uint32_t)file.data[25] << 8 | (uint32_t)file.data[26] << 16);
	out->canvas_height = 1u + ((uint32_t)file.data[27] | (uint32_t)file.data[28] << 8 | (uint32_t)file.data[29] << 16);
	if (out->vp8x_flags & 0x02u) {
		errno = ENOTSUP;
		return -1;
	}
	size_t pos = 30;
	for (;;) {
		if (end - pos < 8u) { /* no image chunk */
			errno = EINVAL;
			return -1;
		}
		const uint8_t* chunk = file.data + pos;
		const uint32_t csize = rd_le32(chunk + 4);
		if (csize > 0xFFFFFFF6u || (size_t)csize > end - pos - 8u) {
			errno = EINVAL;
			return -1;
		}
		if (memcmp(chunk, "VP8L", 4) == 0 || memcmp(chunk, "ANIM", 4) == 0 || memcmp(chunk, "ANMF", 4) == 0) {
			errno = ENOTSUP;
			return -1;
		}
		if (memcmp(chunk, "VP8 ", 4) == 0) {
			out->vp8_chunk_offset = pos + 8u, out->vp8_chunk_size = csize;
			break;
		}
		if (memcmp(chunk, "ALPH", 4) == 0) out->alph_chunk_offset = pos + 8u, out->alph_chunk_size = csize;
		const size_t padded = (size_t)csize + (csize & 1u);
		if (padded > end - pos - 8u) { /* (the pad byte of the last chunk may be missing only for the image) */
			errno = EINVAL;
			return -1;
		}
		pos += 8u + padded;
	}
	Vp8KeyFrameHeader kf;
	ByteSpan payload = {file.data + out->vp8_chunk_offset, out->vp8_chunk_size};
	if (vp8_parse_keyframe_header(payload, &kf) != 0) return -1;
	if (kf.width != out->canvas_width || kf.height != out->canvas_height) {
		errno = EINVAL;
		return -1;
	}
	return 0;
}

/* (here, not beside the stream decoder in vp8_alpha.c: webp_parse_any needs it, and this file links on its own) */
int vp8f_lossless_header(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* alpha_hint) {
	if (!data || !width || !height || !alpha_hint || size < 5 || data[0] != 0x2f) {
		errno = EINVAL;
		return -1;
	}
	const uint32_t v = (uint32_t)data[1] | (uint32_t)data[2] << 8 | (uint32_t)data[3] << 16 | (uint32_t)data[4] << 24;
	if (v >> 29) { /* version */
		errno = EINVAL;
		return -1;
	}
	*width = (v & 0x3FFFu) + 1u, *height = ((v >> 14) & 0x3FFFu) + 1u, *alpha_hint = (v >> 28) & 1u;
	return 0;
}

static void copy_container(WebPContainerL* out, const WebPContainerX* x) {
	out->riff_size = x->riff_size, out->actual_size = x->actual_size;
	out->vp8_chunk_offset = x->vp8_chunk_offset, out->vp8_chunk_size = x->vp8_chunk_size;
	out->alph_chunk_offset = x->alph_chunk_offset, out->alph_chunk_size = x->alph_chunk_size;
	out->extended = x->extended, out->vp8x_flags = x->vp8x_flags;
	out->canvas_width = x->canvas_width, out->canvas_height = x->canvas_height;
}

/* webp_parse_extended's walk, with a 'VP8L' image chunk accepted (simple layout: as libwebp reads it, the
 * chunk inside the RIFF payload and the file, the rest ignored). */
int webp_parse_any(ByteSpan file, WebPContainerL* out) {
	if (!out) return -1;
	memset(out, 0, sizeof(*out));
	WebPContainerX x;
	if (webp_parse_extended(file, &x) == 0) {
		copy_container(out, &x);
		return 0;
	}
	if (errno != ENOTSUP) {
		out->actual_size = file.size;
		return -1;
	}
	/* animation, or a lossless image: the file has passed the checks in front of the chunk walk */
	copy_container(out, &x);
	out->vp8_chunk_offset = 0, out->vp8_chunk_size = 0, out->alph_chunk_offset = 0, out->alph_chunk_size = 0;
	size_t pos, end;
	if (!x.extended) {
		out->riff_size = rd_le32(file.data + 4);
		if (out->riff_size > 0xFFFFFFF6u || (size_t)out->riff_size > file.size - 8u || out->riff_size < 12u) {
			errno = EINVAL;
			return -1;
		}
		pos = 12, end = 8u + (size_t)out->riff_size;
	} else {
		if (x.vp8x_flags & 0x02u) {
			errno = ENOTSUP;
			return -1;
		}
		pos = 30, end = 8u + (size_t)x.riff_size;
	}
	for (;;) {
		if (end - pos < 8u) {
			errno = EINVAL;
			return -1;
		}
		const uint8_t* chunk = file.data + pos;
		const uint32_t csize = rd_le32(chunk + 4);
		if (csize > 0xFFFFFFF6u || (size_t)csize > end - pos - 8u) {
			errno = EINVAL;
			return -1;
		}
		if (memcmp(chunk, "ANIM", 4) == 0 || memcmp(chunk, "ANMF", 4) == 0) {
			errno = ENOTSUP;
			return -1;
		}
		if (memcmp(chunk, "VP8L", 4) == 0) {
			out->vp8l_chunk_offset = pos + 8u, out->vp8l_chunk_size = csize;
			break;
		}
		if (!x.extended || memcmp(chunk, "VP8 ", 4) == 0) { /* (unreachable after webp_parse_extended's verdict) */
			errno = EINVAL;
			return -1;
		}
		const size_t padded = (size_t)csize + (csize & 1u);
		if (padded > end - pos - 8u) {
			errno = EINVAL;
			return -1;
		}
		pos += 8u + padded;
	}
	uint32_t w, h, hint;
	if (vp8f_lossless_header(file.data + out->vp8l_chunk_offset, out->vp8l_chunk_size, &w, &h, &hint) != 0) return -1;
	if (x.extended && (w != out->canvas_width || h != out->canvas_height)) {
		errno = EINVAL;
		return -1;
	}
	if (!x.extended) out->canvas_width = w, out->canvas_height = h;
	return 0;
}

static uint32_t rd_le24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

/* The sub-chunks of one frame from *pos on, in a RIFF payload that ends at `end`, as libwebp's demuxer walks them: an
 * optional ALPH, then 'VP8 ' or 'VP8L'; the walk stops in front of the first chunk that is neither (or a second of
 * either kind) and leaves *pos there.  1 = a frame, 0 = nothing it recognises came first (libwebp drops such a frame
 * without a word), -1 = refused. */
static int anim_frame_chunks(const uint8_t* data, size_t* at, size_t end, WebPAnimFrame* f) {
	uint32_t bw = 0, bh = 0, hint = 0;
	size_t pos = *at;
	for (;;) {
		if (end - pos < 8u) return -1; /* (a frame's walk needs a chunk header to look at, and one after each chunk it took) */
		const uint8_t* chunk = data + pos;
		const uint32_t csize = rd_le32(chunk + 4);
		if (csize > 0xFFFFFFF6u) return -1;
		const size_t padded = (size_t)csize + (csize & 1u);
		if (padded > end - pos - 8u) return -1;
		const int is_vp8 = memcmp(chunk, "VP8 ", 4) == 0, is_vp8l = memcmp(chunk, "VP8L", 4) == 0;
		if (memcmp(chunk, "ALPH", 4) == 0) {
			if (f->alph_offset) break;
			f->alph_offset = pos + 8u, f->alph_size = csize;
		} else if (is_vp8 || is_vp8l) {
			if (is_vp8l && f->alph_offset) return -1;
			if (f->vp8_offset || f->vp8l_offset) break;
			if (is_vp8) {
				Vp8KeyFrameHeader kf;
				ByteSpan payload = {chunk + 8, csize};
				if (vp8_parse_keyframe_header(payload, &kf) != 0) return -1;
				bw = kf.width, bh = kf.height;
				f->vp8_offset = pos + 8u, f->vp8_size = csize;
			} else {
				if (vp8f_lossless_header(chunk + 8, csize, &bw, &bh, &hint) != 0) return -1;
				f->vp8l_offset = pos + 8u, f->vp8l_size = csize;
			}
			f->width = bw, f->height = bh; /* (the bitstream's size counts, whatever the ANMF header names: as in libwebp) */
		} else {
			break;
		}
		pos += 8u + padded;
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
	const uint32_t riff_size = rd_le32(file.data + 4);
	/* the RIFF payload must lie inside the file; bytes after it are ignored */
	if (riff_size < 22u || riff_size > 0xFFFFFFF6u || (size_t)riff_size > file.size - 8u) return -1; /* (a VP8X chunk at the least) */
	const size_t end = 8u + (size_t)riff_size;
	if (memcmp(file.data + 12, "VP8X", 4) != 0) return -1; /* a still picture */
	const uint32_t xsize = rd_le32(file.data + 16);
	if (xsize < 10u || xsize > 0xFFFFFFF6u || (size_t)xsize + (xsize & 1u) > end - 20u) return -1;
	info->vp8x_flags = file.data[20];
	info->canvas_width = 1u + rd_le24(file.data + 24), info->canvas_height = 1u + rd_le24(file.data + 27);
	/* (libwebp's limit is the canvas area; this decoder's is the size of a tensor's picture) */
	if (info->canvas_width > 16383u || info->canvas_height > 16383u) return -1;
	if (!(info->vp8x_flags & 0x02u) || (info->vp8x_flags & ~0x3Eu)) return -1;
	size_t pos = 20u + (size_t)xsize + (xsize & 1u);
	uint32_t anims = 0, n = 0;
	while (pos != end) {
		if (end - pos < 8u) return -1;
		const uint8_t* chunk = file.data + pos;
		const uint32_t csize = rd_le32(chunk + 4);
		if (csize > 0xFFFFFFF6u) return -1;
		const size_t padded = (size_t)csize + (csize & 1u);
		if (padded > end - pos - 8u) return -1;
		if (memcmp(chunk, "VP8X", 4) == 0 || memcmp(chunk, "VP8 ", 4) == 0 || memcmp(chunk, "VP8L", 4) == 0 ||
		    memcmp(chunk, "ALPH", 4) == 0)
			return -1;
		if (memcmp(chunk, "ANIM", 4) == 0) {
			if (padded < 6u) return -1;
			if (anims++ == 0) info->bgcolor = rd_le32(chunk + 8), info->loop_count = (uint32_t)chunk[12] | (uint32_t)chunk[13] << 8;
		} else if (memcmp(chunk, "ANMF", 4) == 0) {
			if (anims == 0 || padded < 16u) return -1;
			WebPAnimFrame f;
			memset(&f, 0, sizeof(f));
			const uint8_t* p = chunk + 8;
			f.offset = pos + 8u, f.size = csize;
			f.x = 2u * rd_le24(p), f.y = 2u * rd_le24(p + 3), f.width = 1u + rd_le24(p + 6), f.height = 1u + rd_le24(p + 9);
			f.duration = rd_le24(p + 12);
			f.dispose = p[15] & 1u, f.blend = (p[15] & 2u) ? 0u : 1u;
			size_t at = pos + 24u;
			const int got = anim_frame_chunks(file.data, &at, end, &f);
			if (got < 0 || at > pos + 8u + padded) return -1; /* (a sub-chunk that runs past the ANMF's own end) */
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
		pos += 8u + padded;
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

int vp8f_decode_memory(const uint8_t* data, size_t size, Vp8KeyFrameHeader* kf, Vp8DecodedFrame* out, int* stage) {
	int st = 0;
	WebPContainer c;
	ByteSpan file = {data, size};
	int rc = -1;
	if (webp_parse_simple_lossy(file, &c) != 0) {
		st = 2;
		goto out;
	}
	ByteSpan payload = {data + c.vp8_chunk_offset, c.vp8_chunk_size};
	if (vp8_parse_keyframe_header(payload, kf) != 0 || !kf->is_key_frame) {
		st = 3;
		goto out;
	}
	if (vp8_decode_decoded_frame(payload, out) != 0) {
		st = 4;
		goto out;
	}
	rc = 0;
out:
	if (stage) *stage = st;
	return rc;
}

/* the VP8 payload of a file: the simple layout, or with VP8F_EXTENDED the extended one as well */
static int locate_payload(ByteSpan file, unsigned flags, WebPContainer* c) {
	if (!(flags & VP8F_EXTENDED)) return webp_parse_simple_lossy(file, c);
	WebPContainerX x;
	if (webp_parse_extended(file, &x) != 0) return -1;
	memset(c, 0, sizeof(*c));
	c->riff_size = x.riff_size, c->actual_size = x.actual_size;
	c->vp8_chunk_offset = x.vp8_chunk_offset, c->vp8_chunk_size = x.vp8_chunk_size;
	return 0;
}

int vp8f_decode_packed_memory(const uint8_t* data, size_t size, Vp8gPackedFrame* out, int* stage, unsigned flags) {
	int st = 0, rc = -1;
	WebPContainer c;
	ByteSpan file = {data, size};
	if (out) memset(out, 0, sizeof(*out));
	if (!out) {
		errno = EINVAL;
		st = 4;
	} else if (locate_payload(file, flags, &c) != 0) {
		st = 2;
	} else {
		ByteSpan payload = {data + c.vp8_chunk_offset, c.vp8_chunk_size};
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
	WebPContainer c;
	ByteSpan file = {data, size};
	if (!kf || !hdr || !tf || !payload_off || !payload_size) {
		errno = EINVAL;
		st = 4;
	} else if (locate_payload(file, flags, &c) != 0) {
		st = 2;
	} else if (c.vp8_chunk_size > 0xFFFFFFF0u) {
		errno = EFBIG;
		st = 4;
	} else {
		ByteSpan payload = {data + c.vp8_chunk_offset, c.vp8_chunk_size};
		if (vp8_parse_keyframe_header(payload, kf) != 0 || !kf->is_key_frame) {
			errno = EINVAL;
			st = 3;
		} else if (vp8f_token_header(payload, kf, hdr, tf, flags & ~VP8F_EXTENDED) != 0) {
			st = 4;
		} else {
			*payload_off = c.vp8_chunk_offset;
			*payload_size = (uint32_t)c.vp8_chunk_size;
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
