/*
 * container_verdicts_main.c -- what the four container parsers say about a file and its damaged copies, as a program
 * of its own linked against libvp8host.so (tests/test_container.py and tests/golden/make_container_verdicts.py run it).
 *
 *   container_verdicts hash  <list>    per file and parser one block on stdout: u32 byte count, then the records
 *   container_verdicts views <list>    (-DWITH_LOCATE) webp_locate_still against the three still parsers; exit 1 and
 *                                      one line per difference on stderr
 *
 * <list> holds one "<seed> <path>" per line.  The cases of a file, in order: whole; cut at every length up to 2048;
 * cut at 64 evenly spaced lengths beyond 2048; 512 copies with one byte changed each (splitmix64 from the seed; every
 * other change falls in the first 64 bytes).  A record: i32 return value, then i32 errno if refused, else every
 * field of the out struct as u64 -- for webp_parse_anim the count-only call and, where that succeeds, the call with
 * exactly nframes of room and its frame records.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../webp-decoder_amd/host/vp8_front.h"

enum { kParsers = 4, kCutAll = 2048, kCutSpaced = 64, kChanges = 512, kHead = 64 };

typedef struct {
	uint8_t* p;
	size_t n, cap;
} Buf;
static Buf blocks[kParsers];
static unsigned differences;
static const char* path;

static void put(Buf* b, const void* src, size_t n) {
	if (b->n + n > b->cap) {
		b->cap = (b->n + n) * 2;
		b->p = (uint8_t*)realloc(b->p, b->cap);
		if (!b->p) exit(3);
	}
	memcpy(b->p + b->n, src, n);
	b->n += n;
}
static void put_i32(Buf* b, int32_t v) { put(b, &v, 4); }
/* the head of a record, from a call made with errno cleared; 1 = accepted, the fields follow */
static int verdict(Buf* b, int rc) {
	const int e = errno;
	put_i32(b, rc);
	if (rc != 0) put_i32(b, e);
	return rc == 0;
}

static void hash_case(ByteSpan s, size_t case_no) {
	(void)case_no;
	WebPContainer c;
	WebPContainerX x;
	WebPContainerL l;
	WebPAnimInfo info;
	int rc;
	errno = 0;
	rc = webp_parse_simple_lossy(s, &c);
	if (verdict(&blocks[0], rc)) {
		const uint64_t v[] = {c.riff_size, c.actual_size, c.vp8_chunk_offset, c.vp8_chunk_size};
		put(&blocks[0], v, sizeof(v));
	}
	errno = 0;
	rc = webp_parse_extended(s, &x);
	if (verdict(&blocks[1], rc)) {
		const uint64_t v[] = {x.riff_size, x.actual_size, x.vp8_chunk_offset, x.vp8_chunk_size, x.alph_chunk_offset,
		                      x.alph_chunk_size, x.extended, x.vp8x_flags, x.canvas_width, x.canvas_height};
		put(&blocks[1], v, sizeof(v));
	}
	errno = 0;
	rc = webp_parse_any(s, &l);
	if (verdict(&blocks[2], rc)) {
		const uint64_t v[] = {l.riff_size, l.actual_size, l.vp8_chunk_offset, l.vp8_chunk_size, l.alph_chunk_offset, l.alph_chunk_size,
		                      l.extended, l.vp8x_flags, l.canvas_width, l.canvas_height, l.vp8l_chunk_offset, l.vp8l_chunk_size};
		put(&blocks[2], v, sizeof(v));
	}
	Buf* b = &blocks[3];
	for (int pass = 0; pass < 2; pass++) {
		WebPAnimFrame* fr = pass ? (WebPAnimFrame*)calloc(info.nframes, sizeof(WebPAnimFrame)) : NULL;
		const uint32_t room = pass ? info.nframes : 0;
		if (pass && !fr) exit(3);
		errno = 0;
		rc = webp_parse_anim(s, &info, fr, room);
		const int ok = verdict(b, rc);
		if (ok) {
			const uint64_t v[] = {info.canvas_width, info.canvas_height, info.bgcolor, info.loop_count, info.nframes, info.vp8x_flags};
			put(b, v, sizeof(v));
		}
		for (uint32_t k = 0; ok && k < room; k++) {
			const WebPAnimFrame* f = &fr[k];
			const uint64_t v[] = {f->offset, f->alph_offset, f->vp8_offset, f->vp8l_offset, f->size, f->alph_size, f->vp8_size, f->vp8l_size,
			                      f->x, f->y, f->width, f->height, f->duration, f->blend, f->dispose, f->has_alpha};
			put(b, v, sizeof(v));
		}
		free(fr);
		if (!ok) break;
	}
}

#ifdef WITH_LOCATE
static void differ(const char* what, unsigned accept, size_t case_no) {
	if (differences++ < 50) fprintf(stderr, "%s: case %zu, accept %u: %s differs\n", path, case_no, accept, what);
}
/* the record against a parser's verdict and fields (a = alph, l = vp8l: 0 where the parser's struct has none) */
static void view(ByteSpan s, unsigned accept, size_t case_no, int rc, int e, size_t vp8, uint32_t vp8n, size_t a, uint32_t an, size_t l,
                 uint32_t ln, uint32_t riff, uint32_t ext, uint32_t flags, int has_size, uint32_t w, uint32_t h) {
	WebPStill st;
	errno = 0;
	const int got = webp_locate_still(s, accept, &st);
	const int ge = errno;
	if (got != rc || (rc != 0 && ge != e)) differ("the verdict", accept, case_no);
	if (got != 0 || rc != 0) return;
	if (st.data != s.data || st.size != s.size) differ("the span", accept, case_no);
	if (st.vp8_offset != vp8 || st.vp8_size != vp8n) differ("VP8", accept, case_no);
	if (st.alph_offset != a || st.alph_size != an) differ("ALPH", accept, case_no);
	if (st.vp8l_offset != l || st.vp8l_size != ln) differ("VP8L", accept, case_no);
	if (st.riff_size != riff || st.extended != ext || st.vp8x_flags != flags) differ("the header", accept, case_no);
	if (has_size && (st.width != w || st.height != h)) differ("the size", accept, case_no);
}
static void views_case(ByteSpan s, size_t case_no) {
	WebPContainer c;
	WebPContainerX x;
	WebPContainerL l;
	errno = 0;
	int rc = webp_parse_simple_lossy(s, &c);
	int e = errno;
	view(s, 0, case_no, rc, e, c.vp8_chunk_offset, c.vp8_chunk_size, 0, 0, 0, 0, c.riff_size, 0, 0, 0, 0, 0);
	errno = 0;
	rc = webp_parse_extended(s, &x);
	e = errno;
	view(s, WEBP_ACCEPT_EXTENDED, case_no, rc, e, x.vp8_chunk_offset, x.vp8_chunk_size, x.alph_chunk_offset, x.alph_chunk_size, 0, 0,
	     x.riff_size, x.extended, x.vp8x_flags, x.extended != 0, x.canvas_width, x.canvas_height);
	errno = 0;
	rc = webp_parse_any(s, &l);
	e = errno;
	view(s, WEBP_ACCEPT_EXTENDED | WEBP_ACCEPT_LOSSLESS, case_no, rc, e, l.vp8_chunk_offset, l.vp8_chunk_size, l.alph_chunk_offset,
	     l.alph_chunk_size, l.vp8l_chunk_offset, l.vp8l_chunk_size, l.riff_size, l.extended, l.vp8x_flags,
	     l.extended || l.vp8l_chunk_offset, l.canvas_width, l.canvas_height);
	/* where the parsers' structs name no size (a simple lossy file) the record has the frame header's, or 0 x 0 */
	WebPStill st;
	Vp8KeyFrameHeader kf;
	if (webp_locate_still(s, WEBP_ACCEPT_EXTENDED, &st) == 0 && !st.extended) {
		const ByteSpan payload = {s.data + st.vp8_offset, st.vp8_size};
		const int parsed = vp8_parse_keyframe_header(payload, &kf) == 0;
		if (st.width != (parsed ? kf.width : 0u) || st.height != (parsed ? kf.height : 0u)) differ("the frame size", WEBP_ACCEPT_EXTENDED, case_no);
	}
}
#endif

static uint64_t rng_state;
static uint32_t rng(void) { /* splitmix64 */
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void every_case(uint8_t* data, size_t n, uint64_t seed, void (*fn)(ByteSpan, size_t)) {
	size_t case_no = 0;
	ByteSpan s = {data, n};
	fn(s, case_no++);
	for (s.size = 0; s.size < n && s.size <= kCutAll; s.size++) fn(s, case_no++);
	for (size_t k = 1; k <= kCutSpaced && n > kCutAll + 1u; k++) {
		s.size = kCutAll + (n - kCutAll) * k / (kCutSpaced + 1u);
		fn(s, case_no++);
	}
	s.size = n;
	rng_state = seed;
	for (int k = 0; k < kChanges && n; k++) {
		const size_t at = rng() % ((k & 1) && n > kHead ? kHead : n);
		const uint8_t old = data[at];
		data[at] ^= (uint8_t)(1u + rng() % 255u);
		fn(s, case_no++);
		data[at] = old;
	}
}

int main(int argc, char** argv) {
	const int views = argc == 3 && strcmp(argv[1], "views") == 0;
	if (argc != 3 || (!views && strcmp(argv[1], "hash") != 0)) return 2;
#ifndef WITH_LOCATE
	if (views) return 2;
#endif
	FILE* list = fopen(argv[2], "r");
	if (!list) return 2;
	static char line[4096];
	while (fgets(line, sizeof(line), list)) {
		char* end;
		const uint64_t seed = strtoull(line, &end, 10);
		line[strcspn(line, "\n")] = 0;
		path = end + 1;
		FILE* f = fopen(path, "rb");
		if (!f) return 2;
		uint8_t* data = (uint8_t*)malloc(1 << 20);
		if (!data) return 3;
		const size_t n = fread(data, 1, 1 << 20, f);
		fclose(f);
		if (!views) {
			every_case(data, n, seed, hash_case);
			for (int p = 0; p < kParsers; p++) {
				const uint32_t bytes = (uint32_t)blocks[p].n;
				fwrite(&bytes, 4, 1, stdout);
				fwrite(blocks[p].p, 1, blocks[p].n, stdout);
				blocks[p].n = 0;
			}
		}
#ifdef WITH_LOCATE
		else every_case(data, n, seed, views_case);
#endif
		free(data);
	}
	fclose(list);
	return differences ? 1 : 0;
}
