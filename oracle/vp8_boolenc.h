/*
 * vp8_boolenc.h -- TEST INFRASTRUCTURE: the RFC 6386 7.3 boolean entropy encoder shared by the
 * stream generators (vp8_repartition.c, vp8_stream_writer.c).  Never linked into the product.
 */
#ifndef VP8_BOOLENC_H
#define VP8_BOOLENC_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
	uint8_t* buf;
	size_t n, cap;
	uint32_t range, low; /* low: the bottom of the interval, 24 pending bits + carry position */
	int shifts_left;     /* normalisation shifts until the next byte leaves `low` */
	int oom;
} BoolEnc;

static inline void enc_init(BoolEnc* e) {
	memset(e, 0, sizeof(*e));
	e->range = 255;
	e->shifts_left = 24;
}

static inline void enc_byte(BoolEnc* e, uint8_t v) {
	if (e->n == e->cap) {
		size_t nc = e->cap ? 2 * e->cap : 4096;
		uint8_t* nb = (uint8_t*)realloc(e->buf, nc);
		if (!nb) {
			e->oom = 1;
			return;
		}
		e->buf = nb, e->cap = nc;
	}
	e->buf[e->n++] = v;
}

/* a carry out of `low` ripples into the bytes already written */
static inline void enc_carry(BoolEnc* e) {
	size_t i = e->n;
	while (i > 0 && e->buf[i - 1] == 0xFF) e->buf[--i] = 0;
	if (i > 0) e->buf[i - 1]++;
}

static inline void enc_bool(BoolEnc* e, uint32_t prob, int bit) {
	const uint32_t split = 1u + (((e->range - 1u) * prob) >> 8);
	if (bit) {
		e->low += split;
		e->range -= split;
	} else {
		e->range = split;
	}
	while (e->range < 128u) {
		e->range <<= 1;
		if (e->low & 0x80000000u) enc_carry(e);
		e->low <<= 1;
		if (--e->shifts_left == 0) {
			enc_byte(e, (uint8_t)(e->low >> 24));
			e->low &= 0xFFFFFFu;
			e->shifts_left = 8;
		}
	}
}

static inline void enc_finish(BoolEnc* e) {
	uint32_t v = e->low;
	int c = e->shifts_left;
	if (v & (1u << (32 - c))) enc_carry(e);
	v <<= c & 7;
	for (c >>= 3; c > 0; c--) v <<= 8;
	for (int i = 0; i < 4; i++, v <<= 8) enc_byte(e, (uint8_t)(v >> 24));
}

static inline void put_le(uint8_t* p, uint32_t v, int n) {
	for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

#endif
