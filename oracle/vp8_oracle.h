/*
 * vp8_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference hot path (src/m06_recon/vp8_recon.c + src/m07_loopfilter/
 * vp8_loopfilter.c) and of the next stage, m08/m09 (YUV->RGB, PPM/PNG writers), used as the parity checker by tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py.  The product path (libvp8g.so) never links or calls it.
 *
 * Pinned by: tests/golden/manifest.json (sha256 of the reference decoder's own -yuv/-yuvf output
 * on every corpus file, generated from the reference compiled here, cross-checked with libwebp
 * 1.2.2) and tests/golden/synth_kat.json (reference m06/m07 output hashes on seeded synthetic
 * frames) -- see tests/test_oracle.py.
 */
#ifndef VP8_ORACLE_H
#define VP8_ORACLE_H

#include "../include/vp8g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Padded (macroblock-aligned) reconstruction, optionally loop-filtered, into caller planes of
 * size (mb_cols*16) x (mb_rows*16) and (mb_cols*8) x (mb_rows*8). */
int oracle_recon_padded(const Vp8DecodedFrame* d, uint8_t* y, uint8_t* u, uint8_t* v, int filtered);

/* m07 alone, in place on a padded image (stride = width). */
int oracle_loopfilter(uint8_t* y, uint8_t* u, uint8_t* v, const Vp8DecodedFrame* d);

/* What oracle_loopfilter does on these planes (copies are filtered): edge positions visited, added
 * into counts[kind][cell]; kind 0 simple, 1 normal MB edge, 2 normal sub-block edge; cell 0 mask
 * fail, 1 mask pass with hev, 2 mask pass without hev (the simple filter uses cells 0 and 2). */
int oracle_loopfilter_census(const uint8_t* y, const uint8_t* u, const uint8_t* v, const Vp8DecodedFrame* d,
                             uint64_t counts[3][3]);

/* The same walk, counting where the filter arithmetic reaches its clamps, added into
 * counts[path][cell].  Paths: 0 simple, 1 normal MB edge with hev, 2 normal MB edge without hev (the
 * MB adjust), 3 normal sub-block edge with hev, 4 normal sub-block edge without hev.  Cell 0 is the
 * number of filtered positions of the path.  Common adjust (paths 0, 1, 3, 4): 1/2 p1-q1 above 127 /
 * below -128 (not path 4, which has no such term), 3/4 raw a above 127 / below -128, 5 clamped a in
 * 124..127, 6/7 sat8 changes q0 - f1 (low / high), 8/9 sat8 changes p0 + f2, 10/11 sat8 changes
 * p1 + a2 or q1 - a2 (path 4 only).  MB adjust (path 2): 1/2 raw w above 127 / below -128, 3/4 sat8
 * changes a p1/q1 tap (low / high), 5/6 a p2/q2 tap, 7/8 p1-q1 above 127 / below -128, 9/10 sat8
 * changes a p0/q0 tap. */
#define OR_AR_PATHS 5
#define OR_AR_CELLS 12
int oracle_loopfilter_arith_census(const uint8_t* y, const uint8_t* u, const uint8_t* v, const Vp8DecodedFrame* d,
                                   uint64_t counts[OR_AR_PATHS][OR_AR_CELLS]);

/* Full m06(+m07) with crop into a malloc()ed cropped I420 image (free with oracle_image_free). */
int oracle_reconstruct(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* d, Yuv420Image* out, int filtered);
void oracle_image_free(Yuv420Image* img);

/* Cropped I420 bytes written back to back (Y, U, V), as `decoder -yuv/-yuvf` writes them.
 * buf must hold w*h + 2*ceil(w/2)*ceil(h/2) bytes. */
int oracle_reconstruct_i420(const Vp8KeyFrameHeader* kf, const Vp8DecodedFrame* d, uint8_t* buf, int filtered);

/* CPU baseline: reconstruct `n` frames (frames[i % nframes]) with `threads` pthreads, one frame
 * per task; returns elapsed seconds (wall), or < 0 on error. */
double oracle_time_batch(const Vp8KeyFrameHeader* const* kfs, const Vp8DecodedFrame* const* frames, int nframes, int n,
                         int threads, int filtered);

/* m08 / m09 (reference src/m08_yuv2rgb_ppm/yuv2rgb_ppm.c, src/m09_png/yuv2rgb_png.c): one RGB24
 * row of the fancy-upsampled conversion, and the complete PPM / PNG files the reference's
 * yuv420_write_ppm_fd / yuv420_write_png_fd emit, written to memory (byte count, or -1). */
void oracle_rgb_row(const Yuv420Image* img, uint32_t y, uint8_t* dst);
size_t oracle_ppm_size(uint32_t w, uint32_t h);
size_t oracle_png_size(uint32_t w, uint32_t h);
long oracle_ppm(const Yuv420Image* img, uint8_t* out, size_t cap);
long oracle_png(const Yuv420Image* img, uint8_t* out, size_t cap);

#ifdef __cplusplus
}
#endif

#endif
