"""Directed frames: inputs that select the data-dependent paths of the kernels which seeded random
frames (webp-decoder_amd/host/vp8_synth.c, profiles 0/1/2) never produce.

A frame starts as vp8g.synth_frame(...) and is rewritten in place through Frame.array(name) and the
Vp8DecodedFrame fields; every draw comes from numpy.random.default_rng(seed).  build(kind, w, h, seed)
is the one entry; KINDS lists every kind.  tests/test_directed.py proves from the arrays (and from
the oracle's loop-filter census) that each kind is what it says.

What the kernels choose by data (csrc/vp8g_kernels.hip frame kernel, csrc/vp8g_quad.inc quad chain):
  * the inverse DCT has three forms -- DC only, "columns 2-3 zero", full -- chosen per WAVE by a ballot
    over the dequantised coefficients of 1 MB (frame kernel) or 4 vertically adjacent MBs (quad
    chain), in the quad chain separately for the luma and the chroma role;
  * the inverse WHT is skipped when no MB of the wave has a Y2 block (all B_PRED);
  * the loop filter leaves out an MB's inner edges when has_coeff == 0 and the MB is not B_PRED,
    keyed on the has_coeff byte alone (reference src/m07_loopfilter/vp8_loopfilter.c:226).

Coefficient shapes of one MB and role (luma = the 16 Y blocks, chroma = the 4 U + 4 V blocks;
coeff_y[.][0] of a non-B_PRED MB stays the garbage profiles 1/2 put there: it must be ignored):
  dc      every AC position zero (Y2 stays as generated, so the WHT feeds the luma DCs)
  cols01  natural positions with (i & 3) >= 2 zero; at least one AC left in columns 0-1 (planted if
          the generator left none)
  full    as generated

Kinds (base profile 1, or 2 for an odd seed: full-range coefficients, every mode):
  uni_<luma>_<chroma>   nine uniform frames: every wave of every kernel takes that form per role,
                        whatever its geometry
  mixed                 shape drawn per MB and role, i.i.d. with MIX_WEIGHTS = dc .55 / cols01 .25 /
                        full .20.  A wave takes the richest shape among its MBs, so over k
                        independent MBs P(dc form) = .55^k, P(cols01 form) = .80^k - .55^k,
                        P(full form) = 1 - .80^k:
                          k = 1 (frame kernel)  55.0 % / 25.0 % / 20.0 %
                          k = 4 (quad chain)     9.2 % / 31.8 % / 59.0 %
                        -- every form >= 5 % per role, and the form changes from step to step
  spoil_<dc|cols01>_<luma|chroma>
                        a uniform dc (or cols01) frame with the generated coefficients put back in
                        ONE block of every k-th MB, k coprime to mb_cols (so the spoiled MBs walk
                        through the columns and the row residues), in a luma block only or in a
                        chroma block only: a lone lane must lift its own role's form and leave the
                        other role's alone.  The spoiling block has an AC in columns 2-3 (planted if
                        the generated block had none).
  wrap                  a uniform dc frame with DCs of +-2114 (Y2 DC, the Y DCs of B_PRED MBs, U/V
                        DCs), q_index 127, DC deltas +15, no segments: 2114 * 314, * 157, * 132 wrap
                        int16 in the packed dequantisation multiply
  bpred_all, bpred_none the whole frame with / without Y2 (no wave / every wave runs the WHT)
Kinds on base profile 0 (small coefficients, smooth output: the loop filter fires):
  skip                  a seeded ~40 % of MBs with Y2/Y/U/V all zero, has_coeff 0, skip_coeff 1;
                        B_PRED and non-B_PRED MBs both among them (no inner edges vs inner edges)
  lie_hasc0             has_coeff = 0 on a seeded half of the MBs that do have coefficients
  lie_hasc1             the skip subset zeroed, but has_coeff = 1 on it
  lf00 .. lf15          the loop-filter header overwritten from LF_CASES (below), skip on top
  sat_mb .. sat_chroma  painted frames (see _paint, _tile): the unfiltered picture is chosen block by
                        block and the coefficients follow, at q_index 4 where every step is exact; the
                        normal filter at levels 57..63 meets steps and patterns that take its arithmetic
                        into the clamps (tests/test_directed.py counts them with the oracle's
                        arithmetic census):
                          sat_mb      flat DC_PRED MBs 56..84 apart: w = 2d beyond +-127 on MB edges
                          sat_sub     flat B_PRED sub-blocks 36..80 apart: a = 3d beyond +-127
                          sat_hev     +-k patterns beside steps: hev with p1 - q1 and a beyond +-127
                          sat_ends    the same at 0 and 255: every tap that can leave 0..255 does
                          sat_sharp   sharpness 3 (interior limit 6): sub-blocks 38..58 apart, MBs, ends
                          sat_seg     absolute segment levels 63 57 48 30, on both sides of 52 (below
                                      it flat MBs that pass the mask cannot saturate w); mb, sub, hev
                          sat_chroma  every design in the chroma planes, luma flat
                        chroma carries the kind's designs too (8x8 MBs of 4x4 blocks)
In every kind but the two lies has_coeff / skip_coeff are recomputed from the coefficients.

LF_CASES: simple / normal filter x sharpness 0..7 (case i: simple = i & 1, sharpness = i >> 1), and
per case (frame level, segmentation, abs, segment levels, deltas, ref delta 0, mode delta 0): frame
levels 0..63, segments on / off, absolute / relative, segments of level 0 beside filtered ones,
lf_mode_delta[0] that takes B_PRED MBs to level 0 and ones that do not, per-MB levels on both sides
of 15 and of 40 (the hev thresholds).

smooth_planes(w, h, seed): padded planes for vp8_loopfilter_apply_keyframe -- a seeded random walk
(steps of a few units, occasional jumps) instead of uniform noise, on which the normal filter's mask
fails at ~95 % of the positions.
step_planes(w, h, seed): padded planes painted from the sat_* designs, for the same entry point under
LF_STEP_CASES (simple and normal filter, levels 57..63, sharpness 0 and > 0).
"""
import math
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
import vp8g  # noqa: E402

SHAPES = ("dc", "cols01", "full")
MIX_WEIGHTS = (0.55, 0.25, 0.20)
UNIFORM = [f"uni_{a}_{b}" for a in SHAPES for b in SHAPES]
SPOILERS = [f"spoil_{s}_{r}" for s in ("dc", "cols01") for r in ("luma", "chroma")]
LF_KINDS = [f"lf{i:02d}" for i in range(16)]
# (appended: build() seeds from KINDS.index(kind), so the kinds before them keep their frames)
SAT_KINDS = ["sat_mb", "sat_sub", "sat_hev", "sat_ends", "sat_sharp", "sat_seg", "sat_chroma"]
KINDS = (UNIFORM + ["mixed"] + SPOILERS + ["wrap", "bpred_all", "bpred_none", "skip", "lie_hasc0", "lie_hasc1"] + LF_KINDS
         + SAT_KINDS)

# (frame level, segmentation_enabled, segmentation_abs, seg_lf_level[4], lf_delta_enabled, lf_ref_delta[0],
#  lf_mode_delta[0]); per-MB levels (non-B_PRED / B_PRED where they differ) in the comments
LF_CASES = [
    (31, 1, 0, (-23, -26, -8, 0), 0, 0, 0),      # 8 5 23 31 (profile 0's own levels)
    (20, 1, 1, (0, 10, 30, 50), 0, 0, 0),        # 0 10 30 50: a level-0 segment
    (12, 0, 0, (0, 0, 0, 0), 1, 4, -63),         # 16 / B_PRED 0
    (63, 0, 0, (0, 0, 0, 0), 0, 0, 0),           # 63
    (45, 1, 0, (-45, -35, -10, 10), 0, 0, 0),    # 0 10 35 55: a level-0 segment
    (30, 1, 1, (14, 15, 39, 40), 1, 0, 5),       # 14 15 39 40 / B_PRED 19 20 44 45
    (50, 0, 0, (0, 0, 0, 0), 1, -12, -20),       # 38 / B_PRED 18
    (0, 1, 1, (0, 0, 25, 42), 0, 0, 0),          # 0 0 25 42: frame level 0, level-0 segments
    (40, 1, 0, (0, -25, -40, 23), 1, 0, -63),    # 40 15 0 63 / B_PRED 0: a level-0 segment
    (13, 0, 0, (0, 0, 0, 0), 1, 2, 30),          # 15 / B_PRED 45
    (5, 1, 1, (3, 0, 63, 20), 0, 0, 0),          # 3 0 63 20: a level-0 segment
    (33, 1, 0, (-63, 5, 10, -20), 1, 2, -3),     # 2 40 45 15 / B_PRED 0 37 42 12
    (60, 1, 1, (60, 41, 16, 0), 1, -1, -15),     # 59 40 15 0 / B_PRED 44 25 0 0: a level-0 segment
    (24, 0, 0, (0, 0, 0, 0), 0, 0, 0),           # 24
    (14, 1, 0, (0, 1, 25, 26), 0, 0, 0),         # 14 15 39 40: both sides of both hev thresholds
    (36, 0, 0, (0, 0, 0, 0), 1, 4, -63),         # 40 / B_PRED 0
]

_C23 = np.flatnonzero((np.arange(16) & 3) >= 2)  # natural positions in columns 2-3
_C01_AC = np.array([1, 4, 5, 8, 9, 12, 13])      # AC positions in columns 0-1


def _coeffs(f):
    n = f.mb_total
    return (f.array("coeff_y").reshape(n, 16, 16), f.array("coeff_u").reshape(n, 4, 16),
            f.array("coeff_v").reshape(n, 4, 16), f.array("coeff_y2").reshape(n, 16))


def mb_classes(f):
    """Per MB the class of the luma and of the chroma role, read from the arrays alone: 0 = dc (no
    AC anywhere), 1 = cols01 (an AC, none in columns 2-3), 2 = full.  int arrays (luma, chroma)."""
    cy, cu, cv, _ = _coeffs(f)
    out = []
    for blocks in (cy, np.concatenate([cu, cv], axis=1)):
        c23 = (blocks[:, :, _C23] != 0).any(axis=(1, 2))
        ac = (blocks[:, :, 1:] != 0).any(axis=(1, 2))
        out.append(np.where(c23, 2, np.where(ac, 1, 0)))
    return out


def coded(f):
    """Per MB: does it carry a coefficient the decoder would have read (Y2 only without B_PRED, the
    Y DCs only with it)?  What has_coeff is when it tells the truth."""
    cy, cu, cv, y2 = _coeffs(f)
    bp = f.array("ymode") == 4
    return ((cy[:, :, 1:] != 0).any(axis=(1, 2)) | (cu != 0).any(axis=(1, 2)) | (cv != 0).any(axis=(1, 2))
            | np.where(bp, (cy[:, :, 0] != 0).any(axis=1), (y2 != 0).any(axis=1)))


def _shape(rng, blocks, shape):
    """Shape the [mb][block][16] view `blocks` (one role) in place: shape[mb] in 0 dc / 1 cols01 / 2 full."""
    blocks[shape == 0, :, 1:] = 0
    for m in np.flatnonzero(shape == 1):
        blocks[m][:, _C23] = 0
        if not (blocks[m][:, _C01_AC] != 0).any():
            blocks[m, rng.integers(blocks.shape[1]), _C01_AC[rng.integers(len(_C01_AC))]] = (1 + 2 * rng.integers(35)) * (1 - 2 * rng.integers(2))


def _shape_frame(rng, f, luma, chroma):
    cy, cu, cv, _ = _coeffs(f)
    _shape(rng, cy, luma)
    uv = np.concatenate([cu, cv], axis=1)
    _shape(rng, uv, chroma)
    cu[:], cv[:] = uv[:, :4], uv[:, 4:]


def _truth(f):
    has = coded(f)
    f.array("has_coeff")[:] = has
    f.array("skip_coeff")[:] = ~has


def _subset(rng, f, p):
    """A seeded subset of the MBs (each with probability p) that holds a B_PRED and a non-B_PRED MB
    whenever the frame has both."""
    sel = rng.random(f.mb_total) < p
    bp = f.array("ymode") == 4
    for cls in (bp, ~bp):
        if cls.any() and not (sel & cls).any():
            sel[np.flatnonzero(cls)[0]] = True
    return sel


def _zero_mbs(f, sel):
    for a in _coeffs(f):
        a[sel] = 0


def spoil_step(mb_cols):
    """The smallest k >= 3 coprime to mb_cols."""
    k = 3
    while math.gcd(k, mb_cols) != 1:
        k += 1
    return k


def _lf_header(f, case):
    lvl, seg, sabs, segl, den, rd, md = LF_CASES[case]
    h = f.frame
    h.lf_use_simple, h.lf_sharpness, h.lf_level = case & 1, case >> 1, lvl
    h.segmentation_enabled, h.segmentation_abs = seg, sabs
    for i in range(4):
        h.seg_lf_level[i] = segl[i]
        if sabs:  # (absolute segments carry absolute quantiser indices too: keep profile 0's 34..52)
            h.seg_quant_idx[i] = 34 + 6 * i
        h.lf_ref_delta[i] = h.lf_mode_delta[i] = 0
    h.lf_delta_enabled, h.lf_ref_delta[0], h.lf_mode_delta[0] = den, rd, md


def mb_lf_levels(f):
    """Per-MB loop-filter level, restated from the frame header (RFC 6386 9.6 / 15.2)."""
    h = f.frame
    lvl = np.full(f.mb_total, int(h.lf_level))
    if h.segmentation_enabled:
        s = np.array([h.seg_lf_level[i] for i in range(4)])[f.array("segment_id") & 3]
        lvl = s if h.segmentation_abs else lvl + s
    lvl = np.clip(lvl, 0, 63)
    if h.lf_delta_enabled:
        lvl = np.clip(lvl + h.lf_ref_delta[0] + np.where(f.array("ymode") == 4, h.lf_mode_delta[0], 0), 0, 63)
    return lvl


# ---- painted frames: the unfiltered picture is chosen, the coefficients follow ----------------------
# At q_index 4 with no quantiser deltas every dequantisation factor is 8 (Y2 DC: 16), so a DC
# coefficient c moves a block by exactly c levels (Y2 DC 4c: the whole MB by c), and one AC coefficient
# k at natural position 1, 2, 3 (across) or 4, 8, 12 (down) adds a fixed zero-mean pattern, e.g.
# position 2: +k -k -k +k.  With DC prediction everywhere (B_DC_PRED sub-blocks, DC_PRED MBs and
# chroma) the reconstruction is clip(mean + pattern) per 4x4 block, whatever the neighbours are.

def _ac_pattern(K, P):
    """The residual [..., 4, 4] of blocks whose only coefficient is K (ints) at natural position P,
    dequantised by 8: the inverse DCT of RFC 6386 14.3 restated."""
    x = np.zeros(K.shape + (16,), np.int64)
    np.put_along_axis(x, P[..., None], 8 * K[..., None], axis=-1)
    x = x.reshape(K.shape + (4, 4))
    mc = lambda v: v + ((v * 20091) >> 16)  # noqa: E731
    ms = lambda v: (v * 35468) >> 16        # noqa: E731

    def half(v, rnd, sh):  # along the second-to-last axis
        a, b = v[..., 0, :] + v[..., 2, :], v[..., 0, :] - v[..., 2, :]
        c, d = ms(v[..., 1, :]) - mc(v[..., 3, :]), mc(v[..., 1, :]) + ms(v[..., 3, :])
        return np.stack([a + d + rnd, b + c + rnd, b - c + rnd, a - d + rnd], axis=-2) >> sh
    t = half(x, 0, 0)
    return np.swapaxes(half(np.swapaxes(t, -1, -2), 4, 3), -1, -2)


def _plan(M, K, P):
    """Pixels of a plane from per-block means, AC coefficients and their positions (grids of 4x4 blocks)."""
    px = np.clip(M[..., None, None] + _ac_pattern(K, P), 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(M.shape[0] * 4, M.shape[1] * 4)


def _dc_pred(px, n):
    """DC prediction of every n x n block of the plane from the plane itself (frame edges: 127 above,
    129 to the left; a 16 / 8 block uses only the edges that exist, a 4x4 sub-block always both)."""
    h, w = px.shape
    a = np.full((h + 1, w + 1), 129, np.int64)
    a[0, :] = 127
    a[1:, 1:] = px
    above = a[0:h:n, 1:].reshape(h // n, w // n, n).sum(-1)
    left = a[1:, 0:w:n].reshape(h // n, n, w // n).sum(1)
    if n == 4:
        return (above + left + 4) >> 3
    both = (above + left + n) >> (5 if n == 16 else 4)
    one = lambda s: (s + n // 2) >> (4 if n == 16 else 3)  # noqa: E731
    i, j = np.indices(both.shape)
    return np.where((i > 0) & (j > 0), both, np.where(i > 0, one(above), np.where(j > 0, one(left), 128)))


def _per_mb(grid, b):
    """A [rows * b, cols * b] grid of blocks as [mb][b * b], blocks in raster order within the MB."""
    r, c = grid.shape[0] // b, grid.shape[1] // b
    return grid.reshape(r, b, c, b).transpose(0, 2, 1, 3).reshape(r * c, b * b)


def _paint(f, bp, luma, chroma):
    """Rewrite f so that its unfiltered reconstruction is the painted picture: bp[mb_rows][mb_cols] says
    which MBs are B_PRED (the others DC_PRED with one mean per MB: their first block's), luma and
    chroma = (M, K, P) block grids as for _plan (chroma: one triple per plane)."""
    rows, cols = bp.shape
    cy, cu, cv, y2 = _coeffs(f)
    for a in (cy, cu, cv, y2):
        a[:] = 0
    f.array("ymode")[:] = np.where(bp, 4, 0).reshape(-1)
    f.array("bmode")[:] = 0
    f.array("uv_mode")[:] = 0
    M, K, P = luma
    bp4 = np.repeat(np.repeat(bp, 4, 0), 4, 1)
    M = np.where(bp4, M, np.repeat(np.repeat(M[::4, ::4], 4, 0), 4, 1))
    px = _plan(M, K, P)
    np.put_along_axis(cy, _per_mb(P, 4)[..., None], _per_mb(K, 4)[..., None].astype(np.int16), axis=2)
    cy[:, :, 0] = np.where(bp.reshape(-1, 1), _per_mb(M - _dc_pred(px, 4), 4), 0)
    y2[:, 0] = np.where(bp, 0, 4 * (M[::4, ::4] - _dc_pred(px, 16))).reshape(-1)
    for c, (M, K, P) in zip((cu, cv), chroma):
        np.put_along_axis(c, _per_mb(P, 2)[..., None], _per_mb(K, 2)[..., None].astype(np.int16), axis=2)
        c[:, :, 0] = _per_mb(M - np.repeat(np.repeat(_dc_pred(_plan(M, K, P), 8), 2, 0), 2, 1), 2)
    h = f.frame
    h.q_index = 4
    h.y1_dc_delta_q = h.y2_dc_delta_q = h.y2_ac_delta_q = h.uv_dc_delta_q = h.uv_ac_delta_q = 0


# What a 2 x 2 MB tile of a painted plane holds (bpm = blocks per MB side: 4 luma, 2 chroma).  The step
# ranges straddle what the filter admits at level 63, sharpness 0 (MB edge 2|p0-q0| + |p1-q1|/2 <= 193,
# sub-block edge <= 189) and what saturates (w = 2d > 127 from d = 64 between flat MBs, a = 3d > 127
# from d = 43 between flat sub-blocks):
#   mb        flat MBs in a checkerboard, neighbours 56..84 apart
#   sub       flat sub-blocks in a checkerboard, 36..80 apart (subsharp: 38..58, for interior limit <= 8)
#   hev       across (position 2) or down (position 8) the tile, blocks alternate between two levels
#             60..78 apart, either with +-k -+k -+k +-k patterns of alternating sign, k 24..31 (p1 - q1
#             beyond +-128 beside a small p0 - q0), or with one small k 2..6 (hev beside a step: a = 2d)
#   ends      at 0 or at 255: zig = 0 2k 2k 0 blocks between flat 0 ones (outer taps leave 0..255), tri =
#             2 0 0 2 between flat 0 ones (the inner p1/q1 tap and the MB adjust's p1/q1 tap leave the
#             range only from such triples), saw = 6 4 0 0 in every block (the MB adjust's p2/q2 tap),
#             fine = means within 5 of the end, any position, |k| <= 3
def _tile(rng, d, i, j, bpm):
    """(M, K, P, B_PRED) of one tile of design d; i, j = the global block indices of its blocks."""
    shp = i.shape
    K, P = np.zeros(shp, np.int64), np.ones(shp, np.int64)
    if d in ("mb", "sub", "subsharp"):
        unit = bpm if d == "mb" else 1
        lo, hi = {"mb": (28, 42), "sub": (18, 40), "subsharp": (19, 29)}[d]
        hu = rng.integers(lo, hi + 1, (2 * bpm, 2 * bpm))
        h = hu[(i - i[0, 0]) // unit, (j - j[0, 0]) // unit]
        s = 1 - 2 * ((i // unit + j // unit) & 1)
        return int(rng.integers(hi + 1, 255 - hi)) + s * h, K, P, d != "mb"
    across = int(rng.integers(2))  # the direction in which the blocks alternate (s = +-1), from a drawn phase
    s = 1 - 2 * (((j if across else i) + int(rng.integers(2))) & 1)
    if d == "hev":
        if rng.integers(2):
            K = -s * rng.integers(24, 32, shp)
            M = int(rng.integers(72, 184)) + s * rng.integers(30, 40, shp)
        else:
            K = np.full(shp, int(rng.integers(2, 7)) * (1 - 2 * int(rng.integers(2))))
            M = int(rng.integers(50, 206)) + s * rng.integers(28, 39, shp)
        return M, K, np.full(shp, 2 if across else 8), True
    assert d == "ends", d
    top, sub = int(rng.integers(2)), int(rng.integers(4))
    if sub == 0:    # zig
        k = rng.integers(20, 32, shp)
        M, K, P = np.where(s > 0, k, 0), np.where(s > 0, -k, 0), np.full(shp, 2 if across else 8)
    elif sub == 1:  # tri
        M, K, P = np.where(s > 0, 1, 0), np.where(s > 0, 1, 0), np.full(shp, 2 if across else 8)
    elif sub == 2:  # saw
        M, K, P = np.full(shp, int(rng.integers(1, 3))), np.full(shp, 3), np.full(shp, 1 if across else 4)
    else:           # fine
        M, K, P = rng.integers(-2, 6, shp), rng.integers(-3, 4, shp), rng.choice([1, 2, 3, 4, 8, 12], shp)
    return (255 - M, -K, P, True) if top else (M, K, P, True)


def _terrain(rng, designs, rows, cols, bpm):
    """Block grids (M, K, P) of a plane of rows x cols MBs and its per-MB B_PRED map, every 2 x 2 MB
    tile of a design drawn from `designs`."""
    ii, jj = np.indices((rows * bpm, cols * bpm))
    M, K, P = np.zeros_like(ii), np.zeros_like(ii), np.ones_like(ii)
    bp = np.zeros((rows, cols), bool)
    for ti in range(0, rows, 2):
        for tj in range(0, cols, 2):
            sl = (slice(ti * bpm, (ti + 2) * bpm), slice(tj * bpm, (tj + 2) * bpm))
            M[sl], K[sl], P[sl], bp[ti:ti + 2, tj:tj + 2] = _tile(rng, designs[rng.integers(len(designs))], ii[sl], jj[sl], bpm)
    return (M, K, P), bp


# kind -> (tile designs, loop-filter level, sharpness)
SAT_SPECS = {"sat_mb": (("mb",), 63, 0), "sat_sub": (("sub",), 63, 0), "sat_hev": (("hev",), 60, 0),
             "sat_ends": (("ends",), 63, 0), "sat_sharp": (("subsharp", "mb", "ends"), 63, 3),
             "sat_seg": (("mb", "sub", "hev"), 0, 0), "sat_chroma": (("mb", "sub", "hev", "ends"), 63, 0)}
SAT_SEG_LEVELS = (63, 57, 48, 30)  # sat_seg: absolute segment levels on both sides of what lets w saturate (52)


def _sat_frame(rng, f, kind):
    designs, level, sharp = SAT_SPECS[kind]
    rows, cols = int(f.frame.mb_rows), int(f.frame.mb_cols)
    luma, bp = _terrain(rng, designs, rows, cols, 4)
    if kind == "sat_chroma":  # luma left without coefficients
        luma, bp = (np.full_like(luma[0], 128), np.zeros_like(luma[1]), luma[2]), np.zeros_like(bp)
    _paint(f, bp, luma, [_terrain(rng, designs, rows, cols, 2)[0] for _ in range(2)])
    if kind == "sat_chroma":
        _coeffs(f)[3][:] = 0
    h = f.frame
    h.lf_use_simple, h.lf_sharpness, h.lf_level, h.lf_delta_enabled = 0, sharp, level, 0
    h.segmentation_enabled = h.segmentation_abs = int(kind == "sat_seg")
    for i in range(4):
        h.seg_lf_level[i], h.seg_quant_idx[i] = (SAT_SEG_LEVELS[i], 4) if kind == "sat_seg" else (0, 0)


def build(kind, width, height, seed):
    """The directed frame `kind` (one of KINDS) of width x height from `seed`: a vp8g.Frame."""
    rng = np.random.default_rng([KINDS.index(kind), width, height, seed])
    smooth = kind in ("skip", "lie_hasc0", "lie_hasc1") or kind in LF_KINDS + SAT_KINDS
    f = vp8g.synth_frame(width, height, seed, 0 if smooth else 1 + (seed & 1))
    n = f.mb_total
    if kind in UNIFORM:
        _, a, b = kind.split("_")
        _shape_frame(rng, f, np.full(n, SHAPES.index(a)), np.full(n, SHAPES.index(b)))
    elif kind == "mixed":
        _shape_frame(rng, f, rng.choice(3, n, p=MIX_WEIGHTS), rng.choice(3, n, p=MIX_WEIGHTS))
    elif kind in SPOILERS:
        _, s, role = kind.split("_")
        cy, cu, cv, _ = _coeffs(f)
        orig = (cy.copy(), np.concatenate([cu, cv], axis=1))
        _shape_frame(rng, f, np.full(n, SHAPES.index(s)), np.full(n, SHAPES.index(s)))
        for m in range(0, n, spoil_step(int(f.frame.mb_cols))):
            if role == "luma":
                b = int(rng.integers(16))
                cy[m, b, 1:] = orig[0][m, b, 1:]  # (position 0 was never touched)
                blk = cy[m, b]
            else:
                b = int(rng.integers(8))
                blk = (cu if b < 4 else cv)[m, b & 3]
                blk[:] = orig[1][m, b]
            if not (blk[_C23] != 0).any():
                blk[6] = (1 + 2 * rng.integers(35)) * (1 - 2 * rng.integers(2))
    elif kind == "wrap":
        _shape_frame(rng, f, np.zeros(n, int), np.zeros(n, int))
        cy, cu, cv, y2 = _coeffs(f)
        bp = f.array("ymode") == 4
        sign = lambda *s: (2114 * (1 - 2 * rng.integers(0, 2, s))).astype(np.int16)  # noqa: E731
        y2[~bp, 0] = sign(int((~bp).sum()))
        cy[bp, :, 0] = sign(int(bp.sum()), 16)
        cu[:, :, 0], cv[:, :, 0] = sign(n, 4), sign(n, 4)
        h = f.frame
        h.q_index, h.segmentation_enabled = 127, 0
        h.y1_dc_delta_q = h.y2_dc_delta_q = h.uv_dc_delta_q = 15
    elif kind == "bpred_all":
        f.array("ymode")[:] = 4
    elif kind == "bpred_none":
        ym, y2 = f.array("ymode"), _coeffs(f)[3]
        for m in np.flatnonzero(ym == 4):  # a Y2 block for the MBs that had none: sparse, full range
            ym[m] = rng.integers(4)
            v = np.where(rng.random(16) < 0.25, rng.integers(-2114, 2115, 16), rng.integers(-70, 71, 16))
            y2[m] = np.where(rng.random(16) < 0.4, v, 0)
    elif kind == "skip":
        _zero_mbs(f, _subset(rng, f, 0.4))
    elif kind == "lie_hasc0":
        _truth(f)
        f.array("has_coeff")[_subset(rng, f, 0.5) & coded(f)] = 0
        return f
    elif kind == "lie_hasc1":
        sel = _subset(rng, f, 0.4)
        _zero_mbs(f, sel)
        _truth(f)
        f.array("has_coeff")[sel] = 1
        return f
    elif kind in LF_KINDS:
        _lf_header(f, LF_KINDS.index(kind))
        _zero_mbs(f, _subset(rng, f, 0.25))
    elif kind in SAT_KINDS:
        _sat_frame(rng, f, kind)
    else:
        raise KeyError(kind)
    _truth(f)
    return f


def smooth_planes(width, height, seed):
    """Padded planes (y, u, v: uint8, width x height and half of each) that the loop filter modifies:
    per plane a row walk plus a column walk (steps -3..3, one in ~30 a jump of +-20..60) plus +-2 of
    noise, folded into 0..255 so the walk stays continuous at the range's ends."""
    rng = np.random.default_rng([0x5100, width, height, seed])
    out = []
    for w, h in ((width, height), (width // 2, height // 2), (width // 2, height // 2)):
        def walk(k):
            s = rng.integers(-3, 4, k)
            jump = rng.random(k) < 1 / 30
            s = np.where(jump, rng.integers(20, 61, k) * (1 - 2 * rng.integers(0, 2, k)), s)
            return np.cumsum(s)
        a = int(rng.integers(60, 200)) + walk(h)[:, None] + walk(w)[None, :] + rng.integers(-2, 3, (h, w))
        out.append(np.abs((a % 510) - 255).astype(np.uint8).reshape(-1))
    return out


# vp8_loopfilter_apply_keyframe (m07 alone): every LF header on smooth planes of this picture size
LF_ENTRY_SIZE = (300, 170)


def lf_entry_case(case):
    """(frame, planes) of LF case `case` for the m07-alone entry point."""
    f = build(LF_KINDS[case], *LF_ENTRY_SIZE, 40 + case)
    return f, smooth_planes(int(f.frame.mb_cols) * 16, int(f.frame.mb_rows) * 16, 40 + case)


def step_planes(width, height, seed):
    """Padded planes (y, u, v as smooth_planes) painted from every tile design of the sat_* kinds: flat
    tiles 36..84 apart, +-k patterns beside steps, and the range's ends -- where the filter's
    intermediates leave [-128, 127] and its taps leave [0, 255]."""
    rng = np.random.default_rng([0x5A7, width, height, seed])
    designs = ("mb", "sub", "subsharp", "hev", "hev", "hev", "ends", "ends")  # (MB edges with hev are the rarest)
    return [_plan(*_terrain(rng, designs, height // 16, width // 16, bpm)[0]).astype(np.uint8).reshape(-1)
            for bpm in (4, 2, 2)]


# vp8_loopfilter_apply_keyframe on step_planes of this picture size: (simple, level, sharpness), one level per MB
LF_STEP_SIZE = (480, 270)
LF_STEP_CASES = [(0, 63, 0), (0, 57, 0), (0, 60, 0), (0, 62, 0), (0, 63, 3), (0, 58, 6), (1, 63, 0), (1, 57, 0), (1, 61, 2), (1, 59, 7)]


def lf_step_case(case):
    """(frame, planes) of LF_STEP_CASES[case] for the m07-alone entry point: every MB B_PRED, so every
    inner edge is filtered."""
    f = build("sat_sub", *LF_STEP_SIZE, 60 + case)
    h = f.frame
    h.lf_use_simple, h.lf_level, h.lf_sharpness = LF_STEP_CASES[case]
    return f, step_planes(int(h.mb_cols) * 16, int(h.mb_rows) * 16, 60 + case)


def same(a, b):
    """Two frames byte-identical: the header (up to the pointers), every array, the picture size."""
    hdr = vp8g.Vp8DecodedFrame.segment_id.offset
    return (bytes(a.kf) == bytes(b.kf) and bytes(a.frame)[:hdr] == bytes(b.frame)[:hdr]
            and all(np.array_equal(a.array(n), b.array(n)) for n, _, _ in vp8g.FRAME_ARRAYS))


# Known-answer cases (tests/golden/directed_kat.json, made by tests/golden/make_directed_kat.py from the
# reference's own m06/m07): every kind at 320x256 (four quads of four rows) and at an odd size.
KAT_SEED = 7
KAT_SIZES = [(320, 256), (33, 50)]


def kat_cases():
    return [(k, w, h, KAT_SEED + i) for k in KINDS for i, (w, h) in enumerate(KAT_SIZES)]


def kat_key(kind, w, h, seed):
    return f"{kind}/{w}x{h}/{seed}"
