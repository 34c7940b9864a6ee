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
In every kind but the two lies has_coeff / skip_coeff are recomputed from the coefficients.

LF_CASES: simple / normal filter x sharpness 0..7 (case i: simple = i & 1, sharpness = i >> 1), and
per case (frame level, segmentation, abs, segment levels, deltas, ref delta 0, mode delta 0): frame
levels 0..63, segments on / off, absolute / relative, segments of level 0 beside filtered ones,
lf_mode_delta[0] that takes B_PRED MBs to level 0 and ones that do not, per-MB levels on both sides
of 15 and of 40 (the hev thresholds).

smooth_planes(w, h, seed): padded planes for vp8_loopfilter_apply_keyframe -- a seeded random walk
(steps of a few units, occasional jumps) instead of uniform noise, on which the normal filter's mask
fails at ~95 % of the positions.
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
KINDS = UNIFORM + ["mixed"] + SPOILERS + ["wrap", "bpred_all", "bpred_none", "skip", "lie_hasc0", "lie_hasc1"] + LF_KINDS

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


def build(kind, width, height, seed):
    """The directed frame `kind` (one of KINDS) of width x height from `seed`: a vp8g.Frame."""
    rng = np.random.default_rng([KINDS.index(kind), width, height, seed])
    smooth = kind in ("skip", "lie_hasc0", "lie_hasc1") or kind in LF_KINDS
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
