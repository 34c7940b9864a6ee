"""CPU tests of the directed frame builder (tests/directed.py): the inputs reach what they claim.

  * determinism: the same arguments give byte-identical arrays and header;
  * shape census from the arrays (numpy, no kernel knowledge);
  * filter census from the oracle (oracle_loopfilter_census: the same walk and predicates as
    oracle_loopfilter, counting): every reachable cell >= 1 000 positions over the directed loop-filter
    set, and >= 100 on the frames with sharpness > 0, with deltas, with a level-0 segment; the smooth
    planes of the m07-alone entry pass the normal mask at >= 10 % of the positions;
  * arithmetic census from the oracle (oracle_loopfilter_arith_census): every reachable clamp of the
    filter's arithmetic, each sign on its own, >= 100 positions over the sat_* kinds (>= 1 000 for w and
    the sub-block a), >= 200 on the step planes of the m07-alone entry, and the simple filter's cells
    >= 100 on the inputs that covered them before; the unreachable cells 0 everywhere;
  * the oracle itself on these frames: equal to the reference where it is built, and to the reference's
    hashes in tests/golden/directed_kat.json everywhere.

Census over lf00..lf15 at 320x256, seed 7 (python -m pytest tests/test_directed.py -s prints it);
rows simple / normal MB edge / normal sub-block edge, cells mask fail / pass with hev / pass without:
  all 16 frames        [119536, 0, 119408] [93620, 2037, 26967] [157340, 6482, 51090]
  sharpness > 0        [106149, 0, 105707] [79109, 1049, 23138] [133000, 3840, 43000]
  deltas enabled       [ 66868, 0,  58268] [41220,  722, 12906] [ 66996, 2440, 23108]
  a level-0 segment    [ 39560, 0,  36248] [39837,  353, 11458] [ 67006, 1677, 21429]
Smooth planes (16 cases, 304x176 padded): normal MB edge [38736, 31546, 7446] = 50 % pass, sub-block
edge [73100, 53706, 12330] = 47 % pass.
For comparison, profiles 1/2 pass the normal mask at ~5 % of positions and uniform noise planes at
well under 1 %.

Arithmetic census (oracle_loopfilter_arith_census: edge positions at which the filter's arithmetic
reaches a clamp; -s prints it).  Rows: the five paths of the filter.  Cells of the common adjust
(simple, hev, and sub-block edge without hev): positions filtered | p1-q1 > 127, < -128 | raw a > 127,
< -128 | clamped a in 124..127 | sat8 changes q0-f1 low, high | p0+f2 low, high | p1+a2 or q1-a2 low, high.
Cells of the MB adjust: positions | raw w > 127, < -128 | sat8 changes a p1/q1 tap low, high | a p2/q2 tap
low, high | sclamp(p1-q1) fires high, low | sat8 changes a p0/q0 tap low, high.  `-` = the path has no such
cell, `0*` = unreachable (test_unreachable_arith_cells).
  sat_* kinds but sat_chroma, 320x256, seed 7
    MB edge, hev            18099 |  246  158 |  1789  1332 |  2161 |  658  584 |  342  616 | -
    MB edge, no hev         58454 | 4601 4589 |   930   734 |   505   748 | 0* 0* | 0* 0*
    sub-block edge, hev     65488 |  682  508 |  5916  5173 |  7180 | 1201 1697 | 1573 1541 | -
    sub-block edge, no hev 159717 |    -    - | 13446 12878 | 13872 |   0*   0* |   0*   0* | 1640  899
  sat_chroma alone (chroma edges only)
    MB edge, hev             2033 |   55   25 |   240   161 |   270 |   98   66 |   32   17 | -
    MB edge, no hev         14713 |  590  551 |    80    71 |    52    41 | 0* 0* | 0* 0*
    sub-block edge, hev      4708 |   74   62 |   293   298 |   353 |   81   37 |  135   96 | -
    sub-block edge, no hev  36142 |    -    - |   216   215 |   222 |   0*   0* |   0*   0* |   50    0
  step_planes, the ten LF_STEP_CASES, 480x272 padded
    simple                 210867 | 2827 2194 |  5405  4448 |  6577 | 2198 2279 | 2133 2333 | -
    MB edge, hev            27947 |  406  312 |  3483  2742 |  4003 |  678  556 |  721  407 | -
    MB edge, no hev         77995 | 3489 3210 |  1785  1544 |   546  1451 | 0* 0* | 0* 0*
    sub-block edge, hev     86660 | 1728 1308 |  7648  6921 |  9381 | 2878 1801 | 2570 1829 | -
    sub-block edge, no hev 241616 |    -    - | 16570 15823 | 17241 |   0*   0* |   0*   0* | 3190 2496
  lf00..lf15 + synthetic profiles 1 and 2 (seed 6), 320x256: what covered the simple filter before
    simple                 154576 | 7756 7865 |  2764  2665 |  9529 | 4759 5253 | 5025 4883 | -
  (the same inputs on the normal filter: w beyond +-127 at 1 / 2 positions, a on sub-block edges at 22 / 17)
"""
import hashlib
import json

import numpy as np
import pytest

import directed as D
from conftest import GOLDEN

CENSUS_SIZE = (320, 256)
REACHABLE = [(0, 0), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
needs_ref = pytest.mark.skipif("not __import__('vp8g').ref_available()", reason="reference build absent")


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.mark.parametrize("kind", D.KINDS)
def test_builder_is_deterministic(kind):
    a, b, c = D.build(kind, 100, 70, 5), D.build(kind, 100, 70, 5), D.build(kind, 100, 70, 6)
    assert D.same(a, b)
    assert not D.same(a, c)


def _blocks(f):
    cy, cu, cv, _ = D._coeffs(f)
    return cy, np.concatenate([cu, cv], axis=1)


@pytest.mark.parametrize("kind", D.UNIFORM + ["wrap"])
def test_uniform_frames_are_uniform(kind):
    """100 % of the blocks of a role are in the frame's class (dc: no AC; cols01: columns 2-3 zero and
    every MB keeps an AC in columns 0-1).  `full` is left as generated: at least 99 % of the MBs have
    an AC in columns 2-3 (P(a generated MB has none) < 1e-4 per role)."""
    f = D.build(kind, *CENSUS_SIZE, 7)
    names = ("dc", "dc") if kind == "wrap" else kind.split("_")[1:]
    for role, name, blocks, cls in zip(("luma", "chroma"), names, _blocks(f), D.mb_classes(f)):
        if name == "dc":
            assert not blocks[:, :, 1:].any(), role
        elif name == "cols01":
            assert not blocks[:, :, D._C23].any(), role
        assert (cls == D.SHAPES.index(name)).mean() >= (0.99 if name == "full" else 1.0), (role, np.bincount(cls))
    assert np.array_equal(f.array("has_coeff") != 0, D.coded(f))
    assert np.array_equal(f.array("skip_coeff") != 0, ~D.coded(f))


def test_wrap_frame_wraps_int16():
    f = D.build("wrap", *CENSUS_SIZE, 7)
    cy, cu, cv, y2 = D._coeffs(f)
    bp = f.array("ymode") == 4
    assert bp.any() and (~bp).any()
    for dcs in (y2[~bp, 0], cy[bp, :, 0], cu[:, :, 0], cv[:, :, 0]):
        assert (np.abs(dcs) == 2114).all() and (dcs > 0).any() and (dcs < 0).any()
    h = f.frame
    assert (h.q_index, h.y1_dc_delta_q, h.y2_dc_delta_q, h.uv_dc_delta_q, h.segmentation_enabled) == (127, 15, 15, 15, 0)
    # RFC 6386 14.1: dc_q(127) = 157 (Y), 2 * 157 (Y2), min(157, 132) (chroma): all beyond int16
    assert min(2114 * 157, 2114 * 314, 2114 * 132) > 32767


def test_mixed_frame_has_every_class_at_its_weight():
    """Both roles: the share of each class within 4 standard deviations of its weight (n = 320 MBs:
    +-11, +-10, +-9 points), and the two roles drawn separately (they differ somewhere)."""
    f = D.build("mixed", *CENSUS_SIZE, 7)
    n = f.mb_total
    luma, chroma = D.mb_classes(f)
    for role, cls in (("luma", luma), ("chroma", chroma)):
        for k, p in enumerate(D.MIX_WEIGHTS):
            share = (cls == k).mean()
            print(f"mixed {role} {D.SHAPES[k]}: {share:.3f} (weight {p})")
            assert abs(share - p) <= 4 * (p * (1 - p) / n) ** 0.5, (role, k, share)
    assert (luma != chroma).any()
    # the weights give every form >= 5 % for the richest of four independent MBs (the quad chain's wave)
    dc4, le1 = D.MIX_WEIGHTS[0] ** 4, (D.MIX_WEIGHTS[0] + D.MIX_WEIGHTS[1]) ** 4
    assert min(dc4, le1 - dc4, 1 - le1) >= 0.05


@pytest.mark.parametrize("kind", D.SPOILERS)
@pytest.mark.parametrize("size", [CENSUS_SIZE, (52, 300)])
def test_spoiler_sits_in_one_block_of_one_role(kind, size):
    f = D.build(kind, *size, 7)
    _, shape, role = kind.split("_")
    base = D.SHAPES.index(shape)
    k = D.spoil_step(int(f.frame.mb_cols))
    assert np.gcd(k, int(f.frame.mb_cols)) == 1
    spoiled = np.arange(f.mb_total) % k == 0
    luma, chroma = D.mb_classes(f)
    mine, other = (luma, chroma) if role == "luma" else (chroma, luma)
    assert (other == base).all()
    assert (mine[spoiled] == 2).all() and (mine[~spoiled] == base).all()
    blocks = _blocks(f)[0 if role == "luma" else 1]
    rich = blocks[:, :, D._C23].any(axis=2)  # per block: an AC in columns 2-3
    assert (rich.sum(axis=1) == spoiled).all()  # exactly one block per spoiled MB


def test_bpred_frames(vp8g):
    a, n = D.build("bpred_all", *CENSUS_SIZE, 7), D.build("bpred_none", *CENSUS_SIZE, 7)
    assert (a.array("ymode") == 4).all()
    assert not (n.array("ymode") == 4).any()
    was_bp = vp8g.synth_frame(*CENSUS_SIZE, 7, 2).array("ymode") == 4  # (the MBs that were given a Y2 block)
    assert was_bp.sum() > 20 and D._coeffs(n)[3][was_bp].any(axis=1).mean() > 0.95


@pytest.mark.parametrize("kind", ["skip", "lie_hasc0", "lie_hasc1"] + D.LF_KINDS)
def test_skip_and_lie_subsets_hold_both_mb_kinds(kind):
    f = D.build(kind, *CENSUS_SIZE, 7)
    bp = f.array("ymode") == 4
    has, coded = f.array("has_coeff") != 0, D.coded(f)
    if kind == "lie_hasc0":
        sub = ~has & coded
        assert not (has & ~coded).any()
    elif kind == "lie_hasc1":
        sub = has & ~coded
        assert not (~has & coded).any()
    else:
        sub = ~coded
        assert np.array_equal(has, coded) and np.array_equal(f.array("skip_coeff") != 0, ~coded)
    assert (sub & bp).sum() >= 5 and (sub & ~bp).sum() >= 5, ((sub & bp).sum(), (sub & ~bp).sum())
    assert (~sub & bp).any() and (~sub & ~bp).any()


def test_lf_headers_cover_every_parameter():
    frames = [D.build(k, *CENSUS_SIZE, 7) for k in D.LF_KINDS]
    hs = [f.frame for f in frames]
    for simple in (0, 1):
        assert {h.lf_sharpness for h in hs if h.lf_use_simple == simple} == set(range(8))
        sel = [(f, D.mb_lf_levels(f)) for f in frames if f.frame.lf_use_simple == simple]
        assert any(f.frame.segmentation_enabled and (lv == 0).any() and (lv > 0).any() for f, lv in sel)
        if not simple:  # both sides of each hev threshold, the adjacent values (the simple filter has no hev)
            assert {14, 15, 39, 40} <= set(np.concatenate([lv for _, lv in sel]).tolist())
        bp0 = [(lv[f.array("ymode") == 4] == 0).all() and (lv[f.array("ymode") != 4] > 0).all() for f, lv in sel
               if f.frame.lf_delta_enabled]
        assert any(bp0) and not all(bp0)
        assert {f.frame.segmentation_enabled for f, _ in sel} == {0, 1}
        assert {f.frame.segmentation_abs for f, _ in sel if f.frame.segmentation_enabled} == {0, 1}
    assert {h.lf_level for h in hs} >= {0, 63} and len({h.lf_level for h in hs}) == 16


def test_filter_census_of_the_directed_lf_set(vp8g):
    """Conditions on the inputs: if a cell falls short, the inputs change, never the floor."""
    subsets = {"all": lambda f, lv: True, "sharpness > 0": lambda f, lv: f.frame.lf_sharpness > 0,
               "deltas enabled": lambda f, lv: f.frame.lf_delta_enabled != 0,
               "a level-0 segment": lambda f, lv: bool(f.frame.segmentation_enabled and (lv == 0).any() and (lv > 0).any())}
    tot = {k: np.zeros((3, 3), np.uint64) for k in subsets}
    for kind in D.LF_KINDS:
        f = D.build(kind, *CENSUS_SIZE, 7)
        c, lv = vp8g.oracle_frame_census(f), D.mb_lf_levels(f)
        for k, pred in subsets.items():
            if pred(f, lv):
                tot[k] += c
    for k, t in tot.items():
        print(f"{k:18s}", *[t[i].tolist() for i in range(3)])
        assert t[0, 1] == 0  # (the simple filter has no hev cell)
        for cell in REACHABLE:
            assert t[cell] >= (1000 if k == "all" else 100), (k, vp8g.LF_KINDS[cell[0]], vp8g.LF_CELLS[cell[1]], int(t[cell]))


def test_census_counts_every_position_once(vp8g):
    """The census visits what the walk visits: on a one-level normal-filter frame with every MB coded,
    per MB 2 x (16 + 8 + 8) MB-edge positions where a neighbour exists and 2 x (3 x 16 + 8 + 8)
    sub-block positions; and it leaves its input planes alone."""
    f = D.build("lf04", 64, 48, 3)  # lf04 (after LF_CASES' order): normal filter
    h = f.frame
    assert not h.lf_use_simple
    h.segmentation_enabled, h.lf_delta_enabled, h.lf_level = 0, 0, 20
    f.array("has_coeff")[:] = 1
    planes = D.smooth_planes(64, 48, 1)
    keep = [p.copy() for p in planes]
    c = vp8g.oracle_loopfilter_census(planes, h)
    assert all(np.array_equal(a, b) for a, b in zip(planes, keep))
    cols, rows = 4, 3
    assert c[0].sum() == 0
    assert c[1].sum() == 32 * ((cols - 1) * rows + (rows - 1) * cols)
    assert c[2].sum() == 2 * 64 * cols * rows


def test_smooth_planes_pass_the_normal_mask(vp8g):
    """The planes of the m07-alone GPU test (directed.lf_entry_case): >= 10 % mask pass on each normal
    kind, so that the filter modifies pixels there under every header."""
    tot = np.zeros((3, 3), np.uint64)
    for case in range(16):
        f, planes = D.lf_entry_case(case)
        tot += vp8g.oracle_loopfilter_census(planes, f.frame)
    for kind in (1, 2):
        share = tot[kind, 1:].sum() / tot[kind].sum()
        print(f"smooth planes, {vp8g.LF_KINDS[kind]}: {tot[kind].tolist()} pass {share:.3f}")
        assert share >= 0.10
    assert tot[0, 0] >= 1000 and tot[0, 2] >= 1000 and tot[1, 1] >= 1000 and tot[2, 1] >= 1000


# ---- the filter's saturating arithmetic (oracle_loopfilter_arith_census) -------------------------------
# (path, cell) of vp8g.LF_ARITH_PATHS / LF_ARITH_CELLS that no input reaches; test_unreachable_arith_cells
UNREACHABLE = {(2, 7), (2, 8), (2, 9), (2, 10), (4, 6), (4, 7), (4, 8), (4, 9)}
W_AND_SUB_A = {(2, 1), (2, 2), (3, 3), (3, 4), (4, 3), (4, 4)}  # MB adjust w, sub-block raw a: each sign


def arith_cells(vp8g, paths):
    return [(p, c) for p in paths for c, name in enumerate(vp8g.LF_ARITH_CELLS[p]) if c and name and (p, c) not in UNREACHABLE]


def show(vp8g, title, t):
    print(title)
    for p, row in enumerate(t):
        print(f"  {vp8g.LF_ARITH_PATHS[p]:28s}", row.tolist())


def check_arith(vp8g, t, paths, floor, floors=()):
    for p, c in UNREACHABLE:
        assert t[p, c] == 0, (vp8g.LF_ARITH_PATHS[p], vp8g.LF_ARITH_CELLS[p][c], int(t[p, c]))
    for p in range(5):  # (a cell the path does not have stays 0, and no cell exceeds the calls)
        assert all(t[p, c] == 0 for c, name in enumerate(vp8g.LF_ARITH_CELLS[p]) if name is None)
        assert (t[p, 1:] <= t[p, 0]).all() or p in (2, 4)  # (paths 2 and 4 count two taps per position)
    for p, c in arith_cells(vp8g, paths):
        need = dict(floors).get((p, c), floor)
        assert t[p, c] >= need, (vp8g.LF_ARITH_PATHS[p], vp8g.LF_ARITH_CELLS[p][c], int(t[p, c]), need)


def test_unreachable_arith_cells():
    """The cells no input reaches, each by exhaustive search over the pixels that enter it, under the
    loosest parameters there are (level 63, sharpness 0: hev threshold 2, MB-edge limit 193).

    MB adjust (MB edge, no hev), sclamp(p1 - q1): |p1 - p0| <= 2 and |q1 - q0| <= 2, so |p1 - q1| <=
    |p0 - q0| + 4, and the mask's 2|p0 - q0| + |p1 - q1| / 2 <= 193 leaves |p1 - q1| < 128.
    MB adjust, sat8 on the p0/q0 taps: with d = q0 - p0 > 0, w <= 2d + 4, and p0 + ((27w + 63) >> 7) >= 256
    would need 74d <= 43.  Searched: every p0, q0 with p1, q1 within 2 of them.
    Sub-block edge without hev, sat8 on q0 - f1 and p0 + f2: a = 3(q0 - p0) alone, |f| <= (3|d| + 4) >> 3
    <= |d| moves each pixel toward the other.  Searched: every p0, q0."""
    sc = lambda v: np.clip(v, -128, 127)  # noqa: E731
    p0, q0, dp, dq = np.meshgrid(np.arange(256), np.arange(256), np.arange(-2, 3), np.arange(-2, 3), indexing="ij")
    p1, q1 = p0 + dp, q0 + dq
    ok = (p1 >= 0) & (p1 <= 255) & (q1 >= 0) & (q1 <= 255) & (2 * abs(p0 - q0) + (abs(p1 - q1) >> 1) <= 193)
    assert ok.sum() > 500_000  # (the search is not vacuous)
    assert (abs(p1 - q1)[ok] < 128).all()
    a27 = (27 * sc(sc(p1 - q1) + 3 * (q0 - p0)) + 63) >> 7
    assert ((p0 + a27)[ok] >= 0).all() and ((p0 + a27)[ok] <= 255).all()
    assert ((q0 - a27)[ok] >= 0).all() and ((q0 - a27)[ok] <= 255).all()
    p0, q0 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a = sc(3 * (q0 - p0))
    f1, f2 = sc(a + 4) >> 3, sc(a + 3) >> 3
    assert (q0 - f1 >= 0).all() and (q0 - f1 <= 255).all() and (p0 + f2 >= 0).all() and (p0 + f2 <= 255).all()


def test_arith_census_of_the_saturating_kinds(vp8g):
    """Every reachable cell of the normal filter, each sign on its own, >= 100 positions over the sat_*
    kinds that paint luma (>= 1 000 for the MB adjust's w and the sub-block edges' raw a); sat_chroma,
    whose luma plane is flat, reaches w and the sub-block a on chroma edges alone; sat_sharp (sharpness
    3: interior limit 6, where w <= 2 * 55 + 4 and the outer a <= 2 * 55 + 12 stay inside) saturates a = 3d on
    sub-block edges without hev; sat_seg has segments on both sides of level 52, below which flat MBs that pass
    the mask cannot saturate w.  If a cell falls short, the inputs change, never the floor."""
    per = {k: vp8g.oracle_frame_arith_census(D.build(k, *CENSUS_SIZE, 7)) for k in D.SAT_KINDS}
    luma = sum(c for k, c in per.items() if k != "sat_chroma")
    show(vp8g, "sat_* kinds but sat_chroma", luma)
    show(vp8g, "sat_chroma", per["sat_chroma"])
    check_arith(vp8g, luma, (1, 2, 3, 4), 100, {c: 1000 for c in W_AND_SUB_A})
    assert luma[0].sum() == 0  # (the normal filter throughout)
    for k, c in per.items():
        check_arith(vp8g, c, (), 0)
    for cell in W_AND_SUB_A:
        assert per["sat_chroma"][cell] >= 100, (cell, int(per["sat_chroma"][cell]))
    for cell in ((4, 3), (4, 4)):
        assert per["sat_sharp"][cell] >= 100, (cell, int(per["sat_sharp"][cell]))
    f = D.build("sat_sharp", *CENSUS_SIZE, 7)
    assert f.frame.lf_sharpness > 0
    f = D.build("sat_seg", *CENSUS_SIZE, 7)
    lv = D.mb_lf_levels(f)
    assert f.frame.segmentation_enabled and (lv >= 57).sum() >= 50 and (lv < 52).sum() >= 50
    assert per["sat_seg"][2, 1] >= 100 and per["sat_seg"][2, 2] >= 100
    for k in D.SAT_KINDS:
        f = D.build(k, *CENSUS_SIZE, 7)
        h = f.frame
        assert not h.lf_use_simple and (k == "sat_seg" or 57 <= h.lf_level <= 63)


def test_saturating_kinds_reconstruct_to_their_plan(vp8g):
    """The painted kinds are what they say: the oracle's unfiltered luma of sat_sub is the checkerboard of
    flat sub-blocks the builder planned (each 4x4 block one value, horizontal neighbours 36..80 apart
    inside a tile)."""
    f = D.build("sat_sub", *CENSUS_SIZE, 7)
    w, h = CENSUS_SIZE
    y = np.frombuffer(vp8g.oracle_reconstruct(f, False), np.uint8)[:w * h].reshape(h // 4, 4, w // 4, 4).astype(int)
    assert (y == y[:, :1, :, :1]).all()
    d = abs(np.diff(y[:, 0, :, 0], axis=1))
    inside = np.arange(1, w // 4) % 8 != 0  # (not across a tile's border)
    assert d[:, inside].min() >= 36 and d[:, inside].max() <= 80


def test_arith_census_of_the_step_planes(vp8g):
    """The planes of the m07-alone GPU test (directed.lf_step_case): every reachable cell of all five
    paths >= 200, summed over the cases; simple and normal headers, sharpness 0 and > 0, levels 57..63."""
    tot = np.zeros((5, 12), np.uint64)
    for case in range(len(D.LF_STEP_CASES)):
        f, planes = D.lf_step_case(case)
        tot += vp8g.oracle_loopfilter_arith_census(planes, f.frame)
    show(vp8g, "step planes", tot)
    check_arith(vp8g, tot, range(5), 200)
    for simple in (0, 1):
        sh = {s for sm, lvl, s in D.LF_STEP_CASES if sm == simple}
        assert 0 in sh and max(sh) > 0
    assert all(57 <= lvl <= 63 for _, lvl, _ in D.LF_STEP_CASES)


def test_arith_census_simple_filter_on_the_lf_set(vp8g):
    """What covers the simple filter's cells today stays: lf00..lf15 plus one simple-filter frame of each
    of the synthetic profiles 1 and 2 (seed 6: level 14, sharpness 0), >= 100 per cell."""
    tot = np.zeros((5, 12), np.uint64)
    for kind in D.LF_KINDS:
        tot += vp8g.oracle_frame_arith_census(D.build(kind, *CENSUS_SIZE, 7))
    for profile in (1, 2):
        f = vp8g.synth_frame(*CENSUS_SIZE, 6, profile)
        assert f.frame.lf_use_simple
        tot += vp8g.oracle_frame_arith_census(f)
    show(vp8g, "lf00..lf15 + profiles 1, 2", tot)
    check_arith(vp8g, tot, (0,), 100)


def test_arith_census_counts_what_the_filter_does(vp8g):
    """The arithmetic census walks what oracle_loopfilter_census walks (cell 0 of its paths = the mask
    pass cells of that table), leaves its planes alone, and on hand-made pixels counts the clamps:
    two flat MBs 70 apart (w = 140) and two flat sub-blocks 50 apart (a = 150), rising and falling."""
    f, planes = D.lf_step_case(0)
    keep = [p.copy() for p in planes]
    a, c = vp8g.oracle_loopfilter_arith_census(planes, f.frame), vp8g.oracle_loopfilter_census(planes, f.frame)
    assert all(np.array_equal(x, y) for x, y in zip(planes, keep))
    assert [int(a[p, 0]) for p in range(5)] == [int(c[0, 2]), int(c[1, 1]), int(c[1, 2]), int(c[2, 1]), int(c[2, 2])]
    f = D.build("sat_sub", 32, 16, 1)  # (every MB B_PRED; level 63, sharpness 0)
    for row, up in (((60, 110, 120, 190), True), ((190, 140, 130, 60), False)):
        y = np.empty((16, 32), np.uint8)  # sub-blocks 50 apart at x = 4, 10 apart at x = 8, MBs 70 apart at x = 16
        y[:, :4], y[:, 4:8], y[:, 8:16], y[:, 16:] = row
        a = vp8g.oracle_loopfilter_arith_census((y.reshape(-1), np.full(128, 128, np.uint8), np.full(128, 128, np.uint8)), f.frame)
        assert a[2, 1:3].tolist() == ([16, 0] if up else [0, 16]), a[2].tolist()
        assert a[4, 3:6].tolist() == ([16, 0, 16] if up else [0, 16, 0]), a[4].tolist()
        assert not a[2, 3:].any() and not a[4, 6:].any() and not a[[0, 1, 3], 1:].any()


def test_saturating_kinds_pass_through_the_stream_writer():
    """The two kinds the GPU pipeline test sends as .webp: the host front end returns the frame."""
    import streams as S
    for kind in ("sat_mb", "sat_seg"):
        f, data = S.directed_stream(kind, *CENSUS_SIZE, 7)
        got = S.decode(data)
        assert got is not None and D.same(f, got), kind


@needs_ref
@pytest.mark.parametrize("kind", D.KINDS)
def test_oracle_matches_reference_on_directed_frames(vp8g, kind):
    for k, w, h, seed in D.kat_cases():
        if k == kind:
            f = D.build(k, w, h, seed)
            for filtered in (False, True):
                assert vp8g.oracle_reconstruct(f, filtered) == vp8g.ref_reconstruct(f, filtered), (k, w, h, filtered)


@needs_ref
def test_oracle_loopfilter_alone_matches_reference_on_smooth_planes(vp8g):
    import ctypes as C
    for case in range(16):
        f, planes = D.lf_entry_case(case)
        w, h = int(f.frame.mb_cols) * 16, int(f.frame.mb_rows) * 16
        ours, ref = [p.copy() for p in planes], [p.copy() for p in planes]
        assert vp8g.oracle_lib().oracle_loopfilter(*[p.ctypes.data for p in ours], C.byref(f.frame)) == 0
        assert vp8g.ref_lib().ref_loopfilter_padded(*[p.ctypes.data for p in ref], w, h, C.byref(f.frame)) == 0
        assert all(np.array_equal(a, b) for a, b in zip(ours, ref)), case
        assert any(not np.array_equal(a, b) for a, b in zip(ours, planes)), case  # (the filter did something)


def test_oracle_vs_directed_kat(vp8g):
    """The oracle against sha256 of the reference's own m06 / m06+m07 output on every directed kind
    (tests/golden/make_directed_kat.py): holds where the reference is not built, too."""
    kat = json.loads((GOLDEN / "directed_kat.json").read_text())["cases"]
    assert set(kat) == {D.kat_key(*c) for c in D.kat_cases()}
    for case in D.kat_cases():
        f = D.build(*case)
        ent = kat[D.kat_key(*case)]
        assert sha(vp8g.oracle_reconstruct(f, False)) == ent["yuv_sha256"], case
        assert sha(vp8g.oracle_reconstruct(f, True)) == ent["yuvf_sha256"], case


def test_unknown_launch_mode_cannot_pass_a_mode_assertion(vp8g, monkeypatch):
    """A library without vp8g_last_launch_mode (an older build under VP8G_LIB): launch_mode() is None,
    and the tests' `mode & MODE_*` raises on it instead of holding vacuously, as it did on -1."""
    import types

    import vp8g_batch
    monkeypatch.setitem(vp8g._libs, "gpu", types.SimpleNamespace(_typed=True))
    mode = vp8g_batch.DeviceBatch.launch_mode(None)
    assert mode is None
    with pytest.raises(TypeError):
        mode & vp8g.MODE_QUAD
