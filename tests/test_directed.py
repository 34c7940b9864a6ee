"""CPU tests of the directed frame builder (tests/directed.py): the inputs reach what they claim.

  * determinism: the same arguments give byte-identical arrays and header;
  * shape census from the arrays (numpy, no kernel knowledge);
  * filter census from the oracle (oracle_loopfilter_census: the same walk and predicates as
    oracle_loopfilter, counting): every reachable cell >= 1 000 positions over the directed loop-filter
    set, and >= 100 on the frames with sharpness > 0, with deltas, with a level-0 segment; the smooth
    planes of the m07-alone entry pass the normal mask at >= 10 % of the positions;
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
