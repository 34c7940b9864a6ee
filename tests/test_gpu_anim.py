"""The animation compositor on the device: vp8g_anim_compose_batch_device against the sequential
restatement (vp8f_anim_compose, itself checked against libwebp in tests/test_anim_host.py) on seeded synthetic
animations, bit for bit; every tensor form; the entry point's checks; and the end-to-end entry on the fixtures of
tests/golden/anim/ against libwebp's canvases and timestamps (tests/golden/anim.json)."""
import errno
import hashlib
import itertools
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ANIM = GOLDEN / "anim"
ALPHAS = np.array([0, 1, 3, 128, 254, 255], np.uint32)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "anim.json").read_text())


def fixture(name):
    return (ANIM / f"{name}.webp").read_bytes()


def picture(rng, w, h, alphas=ALPHAS):
    """uint32 [h, w] 0xAARRGGBB: random colour (also under alpha 0), alpha drawn from `alphas`."""
    return (rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) | np.asarray(alphas, np.uint32)[rng.integers(0, len(alphas), (h, w))] << 24)


def frame(rng, x, y, w, h, blend=1, dispose=0, has_alpha=1, alphas=ALPHAS):
    return {"argb": picture(rng, w, h, alphas), "x": x, "y": y, "blend": blend, "dispose": dispose, "has_alpha": has_alpha}


def random_anim(rng, cw, ch, n):
    """n frames of random rectangles (even origins) and rules on a cw x ch canvas."""
    frames = []
    for _ in range(n):
        x, y = 2 * int(rng.integers(0, (cw + 1) // 2)), 2 * int(rng.integers(0, (ch + 1) // 2))
        w, h = int(rng.integers(1, cw - x + 1)), int(rng.integers(1, ch - y + 1))
        if rng.integers(0, 4) == 0:
            x, y, w, h = 0, 0, cw, ch
        frames.append(frame(rng, x, y, w, h, int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 4) != 0)))
    return (cw, ch, frames)


def check(vp8g, anims, **kw):
    """One launch over `anims`; every canvas equals the restatement's (uint8 / NHWC / RGBA).  Returns the key flags."""
    got = vp8g.gpu_anim_compose(anims, vp8g.tensor_opt((1, 1), "uint8", "NHWC"), 4, **kw)
    keys = []
    for i, (cw, ch, frames) in enumerate(anims):
        want, k = vp8g.host_anim_compose(cw, ch, frames)
        assert got[i].shape == (len(frames), ch, cw, 4)
        for f in range(len(frames)):
            assert np.array_equal(got[i][f].numpy(), vp8g.argb_to_rgba(want[f])), (i, cw, ch, f)
        keys.append(k)
    return keys


def test_small_canvases_and_mixed_launch(vp8g):
    rng = np.random.default_rng(1)
    anims = [random_anim(rng, cw, ch, n) for (cw, ch), n in zip([(1, 1), (2, 2), (3, 5), (3, 5), (1, 1), (7, 2)], [3, 5, 6, 1, 1, 9])]
    check(vp8g, anims)           # animations of different canvases and frame counts in one launch
    for a in anims[:3]:
        check(vp8g, [a])         # and alone


def test_widths_at_the_kernels_boundaries(vp8g):
    """Canvas widths g - 1, g, g + 1 and 2 g for g = the pixels of a thread and of a task: a row's last partial piece,
    rows that end exactly on a piece / task boundary, tasks that span rows, more than one task per segment."""
    per_thread, per_task, _ = vp8g.anim_geometry()
    assert per_thread >= 2 and per_task % per_thread == 0
    rng = np.random.default_rng(2)
    anims = []
    for g, ch in ((per_thread, 5), (per_task, 3)):
        for cw in (g - 1, g, g + 1, 2 * g):
            x1 = 2 * ((cw // 2) // 2)
            frames = [frame(rng, 0, 0, cw, ch, 1, 0),
                      frame(rng, x1, 0, cw - x1, ch, 1, 1),                       # to the right edge, disposed
                      frame(rng, 0, 2 * ((ch - 1) // 2), cw, ch - 2 * ((ch - 1) // 2), 1, 0),  # the bottom rows, whole width
                      frame(rng, max(0, x1 - 2), 0, min(3, cw - max(0, x1 - 2)), 1, 0, 0),
                      frame(rng, 0, 0, cw, ch, 1, 0)]                             # blended where nothing was just cleared
            anims.append((cw, ch, frames))
    check(vp8g, anims)


def test_rectangles_and_every_rule_combination(vp8g):
    """1 x 1 and full rectangles, rectangles on each edge, columns that start and end inside one thread's pixels, and every
    combination of blend, dispose and the previous frame's dispose with the frame inside, across and outside the
    previous rectangle."""
    per_thread, _, _ = vp8g.anim_geometry()
    rng = np.random.default_rng(3)
    cw, ch = 5 * per_thread + 3, 9
    inside_one_thread = [(2 * per_thread + 2, 2, 1, 3), (per_thread, 4, per_thread - 1, 2), (2, 0, 2, ch)]
    edges = [(0, 2, 3, 4), (cw - 3 - (cw - 3) % 2, 2, 3 + (cw - 3) % 2, 4), (4, 0, 7, 2), (4, ch - 1 - (ch - 1) % 2, 7, 1 + (ch - 1) % 2),
             (0, 0, 1, 1), (cw - 1 - (cw - 1) % 2, ch - 1 - (ch - 1) % 2, 1 + (cw - 1) % 2, 1 + (ch - 1) % 2), (0, 0, cw, ch)]
    anims = []
    for rect in inside_one_thread + edges:
        for blend, dispose in itertools.product((0, 1), repeat=2):
            anims.append((cw, ch, [frame(rng, 0, 0, cw, ch, 0, 0), frame(rng, *rect, blend, dispose), frame(rng, 0, 0, cw, ch, 1, 0)]))
    prev = (6, 2, 10, 4)
    places = {"inside": (8, 2, 5, 3), "across": (2, 0, 9, 5), "outside": (0, 6, 5, 3), "same": prev, "around": (4, 0, 14, 8)}
    for (name, rect), pd, blend, dispose in itertools.product(places.items(), (0, 1), (0, 1), (0, 1)):
        anims.append((cw, ch, [frame(rng, 0, 0, cw, ch, 1, 0, alphas=[255, 128]), frame(rng, *prev, 1, pd),
                               frame(rng, *rect, blend, dispose), frame(rng, 0, 0, cw, ch, 1, 0)]))
    check(vp8g, anims)


def test_blend_arithmetic_on_every_alpha_pair(vp8g):
    """Every source alpha of the set over every canvas alpha of the set (and 0: a transparent canvas is not the identity),
    colours 0, 1, 127, 128, 254, 255."""
    vals = np.array([0, 1, 127, 128, 254, 255], np.uint32)
    a = ALPHAS
    sa, da, sc, dc = (v.reshape(-1) for v in np.meshgrid(a, a, vals, vals, indexing="ij"))
    n = sa.size  # 6^4 pixels in one row
    below = (da << 24 | dc << 16 | (255 - dc) << 8 | dc).reshape(1, n)
    above = (sa << 24 | sc << 16 | sc << 8 | (255 - sc)).reshape(1, n)
    frames = [{"argb": below, "x": 0, "y": 0, "blend": 0, "dispose": 0, "has_alpha": 1},
              {"argb": above, "x": 0, "y": 0, "blend": 1, "dispose": 0, "has_alpha": 1}]
    check(vp8g, [(n, 1, frames)])
    want, _ = vp8g.host_anim_compose(n, 1, frames)
    # the three cases that cannot be simplified, by hand
    s255, s0 = (sa == 255), (sa == 0)
    assert np.array_equal(want[1][0][s255], above[0][s255]) and np.array_equal(want[1][0][s0], below[0][s0])
    i = int(np.flatnonzero((sa == 3) & (da == 0) & (sc == 128))[0])
    assert (int(want[1][0][i]) >> 16) & 255 == 127 and int(want[1][0][i]) >> 24 == 3  # c - 1 over a transparent canvas


def test_key_frame_chains_and_frame_counts(vp8g):
    """Chains with no further key frame, one, and several (every frame a segment of its own); F = 1; long chains on a
    small canvas (many segments, and one long segment); F around the per-task frame limit if the kernel has one."""
    _, _, limit = vp8g.anim_geometry()
    rng = np.random.default_rng(4)
    cw, ch = 10, 6
    full = (0, 0, cw, ch)
    part = (2, 2, 5, 3)
    none = [frame(rng, *full, 1, 0)] + [frame(rng, *part, 1, d) for d in (0, 1, 0, 1, 1, 0)]
    one = [frame(rng, *part, 1, 0), frame(rng, *part, 1, 0), frame(rng, *full, 0, 0), frame(rng, *part, 1, 1), frame(rng, *part, 1, 0)]
    every = [frame(rng, *full, 1, 1, has_alpha=k % 2) for k in range(6)]
    by_disposal = [frame(rng, *part, 1, 1) for _ in range(5)] + [frame(rng, *full, 1, 0)]
    opaque_full = [frame(rng, *full, 1, 0, has_alpha=0, alphas=[255]) for _ in range(4)]
    counts = sorted({1, 2, 33} | ({limit - 1, limit, limit + 1, 2 * limit + 1} if limit else set()))
    longs = [[frame(rng, *full, 1, 0)] + [frame(rng, *part, 1, int(k % 3 == 0)) for k in range(n - 1)] for n in counts if n > 0]
    anims = [(cw, ch, f) for f in (none, one, every, by_disposal, opaque_full, *longs)]
    keys = check(vp8g, anims)
    assert keys[0] == [1, 0, 0, 0, 0, 0, 0] and keys[1] == [1, 0, 1, 0, 0] and keys[2] == [1] * 6
    assert keys[3] == [1, 1, 1, 1, 1, 1] and keys[4] == [1] * 4
    assert all(k == [1] + [0] * (len(k) - 1) for k in keys[5:])


TENSOR_FORMS = list(itertools.product(("uint8", "float16", "bfloat16", "float32"), ("NHWC", "NCHW"), (False, True), (3, 4)))


@pytest.mark.parametrize("dtype,layout,bgr,channels", TENSOR_FORMS)
def test_every_tensor_form(vp8g, dtype, layout, bgr, channels):
    """One small animation (an odd width: rows off the dword boundary for the narrow types) through every dtype, layout,
    channel order and channel count, against host_tensor_argb of the restated canvases."""
    rng = np.random.default_rng(5)
    cw, ch = 13, 7
    frames = [frame(rng, 0, 0, cw, ch, 1, 0), frame(rng, 2, 2, 9, 4, 1, 1), frame(rng, 4, 0, 9, 7, 1, 0), frame(rng, 0, 0, cw, ch, 1, 0)]
    opt = vp8g.tensor_opt((cw, ch), dtype, layout, scale=[1 / 255, 0.5, 3.0], bias=[-0.5, 0.25, 1e-3], bgr=bgr)
    got, = vp8g.gpu_anim_compose([(cw, ch, frames)], opt, channels)
    want, _ = vp8g.host_anim_compose(cw, ch, frames)
    for k in range(len(frames)):
        exp = vp8g.host_tensor_argb(want[k], opt, channels)
        assert got[k].dtype == exp.dtype and got[k].shape == exp.shape
        assert torch.equal(got[k].view(torch.uint8), exp.view(torch.uint8)), k


def test_bad_descriptors_are_refused_before_launch(vp8g):
    rng = np.random.default_rng(6)
    a = (12, 8, [frame(rng, 0, 0, 12, 8, 1, 0), frame(rng, 2, 2, 6, 4, 1, 1), frame(rng, 0, 0, 12, 8, 0, 0)])
    b = (6, 4, [frame(rng, 0, 0, 6, 4, 1, 0), frame(rng, 2, 0, 2, 2, 1, 0)])
    opt = vp8g.tensor_opt((1, 1), "float32", "NHWC")
    vp8g.gpu_anim_compose([a, b], opt, 4)

    def field(i, k, name, value):
        def m(descs, recs):
            setattr(recs[i][k], name, value)
        return m

    def desc_field(i, name, value):
        def m(descs, recs):
            setattr(descs[i], name, value)
        return m

    K = vp8g.ANIM_KEY
    bad = {
        "rectangle beyond the right edge": field(0, 1, "width", 11), "rectangle beyond the bottom": field(0, 1, "y", 6),
        "empty rectangle": field(1, 1, "height", 0), "odd x": field(0, 1, "x", 3), "odd y": field(1, 1, "y", 1),
        "picture off a dword": field(0, 0, "src", 2), "unknown flag": field(0, 1, "flags", 16 | 1),
        "key flag cleared": field(0, 2, "flags", 0), "key flag set": field(0, 1, "flags", 1 | 2 | 4 | K),
        "segment table": field(0, 0, "seg_end", 1), "segment count": desc_field(0, "nsegs", 1),
        "tasks out of order": desc_field(1, "task0", 0), "task count": desc_field(0, "ntasks", 1),
        "canvases overlap": desc_field(1, "dst", 64), "canvas off the element size": desc_field(0, "dst", 66),
        "records off 8 bytes": desc_field(0, "frames", 4), "no host records": desc_field(0, "h_frames", None),
        "no frames": desc_field(1, "nframes", 0), "canvas of 0": desc_field(1, "width", 0),
    }
    for why, m in bad.items():
        with pytest.raises(ValueError):
            vp8g.gpu_anim_compose([a, b], opt, 4, mutate=m)
            pytest.fail(why)
    for shift in ((4, 0), (0, 2)):  # the source off 8 bytes, the output off the element size
        with pytest.raises(ValueError):
            vp8g.gpu_anim_compose([a, b], opt, 4, ptr_shift=shift)
    with pytest.raises(ValueError):
        vp8g.gpu_anim_compose([a, b], opt, 5)
    # vp8g_make_anim_desc refuses the same rectangles
    with pytest.raises(ValueError):
        vp8g.gpu_anim_compose([(12, 8, [frame(rng, 8, 2, 6, 4)])], opt, 4)
    with pytest.raises(ValueError):
        vp8g.gpu_anim_compose([(12, 8, [dict(frame(rng, 2, 2, 6, 4), x=3)])], opt, 4)


def groups_by_canvas(golden):
    groups = {}
    for name, e in sorted(golden["files"].items()):
        if e["accepts"] and e.get("decodes") and "divergence" not in e:
            groups.setdefault(tuple(e["canvas"]), []).append(name)
    return groups


def test_end_to_end_equals_libwebp(vp8g, golden):
    """Every fixture libwebp decodes, one call per canvas size: each slot's RGBA bytes and timestamp are libwebp's."""
    groups = groups_by_canvas(golden)
    assert sum(len(g) for g in groups.values()) >= 15 and (64, 48) in groups and (20, 14) in groups and (1, 1) in groups
    for (cw, ch), names in groups.items():
        out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor([fixture(n) for n in names], vp8g.tensor_opt((cw, ch), "uint8", "NHWC"))
        assert st == [0] * len(names), (names, st)
        host = out.cpu().numpy()
        assert host.shape == (sum(golden["files"][n]["nframes"] for n in names), ch, cw, 4)
        for n, f0 in zip(names, first):
            for k, fr in enumerate(golden["files"][n]["frames"]):
                assert hashlib.sha256(host[f0 + k].tobytes()).hexdigest() == fr["rgba"], (n, k)
                assert ts[f0 + k] == fr["timestamp"], (n, k)


def test_end_to_end_other_tensor_forms(vp8g):
    """The mixed lossy / lossless animation as normalised float16 NCHW RGB and as float32 NHWC BGRA, against the host's
    frames, compositor and tensor arithmetic."""
    data = fixture("mixed")
    (cw, ch), frames, _ = vp8g.host_anim_frames(data)
    want, _ = vp8g.host_anim_compose(cw, ch, frames)
    for opt, alpha in ((vp8g.tensor_opt((cw, ch), "float16", "NCHW", mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]), False),
                       (vp8g.tensor_opt((cw, ch), "float32", "NHWC", scale=1 / 255, bgr=True), True)):
        out, first, _, st = vp8g.gpu_decode_webp_anim_tensor([data], opt, alpha=alpha)
        assert st == [0] and first == [0] and out.shape[0] == len(frames)
        for k in range(len(frames)):
            exp = vp8g.host_tensor_argb(want[k], opt, 4 if alpha else 3)
            assert torch.equal(out[k].cpu().view(torch.uint8), exp.view(torch.uint8)), k


def test_batch_of_good_and_bad_files(vp8g, golden):
    """Statuses per file, zero slots for the files that fail after the container, no slots for what is no animation, and
    the good files' slots exact."""
    names = ["c_chunks_between", "bad_truncated", "bad_frame_stream", "rules_a", "still_vp8x", "c_riff_small", "bad_no_frames"]
    out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor([fixture(n) for n in names], vp8g.tensor_opt((16, 12), "uint8", "NHWC"), prefill=0xAB)
    E = errno.EINVAL
    assert st == [0, E, E, E, E, 0, E]
    assert first == [0, 2, 2, 4, 18, 18, 20] and out.shape[0] == 20
    host = out.cpu().numpy()
    for n, f0 in ((names[0], 0), (names[5], 18)):
        for k, fr in enumerate(golden["files"][n]["frames"]):
            assert hashlib.sha256(host[f0 + k].tobytes()).hexdigest() == fr["rgba"], (n, k)
            assert ts[f0 + k] == fr["timestamp"]
    assert not host[2:18].any()  # a frame that does not decode; a canvas of another size
    info, ist = vp8g.anim_info([fixture(n) for n in names])
    assert [i["nframes"] for i in info] == [2, 0, 2, 14, 0, 2, 0] and ist == [0, E, 0, 0, E, 0, E]
    assert info[3] == {"canvas": [20, 14], "nframes": 14, "loop_count": 3}
