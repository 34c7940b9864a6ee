"""Animated files decoded to a target size on the device, bit for bit.

The fused kernel (vp8g_scale_argb_tensor_batch_device: crop + shrink of ARGB straight into tensor elements) against
host_tensor_argb(host_scale_argb(...)) on seeded random pictures, its maker's verdicts and the entry point's checks; then
vp8g_decode_webp_anim_tensor_scaled on the fixtures of tests/golden/anim/ against libwebp's scaled canvases
(tests/golden/anim_scale.json) -- the shrinking cases through the fused kernel, the expanding and crop-only ones through
the planar fall-back."""
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
ALPHAS = np.array([0, 1, 2, 127, 128, 254, 255], np.uint32)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "anim_scale.json").read_text())


@pytest.fixture(scope="module")
def anim_doc():
    return json.loads((GOLDEN / "anim.json").read_text())["files"]


def fixture(name):
    return (ANIM / f"{name}.webp").read_bytes()


def picture(rng, w, h):
    """uint32 [h, w] 0xAARRGGBB: random colour (also under alpha 0); alpha from ALPHAS for half the pixels, uniform bytes
    for the rest."""
    a = np.where(rng.integers(0, 2, (h, w)) == 0, ALPHAS[rng.integers(0, len(ALPHAS), (h, w))], rng.integers(0, 256, (h, w), dtype=np.uint32))
    return rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) | a.astype(np.uint32) << 24


def opt_of(vp8g, c):
    return vp8g.scale_opt(crop=tuple(c["crop"]), scale=tuple(c["scale"]), expand=c["expand"])


def check(vp8g, pics, opts, topt=None, channels=4, **kw):
    """One launch over `pics`; every slot equals the host's scaled picture as a tensor (uint8 / NHWC / RGBA by default)."""
    topt = topt or vp8g.tensor_opt((1, 1), "uint8", "NHWC")
    got = vp8g.gpu_scale_argb_tensor(pics, opts, topt, channels, **kw)
    for i, (a, o) in enumerate(zip(pics, opts)):
        want = vp8g.host_scale_argb(a, o)
        t = vp8g.Vp8gTensorOpt.from_buffer_copy(topt)
        t.width, t.height = want.shape[1], want.shape[0]
        exp = vp8g.host_tensor_argb(want, t, channels)
        assert got[i].shape == exp.shape and got[i].dtype == exp.dtype, (i, a.shape)
        assert torch.equal(got[i].view(torch.uint8), exp.view(torch.uint8)), (i, a.shape, [getattr(o, n) for n, _ in o._fields_])


def test_widths_around_the_load_and_the_tile(vp8g):
    """Window widths g - 1, g, g + 1 and 2 g for g = the pixels of one 16-byte load, and target widths around a task's
    columns (one lane per column: 256), so that rows end inside, on and just past a load and a tile."""
    g, max_seg, run_rows = vp8g.scale_argb_fused_geometry()
    assert g == 4 and max_seg >= 3000 and run_rows >= 2
    rng = np.random.default_rng(1)
    pics, opts = [], []
    for W in (g - 1, g, g + 1, 2 * g):
        for w in sorted({1, W - 1, W} - {0}):
            pics.append(picture(rng, W, 5)), opts.append(vp8g.scale_opt(scale=(w, 3)))
    tile = 256
    for w in (tile - 1, tile, tile + 1, 2 * tile):
        pics.append(picture(rng, w + 3, 4)), opts.append(vp8g.scale_opt(scale=(w, 3)))
        pics.append(picture(rng, 2 * w, 2)), opts.append(vp8g.scale_opt(scale=(w, 1)))
    for o, a in zip(opts, pics):
        assert vp8g.make_scale_argb_tensor_desc(a.shape[1], a.shape[0], o).group == 1
    check(vp8g, pics, opts)


def test_every_source_and_window_phase(vp8g):
    """The source at every dword phase of a 16-byte boundary, the window's origin at every phase (odd origins included),
    windows that end at the picture's last pixel."""
    rng = np.random.default_rng(2)
    a = picture(rng, 41, 19)
    for shift in range(4):
        opts = [vp8g.scale_opt(crop=(left, top, 41 - left - right, 19 - top), scale=(11, 5))
                for left in range(4) for top in (0, 1) for right in (0, 1)]
        check(vp8g, [a] * len(opts), opts, src_shift=shift)


def test_ratios(vp8g):
    """A target equal to the window (not the identity), W -> W - 1, 2 : 1, 17 : 1 (two lanes per column), 3000 x 3 -> 1 x 1
    (64 lanes on one column), 1 x 1 -> 1 x 1, and the longest segment the kernel stages."""
    _, max_seg, _ = vp8g.scale_argb_fused_geometry()
    rng = np.random.default_rng(3)
    cases = [((37, 23), None, (37, 23)), ((37, 23), None, (36, 22)), ((64, 30), None, (32, 15)), ((170, 34), None, (10, 2)),
             ((3000, 3), None, (1, 1)), ((1, 1), None, (1, 1)), ((300, 40), (3, 1, 290, 37), (0, 9)), ((max_seg, 2), None, (1, 1)),
             ((1000, 2), None, (3, 2)), ((1, 9), None, (1, 4)), ((9, 1), None, (4, 1)), ((1, 5), None, (1, 5))]
    pics = [picture(rng, w, h) for (w, h), _, _ in cases]
    opts = [vp8g.scale_opt(crop=c, scale=s) for _, c, s in cases]
    groups = [vp8g.make_scale_argb_tensor_desc(a.shape[1], a.shape[0], o).group for a, o in zip(pics, opts)]
    assert groups[3] == 2 and groups[4] == 64 and groups[7] == 64 and groups[8] == 32 and groups[0] == 1
    same = vp8g.host_scale_argb(pics[0], opts[0])
    assert same.shape == pics[0].shape and not np.array_equal(same, pics[0])
    check(vp8g, pics, opts)          # a mixed batch of sizes, windows and targets in one launch
    for a, o in list(zip(pics, opts))[:5]:
        check(vp8g, [a], [o])        # and alone


def test_runs_and_the_boundary_row(vp8g):
    """Heights that take several runs, so that a run starts with the boundary row of the run above: 5 x 700 -> 5 x 3 (one
    output row per run), and heights of three and more runs with whole and fractional row ratios."""
    _, _, run_rows = vp8g.scale_argb_fused_geometry()
    rng = np.random.default_rng(4)
    cases = [((5, 700), (5, 3)), ((40, 4 * run_rows + 7), (20, 2 * run_rows + 1)), ((9, 3 * run_rows), (9, 3 * run_rows)),
             ((7, 5 * run_rows + 3), (3, 5 * run_rows + 2)), ((6, 8 * run_rows), (6, 16))]
    pics = [picture(rng, w, h) for (w, h), _ in cases]
    opts = [vp8g.scale_opt(scale=s) for _, s in cases]
    for a, o in zip(pics, opts):
        d = vp8g.make_scale_argb_tensor_desc(a.shape[1], a.shape[0], o)
        assert d.ntasks >= 3 * d.tiles_x
    check(vp8g, pics, opts)


TENSOR_FORMS = list(itertools.product(("uint8", "float16", "bfloat16", "float32"), ("NHWC", "NCHW"), (False, True), (3, 4)))


@pytest.mark.parametrize("dtype,layout,bgr,channels", TENSOR_FORMS)
def test_every_tensor_form(vp8g, dtype, layout, bgr, channels):
    """One picture (an odd target width: rows off the dword boundary for the narrow types; quads and a ragged end; two
    lanes per column beside it) through every dtype, layout, channel order and channel count."""
    rng = np.random.default_rng(5)
    pics = [picture(rng, 45, 23), picture(rng, 150, 9)]
    opts = [vp8g.scale_opt(crop=(1, 3, 41, 19), scale=(13, 7)), vp8g.scale_opt(scale=(7, 3))]
    topt = vp8g.tensor_opt((1, 1), dtype, layout, scale=[1 / 255, 0.5, 3.0], bias=[-0.5, 0.25, 1e-3], bgr=bgr)
    check(vp8g, pics, opts, topt, channels, guard=8)


def test_makers_verdicts(vp8g):
    _, max_seg, _ = vp8g.scale_argb_fused_geometry()
    ok = vp8g.make_scale_argb_tensor_desc(67, 45, vp8g.scale_opt(crop=(3, 5, 31, 22), scale=(9, 22)))
    assert (ok.crop_left, ok.crop_top, ok.win_w, ok.win_h, ok.width, ok.height) == (3, 5, 31, 22, 9, 22)
    # the lossy path's filter flag means nothing here
    vp8g.make_scale_argb_tensor_desc(67, 45, vp8g.scale_opt(scale=(9, 22), dwebp_filter=True))
    not_fused = [vp8g.scale_opt(scale=(68, 45), expand=True), vp8g.scale_opt(scale=(67, 46), expand=True), vp8g.scale_opt(scale=(20, 90), expand=True),
                 vp8g.scale_opt(crop=(3, 5, 31, 22)), vp8g.scale_opt()]
    for o in not_fused:
        with pytest.raises(OSError) as ei:
            vp8g.make_scale_argb_tensor_desc(67, 45, o)
        assert ei.value.errno == errno.ENOTSUP
        vp8g.host_scale_argb(np.zeros((45, 67), np.uint32), o)  # valid options: the planar route takes them
    with pytest.raises(OSError) as ei:  # a row segment beyond the staging
        vp8g.make_scale_argb_tensor_desc(max_seg + 1, 2, vp8g.scale_opt(scale=(1, 1)))
    assert ei.value.errno == errno.ENOTSUP
    invalid = [vp8g.scale_opt(crop=(60, 0, 8, 10), scale=(4, 4)), vp8g.scale_opt(crop=(0, 40, 8, 6), scale=(4, 4)),
               vp8g.scale_opt(scale=(68, 45)), vp8g.scale_opt(crop=(3, 5, 0, 10))]
    for o in invalid:
        with pytest.raises(OSError) as ei:
            vp8g.make_scale_argb_tensor_desc(67, 45, o)
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:  # a source off a dword
        vp8g.make_scale_argb_tensor_desc(67, 45, vp8g.scale_opt(scale=(9, 22)), src=2)
    assert ei.value.errno == errno.EINVAL


def test_bad_descriptors_are_refused_before_launch(vp8g):
    rng = np.random.default_rng(6)
    pics = [picture(rng, 37, 23), picture(rng, 64, 30)]
    opts = [vp8g.scale_opt(crop=(1, 1, 33, 21), scale=(11, 7)), vp8g.scale_opt(scale=(32, 15))]
    topt = vp8g.tensor_opt((1, 1), "float32", "NHWC")
    check(vp8g, pics, opts, topt)

    def field(i, name, value):
        def m(descs):
            setattr(descs[i], name, value(getattr(descs[i], name)) if callable(value) else value)
        return m

    bad = {
        "window beyond the right edge": field(0, "win_w", 37), "window beyond the bottom": field(0, "crop_top", 3),
        "target wider than the window": field(0, "width", 34), "target of 0": field(1, "height", 0),
        "fx": field(0, "fx", lambda v: v + 1), "fy": field(1, "fy", 0), "fxy": field(0, "fxy", lambda v: v - 1),
        "group": field(0, "group", 2), "tile": field(1, "tile_w", 128), "run": field(0, "run_h", lambda v: v + 1),
        "tiles": field(1, "tiles_x", 2), "pitch": field(0, "pitch", lambda v: v + 16), "block rows": field(1, "block_rows", lambda v: v + 1),
        "tasks out of order": field(1, "task0", 0), "task count": field(0, "ntasks", lambda v: v + 1), "reserved": field(1, "reserved", 1),
        "source off a dword": field(0, "src", lambda v: v + 2), "slot off the element size": field(1, "dst", lambda v: v + 2),
        "slots overlap": field(1, "dst", 64), "picture narrower than the window": field(0, "src_width", 33),
    }
    for why, m in bad.items():
        with pytest.raises(ValueError):
            check(vp8g, pics, opts, topt, mutate=m)
            pytest.fail(why)
    for shift in ((2, 0, 0), (0, 2, 0), (0, 0, 4)):  # the source off a dword, the output off the element size, the descriptors off 8
        with pytest.raises(ValueError):
            check(vp8g, pics, opts, topt, ptr_shift=shift)
    with pytest.raises(ValueError):
        check(vp8g, pics, opts, topt, channels=5)


# ---- end to end ---------------------------------------------------------------------------------

def fused(vp8g, c, anim_doc) -> bool:
    """Whether the entry sends this golden case through the fused kernel (its maker's verdict), else the planar route."""
    try:
        vp8g.make_scale_argb_tensor_desc(*anim_doc[c["file"]]["canvas"], opt_of(vp8g, c))
        return True
    except OSError as e:
        assert e.errno == errno.ENOTSUP
        return False


def test_end_to_end_equals_libwebp(vp8g, golden, anim_doc):
    """Every case of anim_scale.json, one call per target size (files of different canvases share a tensor): each slot's
    RGBA bytes are libwebp's and each timestamp anim.json's."""
    by_size, routes = {}, {True: 0, False: 0}
    for c in golden["cases"]:
        by_size.setdefault(tuple(c["size"]), []).append(c)
        is_fused = fused(vp8g, c, anim_doc)
        routes[is_fused] += 1
        ww, wh = (c["crop"][2], c["crop"][3]) if any(c["crop"]) else anim_doc[c["file"]]["canvas"]
        assert is_fused == (any(c["scale"]) and c["size"][0] <= ww and c["size"][1] <= wh), c
    assert routes[True] >= 20 and routes[False] >= 15
    for (w, h), cases in by_size.items():
        out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor([fixture(c["file"]) for c in cases], vp8g.tensor_opt((w, h), "uint8", "NHWC"),
                                                              scale=[opt_of(vp8g, c) for c in cases])
        assert st == [0] * len(cases), (w, h, st)
        host = out.cpu().numpy()
        assert host.shape == (sum(len(c["rgba"]) for c in cases), h, w, 4)
        for c, f0 in zip(cases, first):
            for k, want in enumerate(c["rgba"]):
                assert hashlib.sha256(host[f0 + k].tobytes()).hexdigest() == want, (c["file"], c["crop"], c["scale"], k)
                assert ts[f0 + k] == anim_doc[c["file"]]["frames"][k]["timestamp"]


def test_canvases_of_different_sizes_share_one_tensor(vp8g, golden, anim_doc):
    """20 x 14 and 64 x 48 animations and one file whose frame does not decode into one 16 x 12 float16 NCHW tensor: statuses,
    zero slots, the good files' elements; the same call as uint8 RGBA gives libwebp's bytes."""
    names = ["rules_a", "bad_frame_stream", "mixed"]
    files = [fixture(n) for n in names]
    scale = vp8g.scale_opt(scale=(16, 12))
    topt = vp8g.tensor_opt((16, 12), "float16", "NCHW", mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor(files, topt, scale=scale, prefill=3.0)
    assert st == [0, errno.EINVAL, 0] and first == [0, 14, 16] and out.shape == (24, 4, 12, 16) and out.dtype == torch.float16
    host = out.cpu()
    assert not host[14:16].view(torch.uint8).any()
    for n, f0 in ((names[0], 0), (names[2], 16)):
        want, wts = vp8g.host_anim_scaled(fixture(n), scale)
        for k in range(len(want)):
            assert torch.equal(host[f0 + k].view(torch.uint8), vp8g.host_tensor_argb(want[k], topt, 4).view(torch.uint8)), (n, k)
        assert ts[f0:f0 + len(want)] == wts
    u8, first, _, st = vp8g.gpu_decode_webp_anim_tensor(files, vp8g.tensor_opt((16, 12), "uint8", "NHWC"), scale=scale)
    u8 = u8.cpu().numpy()
    for n, f0 in ((names[0], 0), (names[2], 16)):
        c, = [c for c in golden["cases"] if c["file"] == n and c["scale"] == [16, 12] and not any(c["crop"])]
        assert [hashlib.sha256(u8[f0 + k].tobytes()).hexdigest() for k in range(len(c["rgba"]))] == c["rgba"]
    # three channels: alpha dropped after the un-premultiply
    rgb, _, _, st = vp8g.gpu_decode_webp_anim_tensor(files, vp8g.tensor_opt((16, 12), "uint8", "NHWC"), alpha=False, scale=scale)
    assert st == [0, errno.EINVAL, 0] and np.array_equal(rgb.cpu().numpy(), u8[..., :3])


def test_staging_groups_do_not_change_the_output(vp8g):
    """stage_bytes small enough to force one animation per group, and routes mixed within the call (fused, planar: an
    expanding and a crop-only option, and direct), against the default's bytes."""
    names = ["rules_a", "mixed", "rules_b", "one_frame", "rules_a"]
    files = [fixture(n) for n in names]
    scale = [vp8g.scale_opt(scale=(20, 14)), vp8g.scale_opt(crop=(3, 1, 20, 14)), vp8g.scale_opt(crop=(1, 1, 10, 7), scale=(20, 14), expand=True),
             vp8g.scale_opt(scale=(20, 14)), vp8g.scale_opt()]
    topt = vp8g.tensor_opt((20, 14), "float32", "NHWC", scale=1 / 255)
    a, first, ts, st = vp8g.gpu_decode_webp_anim_tensor(files, topt, scale=scale)
    b, first_b, ts_b, st_b = vp8g.gpu_decode_webp_anim_tensor(files, topt, scale=scale, stage_bytes=1)
    assert st == st_b == [0] * 5 and first == first_b and ts == ts_b
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    host = a.cpu()
    for n, o, f0 in zip(names, scale, first):
        want, _ = vp8g.host_anim_scaled(fixture(n), o)
        for k in range(len(want)):
            assert torch.equal(host[f0 + k].view(torch.uint8), vp8g.host_tensor_argb(want[k], topt, 4).view(torch.uint8)), (n, k)


def test_every_route_and_every_failure_in_one_call(vp8g, anim_doc):
    """A direct, a fused and a planar (VP8G_SCALE_EXPAND) file, a file whose option does not give the tensor's size, a still
    picture and a file with a corrupt frame payload in one call into a prefilled 16 x 12 tensor: in file order and in
    reverse, one animation per staging group (stage_bytes = 1) and with the default cap.  Every file's slots, timestamps
    and status are those of the same file decoded alone; a failed file's slots are zero."""
    E = errno.EINVAL
    cases = [("c_chunks_between", vp8g.scale_opt(), 0), ("mixed", vp8g.scale_opt(scale=(16, 12)), 0),
             ("transparent_colour", vp8g.scale_opt(scale=(16, 12), expand=True), 0), ("alpha_bit_cleared", vp8g.scale_opt(scale=(10, 8)), E),
             ("still_vp8x", vp8g.scale_opt(), E), ("bad_frame_stream", vp8g.scale_opt(), E)]
    assert anim_doc["c_chunks_between"]["canvas"] == [16, 12] and anim_doc["bad_frame_stream"]["decodes"] is False
    vp8g.make_scale_argb_tensor_desc(*anim_doc["mixed"]["canvas"], cases[1][1])  # the fused kernel's
    with pytest.raises(OSError) as ei:
        vp8g.make_scale_argb_tensor_desc(*anim_doc["transparent_colour"]["canvas"], cases[2][1])
    assert ei.value.errno == errno.ENOTSUP  # the planar route's
    topt = vp8g.tensor_opt((16, 12), "uint8", "NHWC")
    alone = {}
    for name, o, e in cases:
        out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor([fixture(name)], topt, scale=[o], prefill=0xAB)
        assert st == [e] and first == [0], name
        assert len(out) == (0 if name == "still_vp8x" else anim_doc[name]["nframes"]), name
        if e:
            assert not out.any(), name
        else:
            assert ts == [f["timestamp"] for f in anim_doc[name]["frames"]], name
        alone[name] = (out.cpu(), ts)
    assert not torch.equal(alone["mixed"][0][0], alone["mixed"][0][1])  # (canvases that differ: a slot out of place shows)
    for order in (cases, cases[::-1]):
        want_first = list(itertools.accumulate([0] + [len(alone[name][0]) for name, _, _ in order]))[:-1]
        for stage_bytes in (1, 0):
            out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor([fixture(name) for name, _, _ in order], topt, scale=[o for _, o, _ in order],
                                                                  prefill=0xAB, stage_bytes=stage_bytes)
            assert st == [e for _, _, e in order] and first == want_first, (stage_bytes, st, first)
            host = out.cpu()
            for (name, _, e), f0 in zip(order, first):
                want, wts = alone[name]
                assert torch.equal(host[f0:f0 + len(want)], want), (name, stage_bytes)
                assert ts[f0:f0 + len(want)] == wts, (name, stage_bytes)
                assert not (e and host[f0:f0 + len(want)].any()), (name, stage_bytes)


def test_identity_on_a_matching_canvas_is_the_unscaled_entry(vp8g):
    files = [fixture("rules_a"), fixture("rules_b")]
    topt = vp8g.tensor_opt((20, 14), "bfloat16", "NCHW", scale=1 / 255)
    want, first, ts, st = vp8g.gpu_decode_webp_anim_tensor(files, topt)
    for scale in (vp8g.scale_opt(), [vp8g.scale_opt(), vp8g.scale_opt(crop=(0, 0, 20, 14))]):
        got, first_s, ts_s, st_s = vp8g.gpu_decode_webp_anim_tensor(files, topt, scale=scale)
        assert st == st_s == [0, 0] and first == first_s and ts == ts_s
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_options_that_do_not_fit_fail_their_file_only(vp8g, golden):
    """The golden's refusals, a result that is not the tensor's size, a canvas that does not match without an option: EINVAL
    and zero slots for that file, the others exact."""
    files = [fixture("rules_a"), fixture("rules_a"), fixture("mixed"), fixture("rules_b")]
    r = next(c for c in golden["refusals"] if c["file"] == "rules_a")
    scale = [opt_of(vp8g, r), vp8g.scale_opt(scale=(10, 8)), vp8g.scale_opt(), vp8g.scale_opt(scale=(10, 7))]
    topt = vp8g.tensor_opt((10, 7), "uint8", "NHWC")
    out, first, _, st = vp8g.gpu_decode_webp_anim_tensor(files, topt, scale=scale, prefill=0xAB)
    E = errno.EINVAL
    assert st == [E, E, E, 0] and first == [0, 14, 28, 36]
    host = out.cpu().numpy()
    assert not host[:36].any()
    want, _ = vp8g.host_anim_scaled(files[3], scale[3])
    assert np.array_equal(host[36:], np.stack([vp8g.argb_to_rgba(c) for c in want]))
    lib = vp8g.gpu_lib()
    import ctypes as C
    assert lib.vp8g_decode_webp_anim_tensor_scaled(None, 1, 1, 0, 0, None, 0, 0, C.byref(topt), 4, None, None, None) == -1 and C.get_errno() == E
