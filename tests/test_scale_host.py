"""CPU tests of the crop + downscale path's host side (host/vp8_scale.c): the sequential
restatement of libwebp's rescaler against libwebp's own bytes (tests/golden/scale.json, generated
by tests/golden/make_scale_golden.py), option resolution, and the loop-filter rule.

Bar: byte equality (pinned by sha256 of libwebp 1.2.2's output)."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

from conftest import FIXTURES, GOLDEN

EINVAL = 22


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "scale.json").read_text())


def plane_input(kind, w, h, seed):
    """The generators scale.json records ("inputs")."""
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "binary":
        return (np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8) * np.uint8(255)).tobytes()
    assert kind == "ones"
    return bytes([255]) * n


def test_golden_covers_the_listed_cases(golden):
    pairs = {(tuple(c["src"]), tuple(c["dst"])) for c in golden["planes"]}
    assert len(pairs) == 22 and ((8192, 2100), (1, 1)) in pairs and ((16383, 2), (5, 1)) in pairs
    assert {c["kind"] for c in golden["planes"]} == {"random", "ones", "binary"}
    assert len(golden["decode"]) == 20


def test_host_scale_planes_vs_libwebp(vp8g, golden):
    """vp8f_scale_i420 vs WebPPictureRescale: random, all-255 and 0/255 planes, 1x1 up to both
    maximum dimensions and an accumulator that wraps 2^32."""
    bad = []
    for c in golden["planes"]:
        (W, H), (w, h) = c["src"], c["dst"]
        out, ow, oh = vp8g.host_scale(plane_input(c["kind"], W, H, c["seed"]), W, H, vp8g.scale_opt(scale=(w, h)))
        if (ow, oh) != (w, h) or sha(out) != c["sha256"]:
            bad.append((W, H, w, h, c["kind"]))
    assert not bad, bad


def test_host_scale_decode_vs_libwebp(vp8g, golden):
    """Host front end + oracle reconstruction + vp8f_scale_i420 vs WebPDecode(use_cropping /
    use_scaling): bypass_filtering = 1 is the unfiltered decode, 0 follows libwebp's filter rule."""
    bad = []
    frames = {}
    for c in golden["decode"]:
        f = frames.get(c["file"]) or frames.setdefault(c["file"], vp8g.decode_file(FIXTURES / c["file"]))
        opt = vp8g.scale_opt(crop=c["crop"], scale=c["scale"], dwebp_filter=True)
        filt = vp8g.host_lib().vp8f_scale_filtered(f.width, f.height, C.byref(opt), int(not c["bypass"]))
        out, ow, oh = vp8g.host_scale(vp8g.oracle_reconstruct(f, bool(filt)), f.width, f.height, opt)
        if [ow, oh] != c["size"] or sha(out) != c["sha256"]:
            bad.append((c["file"], c["crop"], c["scale"], c["bypass"]))
    for f in frames.values():
        f.free()
    assert not bad, bad


def test_identity_is_a_copy(vp8g):
    b = plane_input("random", 37, 21, 3)
    assert vp8g.host_scale(b, 37, 21, vp8g.scale_opt()) == (b, 37, 21)


def test_target_size_ceiling_rule(vp8g):
    assert vp8g.scaled_size(1920, 1080, vp8g.scale_opt(scale=(100, 0))) == (100, 57)
    assert vp8g.scaled_size(1920, 1080, vp8g.scale_opt(scale=(0, 100))) == (178, 100)
    assert vp8g.scaled_size(1920, 1080, vp8g.scale_opt(scale=(101, 0))) == (101, 57)
    assert vp8g.scaled_size(1920, 1080, vp8g.scale_opt()) == (1920, 1080)
    # the derived dimension comes from the cropped window
    assert vp8g.scaled_size(333, 200, vp8g.scale_opt(crop=(3, 5, 101, 99), scale=(50, 0))) == (50, 50)
    assert vp8g.scaled_size(333, 200, vp8g.scale_opt(crop=(3, 5, 101, 99))) == (101, 99)


def test_odd_crop_origin_snaps_down_to_even(vp8g):
    g = vp8g.Vp8fScaleGeom()
    opt = vp8g.scale_opt(crop=(3, 5, 101, 99))
    assert vp8g.host_lib().vp8f_scale_resolve(333, 200, C.byref(opt), C.byref(g)) == 0
    assert (g.left, g.top, g.win_w, g.win_h, g.out_w, g.out_h, g.scaling) == (2, 4, 101, 99, 101, 99, 0)
    # and the pixels are those of the window at the even origin
    w, h = 33, 21
    src = plane_input("random", w, h, 9)
    a = np.frombuffer(src, np.uint8)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    Y, U, V = a[:w * h].reshape(h, w), a[w * h:w * h + cw * ch].reshape(ch, cw), a[w * h + cw * ch:].reshape(ch, cw)
    out, ow, oh = vp8g.host_scale(src, w, h, vp8g.scale_opt(crop=(3, 5, 10, 7)))
    exp = Y[4:11, 2:12].tobytes() + U[2:6, 1:6].tobytes() + V[2:6, 1:6].tobytes()
    assert (ow, oh) == (10, 7) and out == exp


@pytest.mark.parametrize("opt", [
    dict(scale=(1921, 0)), dict(scale=(0, 1081)), dict(scale=(1921, 1080)), dict(scale=(1920, 1081)),
    dict(scale=(100, 1081)), dict(crop=(0, 0, 0, 50)), dict(crop=(0, 0, 50, 0)), dict(crop=(10, 10, 0, 0)),
    dict(crop=(0, 0, 1921, 1080)), dict(crop=(1, 0, 1920, 1080)), dict(crop=(0, 1, 1920, 1080)),
    dict(crop=(0, 0, 100, 100), scale=(101, 50)), dict(crop=(0, 0, 100, 100), scale=(50, 101)),
])
def test_invalid_options_are_einval(vp8g, opt):
    lib = vp8g.host_lib()
    g = vp8g.Vp8fScaleGeom()
    o = vp8g.scale_opt(**opt)
    C.set_errno(0)
    assert lib.vp8f_scale_resolve(1920, 1080, C.byref(o), C.byref(g)) == -1 and C.get_errno() == EINVAL
    glib = vp8g.gpu_lib()  # (host code of libvp8g.so: no device call)
    ow, oh, d = C.c_uint32(0), C.c_uint32(0), vp8g.Vp8gScaleDesc()
    C.set_errno(0)
    assert glib.vp8g_scaled_size(1920, 1080, C.byref(o), C.byref(ow), C.byref(oh)) == -1 and C.get_errno() == EINVAL
    C.set_errno(0)
    assert glib.vp8g_make_scale_desc(1920, 1080, 0, 1920 * 1080, 1920 * 1080 + 960 * 540, 1920, 960, C.byref(o), 0, 0,
                                     C.byref(d)) == -1 and C.get_errno() == EINVAL


def test_null_and_malformed_arguments_are_einval(vp8g):
    lib, glib = vp8g.host_lib(), vp8g.gpu_lib()
    g, o = vp8g.Vp8fScaleGeom(), vp8g.scale_opt(scale=(10, 10))
    ow, oh, d = C.c_uint32(0), C.c_uint32(0), vp8g.Vp8gScaleDesc()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    calls = [
        lambda: lib.vp8f_scale_resolve(100, 100, None, C.byref(g)),
        lambda: lib.vp8f_scale_resolve(100, 100, C.byref(o), None),
        lambda: lib.vp8f_scale_resolve(0, 100, C.byref(o), C.byref(g)),
        lambda: lib.vp8f_scale_resolve(16384, 100, C.byref(o), C.byref(g)),
        lambda: lib.vp8f_scale_resolve(100, 100, C.byref(vp8g.Vp8gScaleOpt(0, 0, 0, 0, 10, 10, 2)), C.byref(g)),
        lambda: lib.vp8f_scale_i420(None, p, p, 4, 2, 4, 4, C.byref(o), p, p, p, 4, 2),
        lambda: lib.vp8f_scale_i420(p, p, p, 4, 2, 4, 4, None, p, p, p, 4, 2),
        lambda: lib.vp8f_scale_i420(p, p, p, 3, 2, 4, 4, C.byref(vp8g.scale_opt()), p, p, p, 4, 2),
        lambda: glib.vp8g_scaled_size(100, 100, None, C.byref(ow), C.byref(oh)),
        lambda: glib.vp8g_scaled_size(100, 100, C.byref(o), None, C.byref(oh)),
        lambda: glib.vp8g_make_scale_desc(100, 100, 0, 10000, 12500, 100, 50, None, 0, 0, C.byref(d)),
        lambda: glib.vp8g_make_scale_desc(100, 100, 0, 10000, 12500, 100, 50, C.byref(o), 0, 0, None),
        lambda: glib.vp8g_make_scale_desc(100, 100, 0, 10000, 12500, 99, 50, C.byref(o), 0, 0, C.byref(d)),
        lambda: glib.vp8g_scale_batch_device(None, None, 1, None, None, None),
        lambda: glib.yuv420_rescale(None, C.byref(o), C.byref(vp8g.Yuv420Image())),
        lambda: glib.yuv420_rescale(C.byref(vp8g.Yuv420Image()), None, C.byref(vp8g.Yuv420Image())),
        lambda: glib.vp8g_decode_webp_batch_scaled(None, 1, 1, 0, 0, C.byref(o), 1, None, None),
    ]
    for i, call in enumerate(calls):
        C.set_errno(0)
        assert call() == -1 and C.get_errno() == EINVAL, i


# (W, H, scaled_w, scaled_h) -> does a `filtered` request with VP8G_SCALE_DWEBP_FILTER filter?
FILTER_RULE = [
    (2093, 2500, 224, 224, 0), (2093, 2500, 2000, 2400, 1), (2093, 2500, 1600, 300, 1),
    (1920, 1080, 1440, 810, 1),  # the inequality is strict
    (1920, 1080, 1439, 809, 0), (1920, 1080, 1439, 810, 1), (1920, 1080, 1440, 809, 1),
]


@pytest.mark.parametrize("W,H,w,h,filt", FILTER_RULE)
def test_dwebp_filter_rule(vp8g, W, H, w, h, filt):
    lib = vp8g.host_lib()
    flag, plain = vp8g.scale_opt(scale=(w, h), dwebp_filter=True), vp8g.scale_opt(scale=(w, h))
    assert lib.vp8f_scale_filtered(W, H, C.byref(flag), 1) == filt
    assert lib.vp8f_scale_filtered(W, H, C.byref(plain), 1) == 1  # without the flag, filtered means filtered
    assert lib.vp8f_scale_filtered(W, H, C.byref(flag), 0) == 0 and lib.vp8f_scale_filtered(W, H, C.byref(plain), 0) == 0


def test_dwebp_filter_rule_uses_the_full_picture_and_only_when_scaling(vp8g):
    lib = vp8g.host_lib()
    # a small crop of a large picture, scaled by less than 3/4 of the crop but far below 3/4 of the picture
    o = vp8g.scale_opt(crop=(0, 0, 100, 100), scale=(90, 90), dwebp_filter=True)
    assert lib.vp8f_scale_filtered(1920, 1080, C.byref(o), 1) == 0
    # crop only: no scaling, so filtered stays filtered
    o = vp8g.scale_opt(crop=(0, 0, 100, 100), dwebp_filter=True)
    assert lib.vp8f_scale_filtered(1920, 1080, C.byref(o), 1) == 1


def test_scale_desc_geometry(vp8g):
    """vp8g_make_scale_desc: plane windows, factors and a tiling that covers every output sample."""
    lib = vp8g.gpu_lib()
    d = vp8g.Vp8gScaleDesc()
    o = vp8g.scale_opt(crop=(3, 5, 101, 77), scale=(50, 0))
    W, H, sy, suv = 333, 97, 340, 170
    assert lib.vp8g_make_scale_desc(W, H, 1000, 50000, 70000, sy, suv, C.byref(o), 4096, 7, C.byref(d)) == 0
    assert (d.width, d.height, d.task0, d.crop_left, d.crop_top) == (50, 39, 7, 2, 4)
    y, u, v = d.p[0], d.p[1], d.p[2]
    assert (y.src, y.src_w, y.src_h, y.dst_w, y.dst_h, y.dst) == (1000 + 4 * sy + 2, 101, 77, 50, 39, 4096)
    assert (u.src, u.src_w, u.src_h, u.dst_w, u.dst_h, u.dst) == (50000 + 2 * suv + 1, 51, 39, 25, 20, 4096 + 50 * 39)
    assert (v.src, v.dst) == (70000 + 2 * suv + 1, 4096 + 50 * 39 + 25 * 20)
    assert (y.fx, y.fy) == ((1 << 32) // 50, (1 << 32) // 39) and y.fxy == (39 << 32) // (101 * 77)
    assert d.ntasks == y.ntasks + u.ntasks + v.ntasks
    for p in (y, u, v):
        assert p.tile_w * p.group == 256 and p.tiles_x * p.tile_w >= p.dst_w
        assert p.ntasks == p.tiles_x * -(-p.dst_h // p.run_h) and p.pitch * p.block_rows <= 16448
