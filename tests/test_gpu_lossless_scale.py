"""The device half of the scaled lossless path: vp8g_scale_argb_batch_device -- the split and
merge kernels around the plane rescaler -- against the sequential restatement (vp8f_argb_scale) on random ARGB and
against libwebp on the fixtures (tests/golden/lossless_scale.json); lossless files with a scale option through the
batch pipeline (VP8G_X_LOSSLESS_SCALE).  All comparisons are bit-exact."""
import ctypes as C
import errno
import hashlib
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LOSSLESS = GOLDEN / "lossless"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "lossless_scale.json").read_text())


def fixture(name):
    return (LOSSLESS / f"{name}.webp").read_bytes()


def opt_of(vp8g, c):
    return vp8g.scale_opt(crop=tuple(c["crop"]), scale=tuple(c["scale"]), expand=c["expand"])


def case_of(golden, name, crop=None, scale=None):
    want = (name, list(crop or (0, 0, 0, 0)), list(scale or (0, 0)))
    return next(c for c in golden["cases"] if (c["file"], c["crop"], c["scale"]) == want)


def random_argb(rng, w, h):
    """Uniform colour bytes (not premultiplied: colour may exceed alpha); alpha half uniform, half from the edge values."""
    px = rng.integers(0, 1 << 24, (h, w), dtype=np.uint64).astype(np.uint32)
    edge = rng.choice(np.array([0, 1, 2, 127, 128, 254, 255], np.uint32), (h, w))
    uni = rng.integers(0, 256, (h, w)).astype(np.uint32)
    return px | np.where(rng.integers(0, 2, (h, w)) == 1, edge, uni) << 24


def test_kernels_vs_restatement(vp8g):
    """One launch of mixed pictures: sources at odd dword offsets, guard bytes around every work region and output."""
    S = vp8g.scale_opt
    jobs = [((1, 1), S(scale=(1, 1))), ((1, 1), S(scale=(3, 2), expand=True)), ((5, 3), S(scale=(2, 2))), ((1, 1), S())]
    for w in (3, 4, 5, 15, 16, 17, 63, 64, 65):  # the four-pixel thread, the 16-byte plane row, the wave
        jobs += [((w, 3), S(scale=((w + 1) // 2, 2))), ((w, 3), S(scale=(w + 1, 4), expand=True)), ((w, 3), S(scale=(w, 3))),
                 ((w, 3), S(crop=(1, 1, w - 1, 2)))]
    jobs += [((67, 45), S(scale=(20, 13))), ((67, 45), S(scale=(100, 68), expand=True)), ((257, 70), S(scale=(64, 64))),
             ((257, 70), S(scale=(300, 33), expand=True)), ((257, 70), S(crop=(1, 1, 255, 68)))]
    for left in (0, 1, 2, 3):  # every dword phase of the window's first pixel, an odd top
        jobs += [((67, 45), S(crop=(left, 5, 31, 22), scale=(9, 7))), ((67, 45), S(crop=(left, 7, 33, 21)))]
    # a window that ends at the picture's last column and row; x shrinks while y expands
    jobs += [((67, 45), S(crop=(36, 23, 31, 22), scale=(10, 7))), ((67, 45), S(crop=(36, 23, 31, 22))),
             ((67, 45), S(crop=(3, 5, 31, 22), scale=(9, 30), expand=True))]
    rng = np.random.default_rng(2024)
    pics = [random_argb(rng, w, h) for (w, h), _ in jobs]
    opts = [o for _, o in jobs]
    got = vp8g.gpu_scale_argb(pics, opts, src_shift=1, guard=64)
    for k, (p, o, g) in enumerate(zip(pics, opts, got)):
        want = vp8g.host_scale_argb(p, o)
        assert g.shape == want.shape, (k, jobs[k][0])
        bad = np.argwhere(g != want)
        assert bad.size == 0, (k, jobs[k][0], [getattr(o, n) for n, _ in o._fields_], bad[:4].tolist())
    # the same pictures at the other dword phases of the source
    for shift in (0, 2, 3):
        got = vp8g.gpu_scale_argb(pics[-7:], opts[-7:], src_shift=shift)
        for p, o, g in zip(pics[-7:], opts[-7:], got):
            assert np.array_equal(g, vp8g.host_scale_argb(p, o)), shift


def test_every_alpha_and_colour_pair(vp8g):
    """Every (alpha, colour byte) pair through the one premultiply / un-premultiply of vp8g_scale_device.h: row = alpha,
    column = c, scaled to the picture's own size (still premultiply -> rescale -> un-premultiply), by the planar route at
    every dword phase of the split's 16-byte loads and by the fused kernel.  Expected bytes are the host restatement's."""
    a, c = np.arange(256, dtype=np.uint32)[:, None], np.arange(256, dtype=np.uint32)[None, :]
    pic = a << 24 | ((7 * c + a) & 255) << 16 | (255 - c) << 8 | c
    o = vp8g.scale_opt(scale=(256, 256))
    want = vp8g.host_scale_argb(pic, o)
    # not vacuous: the round trip alone, which changes most pixels and keeps every alpha
    assert np.array_equal(want, vp8g.host_argb_mult(vp8g.host_argb_mult(pic), inverse=True))
    assert (want != pic).mean() > 0.6 and np.array_equal(want >> 24, pic >> 24)
    for shift in range(4):
        (got,) = vp8g.gpu_scale_argb([pic], [o], src_shift=shift)
        assert np.array_equal(got, want), shift
    topt = vp8g.tensor_opt((256, 256), "uint8", "NHWC")
    (t,) = vp8g.gpu_scale_argb_tensor([pic], [o], topt, 4)
    assert torch.equal(t, vp8g.host_tensor_argb(want, topt, 4))


def test_fixtures_equal_libwebps_rgba(vp8g, golden):
    names = sorted({c["file"] for c in golden["cases"]})
    images = []
    for n in names:
        data = fixture(n)
        c = vp8g.parse_any(data)
        images.append(vp8g.lossless_decode_host(data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]))
    argb = dict(zip(names, vp8g.gpu_lossless_argb(images)))
    cases = golden["cases"]
    got = vp8g.gpu_scale_argb([argb[c["file"]] for c in cases], [opt_of(vp8g, c) for c in cases])
    for c, g in zip(cases, got):
        assert list(g.shape[::-1]) == c["size"], c
        assert hashlib.sha256(vp8g.argb_to_rgba(g).tobytes()).hexdigest() == c["rgba"], c


# ---- end to end -------------------------------------------------------------------------------------------

W, H = 32, 20  # the tensor
LL = ["pic_67x45_m4q75", "disc_67x45_m4q75", "levels4_67x45_m4q75", "x_meta", "tiles_67x45_m6q100", "levels40_67x45_m0q50",
      "x_alpha_flag"]
LOSSY = ["ll_levels2_f3", "ll_disc_f2", "ll_tiles_f1"]  # tests/golden/alpha/, 67 x 45
BAD = {"bad_trunc_pic_67x45": errno.EINVAL, "bad_corrupt1": errno.EINVAL, "x_anim_flag": errno.ENOTSUP, "bad_signature": errno.EINVAL}


def batch():
    """The mixed batch of tests/test_gpu_lossless.py: lossy, lossless, undecodable, x_anim_flag."""
    names = [LL[0], LOSSY[0], "bad_trunc_pic_67x45", LL[1], LL[2], LOSSY[1], "x_anim_flag", LL[3], "bad_corrupt1", LL[4], LOSSY[2],
             LL[5], "bad_signature", LL[6]]
    return names, [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() if n in LOSSY else fixture(n) for n in names]


@pytest.mark.parametrize("device_m05", [False, True])
def test_mixed_batch_end_to_end(vp8g, golden, device_m05, monkeypatch):
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    names, files = batch()
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    shrink = vp8g.scale_opt(scale=(W, H))
    kw = dict(scale=shrink, device_m05=device_m05, extended=True, alpha=True, lossless=True)
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, lossless_scale=True, **kw)
    old, st_old = vp8g.gpu_decode_webp_batch_tensor(files, opt, **kw)
    got, old = got.cpu().numpy(), old.cpu().numpy()
    for i, n in enumerate(names):
        if n in LOSSY:
            assert st[i] == 0 == st_old[i] and old[i].any() and np.array_equal(got[i], old[i]), n
        elif n in BAD:
            assert st[i] == BAD[n] == st_old[i] and not got[i].any(), n
        else:
            assert st[i] == 0 and hashlib.sha256(got[i].tobytes()).hexdigest() == case_of(golden, n, scale=(W, H))["rgba"], n
            assert st_old[i] == errno.ENOTSUP and not old[i].any(), n  # without the new flag: what such a frame gets today
    # three channels: alpha dropped
    kw["alpha"] = False
    rgb, st3 = vp8g.gpu_decode_webp_batch_tensor(files, opt, lossless_scale=True, **kw)
    assert st3 == st and np.array_equal(rgb.cpu().numpy(), got[..., :3])


@pytest.mark.parametrize("device_m05", [False, True])
def test_per_frame_options(vp8g, golden, device_m05, monkeypatch):
    """An option each: the refused frames get EINVAL and a zero slot, their neighbours decode."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    name = "disc_67x45_m4q75"
    S = vp8g.scale_opt
    lossy = (GOLDEN / "alpha" / f"{LOSSY[0]}.webp").read_bytes()
    opts = [S(crop=(3, 5, W, H)), S(crop=(1, 3, 64, 40), scale=(W, H)), S(crop=(3, 5, 16, 10), scale=(W, H)),
            S(scale=(W, H)), S(crop=(3, 5, 16, 10), scale=(W, H), expand=True), S(scale=(30, H)), S(scale=(W, H))]
    files = [fixture(name), fixture(name), fixture(name), lossy, fixture(name), fixture(name), fixture(name)]
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, scale=opts, device_m05=device_m05, alpha=True, lossless=True,
                                                lossless_scale=True)
    got = got.cpu().numpy()
    assert st == [0, 0, errno.EINVAL, 0, 0, errno.EINVAL, 0]  # expand without the flag; a result of another size
    assert not got[2].any() and not got[5].any() and got[3].any()
    for i in (0, 1, 4, 6):
        o = opts[i]
        crop = (o.crop_left, o.crop_top, o.crop_w, o.crop_h)
        want = case_of(golden, name, crop=crop if any(crop) else None, scale=(o.scaled_w, o.scaled_h))
        assert hashlib.sha256(got[i].tobytes()).hexdigest() == want["rgba"], i
    # the crop without a target size is the picture's own pixels, from an odd origin
    argb = vp8g.host_lossless_argb(fixture(name))
    assert np.array_equal(got[0], vp8g.argb_to_rgba(argb[5:5 + H, 3:3 + W]))


def test_float_tensor_end_to_end(vp8g):
    names, files = batch()
    opt = vp8g.tensor_opt((W, H), "float16", "NCHW", mean=[0.5, 0.4, 0.3], std=[0.2, 0.3, 0.25], bgr=True)
    o = vp8g.scale_opt(crop=(1, 3, 64, 40), scale=(W, H))
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, scale=o, alpha=True, lossless=True, lossless_scale=True)
    got = got.cpu()
    for i, n in enumerate(names):
        if n in LL:
            want = vp8g.host_tensor_argb(vp8g.host_scale_argb(vp8g.host_lossless_argb(files[i]), o), opt, 4)
            assert st[i] == 0 and torch.equal(got[i].view(torch.uint8), want.view(torch.uint8)), n


def test_xflags(vp8g):
    lib = vp8g.gpu_lib()
    data = fixture(LL[1])
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    spans = (vp8g.ByteSpan * 1)(vp8g.ByteSpan(C.cast(buf, C.POINTER(C.c_uint8)), len(data)))
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    o = vp8g.scale_opt(scale=(W, H))
    out = torch.zeros((1, H, W, 4), dtype=torch.uint8, device="cuda")
    st = (C.c_int * 1)()

    def call(xflags):
        C.set_errno(0)
        rc = lib.vp8g_decode_webp_batch_tensor_any(spans, 1, 1, 0, 0, C.byref(o), 1, C.byref(opt), xflags, C.c_void_p(out.data_ptr()), st)
        return rc, C.get_errno(), st[0]

    assert vp8g.VP8G_X_LOSSLESS_SCALE == 16
    for xflags in (16, 17):  # the new flag needs VP8G_X_LOSSLESS
        assert call(xflags)[:2] == (-1, errno.EINVAL)
    assert call(2 | 1) == (-1, errno.ENOTSUP, errno.ENOTSUP) and not out.any()  # without it: as ever
    assert call(16 | 2 | 1) == (0, 0, 0) and out.any()
    assert call(32 | 16 | 2)[:2] == (-1, errno.EINVAL)
    assert lib.vp8g_abi_version() == 5


def test_refuses_bad_descriptors(vp8g):
    """The host copies are checked before anything is launched."""
    lib = vp8g.gpu_lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    head = lib.vp8g_scale_argb_head_size(2)
    shrink, crop = vp8g.scale_opt(scale=(5, 4)), vp8g.scale_opt(crop=(3, 1, 8, 6))

    def pair():
        d = (vp8g.Vp8gScaleArgbDesc * 2)()
        assert lib.vp8g_make_scale_argb_desc(16, 9, 0, C.byref(shrink), head, 0, 0, 0, 0, 0, C.byref(d[0])) == 0
        a = d[0]
        assert lib.vp8g_make_scale_argb_desc(16, 9, 1024, C.byref(crop), head + a.work_bytes, 256, a.nplanes, a.split_ntasks,
                                             a.scale_ntasks, a.merge_ntasks, C.byref(d[1])) == 0
        return d

    def launch(d, n=2, work=p):
        C.set_errno(0)
        return lib.vp8g_scale_argb_batch_device(d, p, n, p, work, p, None), C.get_errno()

    d = pair()
    assert (d[0].nplanes, d[1].nplanes, d[1].work_bytes) == (4, 0, 0) and d[0].work_bytes == lib.vp8g_scale_argb_work_size(16, 9, C.byref(shrink))
    bad = (-1, errno.EINVAL)

    def plane_dst(d):
        d[0].plane[3].p[0].dst += 16

    def plane_task(d):
        d[0].plane[1].task0 += 1

    changes = {
        "task numbering": [lambda d: setattr(d[1], "split_task0", d[1].split_task0 + 1), lambda d: setattr(d[1], "merge_task0", 0),
                           lambda d: setattr(d[1], "plane0", 0), plane_task],
        "a window outside the picture": [lambda d: setattr(d[1], "crop_left", 9), lambda d: setattr(d[0], "src_height", 8),
                                         lambda d: setattr(d[0], "win_w", 17)],
        "planes somewhere else": [plane_dst, lambda d: setattr(d[0], "out_stride", 8)],
        "a work region inside the head": [lambda d: setattr(d[0], "work", 0)],
    }
    for what, fs in changes.items():
        for k, f in enumerate(fs):
            d = pair()
            f(d)
            assert launch(d) == bad, (what, k)
    assert launch(pair(), n=0) == bad
    assert launch(pair(), work=C.c_void_p(buf.data_ptr() + 4)) == bad   # the work buffer is not 16-byte aligned
    # work regions that overlap
    d = (vp8g.Vp8gScaleArgbDesc * 2)()
    assert lib.vp8g_make_scale_argb_desc(16, 9, 0, C.byref(shrink), head, 0, 0, 0, 0, 0, C.byref(d[0])) == 0
    a = d[0]
    assert lib.vp8g_make_scale_argb_desc(16, 9, 1024, C.byref(shrink), head + a.work_bytes - 16, 256, a.nplanes, a.split_ntasks,
                                         a.scale_ntasks, a.merge_ntasks, C.byref(d[1])) == 0
    assert launch(d) == bad
    # the maker's own refusals
    one = vp8g.Vp8gScaleArgbDesc()
    for args in ((16, 9, 2, shrink, head, 0), (16, 9, 0, shrink, head + 8, 0), (16, 9, 0, shrink, head, 2),
                 (16, 9, 0, vp8g.scale_opt(scale=(17, 9)), head, 0), (16, 9, 0, vp8g.scale_opt(crop=(9, 0, 8, 9)), head, 0)):
        w, h, src, o, work, dst = args
        assert lib.vp8g_make_scale_argb_desc(w, h, src, C.byref(o), work, dst, 0, 0, 0, 0, C.byref(one)) == -1
        assert C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.vp8g_scale_argb_work_size(16, 9, C.byref(vp8g.scale_opt(scale=(17, 9)))) == 0 and C.get_errno() == errno.EINVAL
    assert not buf.any()  # nothing ran
