"""The device half of the lossless (VP8L) path: the inverse-transform kernel against the
sequential restatement (vp8f_lossless_apply) on synthetic images that reach every predictor mode, block size,
hand-over and transform order, and against libwebp on the fixtures; the ARGB tensor kernel against its numpy
restatement; lossless files through the batch pipeline.  All comparisons are bit-exact."""
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
P, CC, SG, CI = 0, 1, 2, 3
NCOLORS = {3: 2, 2: 4, 1: 11, 0: 40}  # colours of a table that packs 8 / 4 / 2 / 1 pixels per byte


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "lossless.json").read_text())


def fixture(name):
    return (LOSSLESS / f"{name}.webp").read_bytes()


def synth(vp8g, rng, w, h, types, bits=2, pack=None):
    """A random image whose transforms are `types` in stream order: every mode 0..15 in the predictor's mode image,
    every byte of a cross-colour entry random (negative multipliers included), random tables and residuals."""
    trs, xs = [], w
    for t in types:
        r = (1 << bits) - 1
        shape = ((h + r) >> bits, (xs + r) >> bits)
        if t == P:
            junk = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFF00FF)
            trs.append({"type": P, "bits": bits, "data": junk | (rng.integers(0, 16, shape).astype(np.uint32) << 8)})
        elif t == CC:
            trs.append({"type": CC, "bits": bits, "data": rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)})
        elif t == SG:
            trs.append({"type": SG, "bits": 0})
        else:
            trs.append({"type": CI, "bits": pack, "data": rng.integers(0, 1 << 32, NCOLORS[pack], dtype=np.uint64).astype(np.uint32)})
            xs = (xs + (1 << pack) - 1) >> pack
    res = rng.integers(0, 1 << 32, (h, xs), dtype=np.uint64).astype(np.uint32)
    return vp8g.lossless_image(res, trs, width=w)


def check(vp8g, images):
    got = vp8g.gpu_lossless_argb(images)  # (odd source offsets, guard bytes around every output)
    for k, (im, g) in enumerate(zip(images, got)):
        want = vp8g.host_lossless_apply(im)
        bad = np.argwhere(g != want)
        assert bad.size == 0, (k, im["width"], im["height"], [t["type"] for t in im["transforms"]], bad[:4].tolist())


def kernel_sizes(vp8g):
    t, band, bands = vp8g.lossless_geometry()  # (from the library: the kernel's own constants)
    rnd = band * bands
    return ([(1, 1), (1, 9), (9, 1), (2, 2), (3, 5)] + [(w, 5) for w in (t - 1, t, t + 1, 2 * t)]
            + [(7, h) for h in (band - 1, band, band + 1)] + [(7, h) for h in (rnd - 1, rnd, rnd + 1)] + [(257, 130)])


@pytest.mark.parametrize("bits", [2, 5, 9])
def test_predictor_vs_restatement(vp8g, bits):
    """The predictor alone, mixed sizes in one launch: tiny images, widths around the tile step, heights around a
    wave's band and around a workgroup round, one image of several bands and tiles."""
    rng = np.random.default_rng(100 + bits)
    check(vp8g, [synth(vp8g, rng, w, h, [P], bits) for w, h in kernel_sizes(vp8g)])


def test_more_images_than_workgroups(vp8g):
    """One workgroup takes several images of mixed sizes and transform lists, one after the other."""
    rng = np.random.default_rng(7)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lists = [[P], [SG, P, CC], [P, CC, SG], [SG, P], [CI, P], [CI, SG, P, CC], [CC], []]
    sizes = [(5, 3), (67, 2), (3, 70), (130, 9), (1, 1), (20, 66)]
    n = cus + 37
    images = [synth(vp8g, rng, *sizes[k % len(sizes)], lists[(k // 2) % len(lists)], bits=2 + k % 3, pack=k % 4) for k in range(n)]
    check(vp8g, images)


# [SG, P, CC] is the order whose inverse is cross colour -> predictor -> add green: the kernel's one fused pass
ORDERS = [[P], [CC], [SG], [CI], [SG, P, CC], [CI, SG, P, CC], [P, CC, SG], [SG, P], [P, CC], [P, CI], [SG, CC], [CC, P],
          [P, CC, SG, CI], [CI, SG, CC, P], [SG, CI, P, CC], [CC, SG, P]]


@pytest.mark.parametrize("pack", [3, 2, 1, 0])
def test_transform_lists_vs_restatement(vp8g, pack):
    """Each single transform, the encoder's order ([SG, P, CC], fully fused; also behind colour indexing), colour indexing read before the predictor ([CI, P]: the predictor
    works at the packed width) and after it ([P, CI]), all four in several orders; at 1, 2, 4 and 8 bits per pixel."""
    rng = np.random.default_rng(40 + pack)
    images = []
    for order in ORDERS + [[CI, P], [CI, P, CC, SG]]:
        for (w, h), bits in (((37, 21), 2), ((70, 67), 3), ((9, 130), 5)):
            images.append(synth(vp8g, rng, w, h, order, bits, pack))
    check(vp8g, images)


def test_cross_colour_negative_multipliers(vp8g):
    rng = np.random.default_rng(3)
    im = synth(vp8g, rng, 33, 9, [P, CC], 2)
    im["transforms"][1]["data"][:] = 0xFF80E0C1  # g2r = -63, g2b = -32, r2b = -128
    im2 = synth(vp8g, rng, 33, 9, [CC], 3)
    im2["transforms"][0]["data"][:] = 0x00FF81FF
    check(vp8g, [im, im2])


def test_fixtures_equal_libwebps_rgba(vp8g, golden):
    names = [n for n, e in golden["files"].items() if e["decodes"]]
    images = []
    for n in names:
        data = fixture(n)
        c = vp8g.parse_any(data)
        images.append(vp8g.lossless_decode_host(data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]))
    got = vp8g.gpu_lossless_argb(images)
    for n, g in zip(names, got):
        assert hashlib.sha256(vp8g.argb_to_rgba(g).tobytes()).hexdigest() == golden["files"][n]["rgba"], n


def test_refuses_bad_descriptors(vp8g):
    lib = vp8g.gpu_lib()
    d = vp8g.Vp8gLosslessDesc()
    T = vp8g.Vp8gLosslessTransform

    def make(w, h, dst, trs):
        arr = (T * 4)(*trs)
        return lib.vp8g_make_lossless_desc(w, h, 0, dst, len(trs), arr, 0, C.byref(d))

    assert make(8, 8, 0, [T(0, P, 2, 8, 0)]) == 0
    for bad in ([T(0, P, 1, 8, 0)], [T(0, P, 10, 8, 0)], [T(0, P, 2, 7, 0)], [T(0, P, 2, 8, 0), T(0, P, 2, 8, 0)], [T(0, 4, 2, 8, 0)],
                [T(0, CI, 3, 8, 3)], [T(0, CI, 0, 8, 257)], [T(0, CI, 3, 8, 2), T(0, P, 2, 8, 0)]):
        assert make(8, 8, 0, bad) == -1 and C.get_errno() == errno.EINVAL, [(t.type, t.bits, t.xsize) for t in bad]
    assert make(8, 8, 0, [T(0, CI, 3, 8, 2), T(0, P, 2, 1, 0)]) == 0
    assert make(0, 8, 0, []) == -1 and make(8, 16384, 0, []) == -1 and make(8, 8, 2, []) == -1
    # the launch validates the host copies before anything runs
    assert make(8, 8, 0, [T(0, P, 2, 8, 0)]) == 0
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    arr = (vp8g.Vp8gLosslessDesc * 1)(d)
    arr[0].tr[0].bits = 12
    p = C.c_void_p(buf.data_ptr())
    assert lib.vp8g_lossless_batch_device(arr, p, 1, p, p, None) == -1 and C.get_errno() == errno.EINVAL
    arr[0].tr[0].bits = 2
    arr[0].task0 = 1
    assert lib.vp8g_lossless_batch_device(arr, p, 1, p, p, None) == -1 and C.get_errno() == errno.EINVAL
    assert lib.vp8g_lossless_batch_device(arr, p, 0, p, p, None) == -1 and C.get_errno() == errno.EINVAL


# ---- ARGB -> tensor -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def argb_inputs():
    rng = np.random.default_rng(11)
    return {s: [rng.integers(0, 1 << 32, (s[1], s[0]), dtype=np.uint64).astype(np.uint32) for _ in range(3)] for s in ((3, 3), (37, 21))}


@pytest.mark.parametrize("dtype", ["uint8", "float16", "bfloat16", "float32"])
def test_tensor_argb_vs_host_tensor(vp8g, argb_inputs, dtype):
    for (w, h), pics in argb_inputs.items():
        for layout in ("NHWC", "NCHW"):
            for bgr in (False, True):
                opt = vp8g.tensor_opt((w, h), dtype, layout, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], bgr=bgr)
                for channels in (3, 4):
                    for shift in (0, 1):  # (shift 1: no slot is 16-byte aligned, and most are not dword-aligned for uint8)
                        got = vp8g.gpu_tensor_argb(pics, opt, channels, slot_shift=shift).cpu()
                        for i, p in enumerate(pics):
                            want = vp8g.host_tensor_argb(p, opt, channels)
                            assert torch.equal(got[i].view(torch.uint8), want.view(torch.uint8)), (w, h, layout, bgr, channels, shift, i)


def test_tensor_argb_uint8_rgba_equals_libwebps_bytes(vp8g, golden):
    for name in ("disc_67x45_m4q75", "levels16_37x21_m6q100"):
        argb = vp8g.host_lossless_argb(fixture(name))
        h, w = argb.shape
        got = vp8g.gpu_tensor_argb([argb], vp8g.tensor_opt((w, h), "uint8", "NHWC"), 4).cpu().numpy()[0]
        assert hashlib.sha256(got.tobytes()).hexdigest() == golden["files"][name]["rgba"], name


def test_tensor_argb_refuses_bad_arguments(vp8g):
    lib = vp8g.gpu_lib()
    opt = vp8g.tensor_opt((4, 4), "float32", "NHWC")
    d = vp8g.Vp8gTensorArgbDesc()
    assert lib.vp8g_make_tensor_argb_desc(C.byref(opt), 4, 0, 0, 0, C.byref(d)) == 0 and d.ntasks == 1
    for ch, src, dst in ((2, 0, 0), (5, 0, 0), (4, 2, 0), (4, 0, 2)):
        assert lib.vp8g_make_tensor_argb_desc(C.byref(opt), ch, src, dst, 0, C.byref(d)) == -1 and C.get_errno() == errno.EINVAL
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    arr = (vp8g.Vp8gTensorArgbDesc * 1)(vp8g.Vp8gTensorArgbDesc(0, 0, 0, 1))
    assert lib.vp8g_tensor_batch_device_argb(arr, p, 1, C.byref(opt), 5, p, p, None) == -1 and C.get_errno() == errno.EINVAL
    arr[0].task0 = 3
    assert lib.vp8g_tensor_batch_device_argb(arr, p, 1, C.byref(opt), 4, p, p, None) == -1 and C.get_errno() == errno.EINVAL


# ---- end to end -------------------------------------------------------------------------------------------

W, H = 67, 45
LL = ["pic_67x45_m4q75", "disc_67x45_m4q75", "levels4_67x45_m4q75", "x_meta", "tiles_67x45_m6q100", "levels40_67x45_m0q50",
      "x_alpha_flag"]
LOSSY = ["ll_levels2_f3", "ll_disc_f2", "ll_tiles_f1"]  # tests/golden/alpha/, 67 x 45
BAD = {"bad_trunc_pic_67x45": errno.EINVAL, "bad_corrupt1": errno.EINVAL, "x_anim_flag": errno.ENOTSUP, "bad_signature": errno.EINVAL,
       "pic_37x21_m0q10": errno.EINVAL}  # (the last one decodes, but is not the tensor's size)


def batch():
    names = [LL[0], LOSSY[0], "bad_trunc_pic_67x45", LL[1], LL[2], LOSSY[1], "x_anim_flag", LL[3], "bad_corrupt1", LL[4], LOSSY[2],
             LL[5], "bad_signature", "pic_37x21_m0q10", LL[6]]
    return names, [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() if n in LOSSY else fixture(n) for n in names]


@pytest.mark.parametrize("device_m05", [False, True])
def test_mixed_batch_end_to_end(vp8g, golden, device_m05, monkeypatch):
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    names, files = batch()
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True, lossless=True)
    old, st_old = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True)
    got, old = got.cpu().numpy(), old.cpu().numpy()
    for i, n in enumerate(names):
        if n in LOSSY:
            assert st[i] == 0 == st_old[i] and np.array_equal(got[i], old[i]), n
        elif n in BAD:
            assert st[i] == BAD[n] and not got[i].any(), n
        else:
            assert st[i] == 0 and hashlib.sha256(got[i].tobytes()).hexdigest() == golden["files"][n]["rgba"], n
        if n not in LOSSY:  # without the flag: what such a file gets today
            assert st_old[i] == errno.ENOTSUP and not old[i].any(), n
    # three channels: alpha dropped
    rgb, st3 = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, lossless=True)
    assert st3 == st and np.array_equal(rgb.cpu().numpy(), got[..., :3])


def test_float_tensor_end_to_end(vp8g):
    names, files = batch()
    opt = vp8g.tensor_opt((W, H), "float16", "NCHW", mean=[0.5, 0.4, 0.3], std=[0.2, 0.3, 0.25], bgr=True)
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, alpha=True, lossless=True)
    got = got.cpu()
    for i, n in enumerate(names):
        if n in LL:
            want = vp8g.host_tensor_argb(vp8g.host_lossless_argb(files[i]), opt, 4)
            assert st[i] == 0 and torch.equal(got[i].view(torch.uint8), want.view(torch.uint8)), n


@pytest.mark.parametrize("device_m05", [False, True])
def test_scaling_a_lossless_frame_is_not_supported(vp8g, golden, device_m05, monkeypatch):
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    files = [fixture(LL[0]), fixture(LL[1]), (GOLDEN / "alpha" / f"{LOSSY[0]}.webp").read_bytes(), fixture(LL[2])]
    ident, crop = vp8g.scale_opt(), vp8g.scale_opt(crop=(0, 0, W, H), scale=(W, H))
    shrink = vp8g.scale_opt(scale=(W, H))
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    # frame 1's option is not the identity for it (a crop of another size): ENOTSUP; its neighbours decode
    opts = [ident, vp8g.scale_opt(crop=(0, 0, W - 2, H)), shrink, crop]
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, scale=opts, device_m05=device_m05, alpha=True, lossless=True)
    got = got.cpu().numpy()
    assert st == [0, errno.ENOTSUP, 0, 0] and not got[1].any()
    for i in (0, 3):
        assert hashlib.sha256(got[i].tobytes()).hexdigest() == golden["files"][LL[0] if i == 0 else LL[2]]["rgba"]
    # a scale to another size is ENOTSUP as well, before the size is compared with the tensor's
    small = vp8g.tensor_opt((32, 20), "uint8", "NHWC")
    _, st = vp8g.gpu_decode_webp_batch_tensor(files[:1], small, scale=vp8g.scale_opt(scale=(32, 20)), alpha=True, lossless=True)
    assert st == [errno.ENOTSUP]


def test_any_refuses_unknown_xflags(vp8g):
    lib = vp8g.gpu_lib()
    data = fixture(LL[0])
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    spans = (vp8g.ByteSpan * 1)(vp8g.ByteSpan(C.cast(buf, C.POINTER(C.c_uint8)), len(data)))
    opt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    out = torch.zeros((1, H, W, 4), dtype=torch.uint8, device="cuda")
    st = (C.c_int * 1)()
    for xflags in (4, 8, 6, 0x80000000):
        assert lib.vp8g_decode_webp_batch_tensor_any(spans, 1, 1, 0, 0, None, 0, C.byref(opt), xflags, C.c_void_p(out.data_ptr()),
                                                     st) == -1 and C.get_errno() == errno.EINVAL
    # without VP8G_X_LOSSLESS it is vp8g_decode_webp_batch_tensor_x: a lossless file is ENOTSUP
    assert lib.vp8g_decode_webp_batch_tensor_any(spans, 1, 1, 0, 0, None, 0, C.byref(opt), 1, C.c_void_p(out.data_ptr()), st) == -1
    assert st[0] == errno.ENOTSUP
    assert lib.vp8g_decode_webp_batch_tensor_any(spans, 1, 1, 0, 0, None, 0, C.byref(opt), 3, C.c_void_p(out.data_ptr()), st) == 0
    assert st[0] == 0 and out.any()
    assert lib.vp8g_abi_version() == 5
