"""CPU tests of the device-tensor path's host side: slot sizes, argument validation and
descriptor numbering of libvp8g.so (host code only, no device call), tensor_opt's normalisation, and
host_tensor -- the restatement the GPU tests compare against -- on hand-computed values.

Bar: exact values (integers, float32 bit patterns)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

EINVAL = 22
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def yuv_to_rgb(y, u, v):
    """libwebp's VP8YuvToRgb: 14-bit fixed point, clip of the value >> 6 to 0..255."""
    def clip(x):
        return min(max(x >> 6, 0), 255)
    yy = (y * 19077) >> 8
    return (clip(yy + ((v * 26149) >> 8) - 14234), clip(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708),
            clip(yy + ((u * 33050) >> 8) - 17685))


def einval(call, fail=-1):
    C.set_errno(0)
    return call() == fail and C.get_errno() == EINVAL


def test_slot_sizes(vp8g):
    lib = vp8g.gpu_lib()
    for dtype, eb in (("uint8", 1), ("float16", 2), ("bfloat16", 2), ("float32", 4)):
        for layout in ("NHWC", "NCHW"):
            for w, h in ((3, 3), (224, 224), (641, 479), (16383, 16383), (1, 1)):
                o = vp8g.tensor_opt((w, h), dtype, layout)
                assert lib.vp8g_tensor_slot_size(C.byref(o)) == 3 * w * h * eb, (dtype, layout, w, h)
    assert lib.vp8g_tensor_slot_size(C.byref(vp8g.tensor_opt((3, 3), "uint8"))) == 27  # (not 16-byte aligned)


def test_torch_and_numpy_dtypes_are_accepted(vp8g):
    assert vp8g.tensor_opt((2, 2), torch.bfloat16).dtype == 2 and vp8g.tensor_opt((2, 2), np.float16).dtype == 1
    assert vp8g.tensor_opt((2, 2), torch.uint8).dtype == 0 and vp8g.tensor_opt((2, 2), "float32").dtype == 3
    with pytest.raises(ValueError):
        vp8g.tensor_opt((2, 2), "int8")
    with pytest.raises(ValueError):
        vp8g.tensor_opt((2, 2), "uint8", layout="CHWN")
    with pytest.raises(ValueError):
        vp8g.tensor_opt((2, 2), "float32", mean=0.5, scale=1.0)


def bad_options(vp8g):
    T = vp8g.Vp8gTensorOpt
    one, zero = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
    out = [T(0, 8, 0, 0, 0, one, zero), T(8, 0, 0, 0, 0, one, zero), T(16384, 8, 0, 0, 0, one, zero),
           T(8, 16384, 0, 0, 0, one, zero), T(8, 8, 4, 0, 0, one, zero), T(8, 8, 0, 2, 0, one, zero),
           T(8, 8, 0, 0, 2, one, zero), T(8, 8, 0, 0, 3, one, zero)]
    for dtype in (1, 2, 3):
        for bad in (math.inf, -math.inf, math.nan):
            for c in range(3):
                v = [1.0, 1.0, 1.0]
                v[c] = bad
                out.append(T(8, 8, dtype, 0, 0, (C.c_float * 3)(*v), zero))
                out.append(T(8, 8, dtype, 1, 0, one, (C.c_float * 3)(*v)))
    return out


def test_invalid_options_are_einval(vp8g):
    lib = vp8g.gpu_lib()
    d = vp8g.Vp8gTensorDesc()
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    span = (vp8g.ByteSpan * 1)()
    for i, o in enumerate(bad_options(vp8g)):
        assert einval(lambda: lib.vp8g_tensor_slot_size(C.byref(o)), fail=0), i
        assert einval(lambda: lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 8, 4, 0, 0, C.byref(d))), i
        assert einval(lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, C.byref(o), p, p, None)), i
        assert einval(lambda: lib.vp8g_decode_webp_batch_tensor(span, 1, 1, 0, 0, None, 0, C.byref(o), p, None)), i
    # scale and bias are ignored for uint8: non-finite values are not an error there
    o = vp8g.Vp8gTensorOpt(8, 8, 0, 0, 0, (C.c_float * 3)(math.nan, 1, 1), (C.c_float * 3)(0, math.inf, 0))
    assert lib.vp8g_tensor_slot_size(C.byref(o)) == 192


def test_null_and_malformed_arguments_are_einval(vp8g):
    lib = vp8g.gpu_lib()
    o = vp8g.tensor_opt((8, 8), "float16", "NCHW")
    d = vp8g.Vp8gTensorDesc()
    assert lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 8, 4, 0, 0, C.byref(d)) == 0
    buf = np.zeros(256, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 1)
    span = (vp8g.ByteSpan * 2)()
    sopt = vp8g.scale_opt(scale=(8, 8))
    calls = [
        lambda: lib.vp8g_make_tensor_desc(None, 0, 64, 80, 8, 4, 0, 0, C.byref(d)),
        lambda: lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 8, 4, 0, 0, None),
        lambda: lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 7, 4, 0, 0, C.byref(vp8g.Vp8gTensorDesc())),  # stride < width
        lambda: lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 8, 3, 0, 0, C.byref(vp8g.Vp8gTensorDesc())),
        lambda: lib.vp8g_make_tensor_desc(C.byref(o), 0, 64, 80, 8, 4, 1, 0, C.byref(vp8g.Vp8gTensorDesc())),  # dst off the element
        lambda: lib.vp8g_tensor_batch_device(None, p, 1, C.byref(o), p, p, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), None, 1, C.byref(o), p, p, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, None, p, p, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, C.byref(o), None, p, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, C.byref(o), p, None, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 0, C.byref(o), p, p, None),
        lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, C.byref(o), p, odd, None),  # d_dst off the element size
        lambda: lib.vp8g_decode_webp_batch_tensor(None, 1, 1, 0, 0, None, 0, C.byref(o), p, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 0, 1, 0, 0, None, 0, C.byref(o), p, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, None, 0, None, p, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, None, 0, C.byref(o), None, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, None, 0, C.byref(o), odd, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 4, None, 0, C.byref(o), p, None),  # unknown flag
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, None, 1, C.byref(o), p, None),  # n_opts without opts
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, C.byref(sopt), 0, C.byref(o), p, None),
        lambda: lib.vp8g_decode_webp_batch_tensor(span, 2, 1, 0, 0, C.byref(sopt), 3, C.byref(o), p, None),
    ]
    for i, call in enumerate(calls):
        assert einval(call), i
    # the float32 element: a base that is 2 off is refused (the descriptor itself is consistent)
    o32 = vp8g.tensor_opt((8, 8), "float32")
    assert einval(lambda: lib.vp8g_tensor_batch_device(C.byref(d), p, 1, C.byref(o32), p, C.c_void_p(base + 2), None))


def test_task_numbering_over_a_mixed_list(vp8g):
    """Tasks are numbered image by image: 256 chunks of 12 pixels of a row per task; a list that skips or
    repeats a number is refused before any launch."""
    lib = vp8g.gpu_lib()
    for (w, h), per in (((1, 1), 1), ((12, 256), 1), ((13, 256), 2), ((224, 224), 17), ((641, 479), 102), ((3840, 2160), 2700)):
        o = vp8g.tensor_opt((w, h), "uint8", "NHWC")
        assert per == -(-(-(-w // 12) * h) // 256)
        n = 5
        descs = (vp8g.Vp8gTensorDesc * n)()
        slot, task0 = lib.vp8g_tensor_slot_size(C.byref(o)), 0
        for i in range(n):
            sy, suv = w + 3 * i, (w + 1) // 2 + i
            assert lib.vp8g_make_tensor_desc(C.byref(o), 1000 * i, 1000 * i + 7, 1000 * i + 9, sy, suv, i * slot, task0,
                                             C.byref(descs[i])) == 0
            d = descs[i]
            assert (d.src_y, d.src_u, d.src_v, d.dst) == (1000 * i, 1000 * i + 7, 1000 * i + 9, i * slot)
            assert (d.stride_y, d.stride_uv, d.task0, d.ntasks) == (sy, suv, i * per, per)
            task0 += d.ntasks
        buf = np.zeros(64, np.uint8)
        p = C.c_void_p(buf.ctypes.data)
        for i, delta in ((1, 1), (3, -1), (0, 1)):
            descs[i].task0 += delta
            assert einval(lambda: lib.vp8g_tensor_batch_device(descs, p, n, C.byref(o), p, p, None)), (w, h, i)
            descs[i].task0 -= delta
        descs[2].ntasks += 1
        assert einval(lambda: lib.vp8g_tensor_batch_device(descs, p, n, C.byref(o), p, p, None)), (w, h)


def test_tensor_opt_mean_std(vp8g):
    o = vp8g.tensor_opt((224, 224), "float16", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    assert (o.width, o.height, o.dtype, o.layout, o.flags) == (224, 224, 1, 1, 0)
    for c in range(3):
        assert o.scale[c] == np.float32(1.0 / (255.0 * IMAGENET_STD[c])) and o.bias[c] == np.float32(-IMAGENET_MEAN[c] / IMAGENET_STD[c])
    o = vp8g.tensor_opt((8, 8), "float32", "NHWC", scale=1 / 255, bgr=True)
    assert list(o.scale) == [float(np.float32(1 / 255))] * 3 and list(o.bias) == [0.0] * 3 and (o.layout, o.flags) == (0, 1)
    o = vp8g.tensor_opt((8, 8), "float32", mean=0.5)  # std defaults to 1
    assert list(o.scale) == [float(np.float32(1 / 255))] * 3 and list(o.bias) == [-0.5] * 3
    o = vp8g.tensor_opt((8, 8), "uint8")
    assert list(o.scale) == [1.0] * 3 and list(o.bias) == [0.0] * 3


def test_host_tensor_grey_2x2(vp8g):
    """Y = (16, 235, 128, 0) with U = V = 128: black, white, mid grey 130, and the clamp at 0."""
    assert [yuv_to_rgb(y, 128, 128) for y in (16, 235, 128, 0)] == [(0, 0, 0), (255, 255, 255), (130, 130, 130), (0, 0, 0)]
    i420 = bytes([16, 235, 128, 0, 128, 128])
    exp = np.array([[[0] * 3, [255] * 3], [[130] * 3, [0] * 3]], np.uint8)
    got = vp8g.host_tensor(i420, 2, 2, vp8g.tensor_opt((2, 2), "uint8", "NHWC"))
    assert got.dtype == torch.uint8 and got.shape == (2, 2, 3) and (got.numpy() == exp).all()
    got = vp8g.host_tensor(i420, 2, 2, vp8g.tensor_opt((2, 2), "uint8", "NCHW"))
    assert got.shape == (3, 2, 2) and (got.numpy() == exp.transpose(2, 0, 1)).all()
    # float32: a rounded multiply, then a rounded add -- 130 / 255 in float32 arithmetic, not in double
    o = vp8g.tensor_opt((2, 2), "float32", "NHWC", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    got = vp8g.host_tensor(i420, 2, 2, o).numpy()
    for c in range(3):
        s, b = np.float32(o.scale[c]), np.float32(o.bias[c])
        for (yy, xx), v in (((0, 0), 0), ((0, 1), 255), ((1, 0), 130), ((1, 1), 0)):
            e = np.float32(np.float32(v) * s) + b
            assert got[yy, xx, c].view(np.uint32) == np.float32(e).view(np.uint32)
    # float16 / bfloat16: that float32 rounded once to nearest-even
    o16 = vp8g.tensor_opt((2, 2), "float16", "NHWC", scale=1 / 255)
    got = vp8g.host_tensor(i420, 2, 2, o16)
    assert got.dtype == torch.float16
    assert got[1, 0, 0].item() == float(np.float16(np.float32(130) * np.float32(1 / 255)))
    ob = vp8g.tensor_opt((2, 2), "bfloat16", "NHWC", scale=1 / 255)
    got = vp8g.host_tensor(i420, 2, 2, ob)
    assert got.dtype == torch.bfloat16
    f = (np.float32(130) * np.float32(1 / 255)).view(np.uint32)
    bf = (int(f) + 0x7FFF + ((int(f) >> 16) & 1)) >> 16
    assert got.view(torch.int16)[1, 0, 0].item() == bf and got[0, 1, 0].item() == 1.0


def test_host_tensor_channel_order_2x1(vp8g):
    """U != V: R and B differ, so a swapped order under bgr shows; scale[0] applies to B then."""
    ys, u, v = (100, 200), 90, 240
    px = [yuv_to_rgb(y, u, v) for y in ys]  # (one chroma sample: the upsampler returns it for both pixels)
    assert all(p[0] != p[2] for p in px) and px[0] == (255, 22, 21)
    i420 = bytes([*ys, u, v])
    rgb = vp8g.host_tensor(i420, 2, 1, vp8g.tensor_opt((2, 1), "uint8", "NHWC")).numpy()
    bgr = vp8g.host_tensor(i420, 2, 1, vp8g.tensor_opt((2, 1), "uint8", "NHWC", bgr=True)).numpy()
    assert rgb.tolist() == [[list(p) for p in px]] and bgr.tolist() == [[list(p[::-1]) for p in px]]
    o = vp8g.tensor_opt((2, 1), "float32", "NCHW", scale=(2.0, 1.0, 0.5), bias=(10.0, 0.0, -1.0), bgr=True)
    got = vp8g.host_tensor(i420, 2, 1, o).numpy()
    assert got.shape == (3, 1, 2)
    for x, (r, g, b) in enumerate(px):
        assert got[:, 0, x].tolist() == [b * 2.0 + 10.0, float(g), r * 0.5 - 1.0]
