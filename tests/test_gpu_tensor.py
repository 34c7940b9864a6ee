"""GPU tests (MI355X) of decode-to-a-device-tensor: the tensor kernel
(webp-decoder_amd/csrc/vp8g_tensor.hip) behind vp8g_tensor_batch_device and
vp8g_decode_webp_batch_tensor.

Bar: bit equality with host_tensor (the numpy / torch-CPU restatement, itself pinned to hand-computed
values in tests/test_tensor_host.py): uint8 as bytes, the float types through their integer views."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest
import torch

from conftest import FIXTURES, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EINVAL = 22
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NORMS = [dict(), dict(scale=1 / 255), IMAGENET]  # identity, (1/255, 0), ImageNet mean / std
INT_VIEW = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}

# chroma rows shorter than 8 samples (w < 15), chunk boundaries on both sides (12, 24), the first-row /
# last-row chroma choice for even and odd heights; then more than one workgroup task per image
WIDTHS = [1, 2, 3, 11, 12, 13, 14, 15, 16, 23, 24, 25, 37, 224]
SIZES = [(w, h) for w in WIDTHS for h in (1, 2, 3, 4, 5)] + [(224, 224), (641, 479)]


def plane_input(kind, w, h, seed):
    """The generators of tests/test_gpu_scale.py, plus all-0."""
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "binary":
        return (np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8) * np.uint8(255)).tobytes()
    return bytes([255 if kind == "ones" else 0]) * n


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


@pytest.fixture(scope="module")
def inputs():
    """Per size: random, all-0, all-255 and 0/255 pictures (one launch converts the four)."""
    return {(w, h): [plane_input(k, w, h, 1000 + 7 * w + h) for k in ("random", "zeros", "ones", "binary")] for w, h in SIZES}


@pytest.mark.parametrize("dtype", ["uint8", "float16", "bfloat16", "float32"])
def test_kernel_vs_host_tensor(vp8g, inputs, dtype):
    bad = []
    for (w, h), imgs in inputs.items():
        for layout in ("NHWC", "NCHW"):
            for bgr in (False, True):
                for ni, norm in enumerate(NORMS[:1] if dtype == "uint8" else NORMS):  # (uint8 ignores scale and bias)
                    opt = vp8g.tensor_opt((w, h), dtype, layout, bgr=bgr, **norm)
                    got = vp8g.gpu_tensor(imgs, w, h, opt).cpu()
                    for i, b in enumerate(imgs):
                        if not same_bits(got[i], vp8g.host_tensor(b, w, h, opt)):
                            bad.append((w, h, layout, bgr, ni, i))
    assert not bad, (len(bad), bad[:12])


def test_uint8_ignores_scale_and_bias(vp8g, inputs):
    imgs = inputs[(37, 5)]
    opt = vp8g.tensor_opt((37, 5), "uint8", "NHWC", scale=(0.5, float("nan"), 3.0), bias=(1.0, 2.0, float("inf")))
    got = vp8g.gpu_tensor(imgs, 37, 5, opt).cpu()
    for i, b in enumerate(imgs):
        assert same_bits(got[i], vp8g.host_tensor(b, 37, 5, vp8g.tensor_opt((37, 5), "uint8", "NHWC")))


@pytest.mark.parametrize("w,h,dtype,layout,gap", [(37, 5, "float32", "NHWC", 0), (37, 5, "uint8", "NCHW", 0), (3, 3, "uint8", "NHWC", 0),
                                                  (5, 3, "float16", "NCHW", 0), (25, 4, "bfloat16", "NHWC", 3)])
def test_mixed_launch_scattered_sources_offset_base(vp8g, w, h, dtype, layout, gap):
    """Five images at padded source strides scattered in the source buffer; the output base one element
    off an aligned allocation (3x3 uint8: 27-byte slots), prefilled with 0xEE: every slot is right and
    no byte outside the slots is written.  gap: elements left between the slots."""
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    rng = np.random.default_rng(31 + w)
    opt = vp8g.tensor_opt((w, h), dtype, layout, bgr=(w == 37), **IMAGENET)
    eb = vp8g.T_ELEM[opt.dtype]
    slot = lib.vp8g_tensor_slot_size(C.byref(opt))
    n, cw, ch = 5, (w + 1) // 2, (h + 1) // 2
    descs = (vp8g.Vp8gTensorDesc * n)()
    chunks, planes, so, task0 = [np.zeros(3, np.uint8)], [], 3, 0  # (source planes start at an odd offset)
    order = [3, 0, 4, 1, 2]  # image i's planes are laid down in this order
    offs = {}
    for i in order:
        tight = plane_input("random" if i else "binary", w, h, 40 + i)
        a = np.frombuffer(tight, np.uint8)
        sy, suv = w + int(rng.integers(0, 9)), cw + int(rng.integers(0, 5))
        o = []
        for pl, pw, ph, st in ((a[:w * h], w, h, sy), (a[w * h:w * h + cw * ch], cw, ch, suv), (a[w * h + cw * ch:], cw, ch, suv)):
            buf = rng.integers(0, 256, size=st * ph, dtype=np.uint8).reshape(ph, st)  # padding = noise
            buf[:, :pw] = pl.reshape(ph, pw)
            o.append(so)
            chunks.append(buf.reshape(-1))
            so += buf.size
        offs[i] = (tight, o, sy, suv)
    dsts = [i * (slot + gap * eb) for i in range(n)]
    for i in range(n):
        tight, o, sy, suv = offs[i]
        planes.append(tight)
        assert lib.vp8g_make_tensor_desc(C.byref(opt), o[0], o[1], o[2], sy, suv, dsts[i], task0, C.byref(descs[i])) == 0
        task0 += descs[i].ntasks
    src = torch.from_numpy(np.concatenate(chunks)).to(dev)
    d_descs = vp8g.device_copy(descs)
    total = dsts[-1] + slot
    out = torch.full((eb + total + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(dev)
    assert lib.vp8g_tensor_batch_device(descs, C.c_void_p(d_descs.data_ptr()), n, C.byref(opt), C.c_void_p(src.data_ptr()),
                                        C.c_void_p(out.data_ptr() + eb), C.c_void_p(stream.cuda_stream)) == 0
    host = out.cpu().numpy()
    untouched = np.ones(host.size, bool)
    for i in range(n):
        exp = vp8g.host_tensor(planes[i], w, h, opt).view(INT_VIEW[vp8g._torch_dtype(opt)]).numpy().tobytes()
        assert len(exp) == slot
        lo = eb + dsts[i]
        assert host[lo:lo + slot].tobytes() == exp, (i, w, h, dtype, layout)
        untouched[lo:lo + slot] = False
    assert (host[untouched] == 0xEE).all()


def test_misaligned_base_is_refused_before_any_launch(vp8g):
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    for dtype, off in (("float16", 1), ("bfloat16", 1), ("float32", 1), ("float32", 2)):
        opt = vp8g.tensor_opt((16, 4), dtype, "NCHW")
        d = vp8g.Vp8gTensorDesc()
        assert lib.vp8g_make_tensor_desc(C.byref(opt), 0, 64, 80, 16, 8, 0, 0, C.byref(d)) == 0
        src = torch.zeros(96, dtype=torch.uint8, device=dev)
        d_d = vp8g.device_copy(d)
        out = torch.full((1024,), 0xEE, dtype=torch.uint8, device=dev)
        C.set_errno(0)
        assert lib.vp8g_tensor_batch_device(C.byref(d), C.c_void_p(d_d.data_ptr()), 1, C.byref(opt), C.c_void_p(src.data_ptr()),
                                            C.c_void_p(out.data_ptr() + off), None) == -1 and C.get_errno() == EINVAL
        files = (vp8g.ByteSpan * 1)()
        C.set_errno(0)
        assert lib.vp8g_decode_webp_batch_tensor(files, 1, 1, 0, 0, None, 0, C.byref(opt), C.c_void_p(out.data_ptr() + off),
                                                 None) == -1 and C.get_errno() == EINVAL
        torch.cuda.synchronize(dev)
        assert bool((out == 0xEE).all())


def test_scale_chains_into_the_tensor_kernel_on_the_device(vp8g):
    """vp8g_scale_batch_device -> vp8g_tensor_batch_device on one stream, no host copy in between:
    equals host_tensor(host_scale(...))."""
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    jobs = [(641, 479), (1920, 1080)]
    w = h = 224
    n = len(jobs)
    sopt = vp8g.scale_opt(scale=(w, h))
    topt = vp8g.tensor_opt((w, h), "float16", "NCHW", **IMAGENET)
    slot = lib.vp8g_tensor_slot_size(C.byref(topt))
    cw, ch = (w + 1) // 2, (h + 1) // 2
    sdescs, tdescs = (vp8g.Vp8gScaleDesc * n)(), (vp8g.Vp8gTensorDesc * n)()
    planes, so, do, st0, tt0 = [], 0, 0, 0, 0
    for i, (W, H) in enumerate(jobs):
        b = plane_input("random", W, H, 900 + i)
        planes.append(b)
        CW, CH = (W + 1) // 2, (H + 1) // 2
        assert lib.vp8g_make_scale_desc(W, H, so, so + W * H, so + W * H + CW * CH, W, CW, C.byref(sopt), do, st0,
                                        C.byref(sdescs[i])) == 0
        assert lib.vp8g_make_tensor_desc(C.byref(topt), do, do + w * h, do + w * h + cw * ch, w, cw, i * slot, tt0,
                                         C.byref(tdescs[i])) == 0
        so += len(b)
        do = (do + vp8g.i420_size(w, h) + 255) // 256 * 256
        st0 += sdescs[i].ntasks
        tt0 += tdescs[i].ntasks
    src = torch.from_numpy(np.frombuffer(b"".join(planes), dtype=np.uint8).copy()).to(dev)
    small = torch.empty(do + 16, dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3, h, w), dtype=torch.float16, device=dev)
    d_s = vp8g.device_copy(sdescs)
    d_t = vp8g.device_copy(tdescs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.vp8g_scale_batch_device(sdescs, C.c_void_p(d_s.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(small.data_ptr()), stream) == 0
    assert lib.vp8g_tensor_batch_device(tdescs, C.c_void_p(d_t.data_ptr()), n, C.byref(topt), C.c_void_p(small.data_ptr()),
                                        C.c_void_p(out.data_ptr()), stream) == 0
    got = out.cpu()
    for i, (W, H) in enumerate(jobs):
        scaled, _, _ = vp8g.host_scale(planes[i], W, H, sopt)
        assert same_bits(got[i], vp8g.host_tensor(scaled, w, h, topt)), (W, H)


E2E_FILES = ["big/k128_normal.webp", "commons/penguin-q20.webp", "big/fhd_normal_sharp5.webp", "big/fhd_simple_sharp3.webp"]


@pytest.fixture(scope="module")
def oracle_frames(vp8g):
    """(width, height, unfiltered I420, filtered I420) of the end-to-end fixtures, decoded once."""
    out = {}
    for rel in E2E_FILES:
        f = vp8g.decode_file(FIXTURES / rel)
        out[rel] = (f.width, f.height, vp8g.oracle_reconstruct(f, False), vp8g.oracle_reconstruct(f, True))
        f.free()
    return out


@pytest.mark.parametrize("device_m05", [False, True], ids=["host-m05", "device-m05"])
def test_decode_webp_batch_tensor_end_to_end(vp8g, oracle_frames, device_m05):
    """.webp -> 64x64 float16 NCHW with ImageNet normalisation: unfiltered, filtered with
    VP8G_SCALE_DWEBP_FILTER (libwebp's per-frame rule) and filtered without it."""
    files = [(FIXTURES / r).read_bytes() for r in E2E_FILES]
    topt = vp8g.tensor_opt((64, 64), "float16", "NCHW", **IMAGENET)
    for filtered, flag in ((False, False), (True, True), (True, False)):
        sopt = vp8g.scale_opt(scale=(64, 64), dwebp_filter=flag)
        out, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, scale=sopt, filtered=filtered, device_m05=device_m05)
        assert st == [0] * len(files)
        assert out.is_cuda and out.dtype == torch.float16 and tuple(out.shape) == (len(files), 3, 64, 64)
        got = out.cpu()
        for i, rel in enumerate(E2E_FILES):
            W, H, unf, filt = oracle_frames[rel]
            use = vp8g.host_lib().vp8f_scale_filtered(W, H, C.byref(sopt), int(filtered))
            scaled, sw, sh = vp8g.host_scale(filt if use else unf, W, H, sopt)
            assert (sw, sh) == (64, 64)
            assert same_bits(got[i], vp8g.host_tensor(scaled, 64, 64, topt)), (rel, filtered, flag)


@pytest.mark.parametrize("device_m05", [False, True], ids=["host-m05", "device-m05"])
def test_failed_frames_get_zero_slots(vp8g, oracle_frames, device_m05):
    """Per-frame options: one frame is an upscale (EINVAL), one a truncated file (its parse errno); their
    slots are zero bytes and the others are right."""
    rels = ["big/k128_normal.webp", "big/fhd_normal_sharp5.webp", "big/k128_normal.webp", None, "commons/penguin-q20.webp"]
    trunc = (ROOT / "tests" / "fixtures_err" / "truncated.webp").read_bytes()
    files = [(FIXTURES / r).read_bytes() if r else trunc for r in rels]
    w, h = 64, 48
    opts = [vp8g.scale_opt(scale=(w, h)), vp8g.scale_opt(crop=(100, 50, 999, 501), scale=(w, h)), vp8g.scale_opt(scale=(129, 64)),
            vp8g.scale_opt(scale=(w, h)), vp8g.scale_opt(scale=(w, h))]
    _, st_img = vp8g.gpu_decode_webp_batch_scaled(files, opts, filtered=True, device_m05=device_m05)
    assert st_img[3] != 0  # (the parse errno the image path reports for this file)
    topt = vp8g.tensor_opt((w, h), "float32", "NHWC", bgr=True, **IMAGENET)
    out, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, scale=opts, filtered=True, device_m05=device_m05)
    assert st == [0, 0, EINVAL, st_img[3], 0]
    got = out.cpu()
    for i, rel in enumerate(rels):
        if st[i]:
            assert not got[i].view(torch.int32).any(), i
            continue
        W, H, _, filt = oracle_frames[rel]
        scaled, _, _ = vp8g.host_scale(filt, W, H, opts[i])
        assert same_bits(got[i], vp8g.host_tensor(scaled, w, h, topt)), i
    # a frame whose scaled size is not the tensor's: EINVAL, zero slot (n_opts = 1)
    out, st = vp8g.gpu_decode_webp_batch_tensor(files[:2], topt, scale=vp8g.scale_opt(scale=(w, 0)), filtered=True,
                                                device_m05=device_m05)
    assert st == [EINVAL, EINVAL] and not out.cpu().view(torch.int32).any()  # (64 x 64 and 64 x 36)


@pytest.mark.parametrize("device_m05", [False, True], ids=["host-m05", "device-m05"])
def test_no_scale_mode(vp8g, device_m05):
    """opts NULL: two 128x128 fixtures into a 128x128 uint8 NHWC tensor = the RGB of their decode; a
    1920x1080 file in the same batch gets EINVAL and a zero slot."""
    rels = ["big/k128_normal.webp", "big/fhd_normal_sharp5.webp", "big/k128_normal.webp"]
    files = [(FIXTURES / r).read_bytes() for r in rels]
    topt = vp8g.tensor_opt((128, 128), "uint8", "NHWC")
    f = vp8g.decode_file(FIXTURES / rels[0])
    assert (f.width, f.height) == (128, 128)
    for filtered in (False, True):
        i420 = vp8g.oracle_reconstruct(f, filtered)
        ppm = vp8g.oracle_encode(i420, 128, 128, "ppm")
        exp = ppm[len(b"P6\n128 128\n255\n"):]
        out, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, filtered=filtered, device_m05=device_m05)
        assert st == [0, EINVAL, 0] and tuple(out.shape) == (3, 128, 128, 3) and out.dtype == torch.uint8
        got = out.cpu().numpy()
        assert got[0].tobytes() == exp and got[2].tobytes() == exp and not got[1].any()
    f.free()


def test_multi_partition(vp8g):
    """A multi-partition stream (opt-in) into 224x224: equals host_tensor(host_scale(...)) of the I420 the
    full-size path decodes (pinned to libwebp's bytes by tests/golden/multipart.json)."""
    name = "mp2_fhd_normal.webp"
    mp = json.loads((GOLDEN / "multipart.json").read_text())
    data = (ROOT / "tests" / "fixtures_mp" / name).read_bytes()
    sopt = vp8g.scale_opt(scale=(224, 224))
    topt = vp8g.tensor_opt((224, 224), "bfloat16", "NCHW", **IMAGENET)
    for device_m05 in (False, True):
        (res,), st = vp8g.gpu_decode_webp_batch_scaled([data], vp8g.scale_opt(), filtered=True, device_m05=device_m05,
                                                       multi_partition=True)
        assert st == [0]
        i420, W, H = res
        assert hashlib.sha256(i420).hexdigest() == mp["files"][name]["yuvf_sha256"]
        scaled, _, _ = vp8g.host_scale(i420, W, H, sopt)
        out, st = vp8g.gpu_decode_webp_batch_tensor([data, data], topt, scale=sopt, filtered=True, device_m05=device_m05,
                                                    multi_partition=True)
        assert st == [0, 0]
        exp = vp8g.host_tensor(scaled, 224, 224, topt)
        got = out.cpu()
        assert same_bits(got[0], exp) and same_bits(got[1], exp), device_m05
        # without the flag the stream is refused like the reference does, and the slot is zero
        out, st = vp8g.gpu_decode_webp_batch_tensor([data], topt, scale=sopt, filtered=True, device_m05=device_m05)
        assert st[0] != 0 and not out.cpu().view(torch.int16).any()
