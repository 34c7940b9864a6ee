"""GPU tests of libwebp's scaled RGB: the tensor kernel's 4:4:4 mode against host_tensor_444, the
4:4:4 scale descriptors through vp8g_scale_batch_device beside ordinary ones, the end-to-end route
(gpu_decode_webp_batch_tensor(..., libwebp_rgb=True)) and the CLI (`decoder -rgb`) against libwebp's own bytes (tests/golden/scale_rgb.json).

Bar: bit equality everywhere."""
import ctypes as C
import errno
import hashlib
import json
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_scale_rgb_host import CROPS, PLANE_SHAPES, random_i420

pytestmark = pytest.mark.gpu

INT_VIEW = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
# a picture narrower than a chunk, a chunk exactly, one pixel more, two chunks and their neighbours; then several tasks
# (13 x 260: 520 chunks of two a row), and a task boundary inside a row (3073 x 1: 257 chunks)
SHAPES = [(w, h) for w in (1, 2, 11, 12, 13, 23, 24, 25) for h in (1, 2, 3)] + [(13, 260), (3073, 1)]
DECODER = ROOT / "webp-decoder_amd" / "bin" / "decoder"


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def pictures(w, h, seed=0):
    """Three pictures as (Y, U, V) planes -- uniform bytes, 0 / 255 only (every clip of VP8YuvToRgb), uniform again -- and
    their alpha: a plane, none (opaque), a plane of 0 / 255."""
    rng = np.random.default_rng(1000 + 7 * w + h + seed)
    planes = [tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)),
              tuple(rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255) for _ in range(3)),
              tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3))]
    alpha = [rng.integers(0, 256, (h, w), dtype=np.uint8), None, rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255)]
    return planes, alpha


def check_444(vp8g, w, h, opt, with_alpha, **stage):
    planes, alpha = pictures(w, h)
    got = vp8g.gpu_tensor_444(planes, w, h, opt, alpha if with_alpha else None, **stage)
    return [i for i in range(len(planes))
            if not same_bits(got[i], vp8g.host_tensor_444(planes[i], opt, ("opaque" if alpha[i] is None else alpha[i]) if with_alpha else None))]


@pytest.mark.parametrize("dtype", ["uint8", "float16", "bfloat16", "float32"])
def test_every_option_on_one_shape(vp8g, dtype):
    """13 x 3: a whole chunk and a partial one per row; an opaque and a non-opaque picture in one launch."""
    bad = []
    for layout in ("NHWC", "NCHW"):
        for bgr in (False, True):
            for norm in ([dict()] if dtype == "uint8" else [dict(), dict(scale=1 / 255), IMAGENET]):
                for with_alpha in (False, True):
                    opt = vp8g.tensor_opt((13, 3), dtype, layout, bgr=bgr, **norm)
                    bad += [(layout, bgr, with_alpha, i) for i in check_444(vp8g, 13, 3, opt, with_alpha)]
    assert not bad, bad


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_vs_host_tensor_444(vp8g, w, h):
    bad = []
    for dtype, layout in (("uint8", "NHWC"), ("uint8", "NCHW"), ("float16", "NCHW"), ("float16", "NHWC")):
        for with_alpha in (False, True):
            opt = vp8g.tensor_opt((w, h), dtype, layout, **(dict() if dtype == "uint8" else IMAGENET))
            bad += [(dtype, layout, with_alpha, i) for i in check_444(vp8g, w, h, opt, with_alpha)]
    assert not bad, bad


@pytest.mark.parametrize("shift,pad", [(1, 0), (3, 5), (0, 0), (15, 1)])
def test_slots_off_a_dword_and_planes_at_odd_offsets(vp8g, shift, pad):
    """Three 3 x 3 uint8 pictures (27-byte slots: the second and third start off a dword) and 25 x 3 ones, every plane
    `shift` bytes off a 16-byte boundary with `pad` bytes between its rows; the guard bytes around every slot stay
    (gpu_tensor_444 raises if not)."""
    bad = []
    for w, h in ((3, 3), (25, 3)):
        for layout in ("NHWC", "NCHW"):
            for with_alpha in (False, True):
                opt = vp8g.tensor_opt((w, h), "uint8", layout)
                bad += [(w, layout, with_alpha, i) for i in check_444(vp8g, w, h, opt, with_alpha, guard=1 if w == 3 else 64, src_shift=shift, src_pad=pad)]
    assert not bad, bad
    st = vp8g.stage_tensor_444(pictures(3, 3)[0], 3, 3, vp8g.tensor_opt((3, 3), "uint8", "NHWC"), guard=1)
    assert [o % 4 for o, _ in st.dst.regions] == [1, 1, 1] and [n for _, n in st.dst.regions] == [27] * 3


def test_launch_refusals(vp8g):
    """vp8g_tensor_batch_device_444 refuses before it launches: EINVAL, and the output still holds its fill."""
    w, h = 13, 3
    planes, alpha = pictures(w, h)
    u8, f16 = vp8g.tensor_opt((w, h), "uint8", "NHWC"), vp8g.tensor_opt((w, h), "float16", "NCHW")

    def refused(opt=u8, with_alpha=False, **kw):
        st = vp8g.stage_tensor_444(planes, w, h, opt, alpha if with_alpha else None)
        mutate = kw.pop("mutate", None)
        with pytest.raises(ValueError, match="EINVAL"):
            vp8g.run_tensor_444(st, mutate=(lambda: mutate(st)) if mutate else None, einval=ValueError, **kw)

    for name in ("descs", "d_descs", "src", "dst"):
        refused(null=(name,))
    for name in ("alpha", "d_alpha"):
        refused(with_alpha=True, null=(name,))
    refused(channels=2)
    refused(channels=0)
    refused(channels=5)
    refused(with_alpha=True, channels=3)  # three channels with alpha arrays
    refused(channels=4)                   # four without
    refused(mutate=lambda st: setattr(st.descs[1], "stride_y", w - 1))
    refused(mutate=lambda st: setattr(st.descs[1], "stride_uv", w - 1))  # (the 4:2:0 kernel's minimum is no pass here)
    refused(mutate=lambda st: setattr(st.descs[2], "stride_uv", (w + 1) // 2))
    refused(with_alpha=True, mutate=lambda st: setattr(st.alpha[0], "stride_a", w - 1))
    refused(mutate=lambda st: setattr(st.descs[1], "task0", st.descs[1].task0 + 1))  # tasks out of order
    refused(mutate=lambda st: setattr(st.descs[0], "ntasks", 2))
    refused(opt=f16, mutate=lambda st: setattr(st.descs[0], "dst", st.descs[0].dst + 1))  # a slot off the element size
    refused(opt=f16, ptr_shift=(0, 1))                                                    # ... and the tensor's base
    # and the same staging goes through untouched
    st = vp8g.stage_tensor_444(planes, w, h, f16, alpha)
    got = vp8g.run_tensor_444(st, einval=ValueError)
    assert all(same_bits(got[i], vp8g.host_tensor_444(planes[i], f16, "opaque" if alpha[i] is None else alpha[i])) for i in range(3))


def test_scale_descriptors_beside_ordinary_ones(vp8g):
    """Every plane shape of the host test as a 4:4:4 descriptor, an ordinary I420 descriptor and a single-plane (alpha)
    one between them, in ONE vp8g_scale_batch_device call: each output equals the host restatement."""
    jobs = []
    for p in PLANE_SHAPES:
        (w, h), target, expand = p.values
        jobs.append(("444", random_i420(w, h, seed=w * 131 + h), w, h, vp8g.scale_opt(scale=target, expand=expand)))
    for crop, scale in CROPS:
        jobs.append(("444", random_i420(128, 128, seed=7), 128, 128, vp8g.scale_opt(crop=crop, scale=scale)))
    jobs.insert(3, ("420", random_i420(33, 31, seed=5), 33, 31, vp8g.scale_opt(scale=(20, 10))))
    plane = np.random.default_rng(9).integers(0, 256, (31, 33), dtype=np.uint8)
    jobs.insert(7, ("plane", plane, 33, 31, vp8g.scale_opt(crop=(3, 5, 20, 20), scale=(9, 0))))
    st = vp8g.stage_scale_batch(jobs)
    assert any(d.p[1].group == 0 and d.p[0].group != 0 for d in st.descs)  # a shrinking luma beside an expanding chroma
    got = vp8g.gpu_scale_batch(jobs)
    for i, ((kind, data, w, h, opt), out) in enumerate(zip(jobs, got)):
        if kind == "444":
            assert np.array_equal(out, vp8g.host_scale_yuv444(data, w, h, opt)), (i, w, h)
        elif kind == "420":
            assert out.tobytes() == vp8g.host_scale(data, w, h, opt)[0], i
        else:
            assert np.array_equal(out, vp8g.host_scale_plane(data, opt)), i
    # the wrapper of the 4:4:4 ones alone
    only = [j for j in jobs if j[0] == "444"][:4]
    for j, out in zip(only, vp8g.gpu_scale_yuv444([j[1] for j in only], [(j[2], j[3]) for j in only], [j[4] for j in only])):
        assert np.array_equal(out, vp8g.host_scale_yuv444(j[1], j[2], j[3], j[4]))


# ---- end to end ----------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "scale_rgb.json").read_text())


def case_opt(vp8g, c):
    return vp8g.scale_opt(crop=c["crop"], scale=c["scale"], dwebp_filter=True, expand=c["expand"])


def case_id(c):
    return f'{c["file"].split("/")[-1]}-{c["crop"]}-{c["scale"]}'


def golden_cases():
    return json.loads((GOLDEN / "scale_rgb.json").read_text())["rgba"]


@pytest.mark.parametrize("c", golden_cases(), ids=case_id)
def test_end_to_end_vs_libwebp(vp8g, c):
    """Every golden case, 4 channels (libwebp's MODE_RGBA bytes) and 3 (the same without A); the cases without a target
    size take the 4:2:0 route, which is libwebp's for them."""
    data = (ROOT / c["file"]).read_bytes()
    topt = vp8g.tensor_opt(c["size"], "uint8", "NHWC")
    kw = dict(scale=case_opt(vp8g, c), libwebp_rgb=True)
    rgba, st = vp8g.gpu_decode_webp_batch_tensor([data], topt, alpha=True, **kw)
    rgba = rgba.cpu().numpy()
    assert st == [0] and rgba.nbytes == c["bytes"] and hashlib.sha256(rgba.tobytes()).hexdigest() == c["sha256"]
    rgb, st = vp8g.gpu_decode_webp_batch_tensor([data], topt, **kw)
    assert st == [0] and np.array_equal(rgb.cpu().numpy(), rgba[..., :3])


@pytest.mark.parametrize("c", golden_cases(), ids=case_id)
def test_existing_route_keeps_its_output(vp8g, c):
    """Without libwebp_rgb the same file and option give what they gave before: the encoder's RGB (fancy upsampling) of
    the scaled I420 -- host_tensor on host_scale's I420 -- which for a target size is not libwebp's."""
    data = (ROOT / c["file"]).read_bytes()
    topt, opt = vp8g.tensor_opt(c["size"], "uint8", "NHWC"), case_opt(vp8g, c)
    f = vp8g.decode_lossy_still(data)
    i420 = vp8g.oracle_reconstruct(f, bool(vp8g.host_lib().vp8f_scale_filtered(f.width, f.height, C.byref(opt), 1)))
    small, w, h = vp8g.host_scale(i420, f.width, f.height, opt)
    f.free()
    got, st = vp8g.gpu_decode_webp_batch_tensor([data], topt, scale=opt, extended=True)
    assert st == [0] and same_bits(got[0].cpu(), vp8g.host_tensor(small, w, h, topt))
    if c["scale"] and w * h > 16:
        assert hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() != hashlib.sha256(
            vp8g.host_still_scaled_rgb(data, opt, 3).tobytes()).hexdigest()


@pytest.mark.parametrize("device_m05", [False, True], ids=["host-m05", "device-m05"])
@pytest.mark.parametrize("chunk_frames", [0, 1], ids=["one-chunk", "a-chunk-each"])
def test_mixed_batch_with_per_frame_options(vp8g, device_m05, chunk_frames, monkeypatch):
    """A frame with a target size, a crop-only frame, a lossless file (VP8G_X_LOSSLESS_SCALE) and a file that does not
    parse in one batch -- in one chunk, so that the chunk makes both tensor launches, and in a chunk each."""
    if chunk_frames:
        monkeypatch.setenv("VP8G_CHUNK_FRAMES", str(chunk_frames))
    W, H = 32, 20
    S = vp8g.scale_opt
    k128 = (ROOT / "tests/fixtures/big/k128_normal.webp").read_bytes()
    files = [(GOLDEN / "alpha" / "ll_disc_f3.webp").read_bytes(), k128, (GOLDEN / "lossless" / "disc_67x45_m4q75.webp").read_bytes(),
             b"RIFF\x10\0\0\0WEBPjunkjunkjunk", k128, (GOLDEN / "alpha" / "enc_q50_af1.webp").read_bytes()]
    opts = [S(scale=(W, H), dwebp_filter=True), S(crop=(3, 5, W, H)), S(crop=(1, 3, 64, 40), scale=(W, H)), S(scale=(W, H)),
            S(crop=(7, 9, 31, 17), scale=(W, H), expand=True, dwebp_filter=True), S(scale=(W, 0))]  # (the last: 32 x 24, not the tensor's size)
    for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW")):
        topt = vp8g.tensor_opt((W, H), dtype, layout, **(dict() if dtype == "uint8" else IMAGENET))
        kw = dict(scale=opts, device_m05=device_m05, alpha=True, lossless=True, lossless_scale=True)
        got, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, libwebp_rgb=True, **kw)
        old, st_old = vp8g.gpu_decode_webp_batch_tensor(files, topt, **kw)
        got, old = got.cpu(), old.cpu()
        assert st == st_old == [0, 0, 0, errno.EINVAL, 0, errno.EINVAL]
        for i in (0, 4):  # a target size: libwebp's RGBA
            want = vp8g.host_still_scaled_rgb(files[i], opts[i], 4)
            planes = [want[..., k] for k in range(4)]  # (R, G, B as "planes" would need the inverse conversion: compare as elements)
            rgb_elems = vp8g._rgb_elements(want[..., :3], topt)
            a_elems = vp8g.host_alpha_channel(planes[3], topt)
            planar = layout == "NCHW"
            exp = torch.cat([rgb_elems, a_elems.unsqueeze(0 if planar else 2)], dim=0 if planar else 2)
            assert same_bits(got[i], exp.contiguous()), i
            assert not same_bits(got[i], old[i]), i
        for i in (1, 2):  # crop only, and the lossless file: the existing routes
            assert same_bits(got[i], old[i]) and bool(old[i].view(INT_VIEW[old.dtype]).any()), i
        for i in (3, 5):  # failed frames: zero slots
            assert not bool(got[i].view(INT_VIEW[got.dtype]).any()), i


def test_entry_point_refusals(vp8g):
    """The new entry point's own argument checks are those of _any; and the bits that existing tests pin as EINVAL on
    the old entry points stay so."""
    lib = vp8g.gpu_lib()
    data = (ROOT / "tests/fixtures/big/k128_normal.webp").read_bytes()
    bufs, spans = vp8g.S.file_spans([data])
    topt, opt = vp8g.tensor_opt((64, 64), "uint8", "NHWC"), vp8g.scale_opt(scale=(64, 64))
    out = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
    st = (C.c_int * 1)()

    def call(fn, xflags, n_opts=1, bflags=0):
        C.set_errno(0)
        rc = fn(spans, 1, 1, 1, bflags, C.byref(opt), n_opts, C.byref(topt), xflags, C.c_void_p(out.data_ptr()), st)
        return rc, C.get_errno()

    for x in (4, 8, 6, 32, 16):  # unknown bits; VP8G_X_LOSSLESS_SCALE without VP8G_X_LOSSLESS
        assert call(lib.vp8g_decode_webp_batch_tensor_rgb, x) == (-1, errno.EINVAL), x
    for x in (4, 8, 6):
        assert call(lib.vp8g_decode_webp_batch_tensor_any, x) == (-1, errno.EINVAL), x
    assert call(lib.vp8g_decode_webp_batch_tensor_rgb, 0, n_opts=2) == (-1, errno.EINVAL)
    assert call(lib.vp8g_decode_webp_batch_tensor_rgb, 0, bflags=4) == (-1, errno.EINVAL)
    assert not bool(out.any())
    assert call(lib.vp8g_decode_webp_batch_tensor_rgb, 0) == (0, 0) and bool(out.any())


# ---- the CLI -------------------------------------------------------------------------------------


def run_decoder(*args):
    return subprocess.run([str(DECODER), *[str(a) for a in args]], capture_output=True, timeout=120)


def test_cli_ppm_scaled_vs_libwebp(vp8g, golden, tmp_path):
    k128 = ROOT / "tests/fixtures/big/k128_normal.webp"
    for c, args in zip(golden["rgb"], [("-scale", 64, 64), ("-crop", 3, 5, 101, 99, "-scale", 50, 0)]):
        out = tmp_path / "out.ppm"
        r = run_decoder("-rgb", *args, k128, out)
        assert r.returncode == 0, r.stderr
        data = out.read_bytes()
        head = b"P6\n%d %d\n255\n" % tuple(c["size"])
        assert data.startswith(head) and len(data) == len(head) + c["bytes"]
        assert hashlib.sha256(data[len(head):]).hexdigest() == c["sha256"]
    # an expanding target, against the host restatement
    r = run_decoder("-rgb", "-scale", 200, 131, "-expand", k128, tmp_path / "big.ppm")
    assert r.returncode == 0, r.stderr
    want = vp8g.host_still_scaled_rgb(k128.read_bytes(), vp8g.scale_opt(scale=(200, 131), expand=True, dwebp_filter=True), 3)
    assert (tmp_path / "big.ppm").read_bytes() == b"P6\n200 131\n255\n" + want.tobytes()
    assert run_decoder("-rgb", "-scale", 200, 131, k128, tmp_path / "no.ppm").returncode == 1  # (upscale needs -expand)


def test_cli_ppm_without_a_target_size_is_the_m08_file(vp8g, golden, tmp_path):
    k128 = ROOT / "tests/fixtures/big/k128_normal.webp"
    f = vp8g.decode_file(k128)
    i420 = vp8g.oracle_reconstruct(f, True)
    w, h = f.width, f.height
    f.free()
    for mode in ("-ppm", "-rgb"):
        r = run_decoder(mode, k128, tmp_path / "plain.ppm")
        assert r.returncode == 0 and (tmp_path / "plain.ppm").read_bytes() == vp8g.oracle_encode(i420, w, h, "ppm")
    # crop only: the m08 writer on the window; its pixels are libwebp's (the golden's RGBA without A)
    r = run_decoder("-rgb", "-crop", 3, 5, 101, 99, k128, tmp_path / "crop.ppm")
    win, cw, ch = vp8g.host_scale(i420, w, h, vp8g.scale_opt(crop=(3, 5, 101, 99)))
    data = (tmp_path / "crop.ppm").read_bytes()
    assert r.returncode == 0 and data == vp8g.oracle_encode(win, cw, ch, "ppm")
    c = next(c for c in golden["rgba"] if c["crop"] == [3, 5, 101, 99] and c["scale"] is None)
    rgba = np.concatenate([np.frombuffer(data, np.uint8)[-3 * cw * ch:].reshape(ch, cw, 3), np.full((ch, cw, 1), 255, np.uint8)], axis=2)
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == c["sha256"]


def test_cli_usage(tmp_path):
    k128 = ROOT / "tests/fixtures/big/k128_normal.webp"
    out = tmp_path / "o"
    assert run_decoder("-png", "-scale", 64, 64, k128, out).returncode == 2
    assert run_decoder("-png", "-crop", 0, 0, 8, 8, k128, out).returncode == 2
    assert run_decoder("-ppm", "-scale", 64, 64, k128, out).returncode == 2  # (-ppm keeps refusing the options: tests/test_gpu_scale.py)
    assert run_decoder("-ppm", "-crop", 0, 0, 8, 8, k128, out).returncode == 2
    assert run_decoder("-rgb", "-expand", k128, out).returncode == 2
    assert run_decoder("-rgb", "-scale", 64, k128, out).returncode == 2
    assert not out.exists()
