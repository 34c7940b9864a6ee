"""GPU tests (MI355X) of the rescaler's expand path (VP8G_SCALE_EXPAND): the expand kernel
(webp-decoder_amd/csrc/vp8g_scale.hip) behind vp8g_scale_batch_device, yuv420_rescale,
vp8g_decode_webp_batch_scaled, vp8g_decode_webp_batch_tensor and `decoder -yuv|-yuvf -scale w h -expand`.

Bar: byte equality -- with the host restatement (host/vp8_scale.c, itself pinned to libwebp's bytes in
tests/test_scale_expand_host.py) and with libwebp's own output (tests/golden/scale_expand.json)."""
import ctypes as C
import hashlib
import json
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EINVAL = 22
DECODER = ROOT / "webp-decoder_amd" / "bin" / "decoder"
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "scale_expand.json").read_text())


def plane_input(kind, w, h, seed):
    """The generators scale.json records ("inputs")."""
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "binary":
        return (np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8) * np.uint8(255)).tobytes()
    assert kind == "ones"
    return bytes([255]) * n


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def golden_plane_cases():
    g = json.loads((GOLDEN / "scale_expand.json").read_text())
    return sorted({tuple(c["src"]) + tuple(c["dst"]) for c in g["planes"]})


@pytest.mark.parametrize("W,H,w,h", golden_plane_cases())
def test_plane_cases_vs_host_and_libwebp(vp8g, golden, W, H, w, h):
    """gpu_scale (yuv420_rescale) vs host_scale and vs WebPPictureRescale's bytes: random, all-255 and
    0/255 inputs, every plane case of scale_expand.json."""
    cases = [c for c in golden["planes"] if c["src"] == [W, H] and c["dst"] == [w, h]]
    assert len(cases) == 3
    opt = vp8g.scale_opt(scale=(w, h), expand=True)
    for c in cases:
        src = plane_input(c["kind"], W, H, c["seed"])
        got, gw, gh = vp8g.gpu_scale(src, W, H, opt)
        exp, ew, eh = vp8g.host_scale(src, W, H, opt)
        assert (gw, gh) == (ew, eh) == (w, h)
        assert got == exp, (c["kind"], first_diff(got, exp))
        assert sha(got) == c["sha256"], c["kind"]


def test_upscale_without_the_flag_is_still_einval(vp8g):
    with pytest.raises((RuntimeError, ValueError)):
        vp8g.gpu_scale(plane_input("random", 16, 16, 1), 16, 16, vp8g.scale_opt(scale=(17, 16)))


def test_mixed_batch_of_shrinking_and_expanding_images(vp8g):
    """vp8g_scale_batch_device: 32 random sizes up to 300x300 with targets up to 400x400 in one call (two
    launches), every x / y mode combination at least three times; source strides padded with noise, the
    source base at an odd offset; every image equals the host result and no byte outside the images is
    written.  A descriptor whose task0 is off by one is refused before any launch."""
    import torch
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    rng = np.random.default_rng(41)
    jobs = []
    for i in range(32):
        W, H = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        xe, ye = bool(i & 1), bool(i & 2)  # luma: x expands / y expands
        w = int(rng.integers(W + 1, 401)) if xe else int(rng.integers(1, W + 1))
        h = int(rng.integers(H + 1, 401)) if ye else int(rng.integers(1, H + 1))
        jobs.append((W, H, w, h))
    modes = [(W < w, H < h) for W, H, w, h in jobs]
    for m in ((False, False), (True, False), (False, True), (True, True)):
        assert modes.count(m) >= 3, m
    n = len(jobs)
    descs = (vp8g.Vp8gScaleDesc * n)()
    chunks, planes, outs, so, do, task0 = [], [], [], 5, 3, 0  # (source planes and the first image at odd offsets)
    for i, (W, H, w, h) in enumerate(jobs):
        tight = plane_input("random", W, H, 700 + i)
        planes.append(tight)
        a = np.frombuffer(tight, np.uint8)
        CW, CH = (W + 1) // 2, (H + 1) // 2
        sy, suv = W + int(rng.integers(0, 40)), CW + int(rng.integers(0, 23))
        offs = []
        for pl, pw, ph, st in ((a[:W * H], W, H, sy), (a[W * H:W * H + CW * CH], CW, CH, suv), (a[W * H + CW * CH:], CW, CH, suv)):
            buf = rng.integers(0, 256, size=st * ph, dtype=np.uint8).reshape(ph, st)  # padding = noise
            buf[:, :pw] = pl.reshape(ph, pw)
            offs.append(so)
            chunks.append(buf.reshape(-1))
            so += buf.size
        opt = vp8g.scale_opt(scale=(w, h), expand=True)
        assert lib.vp8g_make_scale_desc(W, H, offs[0], offs[1], offs[2], sy, suv, C.byref(opt), do, task0,
                                        C.byref(descs[i])) == 0
        outs.append(do)
        do = do + vp8g.i420_size(w, h) + int(rng.integers(1, 70))  # (images at every alignment)
        task0 += descs[i].ntasks
    src = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8)] + chunks)).to(dev)
    d_descs = vp8g.device_copy(descs)
    out = torch.full((do + 64,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    assert lib.vp8g_scale_batch_device(descs, C.c_void_p(d_descs.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)) == 0
    host = out.cpu().numpy()
    untouched = np.ones(host.size, bool)
    for i, (W, H, w, h) in enumerate(jobs):
        exp, _, _ = vp8g.host_scale(planes[i], W, H, vp8g.scale_opt(scale=(w, h), expand=True))
        got = host[outs[i]:outs[i] + len(exp)].tobytes()
        assert got == exp, (i, W, H, w, h, first_diff(got, exp))
        untouched[outs[i]:outs[i] + len(exp)] = False
    assert (host[untouched] == 0xEE).all()
    # inconsistent task numbering is refused before any launch
    descs[1].task0 += 1
    out.fill_(0xEE)
    C.set_errno(0)
    assert lib.vp8g_scale_batch_device(descs, C.c_void_p(d_descs.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)) == -1
    assert C.get_errno() == EINVAL
    assert bool((out == 0xEE).all())
    # and so is an expanding plane whose tiling was tampered with
    descs[1].task0 -= 1
    k = next(i for i, m in enumerate(modes) if m == (True, True))
    descs[k].p[0].run_h += 1
    C.set_errno(0)
    assert lib.vp8g_scale_batch_device(descs, C.c_void_p(d_descs.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)) == -1
    assert C.get_errno() == EINVAL


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
def test_decode_webp_batch_scaled_vs_libwebp(vp8g, golden, device_m05):
    """vp8g_decode_webp_batch_scaled on the fixture cases of scale_expand.json: filtered = 0 vs WebPDecode
    with bypass_filtering, filtered = 1 + VP8G_SCALE_DWEBP_FILTER vs WebPDecode as it is."""
    cases = [c for c in golden["decode"] if c["bypass"] == 0]
    by_key = {(c["file"], tuple(c["crop"] or ()), tuple(c["scale"]), c["bypass"]): c for c in golden["decode"]}
    files = [(FIXTURES / c["file"]).read_bytes() for c in cases]
    opts = [vp8g.scale_opt(crop=c["crop"], scale=c["scale"], dwebp_filter=True, expand=True) for c in cases]
    for filtered in (False, True):
        res, st = vp8g.gpu_decode_webp_batch_scaled(files, opts, filtered=filtered, device_m05=device_m05)
        assert st == [0] * len(cases)
        for c, r in zip(cases, res):
            got, gw, gh = r
            assert [gw, gh] == c["size"], (c["file"], c["scale"])
            g = by_key[(c["file"], tuple(c["crop"] or ()), tuple(c["scale"]), 0 if filtered else 1)]
            assert sha(got) == g["sha256"], (c["file"], c["crop"], c["scale"], filtered)


def test_decode_webp_batch_scaled_per_frame_options(vp8g, oracle_frames):
    """Per-frame options over mixed fixtures: the upscaling frame that carries the flag is decoded, the
    upscaling frame without it gets EINVAL, the downscaling frames are as before."""
    rels = ["big/k128_normal.webp", "big/fhd_normal_sharp5.webp", "commons/penguin-q20.webp", "big/k128_normal.webp",
            "big/fhd_simple_sharp3.webp"]
    opts = [vp8g.scale_opt(scale=(200, 0)), vp8g.scale_opt(crop=(100, 50, 999, 501), scale=(0, 100)),
            vp8g.scale_opt(scale=(224, 224)), vp8g.scale_opt(scale=(129, 64), expand=True),
            vp8g.scale_opt(crop=(7, 9, 640, 480), expand=True)]
    files = [(FIXTURES / r).read_bytes() for r in rels]
    for device_m05 in (False, True):
        res, st = vp8g.gpu_decode_webp_batch_scaled(files, opts, filtered=True, device_m05=device_m05)
        assert st == [EINVAL, 0, 0, 0, 0] and res[0] is None
        for i in (1, 2, 3, 4):
            W, H, _, filt = oracle_frames[rels[i]]
            assert res[i] == vp8g.host_scale(filt, W, H, opts[i]), (i, device_m05)
        assert res[3][1:] == (129, 64)


TENSOR_FILES = ["gen_noise_16x16_q90", "gen_noise_17x17_q90", "gen_noise_31x31_q50", "gen_checker_32x32_q50",
                "gen_checker_33x33_q50", "gen_noise_63x63_q10", "gen_diag_64x64_q50", "gen_noise_127x127_q50",
                "gen_checker_129x129_q90", "gen_checker_400x416_q90", "gen_diag_384x416_q100", "gen_noise_416x384_q10"]


@pytest.mark.parametrize("device_m05", [False, True], ids=["host-m05", "device-m05"])
def test_decode_webp_batch_tensor_224(vp8g, device_m05):
    """vp8g_decode_webp_batch_tensor: twelve fixtures from 16x16 to 416x384 into [12, 3, 224, 224] float16
    with the flag: every slot bit-equal to host_tensor(host_scale(...)).  Without the flag exactly the
    frames smaller than 224 in a dimension get EINVAL and a zero slot."""
    import torch
    files = [(FIXTURES / "generated" / (n + ".webp")).read_bytes() for n in TENSOR_FILES]
    topt = vp8g.tensor_opt((224, 224), "float16", "NCHW", **IMAGENET)
    sopt = vp8g.scale_opt(scale=(224, 224), expand=True)
    exp, small = [], []
    for n in TENSOR_FILES:
        f = vp8g.decode_file(FIXTURES / "generated" / (n + ".webp"))
        scaled, w, h = vp8g.host_scale(vp8g.oracle_reconstruct(f, True), f.width, f.height, sopt)
        assert (w, h) == (224, 224)
        small.append(f.width < 224 or f.height < 224)
        exp.append(vp8g.host_tensor(scaled, 224, 224, topt))
        f.free()
    assert small.count(True) == 9 and small.count(False) == 3
    out, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, scale=sopt, filtered=True, device_m05=device_m05)
    assert st == [0] * len(files)
    got = out.cpu()
    for i in range(len(files)):
        assert torch.equal(got[i].view(torch.int16), exp[i].view(torch.int16)), TENSOR_FILES[i]
    out, st = vp8g.gpu_decode_webp_batch_tensor(files, topt, scale=vp8g.scale_opt(scale=(224, 224)), filtered=True,
                                                device_m05=device_m05)
    assert st == [EINVAL if s else 0 for s in small]
    got = out.cpu()
    for i in range(len(files)):
        if small[i]:
            assert not got[i].view(torch.int16).any(), TENSOR_FILES[i]
        else:
            assert torch.equal(got[i].view(torch.int16), exp[i].view(torch.int16)), TENSOR_FILES[i]


def test_expanded_i420_chains_into_the_encoder_on_the_device(vp8g):
    """The scale -> encoder chain on one stream for one expanding image: equals
    oracle_encode(host_scale(...))."""
    import torch
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    W, H, w, h = 100, 60, 224, 224
    b = plane_input("random", W, H, 950)
    CW, CH, cw, ch = (W + 1) // 2, (H + 1) // 2, (w + 1) // 2, (h + 1) // 2
    opt = vp8g.scale_opt(scale=(w, h), expand=True)
    sdescs = (vp8g.Vp8gScaleDesc * 1)()
    assert lib.vp8g_make_scale_desc(W, H, 0, W * H, W * H + CW * CH, W, CW, C.byref(opt), 0, 0, C.byref(sdescs[0])) == 0
    edescs, eouts, etotal, spans = vp8g.make_enc_descs([(w, h)], "rgb", [(0, w * h, w * h + cw * ch)])
    src = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    small = torch.empty(vp8g.i420_size(w, h) + 16, dtype=torch.uint8, device=dev)
    rgb = torch.empty(etotal + 16, dtype=torch.uint8, device=dev)
    work = torch.empty(lib.vp8g_encode_workspace_size(spans), dtype=torch.uint8, device=dev)
    d_s = vp8g.device_copy(sdescs)
    d_e = vp8g.device_copy(edescs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.vp8g_scale_batch_device(sdescs, C.c_void_p(d_s.data_ptr()), 1, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(small.data_ptr()), stream) == 0
    assert lib.vp8g_encode_batch_device(edescs, C.c_void_p(d_e.data_ptr()), 1, C.c_void_p(small.data_ptr()),
                                        C.c_void_p(rgb.data_ptr()), C.c_void_p(work.data_ptr()), stream) == 0
    host = rgb.cpu().numpy().tobytes()
    scaled, _, _ = vp8g.host_scale(b, W, H, opt)
    ppm = vp8g.oracle_encode(scaled, w, h, "ppm")
    exp = ppm[len(b"P6\n%d %d\n255\n" % (w, h)):]
    assert host[eouts[0]:eouts[0] + len(exp)] == exp


def test_cli_expand(golden, tmp_path):
    """`decoder -yuv|-yuvf -scale w h -expand` writes dwebp's bytes; -expand without -scale is a usage
    error; an upscale without -expand is refused as before."""
    def gold(rel, crop, scale, bypass):
        return next(c for c in golden["decode"] if c["file"] == rel and c["crop"] == crop and c["scale"] == scale
                    and c["bypass"] == bypass)
    k128 = str(FIXTURES / "big/k128_normal.webp")
    out = tmp_path / "o.i420"
    r = subprocess.run([str(DECODER), "-yuvf", "-scale", "64", "300", "-expand", k128, str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sha(out.read_bytes()) == gold("big/k128_normal.webp", None, [64, 300], 0)["sha256"]
    r = subprocess.run([str(DECODER), "-yuv", "-crop", "3", "5", "101", "99", "-scale", "224", "0", "-expand", k128, str(out)],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sha(out.read_bytes()) == gold("big/k128_normal.webp", [3, 5, 101, 99], [224, 0], 1)["sha256"]
    for args in (["-yuv", "-expand"], ["-yuv", "-crop", "0", "0", "8", "8", "-expand"],
                 ["-yuv", "-scale", "200", "200", "-expand", "-expand"], ["-ppm", "-scale", "200", "200", "-expand"]):
        r = subprocess.run([str(DECODER)] + args + [k128, str(out)], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"Usage" in r.stderr, args
    r = subprocess.run([str(DECODER), "-yuv", "-scale", "129", "64", k128, str(out)], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"downscale only" in r.stderr
