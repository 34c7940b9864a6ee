"""GPU tests (MI355X) of decode-to-a-target-size: the crop + downscale kernel
(webp-decoder_amd/csrc/vp8g_scale.hip) behind vp8g_scale_batch_device, yuv420_rescale,
vp8g_decode_webp_batch_scaled and `decoder -yuv|-yuvf [-crop] [-scale]`.

Bar: byte equality -- with the host restatement (host/vp8_scale.c, itself pinned to libwebp's bytes
in tests/test_scale_host.py) and with libwebp's own output (tests/golden/scale.json)."""
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


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


# identity, ratios just under 1, huge ratios, tiles that straddle the workgroup tile width, both
# maximum dimensions, an accumulator that wraps 2^32 (8192x2100 -> 1x1, all-255 only)
PLANE_CASES = [
    (1, 1, 1, 1), (2, 2, 1, 1), (16, 16, 16, 16), (17, 13, 16, 12), (16, 16, 1, 1), (33, 31, 7, 5), (64, 48, 63, 47),
    (129, 77, 64, 38), (100, 100, 33, 34), (257, 3, 3, 3), (3, 257, 3, 2), (5, 5, 5, 1), (5, 5, 1, 5), (1000, 7, 999, 1),
    (255, 255, 254, 3), (640, 480, 224, 224), (16383, 2, 5, 1), (2, 16383, 1, 7), (1920, 1080, 224, 224),
    (3840, 2160, 1, 1), (8192, 2100, 1, 1), (3840, 64, 3, 64),
]


@pytest.mark.parametrize("W,H,w,h", PLANE_CASES)
def test_plane_cases_vs_host_and_libwebp(vp8g, golden, W, H, w, h):
    """gpu_scale (yuv420_rescale) vs host_scale and vs WebPPictureRescale's bytes: random, all-255 and
    0/255 inputs."""
    cases = [c for c in golden["planes"] if c["src"] == [W, H] and c["dst"] == [w, h]]
    assert cases, "case missing from tests/golden/scale.json"
    opt = vp8g.scale_opt(scale=(w, h))
    for c in cases:
        src = plane_input(c["kind"], W, H, c["seed"])
        got, gw, gh = vp8g.gpu_scale(src, W, H, opt)
        exp, ew, eh = vp8g.host_scale(src, W, H, opt)
        assert (gw, gh) == (ew, eh) == (w, h)
        assert got == exp, (c["kind"], first_diff(got, exp))
        assert sha(got) == c["sha256"], c["kind"]


def test_mixed_size_batch_one_launch(vp8g):
    """vp8g_scale_batch_device: 40 mixed sizes + 3840x2160 -> 640x360 + 1x1 in one launch, source
    strides padded beyond the width; every image equals the host result and no byte outside the
    images is written."""
    import torch
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    rng = np.random.default_rng(23)
    jobs = []
    for _ in range(40):
        W, H = int(rng.integers(1, 900)), int(rng.integers(1, 300))
        jobs.append((W, H, int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))))
    jobs += [(3840, 2160, 640, 360), (1, 1, 1, 1)]
    n = len(jobs)
    descs = (vp8g.Vp8gScaleDesc * n)()
    chunks, planes, outs, so, do, task0 = [], [], [], 5, 0, 0  # (source planes start at an odd offset)
    for i, (W, H, w, h) in enumerate(jobs):
        tight = plane_input("random", W, H, 500 + i)
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
        opt = vp8g.scale_opt(scale=(w, h))
        assert lib.vp8g_make_scale_desc(W, H, offs[0], offs[1], offs[2], sy, suv, C.byref(opt), do, task0,
                                        C.byref(descs[i])) == 0
        outs.append(do)
        do = (do + vp8g.i420_size(w, h) + 255) // 256 * 256
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
        exp, _, _ = vp8g.host_scale(planes[i], W, H, vp8g.scale_opt(scale=(w, h)))
        got = host[outs[i]:outs[i] + len(exp)].tobytes()
        assert got == exp, (i, W, H, w, h, first_diff(got, exp))
        untouched[outs[i]:outs[i] + len(exp)] = False
    assert (host[untouched] == 0xEE).all()
    # inconsistent task numbering is refused before any launch
    descs[1].task0 += 1
    C.set_errno(0)
    assert lib.vp8g_scale_batch_device(descs, C.c_void_p(d_descs.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)) == -1
    assert C.get_errno() == EINVAL


@pytest.mark.parametrize("crop,scale", [((0, 0, 333, 97), (111, 33)), ((3, 5, 101, 77), (50, 0)), ((332, 96, 1, 1), (1, 1)),
                                        ((2, 0, 331, 1), (7, 1))])
def test_crop_windows(vp8g, crop, scale):
    src = plane_input("random", 333, 97, 77)
    opt = vp8g.scale_opt(crop=crop, scale=scale)
    got = vp8g.gpu_scale(src, 333, 97, opt)
    exp = vp8g.host_scale(src, 333, 97, opt)
    assert got[1:] == exp[1:] and got[0] == exp[0], (got[1:], exp[1:], first_diff(got[0], exp[0]))


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
def test_decode_webp_batch_scaled_vs_libwebp(vp8g, golden, oracle_frames, device_m05):
    """vp8g_decode_webp_batch_scaled on the fixture cases of scale.json: filtered = 0 vs WebPDecode with
    bypass_filtering, filtered = 1 + VP8G_SCALE_DWEBP_FILTER vs WebPDecode as it is, filtered = 1
    without the flag vs host_scale of the oracle's filtered decode."""
    cases = [c for c in golden["decode"] if c["bypass"] == 0]
    by_key = {(c["file"], tuple(c["crop"] or ()), tuple(c["scale"]), c["bypass"]): c for c in golden["decode"]}
    files = [(FIXTURES / c["file"]).read_bytes() for c in cases]
    for filtered, flag in ((False, False), (True, True), (True, False)):
        opts = [vp8g.scale_opt(crop=c["crop"], scale=c["scale"], dwebp_filter=flag) for c in cases]
        res, st = vp8g.gpu_decode_webp_batch_scaled(files, opts, filtered=filtered, device_m05=device_m05)
        assert st == [0] * len(cases)
        for c, opt, r in zip(cases, opts, res):
            got, gw, gh = r
            assert [gw, gh] == c["size"], (c["file"], c["scale"])
            if filtered and not flag:
                W, H, _, filt = oracle_frames[c["file"]]
                assert got == vp8g.host_scale(filt, W, H, opt)[0], (c["file"], c["crop"], c["scale"])
            else:
                g = by_key[(c["file"], tuple(c["crop"] or ()), tuple(c["scale"]), 0 if filtered else 1)]
                assert sha(got) == g["sha256"], (c["file"], c["crop"], c["scale"], filtered)


def test_decode_webp_batch_scaled_per_frame_options(vp8g, oracle_frames):
    """Per-frame options over mixed fixtures, one of them invalid for its frame (an upscale): that frame
    gets EINVAL, the others are correct.  One option for all frames (n_opts = 1) works too."""
    rels = ["big/k128_normal.webp", "big/fhd_normal_sharp5.webp", "commons/penguin-q20.webp", "big/k128_normal.webp",
            "big/fhd_simple_sharp3.webp"]
    opts = [vp8g.scale_opt(scale=(64, 0)), vp8g.scale_opt(crop=(100, 50, 999, 501), scale=(0, 100)),
            vp8g.scale_opt(scale=(224, 224)), vp8g.scale_opt(scale=(129, 64)), vp8g.scale_opt(crop=(7, 9, 640, 480))]
    files = [(FIXTURES / r).read_bytes() for r in rels]
    for device_m05 in (False, True):
        res, st = vp8g.gpu_decode_webp_batch_scaled(files, opts, filtered=True, device_m05=device_m05)
        assert st == [0, 0, 0, EINVAL, 0] and res[3] is None
        for i in (0, 1, 2, 4):
            W, H, _, filt = oracle_frames[rels[i]]
            assert res[i] == vp8g.host_scale(filt, W, H, opts[i]), (i, device_m05)
    one = vp8g.scale_opt(scale=(100, 0))
    res, st = vp8g.gpu_decode_webp_batch_scaled(files, one, filtered=False)
    assert st == [0] * 5
    for i, rel in enumerate(rels):
        W, H, unf, _ = oracle_frames[rel]
        assert res[i] == vp8g.host_scale(unf, W, H, one), i
    # n_opts must be 1 or n
    with pytest.raises(RuntimeError, match="errno=22"):
        vp8g.gpu_decode_webp_batch_scaled(files, opts[:2])


def test_scaled_i420_chains_into_the_encoder_on_the_device(vp8g):
    """RGB of a scaled picture = vp8g_encode_batch_device on the scaled I420, chained on one stream with
    no host copy in between: equals oracle_encode(host_scale(...))."""
    import torch
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    jobs = [(641, 479, 224, 224), (333, 97, 111, 33), (1920, 1080, 640, 360)]
    n = len(jobs)
    sdescs = (vp8g.Vp8gScaleDesc * n)()
    planes, soffs, doffs, so, do, task0 = [], [], [], 0, 0, 0
    for i, (W, H, w, h) in enumerate(jobs):
        b = plane_input("random", W, H, 900 + i)
        planes.append(b)
        CW, CH = (W + 1) // 2, (H + 1) // 2
        opt = vp8g.scale_opt(scale=(w, h))
        assert lib.vp8g_make_scale_desc(W, H, so, so + W * H, so + W * H + CW * CH, W, CW, C.byref(opt), do, task0,
                                        C.byref(sdescs[i])) == 0
        cw, ch = (w + 1) // 2, (h + 1) // 2
        doffs.append((do, do + w * h, do + w * h + cw * ch))
        so += len(b)
        do = (do + vp8g.i420_size(w, h) + 255) // 256 * 256
        task0 += sdescs[i].ntasks
    edescs, eouts, etotal, spans = vp8g.make_enc_descs([(w, h) for _, _, w, h in jobs], "rgb", doffs)
    src = torch.from_numpy(np.frombuffer(b"".join(planes), dtype=np.uint8).copy()).to(dev)
    small = torch.empty(do + 16, dtype=torch.uint8, device=dev)
    rgb = torch.empty(etotal + 16, dtype=torch.uint8, device=dev)
    work = torch.empty(lib.vp8g_encode_workspace_size(spans), dtype=torch.uint8, device=dev)
    d_s = vp8g.device_copy(sdescs)
    d_e = vp8g.device_copy(edescs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.vp8g_scale_batch_device(sdescs, C.c_void_p(d_s.data_ptr()), n, C.c_void_p(src.data_ptr()),
                                       C.c_void_p(small.data_ptr()), stream) == 0
    assert lib.vp8g_encode_batch_device(edescs, C.c_void_p(d_e.data_ptr()), n, C.c_void_p(small.data_ptr()),
                                        C.c_void_p(rgb.data_ptr()), C.c_void_p(work.data_ptr()), stream) == 0
    host = rgb.cpu().numpy().tobytes()
    for i, (W, H, w, h) in enumerate(jobs):
        scaled, _, _ = vp8g.host_scale(planes[i], W, H, vp8g.scale_opt(scale=(w, h)))
        ppm = vp8g.oracle_encode(scaled, w, h, "ppm")
        exp = ppm[len(b"P6\n%d %d\n255\n" % (w, h)):]
        assert host[eouts[i]:eouts[i] + len(exp)] == exp, (i, W, H, w, h)


def test_yuv420_rescale_single_image(vp8g, golden, oracle_frames):
    """The single-image entry point on a real decode: penguin-q20 -> 224x224 (unfiltered decode =
    libwebp's own choice at this ratio)."""
    W, H, unf, _ = oracle_frames["commons/penguin-q20.webp"]
    got, w, h = vp8g.gpu_scale(unf, W, H, vp8g.scale_opt(scale=(224, 224)))
    g = next(c for c in golden["decode"] if c["file"] == "commons/penguin-q20.webp" and c["scale"] == [224, 224]
             and c["bypass"] == 0)
    assert (w, h) == (224, 224) and sha(got) == g["sha256"]


def test_cli_crop_and_scale(golden, tmp_path):
    """`decoder -yuvf -scale 640 360` and `-yuv -crop 3 5 101 99 -scale 50 0` write dwebp's bytes;
    -crop / -scale with another mode is a usage error."""
    def gold(rel, crop, scale, bypass):
        return next(c for c in golden["decode"] if c["file"] == rel and c["crop"] == crop and c["scale"] == scale
                    and c["bypass"] == bypass)
    out = tmp_path / "o.i420"
    r = subprocess.run([str(DECODER), "-yuvf", "-scale", "640", "360", str(FIXTURES / "big/fhd_normal_sharp5.webp"), str(out)],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sha(out.read_bytes()) == gold("big/fhd_normal_sharp5.webp", None, [640, 360], 0)["sha256"]
    r = subprocess.run([str(DECODER), "-yuv", "-crop", "3", "5", "101", "99", "-scale", "50", "0",
                        str(FIXTURES / "big/k128_normal.webp"), str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sha(out.read_bytes()) == gold("big/k128_normal.webp", [3, 5, 101, 99], [50, 0], 1)["sha256"]
    for args in (["-ppm", "-scale", "64", "64"], ["-png", "-crop", "0", "0", "8", "8"], ["-yuv", "-scale", "64"],
                 ["-yuv", "-scale", "64", "64", "-scale", "32", "32"]):
        r = subprocess.run([str(DECODER)] + args + [str(FIXTURES / "big/k128_normal.webp"), str(out)], capture_output=True,
                           timeout=60)
        assert r.returncode == 2 and b"Usage" in r.stderr, args
    # an upscale is refused with a message, not a usage error
    r = subprocess.run([str(DECODER), "-yuv", "-scale", "129", "64", str(FIXTURES / "big/k128_normal.webp"), str(out)],
                       capture_output=True, timeout=60)
    assert r.returncode == 1 and b"downscale only" in r.stderr
