"""GPU tests (MI355X) of the alpha path: the un-prediction kernel
(webp-decoder_amd/csrc/vp8g_alpha.hip) behind vp8g_alpha_unfilter_batch_device, and alpha as the fourth
channel of the tensor kernel (vp8g_tensor_batch_device_a).

Bar: bit equality -- with host_alpha_unfilter (the sequential CPU restatement, itself pinned to the rule
written out by hand and to libwebp's planes in tests/test_alpha_host.py) and with host_tensor(alpha=...)."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EINVAL = 22
INT_VIEW = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))

# (w, h): degenerate planes, the 64-row band and 64-column tile on both sides, a band boundary mid-plane,
# more bands than one round of the 16-wave workgroup, a plane wider than one scan chunk, a picture size
PLANE_SIZES = [(1, 1), (1, 130), (130, 1), (2, 2), (63, 63), (64, 64), (65, 65), (129, 5), (5, 129), (257, 66), (7, 1100),
               (3, 2100), (1100, 3), (641, 479)]
KINDS = ("random", "zeros", "ones", "binary")


def residual(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "binary":  # the gradient clips on both sides all the time
        return (rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255))
    return np.full((h, w), 255 if kind == "ones" else 0, np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


@pytest.mark.parametrize("kind", KINDS)
def test_unfilter_mixed_sizes_and_filters_in_one_launch(vp8g, kind):
    """All four filters over every size in ONE launch, padded source strides, the destination prefilled
    with 0xEE and 5 guard bytes around every plane (gpu_alpha_unfilter checks them)."""
    planes, filters = [], []
    for i, (w, h) in enumerate(PLANE_SIZES):
        for f in range(4):
            planes.append(residual(kind, w, h, 100 * i + f))
            filters.append(f)
    got = vp8g.gpu_alpha_unfilter(planes, filters, src_pad=3, guard=5)
    bad = [(p.shape[::-1], f) for p, f, g in zip(planes, filters, got) if not np.array_equal(g, vp8g.host_alpha_unfilter(p, f))]
    assert not bad, bad


def test_unfilter_more_planes_than_workgroups(vp8g):
    """300 small planes: the grid-stride loop takes more than one plane per workgroup."""
    rng = np.random.default_rng(7)
    planes = [residual(KINDS[i % 4], int(rng.integers(1, 90)), int(rng.integers(1, 90)), i) for i in range(300)]
    filters = [i % 4 for i in range(300)]
    filters[1::8] = [3] * len(filters[1::8])
    got = vp8g.gpu_alpha_unfilter(planes, filters, src_pad=1, guard=3)
    bad = [i for i, (p, f, g) in enumerate(zip(planes, filters, got)) if not np.array_equal(g, vp8g.host_alpha_unfilter(p, f))]
    assert not bad, bad


def test_unfilter_fixture_planes_hash_to_libwebps(vp8g):
    """Every decodable fixture with alpha: host entropy decode, device un-prediction, libwebp's A hash."""
    golden = json.loads((GOLDEN / "alpha.json").read_text())
    names, planes, filters = [], [], []
    for name, e in sorted(golden["files"].items()):
        if not e["decodes"] or "stats" not in e:
            continue
        data = (GOLDEN / "alpha" / f"{name}.webp").read_bytes()
        c = vp8g.parse_extended(data)
        res, flt, _ = vp8g.alpha_decode_host(data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]], *e["size"])
        names.append(name), planes.append(res), filters.append(flt)
    assert len(names) >= 40 and set(filters) == {0, 1, 2, 3}
    got = vp8g.gpu_alpha_unfilter(planes, filters)
    bad = [n for n, g in zip(names, got) if hashlib.sha256(g.tobytes()).hexdigest() != golden["files"][n]["a"]]
    assert not bad, bad


def test_unfilter_refuses_bad_descriptors(vp8g):
    lib = vp8g.gpu_lib()
    d = vp8g.Vp8gAlphaDesc()
    for args in ((0, 4, 0, 0, 4, 0, 4), (4, 0, 0, 0, 4, 0, 4), (16384, 4, 0, 0, 16384, 0, 16384), (4, 16384, 0, 0, 4, 0, 4),
                 (4, 4, 4, 0, 4, 0, 4), (4, 4, 1, 0, 3, 0, 4), (4, 4, 1, 0, 4, 0, 3)):
        C.set_errno(0)
        assert lib.vp8g_make_alpha_desc(*args, 0, C.byref(d)) == -1 and C.get_errno() == EINVAL, args
    assert lib.vp8g_make_alpha_desc(4, 4, 3, 0, 4, 0, 4, 0, None) == -1
    assert lib.vp8g_make_alpha_desc(4, 4, 3, 0, 4, 0, 4, 0, C.byref(d)) == 0
    dev = torch.device("cuda", 0)
    buf = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    dd = vp8g.device_copy(d)
    p = C.c_void_p(buf.data_ptr())
    for call in ((None, C.c_void_p(dd.data_ptr()), 1, p, p), (C.byref(d), None, 1, p, p), (C.byref(d), C.c_void_p(dd.data_ptr()), 0, p, p),
                 (C.byref(d), C.c_void_p(dd.data_ptr()), 1, None, p), (C.byref(d), C.c_void_p(dd.data_ptr()), 1, p, None)):
        C.set_errno(0)
        assert lib.vp8g_alpha_unfilter_batch_device(*call, None) == -1 and C.get_errno() == EINVAL
    bad = vp8g.Vp8gAlphaDesc.from_buffer_copy(bytes(d))
    bad.filter = 4
    assert lib.vp8g_alpha_unfilter_batch_device(C.byref(bad), C.c_void_p(dd.data_ptr()), 1, p, p, None) == -1
    torch.cuda.synchronize(dev)
    assert bool((buf == 0xEE).all())


# ---- alpha as the fourth channel of the tensor -------------------------------------------------

# (14, 15: the first widths whose chroma rows, 7 and 8 bytes, sit either side of the chunk path's 8-byte load;
# 24, 25: two whole chunks, and two with a one-pixel partial chunk after them)
T_SIZES = [(w, h) for w in (1, 2, 11, 12, 13, 14, 15, 24, 25, 37, 224) for h in (1, 2, 5)] + [(224, 224)]


def i420_input(w, h, seed):
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def alpha_input(w, h, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    a.reshape(-1)[:5] = np.array([0, 1, 127, 254, 255], np.uint8)[:a.size]
    return a


@pytest.fixture(scope="module")
def t_inputs():
    """Per size three pictures: two with alpha planes (every byte value occurs at 224 x 224), one opaque."""
    return {(w, h): ([i420_input(w, h, 9 * w + h + k) for k in range(3)], [alpha_input(w, h, w + 31 * h), alpha_input(w, h, 5), None])
            for w, h in T_SIZES}


@pytest.mark.parametrize("dtype", ["uint8", "float16", "bfloat16", "float32"])
def test_tensor_alpha_vs_host_tensor(vp8g, t_inputs, dtype):
    bad = []
    for (w, h), (imgs, alphas) in t_inputs.items():
        for layout in ("NHWC", "NCHW"):
            for bgr in (False, True):
                opt = vp8g.tensor_opt((w, h), dtype, layout, bgr=bgr, **({} if dtype == "uint8" else IMAGENET))
                got = vp8g.gpu_tensor(imgs, w, h, opt, alpha=alphas).cpu()
                rgb = vp8g.gpu_tensor(imgs, w, h, opt).cpu()
                for i, b in enumerate(imgs):
                    exp = vp8g.host_tensor(b, w, h, opt, alpha="opaque" if alphas[i] is None else alphas[i])
                    g3 = got[i][:3] if layout == "NCHW" else got[i][..., :3]
                    if not same_bits(got[i], exp) or not same_bits(g3.contiguous(), rgb[i]):
                        bad.append((w, h, layout, bgr, i))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("w,h,dtype,layout", [(3, 3, "uint8", "NHWC"), (37, 5, "uint8", "NCHW"), (13, 2, "float16", "NHWC"),
                                              (25, 4, "bfloat16", "NCHW"), (37, 5, "float32", "NHWC")])
def test_tensor_alpha_offset_base_and_padded_planes(vp8g, w, h, dtype, layout):
    """Three images (the middle one opaque) with padded alpha strides at odd offsets; the output base one
    element off an aligned allocation (3 x 3 uint8: 36-byte slots), prefilled with 0xEE."""
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    opt = vp8g.tensor_opt((w, h), dtype, layout, **IMAGENET)
    eb = vp8g.T_ELEM[opt.dtype]
    slot = lib.vp8g_tensor_slot_size_a(C.byref(opt))
    assert slot == 4 * w * h * eb
    n, cw, ch, fsz = 3, (w + 1) // 2, (h + 1) // 2, vp8g.i420_size(w, h)
    imgs = [i420_input(w, h, 70 + i) for i in range(n)]
    alphas = [alpha_input(w, h, 80), None, alpha_input(w, h, 82)]
    descs, al = (vp8g.Vp8gTensorDesc * n)(), (vp8g.Vp8gTensorAlpha * n)()
    chunks, so, task0 = [np.frombuffer(b"".join(imgs), np.uint8), np.zeros(1, np.uint8)], n * fsz + 1, 0
    for i in range(n):
        o = i * fsz
        assert lib.vp8g_make_tensor_desc(C.byref(opt), o, o + w * h, o + w * h + cw * ch, w, cw, i * slot, task0, C.byref(descs[i])) == 0
        task0 += descs[i].ntasks
        if alphas[i] is None:
            al[i] = vp8g.Vp8gTensorAlpha(vp8g.T_OPAQUE, 0, 0)
            continue
        buf = np.full((h, w + 3), 0x5A, np.uint8)
        buf[:, :w] = alphas[i]
        al[i] = vp8g.Vp8gTensorAlpha(so, w + 3, 0)
        chunks.append(buf.reshape(-1))
        so += buf.size
    src = torch.from_numpy(np.concatenate(chunks)).to(dev)
    d_descs = vp8g.device_copy(descs)
    d_al = vp8g.device_copy(al)
    out = torch.full((eb + n * slot + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(dev)
    assert lib.vp8g_tensor_batch_device_a(descs, C.c_void_p(d_descs.data_ptr()), al, C.c_void_p(d_al.data_ptr()), n, C.byref(opt),
                                          C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr() + eb), C.c_void_p(stream.cuda_stream)) == 0
    host = out.cpu().numpy()
    for i in range(n):
        exp = vp8g.host_tensor(imgs[i], w, h, opt, alpha="opaque" if alphas[i] is None else alphas[i])
        exp = exp.view(INT_VIEW[vp8g._torch_dtype(opt)]).numpy().tobytes()
        assert len(exp) == slot and host[eb + i * slot:eb + (i + 1) * slot].tobytes() == exp, (i, w, h, dtype, layout)
    assert (host[:eb] == 0xEE).all() and (host[eb + n * slot:] == 0xEE).all()


def test_tensor_alpha_refuses_bad_arguments(vp8g):
    dev = torch.device("cuda", 0)
    lib = vp8g.gpu_lib()
    opt = vp8g.tensor_opt((16, 4), "float32", "NCHW")
    d, a = vp8g.Vp8gTensorDesc(), vp8g.Vp8gTensorAlpha(96, 16, 0)
    assert lib.vp8g_make_tensor_desc(C.byref(opt), 0, 64, 80, 16, 8, 0, 0, C.byref(d)) == 0
    src = torch.zeros(160, dtype=torch.uint8, device=dev)
    out = torch.full((2048,), 0xEE, dtype=torch.uint8, device=dev)
    d_d = vp8g.device_copy(d)
    d_a = vp8g.device_copy(a)
    pd, pa, ps, po = (C.c_void_p(t.data_ptr()) for t in (d_d, d_a, src, out))
    short = vp8g.Vp8gTensorAlpha(96, 15, 0)  # a stride below the width
    for call in ((C.byref(d), pd, None, pa, 1, C.byref(opt), ps, po), (C.byref(d), pd, C.byref(a), None, 1, C.byref(opt), ps, po),
                 (C.byref(d), pd, C.byref(short), pa, 1, C.byref(opt), ps, po), (C.byref(d), pd, C.byref(a), pa, 0, C.byref(opt), ps, po),
                 (C.byref(d), pd, C.byref(a), pa, 1, C.byref(opt), ps, C.c_void_p(out.data_ptr() + 2)),
                 (C.byref(d), pd, C.byref(a), pa, 1, None, ps, po)):
        C.set_errno(0)
        assert lib.vp8g_tensor_batch_device_a(*call, None) == -1 and C.get_errno() == EINVAL
    torch.cuda.synchronize(dev)
    assert bool((out == 0xEE).all())


# ---- alpha through crop + rescale --------------------------------------------------------------

def test_alpha_plane_scale_vs_host_luma(vp8g):
    """vp8g_make_scale_desc_plane against host_scale's luma plane on the same bytes: shrink, expand, a crop
    with an odd origin, mixed in one launch beside an identity."""
    rng = np.random.default_rng(3)
    cases = [((67, 45), vp8g.scale_opt(scale=(33, 20))), ((67, 45), vp8g.scale_opt(crop=(3, 5, 61, 38), scale=(38, 22))),
             ((67, 45), vp8g.scale_opt(scale=(101, 91), expand=True)), ((37, 21), vp8g.scale_opt(crop=(5, 3, 20, 11), scale=(31, 7), expand=True)),
             ((640, 480), vp8g.scale_opt(scale=(224, 224))), ((64, 48), vp8g.scale_opt()), ((300, 7), vp8g.scale_opt(scale=(1, 1)))]
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) if i % 2 == 0 else rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255)
              for i, ((w, h), _) in enumerate(cases)]
    got = vp8g.gpu_scale_planes(planes, [o for _, o in cases])
    for i, (p, (_, o)) in enumerate(zip(planes, cases)):
        assert np.array_equal(got[i], vp8g.host_scale_plane(p, o)), i


def test_fixture_alpha_unfiltered_and_scaled_on_the_device_hashes_to_libwebps(vp8g):
    """Host entropy decode, then un-prediction and crop / rescale both on the device: libwebp's scaled A plane
    (WebPDecode MODE_YUVA with the golden's options: one shrink with a crop, one expand)."""
    golden = json.loads((GOLDEN / "alpha.json").read_text())
    names, planes, filters = [], [], []
    for name, e in sorted(golden["files"].items()):
        if e["decodes"] and "stats" in e and e["scaled"]:
            data = (GOLDEN / "alpha" / f"{name}.webp").read_bytes()
            c = vp8g.parse_extended(data)
            res, flt, _ = vp8g.alpha_decode_host(data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]], *e["size"])
            names.append(name), planes.append(res), filters.append(flt)
    alpha = vp8g.gpu_alpha_unfilter(planes, filters)
    for case in ("shrink", "expand"):
        opts = [vp8g.scale_opt(crop=s["crop"], scale=s["scale"], expand=s["expand"]) for s in (golden["files"][n]["scaled"][case] for n in names)]
        got = vp8g.gpu_scale_planes(alpha, opts)
        bad = [n for n, g in zip(names, got) if hashlib.sha256(g.tobytes()).hexdigest() != golden["files"][n]["scaled"][case]["a"]]
        assert not bad, (case, bad)


def test_single_plane_descriptors_leave_three_plane_ones_alone(vp8g):
    """A three-plane descriptor built as before still validates and scales beside the new entry point's
    output for its luma plane."""
    rng = np.random.default_rng(11)
    w, h = 67, 45
    i420 = rng.integers(0, 256, vp8g.i420_size(w, h), dtype=np.uint8).tobytes()
    opt = vp8g.scale_opt(crop=(3, 5, 61, 38), scale=(38, 22))
    full, ow, oh = vp8g.gpu_scale(i420, w, h, opt)
    luma = vp8g.gpu_scale_planes([np.frombuffer(i420, np.uint8, w * h).reshape(h, w)], [opt])[0]
    assert full == vp8g.host_scale(i420, w, h, opt)[0] and luma.tobytes() == full[:ow * oh]


# ---- the extended container in front of the batch pipeline ---------------------------------------

@pytest.fixture(scope="module")
def decodable():
    golden = json.loads((GOLDEN / "alpha.json").read_text())
    skip = set(golden["divergences"])
    return golden, [n for n, e in sorted(golden["files"].items()) if e["decodes"] and n not in skip]


def yuv_hashes(i420, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    cuts = [0, w * h, w * h + cw * ch, w * h + 2 * cw * ch]
    return [hashlib.sha256(i420[cuts[k]:cuts[k + 1]]).hexdigest() for k in range(3)]


@pytest.mark.parametrize("device_m05", [False, True])
def test_batch_x_i420_equals_libwebps_yuv(vp8g, decodable, device_m05, monkeypatch):
    """Every decodable fixture (VP8X with and without ALPH, metadata, the ambiguous containers, a simple file)
    beside every fixture libwebp refuses, in one batch of two-frame chunks: Y, U, V hash to libwebp's, the
    refused files get their errno while their neighbours decode."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    golden, good = decodable
    bad = [n for n, e in sorted(golden["files"].items()) if not e["decodes"] and n.startswith("c_") and n != "c_empty_alph"]
    bad.append("c_vp8l_image")  # (c_empty_alph: the container is fine and alpha is not looked at here)
    names = [n for pair in zip(good, bad * (len(good) // len(bad) + 1)) for n in pair]
    files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in names]
    outs, st = vp8g.gpu_decode_webp_batch_x(files, device_m05=device_m05)
    for n, o, s in zip(names, outs, st):
        e = golden["files"][n]
        if n in good:
            assert s == 0 and [o[1], o[2]] == e["size"] and yuv_hashes(o[0], o[1], o[2]) == [e["y"], e["u"], e["v"]], n
        else:
            assert o is None and s == (95 if n in ("c_anim_flag", "c_anmf", "c_vp8l_image") else EINVAL), (n, s)


def test_batch_x_scaled_equals_libwebps_yuv(vp8g, decodable):
    golden, good = decodable
    good = [n for n in good if golden["files"][n]["scaled"]]
    files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in good]
    for case in ("shrink", "expand"):
        cases = [golden["files"][n]["scaled"][case] for n in good]
        opts = [vp8g.scale_opt(crop=s["crop"], scale=s["scale"], expand=s["expand"], dwebp_filter=True) for s in cases]
        outs, st = vp8g.gpu_decode_webp_batch_x(files, scale=opts)
        for n, o, s, c in zip(good, outs, st, cases):
            assert s == 0 and [o[1], o[2]] == c["size"] and yuv_hashes(o[0], o[1], o[2]) == [c["y"], c["u"], c["v"]], (n, case)


@pytest.mark.parametrize("device_m05", [False, True])
def test_batch_tensor_extended_equals_the_rgb_of_the_simple_file(vp8g, decodable, device_m05):
    """gpu_decode_webp_batch_tensor(extended=True) on VP8X files = the old call on the same VP8 payload
    re-wrapped as a simple file; without extended=True the old call still refuses them; xflags bits are EINVAL."""
    golden, good = decodable
    names = [n for n in good if golden["files"][n]["size"] == [37, 21]][:6] + ["c_no_image"]
    files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in names]
    simple = []
    for b in files[:-1]:
        c = vp8g.parse_extended(b)
        pay = b[c["vp8_chunk_offset"]:c["vp8_chunk_offset"] + c["vp8_chunk_size"]]
        body = b"WEBPVP8 " + len(pay).to_bytes(4, "little") + pay + (b"\0" if len(pay) & 1 else b"")
        simple.append(b"RIFF" + len(body).to_bytes(4, "little") + body)
    opt = vp8g.tensor_opt((37, 21), "uint8", "NHWC")
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True)
    ref, st_ref = vp8g.gpu_decode_webp_batch_tensor(simple, opt, device_m05=device_m05)
    assert st == [0] * 6 + [EINVAL] and st_ref == [0] * 6
    assert torch.equal(got[:6].cpu(), ref.cpu()) and not bool(got[6].any())
    _, st_old = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05)
    assert st_old == [EINVAL if vp8g.parse_extended(b)["extended"] else 0 for b in files[:-1]] + [EINVAL] and EINVAL in st_old[:6]
    lib = vp8g.gpu_lib()
    spans = (vp8g.ByteSpan * 1)()
    for xflags in (2, 3, 4):  # unknown bits
        C.set_errno(0)
        assert lib.vp8g_decode_webp_batch_tensor_x(spans, 1, 1, 0, 0, None, 0, C.byref(opt), xflags, C.c_void_p(got.data_ptr()),
                                                   None) == -1 and C.get_errno() == EINVAL


# ---- end to end: .webp with alpha -> RGBA tensor ---------------------------------------------------

def by_size(golden, names):
    groups = {}
    for n in names:
        groups.setdefault(tuple(golden["files"][n]["size"]), []).append(n)
    return groups


@pytest.mark.parametrize("device_m05", [False, True])
def test_rgba_tensor_end_to_end(vp8g, decodable, device_m05, monkeypatch):
    """Every decodable fixture through gpu_decode_webp_batch_tensor(extended=True, alpha=True) as uint8 NHWC, in
    chunks of two frames, each beside the fixtures whose ALPH does not decode: channel 3 hashes to libwebp's A
    (all 255 for a picture without alpha), channels 0-2 equal the 3-channel path on the same file, the
    undecodable ones get EINVAL and a zero slot."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    golden, good = decodable
    seen = 0
    for (w, h), names in sorted(by_size(golden, good).items()):
        bad = [n for n, e in sorted(golden["files"].items())
               if n.startswith(("bad_", "c_empty_alph")) and vp8g.parse_extended((GOLDEN / "alpha" / f"{n}.webp").read_bytes())["canvas_width"] == w]
        order = [n for k, g in enumerate(names) for n in ([g] + bad[k % max(1, len(bad)):][:1])]
        files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in order]
        opt = vp8g.tensor_opt((w, h), "uint8", "NHWC")
        got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True)
        rgb, st3 = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True)
        got, rgb = got.cpu().numpy(), rgb.cpu().numpy()
        assert got.shape == (len(order), h, w, 4) and st3 == [0] * len(order)
        for i, n in enumerate(order):
            if n in names:
                assert st[i] == 0 and hashlib.sha256(got[i, :, :, 3].tobytes()).hexdigest() == golden["files"][n]["a"], n
                assert np.array_equal(got[i, :, :, :3], rgb[i]), n
                seen += 1
            else:
                assert st[i] == EINVAL and not got[i].any(), n
    assert seen == len(good)


@pytest.mark.parametrize("case", ["shrink", "expand"])
def test_rgba_tensor_end_to_end_scaled(vp8g, decodable, case, monkeypatch):
    """The same with the golden's crop / scale options (opts[i] per frame): channel 3 = libwebp's scaled A."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    golden, good = decodable
    good = [n for n in good if golden["files"][n]["scaled"]]
    groups = {}
    for n in good:
        s = golden["files"][n]["scaled"][case]
        groups.setdefault((tuple(s["size"]), tuple(s["crop"] or ()), tuple(s["scale"])), []).append(n)
    for (size, _, _), names in sorted(groups.items()):
        files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in names]
        cases = [golden["files"][n]["scaled"][case] for n in names]
        opts = [vp8g.scale_opt(crop=s["crop"], scale=s["scale"], expand=s["expand"], dwebp_filter=True) for s in cases]
        opt = vp8g.tensor_opt(size, "uint8", "NHWC")
        for device_m05 in (False, True):
            got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, scale=opts, device_m05=device_m05, extended=True, alpha=True)
            rgb, _ = vp8g.gpu_decode_webp_batch_tensor(files, opt, scale=opts, device_m05=device_m05, extended=True)
            got, rgb = got.cpu().numpy(), rgb.cpu().numpy()
            for i, (n, s) in enumerate(zip(names, cases)):
                assert st[i] == 0 and hashlib.sha256(got[i, :, :, 3].tobytes()).hexdigest() == s["a"], (n, case, device_m05)
                assert np.array_equal(got[i, :, :, :3], rgb[i]), (n, case)


def test_rgba_tensor_float16_nchw_and_a_frame_of_another_size(vp8g, decodable):
    golden, good = decodable
    names = ["raw_f3", "x_meta", "ll_argb_f2", "ll_noise_f0", "c_two_alph"]  # (ll_noise_f0 is 64 x 48: not the tensor's size)
    files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in names]
    opt = vp8g.tensor_opt((37, 21), "float16", "NCHW", **IMAGENET)
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, extended=True, alpha=True)
    assert got.shape == (5, 4, 21, 37) and st == [0, 0, 0, EINVAL, 0]
    rgb, _ = vp8g.gpu_decode_webp_batch_tensor(files, opt, extended=True)
    got, rgb = got.cpu(), rgb.cpu()
    for i, n in enumerate(names):
        if st[i]:
            assert not bool(got[i].view(torch.int16).any())
            continue
        a = vp8g.host_alpha_plane(files[i])
        exp = vp8g.host_alpha_channel(np.full((21, 37), 255, np.uint8) if a is None else a, opt)
        assert same_bits(got[i, 3], exp) and same_bits(got[i, :3].contiguous(), rgb[i]), n
