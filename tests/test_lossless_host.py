"""The host half of the lossless (VP8L) path: webp_parse_any, vp8f_lossless_header /
_decode / _apply against libwebp's answers for tests/golden/lossless/ (tests/golden/lossless.json), the old
parsers' unchanged verdicts, the restatement of the ARGB tensor, and a sanitizer run of the new code as a
program of its own."""
import ctypes as C
import errno
import hashlib
import json
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

LOSSLESS = GOLDEN / "lossless"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "lossless.json").read_text())


def fixture(name):
    return (LOSSLESS / f"{name}.webp").read_bytes()


def our_answer(vp8g, data):
    """("decodes", uint32 [h, w]) or (errno name, None)."""
    try:
        return "decodes", vp8g.host_lossless_argb(data)
    except OSError as e:
        return errno.errorcode[e.errno], None


def test_fixture_files_are_the_goldens_and_small(golden):
    names = sorted(p.stem for p in LOSSLESS.glob("*.webp"))
    assert names == sorted(golden["files"])
    for n, e in golden["files"].items():
        data = fixture(n)
        assert len(data) == e["bytes"] <= 32768 and hashlib.sha256(data).hexdigest() == e["sha256"], n
    sizes = {tuple(e["size"]) for e in golden["files"].values() if e["decodes"]}
    assert {(1, 1), (37, 21), (67, 45), (160, 100), (192, 128), (257, 70)} <= sizes


def test_decodable_fixtures_equal_libwebps_rgba(vp8g, golden):
    n = 0
    for name, e in golden["files"].items():
        if not e["decodes"]:
            continue
        verdict, argb = our_answer(vp8g, fixture(name))
        assert verdict == "decodes", name
        assert list(argb.shape[::-1]) == e["size"], name
        assert hashlib.sha256(vp8g.argb_to_rgba(argb).tobytes()).hexdigest() == e["rgba"], name
        n += 1
    assert n >= 24 + 4  # (the 24 encoded pictures and their decodable wrappings)


def test_refused_files_give_their_errno(vp8g, golden):
    seen = set()
    for name, e in golden["files"].items():
        if e["decodes"]:
            continue
        verdict, _ = our_answer(vp8g, fixture(name))
        want = "ENOTSUP" if name in ("x_anim_flag", "x_anmf") else "EINVAL"
        assert verdict == want, name
        seen.add(name)
    for kind in ("bad_trunc_", "bad_trunc8_", "bad_corrupt", "bad_signature", "bad_version", "x_canvas_mismatch", "x_anim_flag", "x_anmf",
                 "c_chunk_overrun", "c_riff_big"):
        assert any(n.startswith(kind) for n in seen), kind


def test_old_parsers_still_refuse_lossless_files(vp8g, golden):
    for name, e in golden["files"].items():
        data = fixture(name)
        try:
            c = vp8g.parse_any(data)
        except OSError:
            continue
        assert c["lossless"] and not c["vp8_chunk_offset"] and not c["alpha"], name
        with pytest.raises(OSError) as ei:
            vp8g.parse_extended(data)
        assert ei.value.errno == errno.ENOTSUP, name
        with pytest.raises(OSError) as ei:
            vp8g.parse_simple(data)
        # (the simple parser knows one layout: anything else is EINVAL, as before)
        assert ei.value.errno == errno.EINVAL, name


def test_parse_any_reads_lossy_files_as_parse_extended(vp8g):
    alpha = json.loads((GOLDEN / "alpha.json").read_text())
    n = 0
    for name in alpha["files"]:
        data = (GOLDEN / "alpha" / f"{name}.webp").read_bytes()
        try:
            x = vp8g.parse_extended(data)
        except OSError as e:
            if name in ("c_simple_vp8l", "c_vp8l_image"):
                assert e.errno == errno.ENOTSUP and vp8g.parse_any(data)["lossless"], name
                continue
            with pytest.raises(OSError) as ei:
                vp8g.parse_any(data)
            assert ei.value.errno == e.errno, name
            continue
        a = vp8g.parse_any(data)
        assert not a["lossless"] and all(a[k] == v for k, v in x.items()), name
        n += 1
    assert n >= 40


def test_container_fields(vp8g):
    data = fixture("x_meta")
    c = vp8g.parse_any(data)
    o, n = c["vp8l_chunk_offset"], c["vp8l_chunk_size"]
    assert data[o - 8:o - 4] == b"VP8L" and struct.unpack("<I", data[o - 4:o])[0] == n and data[o] == 0x2F
    assert c["extended"] == 1 and (c["canvas_width"], c["canvas_height"]) == (67, 45) and c["vp8x_flags"] == 0x2C
    c = vp8g.parse_any(fixture("pic_67x45_m4q75"))
    assert c["extended"] == 0 and c["vp8l_chunk_offset"] == 20 and (c["canvas_width"], c["canvas_height"]) == (67, 45)
    # an ALPH chunk beside a VP8L image is ignored
    c = vp8g.parse_any(fixture("x_alph_ignored"))
    assert c["lossless"] and not c["alpha"]
    assert np.array_equal(vp8g.host_lossless_argb(fixture("x_alph_ignored")), vp8g.host_lossless_argb(fixture("pic_67x45_m4q75")))


def test_header(vp8g):
    lib = vp8g.host_lib()

    def hdr(b):
        w, h, a = C.c_uint32(), C.c_uint32(), C.c_uint32()
        buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
        rc = lib.vp8f_lossless_header(buf, len(b), C.byref(w), C.byref(h), C.byref(a))
        return (w.value, h.value, a.value) if rc == 0 else C.get_errno()

    bits = (37 - 1) | (21 - 1) << 14 | 1 << 28
    assert hdr(b"\x2f" + struct.pack("<I", bits)) == (37, 21, 1)
    assert hdr(b"\x2f" + struct.pack("<I", bits & ~(1 << 28))) == (37, 21, 0)
    assert hdr(b"\x2f" + struct.pack("<I", 0x3FFF | 0x3FFF << 14)) == (16384, 16384, 0)
    assert hdr(b"\x2e" + struct.pack("<I", bits)) == errno.EINVAL
    for version in range(1, 8):
        assert hdr(b"\x2f" + struct.pack("<I", bits | version << 29)) == errno.EINVAL
    assert hdr(b"\x2f" + struct.pack("<I", bits)[:3]) == errno.EINVAL


def test_stats_and_transforms_are_the_recorded_ones(vp8g, golden):
    names = ("predictor", "cross_color", "subtract_green", "color_index")
    for name, e in golden["files"].items():
        if not e["decodes"]:
            continue
        data = fixture(name)
        c = vp8g.parse_any(data)
        im = vp8g.lossless_decode_host(data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]])
        assert im["stats"] == e["ours"]["stats"], name
        assert [(names[t["type"]], t["bits"]) for t in im["transforms"]] == [(t["type"], t["bits"]) for t in e["ours"]["transforms"]]
        # the residual has the packed width when colour indexing is present
        xs = e["size"][0]
        for t in im["transforms"]:
            assert t["xsize"] == xs, name
            if t["type"] == vp8g.L_COLOR_INDEX:
                xs = (xs + (1 << t["bits"]) - 1) >> t["bits"]
        assert im["residual"].shape == (e["size"][1], xs), name


def test_coverage_condition(golden):
    """What the fixtures reach, and what is left to the synthetic images of tests/test_gpu_lossless.py."""
    good = [e["ours"] for e in golden["files"].values() if e["decodes"]]
    orders = {tuple(t["type"] for t in o["transforms"]) for o in good}
    assert {("predictor", "cross_color"), ("subtract_green", "predictor"), ("color_index",), ("color_index", "predictor"), ()} <= orders
    packs = {t["bits"] for o in good for t in o["transforms"] if t["type"] == "color_index"}
    assert packs == {0, 1, 2, 3}
    modes = {m for o in good for m in o["modes"]}
    assert set(range(16)) - modes == set(golden["uncovered"]["predictor_modes"])
    assert set(range(1, 13)) <= modes


def test_apply_hand_computed(vp8g):
    """Every predictor mode on a 3 x 2 image whose only predicted pixel with four neighbours is (1, 1), and the
    rightmost column's TR."""
    res = np.array([[0x01020304, 0x10203040, 0x05060708], [0x0A0B0C0D, 0x00000000, 0x00000000]], np.uint32)

    def add(a, b):
        return sum((((int(a) >> s) + (int(b) >> s)) & 255) << s for s in (0, 8, 16, 24))

    def avg(a, b):
        return sum(((((a >> s) & 255) + ((b >> s) & 255)) >> 1) << s for s in (0, 8, 16, 24))

    def chans(p):
        return [(p >> s) & 255 for s in (0, 8, 16, 24)]

    def join(c):
        return sum(int(v) << s for v, s in zip(c, (0, 8, 16, 24)))

    p00 = add(res[0, 0], 0xFF000000)
    p01 = add(res[0, 1], p00)
    p02 = add(res[0, 2], p01)
    p10 = add(res[1, 0], p00)
    L, T, TL, TR = int(p10), int(p01), int(p00), int(p02)
    cl, ct, ctl = chans(L), chans(T), chans(TL)
    clamp = lambda v: max(0, min(255, v))  # noqa: E731
    a_lt = avg(L, T)
    half = join([clamp(a + int((a - b) / 2)) for a, b in zip(chans(a_lt), ctl)])
    sel = L if sum(abs(a - b) for a, b in zip(ct, ctl)) < sum(abs(a - b) for a, b in zip(cl, ctl)) else T
    want = [0xFF000000, L, T, TR, TL, avg(avg(L, TR), T), avg(L, TL), avg(L, T), avg(TL, T), avg(T, TR),
            avg(avg(L, TL), avg(T, TR)), sel, join([clamp(a + b - c) for a, b, c in zip(cl, ct, ctl)]), half,
            0xFF000000, 0xFF000000]
    for mode in range(16):
        img = vp8g.lossless_image(res, [{"type": vp8g.L_PREDICTOR, "bits": 2, "data": np.array([[mode << 8]], np.uint32)}])
        out = vp8g.host_lossless_apply(img)
        assert [int(out[0, 0]), int(out[0, 1]), int(out[0, 2]), int(out[1, 0])] == [p00, p01, p02, p10], mode
        assert int(out[1, 1]) == want[mode], mode
        # (1, 2) is the rightmost column: its TR is the row's own first pixel
        L2, T2, TL2, TR2 = int(out[1, 1]), p02, p01, p10
        if mode == 3:
            assert int(out[1, 2]) == TR2
        if mode == 9:
            assert int(out[1, 2]) == avg(T2, TR2)
        if mode == 5:
            assert int(out[1, 2]) == avg(avg(L2, TR2), T2)


def test_apply_pointwise_hand_computed(vp8g):
    px = np.array([[0x80FF10F0, 0x01020304]], np.uint32)
    out = vp8g.host_lossless_apply(vp8g.lossless_image(px, [{"type": vp8g.L_SUBTRACT_GREEN, "bits": 0}]))
    assert [int(v) for v in out[0]] == [0x800F1000, 0x01050307]
    # cross colour with negative multipliers: g2r = -32 (0xE0), g2b = 64, r2b = -128
    e = 0xFF000000 | 0x80 << 16 | 0x40 << 8 | 0xE0
    out = vp8g.host_lossless_apply(vp8g.lossless_image(np.array([[0x00107F05]], np.uint32),
                                                       [{"type": vp8g.L_CROSS_COLOR, "bits": 2, "data": np.array([[e]], np.uint32)}]))
    g = 0x7F
    r = (0x10 + ((-32 * g) >> 5)) & 255
    rs = r - 256 if r > 127 else r
    b = (0x05 + ((64 * g) >> 5)) & 255
    b = (b + ((-128 * rs) >> 5)) & 255
    assert int(out[0, 0]) == (r << 16 | g << 8 | b)
    # colour indexing at 2 bits per pixel: four pixels per packed green byte, an index beyond the table reads 0
    table = np.array([0xFF000001, 0xFF000002, 0xFF000003], np.uint32)
    packed = np.array([[0b11100100 << 8, 0b01 << 8]], np.uint32)
    img = vp8g.lossless_image(packed, [{"type": vp8g.L_COLOR_INDEX, "bits": 2, "data": table}], width=5)
    assert [int(v) for v in vp8g.host_lossless_apply(img)[0]] == [0xFF000001, 0xFF000002, 0xFF000003, 0, 0xFF000002]


def test_decode_errors(vp8g):
    good = fixture("pic_37x21_m0q10")
    c = vp8g.parse_any(good)
    p = good[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]
    vp8g.lossless_decode_host(p)
    for bad in (b"", p[:4], p[:5], p[:len(p) - 20], b"\x2e" + p[1:]):
        C.set_errno(0)  # (the call itself must set it: nothing left over from the call before)
        with pytest.raises(OSError) as ei:
            vp8g.lossless_decode_host(bad)
        assert ei.value.errno == errno.EINVAL
    # every truncation of the stream fails with EINVAL set by that call, also where the stream ends between two fields
    # (and after webp_parse_any, which leaves the ENOTSUP of the parser it tries first behind its success)
    lib = vp8g.host_lib()
    buf = (C.c_uint8 * len(p)).from_buffer_copy(p)
    for k in range(len(p)):
        im = vp8g.Vp8fLosslessImage()
        C.set_errno(0)
        assert lib.vp8f_lossless_decode(buf, k, C.byref(im), None) == -1 and C.get_errno() == errno.EINVAL, k
        C.set_errno(errno.ENOTSUP)
        assert lib.vp8f_lossless_decode(buf, k, C.byref(im), None) == -1 and C.get_errno() == errno.EINVAL, k
    assert lib.vp8f_lossless_decode(None, 0, None, None) == -1 and C.get_errno() == errno.EINVAL
    assert lib.vp8f_lossless_apply(None, None) == -1 and C.get_errno() == errno.EINVAL
    lib.vp8f_lossless_free(None)


def test_host_tensor_argb_values(vp8g):
    argb = np.array([[0x80FF0001, 0xFF102030], [0x00000000, 0x01FEFDFC]], np.uint32)
    u8 = vp8g.host_tensor_argb(argb, vp8g.tensor_opt((2, 2), "uint8", "NHWC"), 4)
    assert u8.numpy().tolist() == [[[255, 0, 1, 128], [16, 32, 48, 255]], [[0, 0, 0, 0], [254, 253, 252, 1]]]
    assert np.array_equal(u8.numpy(), vp8g.argb_to_rgba(argb))
    bgr = vp8g.host_tensor_argb(argb, vp8g.tensor_opt((2, 2), "uint8", "NCHW", bgr=True), 3)
    assert bgr.shape == (3, 2, 2) and bgr[0].numpy().tolist() == [[1, 48], [0, 252]]
    f = vp8g.host_tensor_argb(argb, vp8g.tensor_opt((2, 2), "float32", "NHWC", scale=[2.0, 0.5, 1.0], bias=[1.0, 0.0, -1.0]), 4)
    assert f.dtype == torch.float32 and f[0, 0].tolist() == [511.0, 0.0, 0.0, float(np.float32(128) / np.float32(255))]
    assert f[0, 1, 3].item() == 1.0


# ---- robustness: the new code under the sanitizers, as a program of its own -------------------------

def test_lossless_under_sanitizers(tmp_path, golden):
    """tools/lossless_san_main.c + host/vp8_alpha.c + host/webp_riff.c (and the sources they call), built with
    -fsanitize=address,undefined and run as a child process: every fixture, the bad files included, whole,
    truncated and with seeded single-byte corruptions through webp_parse_any, its VP8L payload the same way
    through vp8f_lossless_decode and vp8f_lossless_apply.  Exit 0, no report."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    host = ROOT / "webp-decoder_amd" / "host"
    exe = tmp_path / "lossless_san"
    srcs = [str(ROOT / "tools" / "lossless_san_main.c")] + [str(host / f) for f in ("webp_riff.c", "vp8_parse.c", "vp8_synth.c",
                                                                                  "vp8_scale.c", "vp8_alpha.c")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cc, "-std=c11", "-O2", "-g"] + san + ["-D_POSIX_C_SOURCE=200809L", "-o", str(exe)] + srcs + ["-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = [str(LOSSLESS / f"{n}.webp") for n in sorted(golden["files"], key=lambda n: -golden["files"][n]["bytes"])]
    groups = [files[k::8] for k in range(8)]  # (eight children side by side: the long streams dominate)
    procs = [subprocess.Popen([str(exe)] + g, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for g in groups]
    lines = 0
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0 and "ERROR" not in err and "runtime error" not in err, err[-2000:]
        lines += len(out.splitlines())
    assert lines == len(files)
