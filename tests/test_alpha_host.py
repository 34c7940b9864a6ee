"""CPU tests of the extended container and the ALPH chunk: webp_parse_extended,
vp8f_alpha_decode (raw and the RFC 9649 lossless stream) and the un-prediction's CPU restatement, against
libwebp's answers recorded in tests/golden/alpha.json (tests/golden/make_alpha_golden.py) and against the
rule written out here; the 4-channel tensor's host restatement; a sanitizer run of the new parsers."""
import ctypes as C
import errno
import hashlib
import json
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import FIXTURES, GOLDEN, ROOT

ALPHA = GOLDEN / "alpha"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "alpha.json").read_text())


def fixture(name):
    return (ALPHA / f"{name}.webp").read_bytes()


def our_answer(vp8g, data):
    """("decodes", alpha plane or None) or (errno name, None)."""
    try:
        return "decodes", vp8g.host_alpha_plane(data)
    except OSError as e:
        return errno.errorcode[e.errno], None


def test_fixture_files_are_the_goldens_and_small(golden):
    names = sorted(p.stem for p in ALPHA.glob("*.webp"))
    assert names == sorted(golden["files"])
    for n, e in golden["files"].items():
        data = fixture(n)
        assert len(data) == e["bytes"] <= 16384 and hashlib.sha256(data).hexdigest() == e["sha256"], n
        if e["decodes"]:
            assert e["size"][0] <= 320 and e["size"][1] <= 200


def test_verdicts_and_alpha_planes_equal_libwebps(vp8g, golden):
    """Every fixture: the container + ALPH verdict is libwebp's (WebPDecode), and where it decodes the alpha
    plane hashes to libwebp's A plane (all 255 for a picture without alpha).  The deliberate divergences are
    the ones alpha.json names, each with the project's answer."""
    div = golden["divergences"]
    bad = []
    for n, e in sorted(golden["files"].items()):
        verdict, a = our_answer(vp8g, fixture(n))
        if n in div:
            ours = div[n]["ours"]
            if ours.startswith("decodes as "):
                ok = verdict == "decodes" and hashlib.sha256(a.tobytes()).hexdigest() == golden["files"][ours[11:]]["a"]
            else:
                ok = verdict == ours
        elif not e["decodes"]:
            ok = verdict == ("ENOTSUP" if n in ("c_anim_flag", "c_anmf") else "EINVAL")
        else:
            w, h = e["size"]
            plane = a if a is not None else np.full((h, w), 255, np.uint8)
            ok = verdict == "decodes" and plane.shape == (h, w) and hashlib.sha256(plane.tobytes()).hexdigest() == e["a"]
            ok = ok and (a is None) == e["a_opaque"]
        if not ok:
            bad.append((n, verdict))
    assert not bad, bad
    assert sorted(div) == ["c_simple_vp8l", "c_vp8l_image", "raw_f3_rsrv"]
    assert not golden["files"]["raw_f3_rsrv"]["decodes"] and golden["files"]["c_vp8l_image"]["decodes"]


def test_container_choices(vp8g, golden):
    """The cases the RFC leaves open, as libwebp reads them."""
    c = vp8g.parse_extended(fixture("c_alph_after_image"))
    assert c["extended"] and not c["alpha"] and golden["files"]["c_alph_after_image"]["a_opaque"]
    two = fixture("c_two_alph")
    c = vp8g.parse_extended(two)
    assert c["alpha"] and two.index(b"ALPH") + 8 < c["alph_chunk_offset"] == two.rindex(b"ALPH") + 8  # the last one counts
    assert not vp8g.parse_extended(fixture("c_flag_no_chunk"))["alpha"]
    c = vp8g.parse_extended(fixture("c_chunk_no_flag"))
    assert c["alpha"] and not c["vp8x_flags"] & 0x10
    small = fixture("c_riff_small")
    c = vp8g.parse_extended(small)
    assert c["riff_size"] + 8 < len(small) == c["actual_size"] and c["alpha"]
    c = vp8g.parse_extended(fixture("x_meta"))
    assert c["extended"] and not c["alpha"] and c["vp8x_flags"] == 0x2C and (c["canvas_width"], c["canvas_height"]) == (37, 21)
    c = vp8g.parse_extended(fixture("x_meta_alpha"))
    assert c["alpha"] and c["alph_chunk_size"] == 1 + 37 * 21


@pytest.mark.parametrize("name,err", [("c_anim_flag", errno.ENOTSUP), ("c_anmf", errno.ENOTSUP), ("c_vp8l_image", errno.ENOTSUP),
                                      ("c_simple_vp8l", errno.ENOTSUP), ("c_canvas_mismatch", errno.EINVAL),
                                      ("c_chunk_overrun", errno.EINVAL), ("c_no_image", errno.EINVAL), ("c_riff_big", errno.EINVAL),
                                      ("c_riff_cuts_image", errno.EINVAL), ("c_vp8x_size", errno.EINVAL)])
def test_container_errors(vp8g, name, err):
    with pytest.raises(OSError) as e:
        vp8g.parse_extended(fixture(name))
    assert e.value.errno == err


def test_container_rejects_garbage(vp8g):
    good = fixture("raw_f1")
    for data in (b"", b"RIFF", good[:29], b"RIFX" + good[4:], good[:8] + b"WEBQ" + good[12:]):
        with pytest.raises(OSError) as e:
            vp8g.parse_extended(data)
        assert e.value.errno == errno.EINVAL
    lib = vp8g.host_lib()
    buf, span = vp8g._c_bytes(good)
    assert lib.webp_parse_extended(span, None) == -1


def test_simple_files_parse_as_before(vp8g):
    """parse_extended on the existing simple fixtures finds the payload webp_parse_simple_lossy finds."""
    files = sorted(FIXTURES.glob("*/*.webp"))[:40] + [ALPHA / "c_simple.webp"]
    assert len(files) > 10
    for p in files:
        data = p.read_bytes()
        c = vp8g.parse_extended(data)
        assert (c["vp8_chunk_offset"], c["vp8_chunk_size"]) == vp8g.parse_simple(data) and not c["extended"] and not c["alpha"], p


def test_old_entry_points_still_refuse_extended_files(vp8g):
    for name in ("x_meta", "raw_f1", "enc_q100_af1"):
        data = fixture(name)
        with pytest.raises(OSError) as e:
            vp8g.parse_simple(data)
        assert e.value.errno == errno.EINVAL
        kf, f, stage = vp8g.Vp8KeyFrameHeader(), vp8g.Vp8DecodedFrame(), C.c_int()
        buf, _ = vp8g._c_bytes(data)
        C.set_errno(0)
        assert vp8g.host_lib().vp8f_decode_memory(buf, len(data), C.byref(kf), C.byref(f), C.byref(stage)) == -1
        assert stage.value == 2 and C.get_errno() == errno.EINVAL


def test_coverage_condition(vp8g, golden):
    """Every counter of Vp8fAlphaStats is non-zero in a fixture libwebp decodes, or named in "uncovered"."""
    reached = {k for e in golden["files"].values() if e["decodes"] for k, v in e.get("stats", {}).items() if v}
    missing = [k for k in vp8g.ALPHA_STATS if k not in reached and k not in golden["uncovered"]]
    assert not missing, missing
    assert not golden["uncovered"]  # (libwebp 1.2.2's encoders reach every feature on this set)
    filters = {(e["filter"], bool(e["stats"]["lossless"])) for e in golden["files"].values() if e["decodes"] and "stats" in e}
    assert filters == {(f, l) for f in range(4) for l in (False, True)}


def test_stats_are_the_recorded_ones(vp8g, golden):
    for n, e in golden["files"].items():
        if "stats" in e:
            data = fixture(n)
            c = vp8g.parse_extended(data)
            _, flt, st = vp8g.alpha_decode_host(data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]],
                                                c["canvas_width"], c["canvas_height"])
            assert (flt, st) == (e["filter"], e["stats"]), n


def test_alpha_through_the_host_rescaler_equals_libwebps(vp8g, golden):
    """libwebp rescales A with the luma arithmetic, window and target: the host restatement on the decoded
    plane hashes to WebPDecode's scaled A (one shrink with an odd-origin crop, one expand)."""
    n_checked = 0
    for n, e in sorted(golden["files"].items()):
        if not e["decodes"] or "stats" not in e:
            continue
        a = vp8g.host_alpha_plane(fixture(n))
        for case, s in e["scaled"].items():
            got = vp8g.host_scale_plane(a, vp8g.scale_opt(crop=s["crop"], scale=s["scale"], expand=s["expand"]))
            assert list(got.shape[::-1]) == s["size"] and hashlib.sha256(got.tobytes()).hexdigest() == s["a"], (n, case)
            n_checked += 1
    assert n_checked >= 60


# ---- the un-prediction rule, written out ----------------------------------------------------------

def rule(res, f):
    h, w = res.shape
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            if f == 0 or (x == 0 and y == 0):
                pred = 0
            elif y == 0:
                pred = out[y, x - 1]
            elif x == 0:
                pred = out[y - 1, x]
            elif f == 1:
                pred = out[y, x - 1]
            elif f == 2:
                pred = out[y - 1, x]
            else:
                pred = min(255, max(0, out[y, x - 1] + out[y - 1, x] - out[y - 1, x - 1]))
            out[y, x] = (pred + int(res[y, x])) & 255
    return out.astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 5)])
def test_unfilter_restatement_vs_the_rule(vp8g, shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    for res in (rng.integers(0, 256, shape, dtype=np.uint8), np.full(shape, 255, np.uint8),
                rng.integers(0, 2, shape, dtype=np.uint8) * np.uint8(255)):
        for f in range(4):
            assert np.array_equal(vp8g.host_alpha_unfilter(res, f), rule(res, f)), (shape, f)


def test_unfilter_hand_computed(vp8g):
    """Gradient: a clip at 255 and a clip at 0, worked by hand.
         residuals   200  50 |  top row:  200, 250          (left neighbour)
                      40  10 |  (0,1): 200 + 40 = 240        (neighbour above)
                             |  (1,1): clip(240 + 250 - 200 = 290) = 255, + 10 = 265 & 255 = 9
         residuals    10 100 |  top row: 10, 110; (0,1): 10 + 200 = 210
                     200   7 |  (1,1): clip(210 + 110 - 10 = 310) = 255 -> 6     (then the clip at 0:)
         residuals   250   6 |  top row: 250, 0 (256 & 255); (0,1): 250 + 0 = 250 ... left 250, above 0, aboveleft 250
                       0   3 |  (1,1): clip(250 + 0 - 250 = 0) = 0 -> 3;   and   [[100, 156], [0, 5]]:
                             |  top 100, 0; (0,1) 100; (1,1): clip(100 + 0 - 100) = 0 -> 5; [[9, 1], [1, 1]]:
                             |  top 9, 10; (0,1) 10; (1,1): 10 + 10 - 9 = 11 -> 12"""
    cases = [([[200, 50], [40, 10]], [[200, 250], [240, 9]]), ([[10, 100], [200, 7]], [[10, 110], [210, 6]]),
             ([[250, 6], [0, 3]], [[250, 0], [250, 3]]), ([[100, 156], [0, 5]], [[100, 0], [100, 5]]),
             ([[9, 1], [1, 1]], [[9, 10], [10, 12]])]
    for res, exp in cases:
        assert vp8g.host_alpha_unfilter(np.array(res, np.uint8), 3).tolist() == exp
    # a clip below zero: left 0, above 0, aboveleft 200 -> clip(-200) = 0
    res = np.array([[200, 56], [56, 77]], np.uint8)  # top: 200, 0; (0,1): 200 + 56 = 0
    assert vp8g.host_alpha_unfilter(res, 3).tolist() == [[200, 0], [0, 77]]
    assert vp8g.host_alpha_unfilter(res, 1).tolist() == [[200, 0], [0, 77]]
    assert vp8g.host_alpha_unfilter(res, 2).tolist() == [[200, 0], [0, 77]]
    assert vp8g.host_alpha_unfilter(res, 0).tolist() == res.tolist()
    res = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    assert vp8g.host_alpha_unfilter(res, 1).tolist() == [[1, 3, 6], [5, 10, 16]]
    assert vp8g.host_alpha_unfilter(res, 2).tolist() == [[1, 3, 6], [5, 8, 12]]


def test_alpha_decode_errors(vp8g):
    lib = vp8g.host_lib()
    res = np.zeros(64, np.uint8)
    flt = C.c_uint32()
    raw = bytes([0]) + bytes(16)
    buf, _ = vp8g._c_bytes(raw)

    def call(data, size, w, h, out=res.ctypes.data, f=C.byref(flt)):
        C.set_errno(0)
        return lib.vp8f_alpha_decode(data, size, w, h, out, f, None), C.get_errno()

    assert call(buf, len(raw), 4, 4) == (0, 0)
    for args in ((None, 17, 4, 4), (buf, 0, 4, 4), (buf, 17, 0, 4), (buf, 17, 4, 0), (buf, 17, 16384, 1), (buf, 17, 1, 16384),
                 (buf, 16, 4, 4), (buf, 17, 4, 5)):
        assert call(*args) == (-1, errno.EINVAL), args
    assert call(buf, 17, 4, 4, out=None) == (-1, errno.EINVAL) and call(buf, 17, 4, 4, f=None) == (-1, errno.EINVAL)
    for head in (2, 3):  # unknown compression
        b2, _ = vp8g._c_bytes(bytes([head]) + bytes(16))
        assert call(b2, 17, 4, 4) == (-1, errno.EINVAL)
    for head, f in ((0x04, 1), (0x08, 2), (0x0C, 3), (0xFC, 3), (0x30, 0)):  # filter field; the other bits are ignored
        b2, _ = vp8g._c_bytes(bytes([head]) + bytes(16))
        assert call(b2, 17, 4, 4) == (0, 0) and flt.value == f
    out = np.zeros(4, np.uint8)
    assert lib.vp8f_alpha_unfilter(res.ctypes.data, 2, 2, 4, out.ctypes.data) == -1
    assert lib.vp8f_alpha_unfilter(None, 2, 2, 0, out.ctypes.data) == -1 and lib.vp8f_alpha_unfilter(res.ctypes.data, 0, 2, 0, out.ctypes.data) == -1


def test_truncated_and_corrupted_streams_fail_cleanly(vp8g, golden):
    for n, e in golden["files"].items():
        if n.startswith("bad_"):
            assert not e["decodes"]
            with pytest.raises(OSError) as err:
                vp8g.host_alpha_plane(fixture(n))
            assert err.value.errno == errno.EINVAL, n
    data = fixture("ll_mixed_f3")
    c = vp8g.parse_extended(data)
    alph = data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]]
    for cut in (1, 2, 3, 5, 9, 40, len(alph) // 3, len(alph) - 1):
        with pytest.raises(OSError):
            vp8g.alpha_decode_host(alph[:cut], c["canvas_width"], c["canvas_height"])


# ---- the fourth channel on the host -------------------------------------------------------------

def test_slot_sizes_and_options(vp8g):
    lib = vp8g.gpu_lib()
    for dtype, eb in (("uint8", 1), ("float16", 2), ("bfloat16", 2), ("float32", 4)):
        opt = vp8g.tensor_opt((37, 5), dtype, "NHWC")
        assert lib.vp8g_tensor_slot_size_a(C.byref(opt)) == 4 * 37 * 5 * eb
        assert lib.vp8g_tensor_slot_size(C.byref(opt)) == 3 * 37 * 5 * eb
    assert lib.vp8g_tensor_slot_size_a(C.byref(vp8g.tensor_opt((3, 3), "uint8", "NHWC"))) == 36
    for bad in (vp8g.tensor_opt((0, 5), "uint8"), vp8g.tensor_opt((5, 16384), "uint8")):
        C.set_errno(0)
        assert lib.vp8g_tensor_slot_size_a(C.byref(bad)) == 0 and C.get_errno() == errno.EINVAL
    bad = vp8g.tensor_opt((4, 4), "uint8")
    bad.flags = 2
    assert lib.vp8g_tensor_slot_size_a(C.byref(bad)) == 0 and lib.vp8g_tensor_slot_size_a(None) == 0


def test_host_tensor_alpha_values(vp8g):
    a = np.array([[0, 1, 127, 254, 255]], np.uint8)
    i420 = bytes(5 + 2 * 3)
    exp32 = [0.0, 1.0 / 255.0, 127.0 / 255.0, 254.0 / 255.0, 1.0]
    for layout in ("NHWC", "NCHW"):
        t = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "uint8", layout), alpha=a)
        ch = t[3, 0] if layout == "NCHW" else t[0, :, 3]
        assert t.dtype == torch.uint8 and ch.tolist() == [0, 1, 127, 254, 255]
        t = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "float32", layout, scale=3.0, bias=1.0), alpha=a)
        ch = t[3, 0] if layout == "NCHW" else t[0, :, 3]
        assert ch.tolist() == [float(np.float32(v)) for v in exp32] and ch[4].item() == 1.0  # (scale and bias never touch A)
        t = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "float16", layout), alpha=a)
        ch = t[3, 0] if layout == "NCHW" else t[0, :, 3]
        assert ch.view(torch.int16).tolist() == np.array(exp32, np.float32).astype(np.float16).view(np.int16).tolist()
        assert ch.view(torch.int16).tolist() == [0x0000, 0x1C04, 0x37F8, 0x3BF8, 0x3C00]
        t = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "bfloat16", layout), alpha=a)
        ch = t[3, 0] if layout == "NCHW" else t[0, :, 3]
        assert (ch.view(torch.int16).to(torch.int32) & 0xFFFF).tolist() == [0x0000, 0x3B81, 0x3EFF, 0x3F7F, 0x3F80]
        rgb = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "bfloat16", layout))
        assert torch.equal((t[:3] if layout == "NCHW" else t[..., :3]).contiguous().view(torch.int16), rgb.view(torch.int16))
    t = vp8g.host_tensor(i420, 5, 1, vp8g.tensor_opt((5, 1), "float32", "NCHW"), alpha="opaque")
    assert t.shape == (4, 1, 5) and t[3].tolist() == [[1.0] * 5]


# ---- robustness: the new parsers under the sanitizers, as a program of their own ------------------

def test_parsers_under_sanitizers(tmp_path, golden):
    """tools/alpha_san_main.c + the host sources, built with -fsanitize=address,undefined and run as a child
    process: every fixture whole, truncated at every length and with 2000 seeded single-byte corruptions
    through webp_parse_extended, its ALPH payload the same way through vp8f_alpha_decode.  Exit 0, no report."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    host = ROOT / "webp-decoder_amd" / "host"
    exe = tmp_path / "alpha_san"
    srcs = [str(ROOT / "tools" / "alpha_san_main.c")] + [str(host / f) for f in ("webp_riff.c", "vp8_parse.c", "vp8_synth.c", "vp8_scale.c",
                                                                               "vp8_alpha.c")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.c"
    trivial.write_text("int main(void) { return 0; }\n")
    r = subprocess.run([cc] + san + ["-o", str(tmp_path / "trivial"), str(trivial)], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "trivial")]).returncode != 0:
        pytest.skip("the sanitizer runtime does not link or start here: " + r.stderr[-300:])
    r = subprocess.run([cc, "-std=c11", "-O2", "-g"] + san + ["-D_POSIX_C_SOURCE=200809L", "-o", str(exe)] + srcs + ["-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # (the runtime links: a failure here is a failure of the sources)
    files = [str(ALPHA / f"{n}.webp") for n in sorted(golden["files"], key=lambda n: -golden["files"][n]["bytes"])]
    groups = [files[k::8] for k in range(8)]  # (eight children side by side: the long streams dominate)
    procs = [subprocess.Popen([str(exe)] + g, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for g in groups]
    lines = 0
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0 and "ERROR" not in err and "runtime error" not in err, err[-2000:]
        lines += len(out.splitlines())
    assert lines == len(files)
