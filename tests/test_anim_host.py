"""The host half of the animation path: webp_parse_anim on every fixture of tests/golden/anim/ -- its
verdict against libwebp's WebPAnimDecoderNew and its fields against what the file was assembled from
(tests/golden/anim.json) --, vp8f_anim_compose against libwebp's canvases, the old parsers' unchanged verdicts, and a
sanitizer run of the new code as a program of its own."""
import ctypes as C
import errno
import hashlib
import json
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

ANIM = GOLDEN / "anim"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "anim.json").read_text())


def fixture(name):
    return (ANIM / f"{name}.webp").read_bytes()


def test_fixture_files_are_the_goldens_and_small(golden):
    names = sorted(p.stem for p in ANIM.glob("*.webp"))
    assert names == sorted(golden["files"])
    for n, e in golden["files"].items():
        data = fixture(n)
        assert len(data) == e["bytes"] <= 10240 and hashlib.sha256(data).hexdigest() == e["sha256"], n
        if e["accepts"]:
            assert e["canvas"][0] <= 64 and e["canvas"][1] <= 48 and e["nframes"] <= 14, n
    assert golden["libwebp"]["demux"] == "10200"


def test_verdicts_agree_with_libwebp(vp8g, golden):
    kinds = set()
    for name, e in golden["files"].items():
        try:
            a = vp8g.parse_anim(fixture(name))
        except OSError as err:
            assert err.errno == errno.EINVAL, name
            a = None
        if "divergence" in e:  # a still picture: libwebp shows it as one frame, this parser is for animations
            assert a is None and e["accepts"] and e["divergence"][0] == "EINVAL", name
            continue
        assert (a is not None) == e["accepts"], name
        if a is None:
            kinds.add(name)
            continue
        assert a["canvas"] == e["canvas"] and a["loop_count"] == e["loop_count"] and a["bgcolor"] == e["bgcolor"], name
        assert len(a["frames"]) == e["nframes"], name
    for must in ("bad_truncated", "bad_anmf_before_anim", "bad_outside_canvas", "bad_outside_canvas_y", "bad_no_image_last",
                 "bad_alph_only", "bad_no_frames", "bad_flag_only", "bad_no_anim_flag", "bad_riff_big", "bad_top_level_image",
                 "bad_unknown_before_image", "bad_alph_before_vp8l", "bad_short_anmf", "bad_short_anim", "bad_reserved_flag"):
        assert must in kinds, must


def test_frame_fields_are_the_assembled_ones(vp8g, golden):
    n = 0
    for name, e in golden["files"].items():
        if "built" not in e:
            continue
        data = fixture(name)
        a = vp8g.parse_anim(data)
        b = e["built"]
        assert a["canvas"] == b["canvas"] and a["loop_count"] == b["loop_count"] and len(a["frames"]) == len(b["frames"]), name
        for f, want in zip(a["frames"], b["frames"]):
            assert {k: f[k] for k in want if k != "kind"} == {k: v for k, v in want.items() if k != "kind"}, name
            kind = "lossless" if f["vp8l_size"] else "lossy_alpha" if f["alph_size"] else "lossy"
            assert kind == want["kind"], name
            # the spans name the chunks they say they name
            assert data[f["offset"] - 8:f["offset"] - 4] == b"ANMF" and int.from_bytes(data[f["offset"] - 4:f["offset"]], "little") == f["size"]
            for tag, key in ((b"ALPH", "alph"), (b"VP8 ", "vp8"), (b"VP8L", "vp8l")):
                o, s = f[key + "_offset"], f[key + "_size"]
                assert (o == 0 and s == 0) or (data[o - 8:o - 4] == tag and int.from_bytes(data[o - 4:o], "little") == s), (name, key)
                assert o == 0 or f["offset"] + 16 <= o - 8 and o + s <= f["offset"] + f["size"], (name, key)
        n += 1
    assert n >= 16
    mixed = [f["kind"] for f in golden["files"]["mixed"]["built"]["frames"]]
    assert {"lossy", "lossless", "lossy_alpha"} <= set(mixed)
    # the lossless frame whose header clears the alpha bit: has_alpha follows the header, as libwebp's does
    assert [f["has_alpha"] for f in vp8g.parse_anim(fixture("alpha_bit_cleared"))["frames"]] == [1, 0, 1]


def test_count_only_and_short_room(vp8g):
    lib = vp8g.host_lib()
    data = fixture("rules_a")
    buf, span = vp8g._c_bytes(data)
    info = vp8g.WebPAnimInfo()
    assert lib.webp_parse_anim(span, C.byref(info), None, 0) == 0 and info.nframes == 14 and info.loop_count == 3
    fr = (vp8g.WebPAnimFrame * 4)()
    assert lib.webp_parse_anim(span, C.byref(info), fr, 3) == 0 and info.nframes == 14
    assert fr[2].width and not fr[3].width  # three records written, no more
    assert lib.webp_parse_anim(span, None, None, 0) == -1 and C.get_errno() == errno.EINVAL
    assert lib.webp_parse_anim(span, C.byref(info), None, 2) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    bad, bspan = vp8g._c_bytes(fixture("bad_no_frames"))
    assert lib.webp_parse_anim(bspan, C.byref(info), None, 0) == -1 and C.get_errno() == errno.EINVAL and info.canvas_width == 0


def test_compose_equals_libwebps_canvases(vp8g, golden):
    n = frames = 0
    for name, e in golden["files"].items():
        if not e["accepts"] or not e.get("decodes") or "divergence" in e:
            continue
        (cw, ch), fr, ts = vp8g.host_anim_frames(fixture(name))
        out, _ = vp8g.host_anim_compose(cw, ch, fr)
        assert [cw, ch] == e["canvas"] and len(fr) == e["nframes"], name
        for k, want in enumerate(e["frames"]):
            assert hashlib.sha256(vp8g.argb_to_rgba(out[k]).tobytes()).hexdigest() == want["rgba"], (name, k)
            assert ts[k] == want["timestamp"], (name, k)
        n, frames = n + 1, frames + len(fr)
    assert n >= 15 and frames >= 60


def test_key_frames_of_the_rule_fixtures(vp8g):
    """rules_b: a full-canvas blending frame after a partial KEY frame that disposed is a key frame and comes out equal to
    its source; the same after a partial NON-key frame that disposed is blended everywhere but in that rectangle."""
    (cw, ch), fr, _ = vp8g.host_anim_frames(fixture("rules_b"))
    out, keys = vp8g.host_anim_compose(cw, ch, fr)
    assert keys == [1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(out[1], fr[1]["argb"])
    differs = out[3] != fr[3]["argb"]
    x, y, (h, w) = fr[2]["x"], fr[2]["y"], fr[2]["argb"].shape
    assert not differs[y:y + h, x:x + w].any() and differs.sum() > 50
    # the alpha bit of a lossless header alone decides has_alpha: the full-canvas frame is a key frame although its pixels are not opaque
    (cw, ch), fr, _ = vp8g.host_anim_frames(fixture("alpha_bit_cleared"))
    out, keys = vp8g.host_anim_compose(cw, ch, fr)
    assert keys == [1, 1, 0] and np.array_equal(out[1], fr[1]["argb"]) and (fr[1]["argb"] >> 24 != 255).any()


def test_blend_by_hand(vp8g):
    """The three cases that cannot be simplified: an opaque source is kept (the formula would give c - 1), a transparent
    source keeps the canvas pixel whole, and a translucent source over a transparent canvas is not the identity."""
    def over(s, d):
        below = {"argb": np.array([[d]], np.uint32), "x": 0, "y": 0, "blend": 0, "dispose": 0, "has_alpha": 1}
        above = {"argb": np.array([[s]], np.uint32), "x": 0, "y": 0, "blend": 1, "dispose": 0, "has_alpha": 1}
        return int(vp8g.host_anim_compose(1, 1, [below, above])[0][1, 0, 0])

    def formula(s, d):
        sa, da = s >> 24, d >> 24
        dfa = (da * (256 - sa)) >> 8
        ba = sa + dfa
        scale = (1 << 24) // ba
        out = ba << 24
        for sh in (0, 8, 16):
            out |= ((((s >> sh) & 255) * sa + ((d >> sh) & 255) * dfa) * scale >> 24) << sh
        return out

    assert over(0xFF804020, 0x80112233) == 0xFF804020 != formula(0xFF804020, 0x80112233)
    assert over(0x00804020, 0x80112233) == 0x80112233
    assert over(0x03804020, 0x00000000) == 0x037F3F1F
    for s, d in ((0x80FF0001, 0xFF00FF80), (0x01FFFFFF, 0xFE000000), (0xFE102030, 0x01FFFFFF), (0x80808080, 0x80808080)):
        assert over(s, d) == formula(s, d)
    # after a disposal the cleared pixels take the source as it is; elsewhere the frame blends
    f0 = {"argb": np.full((2, 4), 0xFF102030, np.uint32), "x": 0, "y": 0, "blend": 0, "dispose": 0, "has_alpha": 0}
    f1 = {"argb": np.full((2, 2), 0x80000000, np.uint32), "x": 2, "y": 0, "blend": 1, "dispose": 1, "has_alpha": 1}
    f2 = {"argb": np.full((2, 4), 0x03808080, np.uint32), "x": 0, "y": 0, "blend": 1, "dispose": 0, "has_alpha": 1}
    out, keys = vp8g.host_anim_compose(4, 2, [f0, f1, f2])
    assert keys == [1, 0, 0]
    assert (out[2][:, 2:] == 0x03808080).all() and (out[2][:, :2] == formula(0x03808080, 0xFF102030)).all()


def test_compose_refuses_bad_frames(vp8g):
    f = {"argb": np.zeros((3, 3), np.uint32), "x": 2, "y": 0, "blend": 1, "dispose": 0, "has_alpha": 1}
    for cw, ch in ((4, 3), (5, 2), (0, 3), (16384, 3)):
        with pytest.raises(OSError) as ei:
            vp8g.host_anim_compose(cw, ch, [f])
        assert ei.value.errno == errno.EINVAL
    lib = vp8g.host_lib()
    assert lib.vp8f_anim_compose(4, 4, None, 1, None) == -1 and C.get_errno() == errno.EINVAL
    assert lib.vp8f_anim_keyframes(4, 4, None, 0) == -1 and C.get_errno() == errno.EINVAL


def test_old_parsers_still_refuse_animations(vp8g, golden):
    n = 0
    for name, e in golden["files"].items():
        data = fixture(name)
        try:
            vp8g.parse_anim(data)
        except OSError:
            continue
        for parse in (vp8g.parse_extended, vp8g.parse_any):
            with pytest.raises(OSError) as ei:
                parse(data)
            assert ei.value.errno == errno.ENOTSUP, name
        with pytest.raises(OSError) as ei:
            vp8g.parse_simple(data)
        assert ei.value.errno == errno.EINVAL, name
        n += 1
    assert n >= 16
    assert vp8g.gpu_lib().vp8g_abi_version() == 5


# ---- robustness: the new code under the sanitizers, as a program of its own -------------------------

def test_anim_under_sanitizers(tmp_path, golden):
    """tools/anim_san_main.c + the host sources, built with -fsanitize=address,undefined and run as a child process:
    every fixture, the bad files included, whole, truncated at every length (every chunk boundary among them) and
    with seeded single-byte corruptions through webp_parse_anim; what parses has its frames decoded and composed by
    vp8f_anim_compose.  Exit 0, no report."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    host = ROOT / "webp-decoder_amd" / "host"
    exe = tmp_path / "anim_san"
    srcs = [str(ROOT / "tools" / "anim_san_main.c")] + [str(host / f) for f in ("webp_riff.c", "vp8_parse.c", "vp8_synth.c", "vp8_scale.c",
                                                                              "vp8_alpha.c", "vp8_anim.c")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cc, "-std=c11", "-O2", "-g"] + san + ["-D_POSIX_C_SOURCE=200809L", "-o", str(exe)] + srcs + ["-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = [str(ANIM / f"{n}.webp") for n in sorted(golden["files"], key=lambda n: -golden["files"][n]["bytes"])]
    groups = [files[k::8] for k in range(8)]  # (eight children side by side: the long files dominate)
    procs = [subprocess.Popen([str(exe)] + g, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for g in groups]
    lines, composed = 0, 0
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0 and "ERROR" not in err and "runtime error" not in err, err[-2000:]
        lines += len(out.splitlines())
        composed += sum(int(line.split(" variants parsed, ")[1].split(" composed")[0]) for line in out.splitlines())
    assert lines == len(files) and composed >= 16
