#!/usr/bin/env python3
"""Regenerate tests/golden/anim/*.webp and tests/golden/anim.json: the fixtures of the animation path
 and libwebp's answer for each of them.

The authority is libwebp's WebPAnimDecoder (MODE_RGBA, default options) as installed on the build machine:
tools/libwebp_anim_probe.c is compiled into a temporary directory and linked against libwebpdemux (1.2.0, which
brings its own libwebp 1.2.0).  The sub-frames come from the encoders of libwebp 1.2.2 through the alpha generator's
probe (tools/libwebp_alpha_probe.c), as the other goldens obtain them: lossless (exact), lossy, and lossy with an
ALPH chunk.  Because the two libwebp versions differ, every sub-frame's stand-alone decode by the demuxer's libwebp
is asserted equal to the project's host decode (vp8g.host_still_argb) before anything is written.

The container is assembled by hand, so every offset, flag and order is chosen.  For each file anim.json records
libwebp's verdict (accepts: WebPAnimDecoderNew; decodes: every WebPAnimDecoderGetNext), the canvas, the loop count,
per frame the sha256 of the RGBA canvas and the timestamp, and the fields the file was assembled from (what the
project's parser must report).  A file on which the project deliberately answers otherwise carries a "divergence"
entry (the project's answer and why); on every other file the generator asserts that the parser's verdict is libwebp's.

Usage: python tests/golden/make_anim_golden.py [--check]
"""
import hashlib
import importlib.util
import json
import pathlib
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "anim.json"
DIR = ROOT / "tests" / "golden" / "anim"
INCLUDE = "/opt/conda/include"
LIBDIR = "/opt/conda/lib"
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

_spec = importlib.util.spec_from_file_location("make_alpha_golden", ROOT / "tests" / "golden" / "make_alpha_golden.py")
ag = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ag)
chunk, riff, vp8x, chunks_of = ag.chunk, ag.riff, ag.vp8x, ag.chunks_of

ALPHAS = np.array([0, 1, 3, 128, 254, 255], np.uint32)


class AnimProbe:
    def __init__(self, tmp: pathlib.Path):
        self.tmp = tmp
        self.exe = tmp / "anim_probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(self.exe), str(ROOT / "tools" / "libwebp_anim_probe.c"),
                        "-L", LIBDIR, "-lwebpdemux", "-lwebp", f"-Wl,-rpath,{LIBDIR}"], check=True)
        self.versions = subprocess.run([str(self.exe), "version"], capture_output=True, text=True, check=True).stdout.split()

    def anim(self, data: bytes):
        """None (refused), or {"canvas", "loop_count", "bgcolor", "decodes", "frames": [(rgba bytes, timestamp)]}."""
        src, dst = self.tmp / "in.webp", self.tmp / "out.rgba"
        src.write_bytes(data)
        r = subprocess.run([str(self.exe), "anim", str(src), str(dst)], capture_output=True, text=True)
        if r.returncode == 1:
            return None
        assert r.returncode in (0, 3), r.stderr
        lines = r.stdout.split("\n")
        w, h, n, loop, bg = (int(v) for v in lines[0].split())
        d = {"canvas": [w, h], "loop_count": loop, "bgcolor": bg, "nframes": n, "decodes": r.returncode == 0, "frames": []}
        if d["decodes"]:
            b = dst.read_bytes()
            assert len(b) == n * w * h * 4
            d["frames"] = [(b[k * w * h * 4:(k + 1) * w * h * 4], int(lines[1 + k])) for k in range(n)]
        return d

    def rgba(self, data: bytes):
        src, dst = self.tmp / "in.webp", self.tmp / "out.rgba"
        src.write_bytes(data)
        r = subprocess.run([str(self.exe), "rgba", str(src), str(dst)], capture_output=True, text=True)
        if r.returncode != 0:
            return None
        w, h, _ = (int(v) for v in r.stdout.split())
        return np.frombuffer(dst.read_bytes(), np.uint8).reshape(h, w, 4)


def le24(v: int) -> bytes:
    return struct.pack("<I", v)[:3]


def anim_chunk(loop: int = 0, bg: int = 0) -> bytes:
    return chunk(b"ANIM", struct.pack("<IH", bg, loop))


def anmf(x, y, w, h, duration, blend, dispose, sub: bytes) -> bytes:
    return chunk(b"ANMF", le24(x // 2) + le24(y // 2) + le24(w - 1) + le24(h - 1) + le24(duration)
                 + bytes([(1 if dispose else 0) | (0 if blend else 2)]) + sub)


def noise_argb(w, h, seed, alphas=ALPHAS) -> np.ndarray:
    """uint32 [h, w] 0xAARRGGBB: blocks of colour with a little noise, alpha drawn from `alphas` (every colour
    non-zero, also under alpha 0)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = rng.integers(1, 256, (4, 4, 3))[(y * 4 // max(h, 1)) % 4, (x * 4 // max(w, 1)) % 4]
    rgb = np.clip(base + rng.integers(-3, 4, (h, w, 3)), 1, 255).astype(np.uint32)
    a = np.asarray(alphas, np.uint32)[rng.integers(0, len(alphas), (h, w))]
    return a << 24 | rgb[:, :, 0] << 16 | rgb[:, :, 1] << 8 | rgb[:, :, 2]


class Builder:
    def __init__(self, enc: "ag.Probe"):
        self.enc = enc

    def lossless(self, argb, clear_alpha_bit=False) -> bytes:
        p = bytearray(self.enc.lossless(argb, 4, 75))
        if clear_alpha_bit:
            p[4] &= ~0x10
        return chunk(b"VP8L", bytes(p))

    def lossy(self, w, h, seed, alpha=None) -> bytes:
        """'VP8 ' (opaque), or ALPH + 'VP8 ' when alpha (uint8 [h, w]) is given."""
        p = ag.picture(w, h, seed)
        if alpha is not None:
            p[:, :, 3] = alpha
        cs = chunks_of(self.enc.lossy(p))
        out = b"".join(chunk(t, d) for t, d in cs if t in ((b"ALPH", b"VP8 ") if alpha is not None else (b"VP8 ",)))
        assert (b"ALPH" in out[:4]) == (alpha is not None)
        return out


def sub_kind(sub: bytes) -> str:
    return {b"VP8L": "lossless", b"VP8 ": "lossy", b"ALPH": "lossy_alpha"}[sub[:4]]


def sub_has_alpha(sub: bytes) -> int:
    return 1 if sub[:4] == b"ALPH" else (sub[12] >> 4) & 1 if sub[:4] == b"VP8L" else 0


def assemble(cw, ch, frames, loop=0, bg=0, flags=ag.F_ANIM | ag.F_ALPHA, between=b"", lead=b""):
    """frames: [(x, y, w, h, duration, blend, dispose, sub-chunks)].  Returns (file, assembled fields)."""
    body = vp8x(flags, cw, ch) + lead + anim_chunk(loop, bg)
    for k, (x, y, w, h, dur, blend, dispose, sub) in enumerate(frames):
        body += anmf(x, y, w, h, dur, blend, dispose, sub) + (between if k + 1 < len(frames) else b"")
    fields = [{"x": x, "y": y, "width": w, "height": h, "duration": dur, "blend": int(blend), "dispose": int(dispose),
               "has_alpha": sub_has_alpha(sub), "kind": sub_kind(sub)} for x, y, w, h, dur, blend, dispose, sub in frames]
    return riff(body), {"canvas": [cw, ch], "loop_count": loop, "frames": fields}


def rules_a(b: Builder):
    """20 x 14, 14 lossless frames: every combination of blend, dispose and the previous frame's dispose, rectangles of
    1 x 1, the canvas, touching each edge, inside and outside the previous rectangle."""
    rects = [(0, 0, 20, 14), (2, 2, 9, 7), (4, 4, 5, 3), (10, 6, 10, 8), (0, 0, 1, 1), (0, 4, 7, 10), (6, 0, 14, 5),
             (2, 2, 16, 10), (8, 6, 3, 3), (0, 0, 20, 14), (12, 8, 8, 6), (12, 8, 8, 6), (18, 12, 1, 1), (0, 0, 20, 14)]
    modes = [(1, 0), (1, 1), (1, 0), (0, 1), (1, 1), (1, 0), (0, 0), (1, 1), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (1, 0)]
    return [(x, y, w, h, 40 + 10 * k, bl, di, b.lossless(noise_argb(w, h, 100 + k))) for k, ((x, y, w, h), (bl, di)) in
            enumerate(zip(rects, modes))]


def rules_b(b: Builder):
    """20 x 14, 14 lossless frames: a full-canvas blending frame after a partial KEY frame that disposed to background
    (itself a key frame: it comes out equal to its source) and after a partial NON-key frame that did (blended everywhere
    but in that rectangle); chains of key frames made by disposal alone."""
    full = (0, 0, 20, 14)
    spec = [((4, 2, 9, 7), 1, 1),    # 0 key (first), partial, disposes
            (full, 1, 0),            # 1 key: the previous disposed and was a key frame
            ((6, 4, 8, 6), 1, 1),    # 2 partial, not key, disposes
            (full, 1, 0),            # 3 NOT key: blended outside frame 2's rectangle
            ((0, 0, 20, 14), 1, 1),  # 4 full, alpha, blends: not key; disposes the whole canvas
            ((2, 2, 5, 5), 1, 1),    # 5 key (previous full + disposed), disposes
            ((10, 6, 6, 4), 1, 1),   # 6 key (previous key + disposed), disposes
            ((10, 6, 6, 4), 0, 0),   # 7 key again
            ((8, 4, 10, 8), 1, 0),   # 8 blends over 7
            (full, 0, 0),            # 9 key: full and no blend
            ((0, 10, 20, 4), 1, 1),  # 10 bottom edge
            ((0, 8, 20, 6), 1, 0),   # 11 overlaps the cleared strip and the rows above it
            ((14, 0, 6, 14), 1, 1),  # 12 right edge
            (full, 1, 1)]            # 13 blended outside frame 12's rectangle
    return [(x, y, w, h, 30, bl, di, b.lossless(noise_argb(w, h, 200 + k))) for k, ((x, y, w, h), bl, di) in enumerate(spec)]


def build_fixtures(b: Builder):
    files, built = {}, {}

    def add(name, *a, **kw):
        files[name], built[name] = assemble(*a, **kw)

    add("rules_a", 20, 14, rules_a(b), loop=3)
    add("rules_b", 20, 14, rules_b(b))
    # lossy, lossless and lossy-with-alpha frames in one animation
    disc = ag.alpha_content("disc", 30, 22, 4)
    steps = ALPHAS[np.random.default_rng(9).integers(0, 6, (16, 24))].astype(np.uint8)
    add("mixed", 64, 48, [
        (0, 0, 64, 48, 100, 1, 0, b.lossy(64, 48, 1)),
        (10, 8, 30, 22, 50, 1, 0, b.lossy(30, 22, 2, disc)),
        (20, 20, 25, 17, 50, 1, 1, b.lossless(noise_argb(25, 17, 3))),
        (0, 30, 24, 16, 70, 1, 0, b.lossy(24, 16, 4, steps)),
        (38, 0, 26, 48, 20, 0, 1, b.lossy(26, 48, 5)),
        (0, 0, 64, 48, 60, 1, 0, b.lossless(noise_argb(64, 48, 6))),
        (62, 46, 1, 1, 10, 1, 0, b.lossless(noise_argb(1, 1, 7, [128]))),
        (0, 0, 64, 48, 90, 1, 0, b.lossy(64, 48, 8, ag.alpha_content("ramp", 64, 48, 1))),
    ], loop=1, bg=0x80FF4020)
    add("one_frame", 33, 21, [(0, 0, 33, 21, 120, 1, 0, b.lossless(noise_argb(33, 21, 11)))])
    add("one_frame_partial", 33, 21, [(4, 6, 10, 9, 0, 1, 1, b.lossless(noise_argb(10, 9, 12)))])
    add("zero_durations", 16, 16, [(0, 0, 16, 16, 0, 1, 0, b.lossless(noise_argb(16, 16, 13))),
                                   (2, 2, 8, 8, 0, 1, 0, b.lossless(noise_argb(8, 8, 14))),
                                   (4, 4, 8, 8, 5, 1, 1, b.lossless(noise_argb(8, 8, 15))),
                                   (6, 6, 1, 1, 0, 1, 0, b.lossless(noise_argb(1, 1, 16, [3])))])
    add("canvas_1x1", 1, 1, [(0, 0, 1, 1, 10, 1, 0, b.lossless(noise_argb(1, 1, 17, [1]))),
                             (0, 0, 1, 1, 10, 1, 0, b.lossless(noise_argb(1, 1, 18, [128])))])
    # sa = 0 with colour over an opaque and over a translucent canvas
    add("transparent_colour", 12, 10, [(0, 0, 12, 10, 10, 0, 0, b.lossless(noise_argb(12, 10, 19, [255, 128]))),
                                       (0, 0, 12, 10, 10, 1, 0, b.lossless(noise_argb(12, 10, 20, [0]))),
                                       (2, 2, 8, 6, 10, 1, 0, b.lossless(noise_argb(8, 6, 21, [0, 1, 254])))])
    # a full-canvas lossless frame whose header says "no alpha" while its pixels are not opaque: a key frame by the rule
    add("alpha_bit_cleared", 18, 12, [(0, 0, 18, 12, 10, 1, 0, b.lossless(noise_argb(18, 12, 22))),
                                      (0, 0, 18, 12, 10, 1, 0, b.lossless(noise_argb(18, 12, 23), clear_alpha_bit=True)),
                                      (4, 2, 9, 7, 10, 1, 0, b.lossless(noise_argb(9, 7, 24)))])
    # containers libwebp accepts
    fr = [(0, 0, 16, 12, 10, 1, 0, b.lossless(noise_argb(16, 12, 30))), (2, 2, 8, 6, 15, 1, 0, b.lossless(noise_argb(8, 6, 31)))]
    add("c_chunks_between", 16, 12, fr, flags=ag.F_ANIM | ag.F_ALPHA | ag.F_EXIF | ag.F_ICC, lead=chunk(b"ICCP", b"icc"),
        between=chunk(b"zzzz", b"odd") + chunk(b"EXIF", b"Exif\0\0II"))
    add("c_second_anim_ignored", 16, 12, fr, loop=2, between=anim_chunk(7, 0xFFFFFFFF))
    tail = [(x, y, w, h, d, bl, di, sub + chunk(b"zzzz", b"after the image") + chunk(b"abcd", b"x")) for x, y, w, h, d, bl, di, sub in fr]
    add("c_subchunk_after_image", 16, 12, tail)
    # the ANMF header names 6 x 6, the bitstream is 8 x 6: the bitstream's size counts
    files["c_size_from_bitstream"], built["c_size_from_bitstream"] = assemble(16, 12, [fr[0], (2, 2, 6, 6, 15, 1, 0, fr[1][7])])[0], assemble(16, 12, fr)[1]
    f, built["c_riff_small"] = assemble(16, 12, fr)
    files["c_riff_small"] = f + b"trailing bytes"
    # libwebp walks a frame's sub-chunks up to the first one it does not recognise and reads on from there at the top
    # level: an ANMF that holds nothing it recognises is no frame (dropped) where its content passes as top-level chunks
    # -- nothing, or an unknown chunk -- and refused where an image follows
    f, s = assemble(16, 12, fr)
    body = f[12:]
    hdr = le24(0) + le24(0) + le24(15) + le24(11) + le24(10) + b"\0"
    empty = chunk(b"ANMF", hdr)
    cut = len(vp8x(0, 1, 1)) + len(anim_chunk())
    files["c_empty_frame_dropped"], built["c_empty_frame_dropped"] = riff(body[:cut] + empty + body[cut:]), s
    files["c_unknown_only_dropped"], built["c_unknown_only_dropped"] = riff(body + chunk(b"ANMF", hdr + chunk(b"zzzz", b"first"))), s
    files["bad_unknown_before_image"] = riff(body[:cut] + chunk(b"ANMF", hdr + chunk(b"zzzz", b"first") + fr[0][7]) + body[cut:])
    files["bad_anim_inside_anmf"] = riff(body[:cut] + chunk(b"ANMF", hdr + anim_chunk() + fr[0][7]) + body[cut:])
    # files libwebp refuses
    good, _ = assemble(16, 12, fr)
    files["bad_truncated"] = good[:len(good) - 9]
    files["bad_riff_big"] = good[:4] + struct.pack("<I", len(good) - 8 + 2) + good[8:]
    files["bad_anmf_before_anim"] = riff(vp8x(ag.F_ANIM, 16, 12) + anmf(*fr[0]) + anim_chunk() + anmf(*fr[1]))
    files["bad_outside_canvas"] = assemble(16, 12, [fr[0], (10, 2, 8, 6, 15, 1, 0, fr[1][7])])[0]
    files["bad_outside_canvas_y"] = assemble(16, 12, [fr[0], (2, 8, 8, 6, 15, 1, 0, fr[1][7])])[0]
    files["bad_no_image_last"] = riff(body + empty)
    files["bad_alph_only"] = riff(body + chunk(b"ANMF", le24(0) + le24(0) + le24(15) + le24(11) + le24(10) + b"\0" + chunk(b"ALPH", b"\0" * 193)))
    files["bad_no_frames"] = riff(vp8x(ag.F_ANIM, 16, 12) + anim_chunk())
    files["bad_flag_only"] = riff(vp8x(ag.F_ANIM, 16, 12))
    files["bad_no_anim_flag"] = assemble(16, 12, fr, flags=ag.F_ALPHA)[0]
    files["bad_alph_before_vp8l"] = assemble(16, 12, [fr[0], (2, 2, 8, 6, 15, 1, 0, chunk(b"ALPH", b"\0" * 49) + fr[1][7])])[0]
    files["bad_top_level_image"] = riff(body + fr[0][7])
    files["bad_short_anmf"] = riff(body + chunk(b"ANMF", b"\0" * 14))
    files["bad_short_anim"] = riff(vp8x(ag.F_ANIM, 16, 12) + chunk(b"ANIM", b"\0\0\0\0") + anmf(*fr[0]))
    files["bad_reserved_flag"] = assemble(16, 12, fr, flags=ag.F_ANIM | 0x01)[0]
    files["bad_subchunk_overrun"] = riff(body[:cut] + b"ANMF" + struct.pack("<I", 16 + len(fr[0][7]) - 2) + anmf(*fr[0])[8:] + body[cut:])
    files["bad_vp8l_header"] = assemble(16, 12, [fr[0], (2, 2, 8, 6, 15, 1, 0, chunk(b"VP8L", b"\x2e" + fr[1][7][9:]))])[0]
    files["bad_junk_tail"] = riff(body + b"junk")
    # a frame whose stream does not decode: the container is fine, WebPAnimDecoderGetNext fails
    p = fr[1][7]
    files["bad_frame_stream"], built["bad_frame_stream"] = assemble(16, 12, [fr[0], (2, 2, 8, 6, 15, 1, 0, chunk(b"VP8L", p[8:8 + 5] + bytes(len(p) - 13)))])
    # a still picture: libwebp's WebPAnimDecoder shows it as one frame; webp_parse_anim is for animations only
    files["still_lossless"] = riff(chunk(b"VP8L", fr[0][7][8:]))
    files["still_vp8x"] = riff(vp8x(ag.F_ALPHA, 16, 12) + fr[0][7])
    return files, built


DIVERGENCES = {
    "still_lossless": ("EINVAL", "a still picture is not an animation here; gpu_decode_webp_batch_tensor decodes it"),
    "still_vp8x": ("EINVAL", "a still picture is not an animation here; gpu_decode_webp_batch_tensor decodes it"),
}


def ours(vp8g, data: bytes):
    try:
        return vp8g.parse_anim(data)
    except OSError as e:
        return e.errno


def generate():
    import vp8g
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        pr, b = AnimProbe(tmp), Builder(ag.Probe(tmp))
        files, built = build_fixtures(b)
        entries = {}
        for name, data in sorted(files.items()):
            e = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
            d = pr.anim(data)
            e["accepts"] = d is not None
            mine = ours(vp8g, data)
            if d:
                e.update({k: d[k] for k in ("canvas", "loop_count", "bgcolor", "nframes", "decodes")})
                e["frames"] = [{"rgba": hashlib.sha256(px).hexdigest(), "timestamp": ts} for px, ts in d["frames"]]
            if name in DIVERGENCES:
                e["divergence"] = list(DIVERGENCES[name])
                assert isinstance(mine, int), name
            else:
                assert isinstance(mine, dict) == e["accepts"], (name, "the parser and libwebp disagree", mine if isinstance(mine, int) else "accepted")
            if name in built:
                e["built"] = built[name]
            if isinstance(mine, dict) and d and d["decodes"]:
                # every sub-frame: the demuxer's libwebp and the project's host decoder give the same pixels
                for k, f in enumerate(mine["frames"]):
                    still = vp8g.wrap_anim_frame(data, f)
                    want = pr.rgba(still)
                    assert want is not None and np.array_equal(vp8g.argb_to_rgba(vp8g.host_still_argb(still)), want), (name, k)
            entries[name] = e
        versions = pr.versions
    doc = {
        "about": "libwebp's answers for tests/golden/anim/*.webp (tests/golden/make_anim_golden.py; probe tools/libwebp_anim_probe.c)",
        "libwebp": {"demux": versions[0], "decoder": versions[1], "encoders": "1.2.2 (libwebp.so.7, through tools/libwebp_alpha_probe.c)"},
        "files": entries,
    }
    return files, doc


def main() -> int:
    files, doc = generate()
    text = json.dumps(doc, indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text and all(
            (DIR / f"{n}.webp").exists() and (DIR / f"{n}.webp").read_bytes() == b for n, b in files.items())
        print("anim golden: identical" if same else "anim golden: DIFFERS")
        return 0 if same else 1
    DIR.mkdir(exist_ok=True)
    for n, b in files.items():
        (DIR / f"{n}.webp").write_bytes(b)
    OUT.write_text(text)
    print(f"wrote {len(files)} fixtures ({sum(len(b) for b in files.values())} bytes) and {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
