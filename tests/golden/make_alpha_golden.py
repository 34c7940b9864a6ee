#!/usr/bin/env python3
"""Regenerate tests/golden/alpha/*.webp and tests/golden/alpha.json: the fixtures of the extended
container / alpha path and libwebp's answer for each of them.

The authority is the libwebp installed on the build machine (1.2.2, libwebp.so.7).  A small probe
(tools/libwebp_alpha_probe.c) is compiled into a temporary directory and linked against it; nothing is
written outside that directory, tests/golden/alpha/ and alpha.json.

Every fixture is a hand-wrapped RIFF file (or libwebp's own WebPEncode output, group "enc"):
  VP8 part       libwebp's lossy encoding of a seeded opaque picture of the fixture's size
  raw ALPH       header byte filter << 2, then the forward-filtered plane
  lossless ALPH  header byte filter << 2 | 1, then libwebp's LOSSLESS encoding of an ARGB picture whose
                 green channel is the forward-filtered plane, with the 5 bytes of its VP8L header removed
                 (red and blue non-zero in "argb": the only way to the subtract-green and cross-colour
                 transforms, which libwebp's own alpha encoder never emits)
For each file alpha.json records libwebp's verdict (WebPDecode), the picture size, sha256 of A (MODE_YUVA)
and of Y / U / V (MODE_YUV, what `dwebp -yuv` writes: in MODE_YUVA libwebp multiplies the luma of a picture
with alpha by alpha around its rescaler) plain and under two crop / scale options, and -- where the project's host decoder reads
the ALPH chunk -- the Vp8fAlphaStats it reported.  "uncovered" names every counter of Vp8fAlphaStats that
no fixture libwebp decodes reaches, with the encoder settings tried.

Usage: python tests/golden/make_alpha_golden.py [--check]
"""
import hashlib
import json
import pathlib
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "alpha.json"
DIR = ROOT / "tests" / "golden" / "alpha"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

F_ICC, F_ALPHA, F_EXIF, F_XMP, F_ANIM = 0x20, 0x10, 0x08, 0x04, 0x02


def chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(body: bytes, riff_size=None) -> bytes:
    return b"RIFF" + struct.pack("<I", len(body) + 4 if riff_size is None else riff_size) + b"WEBP" + body


def vp8x(flags: int, w: int, h: int) -> bytes:
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3])


def chunks_of(data: bytes):
    pos, out = 12, []
    while pos + 8 <= len(data):
        n = struct.unpack("<I", data[pos + 4:pos + 8])[0]
        out.append((data[pos:pos + 4], data[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
    return out


def forward_filter(a: np.ndarray, f: int) -> np.ndarray:
    """The residual plane whose un-prediction is `a`."""
    a = a.astype(np.int32)
    h, w = a.shape
    pred = np.zeros_like(a)
    if f:
        pred[0, 1:] = a[0, :-1]
        pred[1:, 0] = a[:-1, 0]
        left, up, ul = a[1:, :-1], a[:-1, 1:], a[:-1, :-1]
        pred[1:, 1:] = left if f == 1 else up if f == 2 else np.clip(left + up - ul, 0, 255)
    return ((a - pred) & 255).astype(np.uint8)


def scale_cases(w: int, h: int, top: int = 5):
    """The two crop / scale options of a w x h fixture: (name, crop or None, scale, expand).
    top = 0 for the streams on which libwebp 1.2.2 contradicts itself under a crop: a colour-indexed lossless
    ALPH with the horizontal filter is un-predicted from the crop's first row on, with nothing above it (its
    paletted path skips the rows above crop_top for filters 0 and 1), so column 0 of the cropped plane is not
    column 0 of the uncropped one.  The project un-predicts the whole plane; those fixtures crop from row 0."""
    if w < 16 or h < 16:
        return []
    return [("shrink", (3, top, w - 6, h - 7), ((w - 6) * 5 // 8, (h - 7) * 3 // 5), False),
            ("expand", None, (w * 3 // 2 + 1, h * 2 + 1), True)]


class Probe:
    def __init__(self, tmp: pathlib.Path):
        self.tmp = tmp
        self.exe = tmp / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(self.exe),
                        str(ROOT / "tools" / "libwebp_alpha_probe.c"), LIBWEBP], check=True)

    def decode(self, data: bytes, crop=None, scale=None):
        src, dst = self.tmp / "in.webp", self.tmp / "out.yuva"
        src.write_bytes(data)
        c, s = crop or (0, 0, 0, 0), scale or (0, 0)
        r = subprocess.run([str(self.exe), "decode", str(src)] + [str(v) for v in c] + [str(s[0]), str(s[1]), str(dst)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            return None
        w, h, has_alpha = (int(v) for v in r.stdout.split())
        b = dst.read_bytes()
        cw, ch = (w + 1) // 2, (h + 1) // 2
        o = [0, w * h, w * h + cw * ch, w * h + 2 * cw * ch, 2 * w * h + 2 * cw * ch]
        assert len(b) == o[4]
        d = {"size": [w, h], "has_alpha": has_alpha}
        for k, name in enumerate("yuva"):
            d[name] = hashlib.sha256(b[o[k]:o[k + 1]]).hexdigest()
        d["a_opaque"] = all(v == 255 for v in b[o[3]:o[4]])
        return d

    def lossless(self, argb: np.ndarray, method: int = 4, quality: int = 75) -> bytes:
        """The VP8L chunk payload libwebp's lossless encoder writes for uint32 [h, w] 0xAARRGGBB pixels."""
        src, dst = self.tmp / "in.argb", self.tmp / "out.webp"
        src.write_bytes(argb.astype("<u4").tobytes())
        h, w = argb.shape
        subprocess.run([str(self.exe), "lossless", str(w), str(h), str(src), str(method), str(quality), str(dst)], check=True)
        (tag, payload), = [c for c in chunks_of(dst.read_bytes()) if c[0] == b"VP8L"]
        return payload

    def lossy(self, rgba: np.ndarray, quality=60, alpha_quality=100, alpha_filtering=1, alpha_compression=1) -> bytes:
        src, dst = self.tmp / "in.rgba", self.tmp / "out.webp"
        src.write_bytes(rgba.astype(np.uint8).tobytes())
        h, w = rgba.shape[:2]
        subprocess.run([str(self.exe), "lossy", str(w), str(h), str(src), str(quality), str(alpha_quality),
                        str(alpha_filtering), str(alpha_compression), str(dst)], check=True)
        return dst.read_bytes()


def picture(w: int, h: int, seed: int, noise: int = 6) -> np.ndarray:
    """A seeded opaque RGBA picture: gradients, a few rectangles and a little noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([(x * 255) // max(1, w - 1), (y * 255) // max(1, h - 1), ((x + y) * 3) & 255], axis=-1).astype(np.int32)
    for _ in range(4):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        rgb[y0:y0 + h // 3 + 1, x0:x0 + w // 3 + 1] = rng.integers(0, 256, 3)
    rgb += rng.integers(-noise, noise + 1, rgb.shape)
    return np.concatenate([np.clip(rgb, 0, 255), np.full((h, w, 1), 255)], axis=-1).astype(np.uint8)


def alpha_content(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind.startswith("levels"):  # n distinct levels in blobs
        n = int(kind[6:])
        levels = np.linspace(0, 255, n).astype(np.int32)
        return levels[((x // 5 + y // 3 + rng.integers(0, 2, (h, w))) * 7) % n].astype(np.uint8)
    if kind == "ramp":
        return ((x * 200) // max(1, w - 1) + (y * 55) // max(1, h - 1)).astype(np.uint8)
    if kind == "disc":  # a soft-edged disc: 0 and 255 plateaus, so the gradient predictor clips
        d = np.hypot(x - w / 2, y - h / 2) / (min(w, h) / 2)
        return np.clip((1.1 - d) * 900, 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "tiles":  # a noisy tile repeated: backward references at short distances
        t = rng.integers(0, 256, (7, 9), dtype=np.uint8)
        return np.tile(t, (h // 7 + 1, w // 9 + 1))[:h, :w]
    if kind == "mixed":  # regions of different statistics: an entropy image pays off
        a = ((x * 255) // max(1, w - 1)).astype(np.uint8)
        a[:h // 2, w // 2:] = rng.integers(0, 256, (h // 2, w - w // 2), dtype=np.uint8)
        a[h // 2:, :w // 2] = np.tile(rng.integers(0, 256, (5, 6), dtype=np.uint8), (h, w))[:h - h // 2, :w // 2]
        a[h // 2:, w // 2:] = (rng.integers(0, 4, (h - h // 2, w - w // 2)) * 85).astype(np.uint8)
        return a
    if kind == "one":
        return np.full((h, w), 200, np.uint8)
    raise ValueError(kind)


# (name, kind, (w, h), filter, lossless encoder (method, quality))
LOSSLESS = [
    ("ll_levels2_f0", "levels2", (37, 21), 0, (4, 75)), ("ll_levels2_f3", "levels2", (67, 45), 3, (4, 75)),
    ("ll_levels4_f1", "levels4", (37, 21), 1, (4, 75)), ("ll_levels4_f0", "levels4", (64, 48), 0, (6, 100)),
    ("ll_levels16_f2", "levels16", (37, 21), 2, (4, 75)), ("ll_levels16_f0", "levels16", (64, 48), 0, (4, 75)),
    ("ll_levels40_f3", "levels40", (64, 48), 3, (4, 75)), ("ll_levels40_f0", "levels40", (64, 48), 0, (4, 75)),
    ("ll_ramp_f0", "ramp", (160, 100), 0, (4, 75)), ("ll_ramp_f1", "ramp", (160, 100), 1, (4, 75)),
    ("ll_ramp_f3", "ramp", (160, 100), 3, (6, 100)), ("ll_disc_f3", "disc", (160, 100), 3, (4, 75)),
    ("ll_disc_f2", "disc", (67, 45), 2, (4, 75)), ("ll_noise_f0", "noise", (64, 48), 0, (4, 75)),
    ("ll_noise_f2", "noise", (37, 21), 2, (0, 10)), ("ll_tiles_f0", "tiles", (160, 100), 0, (4, 75)),
    ("ll_tiles_f1", "tiles", (67, 45), 1, (6, 100)), ("ll_mixed_f0", "mixed", (192, 128), 0, (4, 75)),
    ("ll_mixed_f3", "mixed", (192, 128), 3, (4, 75)),
    ("ll_one_f0", "one", (37, 21), 0, (4, 75)), ("ll_one_f1", "one", (1, 1), 1, (4, 75)),
]
# general ARGB pictures through the header-strip route: (name, (w, h), filter, (method, quality))
ARGB = [("ll_argb_f0", (160, 100), 0, (4, 75)), ("ll_argb_f1", (37, 21), 1, (4, 75)), ("ll_argb_f2", (37, 21), 2, (4, 75)),
        ("ll_argb_f3", (37, 21), 3, (4, 75)), ("ll_argb_m0", (128, 80), 0, (0, 0))]


# Where the project deliberately answers otherwise than libwebp: name -> (the project's answer, why).
# "decodes as X": the alpha plane is that of fixture X.
DIVERGENCES = {
    "c_simple_vp8l": ("ENOTSUP", "a lossless main image is out of scope"),
    "c_vp8l_image": ("ENOTSUP", "a lossless main image is out of scope"),
    "raw_f3_rsrv": ("decodes as raw_f3", "RFC 9649 2.7.1.2: readers MUST ignore the reserved bits; libwebp 1.2.2 refuses a non-zero value"),
}


def build_fixtures(pr: Probe) -> dict:
    files = {}
    vp8_cache = {}

    def vp8(w, h):
        if (w, h) not in vp8_cache:
            (tag, payload), = chunks_of(pr.lossy(picture(w, h, w * 131 + h)))
            assert tag == b"VP8 "
            vp8_cache[(w, h)] = chunk(b"VP8 ", payload)
        return vp8_cache[(w, h)]

    def wrap(w, h, alph, flags=F_ALPHA):
        return riff(vp8x(flags, w, h) + chunk(b"ALPH", alph) + vp8(w, h))

    # raw alpha, each filter
    a = alpha_content("disc", 37, 21, 1)
    for f in range(4):
        files[f"raw_f{f}"] = wrap(37, 21, bytes([f << 2]) + forward_filter(a, f).tobytes())
    # (reserved and pre-processing bits are ignored; libwebp refuses values above 1 in either field)
    files["raw_f3_pre"] = wrap(37, 21, bytes([0x10 | 3 << 2]) + forward_filter(a, 3).tobytes())
    files["raw_f3_rsrv"] = wrap(37, 21, bytes([0x40 | 3 << 2]) + forward_filter(a, 3).tobytes())
    alph_of = {}
    for name, kind, (w, h), f, (m, q) in LOSSLESS:
        res = forward_filter(alpha_content(kind, w, h, w * 7 + h), f)
        argb = 0xFF000000 | (res.astype(np.uint32) << 8)
        alph_of[name] = (w, h, bytes([f << 2 | 1]) + pr.lossless(argb, m, q)[5:])
        files[name] = wrap(w, h, alph_of[name][2])
    for name, (w, h), f, (m, q) in ARGB:
        p = picture(w, h, w + h * 977 + f, noise=1).astype(np.uint32)
        res = forward_filter(p[:, :, 1].astype(np.uint8), f).astype(np.uint32)
        argb = 0xFF000000 | p[:, :, 0] << 16 | res << 8 | p[:, :, 2]
        alph_of[name] = (w, h, bytes([f << 2 | 1]) + pr.lossless(argb, m, q)[5:])
        files[name] = wrap(w, h, alph_of[name][2])
    # libwebp's own encoder
    for aq in (100, 50):
        for af in (0, 1, 2):
            p = picture(64, 48, 5)
            p[:, :, 3] = alpha_content("disc", 64, 48, 9)
            files[f"enc_q{aq}_af{af}"] = pr.lossy(p, alpha_quality=aq, alpha_filtering=af)
    p = picture(37, 21, 6)
    p[:, :, 3] = alpha_content("noise", 37, 21, 3)
    files["enc_random_alpha"] = pr.lossy(p)
    files["enc_uncompressed"] = pr.lossy(p, alpha_compression=0)
    # extended, no alpha, with metadata
    w, h = 37, 21
    files["x_meta"] = riff(vp8x(F_ICC | F_EXIF | F_XMP, w, h) + chunk(b"ICCP", b"icc" * 11) + chunk(b"zzzz", b"odd") + vp8(w, h)
                           + chunk(b"EXIF", b"Exif\0\0II") + chunk(b"XMP ", b"<x/>"))
    files["x_meta_alpha"] = riff(vp8x(F_ICC | F_ALPHA | F_EXIF, w, h) + chunk(b"ICCP", b"i") + chunk(b"ALPH", bytes([4]) + forward_filter(a, 1).tobytes())
                                 + chunk(b"abcd", b"12345") + vp8(w, h) + chunk(b"EXIF", b"e"))
    # containers where the RFC leaves a choice, and malformed ones
    raw1 = bytes([4]) + forward_filter(a, 1).tobytes()
    raw2 = bytes([0]) + a.T.copy().tobytes()
    files["c_alph_after_image"] = riff(vp8x(F_ALPHA, w, h) + vp8(w, h) + chunk(b"ALPH", raw1))
    files["c_two_alph"] = riff(vp8x(F_ALPHA, w, h) + chunk(b"ALPH", raw1) + chunk(b"ALPH", raw2) + vp8(w, h))
    files["c_flag_no_chunk"] = riff(vp8x(F_ALPHA, w, h) + vp8(w, h))
    files["c_chunk_no_flag"] = riff(vp8x(0, w, h) + chunk(b"ALPH", raw1) + vp8(w, h))
    files["c_empty_alph"] = riff(vp8x(F_ALPHA, w, h) + chunk(b"ALPH", b"") + vp8(w, h))
    body = vp8x(F_ALPHA, w, h) + chunk(b"ALPH", raw1) + vp8(w, h)
    files["c_riff_small"] = riff(body + b"trailing bytes", len(body) + 4)
    files["c_riff_big"] = riff(body, len(body) + 4 + 10)
    files["c_riff_cuts_image"] = riff(body, len(body) + 4 - 6)
    files["c_chunk_overrun"] = riff(vp8x(F_ALPHA, w, h) + b"ALPH" + struct.pack("<I", 100000) + raw1 + vp8(w, h))
    files["c_no_image"] = riff(vp8x(F_ALPHA, w, h) + chunk(b"ALPH", raw1))
    files["c_canvas_mismatch"] = riff(vp8x(F_ALPHA, w + 1, h) + chunk(b"ALPH", raw1) + vp8(w, h))
    files["c_vp8x_size"] = riff(b"VP8X" + struct.pack("<I", 12) + bytes([F_ALPHA, 0, 0, 0, w - 1, 0, 0, h - 1, 0, 0, 0, 0]) + vp8(w, h))
    files["c_anim_flag"] = riff(vp8x(F_ALPHA | F_ANIM, w, h) + chunk(b"ALPH", raw1) + vp8(w, h))
    files["c_anmf"] = riff(vp8x(0, w, h) + chunk(b"ANMF", b"\0" * 16 + vp8(w, h)))
    files["c_vp8l_image"] = riff(vp8x(0, w, h) + chunk(b"VP8L", pr.lossless(np.full((h, w), 0xFF102030, np.uint32))))
    files["c_simple_vp8l"] = riff(chunk(b"VP8L", pr.lossless(np.full((h, w), 0xFF102030, np.uint32))))
    files["c_simple"] = riff(vp8(w, h))
    # ALPH streams that do not decode
    files["bad_raw_short"] = wrap(w, h, raw1[:-1])
    files["bad_compression"] = wrap(w, h, bytes([2]) + raw1[1:])
    for name in ("ll_ramp_f3", "ll_argb_f0", "ll_levels4_f1"):
        ww, hh, alph = alph_of[name]
        files["bad_trunc_" + name[3:]] = wrap(ww, hh, alph[:len(alph) // 2])
        files["bad_trunc8_" + name[3:]] = wrap(ww, hh, alph[:8])
    ww, hh, alph = alph_of["ll_argb_f0"]
    for k, off in enumerate((1, 3, 6)):  # the transform bits / the first prefix-code headers
        b = bytearray(alph)
        b[off] ^= 0xFF
        files[f"bad_corrupt{k}"] = wrap(ww, hh, bytes(b))
    return files


# ALPH payloads of 3840 x 2160 planes for tools/alpha_bench.py's end-to-end leg (libwebp's own alpha encoder,
# alpha_quality 100): (name, kind, alpha_filtering).  Written to tests/golden/alpha_bench/NAME.alph.
BENCH_DIR = ROOT / "tests" / "golden" / "alpha_bench"
BENCH = [("uhd_disc", "disc", 1), ("uhd_ramp", "ramp", 2)]


def build_bench(pr: Probe):
    import vp8g
    out, doc = {}, {}
    w, h = 3840, 2160
    for name, kind, af in BENCH:
        p = np.full((h, w, 4), 128, np.uint8)
        a = alpha_content(kind, w, h, 11)
        p[:, :, 3] = a
        alph = dict(chunks_of(pr.lossy(p, quality=30, alpha_filtering=af)))[b"ALPH"]
        assert len(alph) < 600000
        res, flt, st = vp8g.alpha_decode_host(alph, w, h)
        assert np.array_equal(vp8g.host_alpha_unfilter(res, flt), a)  # (alpha_quality 100 is exact)
        out[name] = alph
        doc[name] = {"bytes": len(alph), "sha256": hashlib.sha256(alph).hexdigest(), "size": [w, h], "filter": flt,
                     "a": hashlib.sha256(a.tobytes()).hexdigest(), "stats": st}
    return out, doc


def generate():
    import vp8g
    with tempfile.TemporaryDirectory() as td:
        pr = Probe(pathlib.Path(td))
        files = build_fixtures(pr)
        entries = {}
        for name, data in sorted(files.items()):
            e = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
            d = pr.decode(data)
            e["decodes"] = d is not None
            st = {}
            try:
                c = vp8g.parse_extended(data)
                if c["alpha"]:
                    kf_w, kf_h = c["canvas_width"], c["canvas_height"]
                    _, flt, st = vp8g.alpha_decode_host(
                        data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]], kf_w, kf_h)
                    e["filter"], e["stats"] = flt, st
            except OSError:
                pass
            if d:
                e.update(d)
                e["scaled"] = {}
                top = 0 if st.get("color_index") and e.get("filter") == 1 else 5
                for sname, crop, scale, expand in scale_cases(*d["size"], top):
                    s = pr.decode(data, crop, scale)
                    e["scaled"][sname] = dict(s, crop=list(crop) if crop else None, scale=list(scale), expand=expand)
            entries[name] = e
        bench_files, bench_doc = build_bench(pr)
    reached = {n for e in entries.values() if e["decodes"] for n, v in e.get("stats", {}).items() if v}
    uncovered = {n: "not emitted by libwebp 1.2.2's lossless encoder at methods 0 / 4 / 6, quality 0 - 100, on any picture of the set"
                 for n in vp8g.ALPHA_STATS if n not in reached}
    doc = {
        "about": "libwebp's answers for tests/golden/alpha/*.webp (tests/golden/make_alpha_golden.py; probe tools/libwebp_alpha_probe.c)",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "uncovered": uncovered,
        "divergences": {n: {"ours": a, "why": w} for n, (a, w) in DIVERGENCES.items()},
        "files": entries,
        "bench": bench_doc,
    }
    return files, doc, bench_files


def main() -> int:
    files, doc, bench = generate()
    text = json.dumps(doc, indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text and all(
            (DIR / f"{n}.webp").exists() and (DIR / f"{n}.webp").read_bytes() == b for n, b in files.items()) and all(
            (BENCH_DIR / f"{n}.alph").exists() and (BENCH_DIR / f"{n}.alph").read_bytes() == b for n, b in bench.items())
        print("alpha golden: identical" if same else "alpha golden: DIFFERS")
        return 0 if same else 1
    DIR.mkdir(exist_ok=True)
    BENCH_DIR.mkdir(exist_ok=True)
    for n, b in bench.items():
        (BENCH_DIR / f"{n}.alph").write_bytes(b)
    for n, b in files.items():
        (DIR / f"{n}.webp").write_bytes(b)
    OUT.write_text(text)
    print(f"wrote {len(files)} fixtures ({sum(len(b) for b in files.values())} bytes) and {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
