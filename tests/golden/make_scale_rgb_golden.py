#!/usr/bin/env python3
"""Regenerate tests/golden/scale_rgb.json: sha256 of libwebp's own scaled RGB.

The authority is the libwebp installed on the build machine (1.2.2, libwebp.so.7).  A small probe written
for this purpose (tools/libwebp_scale_rgb_probe.c) is compiled into a temporary directory and linked
against it; nothing is written outside that directory and scale_rgb.json.

  group "rgba"   WebPDecode in MODE_RGBA (not premultiplied) with use_cropping / use_scaling; the loop
                 filter is libwebp's own choice (VP8G_SCALE_DWEBP_FILTER on this side).  A case without a
                 target size (crop only, or no option) is there because it must NOT take the rescaler route.
                 "expand": the target exceeds the window, so this side needs VP8G_SCALE_EXPAND (libwebp needs nothing).
  group "rgb"    the same in MODE_RGB, for the cases the CLI check needs (decoder -rgb -scale).

The file holds hashes only.  Usage: python tests/golden/make_scale_rgb_golden.py [--check]
"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "scale_rgb.json"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"

K128 = "tests/fixtures/big/k128_normal.webp"
FHD = "tests/fixtures/big/fhd_normal_sharp5.webp"
ALPHA = ("tests/golden/alpha/enc_q50_af1.webp", "tests/golden/alpha/enc_random_alpha.webp", "tests/golden/alpha/ll_disc_f3.webp")
# (file, crop (left, top, w, h) or None, (scaled_w, scaled_h) or None)
RGBA_CASES = (
    [(K128, None, s) for s in ((40, 30), (64, 64), (100, 90), (127, 127), (128, 128), (200, 131))]
    + [(K128, (3, 5, 101, 99), s) for s in ((50, 0), (97, 33), (101, 99))]
    + [(K128, (7, 9, 31, 17), (1, 1)), ("tests/fixtures/commons/penguin-q20.webp", None, (224, 224))]
    + [(f, None, s) for f in ALPHA for s in ((20, 0), (0, 9))]
    + [(FHD, None, (640, 360)), (FHD, None, (1919, 1079)), (FHD, (1900, 1000, 20, 80), (10, 40)),
       ("tests/fixtures/big/fhd_simple_sharp3.webp", None, (480, 270))]
    + [(K128, (3, 5, 101, 99), None), (K128, None, None)]  # no target size: the fancy upsampler, not the rescaler
)
EXPANDS = {(K128, None, (200, 131))}  # the target exceeds the window
RGB_CASES = [(K128, None, (64, 64)), (K128, (3, 5, 101, 99), (50, 0))]


def generate() -> dict:
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        probe = tmp / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(probe),
                        str(ROOT / "tools" / "libwebp_scale_rgb_probe.c"), LIBWEBP], check=True)
        groups = {}
        for mode, cases in (("rgba", RGBA_CASES), ("rgb", RGB_CASES)):
            rows = groups[mode] = []
            for rel, crop, scale in cases:
                dst = tmp / "out.raw"
                r = subprocess.run([str(probe), str(ROOT / rel), mode] + [str(v) for v in (crop or (0, 0, 0, 0))]
                                   + [str(v) for v in (scale or (0, 0))] + [str(dst)], check=True, capture_output=True, text=True)
                ow, oh = (int(v) for v in r.stdout.split())
                data = dst.read_bytes()
                assert len(data) == ow * oh * len(mode)
                rows.append({"file": rel, "crop": list(crop) if crop else None, "scale": list(scale) if scale else None,
                             "expand": (rel, crop, scale) in EXPANDS,
                             "size": [ow, oh], "bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()})
    return {
        "about": "sha256 of libwebp's output (tests/golden/make_scale_rgb_golden.py; probe tools/libwebp_scale_rgb_probe.c)",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "rgba": groups["rgba"],
        "rgb": groups["rgb"],
    }


def main() -> int:
    text = json.dumps(generate(), indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text
        print("scale_rgb.json: identical" if same else "scale_rgb.json: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
