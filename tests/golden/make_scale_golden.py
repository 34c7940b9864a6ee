#!/usr/bin/env python3
"""Regenerate tests/golden/scale.json: sha256 of libwebp's own bytes for the crop + downscale path.

The authority is the libwebp installed on the build machine (1.2.2, libwebp.so.7).  A small probe
written for this purpose (tools/libwebp_scale_probe.c) is compiled into a temporary directory and
linked against it; nothing is written outside that directory and scale.json.

  group "planes"   WebPPictureRescale of a W x H 4:2:0 picture to w x h.  Inputs, n = I420 size:
                     random  numpy.random.default_rng(seed).integers(0, 256, size=n, dtype=uint8)
                     binary  numpy.random.default_rng(seed).integers(0, 2, size=n, dtype=uint8) * 255
                     ones    all 255
                   one draw in the order Y, U, V (as random_i420 in tests/test_gpu_rgb.py);
                   seed = W * 131 + H.
  group "decode"   WebPDecode in MODE_YUV with use_cropping / use_scaling and bypass_filtering 0/1
                   on fixtures of tests/fixtures.

The file holds hashes only.  Usage: python tests/golden/make_scale_golden.py [--check]
"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "scale.json"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"

# (W, H, w, h): identity, ratios just under 1, huge ratios, tiles that straddle the kernel's tile
# width, both maximum dimensions, an accumulator that wraps 2^32
PLANE_CASES = [
    (1, 1, 1, 1), (2, 2, 1, 1), (16, 16, 16, 16), (17, 13, 16, 12), (16, 16, 1, 1), (33, 31, 7, 5), (64, 48, 63, 47),
    (129, 77, 64, 38), (100, 100, 33, 34), (257, 3, 3, 3), (3, 257, 3, 2), (5, 5, 5, 1), (5, 5, 1, 5), (1000, 7, 999, 1),
    (255, 255, 254, 3), (640, 480, 224, 224), (16383, 2, 5, 1), (2, 16383, 1, 7), (1920, 1080, 224, 224),
    (3840, 2160, 1, 1), (8192, 2100, 1, 1), (3840, 64, 3, 64),
]
ONES_ONLY = {(8192, 2100, 1, 1)}  # (the accumulator wraps 2^32 only with every sample at 255)
KINDS = ("random", "ones", "binary")

SIMPLE_FHD = "big/fhd_simple_sharp3.webp"
# (fixture, crop (left, top, w, h) or None, (scaled_w, scaled_h))
DECODE_CASES = [
    ("big/k128_normal.webp", None, (64, 64)),
    ("big/k128_normal.webp", None, (96, 0)),
    ("big/k128_normal.webp", None, (127, 127)),
    ("big/k128_normal.webp", (3, 5, 101, 99), (50, 0)),
    ("commons/penguin-q20.webp", None, (224, 224)),
    ("commons/penguin-q20.webp", None, (2000, 2400)),
    ("big/fhd_normal_sharp5.webp", None, (640, 360)),
    ("big/fhd_normal_sharp5.webp", None, (1919, 1079)),
    ("big/fhd_normal_sharp5.webp", (1900, 1000, 20, 80), (10, 40)),
    (SIMPLE_FHD, None, (480, 270)),
]


def plane_input(kind: str, w: int, h: int) -> np.ndarray:
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    seed = w * 131 + h
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)
    if kind == "binary":
        return np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8) * np.uint8(255)
    return np.full(n, 255, dtype=np.uint8)


def generate() -> dict:
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        probe = tmp / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(probe),
                        str(ROOT / "tools" / "libwebp_scale_probe.c"), LIBWEBP], check=True)
        planes = []
        for W, H, w, h in PLANE_CASES:
            for kind in KINDS:
                if (W, H, w, h) in ONES_ONLY and kind != "ones":
                    continue
                src, dst = tmp / "in.i420", tmp / "out.i420"
                src.write_bytes(plane_input(kind, W, H).tobytes())
                subprocess.run([str(probe), "rescale", str(W), str(H), str(w), str(h), str(src), str(dst)], check=True)
                planes.append({"src": [W, H], "dst": [w, h], "kind": kind, "seed": W * 131 + H,
                               "sha256": hashlib.sha256(dst.read_bytes()).hexdigest()})
        decode = []
        for rel, crop, scale in DECODE_CASES:
            for bypass in (0, 1):
                c = crop or (0, 0, 0, 0)
                dst = tmp / "out.i420"
                r = subprocess.run([str(probe), "decode", str(ROOT / "tests" / "fixtures" / rel), str(bypass)]
                                   + [str(v) for v in c] + [str(scale[0]), str(scale[1]), str(dst)], check=True,
                                   capture_output=True, text=True)
                ow, oh = (int(v) for v in r.stdout.split())
                decode.append({"file": rel, "crop": list(crop) if crop else None, "scale": list(scale), "bypass": bypass,
                               "size": [ow, oh], "sha256": hashlib.sha256(dst.read_bytes()).hexdigest()})
    return {
        "about": "sha256 of libwebp's output (tests/golden/make_scale_golden.py; probe tools/libwebp_scale_probe.c)",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "inputs": {
            "random": "numpy.random.default_rng(seed).integers(0, 256, size=n, dtype=uint8), order Y, U, V",
            "binary": "numpy.random.default_rng(seed).integers(0, 2, size=n, dtype=uint8) * 255, order Y, U, V",
            "ones": "all 255",
            "seed": "W * 131 + H",
        },
        "planes": planes,
        "decode": decode,
    }


def main() -> int:
    text = json.dumps(generate(), indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text
        print("scale.json: identical" if same else "scale.json: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
