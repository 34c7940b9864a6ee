#!/usr/bin/env python3
"""Regenerate tests/golden/scale_expand.json: sha256 of libwebp's own bytes for the expand path of the
rescaler (VP8G_SCALE_EXPAND: upscaling, and mixed shrink / expand).

Same authority, probe, input generators and seeds as tests/golden/make_scale_golden.py (which this
script imports them from); only the cases differ.

  group "planes"   WebPPictureRescale of a W x H 4:2:0 picture to w x h, inputs random / ones / binary
  group "decode"   WebPDecode in MODE_YUV with use_cropping / use_scaling and bypass_filtering 0/1

The file holds hashes only.  Usage: python tests/golden/make_scale_expand_golden.py [--check]
"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_scale_golden import INCLUDE, KINDS, LIBWEBP, ROOT, plane_input  # noqa: E402

OUT = ROOT / "tests" / "golden" / "scale_expand.json"

# (W, H, w, h).  Both axes expanding, each mixed direction, sources one sample wide or high, ratios
# one sample over 1, chroma that is an identity or shrinks while luma expands
LISTED = [
    (1, 1, 2, 2), (1, 1, 4, 4), (2, 2, 3, 3), (2, 2, 2, 3), (3, 3, 4, 3), (5, 5, 9, 7), (7, 5, 3, 9), (9, 4, 20, 2),
    (1, 5, 3, 5), (5, 1, 5, 4), (2, 1, 3, 1), (3, 3, 2, 7), (1, 7, 9, 3), (7, 1, 3, 9), (15, 9, 16, 9), (15, 9, 15, 10),
    (16, 16, 37, 41), (13, 17, 12, 40), (40, 3, 41, 2), (31, 33, 32, 34), (64, 48, 65, 47), (64, 48, 63, 49),
    (17, 13, 256, 15), (3, 2, 300, 2), (2, 3, 2, 300), (100, 60, 224, 224),
]
# output widths around the expand kernel's tile widths (64, 128, 256 output columns when y expands, 256
# when only x does), in luma and (twice as wide) in chroma; x expanding, and x shrinking beside y expanding
TILE_WIDTHS = (
    [(40, 5, w, 7) for w in (63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 510, 512, 514)]
    + [(600, 5, 64, 8), (600, 5, 257, 8), (1000, 3, 129, 5)]
    + [(100, 9, w, 7) for w in (255, 256, 257, 511, 513)]
)
# output heights around the run heights (31, 63, 127 output rows for the three tile widths when y
# expands; 64 h / H when only x does)
RUN_HEIGHTS = [
    (10, 20, 200, 31), (10, 20, 200, 32), (10, 20, 200, 63), (10, 40, 100, 63), (10, 40, 100, 64), (10, 40, 100, 127),
    (10, 40, 60, 127), (10, 40, 60, 128), (10, 60, 60, 255), (300, 40, 200, 65),
    (20, 300, 50, 100), (20, 300, 50, 299), (10, 1000, 30, 3),
]
MAXIMA = [(3, 3, 16383, 2), (2, 3, 2, 16383), (16382, 1, 16383, 2)]
PLANE_CASES = LISTED + TILE_WIDTHS + RUN_HEIGHTS + MAXIMA

K128 = "big/k128_normal.webp"
# (fixture, crop (left, top, w, h) or None, (scaled_w, scaled_h))
DECODE_CASES = [
    (K128, None, (200, 200)), (K128, None, (64, 300)), (K128, None, (300, 64)), (K128, None, (129, 0)),
    (K128, (3, 5, 101, 99), (224, 0)),
    ("generated/gen_noise_16x16_q90.webp", None, (224, 224)),
    ("generated/gen_noise_17x17_q90.webp", None, (224, 224)),
    ("generated/gen_noise_31x31_q50.webp", None, (224, 224)),
]


def generate() -> dict:
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        probe = tmp / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(probe),
                        str(ROOT / "tools" / "libwebp_scale_probe.c"), LIBWEBP], check=True)
        planes = []
        for W, H, w, h in PLANE_CASES:
            for kind in KINDS:
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
        "about": "sha256 of libwebp's output (tests/golden/make_scale_expand_golden.py; probe tools/libwebp_scale_probe.c)",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "inputs": "as tests/golden/scale.json",
        "planes": planes,
        "decode": decode,
    }


def main() -> int:
    text = json.dumps(generate(), indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text
        print("scale_expand.json: identical" if same else "scale_expand.json: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
