#!/usr/bin/env python3
"""Regenerate tests/golden/lossless_scale.json: libwebp's answer for the lossless fixtures of
tests/golden/lossless/ decoded with its crop / scale options into RGBA.

The authority is the libwebp installed on the build machine (1.2.2, libwebp.so.7).  A small probe
(tools/libwebp_argb_scale_probe.c) is compiled into a temporary directory and linked against it; nothing is
written outside that directory and lossless_scale.json.  No fixture is written: the files are those of
make_lossless_golden.py.

For each (fixture, option) "cases" records the size libwebp returned and sha256 of its RGBA bytes; every
recorded case is one libwebp accepts.  "refusals" lists options the project refuses for a fixture, with its
errno name; they are not run through libwebp (which clamps or accepts some of them).

Usage: python tests/golden/make_lossless_scale_golden.py [--check]
"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "lossless_scale.json"
DIR = ROOT / "tests" / "golden" / "lossless"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"

# the opaque picture, real alpha (a disc; also at 257 x 70 and behind VP8X), palettes (levels40's carries random
# alpha), one pixel
FIXTURES = ["pic_67x45_m4q75", "disc_67x45_m4q75", "disc_160x100_m0q0", "disc_257x70_m6q100", "x_alpha_flag",
            "levels4_67x45_m4q75", "levels40_67x45_m0q50", "pic_257x70_m4q50", "pic_1x1_m4q75", "one_1x1_m4q75"]


def size_of(name: str):
    doc = json.loads((ROOT / "tests" / "golden" / "lossless.json").read_text())
    return doc["files"][name]["size"]


def options(w: int, h: int):
    """(crop or None, scale or None, expand) for a w x h fixture: the list of the issue, as far as the size allows."""
    o = [(None, None, False)]                                        # identity
    if w > 4 and h > 6:
        o.append(((1, 3, w - 4, h - 6), None, False))                # crop only, odd origin
        o.append(((w - 7, h - 5, 7, 5), None, False))                # ... ending at the last column and row
    if w > 3 and h > 3:
        o.append((None, ((w * 3 + 9) // 10, (h * 3 + 9) // 10), False))  # shrink both axes
        o.append((None, (w - 1, h - 1), False))                      # ... by one
        o.append((None, (w // 2, 0), False))                         # one dimension derived
        o.append((None, (0, h // 3), False))
        o.append((None, (w // 3, h + h // 2), True))                 # shrink x, expand y
        o.append((None, (w + w // 2 + 1, h // 2), True))             # expand x, shrink y
        o.append((None, (w, h // 2), False))                         # one axis kept
        o.append((None, (w // 2, h), False))
    o.append((None, (1, 1), False))                                  # shrink to 1 x 1
    o.append((None, (w + w // 2 + 1, h + h // 2 + 1), True))         # expand both
    o.append((None, (0, 2 * h + 1), True))                           # ... one dimension derived
    o.append((None, (w, h), False))                                  # a target equal to the window
    if w >= 67 and h >= 45:
        o.append(((3, 5, 31, 22), (9, 30), True))                    # crop plus scale: x shrinks, y expands
        o.append(((3, 5, 20, 10), (20, 10), False))                  # ... a target equal to the window
        o.append(((1, 1, 33, 21), (11, 7), False))
        o.append(((2, 3, 16, 16), (40, 0), True))
        o.append(((w - 9, h - 9, 9, 9), (4, 5), False))
    return o


# what the end-to-end test asks of the batch pipeline: the 67 x 45 files of its mixed batch into a 32 x 20 tensor, and
# one file through a per-frame option list
TENSOR = (32, 20)
BATCH = ["pic_67x45_m4q75", "disc_67x45_m4q75", "levels4_67x45_m4q75", "x_meta", "tiles_67x45_m6q100", "levels40_67x45_m0q50",
         "x_alpha_flag"]
PER_FRAME = [((3, 5, 32, 20), None, False), ((1, 3, 64, 40), TENSOR, False), ((3, 5, 16, 10), TENSOR, True)]


def all_cases():
    for name in FIXTURES:
        for o in options(*size_of(name)):
            yield (name,) + o
    for name in BATCH:
        yield name, None, TENSOR, False
    for o in PER_FRAME:
        yield ("disc_67x45_m4q75",) + o


REFUSALS = [
    # (fixture, crop, scale, expand, errno name)
    ("disc_67x45_m4q75", (60, 0, 8, 10), None, False, "EINVAL"),       # left + w > width
    ("disc_67x45_m4q75", (0, 40, 8, 6), None, False, "EINVAL"),        # top + h > height
    ("disc_67x45_m4q75", (3, 5, 0, 10), None, False, "EINVAL"),        # an empty window
    ("disc_67x45_m4q75", None, (68, 45), False, "EINVAL"),             # expand without the flag
    ("disc_67x45_m4q75", None, (0, 46), False, "EINVAL"),
    ("disc_67x45_m4q75", (3, 5, 31, 22), (9, 30), False, "EINVAL"),
    ("disc_67x45_m4q75", None, (16384, 45), True, "EINVAL"),           # a target beyond 16383
    ("pic_1x1_m4q75", (1, 0, 1, 1), None, False, "EINVAL"),
]


def generate():
    cases = []
    with tempfile.TemporaryDirectory() as td:
        td = pathlib.Path(td)
        exe = td / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(exe),
                        str(ROOT / "tools" / "libwebp_argb_scale_probe.c"), LIBWEBP], check=True)
        for name, crop, scale, expand in all_cases():
            c, s = crop or (0, 0, 0, 0), scale or (0, 0)
            dst = td / "out.rgba"
            r = subprocess.run([str(exe), str(DIR / f"{name}.webp"), str(dst)] + [str(v) for v in c + s],
                               capture_output=True, text=True)
            assert r.returncode == 0, (name, crop, scale, r.stderr)
            ow, oh = (int(v) for v in r.stdout.split())
            b = dst.read_bytes()
            assert len(b) == ow * oh * 4
            cases.append({"file": name, "crop": list(c), "scale": list(s), "expand": expand, "size": [ow, oh],
                          "rgba": hashlib.sha256(b).hexdigest()})
    return {
        "about": "libwebp's RGBA for tests/golden/lossless/*.webp decoded with crop / scale options "
                 "(tests/golden/make_lossless_scale_golden.py; probe tools/libwebp_argb_scale_probe.c)",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "cases": cases,
        "refusals": [{"file": f, "crop": list(c or (0, 0, 0, 0)), "scale": list(s or (0, 0)), "expand": e, "errno": en}
                     for f, c, s, e, en in REFUSALS],
    }


def main() -> int:
    doc = generate()
    text = json.dumps(doc, indent=None, separators=(",", ":")).replace('{"file"', '\n{"file"') + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text
        print("lossless scale golden: identical" if same else "lossless scale golden: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {len(doc['cases'])} cases to {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
