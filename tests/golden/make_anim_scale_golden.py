#!/usr/bin/env python3
"""Regenerate tests/golden/anim_scale.json: libwebp's answer for the canvases of the animations of
tests/golden/anim/ cropped and rescaled to a target size.

libwebp has no scaled animation decoder, so the answer is composed of two things it does have.  Canvas k of a
file is what WebPAnimDecoder composes: the host restatement (vp8g.host_anim_compose) gives it, and the generator
asserts that its RGBA has the sha256 anim.json already holds for that canvas (libwebp's own).  That canvas is then
encoded losslessly and exactly by libwebp 1.2.2 (tools/libwebp_alpha_probe.c lossless) and decoded by libwebp with
its crop / scale options into RGBA (tools/libwebp_argb_scale_probe.c) -- the route DESIGN.md §17.7 pins to
vp8f_argb_scale for arbitrary ARGB.  Both probes are compiled into a temporary directory; nothing is written outside
it and anim_scale.json.  No fixture is written: the files are those of make_anim_golden.py.

For each (animation, option) "cases" records the size libwebp returned and, per canvas, the sha256 of its RGBA bytes:
hashes, not pixels.  "refusals" lists options the project refuses for an animation, with its errno name; they are not
run through libwebp (which clamps or accepts some of them).

Usage: python tests/golden/make_anim_scale_golden.py [--check]
"""
import hashlib
import importlib.util
import json
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "anim_scale.json"
DIR = ROOT / "tests" / "golden" / "anim"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

_spec = importlib.util.spec_from_file_location("make_alpha_golden", ROOT / "tests" / "golden" / "make_alpha_golden.py")
ag = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ag)

# both 20 x 14 rule animations, the 64 x 48 one of lossy, lossless and lossy-with-alpha frames, the 1 x 1 canvas, one frame
ANIMS = ["rules_a", "rules_b", "mixed", "canvas_1x1", "one_frame"]


def options(w: int, h: int):
    """(crop or None, scale or None, expand) for a w x h canvas, as far as the size allows."""
    o = [(None, (w, h), False)]                                      # a target equal to the canvas (not the identity)
    o.append((None, (1, 1), False))                                  # shrink to 1 x 1
    o.append((None, (w + w // 2 + 1, 0), True))                      # expand x, the height derived (expands too)
    o.append((None, (w + 1, h + 2), True))                           # expand both axes
    if w > 6 and h > 6:
        o.append((None, ((w * 3 + 9) // 10, (h * 3 + 9) // 10), False))  # shrink both axes
        o.append((None, (w - 1, h - 1), False))                      # ... by one
        o.append((None, (w // 2, 0), False))                         # one dimension derived
        o.append(((1, 3, w - 4, h - 6), (w // 3, h // 3), False))    # an odd-origin crop plus shrink
        o.append(((1, 3, w - 4, h - 6), None, False))                # a crop only
        o.append(((3, 1, w - 5, h - 3), (w - 5, h - 3), False))      # a crop and a target equal to it
        o.append((None, (w // 3, h + h // 2), True))                 # shrink x, expand y
        o.append((None, (w + w // 2 + 1, h // 2), True))             # expand x, shrink y
    return o


# what the end-to-end test asks of the entry: canvases of different sizes into one 16 x 12 tensor
TENSOR = (16, 12)
SHARED = ["rules_a", "mixed"]


def all_cases():
    for name in ANIMS:
        for o in options(*canvas_of(name)):
            yield (name,) + o
    for name in SHARED:
        yield name, None, TENSOR, False


REFUSALS = [
    # (animation, crop, scale, expand, errno name)
    ("rules_a", (15, 0, 8, 10), None, False, "EINVAL"),   # left + w beyond the canvas
    ("rules_a", None, (21, 14), False, "EINVAL"),         # expand without the flag
    ("mixed", (0, 40, 8, 9), (4, 4), False, "EINVAL"),    # top + h beyond the canvas
    ("canvas_1x1", (1, 0, 1, 1), None, False, "EINVAL"),
]


def anim_doc():
    return json.loads((ROOT / "tests" / "golden" / "anim.json").read_text())


def canvas_of(name: str):
    return anim_doc()["files"][name]["canvas"]


def generate():
    import numpy as np
    import vp8g
    doc = anim_doc()["files"]
    cases = []
    with tempfile.TemporaryDirectory() as td:
        td = pathlib.Path(td)
        enc = ag.Probe(td)
        exe = td / "scale_probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(exe),
                        str(ROOT / "tools" / "libwebp_argb_scale_probe.c"), LIBWEBP], check=True)
        stills = {}
        for name in ANIMS:
            (cw, ch), frames, _ = vp8g.host_anim_frames((DIR / f"{name}.webp").read_bytes())
            canvases, _ = vp8g.host_anim_compose(cw, ch, frames)
            assert doc[name]["decodes"] and len(canvases) == doc[name]["nframes"]
            stills[name] = []
            for k, c in enumerate(canvases):
                # the canvas that is encoded is the one libwebp's WebPAnimDecoder composes
                assert hashlib.sha256(vp8g.argb_to_rgba(c).tobytes()).hexdigest() == doc[name]["frames"][k]["rgba"], (name, k)
                path = td / f"{name}_{k}.webp"
                path.write_bytes(ag.riff(ag.chunk(b"VP8L", enc.lossless(np.ascontiguousarray(c), 4, 75))))
                stills[name].append(path)
        for name, crop, scale, expand in all_cases():
            c, s = crop or (0, 0, 0, 0), scale or (0, 0)
            hashes, size = [], None
            for path in stills[name]:
                dst = td / "out.rgba"
                r = subprocess.run([str(exe), str(path), str(dst)] + [str(v) for v in c + s], capture_output=True, text=True)
                assert r.returncode == 0, (name, crop, scale, r.stderr)
                ow, oh = (int(v) for v in r.stdout.split())
                b = dst.read_bytes()
                assert len(b) == ow * oh * 4 and size in (None, [ow, oh])
                size = [ow, oh]
                hashes.append(hashlib.sha256(b).hexdigest())
            cases.append({"file": name, "crop": list(c), "scale": list(s), "expand": expand, "size": size, "rgba": hashes})
    return {
        "about": "libwebp's RGBA for every canvas of tests/golden/anim/*.webp, encoded losslessly and decoded with crop / scale "
                 "options (tests/golden/make_anim_scale_golden.py; probes tools/libwebp_alpha_probe.c, tools/libwebp_argb_scale_probe.c)",
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
        print("anim scale golden: identical" if same else "anim scale golden: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {len(doc['cases'])} cases to {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
