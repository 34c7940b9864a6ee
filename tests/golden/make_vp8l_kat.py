#!/usr/bin/env python3
"""Regenerate tests/golden/vp8l_kat.json: libwebp's answer for every directed VP8L stream of tests/vp8l_streams.py.

The streams themselves are not stored: tests/vp8l_streams.py rebuilds them from its CASES table, and the sha256
recorded here pins what it builds.  The authority is the libwebp installed on the build machine (1.2.2,
libwebp.so.7) through tools/libwebp_lossless_probe.c, compiled into a temporary directory and linked against it,
as tests/golden/make_lossless_golden.py does.  Per case:

  bytes, sha256   of the file the case builds
  decodes         libwebp's verdict (WebPGetFeatures + WebPDecodeRGBA)
  size, rgba      for a stream libwebp decodes: the picture size and the sha256 of WebPDecodeRGBA's bytes
  alpha           for an ALPH case (a VP8X file around the VP8 chunk of a 67 x 45 lossy fixture of
                  tests/golden/alpha/): the sha256 of the alpha plane, every fourth byte of the above

"divergences" lists the streams libwebp decodes and the project's host decoder refuses, each with its reason; a
stream the project decodes and libwebp refuses ends the generator with an error, as does a picture of libwebp's
that is not the writer's.

Usage: python tests/golden/make_vp8l_kat.py [--check]
"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = ROOT / "tests" / "golden" / "vp8l_kat.json"
LIBWEBP = "/usr/lib/x86_64-linux-gnu/libwebp.so.7"
INCLUDE = "/opt/conda/include"
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
sys.path.insert(0, str(ROOT / "tests"))

# streams the project refuses and libwebp decodes: {case: reason}
DIVERGENCES = {}


def probe_rgba(exe: pathlib.Path, tmp: pathlib.Path, data: bytes):
    src, dst = tmp / "in.webp", tmp / "out.rgba"
    src.write_bytes(data)
    r = subprocess.run([str(exe), "rgba", str(src), str(dst)], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    w, h, _ = (int(v) for v in r.stdout.split())
    b = dst.read_bytes()
    assert len(b) == w * h * 4
    return w, h, b


def ours_decodes(vp8g, b) -> bool:
    try:
        if b.container == "alph":
            vp8g.host_alpha_plane(b.data)
        else:
            vp8g.host_lossless_argb(b.data)
        return True
    except OSError:
        return False


def generate():
    import vp8g
    import vp8l_streams as S
    cases = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        exe = tmp / "probe"
        subprocess.run(["gcc", "-std=c11", "-O2", "-I", INCLUDE, "-o", str(exe), str(ROOT / "tools" / "libwebp_lossless_probe.c"),
                        LIBWEBP], check=True)
        for name in S.NAMES:
            b = S.build(name)
            e = {"bytes": len(b.data), "sha256": S.sha(b.data)}
            got = probe_rgba(exe, tmp, b.data)
            e["decodes"] = got is not None
            if b.refuse is True and got is not None:
                raise SystemExit(f"{name}: meant as a refusal, and libwebp decodes it")
            if got is not None:
                w, h, px = got
                e["size"], e["rgba"] = [w, h], S.sha(px)
                if b.container == "alph":
                    plane = np.frombuffer(px, np.uint8).reshape(h, w, 4)[:, :, 3]
                    e["alpha"] = S.sha(plane.tobytes())
                    if b.alpha is None or not np.array_equal(plane, b.alpha):
                        raise SystemExit(f"{name}: libwebp's alpha plane is not the writer's")
                elif b.argb is None or px != S.rgba(b.argb):
                    raise SystemExit(f"{name}: libwebp's picture is not the writer's")
            ours = ours_decodes(vp8g, b)
            if ours and got is None:
                raise SystemExit(f"{name}: the project decodes a stream libwebp refuses")
            if got is not None and not ours and name not in DIVERGENCES:
                raise SystemExit(f"{name}: libwebp decodes a stream the project refuses, and DIVERGENCES gives no reason")
            cases[name] = e
    return {
        "about": "libwebp's answers for the directed VP8L streams of tests/vp8l_streams.py (tests/golden/make_vp8l_kat.py; probe "
                 "tools/libwebp_lossless_probe.c); hashes and small integers only: the streams are rebuilt from the table",
        "libwebp": "1.2.2 (libwebp.so.7)",
        "divergences": [{"case": n, "reason": r} for n, r in sorted(DIVERGENCES.items())],
        "cases": cases,
    }


def main() -> int:
    text = json.dumps(generate(), indent=1) + "\n"
    if "--check" in sys.argv[1:]:
        same = OUT.exists() and OUT.read_text() == text
        print("vp8l kat: identical" if same else "vp8l kat: DIFFERS")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
