#!/usr/bin/env python3
"""Generate tests/golden/directed_kat.json (run where oracle/_ref/libref.so, the reference's own
m01-m07 compiled by oracle/Makefile, exists).

For every case of tests/directed.py kat_cases() -- each directed kind at 320x256 and at 33x50 -- sha256
of the reference's m06 (`yuv`) and m06 + m07 (`yuvf`) output on the frame directed.build() makes.
The inputs are the builder's spec, the outputs hashes: the GPU box needs only this file, never the
reference.  tests/test_directed.py holds the oracle to it, tests/test_gpu_directed.py the kernels.
"""
import hashlib
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import directed  # noqa: E402
import vp8g  # noqa: E402


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def main():
    out = {"generator": "tests/golden/make_directed_kat.py", "spec": "tests/directed.py build(kind, width, height, seed)",
           "reference": "oracle/_ref/libref.so (reference m06/m07)", "cases": {}}
    for case in directed.kat_cases():
        f = directed.build(*case)
        out["cases"][directed.kat_key(*case)] = {"yuv_sha256": sha(vp8g.ref_reconstruct(f, False)),
                                                 "yuvf_sha256": sha(vp8g.ref_reconstruct(f, True))}
        f.free()
    (ROOT / "tests" / "golden" / "directed_kat.json").write_text(json.dumps(out, indent=1) + "\n")
    print("directed KAT:", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
