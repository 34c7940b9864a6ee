#!/usr/bin/env python3
"""Generate tests/golden/stream_kat.json (run where oracle/_ref -- the reference's own m01-m07 and the
libwebp probe, compiled by oracle/Makefile -- exists).

For every case of tests/streams.py CASES: the stream's sha256 and length, the reference's m05
coefficient hash and the sha256 of the reference's `-yuv` / `-yuvf` output on that stream.  A native
multi-partition case, which the reference rejects, takes these three from its one-partition twin (the
same frame).  `libwebp_same` records whether libwebp 1.2.2 (oracle/_ref/libwebp_probe) decodes the
stream itself to the same bytes (null: libwebp refuses the stream).  The bar is the reference:
  * a case built on profile 0 must have libwebp_same true, else generation fails -- unless the
    reference and libwebp themselves differ there and the host path (front end + oracle) equals the
    reference; such a case is named in `notes`;
  * for the full-range kinds (|coefficient| up to 2114: libwebp keeps dequantised coefficients in
    int16) and the cut streams (libwebp refuses a partition shorter than declared) the flag is
    recorded only.
The GPU box needs only this file and oracle/libstreamw.so, never the reference.
"""
import ctypes as C
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import streams  # noqa: E402
import vp8g  # noqa: E402

# Profile-0 cases on which the reference and libwebp 1.2.2 themselves differ (the host path equals the
# reference on each; generation fails for any disagreement not listed here):
KNOWN_DIFFERENCES = {
    "h_seg_nodata_s": "segmentation on with no feature data: libwebp's initial segment mode is absolute (quantiser and "
                      "level 0 in every segment), the reference's is delta (the frame's values)",
    "lf07": "frame filter level 0 with absolute segment levels above 0: libwebp turns the filter off for the whole "
            "frame, the reference filters those segments",
    "lf11": "libwebp adds the ref / mode deltas to the unclamped segment level (33 - 63 + 2 -> 0), the reference clamps "
            "the segment level to 0..63 first (0 + 2 = 2)",
}

PROBE = ROOT / "oracle" / "_ref" / "libwebp_probe"


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def ref_outputs(path, w, h):
    ref = vp8g.ref_lib()
    out = []
    for filtered in (0, 1):
        buf = np.empty(vp8g.i420_size(w, h), np.uint8)
        if ref.ref_decode_i420(str(path).encode(), buf.ctypes.data, buf.size, filtered) != buf.size:
            raise RuntimeError(f"reference decode failed: {path}")
        out.append(buf.tobytes())
    return ref.ref_coeff_hash(str(path).encode()), out[0], out[1]


def libwebp_outputs(path, tmp):
    out = []
    for args in (["-nofilter"], []):
        o = tmp / "lw.yuv"
        if subprocess.run([str(PROBE), *args, str(path), str(o)], capture_output=True).returncode != 0:
            return None
        out.append(o.read_bytes())
    return out


def main():
    out = {"generator": "tests/golden/make_stream_kat.py", "spec": "tests/streams.py CASES / build(case)",
           "reference": "oracle/_ref/libref.so (reference m01-m07); libwebp 1.2.2 via oracle/_ref/libwebp_probe",
           "notes": [], "cases": {}}
    ref_of = {}
    with tempfile.TemporaryDirectory() as d:
        tmp = pathlib.Path(d)
        for case in streams.single_partition() + streams.multi_partition():
            b = streams.build(case)
            path = tmp / "s.webp"
            path.write_bytes(b.data)
            w, h = case["size"]
            if case["log2k"] == 0:
                ref_of[case["name"]] = ref_outputs(path, w, h)
            chash, yuv, yuvf = ref_of[case["twin"] if case["log2k"] else case["name"]]
            lw = libwebp_outputs(path, tmp)
            same = None if lw is None else (lw[0] == yuv and lw[1] == yuvf)
            if streams.base_profile0(case) and not case["cut"] and same is not True:
                g = streams.decode(b.data)
                host = g is not None and vp8g.oracle_reconstruct(g, False) == yuv and vp8g.oracle_reconstruct(g, True) == yuvf
                base = case["twin"] or case["name"]
                if base not in KNOWN_DIFFERENCES or (not case["log2k"] and not host):
                    raise SystemExit(f"{case['name']}: libwebp disagrees with the reference on a profile-0 case")
                out["notes"].append(f"{case['name']}: the reference and libwebp differ ({KNOWN_DIFFERENCES[base]}); "
                                    + (f"as for its one-partition twin {base}" if case["log2k"] else
                                       "the host path equals the reference"))
            out["cases"][case["name"]] = {"sha256": sha(b.data), "length": len(b.data), "coeff_hash": f"{chash:016x}",
                                          "yuv_sha256": sha(yuv), "yuvf_sha256": sha(yuvf), "libwebp_same": same}
    out["cases"] = {c["name"]: out["cases"][c["name"]] for c in streams.CASES}
    (ROOT / "tests" / "golden" / "stream_kat.json").write_text(json.dumps(out, indent=1) + "\n")
    n = sum(1 for v in out["cases"].values() if v["libwebp_same"] is False)
    print("stream KAT:", len(out["cases"]), "cases;", n, "differ from libwebp;", len(out["notes"]), "notes")


if __name__ == "__main__":
    main()
