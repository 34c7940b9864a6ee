"""The RFC 9649 stream decoder of host/vp8_alpha.c against the directed streams of tests/vp8l_streams.py (DESIGN.md
§17.8): what the writer spelled out is what vp8f_lossless_decode / vp8f_alpha_decode must read -- the picture, the
transform list and every counter --, libwebp (tests/golden/vp8l_kat.json) is the second witness for pixels and
verdicts, the refusals are refused at every length, and the whole set runs under the sanitizers as a program of
its own."""
import ctypes as C
import errno
import json
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vp8l_streams as S
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "vp8l_kat.json").read_text())


ACCEPTED = [n for n in S.NAMES if S.build(n).refuse is None]
DECIDED = [n for n in S.NAMES if n not in S.REFUSALS and n not in ACCEPTED]  # (the verdict is libwebp's)


def test_the_table_and_the_json_name_the_same_cases(kat):
    assert list(kat["cases"]) == list(S.NAMES)
    assert set(S.REFUSALS) == {n for n in S.NAMES if S.build(n).refuse is True}
    assert len(ACCEPTED) >= 115 and len(S.REFUSALS) >= 18 and len(DECIDED) == 2
    for n in S.NAMES:
        b = S.build(n)
        assert max(b.width, b.height) <= 300, n
        assert (b.argb is not None or b.alpha is not None) == (n not in S.REFUSALS), n


def test_streams_are_the_recorded_ones(kat):
    for n in S.NAMES:
        b, e = S.build(n), kat["cases"][n]
        assert (len(b.data), S.sha(b.data)) == (e["bytes"], e["sha256"]), n


def decode(vp8g, b):
    """("decodes", picture or alpha plane, transforms, stats) or (errno name, None, None, None)."""
    try:
        if b.container == "alph":
            assert vp8g.parse_extended(b.data)["alpha"]
            res, flt, st = vp8g.alpha_decode_host(b.payload, b.width, b.height)
            return "decodes", vp8g.host_alpha_unfilter(res, flt), None, st
        c = vp8g.parse_any(b.data)
        assert b.data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]] == b.payload
        im = vp8g.lossless_decode_host(b.payload)
        return "decodes", vp8g.host_lossless_apply(im), im["transforms"], im["stats"]
    except OSError as e:
        return errno.errorcode[e.errno], None, None, None


def test_accepted_streams_give_the_writers_picture_and_libwebps(vp8g, kat):
    for n in ACCEPTED:
        b, e = S.build(n), kat["cases"][n]
        verdict, got, _, _ = decode(vp8g, b)
        assert verdict == "decodes" and e["decodes"], n
        assert e["size"] == [b.width, b.height], n
        if b.container == "alph":
            assert np.array_equal(got, b.alpha), n
            assert S.sha(got.tobytes()) == e["alpha"], n
        else:
            bad = np.argwhere(got != b.argb)
            assert bad.size == 0, (n, bad[:4].tolist())
            assert S.sha(vp8g.argb_to_rgba(got).tobytes()) == e["rgba"] == S.sha(S.rgba(b.argb)), n


def test_transforms_and_stats_equal_the_writers_census(vp8g):
    for n in ACCEPTED:
        b = S.build(n)
        _, _, trs, st = decode(vp8g, b)
        assert {k: st[k] for k in S.CENSUS} == {k: b.census[k] for k in S.CENSUS}, n
        assert st["raw"] == 0, n
        if trs is None:
            continue
        assert [(t["type"], t["bits"], t["xsize"], t["ncolors"]) for t in trs] == [
            (t["type"], t["bits"], t["xsize"], t["ncolors"]) for t in b.transforms], n
        for t, want in zip(trs, b.transforms):
            if t["type"] == S.CI:
                assert t["data"].tolist() == want["table"], n
            elif t["type"] != S.SG:
                assert np.array_equal(t["data"], want["data"]), n


def test_refused_streams_are_einval_at_every_length(vp8g, kat):
    lib = vp8g.host_lib()
    zero = bytes(C.sizeof(vp8g.Vp8fLosslessImage))
    for n in S.REFUSALS:
        b = S.build(n)
        assert not kat["cases"][n]["decodes"], n
        assert vp8g.parse_any(b.data)["lossless"], n  # (the container is sound: the stream is what is refused)
        p = b.payload
        buf = (C.c_uint8 * len(p)).from_buffer_copy(p)
        for k in range(len(p), -1, -1):
            im = vp8g.Vp8fLosslessImage()
            C.memset(C.byref(im), 0xA5, C.sizeof(im))
            C.set_errno(0)
            assert lib.vp8f_lossless_decode(buf, k, C.byref(im), None) == -1 and C.get_errno() == errno.EINVAL, (n, k)
            assert bytes(im) == zero, (n, k)


def test_verdicts_are_libwebps(vp8g, kat):
    """Every case, the two whose verdict the format leaves to the decoder included.  The divergences the JSON lists
    (streams the project refuses and libwebp decodes; never the other way round) are exactly the ones found: none."""
    found = []
    for n in S.NAMES:
        verdict, _, _, _ = decode(vp8g, S.build(n))
        theirs = kat["cases"][n]["decodes"]
        assert verdict in ("decodes", "EINVAL"), n
        assert not (verdict == "decodes" and not theirs), n
        if theirs and verdict != "decodes":
            found.append(n)
    assert found == [d["case"] for d in kat["divergences"]] == []
    assert [kat["cases"][n]["decodes"] for n in DECIDED] == [False, False]  # (libwebp 1.2.2 builds unused groups' codes too)


def test_reach(vp8g):
    """The accepted cases reach every item of the list the cases were written from (features the writer records
    while it writes), the refusals are each the neighbour of one of them, and what the parser reports of the cases
    empties the "uncovered" lists of tests/golden/lossless.json."""
    feats = set().union(*(S.build(n).features for n in ACCEPTED))
    missing = S.required() - feats
    assert not missing, sorted(map(str, missing))
    for w in (1, 2, 8, 9, 17):  # 120 distinct plane codes per width
        assert len({c for f in feats if isinstance(f, tuple) and f[0] == "plane_code" and f[1] == w for c in [f[2]]}) == 120
    assert {"invalid_code_in_unused_group"} <= set().union(*(S.build(n).features for n in DECIDED))
    golden = json.loads((GOLDEN / "lossless.json").read_text())
    modes, pbits, cbits, stats = set(), set(), set(), set()
    for n in ACCEPTED:
        _, _, trs, st = decode(vp8g, S.build(n))
        stats |= {k for k, v in st.items() if v}
        for t in trs or ():
            if t["type"] == S.P:
                pbits.add(t["bits"])
                modes |= {int(m) for m in np.unique((t["data"] >> 8) & 15)}
            elif t["type"] == S.CC:
                cbits.add(t["bits"])
    u = golden["uncovered"]
    assert u["predictor_modes"] and u["predictor_bits"] and u["cross_color_bits"]  # (what the fixtures alone leave open)
    assert not set(u["predictor_modes"]) - modes and not set(u["predictor_bits"]) - pbits
    assert not set(u["cross_color_bits"]) - cbits and not set(u["stats"]) - stats
    assert modes == set(range(16)) and pbits == cbits == set(range(2, 10))
    assert stats >= set(S.CENSUS)


def test_expected_pictures_do_not_come_from_the_decoder():
    """The writer's own statements, on values small enough to check by hand."""
    assert S.DIST_MAP[4:10] == [(0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1)] and S.DIST_MAP[96] == (8, 0)
    assert [S.prefix_symbol(v) for v in (1, 4, 5, 6, 7, 9, 4096)] == [(0, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0), (6, 2, 0),
                                                                    (23, 10, 1023)]
    assert S.canonical({0: 2, 1: 1, 2: 3, 3: 3}) == {1: (0, 1), 0: (2, 2), 2: (6, 3), 3: (7, 3)}
    assert S.lengths_of([(16, 3), ("lit", 2), ("lit", 0), (16, 3), (17, 3)], 16) == {0: 8, 1: 8, 2: 8, 3: 2, 5: 2, 6: 2, 7: 2}
    assert S.lengths_of([(18, 11)], 10) is None
    b = S.Bits()
    b.put(1, 1), b.put(0b10, 2), b.put(0x1FF, 9)
    assert b.bytes() == bytes([0b11111101, 0b00001111]) and b.nbits == 12
    assert S.inv_subtract_green([0x80FF10F0]) == [0x800F1000]
    assert S.unfilter([1, 2, 3, 250, 5, 6], 3, 2, 3) == [1, 3, 6, 251, 2, 11]  # (gradient: clip(L + T - TL))


# ---- robustness: every case stream under the sanitizers, as a program of its own --------------------------------

def test_case_streams_under_sanitizers(tmp_path):
    """tools/lossless_san_main.c + the host sources built with -fsanitize=address,undefined and run as a child
    process over every case's file, the refusals included (an ALPH case's headerless stream behind a VP8L header
    of its size): whole, truncated and corrupted through webp_parse_any, vp8f_lossless_decode and
    vp8f_lossless_apply.  Exit 0, no report."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    host = ROOT / "webp-decoder_amd" / "host"
    exe = tmp_path / "lossless_san"
    srcs = [str(ROOT / "tools" / "lossless_san_main.c")] + [str(host / f) for f in ("webp_riff.c", "vp8_parse.c", "vp8_synth.c",
                                                                                  "vp8_scale.c", "vp8_alpha.c")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cc, "-std=c11", "-O2", "-g"] + san + ["-D_POSIX_C_SOURCE=200809L", "-o", str(exe)] + srcs + ["-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for n in S.NAMES:
        b = S.build(n)
        data = b.data
        if b.container == "alph":
            hdr = b"\x2f" + struct.pack("<I", (b.width - 1) | (b.height - 1) << 14)
            data = S.riff(S.chunk(b"VP8L", hdr + b.payload[1:]))
        (tmp_path / f"{n}.webp").write_bytes(data)
        files.append((len(data), str(tmp_path / f"{n}.webp")))
    files = [f for _, f in sorted(files, reverse=True)]
    groups = [files[k::8] for k in range(8)]
    procs = [subprocess.Popen([str(exe)] + g, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for g in groups]
    lines = 0
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0 and "ERROR" not in err and "runtime error" not in err, err[-2000:]
        lines += len(out.splitlines())
    assert lines == len(files)
