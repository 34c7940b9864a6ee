"""GPU tests (MI355X) of the directed VP8 streams (tests/streams.py): the device m05
(csrc/vp8g_m05.hip), the host half that feeds it (vp8f_token_header) and the batch pipeline with its
packed expand step (csrc/vp8g_pipeline.hip) on streams no encoder of the corpus writes -- see
tests/test_streams.py for what the table holds and the CPU proof that it reaches it.

Bars: all nine m05 arrays of the device equal the host front end's (which test_streams.py pins to the
frame the stream was written from and to the reference's m05), cut streams included; the end-to-end
batch in every mode gives status 0 and the reference's `-yuv` / `-yuvf` bytes (sha256 in
tests/golden/stream_kat.json) for every case, the 1024-column and 1024-row frames among them.
Only intact directed streams and their cut variants come here; mutated streams go to the host parser
alone (test_streams.py).
"""
import hashlib
import json
import subprocess

import numpy as np
import pytest

import streams as S
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NAMES = ["coeff_y", "coeff_u", "coeff_v", "coeff_y2", "ymode", "uv_mode", "segment_id", "has_coeff", "bmode"]
DECODER = ROOT / "webp-decoder_amd" / "bin" / "decoder"


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "stream_kat.json").read_text())["cases"]


@pytest.fixture(scope="module")
def everything():
    """(names, streams) of the whole table, single- and multi-partition cases interleaved so that
    neighbours in a batch are unlike frames."""
    a, b = S.single_partition(), S.multi_partition()
    order = []
    while a or b:
        order += a[:3] + b[:1]
        a, b = a[3:], b[1:]
    return [c["name"] for c in order], [S.build(c).data for c in order]


def host_arrays(vp8g, case):
    """The host front end's m05 arrays of a case (multi-partition: the packed decode, expanded)."""
    b = S.build(case)
    if case["log2k"] == 0:
        g = S.decode(b.data)
        return {k: g.array(k).copy() for k in NAMES}
    pf = vp8g.PackedFrame(b.data, multi_partition=True)
    out = vp8g.unpack_coeffs(pf)
    out.update({k: pf.side(k) for k in NAMES[4:]})
    return out


def check_m05(vp8g, cases, multi):
    got = vp8g.gpu_m05([S.build(c).data for c in cases], multi_partition=multi)
    for c, g in zip(cases, got):
        want = host_arrays(vp8g, c)
        for k in NAMES:
            if not np.array_equal(g[k], want[k]):
                bad = np.flatnonzero(g[k] != want[k])
                raise AssertionError(f"{c['name']}: {k} differs at {bad.size} entries, first {bad[:4]}")


def test_m05_arrays_single_partition(vp8g):
    """One launch over every one-partition case, the cut variants among them."""
    check_m05(vp8g, S.single_partition(), False)


def test_m05_arrays_native_multi_partition(vp8g):
    """One token wave per partition (2 / 4 / 8), every start offset modulo 4, fewer rows than partitions
    (1024 x 1) and a one-column row wavefront (1 x 1024)."""
    check_m05(vp8g, S.multi_partition(), True)


def test_multi_partition_cut_in_the_middle(vp8g):
    """Partitions before the last declared short or empty: each token wave reads zeros past its own
    partition's end, never the next partition's bytes -- m05 arrays equal to the host's, and the pipeline
    the same in both modes."""
    check_m05(vp8g, S.MP_CUT_CASES, True)
    files = [S.build(c).data for c in S.MP_CUT_CASES]
    a, sa = vp8g.gpu_decode_webp_batch(files, True, 4, device_m05=False, multi_partition=True)
    b, sb = vp8g.gpu_decode_webp_batch(files, True, 4, device_m05=True, multi_partition=True)
    assert sa == sb == [0] * len(files)
    assert a == b
    for c, o in zip(S.MP_CUT_CASES, a):  # the pixels are the oracle's on the host's decode of the cut stream
        pf = vp8g.PackedFrame(S.build(c).data, multi_partition=True)
        f = S.fresh(c).frame  # (header and modes are partition 0's, which the cuts leave alone)
        for n, v in vp8g.unpack_coeffs(pf).items():
            f.array(n)[:] = v
        f.array("has_coeff")[:] = pf.side("has_coeff")
        assert o == vp8g.oracle_reconstruct(f, True), c["name"]


def check_batch(vp8g, kat, names, files, filtered, device_m05):
    outs, st = vp8g.gpu_decode_webp_batch(files, filtered, 8, device_m05=device_m05, multi_partition=True)
    assert st == [0] * len(names), [(n, s) for n, s in zip(names, st) if s]
    key = "yuvf_sha256" if filtered else "yuv_sha256"
    bad = [n for n, o in zip(names, outs) if sha(o) != kat[n][key]]
    assert not bad, f"{len(bad)} mismatches, e.g. {bad[:8]}"


@pytest.mark.parametrize("device_m05", [False, True], ids=["host_m05", "device_m05"])
@pytest.mark.parametrize("filtered", [False, True], ids=["yuv", "yuvf"])
def test_pipeline_mixed_batch(vp8g, kat, everything, filtered, device_m05):
    check_batch(vp8g, kat, *everything, filtered, device_m05)


def test_pipeline_mixed_batch_pure_device(vp8g, kat, everything, monkeypatch):
    """VP8G_HYBRID=0: no frame of the device-m05 batch goes to the host threads."""
    monkeypatch.setenv("VP8G_HYBRID", "0")
    check_batch(vp8g, kat, *everything, True, True)


@pytest.mark.parametrize("device_m05", [False, True], ids=["host_m05", "device_m05"])
def test_pipeline_small_chunks(vp8g, kat, everything, monkeypatch, device_m05):
    """Chunks of 5 frames: the two device slots alternate across unlike frames."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "5")
    check_batch(vp8g, kat, *everything, True, device_m05)


def test_device_and_host_m05_agree_on_cut_streams(vp8g, kat):
    cases = [c for c in S.CASES if c["cut"]]
    assert len(cases) >= 9
    files = [S.build(c).data for c in cases]
    for filtered in (False, True):
        a, sa = vp8g.gpu_decode_webp_batch(files, filtered, 4, device_m05=False, multi_partition=True)
        b, sb = vp8g.gpu_decode_webp_batch(files, filtered, 4, device_m05=True, multi_partition=True)
        assert sa == sb == [0] * len(cases)
        assert a == b
        key = "yuvf_sha256" if filtered else "yuv_sha256"
        assert [sha(o) for o in a] == [kat[c["name"]][key] for c in cases]


@pytest.mark.parametrize("name", ["h_segdelta_n", "c_wrap_33x50"])
def test_decoder_cli(kat, name, tmp_path):
    """bin/decoder -yuvf on a delta-segment stream and on the +-2114 one."""
    src, out = tmp_path / "s.webp", tmp_path / "s.i420"
    src.write_bytes(S.build(name).data)
    r = subprocess.run([str(DECODER), "-yuvf", str(src), str(out)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sha(out.read_bytes()) == kat[name]["yuvf_sha256"]
