"""CPU tests of the directed VP8 streams (tests/streams.py): the host entropy front end
(host/vp8_parse.c dense and packed sinks, vp8f_token_header) on streams no encoder of the corpus
writes -- loop-filter deltas, delta-mode segments with negative and clamping values, all five
quantiser deltas, segmentation without map / without data, colour-space, clamping and scale bits,
non-skipped all-EOB macroblocks, arbitrary probability tables, +-2114, 1024 macroblock columns / rows,
native 2 / 4 / 8 partitions at every start offset modulo 4, partitions declared short or empty.

  * round trip: vp8f_decode_memory(write(F)) == F byte for byte (header up to the pointers, every
    array), the packed decode expands to the same arrays, the native multi-partition streams decode
    (opt-in) to their twin's arrays and fail without the flag;
  * against the reference's own m05 where it is built: same arrays, byte-equal Vp8CoeffStats (overread
    fields of the cut streams included); it rejects the multi-partition streams;
  * tests/golden/stream_kat.json (tests/golden/make_stream_kat.py): stream sha256, coefficient hash,
    and the oracle's reconstruction of the decoded frame against the reference's `-yuv` / `-yuvf`;
  * the writer's census proves what the table reaches;
  * vp8f_token_header on every case;
  * oracle/front_san (`make -C oracle san`): the front end under ASan + UBSan on the streams and on
    prefixes / bit flips of them, in a process of its own.

Census of the 88 one-partition cases (python -m pytest tests/test_streams.py -s -k census prints it):
  tokens   EOB 148670  ZERO 345717  ONE 44513  TWO 44954  THREE 45403  FOUR 45379
           CAT1 13620  CAT2 5616  CAT3 10963  CAT4 21454  CAT5 43245  CAT6 42244   largest |c| 2114
  leaves   ymode DC 2102 V 1102 H 822 TM 290 B 2235; uv_mode 2675 1933 1203 740; every sub-block mode
           3381..3679; segment ids 840 817 746 822; skip bits 6014 x 0, 197 x 1; 49 non-skipped all-EOB MBs
  native multi-partition streams start their partitions at every offset modulo 4, for 2, 4 and 8 alike.
"""
import ctypes as C
import hashlib
import json
import struct
import subprocess

import numpy as np
import pytest

import directed as D
import streams as S
from conftest import GOLDEN, ROOT

needs_ref = pytest.mark.skipif("not __import__('vp8g').ref_available()", reason="reference build absent")
SINGLE = [c["name"] for c in S.single_partition()]
MULTI = [c["name"] for c in S.multi_partition()]
SIDE = ("ymode", "uv_mode", "segment_id", "has_coeff", "bmode", "skip_coeff")
COEFF = ("coeff_y", "coeff_u", "coeff_v", "coeff_y2")
HDR_FIELDS = [n for n, _ in __import__("vp8g").Vp8DecodedFrame._fields_
              if not n.startswith(("segment_id", "skip", "has_", "ymode", "uv_mode", "bmode", "coeff", "stats"))]


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "stream_kat.json").read_text())["cases"]


def arrays_equal(a, b, names):
    return [n for n in names if not np.array_equal(a(n), b(n))]


def test_table_shape():
    """Every case once with one partition; every size, header recipe (with both filters), coefficient
    kind, probability table and skip variant present; the large sizes on profile 0 only."""
    singles = S.single_partition()
    assert {c["size"] for c in singles} == set(S.SIZES) == {c["size"] for c in S.multi_partition()}
    for h in S.HEADERS:
        assert {c["simple"] for c in singles if c["header"] == h} == {0, 1}, h
    lf = [S.build(c).frame.frame for c in singles if c["frame"].startswith("lf")]
    assert len(lf) == 16 and {h.lf_use_simple for h in lf} == {0, 1}
    assert {c["frame"] for c in singles} >= set(S.COEFF_KINDS) | {"wrap", "mixed", "skip", "bpred_all", "bpred_none"}
    assert {c["probs"] for c in singles} == set(S.PROBS) and {c["skip"] for c in singles} == set(S.SKIPS)
    assert all(c["frame"] in ("p0", "p0c") for c in S.CASES if c["size"] in S.LARGE)
    assert {c["log2k"] for c in S.CASES} == {0, 1, 2, 3}
    for c in S.multi_partition():
        assert S.BY_NAME[c["twin"]]["log2k"] == 0
    cuts = {c["cut"] for c in singles if c["cut"]}
    assert cuts == {(1,), (2,), (3,), (S.CUT_ALL,)}


@pytest.mark.parametrize("name", SINGLE)
def test_round_trip(vp8g, name):
    b = S.build(name)
    g = S.decode(b.data)
    assert g is not None
    if not S.is_cut(b.case):
        assert D.same(g, b.frame), arrays_equal(g.array, b.frame.array, [n for n, _, _ in vp8g.FRAME_ARRAYS])
    pf = vp8g.PackedFrame(b.data, hash_coeffs=True)
    dense = vp8g.unpack_coeffs(pf)
    assert not arrays_equal(g.array, dense.__getitem__, COEFF)
    assert not arrays_equal(g.array, pf.side, SIDE)
    hdr = vp8g.Vp8DecodedFrame.segment_id.offset
    assert bytes(pf.p.kf) == bytes(g.kf) and bytes(pf.p.f)[:hdr] == bytes(g.frame)[:hdr]
    assert bytes(pf.p.f.stats) == bytes(g.frame.stats)


@pytest.mark.parametrize("name", MULTI)
def test_multi_partition_round_trip(vp8g, name):
    b = S.build(name)
    twin = S.build(b.case["twin"])
    assert S.decode(b.data) is None  # the reference-equivalent front end: ENOTSUP
    with pytest.raises(ValueError):
        vp8g.PackedFrame(b.data)
    with pytest.raises(ValueError):
        vp8g.token_header(b.data)
    pf = vp8g.PackedFrame(b.data, hash_coeffs=True, multi_partition=True)
    dense = vp8g.unpack_coeffs(pf)
    for f in (b.frame, twin.frame):
        assert not arrays_equal(f.array, dense.__getitem__, COEFF)
        assert not arrays_equal(f.array, pf.side, SIDE)
    g = S.decode(twin.data)
    hdr = vp8g.Vp8DecodedFrame.segment_id.offset
    assert bytes(pf.p.f)[:hdr] == bytes(g.frame)[:hdr] == bytes(b.frame.frame)[:hdr]
    assert pf.p.f.stats.coeff_hash_fnv1a64 == g.frame.stats.coeff_hash_fnv1a64


@pytest.mark.parametrize("name", [c["name"] for c in S.MP_CUT_CASES])
def test_multi_partition_cut_in_the_middle(vp8g, name):
    """Partitions in the middle declared short or empty: the host decodes them (each partition reads zeros
    past its own end), the table the job carries is the writer's, and the result differs from the intact
    stream's (so the cut matters) while everything partition 0 decides stays."""
    b = S.build(name)
    cs, k = b.census, 1 << b.case["log2k"]
    assert any(cs.part_off[p] == cs.part_end[p] for p in range(k - 1))  # an empty partition before the last
    pf = vp8g.PackedFrame(b.data, hash_coeffs=True, multi_partition=True)
    _, _, tf, _, size = vp8g.token_header(b.data, multi_partition=True)
    assert [tf.part_off[p] for p in range(k)] == [cs.part_off[p] for p in range(k)]
    assert [tf.part_end[p] for p in range(k)] == [cs.part_end[p] for p in range(k)] and cs.part_end[k - 1] == size
    whole = vp8g.PackedFrame(S.build(name.rsplit("_", 1)[0]).data, multi_partition=True)
    for n in ("ymode", "uv_mode", "segment_id", "bmode", "skip_coeff"):
        assert np.array_equal(pf.side(n), whole.side(n)), n
    assert not np.array_equal(pf.masks(), whole.masks())


def test_writer_refuses_what_the_format_cannot_hold(vp8g):
    """EINVAL: |coefficient| > 2114, a mode out of range (profile 2 as generated), a delta beyond its width."""
    prm = S._params(S.BY_NAME["c_p0_33x50"], None, np.random.default_rng(0))

    def refused(f):
        with pytest.raises(OSError) as e:
            S.write(f, prm)
        return e.value.errno == 22

    f = vp8g.synth_frame(33, 50, 3, 0)
    S.write(f, prm)
    f.array("coeff_u")[5] = 2115
    assert refused(f)
    f.array("coeff_u")[5] = -2114
    S.write(f, prm)
    for name, bad in (("ymode", 5), ("uv_mode", 4)):
        keep = int(f.array(name)[2])
        f.array(name)[2] = bad
        assert refused(f)
        f.array(name)[2] = keep
    f.array("ymode")[0], f.array("bmode")[3] = 4, 10
    assert refused(f)
    f.array("bmode")[3] = 9
    f.frame.y2_ac_delta_q = 16
    assert refused(f)
    f.frame.y2_ac_delta_q = -15
    S.write(f, prm)
    raw = vp8g.synth_frame(100, 70, 4, 2)  # profile 2: ymode 5..7, uv_mode 4..7, bmode 10..15
    assert (raw.array("ymode") > 4).any() and refused(raw)


@needs_ref
@pytest.mark.parametrize("name", SINGLE)
def test_host_front_end_equals_reference_m05(vp8g, name, tmp_path):
    b = S.build(name)
    path = tmp_path / "s.webp"
    path.write_bytes(b.data)
    kf, rf = vp8g.Vp8KeyFrameHeader(), vp8g.Vp8DecodedFrame()
    assert vp8g.ref_lib().ref_decode_frame(str(path).encode(), C.byref(kf), C.byref(rf)) == 0
    try:
        g = S.decode(b.data)
        hdr = vp8g.Vp8DecodedFrame.segment_id.offset
        assert bytes(kf) == bytes(g.kf) and bytes(rf)[:hdr] == bytes(g.frame)[:hdr]
        for n, dt, per in vp8g.FRAME_ARRAYS:
            r = np.ctypeslib.as_array(getattr(rf, n), shape=(g.mb_total * per,))
            assert np.array_equal(r, g.array(n)), n
        st = g.frame.stats
        assert bytes(rf.stats) == bytes(st)
    finally:
        vp8g.ref_lib().ref_free_frame(C.byref(rf))


def test_cut_streams_overread():
    """The cut variants do what they are for: the token partition is read past its declared end (and the
    first position is located), in at least one stream per cut length."""
    for cut in (1, 2, 3, S.CUT_ALL):
        hits = 0
        for c in S.single_partition():
            if S.is_cut(c) and c["cut"] == (cut,):
                g = S.decode(S.build(c).data)  # (kept alive: freeing the frame zeroes its statistics)
                st = g.frame.stats
                hits += bool(st.token_overread and st.token_overread_bytes and st.token_overread_mb_index != 0xFFFFFFFF)
        assert hits, cut


@needs_ref
def test_reference_rejects_multi_partition(vp8g, tmp_path):
    for name in MULTI:
        path = tmp_path / "m.webp"
        path.write_bytes(S.build(name).data)
        kf, rf = vp8g.Vp8KeyFrameHeader(), vp8g.Vp8DecodedFrame()
        assert vp8g.ref_lib().ref_decode_frame(str(path).encode(), C.byref(kf), C.byref(rf)) == 4, name


def test_streams_are_deterministic(kat):
    assert list(kat) == [c["name"] for c in S.CASES]
    for c in S.CASES:
        b = S.build(c)
        assert (sha(b.data), len(b.data)) == (kat[c["name"]]["sha256"], kat[c["name"]]["length"]), c["name"]


@pytest.mark.parametrize("name", SINGLE + MULTI)
def test_reconstruction_equals_golden(vp8g, kat, name):
    """The oracle on what the front end decoded (multi-partition: the frame the packed decode was shown
    to equal) against the reference's -yuv / -yuvf on the stream; the coefficient hash against its m05's."""
    b = S.build(name)
    if b.case["log2k"]:
        f = b.frame
        pf = vp8g.PackedFrame(b.data, hash_coeffs=True, multi_partition=True)
        chash = pf.p.f.stats.coeff_hash_fnv1a64
    else:
        f = S.decode(b.data)
        chash = f.frame.stats.coeff_hash_fnv1a64
    ent = kat[name]
    assert f"{chash:016x}" == ent["coeff_hash"]
    assert sha(vp8g.oracle_reconstruct(f, False)) == ent["yuv_sha256"]
    assert sha(vp8g.oracle_reconstruct(f, True)) == ent["yuvf_sha256"]


@pytest.mark.parametrize("name", SINGLE)
def test_frame_desc_tables(vp8g, name):
    """vp8g_make_frame_desc (host code of libvp8g.so: fill_dequant / fill_loopfilter of csrc/vp8g_shim.hip)
    on the decoded header against the RFC restatement streams.expected_desc_tables: delta and absolute
    segments, sums that clamp at both ends, every quantiser delta, loop-filter deltas, sharpness."""
    g = S.decode(S.build(name).data)
    h = g.frame
    d = vp8g.make_desc(g, True, 0, 0)
    dq, lf = S.expected_desc_tables(h)
    assert np.array_equal(np.array([list(r) for r in d.dq]), dq)
    assert np.array_equal(np.array([[list(x) for x in r] for r in d.lf]), lf)
    # (the filter flag is decided over all four segments' levels, used or not)
    assert bool(d.flags & vp8g.VP8G_F_LOOPFILTER) == bool(lf[:, :, 0].any())
    if d.flags & vp8g.VP8G_F_LOOPFILTER:
        assert bool(d.flags & vp8g.VP8G_F_SIMPLE) == bool(h.lf_use_simple)


def test_golden_libwebp_flags(kat):
    """Generation enforced it; the committed file must still say it: libwebp agrees on every profile-0
    case that is not cut, but for the cases the notes name."""
    doc = json.loads((GOLDEN / "stream_kat.json").read_text())
    noted = {n.split(":")[0] for n in doc["notes"]}
    for c in S.CASES:
        if S.base_profile0(c) and not c["cut"] and c["name"] not in noted:
            assert kat[c["name"]]["libwebp_same"] is True, c["name"]
    assert noted and all(kat[n]["libwebp_same"] is False for n in noted)


def test_census_reaches_everything():
    tok = np.zeros(12, np.uint64)
    leaves = {k: 0 for k in ("ymode", "uv_mode", "bmode", "segment")}
    leaves = {k: np.zeros(n, np.uint64) for k, n in (("ymode", 5), ("uv_mode", 4), ("bmode", 10), ("segment", 4))}
    skip_bits = np.zeros(2, np.uint64)
    maxmag, updates, mod4, mod4_by_k = 0, 0, set(), {2: set(), 4: set(), 8: set()}
    signs = {}
    all_eob_mbs = 0
    for c in S.CASES:
        b = S.build(c)
        cs = b.census
        if c["log2k"] == 0:  # (a multi-partition case repeats its twin's tokens)
            tok += np.array(list(cs.tokens), np.uint64)
            for k in leaves:
                leaves[k] += np.array(list(getattr(cs, k)), np.uint64)
            skip_bits += np.array(list(cs.skip_bits), np.uint64)
            maxmag = max(maxmag, int(cs.max_magnitude))
            updates = max(updates, int(cs.prob_updates))
            f = b.frame
            all_eob_mbs += int(((f.array("skip_coeff") == 0) & (f.array("has_coeff") == 0)).sum())
            h = f.frame
            for n in ("y1_dc_delta_q", "y2_dc_delta_q", "y2_ac_delta_q", "uv_dc_delta_q", "uv_ac_delta_q"):
                signs.setdefault(n, set()).add(int(np.sign(getattr(h, n))))
            for n in ("seg_quant_idx", "seg_lf_level", "lf_ref_delta", "lf_mode_delta"):
                for i in range(4):
                    signs.setdefault(f"{n}[{i}]", set()).add(int(np.sign(getattr(h, n)[i])))
        else:
            assert cs.nparts == 1 << c["log2k"]
            offs = {int(cs.part_off_mod4[p]) for p in range(cs.nparts)}
            assert offs == {int(cs.part_off[p]) & 3 for p in range(cs.nparts)}
            mod4 |= offs
            mod4_by_k[cs.nparts] |= offs
    print("tokens", dict(zip(S.TOKENS, tok.tolist())), "max |c|", maxmag)
    print("leaves", {k: v.tolist() for k, v in leaves.items()}, "skip bits", skip_bits.tolist(), "all-EOB MBs", all_eob_mbs)
    print("partition start offsets mod 4", sorted(mod4), {k: sorted(v) for k, v in mod4_by_k.items()})
    assert (tok > 0).all(), dict(zip(S.TOKENS, tok.tolist()))
    # DCT_CAT6 with all 11 extra bits set (the top one, 1024, among them): the format's largest magnitude,
    # 67 + 2047 (no stream can hold the 2048 + 67 a first reading of the token table suggests)
    assert maxmag == S.MAX_MAGNITUDE == 2114
    for k, v in leaves.items():
        assert (v > 0).all(), (k, v.tolist())
    assert (skip_bits > 0).all() and all_eob_mbs > 0
    assert updates == 1056  # a table with every entry replaced
    assert mod4 == {0, 1, 2, 3}
    for n, s in signs.items():
        assert s == {-1, 0, 1}, (n, s)
    hs = [S.build(c).frame.frame for c in S.single_partition()]
    assert {h.lf_delta_enabled for h in hs} == {0, 1} and {h.segmentation_abs for h in hs} == {0, 1}
    assert {(h.q_index, h.y1_dc_delta_q) for h in hs} >= {(0, -15), (0, 15), (127, -15), (127, 15)}
    ps = [S.build(c).params for c in S.single_partition()]
    assert {(p.color_space, p.clamp_type) for p in ps} == {(0, 0), (1, 1)}
    assert {(p.x_scale, p.y_scale) for p in ps} >= {(0, 0), (1, 2), (2, 1)}


@pytest.mark.parametrize("name", SINGLE + MULTI)
def test_token_header(vp8g, name):
    b = S.build(name)
    multi = b.case["log2k"] > 0
    kf, hdr, tf, off, size = vp8g.token_header(b.data, multi_partition=multi)
    assert off == 20 and size == struct.unpack("<I", b.data[16:20])[0] == b.census.payload_size
    want_kf, want = (b.frame.kf, b.frame.frame)
    if not multi:
        g = S.decode(b.data)
        want_kf, want = g.kf, g.frame
    assert bytes(kf) == bytes(want_kf)
    for n in HDR_FIELDS:
        x, y = getattr(hdr, n), getattr(want, n)
        assert (list(x) if hasattr(x, "__len__") else x) == (list(y) if hasattr(y, "__len__") else y), n
    cs = b.census
    k = 1 << b.case["log2k"]
    assert tf.nparts == k == cs.nparts
    assert [tf.part_off[p] for p in range(k)] == [cs.part_off[p] for p in range(k)]
    assert [tf.part_end[p] for p in range(k)] == [cs.part_end[p] for p in range(k)]
    assert tf.p0_end == 10 + kf.first_partition_len == 10 + cs.part0_size
    assert tf.tok_off == tf.part_off[0] == tf.p0_end + 3 * (k - 1) and tf.tok_end == tf.part_end[0]
    assert tf.part_end[k - 1] == size
    assert 128 <= tf.b_range <= 255 and 0 <= tf.b_bits <= 56 and 10 < tf.b_next <= tf.p0_end
    prm = b.params
    seg = want.segmentation_enabled
    assert (tf.seg_enabled, tf.use_skip) == (seg, prm.use_skip)
    assert tf.seg_map_update == (seg and prm.update_mb_segmentation_map)
    assert tf.skip_prob == (prm.skip_prob if prm.use_skip else 0)
    assert list(tf.seg_probs) == (list(prm.seg_tree_probs) if tf.seg_map_update else [255] * 3)
    probs = np.frombuffer(bytes(tf.coeff_probs), np.uint8).reshape(4, 8, 3, 12)
    assert (probs[..., 11] == 0).all()
    assert np.array_equal(probs[..., :11].reshape(-1), np.frombuffer(bytes(prm.coeff_probs), np.uint8))


def test_front_end_under_sanitizers(tmp_path):
    """oracle/front_san (make -C oracle san; ASan + UBSan, a program of its own): the three entry points
    on every stream, its prefixes and seeded bit flips.  CPU only."""
    import torch
    exe = ROOT / "oracle" / "front_san"
    if not exe.exists():
        pytest.skip("oracle/front_san not built (make -C oracle san)")
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    for c in S.CASES:
        if c["size"] not in S.LARGE or c["name"] in ("big_16383x16_plain", "big_16x16383_plain_mp8"):  # (two large ones: time)
            (tmp_path / (c["name"] + ".webp")).write_bytes(S.build(c).data)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "front_san: OK" in r.stdout
