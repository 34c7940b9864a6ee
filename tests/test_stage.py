"""The staging layer of the device-call wrappers (webp-decoder_amd/vp8g_stage.py, the stage_* functions of vp8g.py),
without a GPU.

tests/golden/stage_layout.json holds a list of small cases per wrapper and, for each, what the wrapper's staging produced
before the layer existed: digests of the descriptors and of the source bytes, the sizes of the destination and work
buffers, the outputs' (offset, nbytes).  The stagers are held to it byte for byte -- the misalignment of every source and
the guard geometry are what the GPU tests of the sink kernels run at.  Then the properties themselves, from the staged
objects, and Guarded.check on buffers with one flipped byte."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import GOLDEN

LAYOUT = json.loads((GOLDEN / "stage_layout.json").read_text())
CASES = [(w, k) for w, cases in LAYOUT.items() for k in range(len(cases))]
NCOLORS = {3: 2, 2: 4, 1: 11, 0: 40}


def words(seed, n):
    """n uint32 of a fixed sequence (written out, not drawn from a generator: the record digests these bytes)."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(7919 * seed + 1)
    return ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(24) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def picture(seed, w, h):
    return words(seed, w * h).reshape(h, w)


def scale_opt(vp8g, o):
    return vp8g.scale_opt(crop=o.get("crop"), scale=o.get("scale"), expand=o.get("expand", False))


def lossless_image(vp8g, seed, w, h, types, bits, pack):
    """tests/test_gpu_lossless.py's synth with the fixed sequence: transforms `types` (0 predictor, 1 cross colour,
    2 subtract green, 3 colour index) in stream order."""
    trs, xs = [], w
    for k, t in enumerate(types):
        r = (1 << bits) - 1
        shape = ((h + r) >> bits, (xs + r) >> bits)
        if t in (vp8g.L_PREDICTOR, vp8g.L_CROSS_COLOR):
            trs.append({"type": t, "bits": bits, "data": words(seed + k + 1, shape[0] * shape[1]).reshape(shape)})
        elif t == vp8g.L_SUBTRACT_GREEN:
            trs.append({"type": t, "bits": 0})
        else:
            trs.append({"type": t, "bits": pack, "data": words(seed + k + 1, NCOLORS[pack])})
            xs = (xs + (1 << pack) - 1) >> pack
    return vp8g.lossless_image(words(seed, h * xs).reshape(h, xs), trs, width=w)


def arguments(vp8g, wrapper, c):
    """(args, kwargs) of stage_<wrapper> (and of gpu_<wrapper>) for one case of the list."""
    if wrapper == "alpha_unfilter":
        planes = [picture(i, w, h).astype(np.uint8) for i, (w, h) in enumerate(c["planes"])]
        return (planes, c["filters"]), {k: c[k] for k in ("src_pad", "guard") if k in c}
    if wrapper == "scale_planes":
        planes = [picture(i, w, h).astype(np.uint8) for i, (w, h) in enumerate(c["planes"])]
        return (planes, [scale_opt(vp8g, o) for o in c["opts"]]), {}
    kw = {k: c[k] for k in ("src_shift", "guard") if k in c}
    if wrapper == "lossless_argb":
        return ([lossless_image(vp8g, 10 * i, *im) for i, im in enumerate(c["images"])],), kw
    if wrapper == "anim_compose":
        anims = [(cw, ch, [{"argb": picture(10 * i + k, w, h), "x": x, "y": y, "blend": b, "dispose": d, "has_alpha": a}
                           for k, (x, y, w, h, b, d, a) in enumerate(frames)]) for i, (cw, ch, frames) in enumerate(c["anims"])]
        return (anims, vp8g.tensor_opt((1, 1), c["dtype"], c["layout"]), c["channels"]), kw
    pics = [picture(i, w, h) for i, (w, h) in enumerate(c["pics"])]
    opts = [scale_opt(vp8g, o) for o in c["opts"]]
    if wrapper == "scale_argb":
        return (pics, opts), kw
    assert wrapper == "scale_argb_tensor"
    return (pics, opts, vp8g.tensor_opt((1, 1), c["dtype"], c["layout"]), c["channels"]), kw


def digest(vp8g, b):
    return f"{vp8g.fnv1a64(bytes(b)):016x}"


def record(vp8g, descs, src, dst_size, outputs, work_size=None, work=None):
    """What stage_layout.json holds of one staging.  A descriptor's host pointer (Vp8gAnimDesc.h_frames: where the
    records happen to sit in this process) is not part of it."""
    descs = type(descs).from_buffer_copy(descs)
    for d in descs:
        if hasattr(d, "h_frames"):
            d.h_frames = None
    r = {"descs": digest(vp8g, descs), "src": digest(vp8g, src), "dst_size": int(dst_size), "outputs": [[int(o), int(n)] for o, n in outputs]}
    if work_size is not None:
        r.update(work_size=int(work_size), work=[[int(o), int(n)] for o, n in work])
    return r


def staged(vp8g, wrapper, k):
    args, kw = arguments(vp8g, wrapper, LAYOUT[wrapper][k])
    return getattr(vp8g, f"stage_{wrapper}")(*args, **kw)


def test_the_list_has_what_every_wrapper_needs():
    assert set(LAYOUT) == {"alpha_unfilter", "scale_planes", "lossless_argb", "scale_argb", "scale_argb_tensor", "anim_compose"}
    for wrapper, cases in LAYOUT.items():
        assert len(cases) >= 4, wrapper
        sizes = [tuple(s[:2]) for c in cases for s in c.get("planes", []) + c.get("pics", []) + c.get("images", []) + c.get("anims", [])]
        assert (1, 1) in sizes and len(set(sizes)) >= 3, wrapper
        if wrapper not in ("alpha_unfilter", "scale_planes"):
            assert {c["src_shift"] for c in cases if "src_shift" in c} == {0, 1, 2, 3}, wrapper
            assert any("src_shift" not in c and "guard" not in c for c in cases), wrapper  # the defaults
    alpha = LAYOUT["alpha_unfilter"]
    assert {c.get("src_pad", 0) for c in alpha} >= {0, 3} and {c.get("guard", 0) for c in alpha} >= {0, 3, 5}
    assert any(3 in im[2] for c in LAYOUT["lossless_argb"] for im in c["images"])  # a colour table: a second put
    assert any(2 in im[2] for c in LAYOUT["lossless_argb"] for im in c["images"])  # subtract green: an empty data
    assert all(len({len(a[2]) for a in c["anims"]}) >= 2 for c in LAYOUT["anim_compose"])
    assert {c.get("guard", 64) for c in LAYOUT["scale_argb_tensor"]} >= {8, 64}


@pytest.mark.parametrize("wrapper,k", CASES)
def test_layout_is_the_recorded_one(vp8g, wrapper, k):
    s = staged(vp8g, wrapper, k)
    work = getattr(s, "work", None)
    got = record(vp8g, s.descs, s.src, s.dst.size, s.dst.regions, work and work.size, work and work.regions)
    assert got == LAYOUT[wrapper][k]["record"]


@pytest.mark.parametrize("wrapper,k", CASES)
def test_sources_sit_at_their_shift(vp8g, wrapper, k):
    c = LAYOUT[wrapper][k]
    s = staged(vp8g, wrapper, k)
    shift = c.get("src_shift", 1)
    want = {"alpha_unfilter": {(1, 0)}, "scale_planes": {(1, 0)}, "lossless_argb": {(4, shift)}, "scale_argb": {(16, 4 * shift)},
            "scale_argb_tensor": {(16, 4 * shift)}, "anim_compose": {(16, 4 * shift), (8, 0)}}[wrapper]
    assert {(a, sh) for _, a, sh in s.source.placed} == want
    for off, align, sh in s.source.placed:
        assert off % align == sh % align, (off, align, sh)
    tail = 0 if wrapper in ("alpha_unfilter", "scale_planes") else 16
    assert tail == 0 or (s.src[-tail:] == 0x5A).all()
    if wrapper == "anim_compose":  # the records lie between the pictures, completed
        recs = [(o, a) for o, a, _ in s.source.placed if a == 8]
        assert len(recs) == len(s.recs) and recs[0][0] < s.source.placed[-2][0]
        for (o, _), rec, d in zip(recs, s.recs, s.descs):
            assert bytes(s.src[o:o + C.sizeof(rec)]) == bytes(rec) and d.frames == o


@pytest.mark.parametrize("wrapper,k", CASES)
def test_outputs_are_disjoint_and_a_guard_apart(vp8g, wrapper, k):
    c = LAYOUT[wrapper][k]
    s = staged(vp8g, wrapper, k)
    default = 0 if wrapper in ("alpha_unfilter", "scale_planes") else 64
    for g in [s.dst] + ([s.work] if hasattr(s, "work") else []):
        assert g.guard == c.get("guard", default)
        end = g.head
        for o, n in g.regions:
            assert end + g.guard <= o < end + g.guard + g.round_to and o % g.round_to == g.guard % g.round_to
            end = o + n
        assert g.size - end >= (16 if wrapper == "scale_planes" else g.guard)


def test_source_pads_reserves_and_fills(vp8g):
    import vp8g_stage
    s = vp8g_stage.Source()
    assert s.put(np.array([1, 2, 3], np.uint8), 4, 1) == 1
    at = s.reserve(2, 8)
    assert at == 8 and s.put(np.array([0x01020304], np.uint32), 16, 8) == 24
    s.fill(at, b"\x07\x08")
    assert bytes(s.finish(tail=2)) == bytes([0x5A, 1, 2, 3, 0x5A, 0x5A, 0x5A, 0x5A, 7, 8] + [0x5A] * 14 + [4, 3, 2, 1, 0x5A, 0x5A])
    assert s.placed == [(1, 4, 1), (8, 8, 0), (24, 16, 8)]


def test_guard_check_sees_one_flipped_byte(vp8g):
    import vp8g_stage
    g = vp8g_stage.Guarded(16, 0xEE, round_to=16)
    a, b = g.add(5), g.add(20)
    assert (a, b, g.size) == (16, 48, 96) and g.regions == [(16, 5), (48, 20)]
    buf = np.full(g.size, 0xEE, np.uint8)
    g.check(buf, "test: bytes outside")
    buf[a:a + 5] = buf[b:b + 20] = 1  # the outputs themselves
    g.check(buf, "test: bytes outside")
    places = {"front guard": 0, "front guard's last byte": a - 1, "rounding slack behind an output": a + 5, "middle guard": b - 1,
              "slack behind the last output": b + 20, "last byte of the tail": g.size - 1}
    for why, at in places.items():
        bad = buf.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError, match="test: bytes outside were written"):
            g.check(bad, "test: bytes outside")
            pytest.fail(why)
    w = vp8g_stage.Guarded(8, 0xEE, head=32)
    r = w.add(10)
    assert (r, w.size) == (40, 58)
    buf = np.full(w.size, 0xEE, np.uint8)
    buf[:32] = 3  # the exempt head
    w.check(buf, "test: work")
    for at in (32, 39, 50, 57):  # just behind the head, in front of the region, behind it, the last byte
        bad = buf.copy()
        bad[at] = 0
        with pytest.raises(AssertionError):
            w.check(bad, "test: work")
            pytest.fail(str(at))
