"""The host half of the scaled animation path: host_anim_scaled -- vp8f_anim_compose, then
vp8f_argb_scale of every canvas -- against libwebp's RGBA for the animations of tests/golden/anim/
(tests/golden/anim_scale.json: each canvas encoded losslessly and decoded by libwebp with its crop / scale options)."""
import errno
import hashlib
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ANIM = GOLDEN / "anim"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "anim_scale.json").read_text())


@pytest.fixture(scope="module")
def anim_doc():
    return json.loads((GOLDEN / "anim.json").read_text())["files"]


def opt_of(vp8g, c):
    return vp8g.scale_opt(crop=tuple(c["crop"]), scale=tuple(c["scale"]), expand=c["expand"])


def data_of(name: str) -> bytes:
    return (ANIM / f"{name}.webp").read_bytes()


def test_every_golden_case_equals_libwebps_rgba(vp8g, golden, anim_doc):
    kinds = set()
    for c in golden["cases"]:
        out, ts = vp8g.host_anim_scaled(data_of(c["file"]), opt_of(vp8g, c))
        assert list(out.shape[:0:-1]) == c["size"] and len(out) == len(c["rgba"]) == anim_doc[c["file"]]["nframes"], c
        for k, canvas in enumerate(out):
            assert hashlib.sha256(vp8g.argb_to_rgba(canvas).tobytes()).hexdigest() == c["rgba"][k], (c, k)
        assert ts == [f["timestamp"] for f in anim_doc[c["file"]]["frames"]]
        w, h = anim_doc[c["file"]]["canvas"]
        ww, wh = (c["crop"][2], c["crop"][3]) if any(c["crop"]) else (w, h)
        ow, oh = c["size"]
        kinds.add((any(c["crop"]), any(c["scale"]), (ow > ww) - (ow < ww), (oh > wh) - (oh < wh)))
    assert {c["file"] for c in golden["cases"]} == {"rules_a", "rules_b", "mixed", "canvas_1x1", "one_frame"}
    assert [anim_doc[n]["canvas"] for n in ("rules_a", "rules_b", "mixed", "canvas_1x1")] == [[20, 14], [20, 14], [64, 48], [1, 1]]
    assert anim_doc["one_frame"]["nframes"] == 1
    # a target equal to the canvas, shrink, crop plus shrink, crop only, expand both, each mixed pair, crop and equal target
    assert {(False, True, 0, 0), (False, True, -1, -1), (True, True, -1, -1), (True, False, 0, 0), (False, True, 1, 1),
            (False, True, -1, 1), (False, True, 1, -1), (True, True, 0, 0)} <= kinds
    # odd window origins, derived dimensions, a shrink by one and to 1 x 1 are among the cases
    assert any(c["crop"][0] & 1 and c["crop"][1] & 1 and any(c["scale"]) for c in golden["cases"])
    assert any(c["scale"][1] == 0 and c["scale"][0] for c in golden["cases"])
    assert any(c["size"] == [19, 13] for c in golden["cases"]) and any(c["size"] == [1, 1] and c["file"] == "mixed" for c in golden["cases"])


def test_target_equal_to_the_canvas_is_not_the_identity(vp8g, golden):
    """The premultiply round trip changes translucent pixels (and clears colour under alpha 0); a crop alone copies."""
    (cw, ch), frames, _ = vp8g.host_anim_frames(data_of("rules_a"))
    canvases, _ = vp8g.host_anim_compose(cw, ch, frames)
    same, _ = vp8g.host_anim_scaled(data_of("rules_a"), vp8g.scale_opt(scale=(cw, ch)))
    assert same.shape == canvases.shape and not np.array_equal(same, canvases)
    opaque = (canvases >> 24) == 255
    assert opaque.any() and np.array_equal(same[opaque], canvases[opaque])
    crop, _ = vp8g.host_anim_scaled(data_of("rules_a"), vp8g.scale_opt(crop=(1, 3, 16, 8)))
    assert np.array_equal(crop, canvases[:, 3:11, 1:17])
    ident, _ = vp8g.host_anim_scaled(data_of("rules_a"), vp8g.scale_opt())
    assert np.array_equal(ident, canvases)


def test_refusals_are_refused(vp8g, golden):
    assert len(golden["refusals"]) >= 2
    for c in golden["refusals"]:
        assert c["errno"] == "EINVAL"
        with pytest.raises(OSError) as ei:
            vp8g.host_anim_scaled(data_of(c["file"]), opt_of(vp8g, c))
        assert ei.value.errno == errno.EINVAL, c
    # a file that is no animation
    with pytest.raises(OSError):
        vp8g.host_anim_scaled(data_of("still_lossless"), vp8g.scale_opt(scale=(4, 4)))


def test_golden_is_reproducible():
    r = subprocess.run([sys.executable, str(GOLDEN / "make_anim_scale_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr[-2000:]
