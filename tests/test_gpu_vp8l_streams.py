"""The directed VP8L streams of tests/vp8l_streams.py on the device: what the parser makes of
them -- block bits 4..9, modes 0 / 13 / 14 / 15, colour tables of 1 and 256 entries, none of which a libwebp
encoding of the fixtures brings -- through vp8g_make_lossless_desc and the lossless kernel, through the batch
pipeline beside lossy files and refused streams, and the ALPH cases into RGBA tensors.  Bit equality throughout:
the writer's picture and libwebp's bytes (tests/golden/vp8l_kat.json)."""
import errno
import hashlib
import json

import numpy as np
import pytest
import torch

import vp8l_streams as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STILL = [n for n in S.NAMES if S.build(n).refuse is None and S.build(n).container != "alph"]
ALPH = [n for n in S.NAMES if S.build(n).refuse is None and S.build(n).container == "alph"]
REFUSED = [n for n in S.NAMES if S.build(n).refuse is not None]
LOSSY = ["ll_levels2_f3", "ll_disc_f2", "ll_tiles_f1"]  # tests/golden/alpha/, 67 x 45


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "vp8l_kat.json").read_text())


def lossy(name):
    return (GOLDEN / "alpha" / f"{name}.webp").read_bytes()


def test_parsed_images_through_the_kernel(vp8g):
    """Every accepted still's lossless_decode_host image in one launch of the kernel equals the writer's picture."""
    images = [vp8g.lossless_decode_host(S.build(n).payload) for n in STILL]
    bits = {(t["type"], t["bits"]) for im in images for t in im["transforms"] if t["type"] in (S.P, S.CC)}
    assert bits == {(t, b) for t in (S.P, S.CC) for b in range(2, 10)}
    assert {1, 256} <= {t["ncolors"] for im in images for t in im["transforms"] if t["type"] == S.CI}
    got = vp8g.gpu_lossless_argb(images)
    for n, g in zip(STILL, got):
        bad = np.argwhere(g != S.build(n).argb)
        assert bad.size == 0, (n, bad[:4].tolist())


def batches():
    """The stills grouped by size, each group interleaved with refused streams and lossy fixtures (which decode in
    the 67 x 45 group only)."""
    groups = {}
    for n in STILL:
        groups.setdefault((S.build(n).width, S.build(n).height), []).append(n)
    out, k = [], 0
    for size, names in sorted(groups.items()):
        order = []
        for n in names:
            order += [n, REFUSED[k % len(REFUSED)]] + ([LOSSY[k % 3]] if k % 2 == 0 or size == (67, 45) else [])
            k += 1
        out.append((size, order))
    return out


@pytest.mark.parametrize("device_m05", [False, True])
def test_mixed_batches_end_to_end(vp8g, kat, device_m05, monkeypatch):
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    seen, sizes = set(), set()
    for (w, h), order in batches():
        files = [lossy(n) if n in LOSSY else S.build(n).data for n in order]
        opt = vp8g.tensor_opt((w, h), "uint8", "NHWC")
        got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True, lossless=True)
        got = got.cpu().numpy()
        assert got.shape == (len(order), h, w, 4)
        old = None
        if (w, h) == (67, 45):
            old, st_old = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True)
            old = old.cpu().numpy()
        for i, n in enumerate(order):
            if n in LOSSY and old is not None:
                assert st[i] == 0 == st_old[i] and got[i].any() and np.array_equal(got[i], old[i]), (n, w, h)
            elif n in LOSSY or n in REFUSED:  # (a lossy file of another size, or a stream that does not decode)
                assert st[i] == errno.EINVAL and not got[i].any(), (n, w, h)
            else:
                assert st[i] == 0, (n, st[i])
                assert hashlib.sha256(got[i].tobytes()).hexdigest() == kat["cases"][n]["rgba"], n
                assert np.array_equal(got[i], vp8g.argb_to_rgba(S.build(n).argb)), n
                seen.add(n)
        sizes.add((w, h))
    assert seen == set(STILL) and (67, 45) in sizes and len(sizes) >= 20


def test_float16_nchw_end_to_end(vp8g):
    names = [n for n in STILL if (S.build(n).width, S.build(n).height) == (S.W0, S.H0)]
    assert len(names) >= 12
    files = [S.build(n).data for n in names]
    opt = vp8g.tensor_opt((S.W0, S.H0), "float16", "NCHW", mean=[0.5, 0.4, 0.3], std=[0.2, 0.3, 0.25], bgr=True)
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, alpha=True, lossless=True)
    got = got.cpu()
    for i, n in enumerate(names):
        want = vp8g.host_tensor_argb(S.build(n).argb, opt, 4)
        assert st[i] == 0 and torch.equal(got[i].view(torch.uint8), want.view(torch.uint8)), n


@pytest.mark.parametrize("device_m05", [False, True])
def test_alph_cases_into_rgba_tensors(vp8g, kat, device_m05, monkeypatch):
    """The ALPH cases as VP8X files around the VP8 chunk of a lossy fixture: the alpha channel is the writer's plane and
    libwebp's, the colour is that of the fixture itself."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    assert len(ALPH) == 6
    files = [lossy(S.ALPH_BASE)] + [S.build(n).data for n in ALPH]
    opt = vp8g.tensor_opt((S.ALPH_W, S.ALPH_H), "uint8", "NHWC")
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, opt, device_m05=device_m05, extended=True, alpha=True, lossless=True)
    got = got.cpu().numpy()
    assert st == [0] * len(files) and got[0, :, :, :3].any()
    for i, n in enumerate(ALPH, 1):
        assert np.array_equal(got[i, :, :, 3], S.build(n).alpha), n
        assert hashlib.sha256(got[i, :, :, 3].tobytes()).hexdigest() == kat["cases"][n]["alpha"], n
        assert np.array_equal(got[i, :, :, :3], got[0, :, :, :3]), n
