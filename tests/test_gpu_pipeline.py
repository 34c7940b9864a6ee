"""GPU tests (MI355X) of the end-to-end batch path vp8g_decode_webp_batch (.webp bytes -> I420):
threaded host m05 into the packed wire format, chunked upload, device expansion, the fused
recon(+LF) kernel, D2H (webp-decoder_amd/csrc/vp8g_pipeline.hip).

Bar: bit-exact against the reference decoder's `-yuv` / `-yuvf` output (sha256 in
tests/golden/manifest.json) for every fixture, in one call, whatever the thread count and chunking.
"""
import hashlib

import pytest
import torch

from conftest import FIXTURES, GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.mark.parametrize("filtered,key", [(True, "yuvf_sha256"), (False, "yuv_sha256")])
def test_corpus_one_call(vp8g, manifest, filtered, key):
    rels = sorted(manifest["files"])
    outs, st = vp8g.gpu_decode_webp_batch([(FIXTURES / r).read_bytes() for r in rels], filtered, 16)
    assert st == [0] * len(rels)
    bad = [r for r, o in zip(rels, outs) if sha(o) != manifest["files"][r][key]]
    assert not bad, f"{len(bad)} mismatches, e.g. {bad[:8]}"


def test_thread_counts_and_chunking(vp8g, manifest):
    """Many 4K frames (several chunks, the two device slots alternate) with 1 and 16 threads."""
    rels = ["big/uhd_a_normal_seg4.webp", "big/uhd_b_simple_sharp3.webp", "big/uhd_c_normal_sharp6_seg1.webp",
            "big/k128_normal.webp", "big/fhd_normal_sharp5.webp"]
    files = [(FIXTURES / r).read_bytes() for r in rels]
    seq = [i % len(rels) for i in range(150)]
    for threads in (16, 1):
        use = seq if threads == 16 else seq[:12]
        outs, st = vp8g.gpu_decode_webp_batch([files[i] for i in use], True, threads)
        assert st == [0] * len(use)
        for i, o in zip(use, outs):
            assert sha(o) == manifest["files"][rels[i]]["yuvf_sha256"], (threads, rels[i])


def test_failed_frames_are_isolated(vp8g, manifest):
    good = ["webp/blockcheck2_16x16_000_000_000_255_255_255_q010.webp", "commons/penguin-q20.webp"]
    bad = [(ROOT / "tests" / "fixtures_err" / n).read_bytes() for n in ("empty_riff.webp", "truncated.webp")]
    files = [(FIXTURES / good[0]).read_bytes(), bad[0], b"", (FIXTURES / good[1]).read_bytes(), bad[1]]
    outs, st = vp8g.gpu_decode_webp_batch(files, True, 4)
    assert st[0] == 0 and st[3] == 0 and all(s != 0 for s in (st[1], st[2], st[4]))
    assert outs[1] is None and outs[2] is None and outs[4] is None
    assert sha(outs[0]) == manifest["files"][good[0]]["yuvf_sha256"]
    assert sha(outs[3]) == manifest["files"][good[1]]["yuvf_sha256"]


EINVAL = 22
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
# (fixture of tests/golden/alpha, its own scale options): every picture but ll_noise_f0 reaches the scaled
# tensor's 31 x 17, by a shrink, a crop, or a crop that expands
MIXED = [("raw_f0", dict(scale=(31, 17))),
         ("ll_argb_f0", dict(scale=(31, 17))),  # 15 KB, 160 x 100
         ("ll_noise_f0", dict(scale=(36, 24))),  # 64 x 48: no tensor's size, scaled or not
         ("ll_argb_f1", dict(crop=(3, 2, 30, 16), scale=(31, 17), expand=True)),
         ("bad_corrupt0", dict(scale=(31, 17))),  # ll_argb_f0 with an ALPH that does not decode
         ("x_meta", dict(crop=(5, 3, 20, 11), scale=(31, 17), expand=True)),  # no ALPH: opaque
         ("c_no_image", dict(scale=(31, 17))),  # a refused container
         ("raw_f3", dict(crop=(1, 1, 35, 19), scale=(31, 17))),
         ("ll_levels2_f0", dict(scale=(31, 17)))]


@pytest.mark.parametrize("device_m05", [False, True])
def test_every_sink_agrees_on_one_mixed_batch(vp8g, device_m05, monkeypatch):
    """One batch through every sink of the pipeline, in chunks of two frames with per-frame scale options
    (n_opts = n): 37 x 21 pictures of ~1 KB beside the 15-KB ll_argb_f0 (160 x 100, so it fits the tensor only
    when scaled), a picture of no tensor's size, one whose ALPH does not decode and a refused container.
    With device_m05 the default cost model sends the four heaviest files to the two host threads: VP8G_PIPE_TRACE=1
    shows device_frames=5 host_frames=4, three "chunk device-m05" and two "chunk host-m05" lines for this batch
    (in the unscaled tensor call one host chunk holds only frames of another size: it launches nothing).
    The scaled I420 equals gpu_scale of the unscaled I420; every tensor slot equals gpu_tensor of the matching
    I420; the alpha channel equals host_alpha_plane -> gpu_scale_planes -> gpu_tensor(alpha=...); the statuses
    are 0 / EINVAL as each call's sink requires and failed tensor slots are zero."""
    monkeypatch.setenv("VP8G_CHUNK_FRAMES", "2")
    names = [n for n, _ in MIXED]
    files = [(GOLDEN / "alpha" / f"{n}.webp").read_bytes() for n in names]
    opts = [vp8g.scale_opt(**o) for _, o in MIXED]
    kw = dict(threads=2, device_m05=device_m05)
    refused = [EINVAL if n == "c_no_image" else 0 for n in names]

    plain, st = vp8g.gpu_decode_webp_batch_x(files, **kw)
    assert st == refused and [p is None for p in plain] == [s != 0 for s in refused]
    assert [p[1:] for p in plain if p] == [(160, 100) if n in ("ll_argb_f0", "bad_corrupt0") else (64, 48) if n == "ll_noise_f0"
                                           else (37, 21) for n, s in zip(names, refused) if not s]
    scaled, st = vp8g.gpu_decode_webp_batch_x(files, scale=opts, **kw)
    assert st == refused
    assert scaled == [None if p is None else vp8g.gpu_scale(*p, o) for p, o in zip(plain, opts)]

    def check(got, st, pics, size, topt, alphas=None):
        """Slot i = gpu_tensor of pics[i] where it has the tensor's size (and alphas[i] is no error), else EINVAL and zeros."""
        ok = [p is not None and p[1:] == size and not (alphas and isinstance(alphas[i], Exception)) for i, p in enumerate(pics)]
        assert st == [0 if k else EINVAL for k in ok]
        want = vp8g.gpu_tensor([p[0] for p, k in zip(pics, ok) if k], *size, topt,
                               alpha=[a for a, k in zip(alphas, ok) if k] if alphas else None)
        assert got.shape[0] == len(pics) and got.shape[1:] == want.shape[1:] and got.dtype == want.dtype
        got, want = got.cpu().view(torch.int16), want.cpu().view(torch.int16)
        rows = iter(want)
        for i, k in enumerate(ok):
            assert torch.equal(got[i], next(rows)) if k else not bool(got[i].any()), names[i]

    t_plain = vp8g.tensor_opt((37, 21), "float16", "NCHW", **IMAGENET)
    t_scaled = vp8g.tensor_opt((31, 17), "float16", "NCHW", **IMAGENET)
    check(*vp8g.gpu_decode_webp_batch_tensor(files, t_plain, extended=True, **kw), plain, (37, 21), t_plain)
    check(*vp8g.gpu_decode_webp_batch_tensor(files, t_scaled, scale=opts, extended=True, **kw), scaled, (31, 17), t_scaled)

    alphas = []  # per frame: the scaled alpha plane, None (opaque), or the error of the host decode
    for n, b, o in zip(names, files, opts):
        try:
            a = vp8g.host_alpha_plane(b)
            alphas.append(None if a is None else vp8g.gpu_scale_planes([a], [o])[0])
        except OSError as e:
            alphas.append(e)
    assert [n for n, a in zip(names, alphas) if isinstance(a, Exception)] == ["bad_corrupt0", "c_no_image"]
    assert [n for n, a in zip(names, alphas) if a is None] == ["x_meta"]
    check(*vp8g.gpu_decode_webp_batch_tensor(files, t_scaled, scale=opts, extended=True, alpha=True, **kw), scaled, (31, 17),
          t_scaled, alphas)
