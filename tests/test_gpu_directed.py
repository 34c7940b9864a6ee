"""GPU: the directed frames of tests/directed.py through every reconstruction path, byte for byte
against the oracle (and the uniform kinds, `wrap` and the sat_* kinds against the reference's hashes,
tests/golden/directed_kat.json).  tests/test_directed.py proves on the CPU what each kind reaches;
here is which kernel meets it:

  frame kernel (one workgroup per frame, launch mode 0; ballot over one MB)
      test_single_frame_entry_points_and_small_batch, test_forced_split_factors[3-8] (8 waves), and
      with more frames than CUs (cost-ordered placement) test_frame_kernel_directed_many_frames
  split parts (one frame over several workgroups)    test_forced_split_factors[8-0]
  quad chain (ballot over four vertically adjacent MBs, per role), whole pieces and cut / unaligned
      test_quad_chain_directed, and with the mirror split forced test_quad_chain_directed_mirror_split
  device-memory context path (8200 wide), one-column path (16 wide)   test_extreme_dimensions_directed
  m07 alone on planes the filter modifies            test_loopfilter_entry_point_smooth_planes
  m07 alone on planes that saturate its arithmetic   test_loopfilter_entry_point_step_planes
  the batch pipeline (.webp in, host and device m05) on two sat_* kinds   test_pipeline_saturating_kinds
The sat_* kinds (the loop filter's clamps: w and a beyond +-127, taps beyond 0..255; the census is in
tests/test_directed.py) are part of D.KINDS and so of every test above the m07-alone ones.
and the launch-mode report itself (test_launch_mode_is_zero_after_an_invalid_call).

Reference path: src/m06_recon/vp8_recon.c:444-684 + src/m07_loopfilter/vp8_loopfilter.c:214-280.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import directed as D
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in ("VP8G_SPLIT", "VP8G_WAVES")}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def first_diff(f, got, exp):
    """Where two I420 outputs of frame f first differ: plane, byte offset in it, the two values."""
    k = int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(exp, np.uint8))[0])
    ysz, csz = f.width * f.height, ((f.width + 1) // 2) * ((f.height + 1) // 2)
    plane, o = ("Y", k) if k < ysz else (("U", k - ysz) if k < ysz + csz else ("V", k - ysz - csz))
    return f"{f.width}x{f.height} plane {plane} byte {o} (row {o // (f.width if plane == 'Y' else (f.width + 1) // 2)}): got {got[k]}, expected {exp[k]}"


def check(vp8g, frames, labels, outs, filtered):
    assert len(outs) == len(frames)
    for f, lab, o in zip(frames, labels, outs):
        exp = vp8g.oracle_reconstruct(f, filtered)
        assert len(o) == len(exp), (lab, filtered)
        assert o == exp, f"{lab} filtered={filtered}: {first_diff(f, o, exp)}"


def last_mode(vp8g):
    lib = vp8g.gpu_lib()
    assert hasattr(lib, "vp8g_last_launch_mode"), "the loaded library cannot report its launch mode"
    return int(lib.vp8g_last_launch_mode())


def test_single_frame_entry_points_and_small_batch(vp8g, env):
    """Every kind at 320x256 and at an odd size, one workgroup per frame (VP8G_SPLIT=1; launch mode 0):
    the frame kernel's ballot spans one MB, so `mixed` and the spoilers change its iDCT form from MB to
    MB.  The batch API on all 78 frames; the single-frame entry points on the uniform kinds, `wrap` and
    the sat_* kinds (held to the reference's hashes too), `mixed`, the spoilers and the has_coeff lies."""
    env["VP8G_SPLIT"] = "1"
    env.pop("VP8G_WAVES", None)
    kat = json.loads((GOLDEN / "directed_kat.json").read_text())["cases"]
    cases = D.kat_cases()
    frames = [D.build(*c) for c in cases]
    labels = [D.kat_key(*c) for c in cases]
    for filtered in (False, True):
        outs = vp8g.gpu_reconstruct_batch(frames, filtered)
        assert last_mode(vp8g) == 0
        check(vp8g, frames, labels, outs, filtered)
        for c, f, lab, o in zip(cases, frames, labels, outs):
            if c[0] in D.UNIFORM + ["wrap"] + D.SAT_KINDS:
                assert hashlib.sha256(o).hexdigest() == kat[lab]["yuvf_sha256" if filtered else "yuv_sha256"], lab
            if c[0] in D.UNIFORM + D.SPOILERS + D.SAT_KINDS + ["wrap", "mixed", "lie_hasc0", "lie_hasc1"]:
                one = vp8g.gpu_reconstruct(f, filtered)
                assert last_mode(vp8g) == 0
                assert one == o, f"{lab} filtered={filtered}: single-frame call vs batch, {first_diff(f, one, o)}"


@pytest.mark.parametrize("split,waves", [(3, 8), (8, 0)])
def test_forced_split_factors(vp8g, env, split, waves):
    """Every kind at 48x1840 (115 MB rows: enough row pairs for eight parts of eight waves) and 52x300,
    39 frames in calls of 18, 18 and 3.  VP8G_SPLIT=8: the frames run as split parts (the mode is asserted);
    VP8G_SPLIT=3 with VP8G_WAVES=8: a waves override keeps the shim from splitting, so this is the
    frame kernel at eight waves per workgroup (mode 0)."""
    env["VP8G_SPLIT"] = str(split)
    if waves:
        env["VP8G_WAVES"] = str(waves)
    else:
        env.pop("VP8G_WAVES", None)
    cases = [(k, *((48, 1840) if i % 3 else (52, 300)), 20 + i) for i, k in enumerate(D.KINDS)]
    frames = [D.build(*c) for c in cases]
    labels = [D.kat_key(*c) for c in cases]
    for filtered in (False, True):
        for lo in range(0, len(frames), 18):
            outs = vp8g.gpu_reconstruct_batch(frames[lo:lo + 18], filtered)
            mode = last_mode(vp8g)
            assert mode == (0 if waves else vp8g.MODE_SPLIT_PARTS), mode
            check(vp8g, frames[lo:lo + 18], labels[lo:lo + 18], outs, filtered)


@pytest.mark.parametrize("odd", [False, True], ids=["whole", "odd"])
def test_quad_chain_directed(vp8g, odd):
    """1 200 slots of the 156 directed frames (every kind at four sizes, filtered at two): the quad
    chain's ballot spans four vertically adjacent MBs, separately per role -- uniform frames hold every
    wave to one form at every geometry (last quads of 1..3 rows, cut pieces, one column), `mixed` changes
    the form from step to step inside a chain.  Launch mode: chain + quad."""
    sys.path.insert(0, str(ROOT / "tests"))
    import quad_check
    sizes = quad_check.ODD_SIZES if odd else quad_check.SIZES
    bad = quad_check.run(n=1200, seed=0xD1A, frames=quad_check.directed_frames(sizes))
    assert not bad, f"{len(bad) - 1} slots differ: {bad[:8]}"


@pytest.mark.parametrize("odd", [False, True], ids=["whole", "odd"])
def test_quad_chain_directed_mirror_split(vp8g, odd):
    """The same batch with the mirror split forced (VP8G_SPLITCHAIN=1, child process), two launches."""
    env = dict(os.environ, VP8G_SPLITCHAIN="1")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "quad_check.py"), "--directed"] + (["--odd"] if odd else []),
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().endswith("OK"), r.stdout


@pytest.mark.parametrize("odd", [False, True], ids=["whole", "odd"])
def test_frame_kernel_directed_many_frames(vp8g, odd):
    """The same batch with the chain off (VP8G_CHAIN=0, child process): one workgroup per frame with more frames
    than CUs (ordered_frame's placement runs too); launch mode 0, status 0, every slot exact, empty ones untouched."""
    env = dict(os.environ, VP8G_CHAIN="0")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "quad_check.py"), "--directed"] + (["--odd"] if odd else []),
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().endswith("OK"), r.stdout


@pytest.mark.parametrize("w,h", [(8200, 40), (16, 2000)])
def test_extreme_dimensions_directed(vp8g, w, h):
    """A DC-only, a columns-0-1, a skip and a saturating frame (sat_seg: flat MBs, flat sub-blocks and
    hev tiles under four segment levels) where the per-column context lives in device memory (8200
    wide) and where a frame is one MB column (16 wide)."""
    for kind in ("uni_dc_dc", "uni_cols01_cols01", "skip", "sat_seg"):
        f = D.build(kind, w, h, 3)
        for filtered in (False, True):
            check(vp8g, [f], [f"{kind}/{w}x{h}"], [vp8g.gpu_reconstruct(f, filtered)], filtered)


def lf_entry_point(vp8g, case, f, planes):
    """vp8_loopfilter_apply_keyframe on `planes` under f's header against oracle_loopfilter, plane by plane."""
    lib = vp8g.gpu_lib()
    w, h = int(f.frame.mb_cols) * 16, int(f.frame.mb_rows) * 16
    img = vp8g.Yuv420Image()
    assert lib.yuv420_alloc(C.byref(img), w, h) == 0
    for dst, src in zip((img.y, img.u, img.v), planes):
        C.memmove(dst, src.ctypes.data, src.nbytes)
    assert lib.vp8_loopfilter_apply_keyframe(C.byref(img), C.byref(f.frame)) == 0
    got = [np.ctypeslib.as_array(p, shape=(a.size,)).copy() for p, a in zip((img.y, img.u, img.v), planes)]
    lib.yuv420_free(C.byref(img))
    exp = [p.copy() for p in planes]
    assert vp8g.oracle_lib().oracle_loopfilter(*[p.ctypes.data for p in exp], C.byref(f.frame)) == 0
    assert not np.array_equal(exp[0], planes[0])  # (the filter modified the luma plane)
    for name, g, e in zip("YUV", got, exp):
        assert np.array_equal(g, e), (case, name, int(np.flatnonzero(g != e)[0]))


@pytest.mark.parametrize("case", range(16))
def test_loopfilter_entry_point_smooth_planes(vp8g, case):
    """vp8_loopfilter_apply_keyframe (m07 alone, in place on a padded image) under every directed
    loop-filter header, on smooth planes: ~50 % of the normal filter's positions pass the mask
    (tests/test_directed.py), where the uniform noise of test_gpu_parity's cases passes at < 1 %."""
    lf_entry_point(vp8g, case, *D.lf_entry_case(case))


@pytest.mark.parametrize("case", range(len(D.LF_STEP_CASES)))
def test_loopfilter_entry_point_step_planes(vp8g, case):
    """The same entry point on planes of flat tiles, +-k patterns beside steps and range ends, under
    simple and normal headers at levels 57..63, sharpness 0 and > 0: every reachable clamp of the
    filter's arithmetic fires at >= 200 positions over the cases (tests/test_directed.py)."""
    lf_entry_point(vp8g, case, *D.lf_step_case(case))


@pytest.mark.parametrize("device_m05", [False, True], ids=["host_m05", "device_m05"])
def test_pipeline_saturating_kinds(vp8g, device_m05):
    """sat_mb (w beyond +-127 between flat MBs) and sat_seg (segment levels on both sides of where w can
    saturate; flat sub-blocks and hev tiles) at 320x256, written as .webp by the test stream writer and
    decoded by the batch pipeline, filtered, against the oracle on the frame the stream carries."""
    sys.path.insert(0, str(ROOT / "tests"))
    import streams as S
    built = [S.directed_stream(k, 320, 256, 7) for k in ("sat_mb", "sat_seg")]
    outs, st = vp8g.gpu_decode_webp_batch([d for _, d in built], True, 2, device_m05=device_m05)
    assert st == [0, 0], st
    check(vp8g, [f for f, _ in built], ["sat_mb.webp", "sat_seg.webp"], outs, True)


def test_launch_mode_is_zero_after_an_invalid_call(vp8g):
    """include/vp8g.h: vp8g_last_launch_mode is 0 after a call that failed before its launch.  One
    chain launch (mode != 0), then calls the entry points reject with EINVAL -- a null descriptor
    pointer for vp8g_decode_batch_device, n = 0 for vp8g_reconstruct_batch -- each must leave mode 0,
    not the chain's."""
    import torch
    import vp8g_batch
    dev = torch.device("cuda:0")
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    f = D.build("mixed", 160, 64, 1)
    b = vp8g_batch.DeviceBatch(n, 160, 64, dev)
    for i in range(n):
        b.fill(i, f, True)
    b.commit()
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = vp8g.gpu_lib()

    def chain_launch():
        b.launch(stream)
        torch.cuda.synchronize()
        assert b.status_word() == 0
        mode = b.launch_mode()
        assert mode & vp8g.MODE_CHAIN and mode & vp8g.MODE_QUAD, mode
        assert b.frame_output(n - 1) == vp8g.oracle_reconstruct(f, True)

    chain_launch()
    C.set_errno(0)
    rc = lib.vp8g_decode_batch_device(None, C.c_void_p(b.d_descs.data_ptr()), n, C.byref(b.c_arrays),
                                      C.c_void_p(b.out.data_ptr()), C.c_void_p(stream), 0)
    assert rc == -1 and C.get_errno() == 22
    assert b.launch_mode() == 0
    chain_launch()
    img = vp8g.Yuv420Image()
    kfs = (C.POINTER(vp8g.Vp8KeyFrameHeader) * 1)(C.pointer(f.kf))
    frs = (C.POINTER(vp8g.Vp8DecodedFrame) * 1)(C.pointer(f.frame))
    C.set_errno(0)
    assert lib.vp8g_reconstruct_batch(C.cast(kfs, C.c_void_p), C.cast(frs, C.c_void_p), 0, 1, C.byref(img)) == -1
    assert C.get_errno() == 22
    assert b.launch_mode() == 0
