"""CPU: which recon kernel a batch runs on (vp8g_plan_launch, host code only; csrc/vp8g_plan.hip,
DESIGN.md §3).  No device call is made and the environment is not read.

tests/golden/launch_plan_kat.json holds batches, as runs of equal frames, with the launch the
library chose for them before the planner became one function (recorded from a verbatim copy of the
earlier decision code, which agreed with the planner on every one of 7.2 million random cases).
Every field of the plan must match.  The hand-derived cases below say why.
"""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import ROOT

KAT = ROOT / "tests" / "golden" / "launch_plan_kat.json"
FIELDS = ("quad", "waves", "global_ctx", "parts", "workgroups", "ordered", "mirror_split", "interleave", "whole",
          "ord_first", "lds_bytes", "mode", "gctx_bytes", "mbox_bytes", "snap_bytes", "flags_bytes")
F_LOOPFILTER, F_SIMPLE, F_LF_ONLY = 1, 2, 4

DESC = np.dtype([("mb_cols", "<u4"), ("mb_rows", "<u4"), ("width", "<u4"), ("height", "<u4"), ("stride_y", "<u4"),
                 ("stride_uv", "<u4"), ("mb_offset", "<u8"), ("out_y", "<u8"), ("out_u", "<u8"), ("out_v", "<u8"),
                 ("src", "<u8", 3), ("flags", "<u4"), ("src_stride", "<u4", 2), ("reserved", "<u4"), ("dq", "<i2", (4, 6)),
                 ("lf", "u1", (4, 2, 4))])


def descs_of(vp8g, runs, packed=False):
    """Descriptors of a batch given as runs [count, mb_cols, mb_rows, width, height, flags, lf_level]: planes at
    stride = width, frames one after the other in the output, each starting on a 256-byte boundary
    (vp8g_reconstruct_batch's layout) or, packed, wherever the last one ended; every (segment, mode)
    at filter level lf_level, interior limit 1."""
    assert DESC.itemsize == C.sizeof(vp8g.Vp8gFrameDesc) == 176
    n = sum(r[0] for r in runs)
    a = np.zeros(n, dtype=DESC)
    at, mbs, outb = 0, 0, 0
    for count, cols, rows, w, h, flags, lf in runs:
        s = a[at:at + count]
        size = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        step = size if packed else (size + 255) & ~255
        s["mb_cols"], s["mb_rows"], s["width"], s["height"], s["flags"] = cols, rows, w, h, flags
        s["stride_y"], s["stride_uv"] = w, (w + 1) // 2
        s["mb_offset"] = mbs + np.arange(count, dtype=np.uint64) * np.uint64(cols * rows)
        s["out_y"] = outb + np.arange(count, dtype=np.uint64) * np.uint64(step)
        s["out_u"] = s["out_y"] + np.uint64(w * h)
        s["out_v"] = s["out_u"] + np.uint64(((w + 1) // 2) * ((h + 1) // 2))
        s["lf"][:, :, :, 0], s["lf"][:, :, :, 1] = lf, 1
        at, mbs, outb = at + count, mbs + count * cols * rows, outb + count * step
    return (vp8g.Vp8gFrameDesc * n).from_buffer(a) if n else (vp8g.Vp8gFrameDesc * 0)()


def as_dict(plan):
    return {k: getattr(plan, k) for k in FIELDS}


@pytest.fixture(scope="module")
def kat():
    return json.loads(KAT.read_text())["cases"]


def test_recorded_launches_replay(vp8g, kat):
    bad = []
    for i, c in enumerate(kat):
        split, waves, chain, splitchain, chain_il, order = c["knobs"]
        got = vp8g.plan_launch(descs_of(vp8g, c["runs"], c["packed"]), c["cus"], hint=c["hint"], split=split, waves=waves,
                               chain=chain, splitchain=splitchain, chain_il=chain_il, order=order, policy=c["policy"],
                               may_cross=bool(c["cross"]))
        if as_dict(got) != dict(zip(FIELDS, c["plan"])):
            bad.append((i, c, as_dict(got)))
    assert not bad, f"{len(bad)} of {len(kat)} differ, e.g. {bad[0]}"


def test_recorded_launches_cover_the_table(kat):
    """Every mode the library can report (0, split parts, chain + quad, with the mirror split, with the
    interleave), both kernels, the global-context variant, both callers and both outcomes of the gate;
    and the boundaries: the chain's list at the LDS limit, single and doubled (412 and 206 frames per
    workgroup), the cost sort's scratch (39 552 frames), 4 096 frames, an empty batch, no CU count, and
    the widths at which the column context of 8, 12 and 16 waves leaves LDS (799, 697, 595 columns)."""
    plans = [dict(zip(FIELDS, c["plan"])) for c in kat]
    assert {p["mode"] for p in plans} == {0, 16, 9, 11, 13}
    assert {p["quad"] for p in plans} == {0, 1} and any(p["global_ctx"] for p in plans)
    assert {c["policy"] for c in kat} == {0, 1, 2, 3} and {c["cross"] for c in kat} == {0, 1}
    n_of = [sum(r[0] for r in c["runs"]) for c in kat]
    lists = {-(-n // p["workgroups"]) for n, p in zip(n_of, plans) if p["quad"]}
    assert {205, 206, 207, 411, 412} <= lists  # (413 does not fit: such a batch is no chain)
    assert {39551, 39552, 39553, 4096, 0} <= set(n_of) and 0 in {c["cus"] for c in kat}
    cols = {max(r[1] for r in c["runs"]) for c in kat if c["runs"]}
    assert {799, 800, 697, 698, 595, 596, 1024} <= cols
    assert len(kat) >= 300 and KAT.stat().st_size < 256 * 1024


UHD = [240, 135, 3840, 2160]  # a 4K frame: 240 x 135 macroblocks


def test_hand_derived_launches(vp8g):
    """A device of 256 CUs.

    512 equal 4K frames: more frames than CUs, so the chain, one workgroup per CU with two frames
    each; equal cost classes, so no placement and no mirror split; equal sizes and two frames per
    workgroup, so the interleave: chain | quad | interleave on 256 workgroups, either way the gate.

    One of them at another filter level (cost class 64 + 2 * 63 + 1 against 64): the classes differ,
    so the frames are placed by cost; an ordered batch of at most two frames per workgroup takes the
    mirror split when the gate allows it (and the split excludes the interleave), else the interleave.

    One 4K frame through the reference entry points: 256 CUs / 1 frame is capped at 8 parts, 7 parts
    x 8 waves = 56 row pairs < the frame's 68, so 8 waves x 8 parts; with the gate closed one
    workgroup of 16 waves (a batch of at most one frame per CU), mode 0.  Through the pipeline the
    closed gate leaves the 8 waves it chose for the parts."""
    P = vp8g.plan_launch
    uniform = descs_of(vp8g, [[512] + UHD + [0, 0]])
    for cross in (True, False):
        p = P(uniform, 256, may_cross=cross)
        assert (p.quad, p.workgroups, p.waves, p.ordered, p.mirror_split, p.interleave, p.whole) == (1, 256, 16, 0, 0, 1, 1)
        assert p.mode == vp8g.MODE_CHAIN | vp8g.MODE_QUAD | vp8g.MODE_INTERLEAVE == 13
    mixed = descs_of(vp8g, [[511] + UHD + [0, 0], [1] + UHD + [F_LOOPFILTER, 63]])
    p = P(mixed, 256, may_cross=True)
    assert (p.quad, p.workgroups, p.ordered, p.mirror_split, p.interleave, p.mode) == (1, 256, 1, 1, 0, 11)
    assert p.flags_bytes == 512 * 4 and p.snap_bytes == 512 * 240 * 160
    p = P(mixed, 256, may_cross=False)
    assert (p.quad, p.workgroups, p.ordered, p.mirror_split, p.interleave, p.mode) == (1, 256, 1, 0, 1, 13)
    assert p.flags_bytes == 512 * 4  # (sized before the gate, for either outcome)
    one = descs_of(vp8g, [[1] + UHD + [0, 0]])
    p = P(one, 256, may_cross=True)
    assert (p.quad, p.waves, p.parts, p.workgroups, p.mode) == (0, 8, 8, 8, vp8g.MODE_SPLIT_PARTS)
    assert p.mbox_bytes == 8 * 240 * 160 + 8 * 4
    p = P(one, 256, may_cross=False)
    assert (p.quad, p.waves, p.parts, p.workgroups, p.global_ctx, p.mode) == (0, 16, 1, 1, 0, 0)
    p = P(one, 256, may_cross=False, policy=vp8g.PLAN_PIPELINE)
    assert (p.quad, p.waves, p.parts, p.workgroups, p.global_ctx, p.mode) == (0, 8, 1, 1, 0, 0)
    # the asynchronous device API never splits by itself, a wave hint is taken as given
    p = P(one, 256, policy=vp8g.PLAN_NO_SPLIT)
    assert (p.waves, p.parts, p.mode) == (16, 1, 0)
    p = P(uniform, 256, hint=12)
    assert (p.quad, p.waves, p.workgroups, p.mode) == (0, 12, 512, 0)


@pytest.mark.gpu
def test_reported_mode_is_the_planned_mode(vp8g, monkeypatch):
    """Ties the table to what launches: for four small batches the mode vp8g_last_launch_mode reports
    after a synchronous vp8g_reconstruct_batch is the mode vp8g_plan_launch gives for the same
    descriptors on this device's CU count, the reference policy and an open gate (the device is idle:
    synchronised first).  One 64x64 frame (mode 0); CUs + 1 frames of 32x32, equal (the plain chain)
    and at two filter levels (placed by cost, mirror split); 2 x CUs equal 64x64 frames (interleave).
    Every output equals the oracle's."""
    import torch
    for k in ("VP8G_SPLIT", "VP8G_WAVES", "VP8G_CHAIN", "VP8G_SPLITCHAIN", "VP8G_CHAIN_IL", "VP8G_ORDER"):
        monkeypatch.delenv(k, raising=False)
    lib = vp8g.gpu_lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    a64, a32, b32 = vp8g.synth_frame(64, 64, 0x91A, 0), vp8g.synth_frame(32, 32, 0x91B, 0), vp8g.synth_frame(32, 32, 0x91B, 0)
    for s in range(4):  # (profile 0: absolute segment levels 8, 5, 23, 31)
        b32.frame.seg_lf_level[s] = 63
    exp = {id(f): vp8g.oracle_reconstruct(f, True) for f in (a64, a32, b32)}
    batches = [([a64], 0, 0), ([a32] * (cus + 1), 9, 0), ([a32 if i % 2 else b32 for i in range(cus + 1)], 11, 1),
               ([a64] * (2 * cus), 13, 0)]
    for frames, mode, ordered in batches:
        descs = (vp8g.Vp8gFrameDesc * len(frames))()
        mbs = outb = 0
        for i, f in enumerate(frames):  # (vp8g_reconstruct_batch's layout)
            assert lib.vp8g_make_frame_desc(C.byref(f.kf), C.byref(f.frame), 1, mbs, outb, C.byref(descs[i])) == 0
            mbs += f.frame.mb_cols * f.frame.mb_rows
            outb = (outb + vp8g.i420_size(f.width, f.height) + 255) & ~255
        plan = vp8g.plan_launch(descs, cus)
        assert (plan.mode, plan.ordered) == (mode, ordered)
        torch.cuda.synchronize()
        outs = vp8g.gpu_reconstruct_batch(frames, True)
        assert int(lib.vp8g_last_launch_mode()) == plan.mode, (len(frames), plan.mode)
        assert all(o == exp[id(f)] for f, o in zip(frames, outs))


def test_bad_arguments(vp8g):
    lib = vp8g.gpu_lib()
    out = vp8g.Vp8gLaunchPlan()
    one = descs_of(vp8g, [[1] + UHD + [0, 0]])
    C.set_errno(0)
    assert lib.vp8g_plan_launch(one, 1, 256, 0, 0, 0, -1, -1, -1, 1, 4, 1, C.byref(out)) == -1 and C.get_errno() == 22
    assert lib.vp8g_plan_launch(one, 1, 256, 0, 0, 0, -1, -1, -1, 1, 0, 1, None) == -1
    wide = descs_of(vp8g, [[1, 1025, 4, 16400, 64, 0, 0]])
    assert lib.vp8g_plan_launch(wide, 1, 256, 0, 0, 0, -1, -1, -1, 1, 0, 1, C.byref(out)) == -1
