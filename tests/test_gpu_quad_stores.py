"""GPU: the quad chain's pixel stores and its B_PRED step (csrc/vp8g_quad.inc) on the
shapes where they take another path: a chroma row leaves as one 16-B store of the lane's kept piece
(even MB column) and current piece (odd column), an even last column alone, a cut last column byte by
byte; every B_PRED mode goes through one dot product and one shift.  Every slot is compared byte for
byte with the oracle (reference src/m06_recon/vp8_recon.c:444-684, src/m07_loopfilter/vp8_loopfilter.c:214-280).

Shapes: MB columns 1..5 (even and odd last column, with and without a pair before it), MB rows 1, 4,
5, 9 (one quad, a full quad, a last quad of one row, three quads), widths 16 C (whole pieces: the lean
instantiation) and 16 C - 7 (cut last column, unaligned rows: the general one), each decoded with
the normal filter, the simple filter and unfiltered."""
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

COLS, ROWS = (1, 2, 3, 4, 5), (1, 4, 5, 9)
FILTERS = ("normal", "simple", "off")


def _frame(vp8g, w, h, seed, flt):
    f = vp8g.synth_frame(w, h, seed, 1 + (seed & 1))
    if flt != "off":
        f.frame.lf_use_simple = int(flt == "simple")
        f.frame.lf_level = 20 + seed % 44  # (never 0: the filter runs)
    return f


def _launch(vp8g, b, whole):
    import vp8g_batch  # noqa: F401
    b.commit()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert bool(vp8g.plan_launch(b.h_descs, cus).whole) == whole
    stream = torch.cuda.current_stream(b.dev).cuda_stream
    b.launch(stream)
    torch.cuda.synchronize()
    assert b.status_word() == 0
    mode = b.launch_mode()
    assert mode & vp8g.MODE_CHAIN and mode & vp8g.MODE_QUAD, mode


def _slots():
    """More frames than CUs (the chain's condition), every case at least five times."""
    return torch.cuda.get_device_properties(0).multi_processor_count + 64


def _check_batch(vp8g, cases, whole):
    """cases: (frame, filtered).  Slot i <- case i % len(cases); every slot equals the oracle's output,
    and the rest of the slot (past the frame's I420 bytes) stays untouched."""
    import vp8g_batch
    n = _slots()
    W = max(f.width for f, _ in cases)
    H = max(f.height for f, _ in cases)
    b = vp8g_batch.DeviceBatch(n, W, H, torch.device("cuda:0"))
    b.out.fill_(0xA5)
    for i in range(n):
        b.place(i, *cases[i % len(cases)])
    _launch(vp8g, b, whole)
    exp = [vp8g.oracle_reconstruct(f, flt) for f, flt in cases]
    host = b.out.cpu().numpy().reshape(n, b.frame_bytes)
    bad = []
    for i in range(n):
        e = np.frombuffer(exp[i % len(cases)], np.uint8)
        if not np.array_equal(host[i, :len(e)], e):
            f, flt = cases[i % len(cases)]
            k = int(np.flatnonzero(host[i, :len(e)] != e)[0])
            bad.append(f"slot {i} {f.width}x{f.height} filtered={flt} simple={f.frame.lf_use_simple} byte {k} "
                       f"(luma bytes {f.width * f.height}): got {host[i, k]} expected {e[k]}")
        elif (host[i, len(e):] != 0xA5).any():
            bad.append(f"slot {i}: bytes past the frame written")
    assert not bad, f"{len(bad)} slots differ, e.g. {bad[:4]}"


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "cut"])
def test_quad_stores_columns_rows_filters(vp8g, whole):
    """C = 1..5 x R = 1, 4, 5, 9 x {normal, simple, unfiltered}, at width 16 C and height 16 R (whole
    pieces; odd C gives a chroma stride of 8 C, 8-B but not 16-B aligned) or at width 16 C - 7 and
    height 16 R - 3 (cut last column, odd chroma size, rows that start unaligned)."""
    cases = []
    for c in COLS:
        for r in ROWS:
            for k, flt in enumerate(FILTERS):
                w, h = (16 * c, 16 * r) if whole else (16 * c - 7, 16 * r - 3)
                cases.append((_frame(vp8g, w, h, 0x51 + 64 * c + 8 * r + k, flt), flt != "off"))
    _check_batch(vp8g, cases, whole)
    for f, _ in cases:
        f.free()


def test_quad_stores_chroma_stride_8_not_16(vp8g):
    """Whole-piece frames of 2 and 4 MB columns whose descriptors carry stride_uv = 8 C + 8 (8-B aligned,
    not 16-B aligned): every 16-B chroma store starts 8 B off a 16-B boundary in every other row.  The
    planes equal the oracle's row by row and the 8 bytes between the rows stay untouched."""
    import vp8g_batch
    n = _slots()
    R = 5
    cases = [(_frame(vp8g, 16 * c, 16 * R, 0x77 + 8 * c + k, flt), flt != "off") for c in (2, 4) for k, flt in enumerate(FILTERS)]
    b = vp8g_batch.DeviceBatch(n, 96, 16 * R, torch.device("cuda:0"))  # (slots wide enough for the padded chroma rows)
    b.out.fill_(0xA5)
    for i in range(n):
        f, flt = cases[i % len(cases)]
        b.place(i, f, flt)
        d = b.h_descs[i]
        ch = (f.height + 1) // 2
        d.stride_uv = f.width // 2 + 8
        d.out_v = d.out_u + d.stride_uv * ch
        assert d.stride_uv % 16 == 8 and d.out_v + d.stride_uv * ch <= (i + 1) * b.frame_bytes
    _launch(vp8g, b, True)
    exp = [np.frombuffer(vp8g.oracle_reconstruct(f, flt), np.uint8) for f, flt in cases]
    host = b.out.cpu().numpy().reshape(n, b.frame_bytes)
    bad = []
    for i in range(n):
        f, _ = cases[i % len(cases)]
        e = exp[i % len(cases)]
        w, h, cw, ch = f.width, f.height, f.width // 2, f.height // 2
        su = cw + 8
        uv = host[i, w * h:w * h + 2 * su * ch].reshape(2 * ch, su)
        ok = (np.array_equal(host[i, :w * h], e[:w * h]) and np.array_equal(uv[:, :cw].reshape(-1), e[w * h:])
              and (uv[:, cw:] == 0xA5).all() and (host[i, w * h + 2 * su * ch:] == 0xA5).all())
        if not ok:
            bad.append(i)
    assert not bad, f"{len(bad)} slots differ, e.g. {bad[:8]}"
    for f, _ in cases:
        f.free()


def _bpred_frame(vp8g, w, h, seed):
    """Every MB B_PRED; sub-block b of MB m has mode (b + m) % 10, so each sub-block position meets
    every mode (TM = 1 included) within ten MBs.  At q_index 0 (every factor 4) a third of the blocks
    carry a DC of +512 (residual +256: saturates at 255 whatever the prediction), a third -512 (at 0),
    a third sparse coefficients within +-40 (residuals that stay inside)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import directed
    rng = np.random.default_rng(seed)
    f = vp8g.synth_frame(w, h, seed, 1)
    n = f.mb_total
    h_ = f.frame
    h_.q_index = 0
    h_.y1_dc_delta_q = h_.y2_dc_delta_q = h_.y2_ac_delta_q = h_.uv_dc_delta_q = h_.uv_ac_delta_q = 0
    h_.segmentation_enabled = 0
    h_.lf_use_simple, h_.lf_level = 0, 30
    f.array("ymode")[:] = 4
    m, blk = np.arange(n)[:, None], np.arange(16)[None, :]
    f.array("bmode").reshape(n, 16)[:] = (blk + m) % 10
    cy = f.array("coeff_y").reshape(n, 16, 16)
    kind = (blk + 2 * m) % 3
    small = np.where(rng.random((n, 16, 16)) < 0.2, rng.integers(-40, 41, (n, 16, 16)), 0).astype(np.int16)
    cy[:] = np.where((kind == 2)[:, :, None], small, 0)
    cy[:, :, 0] = np.where(kind == 0, 512, np.where(kind == 1, -512, cy[:, :, 0]))
    f.array("coeff_y2")[:] = 0
    directed._truth(f)
    return f


def test_quad_bpred_every_mode_saturating_residuals(vp8g):
    """A 5 x 5 MB frame (a quad of four B_PRED rows: both groups in every lane; a last quad of one
    row: one group per lane) and a 3 x 2 one, all ten B_PRED modes at every sub-block position with
    residuals that saturate both ways, filtered and unfiltered, through the quad chain; the same
    frames through the single-frame entry point (frame_kernel shares the predictor table)."""
    frames = [_bpred_frame(vp8g, 80, 80, 0xB9), _bpred_frame(vp8g, 48, 32, 0xBA)]
    for f in frames:
        bm = f.array("bmode").reshape(f.mb_total, 16)
        assert all(set(bm[:, b].tolist()) == set(range(10)) for b in range(16)) or f.mb_total < 10
        out = np.frombuffer(vp8g.oracle_reconstruct(f, False), np.uint8)[:f.width * f.height]
        assert (out == 0).any() and (out == 255).any() and ((out > 0) & (out < 255)).any()
    cases = [(f, flt) for f in frames for flt in (True, False)]
    _check_batch(vp8g, cases, True)
    for f, flt in cases:
        assert vp8g.gpu_reconstruct(f, flt) == vp8g.oracle_reconstruct(f, flt)
    for f in frames:
        f.free()
