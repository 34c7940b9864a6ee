"""Batch decoded by the quad chain kernel (csrc/vp8g_quad.inc: four MB rows per wave; every chain
batch), every slot against the oracle.  Imported by tests/test_gpu_quad.py,
and run as a child process there when an environment switch of libvp8g must be set for the whole run
(VP8G_SPLITCHAIN=1: every frame of more than four MB rows split between two workgroups).

Frames (SIZES): widths multiples of 16 (whole 16-B / 8-B row pieces: the kernel's lean instantiation),
heights giving 1..19 MB rows -- last quads of one, two, three and four rows -- and odd pixel heights
(cropped bottom rows); ODD_SIZES adds widths that cut the right MB's pieces and rows that start
unaligned (stride = width: the general instantiation's byte path).  All synthetic
profiles (segments, loop-filter deltas, simple and normal filter, +-2114 coefficients), filtered and
unfiltered, in a scrambled order with one slot in eight left empty.

run(frames=...) decodes a caller's frames instead (directed_frames(): every kind of tests/directed.py
at four of the sizes, filtered at two of them); want_mode: the chain and quad bits, or 0 (VP8G_CHAIN=0)."""
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
import vp8g  # noqa: E402
import vp8g_batch  # noqa: E402

SIZES = [(16, 16), (16, 48), (32, 24), (160, 64), (48, 112), (1024, 80), (160, 96), (64, 200), (128, 304), (96, 36)]
ODD_SIZES = SIZES[:5] + [(1, 1), (17, 16), (33, 50), (100, 70), (250, 130), (1000, 37), (8, 8), (24, 200), (52, 300), (15, 33)]


def directed_frames(sizes, seed=11):
    """Every directed kind at four of `sizes` (kind k: sizes k, k + 3, k + 6, k + 9 mod len); the frames
    at even positions are decoded unfiltered by run(), those at odd positions filtered."""
    import directed
    return [directed.build(kind, *sizes[(k + 3 * r) % len(sizes)], seed + 4 * k + r)
            for k, kind in enumerate(directed.KINDS) for r in range(4)]


def compare(b, frames, pick, empty, exp):
    """Every slot of the batch `b` after a launch against the oracle: slot i holds frames[pick[i]],
    filtered when that index is odd; the slots of `empty` must still hold the 0xA5 fill.  `exp` caches
    the oracle's output per (frame, filtered).  -> [] or ["first: <the first differing slot: its frame,
    plane and byte>", differing slots ..., "empty slot i written" ...]"""
    host, bad = b.out.cpu().numpy(), []
    first = None
    for i in range(len(pick)):
        if i in empty:
            continue
        j = int(pick[i])
        key = (j, bool(j % 2))
        if key not in exp:
            exp[key] = np.frombuffer(vp8g.oracle_reconstruct(frames[j], key[1]), np.uint8)
        got = host[i * b.frame_bytes:i * b.frame_bytes + exp[key].size]
        if not np.array_equal(got, exp[key]):
            if first is None:
                f, k = frames[j], int(np.flatnonzero(got != exp[key])[0])
                ysz, csz = f.width * f.height, ((f.width + 1) // 2) * ((f.height + 1) // 2)
                plane, o = ("Y", k) if k < ysz else (("U", k - ysz) if k < ysz + csz else ("V", k - ysz - csz))
                first = (f"first: slot {i} frame {j} {f.width}x{f.height} filtered={key[1]} plane {plane} byte {o} "
                         f"got {got[k]} expected {exp[key][k]}")
            bad.append(i)
    for i in sorted(empty):
        if not (host[i * b.frame_bytes:i * b.frame_bytes + b.i420] == 0xA5).all():
            bad.append(f"empty slot {i} written")
    return ([first] if first else []) + bad


def run(n=1800, seed=0x0A4D, launches=1, want_split=False, sizes=SIZES, frames=None, want_mode=vp8g.MODE_CHAIN | vp8g.MODE_QUAD):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    sizes_only = frames is None
    if sizes_only:
        frames = [vp8g.synth_frame(*sizes[i % len(sizes)], seed ^ (i * 0x9E37), profile=i % 3) for i in range(40)]
        W = max(w for w, _ in sizes)
        H = max(h for _, h in sizes)
    else:
        W = max(f.width for f in frames)
        H = max(f.height for f in frames)
    b = vp8g_batch.DeviceBatch(n, W, H, dev)
    b.out.fill_(0xA5)
    pick = rng.integers(0, len(frames), n) if sizes_only else rng.permutation(n) % len(frames)  # (a caller's frames: every one decoded)
    empty = set(rng.choice(n, n // 8, replace=False).tolist())
    for i in range(n):
        if i not in empty:
            b.place(i, frames[pick[i]], bool(pick[i] % 2))
    b.commit()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(launches):
        b.launch(stream)
        torch.cuda.synchronize()
        if b.status_word() != 0:
            return [f"status {b.status_word()}"]
        mode = b.launch_mode()
        if mode is None:
            return ["launch mode unknown: the loaded library has no vp8g_last_launch_mode"]
        if (mode if want_mode == 0 else mode & (vp8g.MODE_CHAIN | vp8g.MODE_QUAD)) != want_mode or (want_split and not mode & vp8g.MODE_MIRROR_SPLIT):
            return [f"launch mode {mode}: expected {want_mode}{' with the mirror split' if want_split else ''}"]
    bad = compare(b, frames, pick, empty, {})
    for f in frames:
        f.free()
    return bad


def run_each(n, seed, launches, sizes, slot, want_mode, empties=True, before_launch=None):
    """A batch of `n` slots of `slot` = (width, height) decoded `launches` times, with OTHER frames in the
    same slots every time (launch k: slot i <- frame (pick[i] + k) mod 40 of 40 synthetic frames over
    `sizes`, filtered when that index is odd -- so a slot's frame, size and filter setting change between
    launches and whatever an earlier launch left in a hand-off buffer is the wrong context).  The output is
    refilled with 0xA5 before and compared with the oracle after every launch; `want_mode`: the exact
    launch-mode word.  before_launch(k) is called ahead of launch k.  -> per launch, run()'s list."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    frames = [vp8g.synth_frame(*sizes[i % len(sizes)], seed ^ (i * 0x9E37), profile=i % 3) for i in range(40)]
    b = vp8g_batch.DeviceBatch(n, *slot, dev)
    pick = rng.integers(0, len(frames), n)
    empty = set(rng.choice(n, n // 8, replace=False).tolist()) if empties else set()
    stream = torch.cuda.current_stream(dev).cuda_stream
    exp, out = {}, []
    for k in range(launches):
        pk = (pick + k) % len(frames)
        for i in range(n):
            if i not in empty:
                b.place(i, frames[pk[i]], bool(pk[i] % 2))
        b.commit()
        b.out.fill_(0xA5)
        b.status.zero_()
        if before_launch:
            before_launch(k)
        b.launch(stream)
        torch.cuda.synchronize()
        if b.status_word() != 0:
            out.append([f"status {b.status_word()}"])
            continue
        if b.launch_mode() != want_mode:
            out.append([f"launch mode {b.launch_mode()}: expected {want_mode}"])
            continue
        out.append(compare(b, frames, pk, empty, exp))
    for f in frames:
        f.free()
    return out


if __name__ == "__main__":
    import os
    sizes = ODD_SIZES if "--odd" in sys.argv else SIZES
    if "--directed" in sys.argv:
        sys.path.insert(0, str(ROOT / "tests"))
        bad = run(n=1200, seed=0xD1A, launches=2, want_split=os.environ.get("VP8G_SPLITCHAIN") == "1",
                  frames=directed_frames(sizes), **({"want_mode": 0} if os.environ.get("VP8G_CHAIN") == "0" else {}))
        print("OK" if not bad else f"BAD {len(bad)}: {bad[:8]}")
        sys.exit(0)
    bad = run(launches=2, want_split=os.environ.get("VP8G_SPLITCHAIN") == "1", sizes=sizes)
    print("OK" if not bad else f"BAD {len(bad)}: {bad[:8]}")
