#!/usr/bin/env python3
"""Measure libwebp's scaled RGB against the I420 route on one MI355X, in one process.

Both routes start from N device-resident I420 pictures of one size and end in a float16 NCHW tensor of 224x224:

  i420    vp8g_make_scale_desc      -> vp8g_scale_batch_device -> vp8g_tensor_batch_device      (chroma to ceil(target / 2), fancy upsampling)
  rgb444  vp8g_make_scale_desc_444  -> vp8g_scale_batch_device -> vp8g_tensor_batch_device_444  (chroma to the target, pixel by pixel)

for 4K sources (the source read dominates), 640x480 (chroma 320x240 still shrinks to 224x224) and 400x300 (chroma
200x150 expands in both axes: the expand kernel runs beside the shrink kernel).  The routes alternate, run by run; HIP-event
ms, median / min / max of the warm runs, one cold run of each discarded; the scale launch alone is timed too.  Pictures 0
and N - 1 of both routes are compared with the host restatements.  Writes profiles/scale_rgb_bench.json and prints the
table of §14.2.

  python tools/scale_rgb_bench.py [--frames 512] [--runs 20]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: its HIP runtime serves the process, as in bench.py)

import vp8g  # noqa: E402

TARGET = (224, 224)


class Route:
    """Scale and tensor launches of one route over n tight I420 pictures at `src` (a device tensor)."""

    def __init__(self, kind, src, n, size, dev):
        self.lib, self.kind, self.n, (w, h), self.src = vp8g.gpu_lib(), kind, n, size, src
        lib, y444 = self.lib, kind == "rgb444"
        self.opt = vp8g.scale_opt(scale=TARGET)
        self.topt = vp8g.tensor_opt(TARGET, "float16", "NCHW", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
        tw, th = TARGET
        fsz, cw, ch = vp8g.i420_size(w, h), (w + 1) // 2, (h + 1) // 2
        self.mid_bytes = 3 * tw * th if y444 else vp8g.i420_size(tw, th)
        mslot, tslot = (self.mid_bytes + 255) // 256 * 256, lib.vp8g_tensor_slot_size(C.byref(self.topt))
        self.sdescs, self.tdescs = (vp8g.Vp8gScaleDesc * n)(), (vp8g.Vp8gTensorDesc * n)()
        make_s = lib.vp8g_make_scale_desc_444 if y444 else lib.vp8g_make_scale_desc
        make_t = lib.vp8g_make_tensor_desc_444 if y444 else lib.vp8g_make_tensor_desc
        stask = ttask = 0
        for i in range(n):
            o = i * fsz
            assert make_s(w, h, o, o + w * h, o + w * h + cw * ch, w, cw, C.byref(self.opt), i * mslot, stask, C.byref(self.sdescs[i])) == 0
            p = self.sdescs[i].p
            assert make_t(C.byref(self.topt), p[0].dst, p[1].dst, p[2].dst, p[0].dst_stride, p[1].dst_stride, i * tslot, ttask,
                          C.byref(self.tdescs[i])) == 0
            stask += self.sdescs[i].ntasks
            ttask += self.tdescs[i].ntasks
        self.scale_tasks, self.tensor_tasks = stask, ttask
        self.expand_planes = sum(1 for d in self.sdescs for k in range(3) if d.p[k].group == 0)
        self.d_s, self.d_t = vp8g.device_copy(self.sdescs, dev=dev), vp8g.device_copy(self.tdescs, dev=dev)
        self.mid = torch.empty(n * mslot + 16, dtype=torch.uint8, device=dev)
        self.out = torch.empty((n, 3, th, tw), dtype=torch.float16, device=dev)
        self.mslot = mslot

    def scale(self, stream):
        if self.lib.vp8g_scale_batch_device(self.sdescs, C.c_void_p(self.d_s.data_ptr()), self.n, C.c_void_p(self.src.data_ptr()),
                                            C.c_void_p(self.mid.data_ptr()), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_scale_batch_device: {self.lib.vp8g_last_error()!r}")

    def tensor(self, stream):
        a = (self.tdescs, C.c_void_p(self.d_t.data_ptr()))
        b = (C.c_void_p(self.mid.data_ptr()), C.c_void_p(self.out.data_ptr()), C.c_void_p(stream))
        rc = (self.lib.vp8g_tensor_batch_device_444(*a, None, None, self.n, C.byref(self.topt), 3, *b) if self.kind == "rgb444"
              else self.lib.vp8g_tensor_batch_device(*a, self.n, C.byref(self.topt), *b))
        if rc != 0:
            raise RuntimeError(f"tensor launch: {self.lib.vp8g_last_error()!r}")

    def both(self, stream):
        self.scale(stream)
        self.tensor(stream)

    def parity(self, host_frames, size):
        ok = True
        for i, b in host_frames.items():
            if self.kind == "rgb444":
                p = vp8g.host_scale_yuv444(b, *size, self.opt)
                want = vp8g.host_tensor_444((p[0], p[1], p[2]), self.topt)
            else:
                small, w, h = vp8g.host_scale(b, *size, self.opt)
                want = vp8g.host_tensor(small, w, h, self.topt)
            ok = ok and torch.equal(self.out[i].cpu().view(torch.int16), want.view(torch.int16))
        return ok


def timed_interleaved(legs, runs, dev):
    """{name: median / min / max ms} of `runs` warm runs of every leg, the legs alternating run by run (one cold run each first)."""
    stream = torch.cuda.current_stream(dev)
    for _, fn in legs:
        fn()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _ in legs}
    for _ in range(runs):
        for name, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize(dev)
            ms[name].append(a.elapsed_time(b))
    return {k: {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": runs} for k, v in ms.items()}


def measure(n, size, runs, dev):
    w, h = size
    fsz = vp8g.i420_size(w, h)
    gen = torch.Generator(device=dev)
    gen.manual_seed(w * 131 + h)
    src = torch.randint(0, 256, (n * fsz + 16,), dtype=torch.uint8, device=dev, generator=gen)
    host_frames = {i: src[i * fsz:(i + 1) * fsz].cpu().numpy().tobytes() for i in (0, n - 1)}
    stream = torch.cuda.current_stream(dev).cuda_stream
    routes = {k: Route(k, src, n, size, dev) for k in ("i420", "rgb444")}
    legs = []
    for k, r in routes.items():
        legs += [(k, lambda r=r: r.both(stream)), (k + "_scale_only", lambda r=r: r.scale(stream))]
    row = {"frames": n, "source": [w, h], "target": list(TARGET), "source_bytes": n * fsz, **timed_interleaved(legs, runs, dev)}
    for k, r in routes.items():
        r.both(stream)
        torch.cuda.synchronize(dev)
        row[k].update({"intermediate_bytes": n * r.mid_bytes, "scale_tasks": r.scale_tasks, "tensor_tasks": r.tensor_tasks,
                       "expanding_planes": r.expand_planes,
                       "parity": "bit-exact vs host restatement (2 pictures)" if r.parity(host_frames, size) else "MISMATCH"})
    row["rgb444_over_i420"] = round(row["rgb444"]["ms"] / row["i420"]["ms"], 3)
    return row


def table(res) -> str:
    rows = ["| pictures -> 224x224 float16 NCHW | I420 route | libwebp-RGB route | ratio | scale launch alone (I420 / RGB) | note |",
            "|---|---|---|---|---|---|"]
    for r in res["legs"]:
        a, b = r["i420"], r["rgb444"]
        rows.append(f"| {r['frames']} x {r['source'][0]}x{r['source'][1]} | {a['ms']} ms ({a['min']} .. {a['max']}) | {b['ms']} ms ({b['min']} .. {b['max']}) | "
                    f"{r['rgb444_over_i420']} | {r['i420_scale_only']['ms']} / {r['rgb444_scale_only']['ms']} ms | "
                    f"{b['expanding_planes']} of {3 * r['frames']} planes expand; {a['parity'] if a['parity'] == b['parity'] else 'MISMATCH'} |")
    return "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scale_rgb_bench.json"))
    args = ap.parse_args()
    if args.runs < 10:
        ap.error("--runs >= 10")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "tensor": "float16 NCHW, ImageNet mean / std", "legs": []}
    for size in ((3840, 2160), (640, 480), (400, 300)):
        res["legs"].append(measure(args.frames, size, args.runs, dev))
        torch.cuda.empty_cache()
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(table(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
