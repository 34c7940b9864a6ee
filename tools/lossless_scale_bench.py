#!/usr/bin/env python3
"""Measure the scaled lossless path on one MI355X, in one process, by §17.6's protocol: HIP events
for device time, the cold run discarded, median (min .. max) of the warm runs, every timed configuration compared with
the host's bytes first.

(a) Kernels: N random ARGB pictures of 1920x1080 and N of 3840x2160 -> 224x224 (four distinct pictures, copied on the
    device: every picture has source bytes, work planes and an output of its own; alpha half uniform, half from
    {0, 1, 2, 127, 128, 254, 255}).
      device   vp8g_scale_argb_batch_device, one call over the N device-resident pictures (split, rescaler, merge);
      rescaler vp8g_scale_batch_device alone over the same 4 N planes (left in the work buffer by the call before);
               the call's time less this one is what the planar route adds: the split and merge passes;
      host     vp8f_argb_scale over the same N pictures on 16 threads; wall ms.
    --trace runs only the device calls (for a kernel trace in a run of its own, which names the three kernels' times).
(b) End to end: --e2e-frames 4K lossless files (the two streams of tests/golden/lossless_bench/, alternating) through
    vp8g_decode_webp_batch_tensor_any into a float16 NHWC RGBA tensor: 224x224 with VP8G_X_LOSSLESS_SCALE, beside the
    same files at their own size without it.

Writes profiles/lossless_scale_bench.json (or --out) and prints its rows.

  python tools/lossless_scale_bench.py [--images 256] [--runs 9] [--threads 16] [--e2e-frames 64] [--e2e-runs 9] [--trace]
                                       [--out PATH]
"""
import argparse
import ctypes as C
import hashlib
import json
import pathlib
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: its HIP runtime serves the process, as in bench.py)

import vp8g  # noqa: E402

TARGET = (224, 224)


def summary(ms, nd=3):
    return {"median": round(statistics.median(ms), nd), "min": round(min(ms), nd), "max": round(max(ms), nd), "runs": len(ms)}


def random_argb(rng, w, h):
    px = rng.integers(0, 1 << 24, (h, w), dtype=np.uint64).astype(np.uint32)
    edge = rng.choice(np.array([0, 1, 2, 127, 128, 254, 255], np.uint32), (h, w))
    uni = rng.integers(0, 256, (h, w)).astype(np.uint32)
    return px | np.where(rng.integers(0, 2, (h, w)) == 1, edge, uni) << 24


class DeviceLeg:
    def __init__(self, pics, opt, n, dev):
        self.lib, self.n = vp8g.gpu_lib(), n
        h, w = pics[0].shape
        # every picture has source bytes of its own (copies made on the device), so the split reads from memory, not from
        # four pictures' worth of cache
        assert n % len(pics) == 0
        self.src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pics]).view(np.uint8)).to(dev).repeat(n // len(pics))
        self.descs = (vp8g.Vp8gScaleArgbDesc * n)()
        wo, do = int(self.lib.vp8g_scale_argb_head_size(n)), 0
        planes = ts = tr = tm = 0
        for i in range(n):
            d = self.descs[i]
            assert self.lib.vp8g_make_scale_argb_desc(w, h, i * 4 * w * h, C.byref(opt), wo, do, planes, ts, tr, tm, C.byref(d)) == 0
            planes, ts, tr, tm = planes + d.nplanes, ts + d.split_ntasks, tr + d.scale_ntasks, tm + d.merge_ntasks
            wo += (d.work_bytes + 255) // 256 * 256
            do += (4 * d.width * d.height + 255) // 256 * 256
        self.work = torch.zeros(wo, dtype=torch.uint8, device=dev)
        self.dst = torch.zeros(do, dtype=torch.uint8, device=dev)
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.planes = (vp8g.Vp8gScaleDesc * planes)(*[self.descs[i].plane[c] for i in range(n) for c in range(4)])

    def launch(self, stream):
        if self.lib.vp8g_scale_argb_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n, C.c_void_p(self.src.data_ptr()),
                                                 C.c_void_p(self.work.data_ptr()), C.c_void_p(self.dst.data_ptr()), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_scale_argb_batch_device: {self.lib.vp8g_last_error()!r}")

    def launch_rescaler(self, stream):
        w = C.c_void_p(self.work.data_ptr())  # (its head holds the plane descriptors since the first launch)
        if self.lib.vp8g_scale_batch_device(self.planes, w, len(self.planes), w, w, C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_scale_batch_device: {self.lib.vp8g_last_error()!r}")

    def image(self, i):
        d = self.descs[i]
        return self.dst[d.dst:d.dst + 4 * d.width * d.height].cpu().numpy().view(np.uint32).reshape(d.height, d.width)


def timed(fn, stream, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn(stream.cuda_stream)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def host_run(pics, opt, n, threads, outs):
    lib = vp8g.host_lib()
    h, w = pics[0].shape

    def work(t):
        for i in range(t, n, threads):
            lib.vp8f_argb_scale(pics[i % len(pics)].ctypes.data, w, h, C.byref(opt), outs[t].ctypes.data)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return (time.perf_counter() - t0) * 1e3


def kernel_rows(a, dev, stream):
    rows = []
    opt = vp8g.scale_opt(scale=TARGET)
    for w, h in ((1920, 1080), (3840, 2160)):
        rng = np.random.default_rng(w)
        pics = [random_argb(rng, w, h) for _ in range(4)]
        leg = DeviceLeg(pics, opt, a.images, dev)
        leg.launch(stream.cuda_stream)  # cold
        torch.cuda.synchronize(dev)
        for i in (0, 1, a.images - 1):
            assert np.array_equal(leg.image(i), vp8g.host_scale_argb(pics[i % 4], opt)), (w, h, i)
        if a.trace:
            for _ in range(a.runs):
                leg.launch(stream.cuda_stream)
            torch.cuda.synchronize(dev)
            del leg
            continue
        outs = [np.empty((TARGET[1], TARGET[0]), np.uint32) for _ in range(a.threads)]
        host_run(pics, opt, a.images, a.threads, outs)  # cold
        timed(leg.launch_rescaler, stream, dev)
        dms, sms, hms = [], [], []
        for _ in range(a.runs):
            dms.append(timed(leg.launch, stream, dev))
            sms.append(timed(leg.launch_rescaler, stream, dev))
            hms.append(host_run(pics, opt, a.images, a.threads, outs))
        assert np.array_equal(leg.image(a.images - 1), vp8g.host_scale_argb(pics[(a.images - 1) % 4], opt))
        d, s, hs = summary(dms), summary(sms), summary(hms, 1)
        mpx = a.images * w * h / 1e6
        # what the passes move: the split reads 4 and writes 4 bytes per window pixel, the rescaler reads those 4 again
        row = {"size": [w, h], "target": list(TARGET), "images": a.images, "device_ms": d, "rescaler_alone_ms": s,
               "split_plus_merge_ms": round(d["median"] - s["median"], 3), "host_ms": hs, "host_threads": a.threads,
               "device_mpx_per_s": round(mpx / d["median"] * 1e3, 1), "host_mpx_per_s": round(mpx / hs["median"] * 1e3, 1),
               "device_over_host": round(hs["median"] / d["median"], 2),
               "split_bytes_per_s": round(8 * mpx * 1e6 / ((d["median"] - s["median"]) * 1e-3)) if d["median"] > s["median"] else None}
        rows.append(row)
        print(f"{w}x{h} x{a.images} -> {TARGET[0]}x{TARGET[1]}: device {d['median']:.3f} ms ({d['min']:.3f} .. {d['max']:.3f}), rescaler alone "
              f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f}) | host x{a.threads} {hs['median']:.1f} ms ({hs['min']:.1f} .. {hs['max']:.1f}) | "
              f"x{row['device_over_host']}", flush=True)
        del leg
    torch.cuda.empty_cache()
    return rows


def e2e_leg(a, dev):
    W, H, n = 3840, 2160, a.e2e_frames
    names = sorted(json.loads((ROOT / "tests" / "golden" / "lossless.json").read_text())["bench"])
    streams = [(ROOT / "tests" / "golden" / "lossless_bench" / f"{name}.webp").read_bytes() for name in names]
    files = [streams[i % len(streams)] for i in range(n)]
    bufs = [(C.c_uint8 * len(b)).from_buffer_copy(b) for b in files]
    spans = (vp8g.ByteSpan * n)(*[vp8g.ByteSpan(C.cast(bufs[i], C.POINTER(C.c_uint8)), len(bufs[i])) for i in range(n)])
    lib = vp8g.gpu_lib()
    small, full = vp8g.tensor_opt(TARGET, "float16", "NHWC"), vp8g.tensor_opt((W, H), "float16", "NHWC")
    o = vp8g.scale_opt(scale=TARGET)
    out_s = torch.empty((n, TARGET[1], TARGET[0], 4), dtype=torch.float16, device=dev)
    out_f = torch.empty((n, H, W, 4), dtype=torch.float16, device=dev)
    torch.cuda.synchronize(dev)

    def call(scaled):
        st = (C.c_int * n)()
        xf = vp8g.VP8G_X_LOSSLESS | vp8g.VP8G_X_ALPHA | (vp8g.VP8G_X_LOSSLESS_SCALE if scaled else 0)
        t0 = time.perf_counter()
        rc = lib.vp8g_decode_webp_batch_tensor_any(spans, n, 1, a.threads, 0, C.byref(o) if scaled else None, 1 if scaled else 0,
                                                   C.byref(small if scaled else full), xf,
                                                   C.c_void_p((out_s if scaled else out_f).data_ptr()), st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"vp8g_decode_webp_batch_tensor_any failed: {list(st)[:4]} {lib.vp8g_last_error()!r}")
        return dt

    call(True), call(False)  # cold
    for i in (0, 1, n - 1):  # the scaled tensor against the host's: decode, vp8f_argb_scale, the tensor restatement
        want = vp8g.host_tensor_argb(vp8g.host_scale_argb(vp8g.host_lossless_argb(files[i]), o), small, 4)
        assert torch.equal(out_s[i].cpu().view(torch.uint8), want.view(torch.uint8)), i
    runs = [[], []]
    for _ in range(a.e2e_runs):
        runs[0].append(call(True))
        runs[1].append(call(False))
    rs, rf = summary(runs[0]), summary(runs[1])
    print(f"end to end, {n} 4K lossless files, {a.threads} threads -> float16 NHWC RGBA: {TARGET[0]}x{TARGET[1]} with VP8G_X_LOSSLESS_SCALE "
          f"{rs['median']} s ({rs['min']} .. {rs['max']}) | full size {rf['median']} s ({rf['min']} .. {rf['max']})", flush=True)
    return {"frames": n, "threads": a.threads, "stream_bytes": [len(b) for b in streams], "scaled_224_s": rs, "full_size_s": rf,
            "scaled_equals_host": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--e2e-frames", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="only the device calls of (a), for a kernel trace; writes nothing")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lossless_scale_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = kernel_rows(a, dev, stream)
    if a.trace:
        return
    e2e = e2e_leg(a, dev)
    srcs = sorted((ROOT / "webp-decoder_amd").glob("csrc/*")) + sorted((ROOT / "webp-decoder_amd").glob("host/*")) + [ROOT / "include" / "vp8g.h"]
    tree = hashlib.sha256(b"".join(hashlib.sha256(p.read_bytes()).digest() for p in srcs)).hexdigest()[:16]
    doc = {"tool": "tools/lossless_scale_bench.py", "device": torch.cuda.get_device_name(0),
           "build": f"sources sha256 {tree} (csrc/*, host/*, include/vp8g.h)",
           "timing": "HIP events (device), perf_counter (host, end to end); cold run discarded; median, min .. max",
           "rows": rows, "end_to_end": e2e}
    out = pathlib.Path(a.out)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
