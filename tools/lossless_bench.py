#!/usr/bin/env python3
"""Measure the lossless (VP8L) path on one MI355X, in one process.

Transform kernel, on N images of 1920x1080 and N of 3840x2160, synthetic (no stream): four distinct random ARGB
residuals, replicated, with a uniformly random mode image (every predictor mode, lanes of a wave in different
modes) and the stream order subtract green, predictor, cross colour with 32-pixel blocks, whose inverse -- cross
colour, predictor, add green -- the kernel runs as one fused pass (8 bytes moved per pixel).  Neither side's time
depends on the pixel values, only on the predictor's mode mix, so random residuals favour nobody.
  device  vp8g_lossless_batch_device, one launch over the N device-resident images; HIP-event ms, the cold first
          launch discarded, then the median of the warm runs with min .. max.
  host    vp8f_lossless_apply over the same N images on 16 threads (each thread its share, into a buffer of its
          own); wall ms, same statistics, same run.
One image per size is compared with the host's pixels before anything is timed.

End to end: --e2e-frames 4K lossless files (the two streams of tests/golden/lossless_bench/, alternating) into a
3840x2160 uint8 NHWC RGBA tensor through vp8g_decode_webp_batch_tensor_any(VP8G_X_LOSSLESS | VP8G_X_ALPHA), beside
the host's vp8f_lossless_decode (the entropy half) alone on the same number of threads.

Writes profiles/lossless_bench.json and prints its rows.

  python tools/lossless_bench.py [--images 256] [--runs 9] [--threads 16] [--e2e-frames 64] [--e2e-runs 9] [--build ID]
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

BITS = 5


def summary(ms, nd=3):
    return {"median": round(statistics.median(ms), nd), "min": round(min(ms), nd), "max": round(max(ms), nd), "runs": len(ms)}


def synth(rng, w, h):
    shape = ((h + (1 << BITS) - 1) >> BITS, (w + (1 << BITS) - 1) >> BITS)
    rnd = lambda s: rng.integers(0, 1 << 32, s, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    modes = (rnd(shape) & np.uint32(0xFFFF00FF)) | (rng.integers(0, 14, shape).astype(np.uint32) << 8)
    return vp8g.lossless_image(rnd((h, w)), [{"type": vp8g.L_SUBTRACT_GREEN, "bits": 0},
                                             {"type": vp8g.L_PREDICTOR, "bits": BITS, "data": modes},
                                             {"type": vp8g.L_CROSS_COLOR, "bits": BITS, "data": rnd(shape)}])


class DeviceLeg:
    """N images on the device: the four distinct ones' residuals and transform data uploaded once each; image i reads
    those of i % 4 and writes a buffer of its own."""

    def __init__(self, images, w, h, n, dev):
        self.lib, self.n, self.w, self.h = vp8g.gpu_lib(), n, w, h
        parts, offs, so = [], [], 0
        for im in images:
            o = []
            for a in [im["residual"]] + [t["data"] for t in im["transforms"]]:
                b = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.uint8)
                o.append(so)
                parts.append(b)
                so += b.size
            offs.append(o)
        self.src = torch.from_numpy(np.concatenate(parts)).to(dev)
        self.dst = torch.zeros(n * w * h, dtype=torch.int32, device=dev)
        self.descs = (vp8g.Vp8gLosslessDesc * n)()
        for i in range(n):
            im, o = images[i % len(images)], offs[i % len(images)]
            tr = (vp8g.Vp8gLosslessTransform * 4)(*[vp8g.Vp8gLosslessTransform(o[1 + k], t["type"], t["bits"], t["xsize"], t["ncolors"])
                                                    for k, t in enumerate(im["transforms"])])
            assert self.lib.vp8g_make_lossless_desc(w, h, o[0], 4 * i * w * h, len(im["transforms"]), tr, i, C.byref(self.descs[i])) == 0
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)

    def launch(self, stream):
        if self.lib.vp8g_lossless_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n, C.c_void_p(self.src.data_ptr()),
                                               C.c_void_p(self.dst.data_ptr()), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_lossless_batch_device: {self.lib.vp8g_last_error()!r}")

    def image(self, i):
        return self.dst[i * self.w * self.h:(i + 1) * self.w * self.h].cpu().numpy().view(np.uint32).reshape(self.h, self.w)


def host_run(structs, n, threads, outs):
    lib = vp8g.host_lib()

    def work(t):
        for i in range(t, n, threads):
            lib.vp8f_lossless_apply(C.byref(structs[i % len(structs)][0]), outs[t].ctypes.data)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return (time.perf_counter() - t0) * 1e3


def e2e_leg(a, dev):
    W, H, n = 3840, 2160, a.e2e_frames
    golden = json.loads((ROOT / "tests" / "golden" / "lossless.json").read_text())["bench"]
    streams = [(ROOT / "tests" / "golden" / "lossless_bench" / f"{name}.webp").read_bytes() for name in sorted(golden)]
    files = [streams[i % len(streams)] for i in range(n)]
    bufs = [(C.c_uint8 * len(b)).from_buffer_copy(b) for b in files]
    spans = (vp8g.ByteSpan * n)(*[vp8g.ByteSpan(C.cast(bufs[i], C.POINTER(C.c_uint8)), len(bufs[i])) for i in range(n)])
    lib, host = vp8g.gpu_lib(), vp8g.host_lib()
    topt = vp8g.tensor_opt((W, H), "uint8", "NHWC")
    out = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def tensor():
        st = (C.c_int * n)()
        t0 = time.perf_counter()
        rc = lib.vp8g_decode_webp_batch_tensor_any(spans, n, 1, a.threads, 0, None, 0, C.byref(topt),
                                                   vp8g.VP8G_X_LOSSLESS | vp8g.VP8G_X_ALPHA, C.c_void_p(out.data_ptr()), st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"vp8g_decode_webp_batch_tensor_any failed: {lib.vp8g_last_error()!r}")
        return dt

    def entropy_only():
        def work(t):
            for i in range(t, n, a.threads):
                c = vp8g.WebPContainerL()
                im = vp8g.Vp8fLosslessImage()
                if host.webp_parse_any(spans[i], C.byref(c)) != 0 or not c.vp8l_chunk_offset:
                    raise RuntimeError("webp_parse_any failed")
                if host.vp8f_lossless_decode(C.cast(bufs[i], C.c_void_p).value + c.vp8l_chunk_offset, c.vp8l_chunk_size, C.byref(im),
                                             None) != 0:
                    raise RuntimeError("vp8f_lossless_decode failed")
                host.vp8f_lossless_free(C.byref(im))

        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            list(ex.map(work, range(a.threads)))
        return time.perf_counter() - t0

    tensor(), entropy_only()  # cold
    same = all(hashlib.sha256(out[i].cpu().numpy().tobytes()).hexdigest() == golden[sorted(golden)[i % len(streams)]]["rgba"]
               for i in (0, 1, n - 1))
    runs = [[], []]
    for _ in range(a.e2e_runs):
        runs[0].append(tensor())
        runs[1].append(entropy_only())
    rt, re_ = summary(runs[0]), summary(runs[1])
    rt["equals_libwebp_rgba"] = same
    print(f"end to end, {n} 4K lossless files, {a.threads} threads -> uint8 NHWC RGBA tensor: {rt['median']} s ({rt['min']} .. {rt['max']}) | "
          f"vp8f_lossless_decode alone {re_['median']} s ({re_['min']} .. {re_['max']}); equal to libwebp {same}", flush=True)
    return {"frames": n, "threads": a.threads, "stream_bytes": [len(b) for b in streams], "tensor_s": rt, "entropy_decode_alone_s": re_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--e2e-frames", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=9)
    ap.add_argument("--build", default="", help="what was measured (a commit id or source hash), recorded in the output")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        rng = np.random.default_rng(w)
        images = [synth(rng, w, h) for _ in range(4)]
        structs = [vp8g.lossless_struct(im) for im in images]
        outs = [np.empty((h, w), np.uint32) for _ in range(a.threads)]
        leg = DeviceLeg(images, w, h, a.images, dev)
        leg.launch(stream.cuda_stream)  # cold
        torch.cuda.synchronize(dev)
        for i in (0, 1, a.images - 1):
            assert np.array_equal(leg.image(i), vp8g.host_lossless_apply(images[i % 4])), (w, h, i)
        dms, hms = [], []
        host_run(structs, a.images, a.threads, outs)  # cold
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            leg.launch(stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            dms.append(e0.elapsed_time(e1))
            hms.append(host_run(structs, a.images, a.threads, outs))
        d, hs = summary(dms), summary(hms, 1)
        mpx = a.images * w * h / 1e6
        row = {"size": [w, h], "images": a.images, "transforms": "stream order subtract green, predictor, cross colour (one fused pass); 32-pixel blocks; modes 0..13 uniform",
               "device_ms": d, "host_ms": hs, "host_threads": a.threads, "device_mpx_per_s": round(mpx / d["median"] * 1e3, 1),
               "host_mpx_per_s": round(mpx / hs["median"] * 1e3, 1), "device_over_host": round(hs["median"] / d["median"], 2)}
        rows.append(row)
        print(f"{w}x{h} x{a.images} device {d['median']:9.3f} ms ({d['min']:.3f} .. {d['max']:.3f}) {row['device_mpx_per_s']:9.1f} Mpx/s | "
              f"host x{a.threads} {hs['median']:9.1f} ms ({hs['min']:.1f} .. {hs['max']:.1f}) {row['host_mpx_per_s']:8.1f} Mpx/s | "
              f"x{row['device_over_host']}", flush=True)
        del leg
    torch.cuda.empty_cache()
    e2e = e2e_leg(a, dev)
    srcs = sorted((ROOT / "webp-decoder_amd").glob("csrc/*")) + sorted((ROOT / "webp-decoder_amd").glob("host/*")) + [ROOT / "include" / "vp8g.h"]
    tree = hashlib.sha256(b"".join(hashlib.sha256(p.read_bytes()).digest() for p in srcs)).hexdigest()[:16]
    doc = {"tool": "tools/lossless_bench.py", "device": torch.cuda.get_device_name(0),
           "build": a.build or f"sources sha256 {tree} (csrc/*, host/*, include/vp8g.h)", "sources_sha256": tree,
           "timing": "HIP events (device), perf_counter (host); cold run discarded; median, min .. max",
           "rows": rows, "end_to_end": e2e}
    out = ROOT / "profiles" / "lossless_bench.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
