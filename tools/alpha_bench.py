#!/usr/bin/env python3
"""Measure the alpha un-prediction on one MI355X, in one process.

Per filter (0 none, 1 horizontal, 2 vertical, 3 gradient), on N planes of 3840x2160 and N of 224x224:
  device  vp8g_alpha_unfilter_batch_device, one launch over the N device-resident residual planes (four
          distinct random planes, replicated); HIP-event ms, the cold first launch discarded, then the median of
          the warm runs with min .. max; GB/s read + written against the achievable HBM rate.
  host    vp8f_alpha_unfilter over the same N planes on 16 threads (each thread un-predicts its share of the
          planes, from the four distinct ones, into a buffer of its own); wall ms, same statistics, same run.
One plane per filter and size is compared with the host's bytes before anything is timed.

End to end: --e2e-frames 4K files with alpha -- the VP8 payloads of the four UHD fixtures
wrapped as VP8X + ALPH + VP8 with the ALPH payloads of tests/golden/alpha_bench/ (libwebp's alpha encoder on a
soft-edged disc, 112 KB, and on a ramp, 0.5 KB) -- into 224x224 float16 NCHW RGBA through
vp8g_decode_webp_batch_tensor_x(VP8G_X_ALPHA), beside the same VP8 payloads re-wrapped as simple files through
vp8g_decode_webp_batch_tensor (3 channels) of --parent-lib (a libvp8g.so built from the parent commit, loaded
side by side; without it this tree's library); one input buffer per frame, the same buffers' payloads for
both legs, the legs alternating call by call, and the host's vp8f_alpha_decode alone on the same threads.

Writes profiles/alpha_bench.json (with --build, the source it measured) and prints the table of DESIGN.md §16.

  python tools/alpha_bench.py [--planes 512] [--runs 9] [--threads 16] [--e2e-frames 256] [--e2e-runs 9]
                              [--parent-lib PATH] [--build ID]
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

HBM_ACHIEVABLE_TBS = 6.29  # the achievable HBM read rate the microarchitecture notes give for this part
FILTERS = ("none", "horizontal", "vertical", "gradient")


def summary(ms, nd=3):
    return {"median": round(statistics.median(ms), nd), "min": round(min(ms), nd), "max": round(max(ms), nd), "runs": len(ms)}


class DeviceLeg:
    def __init__(self, planes, w, h, n, flt, dev):
        self.lib, self.n, self.w, self.h = vp8g.gpu_lib(), n, w, h
        k = len(planes)
        self.src = torch.empty(n * w * h, dtype=torch.uint8, device=dev)
        view = self.src.view(n, w * h)
        for j, p in enumerate(planes):
            view[j::k] = torch.from_numpy(p.reshape(-1)).to(dev)
        self.dst = torch.zeros(n * w * h, dtype=torch.uint8, device=dev)
        self.descs = (vp8g.Vp8gAlphaDesc * n)()
        for i in range(n):
            assert self.lib.vp8g_make_alpha_desc(w, h, flt, i * w * h, w, i * w * h, w, i, C.byref(self.descs[i])) == 0
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)

    def launch(self, stream):
        if self.lib.vp8g_alpha_unfilter_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n,
                                                     C.c_void_p(self.src.data_ptr()), C.c_void_p(self.dst.data_ptr()),
                                                     C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_alpha_unfilter_batch_device: {self.lib.vp8g_last_error()!r}")

    def plane(self, i):
        return self.dst[i * self.w * self.h:(i + 1) * self.w * self.h].cpu().numpy().reshape(self.h, self.w)


def host_run(planes, w, h, n, flt, threads, outs):
    lib = vp8g.host_lib()

    def work(t):
        for i in range(t, n, threads):
            lib.vp8f_alpha_unfilter(planes[i % len(planes)].ctypes.data, w, h, flt, outs[t].ctypes.data)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return (time.perf_counter() - t0) * 1e3


UHD = ["big/uhd_a_normal_seg4.webp", "big/uhd_b_simple_sharp3.webp", "big/uhd_c_normal_sharp6_seg1.webp",
       "big/uhd_d_normal_q90.webp"]
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def chunk(tag, payload):
    return tag + len(payload).to_bytes(4, "little") + payload + (b"\0" if len(payload) & 1 else b"")


def riff(body):
    return b"RIFF" + (len(body) + 4).to_bytes(4, "little") + b"WEBP" + body


def e2e_legs(a, dev):
    W, H, n = 3840, 2160, a.e2e_frames
    golden = json.loads((ROOT / "tests" / "golden" / "alpha.json").read_text())["bench"]
    alphs = []
    for name, e in sorted(golden.items()):
        b = (ROOT / "tests" / "golden" / "alpha_bench" / f"{name}.alph").read_bytes()
        res, flt, _ = vp8g.alpha_decode_host(b, W, H)
        assert hashlib.sha256(vp8g.host_alpha_unfilter(res, flt).tobytes()).hexdigest() == e["a"], name
        alphs.append(b)
    payloads = []
    for r in UHD:
        f = (ROOT / "tests" / "fixtures" / r).read_bytes()
        off, size = vp8g.parse_simple(f)
        payloads.append(f[off:off + size])
    vp8x = chunk(b"VP8X", bytes([0x10, 0, 0, 0]) + (W - 1).to_bytes(3, "little") + (H - 1).to_bytes(3, "little"))
    rgba_files = [riff(vp8x + chunk(b"ALPH", alphs[(i // 4) % len(alphs)]) + chunk(b"VP8 ", payloads[i % 4])) for i in range(n)]
    rgb_files = [riff(chunk(b"VP8 ", payloads[i % 4])) for i in range(n)]

    def spans_of(files):
        bufs = [(C.c_uint8 * len(b)).from_buffer_copy(b) for b in files]
        return bufs, (vp8g.ByteSpan * n)(*[vp8g.ByteSpan(C.cast(bufs[i], C.POINTER(C.c_uint8)), len(bufs[i])) for i in range(n)])

    keep_a, spans_a = spans_of(rgba_files)
    keep_b, spans_b = spans_of(rgb_files)
    lib = vp8g.gpu_lib()
    parent = C.CDLL(str(pathlib.Path(a.parent_lib).resolve()), use_errno=True) if a.parent_lib else lib
    P = C.POINTER
    parent.vp8g_decode_webp_batch_tensor.argtypes = [P(vp8g.ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                     P(vp8g.Vp8gScaleOpt), C.c_uint32, P(vp8g.Vp8gTensorOpt), C.c_void_p, P(C.c_int)]
    sopt = vp8g.scale_opt(scale=(224, 224))
    topt = vp8g.tensor_opt((224, 224), "float16", "NCHW", **IMAGENET)
    out4 = torch.empty((n, 4, 224, 224), dtype=torch.float16, device=dev)
    out3 = torch.empty((n, 3, 224, 224), dtype=torch.float16, device=dev)
    torch.cuda.synchronize(dev)

    def rgba():
        st = (C.c_int * n)()
        t0 = time.perf_counter()
        rc = lib.vp8g_decode_webp_batch_tensor_x(spans_a, n, 1, a.threads, 0, C.byref(sopt), 1, C.byref(topt), vp8g.VP8G_X_ALPHA,
                                                 C.c_void_p(out4.data_ptr()), st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"vp8g_decode_webp_batch_tensor_x failed: {lib.vp8g_last_error()!r}")
        return dt

    def rgb():
        st = (C.c_int * n)()
        t0 = time.perf_counter()
        rc = parent.vp8g_decode_webp_batch_tensor(spans_b, n, 1, a.threads, 0, C.byref(sopt), 1, C.byref(topt),
                                                  C.c_void_p(out3.data_ptr()), st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError("vp8g_decode_webp_batch_tensor (parent leg) failed")
        return dt

    def alpha_only():  # the ALPH entropy decode of the batch alone, on the same number of host threads
        host = vp8g.host_lib()
        res = [np.empty(W * H, np.uint8) for _ in range(a.threads)]

        def work(t):
            flt = C.c_uint32()
            for i in range(t, n, a.threads):
                b = alphs[(i // 4) % len(alphs)]
                host.vp8f_alpha_decode(b, len(b), W, H, res[t].ctypes.data, C.byref(flt), None)

        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            list(ex.map(work, range(a.threads)))
        return time.perf_counter() - t0

    rgb(), rgba(), alpha_only()  # cold
    same_rgb = bool(torch.equal(out4[:, :3].contiguous().view(torch.int16), out3.view(torch.int16)))
    exp_a = vp8g.host_alpha_channel(vp8g.host_scale_plane(vp8g.host_alpha_unfilter(*vp8g.alpha_decode_host(alphs[0], W, H)[:2]), sopt), topt)
    same_a = bool(torch.equal(out4[0, 3].cpu().view(torch.int16), exp_a.view(torch.int16)))
    runs = [[], [], []]
    for _ in range(a.e2e_runs):
        runs[0].append(rgb())
        runs[1].append(rgba())
        runs[2].append(alpha_only())
    r3, r4, ra = summary(runs[0]), summary(runs[1]), summary(runs[2])
    r3["library"] = "parent build (--parent-lib)" if a.parent_lib else "this tree"
    r4.update({"over_rgb_median": round(r4["median"] / r3["median"], 3), "rgb_channels_equal_rgb_leg": same_rgb,
               "alpha_channel_equals_host": same_a})
    print(f"end to end, {n} 4K files, {a.threads} threads -> 224x224 float16 NCHW: RGB ({r3['library']}) {r3['median']} s "
          f"({r3['min']} .. {r3['max']}) | RGBA {r4['median']} s ({r4['min']} .. {r4['max']}) = x{r4['over_rgb_median']} | "
          f"vp8f_alpha_decode alone {ra['median']} s ({ra['min']} .. {ra['max']}); RGB equal {same_rgb}, A equal {same_a}", flush=True)
    return {"frames": n, "threads": a.threads, "alph_payload_bytes": [len(b) for b in alphs], "rgb_224_f16_nchw_s": r3,
            "rgba_224_f16_nchw_s": r4, "alpha_decode_alone_s": ra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--e2e-frames", type=int, default=256)
    ap.add_argument("--e2e-runs", type=int, default=9)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--build", default="", help="what was measured (a commit id or source hash), recorded in the output")
    a = ap.parse_args()
    assert a.runs >= 9 and a.e2e_runs >= 9
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = []
    for w, h in ((3840, 2160), (224, 224)):
        rng = np.random.default_rng(w)
        planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(4)]
        outs = [np.empty((h, w), np.uint8) for _ in range(a.threads)]
        nbytes = 2 * a.planes * w * h
        for flt in range(4):
            leg = DeviceLeg(planes, w, h, a.planes, flt, dev)
            leg.launch(stream.cuda_stream)  # cold
            torch.cuda.synchronize(dev)
            for i in (0, 1, a.planes - 1):
                assert np.array_equal(leg.plane(i), vp8g.host_alpha_unfilter(planes[i % 4], flt)), (w, h, flt, i)
            dms, hms = [], []
            host_run(planes, w, h, a.planes, flt, a.threads, outs)  # cold
            for _ in range(a.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                leg.launch(stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                dms.append(e0.elapsed_time(e1))
                hms.append(host_run(planes, w, h, a.planes, flt, a.threads, outs))
            d, hs = summary(dms), summary(hms, 1)
            row = {"size": [w, h], "planes": a.planes, "filter": FILTERS[flt], "device_ms": d, "host_ms": hs,
                   "host_threads": a.threads, "device_gbs": round(nbytes / d["median"] / 1e6, 1),
                   "device_pct_of_hbm": round(100 * nbytes / d["median"] / 1e6 / (HBM_ACHIEVABLE_TBS * 1e3), 1),
                   "host_gbs": round(nbytes / hs["median"] / 1e6, 2), "device_over_host": round(hs["median"] / d["median"], 1)}
            rows.append(row)
            print(f"{w}x{h} x{a.planes} {FILTERS[flt]:10s} device {d['median']:9.3f} ms ({d['min']:.3f} .. {d['max']:.3f}) "
                  f"{row['device_gbs']:8.1f} GB/s {row['device_pct_of_hbm']:5.1f}% | host x{a.threads} {hs['median']:9.1f} ms "
                  f"({hs['min']:.1f} .. {hs['max']:.1f}) {row['host_gbs']:7.2f} GB/s | x{row['device_over_host']}", flush=True)
            del leg
    torch.cuda.empty_cache()
    e2e = e2e_legs(a, dev)
    srcs = sorted((ROOT / "webp-decoder_amd").glob("csrc/*")) + sorted((ROOT / "webp-decoder_amd").glob("host/*")) + [ROOT / "include" / "vp8g.h"]
    tree = hashlib.sha256(b"".join(hashlib.sha256(p.read_bytes()).digest() for p in srcs)).hexdigest()[:16]
    doc = {"tool": "tools/alpha_bench.py", "device": torch.cuda.get_device_name(0),
           "build": a.build or f"sources sha256 {tree} (csrc/*, host/*, include/vp8g.h)", "sources_sha256": tree,
           "hbm_achievable_tbs": HBM_ACHIEVABLE_TBS, "timing": "HIP events (device), perf_counter (host); cold run discarded; median, min .. max",
           "rows": rows, "end_to_end": e2e}
    out = ROOT / "profiles" / "alpha_bench.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
