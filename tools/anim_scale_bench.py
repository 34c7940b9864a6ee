#!/usr/bin/env python3
"""Measure the scaled animation path on one MI355X, in one process, by the protocol of §17.6 and §17.7:
HIP events for device time, the cold run discarded, median (min .. max) of the warm runs, every timed configuration
compared with the host's bytes first.

(a) The fused call against the planar route, alternating in the same process: N random ARGB pictures of 1920x1080 and
    N of 3840x2160 -> 224x224 uint8 NHWC RGBA (four distinct pictures, copied on the device: every picture has source
    bytes and a slot of its own; alpha half uniform, half from {0, 1, 2, 127, 128, 254, 255} -- §17.7's rows).
      planar  vp8g_scale_argb_batch_device, then vp8g_tensor_batch_device_argb on the same stream (five launches, a work
              buffer);
      fused   vp8g_scale_argb_tensor_batch_device (one launch).
    The baseline is the planar route as measured in this run.  "condition_met": the fused median is below the planar
    median and their (min .. max) ranges do not overlap.
(b) End to end, reported only: --e2e-files animated files of 16 lossless frames on a 512 x 512 canvas (assembled in
    memory from the streams of tests/golden/lossless/, as tools/anim_bench.py does) through
    vp8g_decode_webp_anim_tensor_scaled into a 224 x 224 float16 NHWC RGBA tensor, beside vp8g_decode_webp_anim_tensor on
    the same files at the canvas size; wall s.  The host's entropy decode of the frames dominates both.

Writes profiles/anim_scale_bench.json (or --out) and prints its rows.

  python tools/anim_scale_bench.py [--images 256] [--runs 9] [--threads 16] [--e2e-files 64] [--e2e-runs 5] [--out PATH]
"""
import argparse
import ctypes as C
import hashlib
import json
import pathlib
import statistics
import struct
import sys

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


class Legs:
    """The same N device-resident pictures through both routes, each into a [N, 224, 224, 4] uint8 tensor of its own."""

    def __init__(self, pics, opt, n, dev):
        self.lib, self.n = vp8g.gpu_lib(), n
        lib = self.lib
        h, w = pics[0].shape
        assert n % len(pics) == 0
        self.src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pics]).view(np.uint8)).to(dev).repeat(n // len(pics))
        self.topt = vp8g.tensor_opt(TARGET, "uint8", "NHWC")
        slot = int(lib.vp8g_tensor_slot_size_a(C.byref(self.topt)))
        # planar: scaled ARGB pictures in `mid`, then the tensor kernel
        self.pd = (vp8g.Vp8gScaleArgbDesc * n)()
        self.td = (vp8g.Vp8gTensorArgbDesc * n)()
        wo, mo = int(lib.vp8g_scale_argb_head_size(n)), 0
        planes = ts = tr = tm = tt = 0
        for i in range(n):
            d = self.pd[i]
            assert lib.vp8g_make_scale_argb_desc(w, h, i * 4 * w * h, C.byref(opt), wo, mo, planes, ts, tr, tm, C.byref(d)) == 0
            assert lib.vp8g_make_tensor_argb_desc(C.byref(self.topt), 4, mo, i * slot, tt, C.byref(self.td[i])) == 0
            planes, ts, tr, tm, tt = planes + d.nplanes, ts + d.split_ntasks, tr + d.scale_ntasks, tm + d.merge_ntasks, tt + self.td[i].ntasks
            wo += (d.work_bytes + 255) // 256 * 256
            mo += (4 * d.width * d.height + 255) // 256 * 256
        self.work = torch.zeros(wo, dtype=torch.uint8, device=dev)
        self.mid = torch.zeros(mo, dtype=torch.uint8, device=dev)
        self.work_bytes = wo + mo
        self.out_planar = torch.zeros((n, TARGET[1], TARGET[0], 4), dtype=torch.uint8, device=dev)
        self.d_pd = torch.frombuffer(bytearray(bytes(self.pd)), dtype=torch.uint8).to(dev)
        self.d_td = torch.frombuffer(bytearray(bytes(self.td)), dtype=torch.uint8).to(dev)
        # fused: straight into the tensor
        self.fd = (vp8g.Vp8gScaleArgbTensorDesc * n)()
        task0 = 0
        for i in range(n):
            assert lib.vp8g_make_scale_argb_tensor_desc(w, h, i * 4 * w * h, C.byref(opt), i * slot, task0, C.byref(self.fd[i])) == 0
            task0 += self.fd[i].ntasks
        self.fused_tasks = task0
        self.out_fused = torch.zeros((n, TARGET[1], TARGET[0], 4), dtype=torch.uint8, device=dev)
        self.d_fd = torch.frombuffer(bytearray(bytes(self.fd)), dtype=torch.uint8).to(dev)

    def planar(self, stream):
        lib, s = self.lib, C.c_void_p(stream)
        if lib.vp8g_scale_argb_batch_device(self.pd, C.c_void_p(self.d_pd.data_ptr()), self.n, C.c_void_p(self.src.data_ptr()),
                                            C.c_void_p(self.work.data_ptr()), C.c_void_p(self.mid.data_ptr()), s) != 0 or \
           lib.vp8g_tensor_batch_device_argb(self.td, C.c_void_p(self.d_td.data_ptr()), self.n, C.byref(self.topt), 4,
                                             C.c_void_p(self.mid.data_ptr()), C.c_void_p(self.out_planar.data_ptr()), s) != 0:
            raise RuntimeError(f"planar route: errno {C.get_errno()} {lib.vp8g_last_error()!r}")

    def fused(self, stream):
        if self.lib.vp8g_scale_argb_tensor_batch_device(self.fd, C.c_void_p(self.d_fd.data_ptr()), self.n, C.byref(self.topt), 4,
                                                        C.c_void_p(self.src.data_ptr()), C.c_void_p(self.out_fused.data_ptr()),
                                                        C.c_void_p(stream)) != 0:
            raise RuntimeError(f"fused route: errno {C.get_errno()} {self.lib.vp8g_last_error()!r}")


def timed(fn, stream, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn(stream.cuda_stream)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def kernel_rows(a, dev, stream):
    rows = []
    opt = vp8g.scale_opt(scale=TARGET)
    for w, h in ((1920, 1080), (3840, 2160)):
        rng = np.random.default_rng(w)
        pics = [random_argb(rng, w, h) for _ in range(4)]
        leg = Legs(pics, opt, a.images, dev)
        leg.planar(stream.cuda_stream), leg.fused(stream.cuda_stream)  # cold
        torch.cuda.synchronize(dev)
        for i in (0, 1, 2, 3, a.images - 1):  # both routes against the host's bytes, then against each other everywhere
            want = vp8g.argb_to_rgba(vp8g.host_scale_argb(pics[i % 4], opt))
            assert np.array_equal(leg.out_planar[i].cpu().numpy(), want) and np.array_equal(leg.out_fused[i].cpu().numpy(), want), (w, h, i)
        assert torch.equal(leg.out_planar, leg.out_fused)
        leg.out_fused.zero_()
        pms, fms = [], []
        for _ in range(a.runs):
            pms.append(timed(leg.planar, stream, dev))
            fms.append(timed(leg.fused, stream, dev))
        assert torch.equal(leg.out_planar, leg.out_fused)
        p, f = summary(pms), summary(fms)
        met = f["median"] < p["median"] and f["max"] < p["min"]
        row = {"size": [w, h], "target": list(TARGET), "images": a.images, "planar_ms": p, "fused_ms": f,
               "fused_over_planar": round(f["median"] / p["median"], 3), "condition_met": met,
               "fused_source_gb_per_s": round(a.images * w * h * 4 / f["median"] / 1e6, 1),
               "fused_tasks": leg.fused_tasks, "planar_work_bytes": leg.work_bytes, "fused_work_bytes": 0}
        rows.append(row)
        print(f"{w}x{h} x{a.images} -> {TARGET[0]}x{TARGET[1]} uint8 NHWC RGBA: planar {p['median']:.3f} ms ({p['min']:.3f} .. {p['max']:.3f}) | "
              f"fused {f['median']:.3f} ms ({f['min']:.3f} .. {f['max']:.3f}) | fused / planar {row['fused_over_planar']} | "
              f"condition {'met' if met else 'NOT met'}", flush=True)
        del leg
        torch.cuda.empty_cache()
    return rows


def e2e_leg(a, dev):
    names = ["pic_67x45_m4q75", "smooth_160x100_m6q100", "disc_160x100_m0q0", "smooth_192x128_m4q75", "tiles_160x100_m4q75", "disc_67x45_m4q75",
             "mixed_192x128_m4q75", "levels16_160x100_m4q75"]
    subs = []
    for nme in names:
        data = (ROOT / "tests" / "golden" / "lossless" / f"{nme}.webp").read_bytes()
        c = vp8g.parse_any(data)
        p = data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]
        subs.append((c["canvas_width"], c["canvas_height"], b"VP8L" + struct.pack("<I", len(p)) + p + (b"\0" if len(p) & 1 else b"")))
    cw, ch, nf = 512, 512, 16

    def le24(v):
        return struct.pack("<I", v)[:3]

    def build(seed):
        rng = np.random.default_rng(seed)
        body = b"VP8X" + struct.pack("<I", 10) + bytes([0x12, 0, 0, 0]) + le24(cw - 1) + le24(ch - 1) + b"ANIM" + struct.pack("<IIH", 6, 0, 0)
        for k in range(nf):
            w, h, sub = subs[int(rng.integers(0, len(subs)))]
            x, y = 2 * int(rng.integers(0, (cw - w) // 2 + 1)), 2 * int(rng.integers(0, (ch - h) // 2 + 1))
            pay = le24(x // 2) + le24(y // 2) + le24(w - 1) + le24(h - 1) + le24(40) + bytes([int(k % 3 == 0) | (2 if k % 5 == 0 else 0)]) + sub
            body += b"ANMF" + struct.pack("<I", len(pay)) + pay
        return b"RIFF" + struct.pack("<I", len(body) + 4) + b"WEBP" + body

    distinct = [build(s) for s in range(4)]
    files = [distinct[i % 4] for i in range(a.e2e_files)]
    small, full = vp8g.tensor_opt(TARGET, "float16", "NHWC", scale=1 / 255), vp8g.tensor_opt((cw, ch), "float16", "NHWC", scale=1 / 255)
    o = vp8g.scale_opt(scale=TARGET)
    out, first, _, st = vp8g.gpu_decode_webp_anim_tensor(files, small, threads=a.threads, scale=o)  # cold
    assert not any(st), st
    want, _ = vp8g.host_anim_scaled(distinct[1], o)
    same = all(torch.equal(out[first[1] + k].cpu().view(torch.uint8), vp8g.host_tensor_argb(want[k], small, 4).view(torch.uint8)) for k in range(nf))
    assert same
    del out
    vp8g.gpu_decode_webp_anim_tensor(files, full, threads=a.threads)  # cold
    runs = [[], []]
    for _ in range(a.e2e_runs):
        vp8g.gpu_decode_webp_anim_tensor(files, small, threads=a.threads, scale=o)
        runs[0].append(vp8g.gpu_decode_webp_anim_tensor.seconds)
        vp8g.gpu_decode_webp_anim_tensor(files, full, threads=a.threads)
        runs[1].append(vp8g.gpu_decode_webp_anim_tensor.seconds)
    rs, rf = summary(runs[0], 4), summary(runs[1], 4)
    print(f"end to end, {a.e2e_files} files x {nf} lossless frames on {cw}x{ch}, {a.threads} threads -> float16 NHWC RGBA: {TARGET[0]}x{TARGET[1]} scaled "
          f"{rs['median']} s ({rs['min']} .. {rs['max']}) | unscaled {rf['median']} s ({rf['min']} .. {rf['max']}); scaled equals the host {same}", flush=True)
    return {"files": a.e2e_files, "frames_per_file": nf, "canvas": [cw, ch], "target": list(TARGET), "threads": a.threads,
            "file_bytes": [len(b) for b in distinct], "scaled_s": rs, "unscaled_s": rf, "scaled_equals_host": same,
            "scaled_tensor_bytes": a.e2e_files * nf * TARGET[0] * TARGET[1] * 8, "unscaled_tensor_bytes": a.e2e_files * nf * cw * ch * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--e2e-files", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "anim_scale_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = kernel_rows(a, dev, stream)
    e2e = e2e_leg(a, dev)
    srcs = sorted((ROOT / "webp-decoder_amd").glob("csrc/*")) + sorted((ROOT / "webp-decoder_amd").glob("host/*")) + [ROOT / "include" / "vp8g.h"]
    tree = hashlib.sha256(b"".join(hashlib.sha256(p.read_bytes()).digest() for p in srcs)).hexdigest()[:16]
    doc = {"tool": "tools/anim_scale_bench.py", "device": torch.cuda.get_device_name(0),
           "build": f"sources sha256 {tree} (csrc/*, host/*, include/vp8g.h)",
           "timing": "HIP events (device), perf_counter (end to end); cold run discarded; median, min .. max; the two routes alternate",
           "condition": "fused median < planar median and fused max < planar min, on both rows",
           "condition_met": all(r["condition_met"] for r in rows), "rows": rows, "end_to_end": e2e}
    out = pathlib.Path(a.out)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
