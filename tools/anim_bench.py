#!/usr/bin/env python3
"""Measure the animation path on one MI355X, in one process.

Compositor, synthetic frames (no streams), uint8 / NHWC / RGBA canvases:
  many    64 animations of 32 frames on a 512 x 512 canvas: a full first frame, then rectangles of a quarter to the
          whole canvas with mixed blend and disposal (a few key frames inside)
  uhd     16 animations of 8 frames on a 3840 x 2160 canvas: a full first frame, then 256 x 256 frames
  device  vp8g_anim_compose_batch_device, one launch over all animations (four distinct ones' pictures on the device,
          replicated through the descriptors; every animation writes canvases of its own); HIP-event ms, the cold first
          launch discarded, then the median of the warm runs with min .. max
  host    vp8f_anim_compose over the same animations on 16 threads (each thread its share, into canvases of its own);
          wall ms, same statistics, same run
Bytes moved = the sub-frame bytes the compositor must read (4 per rectangle pixel) + the canvas bytes it must write;
the rate is that over the device's median.  One animation per workload is compared with the host's canvases before
anything is timed.

End to end: --e2e-files animated files of 16 lossless frames on a 192 x 128 canvas (assembled in memory from the
streams of tests/golden/lossless/) through vp8g_decode_webp_anim_tensor into a uint8 NHWC RGBA tensor; wall s.

Writes profiles/anim_bench.json and prints its rows.

  python tools/anim_bench.py [--runs 7] [--threads 16] [--e2e-files 64] [--e2e-runs 5] [--build ID]
"""
import argparse
import ctypes as C
import hashlib
import json
import pathlib
import statistics
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: its HIP runtime serves the process, as in bench.py)

import vp8g  # noqa: E402

ALPHAS = np.array([0, 1, 3, 128, 254, 255], np.uint32)


def summary(ms, nd=3):
    return {"median": round(statistics.median(ms), nd), "min": round(min(ms), nd), "max": round(max(ms), nd), "runs": len(ms)}


def picture(rng, w, h):
    return rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) | ALPHAS[rng.integers(0, 6, (h, w))] << 24


def synth(rng, cw, ch, n, small):
    frames = [{"argb": picture(rng, cw, ch), "x": 0, "y": 0, "blend": 1, "dispose": 0, "has_alpha": 1}]
    for k in range(1, n):
        if small:
            w = h = small
        else:
            w, h = int(rng.integers(cw // 2, cw + 1)), int(rng.integers(ch // 2, ch + 1))
            if k % 11 == 0:
                w, h = cw, ch
        x, y = 2 * int(rng.integers(0, (cw - w) // 2 + 1)), 2 * int(rng.integers(0, (ch - h) // 2 + 1))
        frames.append({"argb": picture(rng, w, h), "x": x, "y": y, "blend": int(k % 5 != 0), "dispose": int(k % 3 == 0), "has_alpha": int(k % 11 != 0)})
    return frames


class DeviceLeg:
    def __init__(self, distinct, cw, ch, n, dev):
        self.lib, self.n, self.cw, self.ch = vp8g.gpu_lib(), n, cw, ch
        parts, so, recs = [], 0, []
        for frames in distinct:
            srcs = []
            for f in frames:
                b = np.ascontiguousarray(f["argb"]).reshape(-1).view(np.uint8)
                srcs.append(so)
                parts.append(b)
                so += b.size
            recs.append(srcs)
        so = (so + 7) // 8 * 8
        pic_bytes = so
        self.descs = (vp8g.Vp8gAnimDesc * n)()
        self.recs, self.nframes = [], [len(distinct[i % len(distinct)]) for i in range(n)]
        task0 = do = 0
        rec_bytes = []
        for i in range(n):
            frames = distinct[i % len(distinct)]
            rec = vp8g.anim_records(frames, recs[i % len(distinct)])
            assert self.lib.vp8g_make_anim_desc(cw, ch, rec, len(frames), so, do, task0, C.byref(self.descs[i])) == 0
            self.recs.append(rec)
            rec_bytes.append(np.frombuffer(bytes(rec), np.uint8))
            so += rec_bytes[-1].size
            task0 += self.descs[i].ntasks
            do += len(frames) * cw * ch * 4
        pad = np.zeros(pic_bytes - sum(p.size for p in parts), np.uint8)
        self.src = torch.from_numpy(np.concatenate(parts + [pad] + rec_bytes)).to(dev)
        self.dst = torch.empty(do, dtype=torch.uint8, device=dev)
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.opt = vp8g.tensor_opt((cw, ch), "uint8", "NHWC")
        self.tasks, self.segments = task0, sum(d.nsegs for d in self.descs)
        self.read_bytes = sum(4 * f["argb"].size for i in range(n) for f in distinct[i % len(distinct)])
        self.write_bytes = do

    def launch(self, stream):
        if self.lib.vp8g_anim_compose_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n, C.byref(self.opt), 4,
                                                   C.c_void_p(self.src.data_ptr()), C.c_void_p(self.dst.data_ptr()), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_anim_compose_batch_device: errno {C.get_errno()} {self.lib.vp8g_last_error()!r}")

    def canvases(self, i):
        d = self.descs[i]
        return self.dst[d.dst:d.dst + self.nframes[i] * self.cw * self.ch * 4].cpu().numpy().reshape(self.nframes[i], self.ch, self.cw, 4)


def host_run(structs, cw, ch, n, threads, outs):
    lib = vp8g.host_lib()

    def work(t):
        for i in range(t, n, threads):
            fr = structs[i % len(structs)][0]
            if lib.vp8f_anim_compose(cw, ch, fr, len(fr), outs[t].ctypes.data) != 0:
                raise RuntimeError("vp8f_anim_compose failed")

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return (time.perf_counter() - t0) * 1e3


def e2e_leg(a, dev):
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    names = ["pic_67x45_m4q75", "smooth_160x100_m6q100", "disc_160x100_m0q0", "smooth_192x128_m4q75", "tiles_160x100_m4q75", "disc_67x45_m4q75",
             "mixed_192x128_m4q75", "levels16_160x100_m4q75"]
    subs = []
    for nme in names:
        data = (ROOT / "tests" / "golden" / "lossless" / f"{nme}.webp").read_bytes()
        c = vp8g.parse_any(data)
        p = data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]
        subs.append((c["canvas_width"], c["canvas_height"], b"VP8L" + struct.pack("<I", len(p)) + p + (b"\0" if len(p) & 1 else b"")))
    cw, ch, nf = 192, 128, 16

    def le24(v):
        return struct.pack("<I", v)[:3]

    def build(seed):
        rng = np.random.default_rng(seed)
        body = b"VP8X" + struct.pack("<I", 10) + bytes([0x12, 0, 0, 0]) + le24(cw - 1) + le24(ch - 1) + b"ANIM" + struct.pack("<IIH", 6, 0, 0)
        for k in range(nf):
            w, h, sub = subs[3 if k == 0 else int(rng.integers(0, len(subs)))]
            x, y = 2 * int(rng.integers(0, (cw - w) // 2 + 1)), 2 * int(rng.integers(0, (ch - h) // 2 + 1))
            pay = le24(x // 2) + le24(y // 2) + le24(w - 1) + le24(h - 1) + le24(40) + bytes([int(k % 3 == 0) | (2 if k % 5 == 0 else 0)]) + sub
            body += b"ANMF" + struct.pack("<I", len(pay)) + pay
        return b"RIFF" + struct.pack("<I", len(body) + 4) + b"WEBP" + body

    distinct = [build(s) for s in range(4)]
    files = [distinct[i % 4] for i in range(a.e2e_files)]
    opt = vp8g.tensor_opt((cw, ch), "uint8", "NHWC")
    out, first, ts, st = vp8g.gpu_decode_webp_anim_tensor(files, opt, threads=a.threads)  # cold
    assert not any(st), st
    (w0, h0), frames, _ = vp8g.host_anim_frames(distinct[1])
    want, _ = vp8g.host_anim_compose(w0, h0, frames)
    same = all(np.array_equal(out[first[1] + k].cpu().numpy(), vp8g.argb_to_rgba(want[k])) for k in range(nf))
    runs = []
    for _ in range(a.e2e_runs):
        vp8g.gpu_decode_webp_anim_tensor(files, opt, threads=a.threads)
        runs.append(vp8g.gpu_decode_webp_anim_tensor.seconds)
    r = summary(runs, 4)
    r["equals_host"] = same
    print(f"end to end, {a.e2e_files} files x {nf} lossless frames on {cw}x{ch}, {a.threads} threads -> uint8 NHWC RGBA: {r['median']} s "
          f"({r['min']} .. {r['max']}); equal to the host's canvases {same}", flush=True)
    return {"files": a.e2e_files, "frames_per_file": nf, "canvas": [cw, ch], "threads": a.threads, "file_bytes": [len(b) for b in distinct], "tensor_s": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--e2e-files", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--build", default="", help="what was measured (a commit id or source hash), recorded in the output")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = []
    for name, (cw, ch), n, nf, small in (("many", (512, 512), 64, 32, 0), ("uhd", (3840, 2160), 16, 8, 256)):
        rng = np.random.default_rng(cw)
        distinct = [synth(rng, cw, ch, nf, small) for _ in range(4)]
        structs = [vp8g._anim_host_structs(f) for f in distinct]
        leg = DeviceLeg(distinct, cw, ch, n, dev)
        leg.launch(stream.cuda_stream)  # cold
        torch.cuda.synchronize(dev)
        for i in (0, n - 1):
            want, _ = vp8g.host_anim_compose(cw, ch, distinct[i % 4])
            got = leg.canvases(i)
            assert all(np.array_equal(got[k], vp8g.argb_to_rgba(want[k])) for k in range(nf)), (name, i)
        outs = [np.empty((nf, ch, cw), np.uint32) for _ in range(a.threads)]
        host_run(structs, cw, ch, n, a.threads, outs)  # cold
        dms, hms = [], []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            leg.launch(stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            dms.append(e0.elapsed_time(e1))
            hms.append(host_run(structs, cw, ch, n, a.threads, outs))
        d, hs = summary(dms), summary(hms, 1)
        moved = leg.read_bytes + leg.write_bytes
        row = {"workload": name, "canvas": [cw, ch], "animations": n, "frames": nf, "segments": leg.segments, "tasks": leg.tasks,
               "read_bytes": leg.read_bytes, "write_bytes": leg.write_bytes, "device_ms": d, "host_ms": hs, "host_threads": a.threads,
               "device_gb_per_s": round(moved / d["median"] / 1e6, 1), "host_gb_per_s": round(moved / hs["median"] / 1e6, 2),
               "device_over_host": round(hs["median"] / d["median"], 1)}
        rows.append(row)
        print(f"{name}: {n} x {nf} frames on {cw}x{ch}: device {d['median']:9.3f} ms ({d['min']:.3f} .. {d['max']:.3f}) {row['device_gb_per_s']:8.1f} GB/s | "
              f"host x{a.threads} {hs['median']:9.1f} ms ({hs['min']:.1f} .. {hs['max']:.1f}) {row['host_gb_per_s']:6.2f} GB/s | x{row['device_over_host']}",
              flush=True)
        del leg, outs
        torch.cuda.empty_cache()
    e2e = e2e_leg(a, dev)
    srcs = sorted((ROOT / "webp-decoder_amd").glob("csrc/*")) + sorted((ROOT / "webp-decoder_amd").glob("host/*")) + [ROOT / "include" / "vp8g.h"]
    tree = hashlib.sha256(b"".join(hashlib.sha256(p.read_bytes()).digest() for p in srcs)).hexdigest()[:16]
    doc = {"tool": "tools/anim_bench.py", "device": torch.cuda.get_device_name(0),
           "build": a.build or f"sources sha256 {tree} (csrc/*, host/*, include/vp8g.h)", "sources_sha256": tree,
           "timing": "HIP events (device), perf_counter (host); cold run discarded; median, min .. max",
           "bytes": "read_bytes = 4 per pixel of every frame rectangle; write_bytes = 4 per canvas pixel per frame (uint8 NHWC RGBA)",
           "rows": rows, "end_to_end": e2e}
    out = ROOT / "profiles" / "anim_bench.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
