#!/usr/bin/env python3
"""Measure decode-to-a-target-size on one MI355X, in one process.

 (i)  the scale kernel alone: N device-resident 4K I420 frames (the reconstruction of the four UHD
      fixtures, replicated) -> 224x224, 1920x1080 and 3839x2159; HIP-event ms and the achieved read
      rate (source bytes / t), next to the recon(+LF) launch over the same batch, and recon + scale
      back to back with and without VP8G_SCALE_DWEBP_FILTER (with it, 4K -> 224x224 skips m07).
 (ii) end to end: vp8g_decode_webp_batch_scaled(4K -> 224x224) against vp8g_decode_webp_batch on the
      same files: seconds and MP/s of source pixels, median / min / max.

Every leg: the cold first call discarded, then the median of the warm runs.  Writes
profiles/scale_bench.json and prints the table of DESIGN.md §14.

  python tools/scale_bench.py [--frames 512] [--runs 12] [--e2e-frames 256] [--e2e-runs 5]

 --expand: instead, the expand kernel (VP8G_SCALE_EXPAND) alone over N device-resident random I420
      frames: 160x120 -> 224x224, 500x200 -> 224x224 (x shrinks, y expands) and 256x256 -> 512x512, each
      next to a yardstick in the same process: the shrink kernel writing the same number of output
      samples at a ratio just under 1 ((w + 1) x (h + 1) -> w x h).  HIP-event ms and the achieved
      read + write rate.  Writes profiles/scale_expand_bench.json and prints its rows of §14.

  python tools/scale_bench.py --expand [--frames 512] [--runs 12]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

import torch  # noqa: E402  (first: its HIP runtime serves the process, as in bench.py)

import vp8g  # noqa: E402
import vp8g_batch  # noqa: E402

UHD = ["big/uhd_a_normal_seg4.webp", "big/uhd_b_simple_sharp3.webp", "big/uhd_c_normal_sharp6_seg1.webp",
       "big/uhd_d_normal_q90.webp"]
W, H = 3840, 2160
HBM_ACHIEVABLE_TBS = 6.29  # the achievable HBM read rate the microarchitecture notes give for this part


def timed_ms(launch, runs, dev):
    """Median / min / max HIP-event ms of `runs` warm launches (one cold launch discarded)."""
    stream = torch.cuda.current_stream(dev)
    launch()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        launch()
        b.record(stream)
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "runs": runs}


class ScaleLeg:
    """One vp8g_scale_batch_device launch over a DeviceBatch's output."""

    def __init__(self, batch, opt, dev):
        self.lib, self.n = vp8g.gpu_lib(), batch.n
        self.descs = (vp8g.Vp8gScaleDesc * batch.n)()
        ow, oh = vp8g.scaled_size(W, H, opt)
        self.size = (ow, oh)
        slot = (vp8g.i420_size(ow, oh) + 255) // 256 * 256
        task0 = 0
        for i in range(batch.n):
            d = batch.h_descs[i]
            assert self.lib.vp8g_make_scale_desc(W, H, d.out_y, d.out_u, d.out_v, d.stride_y, d.stride_uv, C.byref(opt),
                                                 i * slot, task0, C.byref(self.descs[i])) == 0
            task0 += self.descs[i].ntasks
        self.tasks = task0
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.out = torch.empty(batch.n * slot + 16, dtype=torch.uint8, device=dev)
        self.slot, self.src = slot, batch.out

    def launch(self, stream):
        rc = self.lib.vp8g_scale_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n,
                                              C.c_void_p(self.src.data_ptr()), C.c_void_p(self.out.data_ptr()), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"vp8g_scale_batch_device: {self.lib.vp8g_last_error()!r}")

    def frame(self, i):
        n = vp8g.i420_size(*self.size)
        return self.out[i * self.slot:i * self.slot + n].cpu().numpy().tobytes()


class PlainLeg:
    """One vp8g_scale_batch_device call over n tight random I420 frames of one size."""

    def __init__(self, n, size, target, expand, dev):
        import numpy as np
        self.lib, self.n, (sw, sh), (tw, th) = vp8g.gpu_lib(), n, size, target
        self.opt = vp8g.scale_opt(scale=target, expand=expand)
        fsz, slot = vp8g.i420_size(sw, sh), (vp8g.i420_size(tw, th) + 255) // 256 * 256
        cw, ch = (sw + 1) // 2, (sh + 1) // 2
        self.frames = [np.random.default_rng(77 + i).integers(0, 256, size=fsz, dtype=np.uint8) for i in range(4)]
        self.src = torch.from_numpy(np.concatenate([self.frames[i % 4] for i in range(n)])).to(dev)
        self.descs = (vp8g.Vp8gScaleDesc * n)()
        task0 = 0
        for i in range(n):
            o = i * fsz
            assert self.lib.vp8g_make_scale_desc(sw, sh, o, o + sw * sh, o + sw * sh + cw * ch, sw, cw, C.byref(self.opt),
                                                 i * slot, task0, C.byref(self.descs[i])) == 0
            task0 += self.descs[i].ntasks
        self.tasks, self.slot, self.size, self.target = task0, slot, size, target
        self.bytes = n * (fsz + vp8g.i420_size(tw, th))  # read + written
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.out = torch.empty(n * slot + 16, dtype=torch.uint8, device=dev)

    def launch(self, stream):
        rc = self.lib.vp8g_scale_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n,
                                              C.c_void_p(self.src.data_ptr()), C.c_void_p(self.out.data_ptr()), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"vp8g_scale_batch_device: {self.lib.vp8g_last_error()!r}")

    def parity(self):
        n = vp8g.i420_size(*self.target)
        return all(self.out[i * self.slot:i * self.slot + n].cpu().numpy().tobytes()
                   == vp8g.host_scale(self.frames[i % 4].tobytes(), *self.size, self.opt)[0] for i in (0, 1, 2, 3, self.n - 1))


def expand_legs(args, dev):
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"frames": args.frames, "legs": []}
    for size, target in (((160, 120), (224, 224)), ((500, 200), (224, 224)), ((256, 256), (512, 512))):
        row = {"source": list(size), "target": list(target)}
        for key, leg in (("expand", PlainLeg(args.frames, size, target, True, dev)),
                         ("yardstick_shrink", PlainLeg(args.frames, (target[0] + 1, target[1] + 1), target, False, dev))):
            t = timed_ms(lambda: leg.launch(stream), args.runs, dev)
            rate = leg.bytes / (t["ms"] * 1e-3) / 1e12
            t.update({"source": list(leg.size), "tasks": leg.tasks, "bytes_read_and_written": leg.bytes,
                      "TBs": round(rate, 3), "fraction_of_achievable": round(rate / HBM_ACHIEVABLE_TBS, 3),
                      "parity": "bit-exact vs host restatement (5 frames)" if leg.parity() else "MISMATCH"})
            row[key] = t
            del leg
        row["expand_over_yardstick"] = round(row["expand"]["ms"] / row["yardstick_shrink"]["ms"], 3)
        out["legs"].append(row)
    return out


def expand_table(res) -> str:
    rows = ["| leg | median | min .. max | note |", "|---|---|---|---|"]
    for r in res["expand"]["legs"]:
        for key in ("expand", "yardstick_shrink"):
            x = r[key]
            name = "expand" if key == "expand" else "yardstick, shrink kernel"
            rows.append(f"| {name}: {res['expand']['frames']} x {x['source'][0]}x{x['source'][1]} -> {r['target'][0]}x{r['target'][1]} | "
                        f"{x['ms']} ms | {x['min']} .. {x['max']} | {x['TBs']} TB/s read + written = {x['fraction_of_achievable']} of "
                        f"{HBM_ACHIEVABLE_TBS} TB/s; {x['tasks']} tasks"
                        + (f"; {r['expand_over_yardstick']} of the yardstick |" if key == "expand" else " |"))
    return "\n".join(rows)


def kernel_legs(args, dev):
    frames = [vp8g.decode_file(ROOT / "tests" / "fixtures" / r) for r in UHD]
    stream = torch.cuda.current_stream(dev).cuda_stream
    src_bytes = args.frames * vp8g.i420_size(W, H)
    out = {"frames": args.frames, "source_bytes": src_bytes,
           "hbm_bound_ms": round(src_bytes / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3, 3)}
    batches = {}
    for filtered in (True, False):
        b = vp8g_batch.DeviceBatch(args.frames, W, H, dev)
        b.replicate(frames, filtered)
        b.commit()
        batches[filtered] = b
        out["recon_filtered" if filtered else "recon_unfiltered"] = timed_ms(lambda: b.launch(stream), args.runs, dev)
    bf, bu = batches[True], batches[False]
    oracle = {True: [vp8g.oracle_reconstruct(f, True) for f in frames], False: [vp8g.oracle_reconstruct(f, False) for f in frames]}
    out["scale"] = []
    for tw, th in ((224, 224), (1920, 1080), (3839, 2159)):
        opt = vp8g.scale_opt(scale=(tw, th))
        leg = ScaleLeg(bf, opt, dev)
        t = timed_ms(lambda: leg.launch(stream), args.runs, dev)
        ok = all(leg.frame(i) == vp8g.host_scale(oracle[True][i % 4], W, H, opt)[0] for i in (0, 1, 2, 3, args.frames - 1))
        t.update({"target": [tw, th], "tasks": leg.tasks, "read_TBs": round(src_bytes / (t["ms"] * 1e-3) / 1e12, 3),
                  "fraction_of_achievable": round(src_bytes / (t["ms"] * 1e-3) / 1e12 / HBM_ACHIEVABLE_TBS, 3),
                  "fraction_of_recon_filtered": round(t["ms"] / out["recon_filtered"]["ms"], 3),
                  "parity": "bit-exact vs host restatement (5 frames)" if ok else "MISMATCH"})
        out["scale"].append(t)
        del leg
    # 4K -> 224x224, recon + scale back to back: without the flag filtered means filtered; with it
    # libwebp's rule skips the loop filter (224 < 3840 * 3 / 4 and 224 < 2160 * 3 / 4)
    for flag, b in ((False, bf), (True, bu)):
        opt = vp8g.scale_opt(scale=(224, 224), dwebp_filter=flag)
        assert vp8g.host_lib().vp8f_scale_filtered(W, H, C.byref(opt), 1) == (0 if flag else 1)
        leg = ScaleLeg(b, opt, dev)

        def both(b=b, leg=leg):
            b.launch(stream)
            leg.launch(stream)
        out["recon_plus_scale_224_dwebp_filter" if flag else "recon_plus_scale_224"] = timed_ms(both, args.runs, dev)
        del leg
    for f in frames:
        f.free()
    return out


def e2e_legs(args):
    files = [(ROOT / "tests" / "fixtures" / r).read_bytes() for r in UHD]
    batch = [files[i % 4] for i in range(args.e2e_frames)]
    mp = args.e2e_frames * W * H / 1e6

    def leg(call, seconds_of):
        call()  # cold
        runs = []
        for _ in range(args.e2e_runs):
            call()
            runs.append(seconds_of())
        med = statistics.median(runs)
        return {"seconds": round(med, 3), "min": round(min(runs), 3), "max": round(max(runs), 3), "runs": len(runs),
                "MPs": round(mp / med, 1)}

    out = {"frames": args.e2e_frames, "source_megapixels": round(mp, 1)}
    out["full_size"] = leg(lambda: vp8g.gpu_decode_webp_batch(batch, True), lambda: vp8g.gpu_decode_webp_batch.seconds)
    for flag in (False, True):
        opt = vp8g.scale_opt(scale=(224, 224), dwebp_filter=flag)
        out["scaled_224_dwebp_filter" if flag else "scaled_224"] = leg(
            lambda: vp8g.gpu_decode_webp_batch_scaled(batch, opt, True), lambda: vp8g.gpu_decode_webp_batch_scaled.seconds)
    return out


def table(res) -> str:
    k, e = res["kernel"], res["end_to_end"]
    rows = ["| leg | median | min .. max | note |", "|---|---|---|---|"]
    rows.append(f"| recon + LF launch, {k['frames']} 4K frames | {k['recon_filtered']['ms']} ms | {k['recon_filtered']['min']} .. "
                f"{k['recon_filtered']['max']} | the batch the scale kernel reads |")
    rows.append(f"| recon launch, no LF | {k['recon_unfiltered']['ms']} ms | {k['recon_unfiltered']['min']} .. "
                f"{k['recon_unfiltered']['max']} | |")
    for s in k["scale"]:
        rows.append(f"| scale -> {s['target'][0]}x{s['target'][1]} | {s['ms']} ms | {s['min']} .. {s['max']} | "
                    f"{s['read_TBs']} TB/s read = {s['fraction_of_achievable']} of {HBM_ACHIEVABLE_TBS} TB/s (bound "
                    f"{k['hbm_bound_ms']} ms); {s['fraction_of_recon_filtered']} of the recon + LF launch; {s['tasks']} tasks |")
    a, b = k["recon_plus_scale_224"], k["recon_plus_scale_224_dwebp_filter"]
    rows.append(f"| recon + LF + scale -> 224x224 | {a['ms']} ms | {a['min']} .. {a['max']} | filtered, no flag |")
    rows.append(f"| recon + scale -> 224x224, VP8G_SCALE_DWEBP_FILTER | {b['ms']} ms | {b['min']} .. {b['max']} | m07 skipped |")
    for key, name in (("full_size", "vp8g_decode_webp_batch (full size)"), ("scaled_224", "vp8g_decode_webp_batch_scaled -> 224x224"),
                      ("scaled_224_dwebp_filter", "the same with VP8G_SCALE_DWEBP_FILTER")):
        x = e[key]
        rows.append(f"| end to end, {e['frames']} frames: {name} | {x['seconds']} s | {x['min']} .. {x['max']} | {x['MPs']} MP/s of "
                    f"source pixels |")
    return "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--e2e-frames", type=int, default=256)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--expand", action="store_true", help="the expand kernel's legs only (profiles/scale_expand_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 10 or args.e2e_runs < 5:
        ap.error("--runs >= 10 and --e2e-runs >= 5")
    dev = torch.device("cuda", 0)
    if args.expand:
        res = {"device": torch.cuda.get_device_name(dev), "expand": expand_legs(args, dev)}
        pathlib.Path(args.out or ROOT / "profiles" / "scale_expand_bench.json").write_text(json.dumps(res, indent=1) + "\n")
        print(expand_table(res))
        return 0
    args.out = args.out or str(ROOT / "profiles" / "scale_bench.json")
    res = {"device": torch.cuda.get_device_name(dev), "kernel": kernel_legs(args, dev)}
    torch.cuda.empty_cache()
    res["end_to_end"] = e2e_legs(args)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(table(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
