#!/usr/bin/env python3
"""Measure decode-to-a-device-tensor on one MI355X, in one process.

 (i)   the tensor kernel against the file encoder: N device-resident 4K I420 frames (the filtered
       reconstruction of the four UHD fixtures, replicated) -> uint8 NHWC, interleaved run by run
       with vp8g_encode_batch_device in VP8G_ENC_RGB on the same input.  The two write identical
       bytes (checked), so the encoder is the yardstick.
 (ii)  the legs with no predecessor: the same frames -> float16 NCHW, and the data-loader shape, N
       224x224 I420 pictures (the host rescale of the four frames, replicated) -> float16 NCHW; and the
       4-channel kernel (vp8g_tensor_batch_device_a, one random alpha plane per picture): the 4K frames ->
       uint8 NHWC RGBA, the 224x224 pictures -> float16 NCHW RGBA.  HIP-event ms and the achieved bytes/s
       read + written against the achievable HBM rate.
 (iii) end to end: vp8g_decode_webp_batch_tensor(4K -> 224x224 float16 NCHW) against
       vp8g_decode_webp_batch_scaled(4K -> 224x224), interleaved call by call.  --parent-lib names a
       libvp8g.so built from the parent commit for the scaled leg (loaded side by side); without it
       the scaled leg runs this tree's library.

Every leg: the cold first call discarded, then the median of the warm runs with min .. max.  Writes
profiles/tensor_bench.json and prints the table of DESIGN.md §15.  --e2e-frames 0 leaves (iii) out (an A/B of
the kernels alone: VP8G_LIB=<another build's libvp8g.so> runs the same legs on that library).

  python tools/tensor_bench.py [--frames 512] [--runs 12] [--e2e-frames 256] [--e2e-runs 5] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: its HIP runtime serves the process, as in bench.py)

import vp8g  # noqa: E402

UHD = ["big/uhd_a_normal_seg4.webp", "big/uhd_b_simple_sharp3.webp", "big/uhd_c_normal_sharp6_seg1.webp",
       "big/uhd_d_normal_q90.webp"]
W, H = 3840, 2160
HBM_ACHIEVABLE_TBS = 6.29  # the achievable HBM read rate the microarchitecture notes give for this part
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def summary(ms, nd=3):
    return {"median": round(statistics.median(ms), nd), "min": round(min(ms), nd), "max": round(max(ms), nd), "runs": len(ms)}


def timed_interleaved(launches, runs, dev):
    """HIP-event ms of `runs` warm launches of every leg, the legs alternating (one cold launch each discarded)."""
    stream = torch.cuda.current_stream(dev)
    for f in launches:
        f()
    torch.cuda.synchronize(dev)
    ms = [[] for _ in launches]
    for _ in range(runs):
        for k, f in enumerate(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            f()
            b.record(stream)
            torch.cuda.synchronize(dev)
            ms[k].append(a.elapsed_time(b))
    return [summary(m) for m in ms]


class Source:
    """n device-resident I420 pictures of one size: slot i <- pictures[i % K] at 256-byte aligned steps, each
    followed by its alpha plane (w x h random bytes per picture; only the 4-channel legs read it)."""

    def __init__(self, pictures, w, h, n, dev):
        self.w, self.h, self.n, self.pictures = w, h, n, pictures
        self.alphas = [np.random.default_rng(k).integers(0, 256, (h, w), dtype=np.uint8) for k in range(len(pictures))]
        self.i420 = vp8g.i420_size(w, h)
        self.step = (self.i420 + w * h + 255) // 256 * 256
        self.buf = torch.empty(n * self.step + 16, dtype=torch.uint8, device=dev)
        view = self.buf[:n * self.step].view(n, self.step)
        for j, (p, a) in enumerate(zip(pictures, self.alphas)):
            view[j::len(pictures), :self.i420] = torch.from_numpy(np.frombuffer(p, np.uint8).copy()).to(dev)
            view[j::len(pictures), self.i420:self.i420 + w * h] = torch.from_numpy(a.reshape(-1)).to(dev)

    def planes(self, i):
        cw, ch = (self.w + 1) // 2, (self.h + 1) // 2
        o = i * self.step
        return o, o + self.w * self.h, o + self.w * self.h + cw * ch


class TensorLeg:
    """One vp8g_tensor_batch_device launch over a Source; alpha: vp8g_tensor_batch_device_a with the Source's alpha planes."""

    def __init__(self, src, opt, dev, alpha=False):
        self.lib, self.src, self.opt, self.n, self.alpha = vp8g.gpu_lib(), src, opt, src.n, alpha
        self.slot = (self.lib.vp8g_tensor_slot_size_a if alpha else self.lib.vp8g_tensor_slot_size)(C.byref(opt))
        self.descs = (vp8g.Vp8gTensorDesc * src.n)()
        task0 = 0
        for i in range(src.n):
            y, u, v = src.planes(i)
            assert self.lib.vp8g_make_tensor_desc(C.byref(opt), y, u, v, src.w, (src.w + 1) // 2, i * self.slot, task0,
                                                  C.byref(self.descs[i])) == 0
            task0 += self.descs[i].ntasks
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.al = (vp8g.Vp8gTensorAlpha * src.n)(*[vp8g.Vp8gTensorAlpha(i * src.step + src.i420, src.w, 0) for i in range(src.n)])
        self.d_al = torch.frombuffer(bytearray(bytes(self.al)), dtype=torch.uint8).to(dev)
        self.out = torch.empty(vp8g._tensor_shape(src.n, opt, 4 if alpha else 3), dtype=vp8g._torch_dtype(opt), device=dev)
        self.bytes = src.n * (src.i420 + (src.w * src.h if alpha else 0) + self.slot)  # read + written

    def launch(self, stream):
        if self.alpha:
            if self.lib.vp8g_tensor_batch_device_a(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.al,
                                                   C.c_void_p(self.d_al.data_ptr()), self.n, C.byref(self.opt),
                                                   C.c_void_p(self.src.buf.data_ptr()), C.c_void_p(self.out.data_ptr()),
                                                   C.c_void_p(stream)) != 0:
                raise RuntimeError(f"vp8g_tensor_batch_device_a: {self.lib.vp8g_last_error()!r}")
            return
        if self.lib.vp8g_tensor_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n, C.byref(self.opt),
                                             C.c_void_p(self.src.buf.data_ptr()), C.c_void_p(self.out.data_ptr()),
                                             C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_tensor_batch_device: {self.lib.vp8g_last_error()!r}")

    def parity(self, picks):
        int_view = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
        for i in picks:
            k = i % len(self.src.pictures)
            exp = vp8g.host_tensor(self.src.pictures[k], self.src.w, self.src.h, self.opt, alpha=self.src.alphas[k] if self.alpha else None)
            if not torch.equal(self.out[i].cpu().view(int_view[exp.dtype]), exp.view(int_view[exp.dtype])):
                return "MISMATCH"
        return f"bit-exact vs host_tensor ({len(picks)} frames)"


class EncoderLeg:
    """One vp8g_encode_batch_device launch (VP8G_ENC_RGB) over a Source."""

    def __init__(self, src, dev):
        self.lib, self.src, self.n = vp8g.gpu_lib(), src, src.n
        self.descs, self.outs, total, spans = vp8g.make_enc_descs([(src.w, src.h)] * src.n, "rgb", [src.planes(i) for i in range(src.n)])
        self.d_descs = torch.frombuffer(bytearray(bytes(self.descs)), dtype=torch.uint8).to(dev)
        self.out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        self.work = torch.empty(self.lib.vp8g_encode_workspace_size(spans), dtype=torch.uint8, device=dev)
        self.bytes = src.n * (src.i420 + 3 * src.w * src.h)

    def launch(self, stream):
        if self.lib.vp8g_encode_batch_device(self.descs, C.c_void_p(self.d_descs.data_ptr()), self.n,
                                             C.c_void_p(self.src.buf.data_ptr()), C.c_void_p(self.out.data_ptr()),
                                             C.c_void_p(self.work.data_ptr()), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"vp8g_encode_batch_device: {self.lib.vp8g_last_error()!r}")

    def frame(self, i):
        return self.out[self.outs[i]:self.outs[i] + 3 * self.src.w * self.src.h]


def rate(leg_bytes, t):
    tbs = leg_bytes / (t["median"] * 1e-3) / 1e12
    t.update({"bytes_read_written": leg_bytes, "TBs": round(tbs, 3), "fraction_of_achievable": round(tbs / HBM_ACHIEVABLE_TBS, 3)})
    return t


def kernel_legs(args, dev):
    frames = [vp8g.decode_file(ROOT / "tests" / "fixtures" / r) for r in UHD]
    full = [vp8g.oracle_reconstruct(f, True) for f in frames]
    for f in frames:
        f.free()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = args.frames
    picks = (0, 1, 2, 3, n - 1)
    out = {"frames": n}
    src = Source(full, W, H, n, dev)
    enc = EncoderLeg(src, dev)
    u8 = TensorLeg(src, vp8g.tensor_opt((W, H), "uint8", "NHWC"), dev)
    t_enc, t_u8 = timed_interleaved([lambda: enc.launch(stream), lambda: u8.launch(stream)], args.runs, dev)
    same = all(torch.equal(enc.frame(i), u8.out[i].reshape(-1)) for i in picks)
    out["encoder_rgb_4k"] = rate(enc.bytes, t_enc)
    out["tensor_u8_nhwc_4k"] = rate(u8.bytes, t_u8)
    out["tensor_u8_nhwc_4k"].update({"parity": u8.parity(picks[:2]), "same_bytes_as_encoder": bool(same),
                                     "vs_encoder_median": round(t_u8["median"] / t_enc["median"], 3),
                                     "within_encoder_spread": bool(t_enc["min"] <= t_u8["median"] <= t_enc["max"]
                                                                   or t_u8["median"] <= t_enc["median"])})
    del enc, u8
    torch.cuda.empty_cache()
    f16 = TensorLeg(src, vp8g.tensor_opt((W, H), "float16", "NCHW", **IMAGENET), dev)
    (t,) = timed_interleaved([lambda: f16.launch(stream)], args.runs, dev)
    out["tensor_f16_nchw_4k"] = rate(f16.bytes, t)
    out["tensor_f16_nchw_4k"]["parity"] = f16.parity(picks[:2])
    del f16
    torch.cuda.empty_cache()
    u8a = TensorLeg(src, vp8g.tensor_opt((W, H), "uint8", "NHWC"), dev, alpha=True)
    (t,) = timed_interleaved([lambda: u8a.launch(stream)], args.runs, dev)
    out["tensor_u8_nhwc_rgba_4k"] = rate(u8a.bytes, t)
    out["tensor_u8_nhwc_rgba_4k"]["parity"] = u8a.parity(picks[:2])
    del u8a, src
    torch.cuda.empty_cache()
    sopt = vp8g.scale_opt(scale=(224, 224))
    small = Source([vp8g.host_scale(b, W, H, sopt)[0] for b in full], 224, 224, n, dev)
    s16 = TensorLeg(small, vp8g.tensor_opt((224, 224), "float16", "NCHW", **IMAGENET), dev)
    (t,) = timed_interleaved([lambda: s16.launch(stream)], args.runs, dev)
    out["tensor_f16_nchw_224"] = rate(s16.bytes, t)
    out["tensor_f16_nchw_224"]["parity"] = s16.parity(picks)
    s16a = TensorLeg(small, vp8g.tensor_opt((224, 224), "float16", "NCHW", **IMAGENET), dev, alpha=True)
    (t,) = timed_interleaved([lambda: s16a.launch(stream)], args.runs, dev)
    out["tensor_f16_nchw_rgba_224"] = rate(s16a.bytes, t)
    out["tensor_f16_nchw_rgba_224"]["parity"] = s16a.parity(picks)
    return out


def scaled_call(lib):
    """vp8g_decode_webp_batch_scaled of a libvp8g.so handle (this tree's, or another build loaded side by
    side): a callable (spans, n, opt) -> seconds of the C call alone."""
    P = C.POINTER
    lib.vp8g_decode_webp_batch_scaled.argtypes = [P(vp8g.ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                  P(vp8g.Vp8gScaleOpt), C.c_uint32, P(vp8g.Yuv420Image), P(C.c_int)]
    lib.yuv420_free.argtypes = [P(vp8g.Yuv420Image)]
    lib.yuv420_free.restype = None

    def call(spans, n, opt):
        imgs, st = (vp8g.Yuv420Image * n)(), (C.c_int * n)()
        t0 = time.perf_counter()
        rc = lib.vp8g_decode_webp_batch_scaled(spans, n, 1, 0, 0, C.byref(opt), 1, imgs, st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError("vp8g_decode_webp_batch_scaled failed")
        for i in range(n):
            lib.yuv420_free(C.byref(imgs[i]))
        return dt
    return call


def e2e_legs(args, dev):
    files = [(ROOT / "tests" / "fixtures" / r).read_bytes() for r in UHD]
    n = args.e2e_frames
    mp = n * W * H / 1e6
    sopt = vp8g.scale_opt(scale=(224, 224))
    topt = vp8g.tensor_opt((224, 224), "float16", "NCHW", **IMAGENET)
    # both legs read the same input: one buffer per frame (a loader's files are distinct), built once
    bufs = [(C.c_uint8 * len(files[i % 4])).from_buffer_copy(files[i % 4]) for i in range(n)]
    spans = (vp8g.ByteSpan * n)(*[vp8g.ByteSpan(C.cast(bufs[i], C.POINTER(C.c_uint8)), len(bufs[i])) for i in range(n)])
    lib = vp8g.gpu_lib()
    scaled_of = scaled_call(C.CDLL(str(pathlib.Path(args.parent_lib).resolve()), use_errno=True) if args.parent_lib else lib)
    out = torch.empty((n, 3, 224, 224), dtype=torch.float16, device=dev)
    torch.cuda.synchronize(dev)

    def scaled():
        return scaled_of(spans, n, sopt)

    def tensor():
        st = (C.c_int * n)()
        t0 = time.perf_counter()
        rc = lib.vp8g_decode_webp_batch_tensor(spans, n, 1, 0, 0, C.byref(sopt), 1, C.byref(topt), C.c_void_p(out.data_ptr()), st)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"vp8g_decode_webp_batch_tensor failed: {lib.vp8g_last_error()!r}")
        return dt

    scaled(), tensor()  # cold
    runs = [[], []]
    for _ in range(args.e2e_runs):
        runs[0].append(scaled())
        runs[1].append(tensor())
    a, b = summary(runs[0]), summary(runs[1])
    a["MPs"], b["MPs"] = round(mp / a["median"], 1), round(mp / b["median"], 1)
    a["library"] = "parent build (--parent-lib)" if args.parent_lib else "this tree"
    b["vs_scaled_median"] = round(b["median"] / a["median"], 3)
    b["within_scaled_spread"] = bool(b["median"] <= a["max"])
    return {"frames": n, "source_megapixels": round(mp, 1), "scaled_224_i420_download": a, "tensor_224_f16_nchw": b}


def table(res) -> str:
    k, e = res["kernel"], res.get("end_to_end")
    rows = ["| leg | median | min .. max | note |", "|---|---|---|---|"]
    names = (("encoder_rgb_4k", f"vp8g_encode_batch_device, VP8G_ENC_RGB, {k['frames']} 4K frames"),
             ("tensor_u8_nhwc_4k", "tensor kernel, uint8 NHWC, same frames"),
             ("tensor_f16_nchw_4k", "tensor kernel, float16 NCHW, same frames"),
             ("tensor_u8_nhwc_rgba_4k", "tensor kernel, uint8 NHWC RGBA, same frames and an alpha plane each"),
             ("tensor_f16_nchw_224", f"tensor kernel, float16 NCHW, {k['frames']} x 224x224"),
             ("tensor_f16_nchw_rgba_224", "tensor kernel, float16 NCHW RGBA, same pictures and an alpha plane each"))
    for key, name in names:
        x = k[key]
        note = f"{x['TBs']} TB/s read + written = {x['fraction_of_achievable']} of {HBM_ACHIEVABLE_TBS} TB/s"
        if "vs_encoder_median" in x:
            note += f"; {x['vs_encoder_median']} of the encoder's median; same bytes as the encoder: {x['same_bytes_as_encoder']}"
        if "parity" in x:
            note += f"; {x['parity']}"
        rows.append(f"| {name} | {x['median']} ms | {x['min']} .. {x['max']} | {note} |")
    if not e:
        return "\n".join(rows)
    a, b = e["scaled_224_i420_download"], e["tensor_224_f16_nchw"]
    rows.append(f"| end to end, {e['frames']} 4K files: vp8g_decode_webp_batch_scaled -> 224x224 ({a['library']}) | {a['median']} s | "
                f"{a['min']} .. {a['max']} | {a['MPs']} MP/s of source pixels |")
    rows.append(f"| end to end: vp8g_decode_webp_batch_tensor -> 224x224 float16 NCHW | {b['median']} s | {b['min']} .. {b['max']} | "
                f"{b['MPs']} MP/s; {b['vs_scaled_median']} of the scaled leg's median |")
    return "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--e2e-frames", type=int, default=256, help="0: kernel legs only")
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tensor_bench.json"))
    args = ap.parse_args()
    if args.frames < 5 or args.runs < 1 or args.e2e_runs < 1:
        ap.error("--frames >= 5, --runs >= 1, --e2e-runs >= 1")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "kernel": kernel_legs(args, dev)}
    torch.cuda.empty_cache()
    if args.e2e_frames:
        res["end_to_end"] = e2e_legs(args, dev)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(table(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
