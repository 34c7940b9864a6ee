"""Helper of tests/test_gpu_skew.py, run as a child process with VP8G_LIB = lib/diag/libvp8g_skew.so: one
mode's hand-offs under the skewed schedule (csrc/vp8g_skew.h), every output against the
oracle / the host m05, then the same comparison with one wait's threshold a step too low (the mutants).

    skew_check.py MODE [LENGTH]      MODE: quad_plain quad_split quad_il frame m05

prints one JSON line: {"clean": {case: [differences]}, "census": {site: [satisfied, spun]},
"mutants": {site: {"bad": count, "status": [...]}}}.  `measure(mode, lengths, runs)` is the calibration of
the delay length recorded in DESIGN.md (tools: python tests/skew_check.py --measure MODE)."""
import json
import os
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import vp8g  # noqa: E402
import quad_check  # noqa: E402

# The delay after a publish, in s_sleep(127) (four times the smallest power of two at
# which every mutant was caught in five runs out of five).
LENGTH = 4
SEEDS = (0x51, 0x52, 0x53)

# MB columns 1, 2, 3, 9, 64 x MB rows 5, 9, 19 (two, three and five quads; last quads of one and of three
# rows); the wide frame at five rows only (the slot is 1024 x 80: 320 MBs, which every other size fits);
# and one frame of 160 MB rows, 20 quads per mirror-split segment: with more than 16 units between a
# frame's first unit and the last quad of the frame two places before it, the table-slot wait is also
# met already satisfied
WHOLE = [(16, 80), (32, 144), (48, 304), (144, 80), (1024, 80), (16, 304), (32, 80), (48, 144), (144, 304), (144, 144),
         (16, 2560)]
CUT = [(11, 77), (27, 141), (45, 300), (139, 80), (1019, 75), (9, 290), (32, 80), (40, 131), (144, 304), (133, 139),
       (13, 2551)]
SLOT = (1024, 80)
# the interleave takes one frame size per batch: one batch per size, MB columns x rows 1 x 5, 2 x 9, 3 x 19,
# 9 x 9 and 64 x 5 (C = 1 and 2: with dg = 2 too `need` is always the clamp Tprev; two, three and five quads,
# last quads of one and of three rows), and 3 x 32 (eight quads: 16 units per pair of frames, so that the
# table-slot wait for frame j - 4 is also met already satisfied)
IL_SIZES = {"whole": [(16, 80), (32, 144), (48, 304), (144, 144), (1024, 80), (48, 512)],
            "cut": [(11, 77), (27, 141), (45, 300), (133, 139), (1019, 75), (40, 500)]}
Q = vp8g.MODE_CHAIN | vp8g.MODE_QUAD
QUAD = {  # mode: (environment, launch-mode word, frames per workgroup, empties)
    "quad_plain": ({"VP8G_SPLITCHAIN": "0", "VP8G_CHAIN_IL": "0"}, Q, 4, True),
    "quad_split": ({"VP8G_SPLITCHAIN": "1", "VP8G_CHAIN_IL": "0"}, Q | vp8g.MODE_MIRROR_SPLIT, 4, True),
    # (seven per workgroup for the frame of 32 MB rows: the first unit of the list's frame 6 follows, on its
    # wave, a unit that itself waited for frames 0 and 1 -- the table-slot wait for frame 2 is then also met
    # already satisfied)
    "quad_il": ({"VP8G_SPLITCHAIN": "0", "VP8G_CHAIN_IL": "1"}, Q | vp8g.MODE_INTERLEAVE, 7, False),
}
MUTANTS = {"quad_plain": ("quad_need", "quad_ring0"), "quad_split": ("quad_flag",), "quad_il": (),
           "frame": ("frame_wg", "frame_part"), "m05": ()}
SITES = {"quad_plain": ("quad_need", "quad_ring0", "quad_start", "quad_slot"),
         "quad_split": ("quad_need", "quad_ring0", "quad_start", "quad_slot", "quad_flag"),
         "quad_il": ("quad_need", "quad_ring0", "quad_start", "quad_slot"),
         "frame": ("frame_wg", "frame_part"), "m05": ("m05_ring", "m05_prod", "m05_up")}


def quad(mode, length, early=-1, seeds=SEEDS, cases=("whole", "cut")):
    env, want, per_wg, empties = QUAD[mode]
    os.environ.update(env)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    for case in cases:
        batches = [([sz], sz) for sz in IL_SIZES[case]] if mode == "quad_il" else [(WHOLE if case == "whole" else CUT, SLOT)]
        for k, (sizes, slot) in enumerate(batches):
            # (the interleave's short frames: five per workgroup, what its table-slot wait needs; the
            # seven are for the 32-row frame alone, where that wait is met satisfied)
            n = (5 if mode == "quad_il" and slot[1] < 500 else per_wg) * cus + 3
            res = quad_check.run_each(n, 0x5E0 + len(case) + 16 * k, len(seeds), sizes, slot, want, empties,
                                      lambda k: vp8g.skew_set(seeds[k], length, early))
            tag = f"{case} {slot[0]}x{slot[1]}" if mode == "quad_il" else case
            for s, bad in zip(seeds, res):
                out[f"{tag} seed {s:#x}"] = bad[:6] + ([f"... {len(bad) - 1} slots"] if len(bad) > 6 else [])
    return out


# (the one of 114 MB rows: 57 row pairs, the fewest of which eight parts of 8 waves each get one -- with
# fewer the plan lowers VP8G_SPLIT=8 to four parts)
FRAME_CASES = [(16, 900, 14, 1), (333, 470, 13, 0), (64, 64, 16, 2), (1280, 720, 15, 0), (16, 1824, 18, 1)]
WIDE = (16383, 96, 17, 1)  # 1024 MB columns: the column context in device memory (global-context variant)
# (VP8G_WAVES stays unset with a split factor: a wave hint means one workgroup per frame to the plan)
FRAME_CONFIGS = [("parts 2", 2, 0), ("parts 3", 3, 0), ("parts 8", 8, 0), ("8 waves", 1, 8), ("16 waves", 1, 16), ("gctx", 1, 0)]


def frame(length, early=-1, seeds=SEEDS, census=None):
    """census: filled with the counts of each configuration on its own, {"site [config]": [satisfied, spun]}
    -- frame_part where the frame is split into parts, frame_wg where one workgroup decodes it."""
    lib = vp8g.gpu_lib()
    frames = [vp8g.synth_frame(*c) for c in FRAME_CASES]
    wide = [vp8g.synth_frame(*WIDE)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    exp = {}
    out = {}

    def one(tag, fs, filtered, split, waves, gctx):
        try:
            outs = vp8g.gpu_reconstruct_batch(fs, filtered)
        except RuntimeError as e:  # (a non-zero status word ends the call with an error)
            out[tag] = [f"error {e}"]
            return
        mode = int(lib.vp8g_last_launch_mode())
        descs = (vp8g.Vp8gFrameDesc * len(fs))(*[vp8g.make_desc(f, filtered, 0, 0) for f in fs])
        plan = vp8g.plan_launch(descs, cus, split=split, waves=waves)
        ok = (mode == plan.mode and bool(mode & vp8g.MODE_SPLIT_PARTS) == (split > 1) and not mode & vp8g.MODE_CHAIN
              and plan.quad == 0 and bool(plan.global_ctx) == gctx and plan.parts == split and (not waves or plan.waves == waves))
        bad = [] if ok else [f"launch mode {mode}: plan mode {plan.mode} parts {plan.parts} waves {plan.waves} gctx {plan.global_ctx}"]
        for f, o in zip(fs, outs):
            key = (id(f), filtered)
            if key not in exp:
                exp[key] = vp8g.oracle_reconstruct(f, filtered)
            if o != exp[key]:
                q = int(np.flatnonzero(np.frombuffer(o, np.uint8) != np.frombuffer(exp[key], np.uint8))[0])
                bad.append(f"{f.width}x{f.height} first byte {q}")
        out[tag] = bad

    for name, split, waves in FRAME_CONFIGS:
        if early == vp8g.SKEW_SITES.index("frame_wg") and split > 1:
            continue
        if early == vp8g.SKEW_SITES.index("frame_part") and split == 1:
            continue
        os.environ["VP8G_SPLIT"] = str(split)
        os.environ.pop("VP8G_WAVES", None)
        if waves:
            os.environ["VP8G_WAVES"] = str(waves)
        vp8g.skew_census()
        for s in seeds:
            vp8g.skew_set(s, length, early)
            if name == "gctx":
                one(f"gctx seed {s:#x}", wide, True, split, waves, True)
                continue
            for filtered in (False, True):
                one(f"{name} filtered {int(filtered)} seed {s:#x}", frames, filtered, split, waves, False)
        if census is not None:
            site = "frame_part" if split > 1 else "frame_wg"
            census[f"{site} [{name}]"] = vp8g.skew_census()[site]
    return out


M05_NAMES = ["coeff_y", "coeff_u", "coeff_v", "coeff_y2", "ymode", "uv_mode", "segment_id", "has_coeff", "bmode"]


def m05(length, seeds=SEEDS):
    import streams as S
    cases = [S.BY_NAME[n] for n in ("lf06", "c_mixed_320x64", "h_segdelta_n", "big_16383x16_plain")]
    cases += [c for c in S.multi_partition() if c["size"] in S.SIZES[1:5]]
    # 1024 MB columns x 12 rows = 12 288 MBs, one and a half times the ring's 8 192, every MB with its
    # tokens (no skip flag) in one partition: the modes wave runs into the ring's end
    c = S._case("skew_wrap", "p0", "plain", 0, "default", "off", (16383, 192), 21, 0)
    S.BY_NAME[c["name"]] = c
    cases.append(c)
    assert {c["log2k"] for c in cases} == {0, 1, 2, 3}
    want = []
    for c in cases:
        b = S.build(c)
        if c["log2k"] == 0:
            g = S.decode(b.data)
            want.append({k: g.array(k).copy() for k in M05_NAMES})
        else:
            pf = vp8g.PackedFrame(b.data, multi_partition=True)
            w = vp8g.unpack_coeffs(pf)
            w.update({k: pf.side(k) for k in M05_NAMES[4:]})
            want.append(w)
    out = {}
    for s in seeds:
        vp8g.skew_set(s, length, -1)
        try:
            got = vp8g.gpu_m05([S.build(c).data for c in cases], multi_partition=True)
        except RuntimeError as e:  # (a non-zero status word)
            out[f"seed {s:#x}"] = [f"error {e}"]
            continue
        out[f"seed {s:#x}"] = [f"{c['name']}: {k}" for c, g, w in zip(cases, got, want) for k in M05_NAMES
                               if not np.array_equal(g[k], w[k])]
    return out


def run_mode(mode, length, early=-1, seeds=SEEDS, **kw):
    if mode in QUAD:
        return quad(mode, length, early, seeds, **kw)
    return frame(length, early, seeds, **kw) if mode == "frame" else m05(length, seeds)


def summary(res):
    return {"bad": sum(1 for v in res.values() if v and not v[0].startswith(("status", "error", "launch mode"))),
            "status": sorted({v[0] for v in res.values() if v and v[0].startswith(("status", "error", "launch mode"))})}


def main(mode, length):
    import time
    t0 = time.time()
    vp8g.skew_census()
    per_config = {}
    clean = run_mode(mode, length, **({"census": per_config} if mode == "frame" else {}))
    t1 = time.time()
    census = per_config or {k: v for k, v in vp8g.skew_census().items() if k in SITES[mode]}
    mutants = {}
    for site in MUTANTS[mode]:
        kw = {"cases": ("whole",)} if mode in QUAD else {}
        mutants[site] = summary(run_mode(mode, length, vp8g.SKEW_SITES.index(site), **kw))
    print(json.dumps({"clean": clean, "census": census, "mutants": mutants,
                      "seconds": [round(t1 - t0, 2), round(time.time() - t1, 2)]}))


def measure(mode, lengths=(0, 1, 2, 4, 8, 16), runs=5):
    """Per delay length and mutant of `mode`: in how many of `runs` runs (one seed each) the comparison
    reported a differing output."""
    for length in lengths:
        row = {}
        for site in MUTANTS[mode]:
            kw = {"cases": ("whole",)} if mode in QUAD else {}
            hits = [summary(run_mode(mode, length, vp8g.SKEW_SITES.index(site), seeds=(0x700 + r,), **kw)) for r in range(runs)]
            row[site] = [sum(1 for h in hits if h["bad"]), sorted({s for h in hits for s in h["status"]})]
        print(json.dumps({"length": length, "caught_of_%d" % runs: row}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--measure":
        measure(sys.argv[2], *([tuple(int(x) for x in sys.argv[3].split(","))] if len(sys.argv) > 3 else []))
    else:
        main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else LENGTH)
