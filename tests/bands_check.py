"""Helper of tests/test_gpu_bands.py, run as a child process with VP8G_LIB = lib/diag/libvp8g_skew.so: the banded
wavefront kernel of one unit under the skew build's LDS poison (csrc/vp8g_skew.h), every shape of
tests/bands.py against the sequential restatement -- with the shipped schedule, then with one term of the
schedule altered (the mutants).

    bands_check.py KERNEL      KERNEL: lossless alpha

prints one JSON line: {mutant: {"WxH": differing pixels, or a text if the launch did not return 0}} with mutant
"none" first; a (mutant, shape) pair that tests/bands.py calls unsettled is not run."""
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "webp-decoder_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402,F401  (first: its HIP runtime serves the process, as in conftest.py)
import vp8g  # noqa: E402
import bands  # noqa: E402


def predictor_image(rng, w, h, bits=2):
    """A w x h image whose one transform is the predictor: uniformly random residuals, every mode 0..15 in the mode
    image (and random bytes around the mode, which the kernel must ignore)."""
    r = (1 << bits) - 1
    shape = ((h + r) >> bits, (w + r) >> bits)
    junk = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFF00FF)
    modes = junk | (rng.integers(0, 16, shape).astype(np.uint32) << 8)
    res = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    return vp8g.lossless_image(res, [{"type": vp8g.L_PREDICTOR, "bits": bits, "data": modes}], width=w)


def cases(kernel):
    """[(shape, run() -> device output, expected output)]: inputs and restatement made once, launched per mutant."""
    out = []
    for k, (w, h) in enumerate(bands.SHAPES[kernel]):
        rng = np.random.default_rng(900 + k)
        if kernel == "lossless":
            im = predictor_image(rng, w, h)
            out.append(((w, h), (lambda im=im: vp8g.gpu_lossless_argb([im])[0]), vp8g.host_lossless_apply(im)))
        else:
            res = rng.integers(0, 256, (h, w), dtype=np.uint8)
            out.append(((w, h), (lambda res=res: vp8g.gpu_alpha_unfilter([res], [3], src_pad=3, guard=5)[0]), vp8g.host_alpha_unfilter(res, 3)))
    return out


def main(kernel):
    todo = cases(kernel)
    result = {}
    for mutant in ("none",) + bands.GPU_MUTANTS:
        vp8g.band_mutant(kernel, mutant)
        row = result.setdefault(mutant, {})
        for (w, h), run, want in todo:
            if mutant != "none" and (w, h) in bands.UNSETTLED[kernel][mutant]:
                continue
            try:
                row[f"{w}x{h}"] = int(np.count_nonzero(run() != want))
            except (RuntimeError, AssertionError) as e:  # (a launch that failed; bytes written outside the image)
                row[f"{w}x{h}"] = f"{type(e).__name__}: {e}"
                print(json.dumps(result))  # nothing more is launched after it
                return
    vp8g.band_mutant(kernel, "none")
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1])
