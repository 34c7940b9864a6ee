"""GPU: the banded wavefront kernels at the widths and heights the other tests do not reach (DESIGN.md §16.7,
§17.5; shapes, geometry and the model of the schedule in tests/bands.py).

The lossless predictor (csrc/vp8g_lossless.hip) against vp8f_lossless_apply and the alpha gradient un-filter
(csrc/vp8g_alpha.hip) against vp8f_alpha_unfilter, bit for bit, on uniformly random residuals -- what makes a
wrong or stale hand-over between bands run down the picture: the last width of the short round and the first
of the long one, two, three and sixteen rounds, the full-width row carrying hundreds and thousands of columns, a
launch with more than 64 KiB of dynamic LDS, the largest sizes the descriptors take; the 4K bench fixtures
against libwebp's hashes; and, in a child process per kernel on lib/diag/libvp8g_skew.so (tests/bands_check.py),
every shape again with the workgroup's LDS poisoned before every image, then with one term of the schedule
altered -- where the output must differ on exactly the shapes the model names."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bands
from bands_check import predictor_image
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SKEW_LIB = ROOT / "webp-decoder_amd" / "lib" / "diag" / "libvp8g_skew.so"
P, CC, SG, CI = 0, 1, 2, 3


def test_library_geometry_is_the_models(vp8g):
    g, a = bands.LOSSLESS, bands.ALPHA
    assert vp8g.lossless_geometry() == (g["unit"], bands.BAND, bands.WAVES)
    assert vp8g.band_handover("lossless") == (g["skew"], g["delay"], g["ring"], g["full"]) and g["lag"] == 63 * g["skew"]
    assert vp8g.band_handover("alpha") == (a["unit"], a["delay"], a["ring"], a["full"])
    assert {m: vp8g.BAND_MUTANTS.index(m) for m in bands.MUTANTS} == bands.MUTANTS


# ---- lossless ----------------------------------------------------------------------------------------------

def image(vp8g, rng, w, h, types, bits=2, pack=1):
    """As `synth` of tests/test_gpu_lossless.py: random residuals, every mode 0..15, random cross-colour bytes and tables."""
    trs, xs = [], w
    for t in types:
        r = (1 << bits) - 1
        shape = ((h + r) >> bits, (xs + r) >> bits)
        if t == P:
            junk = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFF00FF)
            trs.append({"type": P, "bits": bits, "data": junk | (rng.integers(0, 16, shape).astype(np.uint32) << 8)})
        elif t == CC:
            trs.append({"type": CC, "bits": bits, "data": rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)})
        elif t == SG:
            trs.append({"type": SG, "bits": 0})
        else:
            trs.append({"type": CI, "bits": pack, "data": rng.integers(0, 1 << 32, 11, dtype=np.uint64).astype(np.uint32)})
            xs = (xs + (1 << pack) - 1) >> pack
    res = rng.integers(0, 1 << 32, (h, xs), dtype=np.uint64).astype(np.uint32)
    return vp8g.lossless_image(res, trs, width=w)


def check_lossless(vp8g, images):
    got = vp8g.gpu_lossless_argb(images)  # (odd source offsets, guard bytes around every output)
    for k, (im, g) in enumerate(zip(images, got)):
        bad = np.argwhere(g != vp8g.host_lossless_apply(im))
        assert bad.size == 0, (k, im["width"], im["height"], [t["type"] for t in im["transforms"]], len(bad), bad[:4].tolist())


@pytest.mark.parametrize("w,h", bands.LOSSLESS_SHAPES)
def test_lossless_predictor(vp8g, w, h):
    check_lossless(vp8g, [predictor_image(np.random.default_rng(w + h), w, h)])


def test_lossless_predictor_largest(vp8g):
    """The full-width row's top columns across a round: 16383 x 1026."""
    w, h = bands.LOSSLESS_LARGEST
    check_lossless(vp8g, [predictor_image(np.random.default_rng(1), w, h)])


def test_lossless_lds_sized_by_the_widest_image_of_a_launch(vp8g):
    rng = np.random.default_rng(2)
    sizes = bands.LOSSLESS_MIXED
    assert max(w for w, _ in sizes) == bands.MAX_DIM
    check_lossless(vp8g, [predictor_image(rng, w, h) for w, h in sizes + sizes[::-1]])


ORDERS = {"fused": [SG, P, CC], "in_place": [P, CC, SG]}


@pytest.mark.parametrize("w,h", bands.LOSSLESS_ORDERS_AT)
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_lossless_fused_and_in_place_pass(vp8g, order, w, h):
    """[SG, P, CC]: cross colour on the predictor's load and add green on its store; [P, CC, SG]: the predictor as
    the last pass, reading the buffer it writes."""
    check_lossless(vp8g, [image(vp8g, np.random.default_rng(w + h + len(order)), w, h, ORDERS[order])])


@pytest.mark.parametrize("w,h", bands.LOSSLESS_PACKED_AT)
def test_lossless_predictor_at_the_packed_width(vp8g, w, h):
    """[CI, P] at two pixels a byte: the predictor runs at the packed width, the unpacking widens the rows in place."""
    im = image(vp8g, np.random.default_rng(w + h), w, h, [CI, P], pack=1)
    assert im["residual"].shape[1] == (w + 1) // 2
    check_lossless(vp8g, [im])


def test_lossless_blocks_of_512(vp8g):
    """Predictor and cross-colour blocks of 512 x 512 (bits 9) in the long round over two rounds."""
    check_lossless(vp8g, [image(vp8g, np.random.default_rng(9), 2755, 1089, [SG, P, CC], bits=9)])


def test_lossless_bench_fixtures_equal_libwebps_rgba(vp8g):
    """The 3840 x 2160 streams of tools/lossless_bench.py through the batch pipeline: libwebp's RGBA."""
    golden = json.loads((GOLDEN / "lossless.json").read_text())["bench"]
    names = sorted(golden)
    assert names == ["uhd_bands16", "uhd_flat"] and all(golden[n]["size"] == [3840, 2160] for n in names)
    files = [(GOLDEN / "lossless_bench" / f"{n}.webp").read_bytes() for n in names]
    got, st = vp8g.gpu_decode_webp_batch_tensor(files, vp8g.tensor_opt((3840, 2160), "uint8", "NHWC"), alpha=True, lossless=True)
    got = got.cpu().numpy()
    for i, n in enumerate(names):
        assert st[i] == 0 and hashlib.sha256(got[i].tobytes()).hexdigest() == golden[n]["rgba"], n


# ---- alpha ---------------------------------------------------------------------------------------------------

def check_alpha(vp8g, planes, filters):
    got = vp8g.gpu_alpha_unfilter(planes, filters, src_pad=3, guard=5)  # (padded strides, guard bytes around every plane)
    for k, (p, f, g) in enumerate(zip(planes, filters, got)):
        bad = np.argwhere(g != vp8g.host_alpha_unfilter(p, f))
        assert bad.size == 0, (k, p.shape[::-1], f, len(bad), bad[:4].tolist())


def plane(rng, w, h):
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


@pytest.mark.parametrize("w,h", bands.ALPHA_SHAPES)
def test_alpha_gradient(vp8g, w, h):
    check_alpha(vp8g, [plane(np.random.default_rng(w + h), w, h)], [3])


@pytest.mark.parametrize("w,h", bands.ALPHA_ALL_FILTERS)
def test_alpha_every_filter_at_the_largest_sizes(vp8g, w, h):
    """Also the column-0 and row-0 scans of filters 1 and 2, which live in the full-width row."""
    rng = np.random.default_rng(w)
    check_alpha(vp8g, [plane(rng, w, h) for _ in range(4)], [0, 1, 2, 3])


def test_alpha_filters_mixed_over_the_wide_shapes(vp8g):
    rng = np.random.default_rng(4)
    sizes = [(16383, 66), (1858, 1089), (16383, 3), (3, 16383), (2049, 1089), (16383, 66), (1857, 1089), (16383, 66)]
    filters = [3, 1, 3, 2, 3, 1, 2, 0]
    check_alpha(vp8g, [plane(rng, w, h) for w, h in sizes], filters)


def test_alpha_bench_fixtures_equal_libwebps_planes(vp8g):
    """The 3840 x 2160 ALPH streams of tools/alpha_bench.py: host entropy decode, device un-filter, libwebp's plane."""
    golden = json.loads((GOLDEN / "alpha.json").read_text())["bench"]
    names = sorted(golden)
    assert names == ["uhd_disc", "uhd_ramp"] and {golden[n]["filter"] for n in names} == {0, 3}
    planes, filters = [], []
    for n in names:
        res, flt, _ = vp8g.alpha_decode_host((GOLDEN / "alpha_bench" / f"{n}.alph").read_bytes(), *golden[n]["size"])
        assert flt == golden[n]["filter"]
        planes.append(res), filters.append(flt)
    got = vp8g.gpu_alpha_unfilter(planes, filters)
    for n, g in zip(names, got):
        assert hashlib.sha256(g.tobytes()).hexdigest() == golden[n]["a"], n


# ---- the skew build: poisoned LDS, and the mutants -------------------------------------------------------

_RESULTS = {}


def result(kernel):
    """The kernel's child process, run once: a child that failed, died or ran out of time fails every test of the
    kernel from the stored outcome -- nothing is started a second time on a device that just faulted."""
    if kernel not in _RESULTS:
        try:
            r = subprocess.run([sys.executable, str(ROOT / "tests" / "bands_check.py"), kernel], capture_output=True, text=True,
                               timeout=240, env=dict(os.environ, VP8G_LIB=str(SKEW_LIB)))
            if r.returncode == 0:
                _RESULTS[kernel] = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                _RESULTS[kernel] = f"exit status {r.returncode}\n{r.stderr[-2000:]}"
        except Exception as e:  # (no time left, no JSON line)
            _RESULTS[kernel] = f"{type(e).__name__}: {e}"
    assert isinstance(_RESULTS[kernel], dict), f"bands_check.py {kernel}: {_RESULTS[kernel]}"
    return _RESULTS[kernel]


def names(shapes):
    return [f"{w}x{h}" for w, h in shapes]


@pytest.mark.parametrize("kernel", ["lossless", "alpha"])
def test_exact_with_poisoned_lds(vp8g, kernel):
    """The shipped schedule in the skew build, the LDS filled with 0xA5 before every image: every shape exact."""
    row = result(kernel)["none"]
    assert list(row) == names(bands.SHAPES[kernel]) and not any(row.values()), row


@pytest.mark.parametrize("mutant", bands.GPU_MUTANTS)
@pytest.mark.parametrize("kernel", ["lossless", "alpha"])
def test_mutant_differs_where_the_model_says(vp8g, kernel, mutant):
    """One term of the schedule altered: every launch returns 0, and the output differs from the restatement on
    exactly the shapes of bands.DIFFERS -- every other shape that was run is exact."""
    row = result(kernel).get(mutant)
    ran = [sh for sh in bands.SHAPES[kernel] if sh not in bands.UNSETTLED[kernel][mutant]]
    assert row is not None and list(row) == names(ran), (row, result(kernel))
    assert all(isinstance(v, int) for v in row.values()), row
    assert [k for k, v in row.items() if v] == names(bands.DIFFERS[kernel][mutant]), row
