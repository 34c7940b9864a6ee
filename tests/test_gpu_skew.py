"""GPU: the hand-offs between waves under a skewed schedule and poisoned context.

The progress words and flags of the quad chain (csrc/vp8g_quad.inc), of frame_kernel and its mailbox
(csrc/vp8g_kernels.hip) and of the device m05 (csrc/vp8g_m05.hip) are published a step late by producers
that usually run well ahead, and the hand-off buffers keep the previous launch's (correct) bytes: a
threshold one step too small reads finished data almost every time.  lib/diag/libvp8g_skew.so
(csrc/vp8g_skew.h) sleeps after a quarter of the publishes, fills the hand-off buffers with 0xA5 before
every launch, counts per wait site how often it was entered satisfied and how often it spun, and can lower
one wait's threshold by a step.

One child process per mode (tests/skew_check.py, VP8G_LIB set for the whole run; its result shared by the
mode's tests): three seeds per case, frames that change between launches, every output byte for byte
against oracle_reconstruct / the host m05 with status word 0; every wait site of the mode spun at least once
and passed without spinning at least once; and every mutant (one threshold a step too low) makes the same
comparison report a difference."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SKEW_LIB = ROOT / "webp-decoder_amd" / "lib" / "diag" / "libvp8g_skew.so"
MODES = ("quad_plain", "quad_split", "quad_il", "frame", "m05")
MUTANTS = [("quad_plain", "quad_need"), ("quad_plain", "quad_ring0"), ("quad_split", "quad_flag"), ("frame", "frame_wg"),
           ("frame", "frame_part")]


# wait sites whose census the mode reports (frame: one entry per configuration -- frame_part of 2, 3 and 8
# parts, frame_wg of one workgroup with 8 and with 16 waves and of the global-context variant)
N_SITES = {"quad_plain": 4, "quad_split": 5, "quad_il": 4, "frame": 6, "m05": 3}
_RESULTS = {}


def result(mode):
    """The mode's child process, run once: a child that failed, died or ran out of time fails every test of
    the mode from the stored outcome -- nothing is started a second time on a device that just faulted."""
    if mode not in _RESULTS:
        env = dict(os.environ, VP8G_LIB=str(SKEW_LIB))
        for k in ("VP8G_SPLIT", "VP8G_WAVES", "VP8G_CHAIN", "VP8G_SPLITCHAIN", "VP8G_CHAIN_IL", "VP8G_ORDER"):
            env.pop(k, None)
        try:
            r = subprocess.run([sys.executable, str(ROOT / "tests" / "skew_check.py"), mode], capture_output=True, text=True,
                               timeout=300, env=env)
            if r.returncode == 0:
                _RESULTS[mode] = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                _RESULTS[mode] = f"exit status {r.returncode}\n{r.stderr[-2000:]}"
        except Exception as e:  # (no time left, no JSON line)
            _RESULTS[mode] = f"{type(e).__name__}: {e}"
    assert isinstance(_RESULTS[mode], dict), f"skew_check.py {mode}: {_RESULTS[mode]}"
    return _RESULTS[mode]


def census_table(census):
    return "\n".join(f"{site:24s} satisfied {a:9d}  spun {b:9d}" for site, (a, b) in census.items())


@pytest.mark.parametrize("mode", MODES)
def test_bit_exact_under_skew(vp8g, mode):
    """Every case of the mode under three seeds: no differing slot, status word 0, the expected launch mode."""
    bad = {k: v for k, v in result(mode)["clean"].items() if v}
    assert len(result(mode)["clean"]) >= 3
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_every_wait_site_spun_and_passed(vp8g, mode):
    """Over the seeds of the mode, each of its wait sites was entered already satisfied at least once and
    had to spin at least once: both orders of every hand-off were met.  (frame_kernel: in each configuration
    on its own.)"""
    census = result(mode)["census"]
    assert len(census) == N_SITES[mode], census
    short = [site for site, (a, b) in census.items() if a == 0 or b == 0]
    assert not short, f"{short}\n{census_table(census)}"


@pytest.mark.parametrize("mode,site", MUTANTS)
def test_mutant_is_caught(vp8g, mode, site):
    """The site's threshold one step too low (quad_flag: the previous epoch accepted): the same comparison
    reports at least one differing output, and the status word stays 0."""
    m = result(mode)["mutants"][site]
    assert not m["status"], m
    assert m["bad"] >= 1, m
