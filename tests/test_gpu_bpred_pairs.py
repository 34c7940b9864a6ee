"""The quad kernel's B_PRED wavefront with three or four B_PRED MBs in a step (csrc/vp8g_quad.inc, the
`else if (bp_lane)` arm: sub-steps 2..7 run both groups as one pass, lanes 0..7 / 8..15 of a quarter
taking group 0's / group 1's sub-block, two pixels a lane).

The synthetic profiles carry 10-20 % B_PRED MBs and the directed kinds none but bpred_all, so steps with
exactly three or four B_PRED MBs beside whole-block MBs are what the suite lacked.  The frames here are
profile-2 synthetic frames (bmode 0..15 in every MB: every mode and the out-of-range ones) with ymode = 4
on a seeded 50 %, 75 % and 100 % of the MBs and has_coeff made to tell the truth again, at

  112x64   7 x 4 MBs: seven columns is the narrowest frame in which all four quarters are active in a step
  112x112  7 x 7 MBs: the second quad has three rows
  96x48    6 x 3 MBs: three rows is the shortest frame that reaches the arm; at most three quarters active
  107x59   cut right pieces and unaligned rows: the kernel's general instantiation

The host-only test walks the quad schedule -- quarter h of quad k works on MB (4 k + h, t - 2 h) at step
t -- over these frames and asserts what they reach; the GPU tests decode them through the chain, filtered
and unfiltered, every slot against the oracle.  Reference path: src/m06_recon/vp8_recon.c:218-358 (the
sub-block predictors), :444-684 (the MB driver).
"""
import sys

import numpy as np
import pytest

import directed as D
from conftest import ROOT

WHOLE_SIZES = [(112, 64), (112, 112), (96, 48)]
GENERAL_SIZE = (107, 59)
SHARES = (0.5, 0.75, 1.0)
SEED = 6  # (searched on the CPU: the smallest for which test_frames_reach_the_three_or_four_arm holds)


def build(vp8g, width, height, share, seed):
    """A profile-2 synthetic frame with ymode = 4 on a seeded `share` of its MBs."""
    f = vp8g.synth_frame(width, height, seed, profile=2)
    rng = np.random.default_rng([0xB4ED, width, height, int(share * 100), seed])
    n = f.mb_total
    ym = f.array("ymode")
    ym[ym == 4] = 0  # (the profile's own B_PRED MBs: the share below is the whole of them)
    ym[rng.permutation(n)[:int(round(share * n))]] = 4
    has = D.coded(f)
    f.array("has_coeff")[:] = has
    f.array("skip_coeff")[:] = ~has
    return f


def frames_for(vp8g, sizes, copies=2):
    """Every size at every share, twice in a row: quad_check.run decodes the frame at an even position
    unfiltered and the one at an odd position filtered (and frees each, so the two are separate frames)."""
    return [build(vp8g, w, h, share, SEED + 16 * k + i) for k, (w, h) in enumerate(sizes) for i, share in enumerate(SHARES)
            for _ in range(copies)]


def arm_steps(f):
    """The steps of the quad schedule in which three or four of the wave's MBs are B_PRED:
    [(B_PRED quarters, active quarters, [that step's B_PRED MB indices])]."""
    rows, cols = int(f.frame.mb_rows), int(f.frame.mb_cols)
    bp = (f.array("ymode") == 4).reshape(rows, cols)
    out = []
    for r0 in range(0, rows, 4):
        for t in range(cols + 6):
            act = [h for h in range(4) if r0 + h < rows and 0 <= t - 2 * h < cols]
            on = [h for h in act if bp[r0 + h, t - 2 * h]]
            if len(on) >= 3:
                out.append((tuple(on), tuple(act), [(r0 + h) * cols + t - 2 * h for h in on]))
    return out


def test_frames_reach_the_three_or_four_arm(vp8g):
    """Host only: over the chosen frames the schedule has steps with exactly three and exactly four B_PRED
    MBs; among the steps with three beside a whole-block MB, that MB sits in each of the four quarters;
    steps with three B_PRED MBs and an idle fourth quarter occur (three-row quads); and in such steps
    every mode 0..9 and an out-of-range mode occur in group 0 and in group 1 of the sub-steps 2..7."""
    frames = frames_for(vp8g, WHOLE_SIZES + [GENERAL_SIZE], copies=1)
    counts = {3: 0, 4: 0}
    odd_quarter, idle_quarter = set(), 0
    modes = (set(), set())
    for f in frames:
        bm = f.array("bmode").reshape(-1, 16)
        for on, act, mbs in arm_steps(f):
            counts[len(on)] += 1
            if len(on) == 3 and len(act) == 4:
                odd_quarter |= set(act) - set(on)
            idle_quarter += len(on) == 3 and len(act) == 3
            for s in range(2, 8):  # group g's sub-block at sub-step s: (i0 + g, s - 2 i0 - 2 g)
                i0 = 0 if s <= 3 else (s - 2) >> 1
                b0 = 4 * i0 + (s - 2 * i0)
                for g in range(2):
                    modes[g].update(int(m) for m in bm[mbs, b0 + 2 * g])
        f.free()
    print(f"steps with 3 / 4 B_PRED MBs: {counts[3]} / {counts[4]}; three-row steps: {idle_quarter}; "
          f"the whole-block MB's quarter: {sorted(odd_quarter)}; modes: {sorted(modes[0])} / {sorted(modes[1])}")
    assert counts[3] > 0 and counts[4] > 0, counts
    assert odd_quarter == {0, 1, 2, 3}, odd_quarter
    assert idle_quarter > 0, idle_quarter
    for g in range(2):
        assert modes[g] >= set(range(10)) and max(modes[g]) >= 10, (g, sorted(modes[g]))


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["whole", "general"])
def test_quad_chain_three_or_four_bpred_mbs(vp8g, general):
    """The frames above through the quad chain, each filtered and unfiltered, every slot against the
    oracle: the whole-piece sizes alone (the lean instantiation), and with 107x59 among them (a batch
    with one cut frame takes the general instantiation)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import quad_check
    frames = frames_for(vp8g, WHOLE_SIZES + ([GENERAL_SIZE] if general else []))
    bad = quad_check.run(n=1200, seed=0xB9ED + general, frames=frames)
    assert not bad, f"{len(bad)} slots differ, e.g. {bad[:8]}"
