"""The banded wavefront kernels: their hand-over geometry stated once, a model of the schedule, and the shapes
the GPU tests run.

Two kernels share one scheme -- the lossless predictor (csrc/vp8g_lossless.hip, predictor_pass) and the alpha
gradient un-filter (csrc/vp8g_alpha.hip, filter 3).  One workgroup of 16 waves handles an image; a wave takes
a band of 64 rows, one row per lane; band b trails band b - 1 by `delay` steps and reads that band's bottom
row (lane 63's results) from a ring in LDS that lane 63 of the wave above writes; bands beyond the 16th wait
for the next round, and wave 15 hands its bottom row to wave 0 of the next round through a full-width row.
A step is a group of 64 columns of lane 0, the steps are separated by workgroup barriers, and a round lasts
round_len = max(n + delay, 16 delay) steps for an image of n steps a band.

What the model knows of a kernel is what lane 63 writes and what lane 0 reads in step k of a band, in the
kernel's own index arithmetic (`_lossless_io`, `_alpha_io`; each with the iteration of the step's inner loop, of four
columns, in which it happens -- a read at the iteration's start, a write at its end):
  lossless   slot = column x.  Step k writes the columns 64 k - 126 .. 64 k - 63 that lie in the image and
             reads the columns 64 k + 1 .. 64 k + 64 below the width (TR of the band's first row), and
             column 0 in step 0.
  alpha      slot = dword u of the writer's step counter t (t = column + 63 in lane 63).  Tile step k writes
             the dwords 16 k .. 16 k + 15, whatever they hold; at t4 = 64 k + 4 c lane 0 reads the dwords
             t4 / 4 + 15 (its byte 3 is column t4) and t4 / 4 + 16 (columns t4 + 1 .. t4 + 3), and uses them
             where those columns are below the width.  Both the read and the write stand between the first
             and the second barrier of a tile step (the load of the tile precedes the first, its store
             follows the second): within a step they are unordered, as in the lossless kernel, so the model
             keeps one time per step for both kernels.
A read is sound when the newest write to its slot from an EARLIER step is the band above's write of that very
column, and no write of the same step touches the slot.  `simulate` plays the schedule step by step and is
the definition; `hazards` answers the same question per read in closed form over numpy arrays (the sweep of
tests/test_bands.py needs its speed), and the two are held together on every shape below.

Columns stand for their neighbours: the steps in which a column is written and read change only at the
columns x = 0, 1, 2 (mod 64) (dwords u = 0, 15 (mod 16); `_firsts`), and the rings are multiples of 64 columns, so the
runs between those columns collide with one another exactly when their first columns do.  The model looks at
those first columns only (`every=True`: at all of them; tests/test_bands.py compares the two)."""
import collections
import functools

import numpy as np

WAVES, BAND, MAX_DIM = 16, 64, 16383

# The kernels' constants (tests/test_gpu_bands.py: equal to vp8g_lossless_geometry / vp8g_lossless_handover /
# vp8g_alpha_handover of the library).  ring and full in slots of the model AND in the kernels' own units:
# lossless pixels; alpha bytes, four to a slot.
LOSSLESS = {"unit": 64, "skew": 2, "lag": 126, "delay": 3, "ring": 256, "full": 16384 + 64, "slot": 1}
ALPHA = {"unit": 64, "lag": 63, "delay": 2, "ring": 256, "full": 16640, "slot": 4}
GEOMETRY = {"lossless": LOSSLESS, "alpha": ALPHA}
FULL_MASK = 0x7FFF  # the mask of the full-width row in both kernels ("its mask changes nothing")

# The mutants of the skew build, by the value of vp8g_band_mutant_<unit> (csrc/vp8g_skew.h: kBandMut*)
MUTANTS = {"delay": 1, "round": 2, "ring": 3, "nolong": 4}


def mutation(kernel, name):
    """The keyword arguments of hazards / simulate that make the model the named mutant of the skew build."""
    g = GEOMETRY[kernel]
    return {"delay": {"delay": g["delay"] - 1}, "round": {"round_adjust": -1}, "ring": {"ring": g["ring"] // 2},
            "nolong": {"long_round": False}}[name]


def steps_of(kernel, w, **kw):
    """Steps (groups, tiles) a band of a w-wide image takes: the kernels' ngroups / ntiles."""
    g = dict(GEOMETRY[kernel], **kw)
    if kernel == "lossless":
        g["lag"] = 63 * g["skew"]
    return (w + g["lag"] + g["unit"] - 1) // g["unit"]


def widths_of(kernel, n):
    """The widths (first, last) whose bands take n steps, clipped to 1 .. MAX_DIM; None if there is none."""
    g = GEOMETRY[kernel]
    lo, hi = max(1, g["unit"] * (n - 1) - g["lag"] + 1), min(MAX_DIM, g["unit"] * n - g["lag"])
    return (lo, hi) if lo <= hi else None


def _lossless_io(g, w, k):
    """(columns lane 63 writes, columns lane 0 reads, none read in vain) in group k of a band: predictor_pass's x0 + q - kSkew * 63
    under `x >= 0 && x < w`, and hr[0] at k = 0 with xi = x0 + q + 1 under `xi < w`."""
    G, lag = g["unit"], 63 * g["skew"]
    writes = [(k * G + i - lag, i // 4) for i in range(G) if 0 <= k * G + i - lag < w]
    reads = ([(0, 0)] if k == 0 else []) + [(k * G + i + 1, i // 4) for i in range(G) if k * G + i + 1 < w]
    return writes, reads, []


def _alpha_io(g, w, k):
    """(dwords lane 63 writes, dwords lane 0 reads and uses, dwords it reads and does not use) in tile step k of a
    band: hw32[(t4 & mask) >> 2] for every c, and d0 / d1 at pos = t4 + 60 and pos + 4, used where column t4 (d0) or
    t4 + 1 (d1) is below the width."""
    T = g["unit"]
    writes = [((k * T + 4 * c) // 4, c) for c in range(T // 4)]
    reads, idle = [], []
    for c in range(T // 4):
        t4 = k * T + 4 * c
        (reads if t4 < w else idle).append(((t4 + 60) // 4, c))
        (reads if t4 + 1 < w else idle).append(((t4 + 64) // 4, c))
    return writes, reads, idle


def _firsts(kernel, g):
    """(period, the columns within a period at which the step of a column's write or of its read changes)."""
    if kernel == "lossless":  # written from 64 k - lag on, read from 64 k + 1 on; column 0 is read apart
        return g["unit"], {0, 1, -63 * g["skew"] % g["unit"]}
    return g["unit"] // 4, {0, g["unit"] // 4 - 1}  # written from dword 16 k on, read from 16 k + 15 (d0) and 16 k + 16 (d1) on


_IO = {"lossless": _lossless_io, "alpha": _alpha_io}

SHIFTS = (-2, -1, 0, 1, 2)  # `simulate(detail=True)`: iterations the writing wave is taken to be ahead within a step

Verdict = collections.namedtuple("Verdict", "bad_reads dropped out_of_bounds")
Verdict.__bool__ = lambda v: bool(v.bad_reads or v.dropped or v.out_of_bounds)
Verdict.__doc__ = """bad_reads: reads (of the columns the model looks at) that do not find the band above's write of that
column; dropped: (band, step) pairs that no wave ever runs; out_of_bounds: accesses beyond the full-width row (reads
whose value goes unused among them)."""


@functools.lru_cache(maxsize=16)
def _columns(kernel, w, skew, every):
    """Per step of a band of a w-wide image ([(column, iteration)] written, read and used, read in vain), of the
    columns the model looks at; and (the step in which each column is written, first column, last column)."""
    g = dict(GEOMETRY[kernel], skew=skew)
    period, firsts = _firsts(kernel, g)
    keep = (lambda c: True) if every else (lambda c: c % period in firsts)
    io, cols, at = [], [], []
    for k in range(steps_of(kernel, w, **({"skew": skew} if kernel == "lossless" else {}))):
        wr, rd, idle = _IO[kernel](g, w, k)
        cols += [c for c, _ in wr]
        at += [k] * len(wr)
        io.append(([e for e in wr if keep(e[0])], [e for e in rd if keep(e[0])], [e for e in idle if keep(e[0])]))
    # every column once, in rising order, none left out: the closed form of `hazards` leans on it
    assert cols == list(range(cols[0], cols[-1] + 1))
    KW = np.full(cols[-1] + 1, -1, np.int64)
    KW[cols] = at
    return io, (KW, cols[0], cols[-1])


class _Schedule:
    """The kernel's pacing for one image: everything predictor_pass / the filter-3 branch derive from w and h."""

    def __init__(self, kernel, w, h, delay=None, ring=None, skew=None, full=None, round_adjust=0, long_round=True, every=False):
        g = dict(GEOMETRY[kernel])
        for key, v in (("delay", delay), ("ring", ring), ("skew", skew), ("full", full)):
            if v is not None:
                if key not in g:
                    raise ValueError(f"{kernel} has no {key}")
                g[key] = v
        if g["ring"] & (g["ring"] - 1) or g["ring"] % g["slot"]:
            raise ValueError("the rings are indexed through a mask")
        self.kernel, self.g, self.w, self.h = kernel, g, w, h
        self.delay = g["delay"]
        self.n = steps_of(kernel, w, **({"skew": g["skew"]} if kernel == "lossless" else {}))
        self.nbands = (h + BAND - 1) // BAND
        self.rounds = (self.nbands + WAVES - 1) // WAVES
        long = self.n + self.delay > WAVES * self.delay and long_round
        self.round_len = (self.n + self.delay if long else WAVES * self.delay) + round_adjust
        if self.round_len < 1 or self.delay < 0:
            raise ValueError("no such schedule")
        self.steps = (self.rounds - 1) * self.round_len + (WAVES - 1) * self.delay + self.n
        self.ring_mask = g["ring"] // g["slot"] - 1
        self.full_mask = FULL_MASK // g["slot"]
        # the full-width row of a launch of this image alone (lossless: sized by the width), within the most a launch gets
        self.full_slots = min(((w + 64) & ~63), g["full"]) if kernel == "lossless" else g["full"] // g["slot"]
        self.io, self.written_in = _columns(kernel, w, g["skew"] if kernel == "lossless" else 0, every)

    def band_at(self, st, wave):
        """(band, step of the band) that `wave` runs at step st, or None: the kernels' rel, p, k, b and `on`."""
        rel = st - self.delay * wave
        p = rel // self.round_len if rel >= 0 else self.rounds
        k = rel - p * self.round_len
        b = p * WAVES + wave
        return (b, k) if p < self.rounds and b < self.nbands and k < self.n else None

    def writes_rows(self, b):
        """Whether lane 63 of band b writes its results: lossless under `rowok`, alpha always."""
        return b < self.nbands and (self.kernel == "alpha" or b * BAND + 63 < self.h)

    def mask(self, wave_of_writer):
        return self.full_mask if wave_of_writer == WAVES - 1 else self.ring_mask


def simulate(kernel, w, h, detail=False, **kw):
    """The schedule played step by step.  Per step: every running wave's reads are looked up in what earlier
    steps left in the rings and the full-width row, then the step's writes are applied; a slot written twice in
    one step, or written in the step it is read in, holds nothing to rely on.
    detail: (verdict, {shift: reads that go wrong}) -- what a run sees if, within a step, every wave walks its
    sixteen iterations at the same pace and the writing wave is `shift` iterations ahead of the reading one: a
    write of iteration cw is then there for a read of iteration cr when cw - shift < cr."""
    s = _Schedule(kernel, w, h, **kw)
    state = {}  # (writer wave, slot) -> (band, column), or None after two writes in one step
    bad = oob = 0
    paced = {shift: 0 for shift in SHIFTS}
    ran = set()
    for st in range(s.steps):
        writes, reads = {}, []
        for wave in range(WAVES):
            at = s.band_at(st, wave)
            if at is None:
                continue
            b, k = at
            ran.add(at)
            wr, rd, idle = s.io[k]
            if s.writes_rows(b):
                for c, it in wr:
                    key = (wave, c & s.mask(wave))
                    writes.setdefault(key, []).append((it, (b, c)))
                    oob += wave == WAVES - 1 and key[1] >= s.full_slots
            if b:  # (band 0 reads nothing: `b ? ... : 0u`)
                src = (wave - 1) % WAVES
                for c, it in rd:
                    reads.append(((src, c & s.mask(src)), (b - 1, c), it))
                oob += sum(1 for c, _ in rd + idle if src == WAVES - 1 and c & s.mask(src) >= s.full_slots)
        bad += sum(1 for key, want, _ in reads if key in writes or state.get(key) != want)
        if detail:
            for key, want, cr in reads:
                for shift in SHIFTS:
                    there = sorted(e for e in writes.get(key, ()) if e[0] - shift < cr)
                    found = state.get(key) if not there else None if len(there) > 1 and there[-1][0] == there[-2][0] else there[-1][1]
                    paced[shift] += found != want
        state.update({key: v[0][1] if len(v) == 1 else None for key, v in writes.items()})
    dropped = sum(1 for b in range(s.nbands) for k in range(s.n) if (b, k) not in ran)
    return (Verdict(bad, dropped, oob), paced) if detail else Verdict(bad, dropped, oob)


def hazards(kernel, w, h, **kw):
    """The verdict of `simulate` without playing the steps.  Band b runs its step k at
    start(b) + k, start(b) = (b // 16) round_len + delay (b % 16), for k < min(n, round_len).  A read of column c
    by band b in its step kr is sound when the band above wrote c in an earlier step, tw < tr, and no other write
    into the same slot of the same wave -- column c + i M of band b - 1 + 16 m, M the ring -- falls into tw .. tr.
    Bands differ only in whether wave 0 runs them (the full-width row, the round's delay) and in which of the
    bands b - 1 + 16 m exist: one evaluation per such kind of band."""
    s = _Schedule(kernel, w, h, **kw)
    ne = min(s.n, s.round_len)  # steps of a band that ever run
    dropped = s.nbands * (s.n - ne)
    KW, c0, cmax = s.written_in
    rc = np.asarray([c for k in range(ne) for c, _ in s.io[k][1]], np.int64)
    rk = np.asarray([k for k in range(ne) for _ in s.io[k][1]], np.int64)
    every_read = np.asarray([c for k in range(ne) for c, _ in s.io[k][1] + s.io[k][2]], np.int64)
    wcols = np.asarray([c for k in range(ne) for c, _ in s.io[k][0]], np.int64)
    bands = np.arange(1, s.nbands)
    writers = np.asarray([s.writes_rows(x) for x in range(s.nbands)], bool)
    # the full-width row: what the writes of wave 15's bands and the reads of wave 0's reach
    oob = int(np.count_nonzero(writers[WAVES - 1::WAVES])) * int(np.count_nonzero((wcols & s.full_mask) >= s.full_slots))
    oob += int(np.count_nonzero(bands % WAVES == 0)) * int(np.count_nonzero((every_read & s.full_mask) >= s.full_slots))
    if not bands.size or not rc.size:
        return Verdict(0, dropped, oob)
    # times relative to the start of the band above: the write a read wants (-1: never made), the read by kind of band
    lo = np.where((rc >= c0) & (rc <= cmax), KW[np.clip(rc, 0, max(cmax, 0))], -1)
    lo = np.where(lo < ne, lo, -1)
    hi = {False: s.delay + rk, True: s.round_len - (WAVES - 1) * s.delay + rk}
    span = (s.nbands + WAVES - 1) // WAVES
    ms = [m for m in range(-span, span + 1)
          if any((np.minimum(hi[t] - m * s.round_len, ne - 1) >= 0).any() and (lo - m * s.round_len <= ne - 1).any() for t in hi)]
    others = bands[:, None] - 1 + WAVES * np.asarray(ms)[None, :]
    exists = (others >= 0) & (others < s.nbands) & writers[np.clip(others, 0, s.nbands - 1)]
    kinds, counts = np.unique(np.concatenate([(bands % WAVES == 0)[:, None], exists], axis=1), axis=0, return_counts=True)
    bad = 0
    for kind, count in zip(kinds, counts):
        wave0 = bool(kind[0])
        M = (s.full_mask if wave0 else s.ring_mask) + 1
        ok = (lo >= 0) & (lo < hi[wave0])
        clobbered = np.zeros(ok.shape, bool)
        for m, there in zip(ms, kind[1:]):
            if not there:
                continue
            lo_m, hi_m = lo - m * s.round_len, np.minimum(hi[wave0] - m * s.round_len, ne - 1)
            # the first column = c (mod M) that is written in step lo_m or later (the wanted write itself apart)
            first = np.searchsorted(KW[c0:], np.maximum(lo_m, 0), "left") + c0
            c1 = rc + M * -((rc - first) // M)
            if m == 0:
                c1 = np.where(c1 == rc, c1 + M, c1)
            at = KW[np.clip(c1, 0, max(cmax, 0))]
            clobbered |= (c1 <= cmax) & (at <= hi_m) & (at >= lo_m)
        bad += int(count) * int(np.count_nonzero(~ok | clobbered))
    return Verdict(bad, dropped, oob)


# ---- the shapes of tests/test_gpu_bands.py --------------------------------------------------------------------
# (w, h): what each reaches is told in DESIGN.md §17.5 / §16.7
LOSSLESS_SHAPES = [(2754, 66), (2755, 66), (2754, 1089), (2755, 1089), (300, 1089), (130, 2060), (700, 200), (12287, 2), (12288, 2),
                   (16383, 66), (5, 16383)]
LOSSLESS_LARGEST = (16383, 1026)  # 67 MB each way: a test of its own, and not among the mutant runs
LOSSLESS_ORDERS_AT = [(2755, 1089), (300, 1089), (700, 200), (16383, 66)]  # also [SG, P, CC] (fused) and [P, CC, SG] (in place)
# [CI, P] at pack 1, two pixels a byte: the predictor runs at the packed widths 2755, 300, 700 and 8192 (of the widest image)
LOSSLESS_PACKED_AT = [(2 * 2755 - 1, 1089), (600, 1089), (1400, 200), (16383, 66)]
LOSSLESS_MIXED = [(16383, 3), (5, 3), (67, 2)]  # one launch: LDS sized by the widest image
# ((2049, 1089): 33 tiles -- in the long round the ring of four tiles leaves round_len no slack at ntiles = 1 (mod 4))
ALPHA_SHAPES = [(1857, 66), (1858, 66), (1857, 1089), (1858, 1089), (2049, 1089), (300, 1089), (130, 2060), (700, 200), (16383, 66),
                (16383, 1026), (5, 16383)]
ALPHA_ALL_FILTERS = [(16383, 3), (3, 16383)]
SHAPES = {"lossless": LOSSLESS_SHAPES, "alpha": ALPHA_SHAPES}
# narrow shapes of the older tests, where the model shows what guards the simple off-by-ones
NARROW = {"lossless": [(7, 1025), (257, 130)], "alpha": [(7, 1100), (257, 66)]}

# The model's verdict per (mutant, shape of SHAPES[kernel]), as tests/test_gpu_bands.py asserts it of the skew build:
#   DIFFERS    a band's step is never run, or a read goes wrong when the waves of a step keep the same pace
#              (`simulate(detail=True)`, shift 0): the device output must differ;
#   UNSETTLED  `hazards` finds a bad read, but each of them is a race within one step that the reader wins at an
#              even pace, and at any pace within two iterations of it: nothing is asserted of the device, and the
#              pair is not run;
#   every other shape is free of hazards under the mutant: the device output must be exact.
# Every bad read of the delay, round and ring mutants is such a race within a step (the terms are tight by one
# step); those of delay and round the reader loses at an even pace (the write it wants comes in the same
# iteration or later), those of the halved ring it wins by fifteen iterations (written in the step's last iteration, read in its first): the halved ring is not
# observable on the device and is left out of the runs (GPU_MUTANTS).  tests/test_bands.py holds this table
# to the model.
DIFFERS = {
    "lossless": {
        "delay": [(2754, 66), (2755, 66), (2754, 1089), (2755, 1089), (300, 1089), (130, 2060), (700, 200), (16383, 66), (5, 16383)],
        "round": [(2754, 1089), (300, 1089), (130, 2060), (5, 16383)],
        "ring": [],
        "nolong": [(12287, 2), (12288, 2), (16383, 66)],
    },
    "alpha": {
        "delay": [(1857, 66), (1858, 66), (1857, 1089), (1858, 1089), (2049, 1089), (300, 1089), (130, 2060), (700, 200), (16383, 66),
                  (16383, 1026), (5, 16383)],
        "round": [(1857, 1089), (300, 1089), (130, 2060), (5, 16383)],
        "ring": [],
        "nolong": [(2049, 1089), (16383, 66), (16383, 1026)],
    },
}
UNSETTLED = {
    "lossless": {"delay": [], "round": [], "nolong": [],
                 "ring": [(2754, 66), (2755, 66), (2754, 1089), (2755, 1089), (300, 1089), (130, 2060), (700, 200), (16383, 66)]},
    "alpha": {"delay": [], "round": [(2049, 1089)], "nolong": [],
              "ring": [(1857, 66), (1858, 66), (1857, 1089), (1858, 1089), (2049, 1089), (300, 1089), (130, 2060), (700, 200), (16383, 66),
                       (16383, 1026)]},
}
GPU_MUTANTS = ("delay", "round", "nolong")


def classify(kernel, w, h, mutant):
    """"differs" / "unsettled" / "exact": the model's verdict on a shape under a mutant, as the table above records it."""
    v, paced = simulate(kernel, w, h, detail=True, **mutation(kernel, mutant))
    return "differs" if v.dropped or paced[0] else "unsettled" if v else "exact"
