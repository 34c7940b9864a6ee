"""The model of the banded wavefront kernels' schedule (tests/bands.py), on the CPU:
the shipped constants are free of hazards at every number of steps a band can take and at every shape the GPU
tests run, a constant altered against a term of the kernels' static_asserts is not, and the table of what each
mutant of the skew build must show on the device is the model's."""
import numpy as np
import pytest

import bands as B

KERNELS = ("lossless", "alpha")


def heights(rounds):
    """Full rounds, and a last round of wave 0 with a whole band and wave 1 with a band of one row."""
    return {1024 * rounds, 1024 * (rounds - 1) + 65}


def sweep(kernel):
    """(w, h): per number of steps a band can take, the first, a middle and the last width that gives it, each
    with 1, 2, 3 and 16 rounds."""
    for n in range(1, B.steps_of(kernel, B.MAX_DIM) + 1):
        r = B.widths_of(kernel, n)
        if r:
            for w in sorted({r[0], (r[0] + r[1]) // 2, r[1]}):
                assert B.steps_of(kernel, w) == n
                for rounds in (1, 2, 3, 16):
                    for h in heights(rounds):
                        yield w, min(h, B.MAX_DIM)


def test_every_step_count_a_width_can_give_is_reached():
    assert {B.steps_of("lossless", w) for w in range(1, B.MAX_DIM + 1)} == set(range(2, 259))
    assert {B.steps_of("alpha", w) for w in range(1, B.MAX_DIM + 1)} == set(range(1, 258))
    for kernel in KERNELS:
        assert {B.steps_of(kernel, w) for w, _ in sweep(kernel)} == {B.steps_of(kernel, w) for w in range(1, B.MAX_DIM + 1)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_shipped_schedule_is_free_of_hazards_at_every_width(kernel):
    bad = [(w, h) for w, h in sweep(kernel) if B.hazards(kernel, w, h)]
    assert not bad, bad[:8]


def gpu_shapes(kernel):
    if kernel == "alpha":
        return B.ALPHA_SHAPES + B.ALPHA_ALL_FILTERS
    # (at pack 1 the predictor of [CI, P] runs at the packed width)
    return B.LOSSLESS_SHAPES + [B.LOSSLESS_LARGEST] + B.LOSSLESS_MIXED + [((w + 1) // 2, h) for w, h in B.LOSSLESS_PACKED_AT]


@pytest.mark.parametrize("kernel", KERNELS)
def test_closed_form_equals_the_played_schedule(kernel):
    """`hazards` against `simulate`, verdict for verdict: every GPU shape and the older tests' narrow ones, shipped and
    under every mutant, and a seeded sample of other shapes and altered constants."""
    shapes = gpu_shapes(kernel) + B.NARROW[kernel] + [(1, 1), (1, 5000), (64, 64), (65, 129), (2, 1025)]
    for w, h in shapes:
        for kw in [{}] + [B.mutation(kernel, m) for m in B.MUTANTS]:
            assert B.hazards(kernel, w, h, **kw) == B.simulate(kernel, w, h, **kw), (w, h, kw)
    rng = np.random.default_rng(5)
    for _ in range(60):
        w, h = int(rng.integers(1, 4000)), int(rng.integers(1, 3200))
        kw = {"delay": int(rng.integers(1, 5)), "ring": int(2 ** rng.integers(6, 10)), "round_adjust": int(rng.integers(-3, 2)),
              "long_round": bool(rng.integers(0, 2))}
        assert B.hazards(kernel, w, h, **kw) == B.simulate(kernel, w, h, **kw), (w, h, kw)


@pytest.mark.parametrize("kernel", KERNELS)
def test_first_columns_stand_for_their_runs(kernel):
    """Looking at the first column of every run gives the verdict of looking at every column (the count differs)."""
    for w, h in [(7, 1025), (130, 130), (257, 130), (300, 1089), (700, 200), (1000, 1100)]:
        for kw in [{}, {"skew": 3} if kernel == "lossless" else {"delay": 3}] + [B.mutation(kernel, m) for m in B.MUTANTS]:
            few, all_ = B.hazards(kernel, w, h, **kw), B.hazards(kernel, w, h, every=True, **kw)
            assert bool(few) == bool(all_) and few.dropped == all_.dropped and few.bad_reads <= all_.bad_reads, (w, h, kw)
            assert all_ == B.simulate(kernel, w, h, every=True, **kw)


@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_shapes_are_free_of_hazards(kernel):
    for w, h in gpu_shapes(kernel):
        v, paced = B.simulate(kernel, w, h, detail=True)
        assert not v and not any(paced.values()), (w, h, v, paced)


def test_gpu_shapes_hold_the_regimes_they_are_there_for():
    g, a = B.LOSSLESS, B.ALPHA
    short = lambda geo, n: n + geo["delay"] <= B.WAVES * geo["delay"]
    assert short(g, B.steps_of("lossless", 2754)) and not short(g, B.steps_of("lossless", 2755))
    assert short(a, B.steps_of("alpha", 1857)) and not short(a, B.steps_of("alpha", 1858))
    lds = lambda maxw: (B.WAVES * g["ring"] + ((maxw + 64) & ~63)) * 4  # vp8g_lossless_batch_device
    assert lds(12287) == 65536 < lds(12288) and lds(B.MAX_DIM) == 80 * 1024 <= (B.WAVES * g["ring"] + g["full"]) * 4
    rounds = lambda h: -(-(-(-h // 64)) // B.WAVES)
    assert [rounds(h) for h in (66, 1089, 2060, 16383, 1026)] == [1, 2, 3, 16, 2]
    assert B.steps_of("alpha", 2049) % 4 == 1 and not short(a, B.steps_of("alpha", 2049))
    # the packed width of (2755, .) under [CI, P] at pack 1 is the first of the long round
    assert ((2 * 2755 - 1) + 1) // 2 == 2755 and (2 * 2755 - 1, 1089) in B.LOSSLESS_PACKED_AT


@pytest.mark.parametrize("kernel", KERNELS)
def test_table_of_mutants_is_the_models(kernel):
    for mutant in B.MUTANTS:
        got = {v: [sh for sh in B.SHAPES[kernel] if B.classify(kernel, *sh, mutant) == v] for v in ("differs", "unsettled")}
        assert got["differs"] == B.DIFFERS[kernel][mutant], (mutant, got["differs"])
        assert got["unsettled"] == B.UNSETTLED[kernel][mutant], (mutant, got["unsettled"])
        # exact means free of hazards by the barriers alone, not merely at an even pace
        for sh in B.SHAPES[kernel]:
            if sh not in got["differs"] + got["unsettled"]:
                assert not B.hazards(kernel, *sh, **B.mutation(kernel, mutant)), (mutant, sh)


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_mutant_run_on_the_device_is_exposed_there(kernel):
    """Each mutant of the GPU runs differs on at least one shape (the band delay on every shape of more than one band);
    the halved ring is a hazard by the barriers (the static_assert's term is needed) that no shape shows at an even pace."""
    for mutant in B.GPU_MUTANTS:
        assert B.DIFFERS[kernel][mutant]
    assert set(B.DIFFERS[kernel]["delay"]) == {(w, h) for w, h in B.SHAPES[kernel] if h > B.BAND}
    assert set(B.MUTANTS) - set(B.GPU_MUTANTS) == {"ring"}
    assert not B.DIFFERS[kernel]["ring"] and B.UNSETTLED[kernel]["ring"]
    # the mutants that the long round alone guards against: only shapes of the long round show them
    assert all(B.steps_of(kernel, w) + B.GEOMETRY[kernel]["delay"] > B.WAVES * B.GEOMETRY[kernel]["delay"] for w, _ in B.DIFFERS[kernel]["nolong"])


# a constant against one term of the static_assert "hand-over geometry" of its kernel
ALTERED = [("lossless", {"delay": 2}),   # kDelay * kG >= kG + kLag + 1
           ("lossless", {"skew": 3}),    # the same term through kLag = 63 kSkew
           ("lossless", {"ring": 128}),  # kRing >= kDelay * kG + kG - kLag
           ("lossless", {"full": 16320}),  # (the row of the widest image a launch may hold)
           ("alpha", {"delay": 1}),      # kDelay * kT >= kT + 63
           ("alpha", {"ring": 128}),     # kRing >= (kDelay + 2) * kT
           ("alpha", {"full": 16500})]   # kFull >= 16383 + 63 + kT + 8


@pytest.mark.parametrize("kernel,altered", ALTERED)
def test_a_constant_against_a_static_assert_term_shows(kernel, altered, monkeypatch):
    (key, value), = altered.items()
    shapes = [(w, h) for w, h in sweep(kernel) if h in (1024, 1089)][::-1]
    assert any(B.hazards(kernel, w, h, **altered) for w, h in shapes)
    # and altered in the module itself, as an edit of bands.py would
    monkeypatch.setitem(B.GEOMETRY[kernel], key, value)
    assert any(B.hazards(kernel, w, h) for w, h in shapes)
    monkeypatch.undo()
    assert not any(B.hazards(kernel, w, h) for w, h in shapes[::7])


def test_slack_of_the_round_length():
    """What DESIGN.md records: in the short round round_len is tight (one step less is a hazard at every number of
    steps but the smallest, where wave 15 is through before wave 0 comes round); in the lossless long round it has
    one to three steps to spare at every width, in the alpha long round none at ntiles = 1 (mod 4)."""
    def spare(kernel, n):
        w = B.widths_of(kernel, n)[1]
        k = 0
        while not any(B.hazards(kernel, w, h, round_adjust=-k - 1) for h in (1089, 2060)):
            k += 1
        return k
    assert [spare("lossless", n) for n in (3, 20, 45)] == [0, 0, 0] and [spare("alpha", n) for n in (2, 20, 30)] == [0, 0, 0]
    assert {spare("lossless", n) for n in range(46, 259)} == {1, 2, 3}
    assert all(spare("alpha", n) == 0 for n in range(33, 257, 4)) and {spare("alpha", n) for n in range(31, 258)} == {0, 1, 2}
