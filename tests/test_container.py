"""The container front end (host/webp_riff.c) held to the verdicts of the parsers it replaced, and its one record
(webp_locate_still) to the three parsers that are now views of it.  CPU only; the loops run in a C driver
(tools/container_verdicts_main.c) linked against the built libvp8host.so."""
import json
import pathlib
import subprocess

import pytest

import container_cases as K

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "container_verdicts.json"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("container")
    names = K.inputs()
    K.build_driver(tmp / "verdicts", K.ROOT, with_locate=True)
    K.write_list(tmp / "list", names)
    return tmp / "verdicts", tmp / "list", names


def test_inputs_are_the_recorded_ones(driver):
    """The golden containers of at most 8 KiB (132 files, 203 kB), the two bad fixtures, the three smallest good ones --
    the files, byte for byte in length, that the recorded verdicts are about."""
    golden = json.loads(GOLDEN.read_text())
    names = driver[2]
    assert len([n for n in names if n.startswith("golden/")]) == 132
    assert len([n for n in names if n.startswith("fixtures_err/")]) == 2 and len([n for n in names if n.startswith("fixtures/")]) == 3
    assert {n: (K.ROOT / "tests" / n).stat().st_size for n in names} == golden["bytes"]
    assert golden["parsers"] == list(K.PARSERS)


def test_parsers_give_the_recorded_verdicts(driver):
    """Every input whole, cut at every length up to 2048 and at 64 lengths beyond, and with 512 seeded one-byte changes:
    the return value, the errno of a refusal and every field of an accepted file's struct (for webp_parse_anim the
    frame records too), from each of the four parsers, hash to what the parsers before the one-walk front end gave
    (tests/golden/make_container_verdicts.py)."""
    exe, lst, names = driver
    golden = json.loads(GOLDEN.read_text())["sha256"]
    got = K.verdicts(exe, lst, names)
    wrong = [(n, p) for n in names for p in K.PARSERS if got[n][p] != golden[n][p]]
    assert not wrong, f"{len(wrong)} of {len(names) * len(K.PARSERS)} differ, first {wrong[:5]}"


def test_views_equal_the_record(driver):
    """On the same cases, in each of its three modes: webp_locate_still refuses exactly where the matching parser
    refuses, with its errno, and where both accept its offsets, sizes, header fields and dimensions are the parser's
    (for a simple lossy file, whose parsers name no size: the key-frame header's, or 0 x 0 if that does not parse)."""
    exe, lst, _ = driver
    r = subprocess.run([str(exe), "views", str(lst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
