#!/usr/bin/env python3
"""Writes tests/golden/container_verdicts.json: what the four container parsers of the commit BEFORE the one-walk
container front end (webp_locate_still) said about every input of tests/container_cases.py -- whole, truncated and with
single bytes changed; tools/container_verdicts_main.c lists the cases and the record format.  One sha256 per input
and parser.

The library under test is therefore not this tree's: build that parent commit in a checkout of its own and name it,

    git worktree add /tmp/parent <commit> && make -C /tmp/parent lib
    python tests/golden/make_container_verdicts.py /tmp/parent [<commit>]

The inputs and the driver are this tree's; only libvp8host.so is the parent's.  tests/test_container.py holds the
current library to the file.  Regenerate it only when inputs are added, never to make a changed parser pass.
"""
import json
import pathlib
import subprocess
import sys
import tempfile

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import container_cases as K  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    parent = pathlib.Path(sys.argv[1]).resolve()
    nm = subprocess.run(["nm", "-D", str(parent / "webp-decoder_amd" / "lib" / "libvp8host.so")], capture_output=True, text=True).stdout
    assert "webp_locate_still" not in nm, "that library already has webp_locate_still: not the parent"
    names = K.inputs()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        K.build_driver(tmp / "verdicts", parent, with_locate=False)
        K.write_list(tmp / "list", names)
        v = K.verdicts(tmp / "verdicts", tmp / "list", names)
    commit = sys.argv[2] if len(sys.argv) == 3 else subprocess.run(["git", "-C", str(parent), "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"library": "libvp8host.so of the parent commit, built in a checkout of its own", "parent_commit": commit or None,
           "cases": "tools/container_verdicts_main.c", "parsers": list(K.PARSERS),
           "bytes": {n: (K.ROOT / "tests" / n).stat().st_size for n in names}, "sha256": v}
    (HERE / "container_verdicts.json").write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(names)} inputs, {sum(doc['bytes'].values())} bytes")


if __name__ == "__main__":
    main()
