"""GPU: a plain `bench.py --dump-outputs DIR` run on a small uhd4 batch: --steps sets the timed steps, the
result line carries ms_per_step and no --full object, and DIR/i420_sample.npy holds exactly the bytes
of each slot's I420 (the C restatement's output for fixture i % 4) at the seeded positions, twice the
same.  Reference path: src/m06_recon/vp8_recon.c:718 + m07 per frame (oracle/vp8_oracle.c)."""
import json
import sys

import numpy as np
import pytest

from conftest import FIXTURES, ROOT

pytestmark = pytest.mark.gpu

N = 6  # slots 4, 5 are second copies of fixtures 0, 1


def _run(bench, capsys, out_dir):
    bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", str(N), "--dump-outputs", str(out_dir)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), np.load(out_dir / "i420_sample.npy")


def test_plain_run_dumps_the_timed_outputs(tmp_path, capsys, vp8g):
    sys.path.insert(0, str(ROOT))
    import bench
    line, got = _run(bench, capsys, tmp_path / "a")
    assert line["steps"] == 3 and len(line["kernel_ms_steps"]) == 3 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (ms_per_step is rounded to 1 us, value to 0.1)
    assert line["value"] == pytest.approx(N * 3840 * 2160 / 1e6 / (line["ms_per_step"] * 1e-3),
                                          rel=0.0006 / line["ms_per_step"] + 1e-4)
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("MP/s", True, "u8")
    assert line["cpu_baseline"] is None and line["parity"].startswith("not checked")
    assert not {"workloads", "encode", "end_to_end", "parity_failure"} & set(line)

    i420 = vp8g.i420_size(3840, 2160)
    s = min(i420, bench.DUMP_VALUES // N)
    assert got.dtype == np.float32 and got.shape == (N, s) and got.nbytes <= 64 << 20
    want = []
    for rel in bench.UHD:
        f = vp8g.decode_file(FIXTURES / rel)
        want.append(np.frombuffer(vp8g.oracle_reconstruct(f, True), dtype=np.uint8))
        f.free()
    for i in range(N):
        idx = bench.dump_positions(i420, s, i)
        # one position in each of s equal strata: distinct, and every plane and MB row is sampled
        assert idx.shape == (s,) and np.array_equal(idx // (i420 // s), np.arange(s))
        assert i == 0 or not np.array_equal(idx, bench.dump_positions(i420, s, i - 1))
        assert np.array_equal(got[i], want[i % 4][idx].astype(np.float32)), f"slot {i}"

    _, again = _run(bench, capsys, tmp_path / "b")
    assert np.array_equal(got, again)
