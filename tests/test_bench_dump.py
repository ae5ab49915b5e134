"""CPU (-m "not gpu"): bench.py --dump-outputs and --steps, through bench.main() itself at N = 1 with the stand-in platform of
tests/test_bench_gloo.py (the kernel bodies compiled lane-serial on CPU tensors).  --steps K runs K timed steps after the warm-up; the dump holds the
last timed step's results as float32 / float64 .npy files within 64 MB, the same for two runs of the same arguments, and the sampled buffers' frames
and decoded bytes are those of the generator's buffers."""
import json
import os

import numpy as np
import pytest

import bench
from test_bench_gloo import _GlooPlatform


def _run(args, capsys):
    plats = []

    def factory(zj, local):
        plats.append(_GlooPlatform(zj, local)); return plats[-1]
    bench.main(args, platform_factory=factory)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), plats[0].B


def test_bench_dump_outputs_and_steps(tmp_path, capsys, monkeypatch):
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    n, size, steps = 5, 4096, 3
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--buffers", str(n), "--size", str(size), "--level", "1",
            "--skip-cpu", "--skip-lds3", "--e2e-sample", "0"]
    dumps = []
    for name in ("a", "b"):
        j, B = _run(args + ["--dump-outputs", str(tmp_path / name)], capsys)
        assert j["steps"] == steps and j["parity"]["gpu_roundtrip_exact"] is True
        assert B.calls == {"compress": 1 + steps, "pack": 1 + steps, "decompress": 1 + steps}        # warm-up + the timed steps, nothing else
        files = sorted(os.listdir(tmp_path / name))
        assert files == sorted(f + ".npy" for f in ("sample_index", "decompressed_sizes", "decompressed_sample", "compressed_sizes",
                                                   "compressed_frames_sample", "compressed_frames_sample_offsets"))
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64_000_000
        arrs = {f[:-4]: np.load(tmp_path / name / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        dumps.append(arrs)
    a, b = dumps
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)                       # same arguments, same outputs
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == n and (a["decompressed_sizes"] == size).all() and (a["compressed_sizes"] > 0).all()
    zj = B.zj
    raw = np.frombuffer(zj.synth_host(size, 0, n), dtype=np.uint8).reshape(n, size)
    assert np.array_equal(a["decompressed_sample"], raw[idx].astype(np.float32))
    off = a["compressed_frames_sample_offsets"].astype(np.int64)
    frames = a["compressed_frames_sample"].astype(np.uint8)
    for r, i in enumerate(idx):
        f = frames[off[r]:off[r + 1]].tobytes()
        assert len(f) == a["compressed_sizes"][i]
        assert B.util.emu_decompress(B.L, f, size) == raw[i].tobytes()


def test_plain_run_is_the_warm_up_and_the_timed_steps(capsys, monkeypatch):
    """without --full and without any --skip-* option, a level-3 run of the metric's mode does nothing beyond its headline: no LDS-table pass, no
    reference gates, no CPU or end-to-end legs (those fields null), the GPU round trip still checked"""
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    steps = 2
    j, B = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--buffers", "4", "--size", "4096", "--level", "3"], capsys)
    assert B.calls == {"compress": 1 + steps, "pack": 1 + steps, "decompress": 1 + steps}
    assert j["steps"] == steps and j["config"]["level"] == 3 and j["config"]["value_is"] == "both"
    assert all(j[k] is None for k in ("lds_tables_level3", "small_batch_level3", "cpu_baseline", "end_to_end", "multi_inprocess"))
    assert j["parity"] == {"gpu_roundtrip_exact": True}


def test_full_is_off_by_default_and_carries_multi():
    assert bench.parse([]).full is False and bench.parse(["--full"]).full is True
    assert bench.parse(["--full", "--multi", "inprocess"]).multi == "inprocess"
    with pytest.raises(SystemExit):
        bench.parse(["--multi", "inprocess"])


def test_bench_refuses_zero_steps():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
