"""bench.py --dump-outputs DIR: what the last timed step returned, written as DIR/<name>.npy in float32, so that two builds of
the project can be compared output for output; --steps sets the number of timed steps and is validated."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("dh_bench_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_parse_dump_outputs_and_steps():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == "out"
    assert bench.parse([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_parse_full_is_off_by_default():
    bench = _bench()
    assert bench.parse([]).full is False
    a = bench.parse(["--full", "--no-phases"])
    assert a.full is True and a.phases is False


def test_dump_outputs_writes_float32_npy(tmp_path):
    bench = _bench()
    x = torch.randn(1, 8, 8, 4, generator=torch.Generator().manual_seed(0)).half()
    d = tmp_path / "dump"
    shapes = bench.dump_outputs(str(d), {"latents": x})
    assert shapes == {"latents": [1, 8, 8, 4]} and sorted(os.listdir(d)) == ["latents.npy"]
    got = np.load(d / "latents.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.float().numpy())
