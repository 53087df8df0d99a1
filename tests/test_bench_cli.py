"""bench.py's command line and its --dump-outputs writer (no GPU: the frames here are host tensors)."""
import importlib
import os
import sys

import numpy as np
import pytest


@pytest.fixture()
def bench(monkeypatch):
    monkeypatch.setenv("RTG_BENCH_QUEUES_AS_GIVEN", "1")     # importing bench.py must not touch the queue count here
    monkeypatch.setattr(sys, "path", list(sys.path))
    return importlib.import_module("bench")


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_frames(bench, tmp_path):
    import torch
    hdr = torch.arange(5 * 7 * 3, dtype=torch.float32).reshape(5, 7, 3) / 3
    ldr = (torch.arange(5 * 7 * 3) % 251).to(torch.uint8).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "out"), {"hdr": hdr, "ldr": ldr})
    got_h, got_l = np.load(tmp_path / "out" / "hdr.npy"), np.load(tmp_path / "out" / "ldr.npy")
    assert got_h.dtype == got_l.dtype == np.float32
    assert np.array_equal(got_h, hdr.numpy()) and np.array_equal(got_l, ldr.numpy().astype(np.float32))


def test_dump_outputs_samples_within_the_budget(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * (4096 + 40 * 12))     # 40 pixels of 3 floats per frame
    frame = torch.arange(9 * 11 * 3, dtype=torch.float32).reshape(9, 11, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"hdr": frame, "ldr": frame * 2})
    a, b = np.load(tmp_path / "a" / "hdr.npy"), np.load(tmp_path / "b" / "hdr.npy")
    assert a.shape == (40, 3) and np.array_equal(a, b)                  # the same sample every run
    first = a[:, 0].astype(np.int64)
    assert np.all(np.diff(first) > 0) and np.all(first % 3 == 0)        # whole pixels, in frame order
    assert np.array_equal(a, frame.reshape(-1, 3).numpy()[first // 3])
    assert np.array_equal(np.load(tmp_path / "a" / "ldr.npy"), 2 * a)   # the same pixels of every frame
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET
