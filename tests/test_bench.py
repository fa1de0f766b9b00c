"""bench.py command-line contract on CPU (tiny model): the result line,
--steps, --dump-outputs and --full."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench  # repository root is on sys.path (conftest.py)

ROOT = os.path.dirname(os.path.abspath(bench.__file__))

TINY = [
    "--gpus", "1", "--model", "tiny", "--global-batch", "3",
    "--width", "64", "--height", "64", "--denoise-steps", "2",
]


def _run(extra):
    env = {
        k: v for k, v in os.environ.items()
        if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")
    }
    # CPU path regardless of the machine (the tiny model is a CPU fixture)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py")] + TINY + extra,
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=120,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Two plain runs with different step counts, both dumping outputs."""
    d = tmp_path_factory.mktemp("bench")
    r1 = _run(["--steps", "2", "--warmup", "1",
               "--dump-outputs", str(d / "a")])
    r2 = _run(["--steps", "1", "--warmup", "0", "--full",
               "--dump-outputs", str(d / "b")])
    return d, r1, r2


class TestBenchCli:
    def test_result_line_fields(self, dumped):
        _, r1, r2 = dumped
        for r, steps, warmup in ((r1, 2, 1), (r2, 1, 0)):
            for key in ("metric", "value", "unit", "higher_is_better",
                        "dtype", "ms_per_step"):
                assert key in r
            assert r["steps"] == steps and r["warmup"] == warmup
            assert r["unit"] == "images/sec" and r["higher_is_better"] is True
            assert r["dtype"] == "fp32"
            assert r["ms_per_step"] > 0
            # value is global_batch images per step of ms_per_step
            assert r["value"] == pytest.approx(
                3 * 1000.0 / r["ms_per_step"], rel=1e-2
            )

    def test_dump_files(self, dumped):
        d, _, _ = dumped
        assert sorted(os.listdir(d / "a")) == ["images.npy", "seeds.npy"]
        images = np.load(d / "a" / "images.npy")
        seeds = np.load(d / "a" / "seeds.npy")
        assert images.dtype == np.float32 and images.shape == (3, 64, 64, 3)
        assert seeds.dtype == np.float64 and seeds.shape == (3,)
        assert images.min() >= 0 and images.max() <= 255
        assert images.std() > 0

    def test_dump_identical_run_to_run(self, dumped):
        d, _, _ = dumped
        for name in ("images.npy", "seeds.npy"):
            assert np.array_equal(np.load(d / "a" / name),
                                  np.load(d / "b" / name))

    def test_rejects_zero_steps(self):
        proc = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
            cwd=ROOT, capture_output=True, text=True, timeout=120,
        )
        assert proc.returncode == 2


class TestDumpOutputs:
    def _res(self, n, h, w):
        g = torch.Generator().manual_seed(3)
        images = torch.randint(0, 256, (n, h, w, 3), generator=g,
                               dtype=torch.uint8)
        return SimpleNamespace(images=images, seeds=list(range(10, 10 + n)))

    def test_small_gallery_written_whole(self, tmp_path):
        res = self._res(2, 8, 8)
        bench.dump_outputs(str(tmp_path), res)
        out = np.load(tmp_path / "images.npy")
        assert np.array_equal(out, res.images.numpy().astype(np.float32))
        assert np.load(tmp_path / "seeds.npy").tolist() == [10.0, 11.0]

    def test_large_gallery_is_fixed_seeded_sample(self, tmp_path, monkeypatch):
        monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
        res = self._res(4, 16, 16)  # 3072 elements > 1000
        bench.dump_outputs(str(tmp_path / "x"), res)
        bench.dump_outputs(str(tmp_path / "y"), res)
        x = np.load(tmp_path / "x" / "images.npy")
        assert x.dtype == np.float32 and x.shape == (1000,)
        assert np.array_equal(x, np.load(tmp_path / "y" / "images.npy"))
        idx = np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(
            0, res.images.numel(), size=1000
        )
        assert np.array_equal(
            x, res.images.reshape(-1).numpy()[idx].astype(np.float32)
        )

    def test_budget_is_under_64_mb(self):
        assert bench.DUMP_MAX_ELEMS * 4 <= 64 * 1024 * 1024 // 2
