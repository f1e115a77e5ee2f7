"""bench.py's command line: --dump-outputs (CPU: the size cap and the fixed row sample; GPU: two runs with the same arguments
write the same arrays) and what a plain run leaves to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_caps_the_size_with_a_fixed_row_sample(tmp_path):
    import bench
    N, S = 4096, 64
    g = torch.Generator().manual_seed(0)
    res = {"img_coarse": torch.rand(N, 3, generator=g), "depth_rnd": torch.rand(N, generator=g),
           "xyz_camera_vis": torch.rand(N, S, 3, generator=g), "loss_sums": torch.rand(2, generator=g, dtype=torch.float64),
           "n_used": torch.arange(N, dtype=torch.int32)}
    limit = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, rows=N, limit=limit)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(res)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype in (np.float32, np.float64), k
    assert a["loss_sums"].dtype == np.float64 and a["n_used"].dtype == np.float32
    # the narrow per-ray arrays whole, the per-sample one on the recorded sample of rays
    assert a["img_coarse"].shape == (N, 3) and np.array_equal(a["img_coarse"], res["img_coarse"].numpy())
    m = json.load(open(tmp_path / "a" / "manifest.json"))
    assert m["sample"]["arrays"] == ["xyz_camera_vis"] and m["arrays"]["xyz_camera_vis"]["shape"] == [N, S, 3]
    idx = np.sort(np.random.default_rng(0).permutation(N)[:m["sample"]["kept"]])
    assert 0 < idx.size < N and np.array_equal(a["xyz_camera_vis"], res["xyz_camera_vis"].numpy()[idx])
    # under the limit: everything whole, no sample
    bench.dump_outputs(str(tmp_path / "c"), res, rows=N, limit=64_000_000)
    c = _load(tmp_path / "c")
    assert c["xyz_camera_vis"].shape == (N, S, 3) and json.load(open(tmp_path / "c" / "manifest.json"))["sample"] is None


def _bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_reproducible_outputs_and_full_adds_the_secondary_figures(tmp_path):
    base = ["--gpus", "1", "--rays", "4096", "--samples", "64", "--warmup", "1", "--settle", "0"]
    runs = [_bench(base + ["--steps", str(k), "--dump-outputs", str(tmp_path / f"d{k}")]) for k in (3, 4)]
    for k, d in zip((3, 4), runs):
        assert d["steps"] == k and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "rays/s" and d["dtype"] == "f16"
        assert d["value_at_parity"] == d["value"] and d["higher_is_better"] is True
        # a plain run times the headline workload only
        assert d["configs"] is None and d["parity_mode"] is None and d["throughput_mode"] is None and "cpu_baseline" not in d
    a, b = _load(tmp_path / "d3"), _load(tmp_path / "d4")
    assert {"img_coarse", "depth_rnd", "sil_coarse", "xyz_canonical_vis", "frame_cyc_dis", "loss_sums"} <= set(a)
    assert a["img_coarse"].shape == (4096, 3)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    full = _bench(base + ["--steps", "3", "--full", "--no-configs", "--no-cpu-baseline"])
    assert full["parity_mode"]["rays_per_s"] > 0 and full["throughput_mode"]["rays_per_s"] > 0
    assert full["fp32_parity_mode_rays_per_s"] > 0
