"""bench.py's host-side helpers (no GPU): the committed PMC summary parses into the roofline's
`traffic`, the CLI keeps the driver's flags, the oracle thread cap holds, --dump-outputs writes what it promises;
and (GPU) a plain run stays lean."""
import json
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def test_profiled_traffic_is_tied_to_the_build(tmp_path):
    """`roofline.traffic` comes from a rocprofv3 counter pass (tools/gpu_profile.sh -> profiles/*_pmc_hbm_traffic.csv); the file
    names the build it was measured on and bench.py refuses it for any other (no stale counter files)."""
    import bench
    mine = bench.build_hash()
    assert mine and len(mine) == 16
    body = ("# rocprofv3 ...\nkernel,launches,fetch_MB,fetch_x2_MB,write_MB\n"
            '"mftx::conv_gemm_kernel<128, 192, 4, 2, 1, 32, 2, 3, 0>",24,20.0,40.0,22.0\n'
            '"mftx::gru_half_kernel<2, 64, 1, 5>",24,30.0,60.0,18.0\n'
            '"mftx::ou_head_kernel<128, 5>",24,40.0,80.0,10.0\n'
            '"mftx::volume_tile_kernel",2,200.0,200.0,600.0\n')
    (tmp_path / "r9z_pmc_hbm_traffic.csv").write_text(f"# build: {mine}  (sha256 ...)\n" + body)
    traffic, source = bench.profiled_traffic(tmp_path)
    assert abs(traffic - (62e6 + 78e6 + 90e6) / 3) < 1 and source.startswith("r9z_pmc_hbm_traffic.csv") and mine in source
    (tmp_path / "r9z_pmc_hbm_traffic.csv").write_text("# build: 0123456789abcdef\n" + body)
    traffic, source = bench.profiled_traffic(tmp_path)
    assert traffic is None and "refused" in source
    (tmp_path / "r9z_pmc_hbm_traffic.csv").write_text(body)              # a file from before the rule: no build line
    assert bench.profiled_traffic(tmp_path)[0] is None
    # the committed file parses (whether or not it belongs to the library built here)
    traffic, source = bench.profiled_traffic()
    assert source and (traffic is None or 2e7 < traffic < 3e8)


def test_cli_flags_of_the_driver_contract():
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in out.stdout


def test_cli_flags_full_and_dump_outputs():
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--full", "--dump-outputs"):
        assert flag in out.stdout


def _fake_meta(H, W, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(result=SimpleNamespace(flow=torch.randn(2, H, W, generator=g), occlusion=torch.rand(1, H, W, generator=g),
                                                  sigma=torch.rand(1, H, W, generator=g)))


def test_dump_outputs_writes_the_result_planes(tmp_path):
    import bench
    meta = _fake_meta(24, 40)
    assert bench.dump_outputs(meta, tmp_path / "out") == ["flow", "occlusion", "sigma"]
    for k, shape in (("flow", (2, 24, 40)), ("occlusion", (1, 24, 40)), ("sigma", (1, 24, 40))):
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == shape
        assert np.array_equal(a, getattr(meta.result, k).numpy())


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    """Above the size limit every plane keeps the same seeded pixels, and pixel_index.npy says which: two dumps agree."""
    import bench
    meta = _fake_meta(64, 80)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 1000)
    names = bench.dump_outputs(meta, tmp_path / "a")
    assert names == ["flow", "occlusion", "pixel_index", "sigma"]
    bench.dump_outputs(meta, tmp_path / "b")
    total = 0
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) == len(np.unique(idx)) and idx.max() < 64 * 80
    for k in ("flow", "occlusion", "sigma", "pixel_index"):
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b) and a.dtype in (np.float32, np.float64)
        total += a.nbytes
    assert total <= 16 * 1000
    flat = meta.result.flow.numpy().reshape(2, -1)[:, idx.astype(np.int64)]
    assert np.array_equal(np.load(tmp_path / "a" / "flow.npy"), flat)


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times --steps steps and carries the headline keys only; --dump-outputs writes the last timed
    frame's result planes."""
    env = {k: v for k, v in os.environ.items() if k not in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["pairs_per_frame"]["timed_min"] == 7
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * d["value"] * d["ms_per_step"]
    for k in ("roofline", "kernels", "cpu_baseline", "parity", "other_arith", "host_io_fps", "api_default_fps"):
        assert k not in d, k
    for k, shape in (("flow", (2, 512, 512)), ("occlusion", (1, 512, 512)), ("sigma", (1, 512, 512))):
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), k
    assert np.abs(np.load(tmp_path / "out" / "flow.npy")).max() > 0


def test_oracle_thread_cap(monkeypatch):
    import bench
    monkeypatch.setenv("MFT_ORACLE_THREADS", "4")
    assert bench.oracle_threads() <= 4
    monkeypatch.delenv("MFT_ORACLE_THREADS")
    assert 1 <= bench.oracle_threads() <= 16


def test_committed_bench_line_has_the_contract_keys():
    lines = sorted((REPO / "profiles").glob("r[0-9]*_bench.json"))
    d = json.loads(lines[-1].read_text())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["config"]["workload"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["sample"]
