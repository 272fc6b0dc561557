"""`bench.py --dump-outputs DIR`: a plain run (no --full) writes what the last timed
step left in the solution buffers as DIR/<name>.npy and prints ONE JSON line that
carries ms_per_step and none of the --full measurements."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("x", "u", "pi", "status", "iter")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fake_solution(torch, batch, N, dtype):
    g = torch.Generator().manual_seed(5)
    sol = {k: torch.randn(batch, n, 12, generator=g, dtype=torch.float64).to(dtype)
           for k, n in (("x", N + 1), ("u", N), ("pi", N + 1))}
    sol["status"] = torch.arange(batch, dtype=torch.int32) % 3
    sol["iter"] = torch.arange(batch, dtype=torch.int32)
    return sol


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch, dtype):
    """No GPU: dump_outputs on host tensors.  Under the size limit every QP is written; over it,
    the same sorted sample of QPs in every array and in every run, within the limit."""
    import torch
    bench = _bench()
    batch, N = 257, 3
    tdt = getattr(torch, dtype)
    sol = _fake_solution(torch, batch, N, tdt)
    bench.dump_outputs(tmp_path / "all", sol, 0, 1)
    got = {f.stem: np.load(f) for f in (tmp_path / "all").glob("*.npy")}
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        want = sol[k].numpy()
        assert got[k].dtype == (np.float32 if k in ("status", "iter") else np.dtype(dtype)), k
        assert np.array_equal(got[k], want), k

    per_qp = (3 * N + 2) * 12 * sol["x"].element_size() + 8
    limit = 100 * per_qp + per_qp // 2  # room for 100 QPs, not 101
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", limit)
    for d in ("s1", "s2"):
        bench.dump_outputs(tmp_path / d, sol, 0, 1)
    s1 = {k: np.load(tmp_path / "s1" / f"{k}.npy") for k in NAMES}
    s2 = {k: np.load(tmp_path / "s2" / f"{k}.npy") for k in NAMES}
    assert sum(a.nbytes for a in s1.values()) <= limit
    idx = s1["iter"].astype(np.int64)  # iter holds the QP index
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx[-1] < batch
    for k in NAMES:
        assert np.array_equal(s1[k], s2[k]), k
        assert np.array_equal(s1[k], got[k][idx]), k

    # ranks of an N > 1 run write their own files
    bench.dump_outputs(tmp_path / "r", sol, 1, 2)
    assert sorted(f.name for f in (tmp_path / "r").iterdir()) == sorted(f"{k}_rank1.npy" for k in NAMES)


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """The dumped arrays are bit for bit the C-ABI's solve of the same seeded shard."""
    import torch
    batch, N, steps = 600, 10, 2
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "unconstr_n10_b4096",
           "--batch", str(batch), "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(batch / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["success_rate"] == 1.0 and d["cpu_baseline"] is None
    for key in ("ipm_workloads", "sqp_pipeline", "host_buffers", "reference_call_pattern"):
        assert key not in d, key
    got = {f.stem: np.load(f) for f in (tmp_path / "out").glob("*.npy")}
    assert sorted(got) == sorted(NAMES)

    bench = _bench()
    pkg = bench.import_pkg()
    device = torch.device("cuda", 0)
    h = pkg.capi.Handle(N, 12, 12, 0, False, False, capacity=batch, device=0)
    dt, _, _, _ = bench.device_shard(pkg, h, N, "none", batch, 0, 1003, device)
    sol_t, data, sol = bench.shard_buffers(pkg.capi, dt, batch, N, "f64", device)
    h.solve_device(batch, pkg.capi.settings_struct(bench.NMPC_SETTINGS), data, sol)
    h.synchronize()
    for k in NAMES:
        want = sol_t[k].cpu().numpy()
        assert got[k].dtype == (np.float32 if k in ("status", "iter") else np.float64), k
        assert np.array_equal(got[k], want), k
