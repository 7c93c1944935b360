"""bench.py contract on one GPU, and a 2-rank rehearsal of the multi-GPU path
(routed set/get over ShardedKV with GpuShard kernels; gloo backend so both ranks
can share the single GPU of a test box -- RCCL runs the same ShardedKV code)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--keys-per-gpu", "1000000", "--batch", "200000", "--steps", "2", "--warmup", "1", "--embed-batch", "8",
         "--embed-seq", "128", "--verify", "2000"]
FULL = ["--full", *SMALL]  # the integrity check and every measurement beside the headline


def _json(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_single_gpu_contract():
    r = subprocess.run([sys.executable, "bench.py", *FULL], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["integrity_failures"] == 0 and d["value"] > 0
    # config #2 literally (every client stream posts its own slice) beside the fused grid
    assert d["kv_async_ops_per_s"] > 0 and d["kv_async_integrity_failures"] == 0, d.get("kv_async_submission")
    assert d["kv_async_streams"] == {"writer": 32, "reader": 32}


def test_bench_plain_run_dumps_outputs(tmp_path):
    """Without --full: the headline only, the rows of everything else null, and --dump-outputs writes the
    last timed step's outputs as float32 arrays of at most 64 MB in all."""
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *SMALL, "--steps", "3", "--search-keys", "100000",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json(r.stdout)
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "ops/s"
    for k in ("kv_async_ops_per_s", "host_api_ops_per_s", "embed_e2e_vectors_per_s", "daemon_vectors_per_s",
              "search_qps", "mixed5_qps", "exchange_ratio", "integrity_source"):
        assert d[k] is None, k
    arrs = {f.stem: np.load(f) for f in out.iterdir()}
    assert set(arrs) == {"get_values", "get_status", "get_lens", "set_status", "embed_vectors", "embed_status"}
    assert all(a.dtype == np.float32 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    n = arrs["get_values"].shape[0]
    assert arrs["get_values"].shape == (n, 256) and arrs["get_lens"].shape == arrs["get_status"].shape == (n,)
    assert (arrs["get_status"] == 0).all() and (arrs["get_lens"] == 150).all() and (arrs["set_status"] == 0).all()
    rows = arrs["get_values"].astype(np.uint8)
    assert all(bytes(row[:4]) == b"ver:" for row in rows) and not rows[:, 150:].any()
    assert arrs["embed_vectors"].shape == (8, 768) and np.isfinite(arrs["embed_vectors"]).all()
    assert (arrs["embed_status"] == 0).all()


def test_bench_two_rank_rehearsal_gloo():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2",
                        "--backend", "gloo", *FULL, "--search-keys", "2000000"],  # two ranks share one GPU's HBM
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    d = _json(r.stdout)
    assert d["n_gpus"] == 2 and d["integrity_failures"] == 0
    assert d["kv_ok"] >= 0.999 * d["config"]["global_batch"] * 2  # routed ops of the 2 timed steps succeeded
