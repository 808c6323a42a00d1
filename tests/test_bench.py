"""bench.py's plain run and --dump-outputs: the headline line it prints, and the outputs it writes for comparing two builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fec_testlib as T

sys.path.insert(0, T.ROOT)
import bench  # noqa: E402


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("bits", "frames", "ret")}


def test_dump_outputs_fits_the_limit_with_a_fixed_sample(tmp_path):
    """A batch of 4096 B4 frames (4050 message bytes each) does not fit 64 MB as float32: a seeded sample of its frames is written,
    the same one every time; a small batch is written whole."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 256, (4096, 4050), dtype=np.uint8)
    ret = rng.integers(-1, 50, 128).astype(np.int32)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(np, str(a), bits, ret)
    bench.dump_outputs(np, str(b), bits, ret)
    assert sum(f.stat().st_size for f in a.iterdir()) <= bench.DUMP_LIMIT
    da, db = _load(str(a)), _load(str(b))
    assert da["bits"].dtype == np.float32 and da["ret"].dtype == np.float32 and da["frames"].dtype == np.float64
    idx = da["frames"].astype(np.int64)
    assert 0 < idx.size < 4096 and np.all(np.diff(idx) > 0) and idx[-1] < 4096
    assert np.array_equal(da["bits"], bits[idx].astype(np.float32)) and np.array_equal(da["ret"], ret.astype(np.float32))
    for k in da:
        assert np.array_equal(da[k], db[k])
    c = tmp_path / "c"
    bench.dump_outputs(np, str(c), bits[:256], ret[:8])
    dc = _load(str(c))
    assert np.array_equal(dc["frames"], np.arange(256, dtype=np.float64)) and np.array_equal(dc["bits"], bits[:256].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_what_it_decoded(tmp_path):
    """A plain run (no --full): exactly --steps timed steps, the headline fields, none of the --full parts; the dumped outputs of its
    last step are the decode of its own seeded input (first group against the CPU checker)."""
    import torch
    nf, steps = 256, 3
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(T.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--frames", str(nf), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "int8"
    assert d["metric"].startswith("FECFRAMEs/sec") and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - nf * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert d["roofline"]["launches"] > 0  # HIP events of the timed steps themselves
    for k in ("configs", "cpu_baseline", "shader_clock", "host_link", "device_copy", "demap"):
        assert k not in d, k

    got = _load(str(out))
    N, K, _, _ = T.ldpc_info("S2_TABLE_B4")
    assert got["bits"].shape == (nf, K // 8) and np.array_equal(got["frames"], np.arange(nf, dtype=np.float64))
    assert got["ret"].shape == (nf // 32,)
    x = bench.noise_llr(torch, nf, N, torch.device("cuda", 0), 12345)[:32].cpu().numpy()
    if T.ref_ldpc() is not None:
        want, wret = T.ref_ldpc_decode("S2_TABLE_B4", x, 0, 50)
    else:
        want, wret = T.oracle_ldpc_decode("S2_TABLE_B4", x, 32, 50)
    assert got["ret"][:1].tolist() == [float(v) for v in wret]
    assert np.array_equal(got["bits"][:32].astype(np.uint8), T.pack_bits(want, K))
