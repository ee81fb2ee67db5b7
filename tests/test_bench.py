"""bench.py's plain run and --dump-outputs: the files it writes, their types and their sizes (CPU), and on the GPU
a plain run whose dumped results are checked against the input it decoded."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_are_fixed_typed_and_bounded(tmp_path):
    """Host tensors stand in for the device buffers: the same buffers give the same files, every file is float32 or
    float64, the Adler-32 keeps its unsigned value, and the whole dump stays under 64 MB."""
    bench = _bench()
    n, L = 65536, 1024
    g = torch.Generator().manual_seed(7)
    out = torch.randint(0, 256, (n * L,), dtype=torch.uint8, generator=g)
    out_len = torch.full((n,), L, dtype=torch.int32)
    status = torch.zeros(n, dtype=torch.int32)
    adler = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, generator=g)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        bench.dump_outputs(d, "decode", n, L, out, out_len, status, adler, None, 0)
    names = sorted(os.listdir(a))
    assert names == ["adler.npy", "out_bytes.npy", "out_len.npy", "out_streams.npy", "status.npy"]
    total = 0
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += os.path.getsize(os.path.join(a, name))
    assert total <= 64 * 2**20
    assert np.array_equal(np.load(os.path.join(a, "adler.npy")), adler.numpy().view(np.uint32).astype(np.float64))
    assert np.load(os.path.join(a, "out_streams.npy")).shape == (64, L)
    assert np.load(os.path.join(a, "out_bytes.npy")).shape == (bench.DUMP_SAMPLE,)

    bound = 70000
    enc = torch.randint(0, 256, (256 * bound,), dtype=torch.uint8, generator=g)
    clen = torch.randint(100, bound, (256,), dtype=torch.int32, generator=g)
    e = str(tmp_path / "e")
    bench.dump_outputs(e, "encode", 256, L, None, clen, None, None, enc, bound)
    assert sorted(os.listdir(e)) == ["comp_len.npy", "comp_streams.npy"]
    assert np.array_equal(np.load(os.path.join(e, "comp_len.npy")), clen.numpy().astype(np.float64))
    cs = np.load(os.path.join(e, "comp_streams.npy"))
    assert cs.dtype == np.float32 and cs.shape[1] == bound


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_it_decoded(tmp_path):
    """`bench.py --gpus 1` without --full: one JSON line with the contract fields and none of the --full extras, the
    asked number of steps, and dumped results that are those of the input (every stream Ok and whole, the Adler-32 of
    the synthetic buffers)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, ROOT)
    from fdeflate_amd import synth
    n, L = 4096, 65536
    d = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(n),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", d],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0
    assert "also" not in r and "cpu_baseline" not in r
    assert np.all(np.load(os.path.join(d, "status.npy")) == 0)
    assert np.all(np.load(os.path.join(d, "out_len.npy")) == L)
    ad = np.load(os.path.join(d, "adler.npy"))
    assert ad.shape == (n,)
    for i in (0, 1, n // 2, n - 1):
        assert ad[i] == zlib.adler32(synth.gen_stream_np(i, L).tobytes()), i
