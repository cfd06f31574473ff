"""bench.py's plain run and --dump-outputs: the sample of the outputs is the same from run to run, stays inside the streams the
step wrote and within its byte budget (no GPU); a small plain run on the GPU prints the headline line and dumps what its last
timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import datagen
import oracle


def _fake_step(nb, stride, seed):
    import torch
    import kanzi_amd as kz
    rng = np.random.default_rng(seed)
    enc = (kz.BlockResult * nb)()
    dec = (kz.BlockResult * nb)()
    d_enc = np.full((nb, stride), 255, dtype=np.uint8)                # 255 = past the end of a stream
    d_dec = np.full((nb, stride), 255, dtype=np.uint8)
    for b in range(nb):
        nbytes = int(rng.integers(1, stride + 1)) if b != 1 else stride
        enc[b].bits, enc[b].length, enc[b].skipFlags, enc[b].mode = 8 * nbytes - int(rng.integers(0, 8)), int(rng.integers(0, stride)), b & 3, 1
        dec[b].length = int(rng.integers(1, stride + 1))
        d_enc[b, :nbytes] = rng.integers(0, 255, nbytes)
        d_dec[b, :dec[b].length] = rng.integers(0, 255, dec[b].length)
    return enc, dec, torch.from_numpy(d_enc), torch.from_numpy(d_dec)


def test_dump_outputs_is_a_fixed_sample_of_the_step_within_budget(tmp_path):
    import bench
    nb, stride, budget = 6, 5000, 150000
    enc, dec, d_enc, d_dec = _fake_step(nb, stride, 3)
    sizes = bench.dump_outputs(str(tmp_path / "a"), enc, dec, d_enc, d_dec, budget)
    bench.dump_outputs(str(tmp_path / "b"), enc, dec, d_enc, d_dec, budget)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in sizes) and "encoded_sample.npy" in names and "decoded_sample.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= budget and sizes["encoded_sample"] > 2 * sizes["decoded_sample"]
    bits = np.load(tmp_path / "a" / "encode_bits.npy")
    assert bits.dtype == np.float64 and list(bits) == [r.bits for r in enc]
    assert list(np.load(tmp_path / "a" / "decode_length.npy")) == [r.length for r in dec]
    es, ds = np.load(tmp_path / "a" / "encoded_sample.npy"), np.load(tmp_path / "a" / "decoded_sample.npy")
    assert es.shape[0] == nb and ds.shape[0] == nb and es.shape[1] > 100
    assert es.max() < 255 and ds.max() < 255 and es.min() >= 0          # every position lies inside its block's stream
    assert np.isin(es[1], d_enc[1].numpy()).all() and len(np.unique(es[1])) > 100
    # another step's bytes give another sample; a budget smaller than the per-block arrays still writes every file
    enc2, dec2, d_enc2, d_dec2 = _fake_step(nb, stride, 4)
    bench.dump_outputs(str(tmp_path / "c"), enc2, dec2, d_enc2, d_dec2, budget)
    assert not np.array_equal(np.load(tmp_path / "c" / "encoded_sample.npy"), es)
    small = bench.dump_outputs(str(tmp_path / "d"), enc, dec, d_enc, d_dec, 1000)
    assert small["encoded_sample"] == small["decoded_sample"] == 4 * nb


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(built, tmp_path):
    """bench.py without --full: warm-up and --steps timed steps of the bulk batch, one JSON line with the headline keys and none of
    the --full sections; --dump-outputs holds the last step's results: at the sampled places its encoded sample is the oracle's
    block stream and its decoded sample the input."""
    import bench
    nb, distinct, bs = 6, 3, 128 * 1024
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", str(nb),
                        "--distinct", str(distinct), "--block-size", str(bs), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "u8" and line["steps"] == 2
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["config"]["round_trip_ok"] is True
    assert not {"roofline", "kernels", "cpu_baseline", "detail"} & set(line) and "chains" not in line["config"]
    bits = np.load(tmp_path / "encode_bits.npy")
    assert bits.shape == (nb,) and (bits > 0).all() and np.array_equal(bits[:distinct], bits[distinct:])   # the batch tiles its blocks
    assert list(np.load(tmp_path / "decode_length.npy")) == [bs] * nb
    total = sum(os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path) if n.endswith(".npy"))
    assert total <= bench.DUMP_BYTES
    es, ds = np.load(tmp_path / "encoded_sample.npy"), np.load(tmp_path / "decoded_sample.npy")
    assert es.dtype == ds.dtype == np.float32
    # the positions are the seeded ones dump_outputs draws: the encoded sample must be the oracle's block stream there, the
    # decoded sample the input
    src = np.stack([datagen.block(b % distinct, bs) for b in range(nb)])
    rng = np.random.default_rng(bench.DUMP_SEED)
    u = rng.random(es.shape)
    for b in range(nb):
        stream, wbits = oracle.encode_block("BWT+RANK+ZRLT", "ANS0", src[b].tobytes(), block_size=bs)[:2]
        assert bits[b] == wbits, b
        n = (wbits + 7) // 8
        pos = np.minimum((u[b] * n).astype(np.int64), n - 1)
        assert np.array_equal(es[b], np.frombuffer(stream, np.uint8)[pos].astype(np.float32)), b
    pos = np.minimum((rng.random(ds.shape) * bs).astype(np.int64), bs - 1)
    assert np.array_equal(ds, np.take_along_axis(src, pos, axis=1).astype(np.float32))
