"""CPU: bench.py's option parsing and --dump-outputs writer (no GPU touched)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _result(seed):
    g = torch.Generator().manual_seed(seed)
    big = torch.rand((bench.DUMP_MAX_ELEMS + 1234,), generator=g)
    return {"pred": torch.rand((2, 1, 5, 7), generator=g).half(), "pred_inter_tensor": big,
            "offset": None, "aff": torch.rand((2, 9, 5, 7), generator=g), "confidence": torch.rand((2, 1, 5, 7), generator=g)}


def test_dump_outputs_writes_float32_and_samples_large_arrays_reproducibly(tmp_path):
    r = _result(3)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(r, a, 1, 0)
    bench.dump_outputs(r, b, 1, 0)
    assert sorted(os.listdir(a)) == ["aff.npy", "confidence.npy", "pred.npy", "pred_inter.npy"]
    total = 0
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 * 2 ** 20
    assert np.array_equal(np.load(os.path.join(a, "aff.npy")), r["aff"].numpy())
    assert np.array_equal(np.load(os.path.join(a, "pred.npy")), r["pred"].float().numpy())
    s = np.load(os.path.join(a, "pred_inter.npy"))
    assert s.shape == (bench.DUMP_MAX_ELEMS,)
    # the sample is a fixed, sorted subset of the flattened array
    flat = r["pred_inter_tensor"].numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(flat.size, bench.DUMP_MAX_ELEMS, replace=False))
    assert np.array_equal(s, flat[idx])
