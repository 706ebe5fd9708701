"""bench.py's contract: a plain run times exactly --steps steps and prints the headline line only; --dump-outputs writes the last timed
step's logits, loss and parameter gradients as float32 .npy files, the same arrays from run to run (seeded inputs, deterministic kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers

BENCH = os.path.join(helpers.ROOT, 'bench.py')
HEADLINE_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY_KEYS = ('roofline', 'roofline_mfma', 'breakdown_ms_per_step', 'small_batch', 'optimizer', 'configs')


def _load_dir(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith('.npy')}


def test_dump_outputs_stays_within_its_budget_at_fixed_positions(tmp_path, monkeypatch):
    """Over the byte budget every array is cut to the same seeded sample of its elements: two dumps of the same tensors agree."""
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 1000)
    model = torch.nn.Linear(100, 30)
    g = torch.Generator().manual_seed(1)
    model.weight.grad = torch.randn(30, 100, generator=g)
    model.bias.grad = torch.randn(30, generator=g)
    logits, loss = torch.randn(4, 5, generator=g), torch.tensor(0.25)
    for d in ('a', 'b'):
        assert bench.dump_outputs(str(tmp_path / d), logits, loss, model, 5) == 4
    a, b = _load_dir(tmp_path / 'a'), _load_dir(tmp_path / 'b')
    assert sorted(a) == ['grad.bias', 'grad.weight', 'logits', 'loss']
    assert sum(v.size for v in a.values()) * 4 <= 4 * 1000
    for k in a:
        assert a[k].dtype == np.float32
        np.testing.assert_array_equal(a[k], b[k])
    assert np.isin(a['grad.weight'], model.weight.grad.numpy().ravel()).all()


def test_dump_outputs_writes_whole_arrays_under_the_budget(tmp_path):
    import bench
    model = torch.nn.Linear(3, 2)
    model.weight.grad, model.bias.grad = torch.arange(6.0).view(2, 3), torch.tensor([1.0, -1.0])
    bench.dump_outputs(str(tmp_path), torch.arange(10.0), torch.tensor(1.5), model, 5)
    out = _load_dir(tmp_path)
    np.testing.assert_array_equal(out['logits'], np.arange(10.0, dtype=np.float32).reshape(2, 5))
    np.testing.assert_array_equal(out['grad.weight'], model.weight.grad.numpy())
    assert out['loss'] == np.float32(1.5)


def _plain_run(tmp_path, tag):
    dump = tmp_path / tag
    cmd = [sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '2', '--questions', '2', '--n-concept', '5000',
           '--dump-outputs', str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), _load_dir(dump)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    out, arrays = _plain_run(tmp_path, 'a')
    for k in HEADLINE_KEYS:
        assert k in out, k
    assert out['steps'] == 3 and out['repeats'] == 1 and len(out['repeat_ms_per_step']) == 1
    assert out['ms_per_step'] > 0 and out['value'] > 0 and out['higher_is_better'] is True
    assert out['cpu_baseline'] is None
    for k in FULL_ONLY_KEYS:
        assert k not in out, k
    assert arrays['logits'].shape == (2, 5) and arrays['loss'].shape == ()
    grads = [k for k in arrays if k.startswith('grad.')]
    assert len(grads) > 50
    assert sum(v.nbytes for v in arrays.values()) <= 64 * 2 ** 20
    for k, v in arrays.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    assert any(np.abs(arrays[k]).max() > 0 for k in grads)
    _, again = _plain_run(tmp_path, 'b')
    assert sorted(again) == sorted(arrays)
    for k in arrays:
        scale = max(float(np.abs(arrays[k]).max()), 1e-30)
        np.testing.assert_allclose(again[k], arrays[k], rtol=0, atol=1e-6 * scale, err_msg=k)
