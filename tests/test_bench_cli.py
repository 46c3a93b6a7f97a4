"""bench.py's launcher contract on a machine without GPUs: `--gpus N` must never silently run a smaller job."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, env=e,
                          timeout=300)


def test_gpus_flag_without_enough_gpus_is_refused():
    import torch
    if torch.cuda.device_count() >= 4:
        import pytest
        pytest.skip('enough GPUs here')
    r = _run(['--gpus', '4', '--steps', '1', '--warmup', '0'])
    assert r.returncode == 2 and 'refusing' in r.stderr and '"n_gpus"' not in r.stdout


def test_world_size_mismatch_is_refused():
    r = _run(['--gpus', '8', '--steps', '1', '--warmup', '0'], env={'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '2'})
    assert r.returncode == 2 and 'does not match' in r.stderr and '"n_gpus"' not in r.stdout


def test_dump_outputs_keeps_a_seeded_sample_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    labels = np.arange(6 * 8 * 8, dtype=np.int64).reshape(6, 8, 8) + 10000
    big = np.zeros((6, 4), np.int64)
    big[:, 0] = 2 ** 40                      # not exact in float32: written as float64
    monkeypatch.setattr(bench, 'DUMP_BYTES', 3 * (8 * 8 * 4 + 4 * 8))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'labels': labels, 'big': big})
    a = np.load(tmp_path / 'a' / 'labels.npy')
    idx = np.load(tmp_path / 'a' / 'labels_index.npy').astype(np.int64)
    assert a.dtype == np.float32 and a.shape == (3, 8, 8) and len(idx) == 3 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a, labels[idx].astype(np.float32))
    g = np.load(tmp_path / 'a' / 'big.npy')
    assert g.dtype == np.float64 and np.array_equal(g, big[idx].astype(np.float64))
    assert np.array_equal(a, np.load(tmp_path / 'b' / 'labels.npy'))
    bench.dump_outputs(str(tmp_path / 'c'), {'labels': labels[:2]})        # fits: everything, no index file
    assert np.array_equal(np.load(tmp_path / 'c' / 'labels.npy'), labels[:2].astype(np.float32))
    assert not (tmp_path / 'c' / 'labels_index.npy').exists()


def test_dump_outputs_is_refused_outside_the_tiles_workload():
    r = _run(['--workload', 'stack3d', '--steps', '1', '--warmup', '0', '--dump-outputs', 'unused'])
    assert r.returncode == 2 and 'tiles workload' in r.stderr
