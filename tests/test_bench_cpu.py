"""bench.py's command line and its output dump, without a device: a plain run leaves the after-run checks to --full, and
--dump-outputs writes float32 / float64 arrays within 64 MB, the same ones for the same inputs."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_leaves_the_checks_to_full(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'out')
    assert a.full and a.dump_outputs == 'out'


def test_dump_outputs_dtypes_size_and_determinism(tmp_path):
    te = 2 * bench.DUMP_TABLE_SAMPLE
    g = torch.Generator().manual_seed(0)
    model = types.SimpleNamespace(arena=torch.nn.Parameter(torch.randn(te + 15360, generator=g)), table_elems=te)
    n, nc = 1008 * 756, 20                     # more per-pixel bytes than the dump keeps: a seeded sample of rows
    ids = torch.arange(n, dtype=torch.float32)
    pixels = {'rgb_map': ids[:, None].repeat(1, 3), 'trans_map': ids.clone(), 'classes': (ids[:, None] % 2048).repeat(1, nc).half()}
    loss = torch.tensor(1.25)
    bench.dump_outputs(str(tmp_path / 'a'), model, loss, 4321, pixels)
    bench.dump_outputs(str(tmp_path / 'b'), model, loss, 4321, pixels)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    assert {'loss.npy', 'samples.npy', 'params_mlp.npy', 'params_table_sample.npy', 'rgb_map_rows_sample.npy'} <= set(names)
    total = 0
    arrays = {}
    for f in names:
        x = np.load(tmp_path / 'a' / f)
        assert x.dtype in (np.float32, np.float64), (f, x.dtype)
        assert np.array_equal(x, np.load(tmp_path / 'b' / f)), f
        total += x.nbytes
        arrays[f[:-4]] = x
    assert total <= 64 * 1000 * 1000
    assert float(arrays['loss'][0]) == 1.25 and float(arrays['samples'][0]) == 4321.0
    assert np.array_equal(arrays['params_mlp'], model.arena.detach()[te:].numpy())
    # every per-pixel array keeps the same rows, in pixel order
    rows = arrays['trans_map_rows_sample'][:, 0]
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(arrays['rgb_map_rows_sample'][:, 2], rows) and np.array_equal(arrays['classes_rows_sample'][:, -1], rows % 2048)
