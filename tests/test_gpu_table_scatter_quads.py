"""The spatially ordered table scatter (table_scatter.hip) where its QUAD logic can fail.

The kernel locates the samples of steps 4q .. 4q + 3 of a tile in one pass -- lane (level, j) takes sample 4q + j -- and each
step reads its record from the lane of its quad that made it; a block change inside a quad repeats the pass against the new
anchors.  The cases (table_scatter_quad_cases.py; what they put in front of the kernel is checked on the reference side by
test_table_scatter_quads_cpu.py) are rows of independent 16-sample tiles, one wave each:

  counts           1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33 samples of one block, as the capacity and as a device count
                   below a capacity of 7 more (live positions with gradients behind the count)
  block change     in front of step k of a tile for every k = 0 .. 15, as the +x neighbour (shift-carry), as a block in
                   another cell of the coarsest level (whole flush, every level re-anchors) and as the +y neighbour inside one
                   coarse cell (only the finer levels re-anchor)
  two changes      inside one quad, for every quad and five pairs of steps
  dead samples     NaN and outside the cube at every step of a tile; outside the cube directly before a block change at
                   every step, which includes the first sample of a tile
  types            bf16 compute with f16 tables and with fp32 tables
  determinism      one block, one wave (1 .. 16 samples): twice, table gradient bit for bit

Per case as in test_gpu_table_scatter_walk.py and with its bars: sorted walk against the run-tracker kernel per level and
encoder (rel-L2 <= 2e-5, exactly zero where the reference is zero, MLP gradients < 2e-5) and the colour table against the fp64
scatter of the encoder gradient the gradients-out kernel wrote (2e-5); the permutation that ran is the identity the census
was taken on.  Measured on these cases: 0 .. 1.1e-6 against the tracker, 1.1e-8 .. 1.9e-7 against the fp64
scatter.

Not here: the branch that sends a sample's corners straight to the table (a cell that fp32 rounding puts one past the
lattice).  No position reaches it on this grid -- test_table_scatter_quads_cpu.py::test_no_position_reaches_the_direct_branch
gives the argument and evaluates the float32 model at the end of every block."""
import numpy as np
import pytest
import torch

import table_scatter_quad_cases as Q
from test_gpu_table_scatter_carry import T, _backward, _model, _sorted_vs_tracker, _upstream
from test_gpu_table_scatter_walk import _vs_fp64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev)


def _run(O, m, pts, count, seed, fp64=True):
    M = pts.shape[0]
    xyzs = T(np.array(pts), m.arena.device)
    counter = None if count == M else torch.tensor([count, 0], dtype=torch.int32, device=xyzs.device)
    perm = _sorted_vs_tracker(m, xyzs, counter, seed)
    assert np.array_equal(perm.cpu().numpy().astype(np.int64), np.arange(M))      # the walk the census describes
    if fp64:
        _vs_fp64(O, m, pts, count, xyzs, counter, perm)


@pytest.mark.parametrize('below_capacity', (False, True))
@pytest.mark.parametrize('n', Q.COUNTS)
def test_counts_around_a_quad(O, dev, model, n, below_capacity):
    pts = Q.one_block(n + 7 if below_capacity else n)
    _run(O, model, pts, n, 31)


@pytest.mark.parametrize('form', Q.FORMS)
def test_block_change_in_front_of_every_step(O, dev, model, form):
    pts = Q.block_change(form)
    _run(O, model, pts, pts.shape[0], 32)


def test_two_block_changes_inside_one_quad(O, dev, model):
    pts, _ = Q.two_changes()
    _run(O, model, pts, pts.shape[0], 33)


def test_dead_samples_at_every_step(O, dev, model):
    pts = Q.dead_samples()
    _run(O, model, pts, pts.shape[0], 34)


@pytest.mark.parametrize('table_dtype', (None, torch.float32))
def test_bf16_compute(O, dev, table_dtype):
    m = _model(dev, 'bf16', table_dtype)
    for pts in (Q.block_change('plus_x'), Q.two_changes()[0], Q.dead_samples()):
        _run(O, m, pts, pts.shape[0], 35, fp64=False)


def test_one_wave_one_block_is_deterministic(O, dev, model):
    """one wave, one block: nothing leaves the lattices before the final flush, so every table row gets its sums from one wave
    and in one order"""
    te = model.table_elems
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16):
        xyzs = T(Q.one_block(n), dev)
        gs, gr = _upstream(n, dev, 36)
        perm = model.sample_order(xyzs)
        g1 = _backward(model, xyzs, None, perm, gs, gr)[:te]
        g2 = _backward(model, xyzs, None, perm, gs, gr)[:te]
        assert float(np.abs(g1).sum()) > 0
        assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), n
