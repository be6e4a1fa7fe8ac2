"""The spatially ordered table scatter (table_scatter.hip) where a wave walks MORE THAN ONE 16-sample tile.

The launch partition this file relies on (restated in table_scatter_cases.launch_model from nsr_table_scatter_launch and the
head of k_table_scatter): nblocks = max(1, min(4096, ceil(ceil(M / 16) / 4))) workgroups of 4 waves for a capacity of M
slots, and with Mc the device count every wave takes per = ceil(ceil(Mc / 16) / (4 nblocks)) consecutive tiles.  Up to
262 144 samples per == 1, which is all the synthetic cases of test_gpu_table_scatter_carry.py reach (its marched patch
does run more than one tile a wave, judged by one aggregate per level against the tracker); production batches (90 000 rays and more)
run per >= 2, where the block key, the lattices, the ring of gradient rows, the next tile's positions and -- from per == 3,
above 524 288 samples -- the permutation entries fetched two tiles ahead are carried across a tile boundary.  The cases:

  two_tiles             262 144 + 5 samples: 8 192 waves with two tiles, one with a tile of 5 samples, 8 191 with none
  threshold             its first 262 144: per == 1 with every one of the 16 384 waves busy, the largest single-tile launch
  long_blocks           ~270 000 samples in blocks of 20 .. 40, which span the boundaries
  three_tiles           524 288 + 16 + 7: per == 3, the last busy wave has one tile of 7 samples
  count_in_second_tile  capacity 300 000, device count 262 144 + 16 + 9: the count ends at lane 9 of the last busy wave's
                        second tile, with live positions and non-zero upstream gradients behind it

Blocks of 1 .. 5 samples from the carry test's generators (x-runs of four, gaps of 2 and 5, 2 x 2 Morton groups, dead samples
between neighbours) plus points exactly on block faces, spread over the whole encoded range of block coordinates.

What keeps this from passing vacuously is checked on the reference side by test_table_scatter_walk_cpu.py, and here the
permutation that ran is compared with the NumPy walk order those checks use:
  * launch: the per, full, short and empty wave counts above (count_in_second_tile: 8 193 full waves, the count 9 lanes into
    the second tile of the last);
  * census of the interior tile boundaries (between two tiles of one wave), by the last live sample before and the first
    after: for two_tiles, long_blocks and three_tiles at least 100 each of (a) same block, (b) the +x neighbour with y and z
    equal -- the shift-carry of the block-anchored levels --, (c) any other block change, (d) a dead sample in lane 15 of the
    first tile, (e) a dead sample in lane 0 of the second; long_blocks: at least 100 strictly inside a block of 20 samples or
    more; three_tiles: at least 100 each of (a), (b), (c) separately at the first -> second and the second -> third boundary;
  * row load: no table row of any level receives more than 1 500 contributions, so the derivation of the 2e-5 bar in
    test_gpu_table_scatter_carry.py's docstring carries over unchanged (largest loads: 1 237 .. 1 406 on level 0).  Every
    level of this grid is hashed and the coarse levels' hash is uneven, which is why a fifth of the samples (more than half
    in three_tiles) are dead: see table_scatter_cases._Places;
  * the fp64 bincount scatter against the oracle's own fp32 encoder backward, per level, on two_tiles and long_blocks with a
    seeded encoder gradient of the magnitudes read back here (mean -0.008, std 0.28): rel-L2 5.5e-8 .. 5.0e-7 (bar 1e-5).
  * a host model of three mistakes in the code that carries state into a wave's next tile (the ring's wrap refill or the
    next tile's positions read through this tile's permutation entries; the entries two tiles ahead never fetched) scatters,
    on two_tiles and three_tiles, a result 0.58 .. 1.1 in rel-L2 away from the right one on every level; the last of the
    three changes nothing below three tiles a wave, so three_tiles alone can tell it (table_scatter_cases.walk_inputs).

Per case, as in the carry test and with its bars (reference LLFF grid, f16 tables, f16 compute, nc = 5): sorted walk against
the run-tracker kernel per level and encoder (rel-L2 <= 2e-5, exactly zero where the reference is zero, MLP gradients
< 2e-5), and the colour table against the fp64 scatter of the encoder gradient the gradients-out kernel wrote (2e-5; the
density table exactly zero).  count_in_second_tile also against the truncated batch and with NaN behind the count;
two_tiles also with bf16 compute and fp32 tables, and twice with one permutation (rel-L2 <= 2e-6: the same arithmetic,
atomics order only).

Not reached: the branch fmaxf(d0, d1, d2) > Sm2 of the kernel (a cell that fp32 rounding puts one past the lattice, direct
atomics).  For both grids the suite uses (min_res 16 and 2, 16 levels up to 4096) and every block group of every level, the
largest fp32 u of the group against the group's anchor was evaluated on the CPU: no position reaches the branch."""
import numpy as np
import pytest
import torch

import table_scatter_cases as C
from helpers import rel_l2
from test_gpu_table_scatter_carry import NC, T, _backward, _check_per_level, _model, _sorted_vs_tracker, _upstream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev)


def _inputs(name, dev):
    pts, count = C.walk_case(name)
    M = pts.shape[0]
    counter = None if count == M else torch.tensor([count, 0], dtype=torch.int32, device=dev)
    return pts, count, T(np.array(pts), dev), counter               # a copy: the shared case is read-only


def _assert_walk(perm, pts, count):
    """the permutation that ran is the one the CPU census was taken on"""
    ph = perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(ph[:count], C.walk_order(pts, count))
    assert np.array_equal(ph[count:], np.arange(count, pts.shape[0]))


def _vs_fp64(O, m, pts, count, xyzs, counter, perm):
    """colour table only, unit upstream gradients; the encoder gradient is what the gradients-out kernel wrote"""
    M = pts.shape[0]
    gs = torch.zeros(M, device=xyzs.device)
    gr = torch.ones(M, 3 + NC, device=xyzs.device)
    m.train_density_table = False
    try:
        g = _backward(m, xyzs, counter, perm, gs, gr)
        genc = m._bwd_ws[:M * 64].view(M, 16, 4)[:count, :, 2:4].cpu().numpy()
    finally:
        m.train_density_table = True
    assert np.array_equal(m._offsets_np, C.level_offsets(O))
    print('encoder gradient: mean %.3g, std %.3g' % (float(genc.mean()), float(genc.std())))
    u = C.unit_of(pts[:count])
    want = C.np_trilinear_scatter(O, u, C.live_of(u), genc, m._offsets_np, m.rows)
    got = g[:m.table_elems].reshape(m.rows, 2, 2)
    assert not got[:, 0].any()                                   # the density table is not trained
    assert float(np.abs(want).sum()) > 0
    _check_per_level(m, got[:, 1:2], want[:, None, :], 'sorted vs fp64 scatter')


@pytest.mark.parametrize('name', C.WALK_CASES)
def test_walk_case(O, dev, model, name):
    pts, count, xyzs, counter = _inputs(name, dev)
    lm = C.launch_model(pts.shape[0], count)
    assert lm['per'] == C.EXPECTED_LAUNCH[name][0]
    perm = _sorted_vs_tracker(model, xyzs, counter, 21)
    _assert_walk(perm, pts, count)
    _vs_fp64(O, model, pts, count, xyzs, counter, perm)


def test_count_in_second_tile_equals_truncated_batch_and_reads_nothing_behind(O, dev, model):
    pts, count, xyzs, counter = _inputs('count_in_second_tile', dev)
    M = pts.shape[0]
    te = model.table_elems
    gs, gr = _upstream(M, dev, 22)
    assert float(gr[count:].abs().min()) > 0 and C.live_of(C.unit_of(pts[count:])).sum() > 30000
    perm = model.sample_order(xyzs, m_dev=counter)
    g_full = _backward(model, xyzs, counter, perm, gs, gr)
    cut = xyzs[:count].contiguous()
    g_cut = _backward(model, cut, None, model.sample_order(cut), gs[:count].contiguous(), gr[:count].contiguous())
    _check_per_level(model, g_full[:te].reshape(model.rows, 2, 2), g_cut[:te].reshape(model.rows, 2, 2), 'count vs truncated')
    # the slots behind the count are never read
    nan_xyzs = xyzs.clone()
    nan_xyzs[count:] = float('nan')
    perm_nan = model.sample_order(nan_xyzs, m_dev=counter)
    assert torch.equal(perm_nan, perm)
    g_nan = _backward(model, nan_xyzs, counter, perm_nan, gs, gr)
    assert np.isfinite(g_nan).all()
    _check_per_level(model, g_nan[:te].reshape(model.rows, 2, 2), g_full[:te].reshape(model.rows, 2, 2), 'NaN behind the count')


def test_two_tiles_bf16_compute_fp32_tables(O, dev):
    m = _model(dev, 'bf16', torch.float32)
    pts, count, xyzs, counter = _inputs('two_tiles', dev)
    perm = _sorted_vs_tracker(m, xyzs, counter, 23)
    _assert_walk(perm, pts, count)


def test_two_tiles_run_to_run(O, dev, model):
    pts, count, xyzs, counter = _inputs('two_tiles', dev)
    gs, gr = _upstream(pts.shape[0], dev, 24)
    perm = model.sample_order(xyzs)
    te = model.table_elems
    g1 = _backward(model, xyzs, None, perm, gs, gr)[:te]
    g2 = _backward(model, xyzs, None, perm, gs, gr)[:te]
    assert float(np.abs(g1).sum()) > 0
    r = rel_l2(g2, g1)
    print('run to run: rel-L2 %.3g' % r)
    assert r <= 2e-6                                             # the same arithmetic; atomics order only
