"""GPU: the occupancy-grid floater cull (nsr_occ_components / nsr_occ_component_stats / nsr_occ_cull, the keep rule of
nerfstyle_amd/raymarching.py, Renderer.cull_floaters) against the CPU restatement of the definition (tests/occ_cull_ref.py).
There is no tolerance in this file: labels, statistics, keep, the bitfield, the grid's words and the counts are integers or bit
patterns and must be EQUAL.  Every case runs twice and must give the same bits both times."""
import numpy as np
import pytest
import torch

import occ_cull_ref as R

pytestmark = pytest.mark.gpu

# -1, +0, 0.5, 3.25, the smallest denormal, -0.0, a quiet NaN, a negative NaN with a payload
PATTERN = np.array([0xBF800000, 0x00000000, 0x3F000000, 0x40500000, 0x00000001, 0x80000000, 0x7FC00000, 0xFFC01234], np.uint32)


def _grid_words(cells, seed=2):
    return PATTERN[np.random.default_rng(seed).integers(0, PATTERN.size, cells)]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                 # a copy: the cases' arrays are read-only


def _labels_and_stats(dev, name):
    from nerfstyle_amd import raymarching as rm
    C, H, bits = R.cases()[name]
    b = _dev(bits, dev)
    labels = rm.occupancy_components(b, C, H)
    n, lo, hi = rm.occupancy_component_stats(labels, C, H)
    assert torch.equal(b.cpu(), torch.from_numpy(np.array(bits)))                          # the input is only read
    return labels, n, lo, hi


@pytest.mark.parametrize('name', sorted(R.cases()))
def test_labels_and_statistics_equal_the_restatement(dev, name):
    C, H, bits = R.cases()[name]
    want, stats = R.reference(name)
    cells = C * H ** 3
    runs = [_labels_and_stats(dev, name) for _ in range(2)]
    for labels, n, lo, hi in runs:
        assert labels.dtype == n.dtype == lo.dtype == hi.dtype == torch.int32
        assert labels.shape == n.shape == (cells,) and lo.shape == hi.shape == (cells, 3)
        assert np.array_equal(labels.cpu().numpy(), want)
        assert np.array_equal(n.cpu().numpy().view(np.uint32), stats['n_cells'])
        assert np.array_equal(lo.cpu().numpy(), stats['lo']) and np.array_equal(hi.cpu().numpy(), stats['hi'])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', sorted(R.cases()))
def test_keep_and_cull_equal_the_restatement(dev, name):
    from nerfstyle_amd import raymarching as rm
    C, H, bits = R.cases()[name]
    cells = C * H ** 3
    want_labels, want_stats = R.reference(name)
    labels, n, lo, hi = _labels_and_stats(dev, name)
    grid = _grid_words(cells)
    for rule in R.RULES + (dict(min_cells=H ** 3 + 1),):
        want_keep = R.keep_rule(want_labels, want_stats, C, H, R.BOUND, **rule)
        want_grid, want_bits, want_n = R.cull(grid, bits, want_labels, want_keep, C, H)
        keep = rm.keep_occupancy_components(n, lo, hi, C, H, R.BOUND, **rule)
        assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), want_keep), rule
        for permanent in (True, True, False):                                  # twice the same bits; then the bits alone
            g = _dev(grid.view(np.float32).reshape(C, H ** 3), dev)
            b = _dev(bits, dev)
            n_culled = rm.cull_occupancy(g if permanent else None, b, labels, keep, C, H)
            assert n_culled.dtype == torch.int32 and np.array_equal(n_culled.cpu().numpy().view(np.uint32), want_n), rule
            assert np.array_equal(b.cpu().numpy(), want_bits), rule
            got = g.cpu().numpy().view(np.uint32).reshape(-1)
            assert np.array_equal(got, want_grid if permanent else grid), rule  # NaN, -0.0 and -1 keep their bits; culled: 0xBF800000
        # a second cull of the result, from fresh labels, closes nothing
        again = rm.cull_occupancy(g, b, rm.occupancy_components(b, C, H), keep, C, H)
        assert not again.any() and np.array_equal(b.cpu().numpy(), want_bits), rule
    if R.occupied(bits, C, H).any():
        assert (want_grid[R.occupied(bits, C, H)] == 0xBF800000).all() and not want_bits.any()       # the last rule keeps nothing


def test_renderer_cull_floaters(dev):
    """on the small renderer: one component per cascade is left; the marks survive update_state; a cull that keeps nothing
    renders the background; a second cull closes nothing"""
    from helpers import render_setup
    from nerfstyle_amd import raymarching as rm
    from nerfstyle_amd.common import Box2D
    r, ref, poses, intr, bits = render_setup(dev)
    C, H = r.cascade, r.cfg.grid_size
    assert (C, H) == (2, 128)
    grid_before, bits_before = r.density_grid.clone(), r.density_bitfield.clone()
    occ_before = torch.from_numpy(R.occupied(bits_before.cpu().numpy(), C, H)).to(dev)
    labels_before = rm.occupancy_components(bits_before, C, H)
    n_before = rm.occupancy_component_stats(labels_before, C, H)[0].view(C, -1)
    roots_before = (labels_before == torch.arange(C * H ** 3, dtype=torch.int32, device=dev)).view(C, -1).sum(1)
    assert (roots_before > 1).all()                                            # there is something to cull
    for rule in (dict(min_cells=-1), dict(min_cells=1.5), dict(min_diagonal=-0.5), dict(min_diagonal=float('nan')),
                 dict(keep_largest=0), dict(keep_largest=2.5)):
        with pytest.raises(ValueError, match='cull_floaters: '):
            r.cull_floaters(**rule)

    n_culled, labels = r.cull_floaters(keep_largest=1, return_labels=True)
    assert torch.equal(labels, labels_before) and n_culled.dtype == torch.int32 and n_culled.shape == (C,)
    after = rm.occupancy_components(r.density_bitfield, C, H)
    roots_after = (after == torch.arange(C * H ** 3, dtype=torch.int32, device=dev)).view(C, -1).sum(1)
    assert roots_after.tolist() == [1, 1]
    occ_after = torch.from_numpy(R.occupied(r.density_bitfield.cpu().numpy(), C, H)).to(dev)
    assert not (occ_after & ~occ_before).any()
    assert torch.equal(occ_after.view(C, -1).sum(1), n_before.max(dim=1).values)          # what is left is the largest component
    culled = occ_before & ~occ_after
    assert torch.equal(culled.view(C, -1).sum(1).to(torch.int32), n_culled) and (n_culled > 0).all()
    g = r.density_grid.view(-1)
    assert (g[culled] == -1.0).all() and torch.equal(g[~culled].view(torch.int32), grid_before.view(-1)[~culled].view(torch.int32))
    assert not r.cull_floaters(keep_largest=1).any()                           # a second cull closes nothing

    r.update_state()
    g = r.density_grid.view(-1)
    occ_now = torch.from_numpy(R.occupied(r.density_bitfield.cpu().numpy(), C, H)).to(dev)
    assert (g[culled] == -1.0).all() and not (occ_now & culled).any()

    # bits only: the grid is untouched
    r.density_grid, r.density_bitfield = grid_before.clone(), bits_before.clone()
    n_bits_only = r.cull_floaters(keep_largest=1, permanent=False)
    assert torch.equal(n_bits_only, n_culled) and torch.equal(r.density_grid.view(torch.int32), grid_before.view(torch.int32))
    assert torch.equal(torch.from_numpy(R.occupied(r.density_bitfield.cpu().numpy(), C, H)).to(dev), occ_after)

    # a rule that keeps nothing: every ray sees the white background
    n_all = r.cull_floaters(min_cells=H ** 3 + 1)
    assert torch.equal(n_all.to(torch.int64), occ_after.view(C, -1).sum(1)) and not r.density_bitfield.any()
    out = r.render(torch.tensor(poses[5], device=dev), None, patch=Box2D(100, 60, 64, 48), training=False)
    assert out['rgb_map'].shape == (64 * 48, 3) and (out['rgb_map'] == 1.0).all()
    assert not r.cull_floaters(min_cells=H ** 3 + 1).any()

