"""GPU: the occupancy-grid floater cull (csrc/occ_components.hip) where tests/test_gpu_occ_cull.py does not reach: past the one
grid of 2048 blocks that every launch is capped at (a second trip of the grid-stride loops, which lands in another cascade than
the first), with labels that are not this grid's, with guard bands around every output and inside a captured graph.  The cases
at which one block holds several cascades (C >= 4 at H = 8) and at which a block meets more roots than its table has slots run
through the parametrised tests of tests/test_gpu_occ_cull.py (occ_cull_ref.cases()); tests/test_occ_cull_cpu.py asserts that
they do so.

As there, nothing here has a tolerance: labels, statistics, keep, the bitfield, the grid's words and the counts are integers or
bit patterns and must be EQUAL to the restatement (tests/occ_cull_ref.py), and equal again on a second run."""
import numpy as np
import pytest
import torch

import occ_cull_ref as R
from test_gpu_occ_cull import _dev, _grid_words       # the grid's words are drawn from that file's PATTERN

pytestmark = pytest.mark.gpu

INVALID = -1                                     # NSR_ERR_INVALID_ARG
SENTINEL = 0x5A5A5A5A


def _np(t):
    return t.cpu().numpy()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- past one grid of blocks ------------------------------------------------------------------------------------------------
def test_past_the_grid_cap(dev):
    """C = 3, H = 128: 786 432 bitfield bytes, 3072 blocks' worth for a grid capped at 2048.  Blocks 0..1023 take a second trip,
    which is cascade 2 where their first was cascade 0: the statistics' table lives on across the two, and the cull's count of
    the second trip belongs to another cascade than that of the first (the three counts differ under every rule)."""
    from nerfstyle_amd import raymarching as rm
    C, H = 3, 128
    cells = C * H ** 3
    bits, want_labels, want_stats = R.box_reference(H)
    assert bits.size == 786432 > 2048 * 256
    b0 = _dev(bits, dev)
    runs = []
    for _ in range(2):
        labels = rm.occupancy_components(b0, C, H)
        runs.append((labels,) + tuple(rm.occupancy_component_stats(labels, C, H)))
    assert np.array_equal(_np(b0), bits)                                       # the input is only read
    labels, n, lo, hi = runs[0]
    assert np.array_equal(_np(labels), want_labels)
    assert np.array_equal(_u32(n), want_stats['n_cells'])
    assert np.array_equal(_np(lo), want_stats['lo']) and np.array_equal(_np(hi), want_stats['hi'])
    for a, b in zip(*runs):
        assert torch.equal(a, b)

    grid = _grid_words(cells)
    occ = R.occupied(bits, C, H)
    for rule in R.BOX_RULES + (dict(min_cells=H ** 3 + 1),):
        want_keep = R.keep_rule(want_labels, want_stats, C, H, R.BOUND, **rule)
        want_grid, want_bits, want_n = R.cull(grid, bits, want_labels, want_keep, C, H)
        keep = rm.keep_occupancy_components(n, lo, hi, C, H, R.BOUND, **rule)
        assert np.array_equal(_np(keep), want_keep), rule
        for permanent in (True, True, False):                                  # twice the same bits; then the bits alone
            g = _dev(grid.view(np.float32).reshape(C, H ** 3), dev)
            b = _dev(bits, dev)
            n_culled = rm.cull_occupancy(g if permanent else None, b, labels, keep, C, H)
            print(rule, 'permanent' if permanent else 'bits only', 'n_culled', _u32(n_culled).tolist(), 'want', want_n.tolist())
            assert np.array_equal(_u32(n_culled), want_n), rule
            assert np.array_equal(_np(b), want_bits), rule
            assert np.array_equal(_u32(g).reshape(-1), want_grid if permanent else grid), rule
        again = rm.cull_occupancy(g, b, rm.occupancy_components(b, C, H), keep, C, H)       # from fresh labels: closes nothing
        assert not again.any() and np.array_equal(_np(b), want_bits), rule
    assert (want_grid[occ] == 0xBF800000).all() and not want_bits.any()        # the last rule keeps nothing


# ---- labels that are not this grid's ----------------------------------------------------------------------------------------
def test_foreign_labels(dev):
    """one occupied cell in twenty carries a label outside 0 .. cells - 1.  The statistics count it as unoccupied; the cull
    leaves it alone and does not read keep[] through it: keep has exactly `cells` entries between two bands of zeros, so a read
    at keep[cells] or keep[cells + 7] would find "not kept" and close the cell."""
    from nerfstyle_amd import raymarching as rm
    name = 'random_16x2'
    C, H, bits = R.cases()[name]
    cells = C * H ** 3
    rng = np.random.default_rng(17)
    lab = np.array(R.reference(name)[0])
    occ = np.flatnonzero(lab >= 0)
    chosen = rng.choice(occ, occ.size // 20, replace=False)
    foreign = np.array([cells, cells + 7, 0x7fffffff, -2], np.int64)[np.arange(chosen.size) % 4]
    lab[chosen] = foreign
    assert lab.dtype == np.int32 and np.array_equal(lab[chosen].astype(np.int64), foreign) and not R.own_labels(lab, C, H)[chosen].any()
    assert (R.reference(name)[0][chosen] == chosen).any()                      # there are roots among them
    want_stats = R.component_stats(lab, C, H)
    keep_np = (rng.random(cells) < 0.5).astype(np.uint8)                       # the kernel's side of the cull needs no rule
    grid = _grid_words(cells, seed=5)
    want_grid, want_bits, want_n = R.cull(grid, bits, lab, keep_np, C, H)
    assert R.occupied(want_bits, C, H)[chosen].all() and (want_n > 0).all()    # the reference closes none of them
    assert (want_grid[chosen] == grid[chosen]).all()

    labels = _dev(lab, dev)
    band = 256
    buf = torch.zeros(cells + 2 * band, dtype=torch.uint8, device=dev)
    keep = buf[band:band + cells]
    keep.copy_(_dev(keep_np, dev))
    for _ in range(2):
        n, lo, hi = rm.occupancy_component_stats(labels, C, H)
        assert np.array_equal(_u32(n), want_stats['n_cells'])
        assert np.array_equal(_np(lo), want_stats['lo']) and np.array_equal(_np(hi), want_stats['hi'])
        for permanent in (True, False):
            g = _dev(grid.view(np.float32).reshape(C, H ** 3), dev)
            b = _dev(bits, dev)
            n_culled = rm.cull_occupancy(g if permanent else None, b, labels, keep, C, H)
            assert np.array_equal(_u32(n_culled), want_n)
            assert np.array_equal(_np(b), want_bits)
            assert np.array_equal(_u32(g).reshape(-1), want_grid if permanent else grid)
    assert np.array_equal(_np(labels), lab) and np.array_equal(_np(keep), keep_np) and not buf[:band].any() and not buf[-band:].any()


# ---- the three entries themselves, with guard bands ---------------------------------------------------------------------------
class _Guarded:
    """a slice of a larger buffer filled with a sentinel: `lead` elements before it (which sets its alignment) and 64 after"""

    def __init__(self, dev, n, dtype, lead, sentinel=SENTINEL):
        self.buf = torch.full((lead + n + 64,), sentinel, dtype=dtype, device=dev)
        self.t, self.lead, self.n, self.sentinel = self.buf[lead:lead + n], lead, n, sentinel

    def ptr(self):
        return self.t.data_ptr()

    def bands_intact(self):
        return bool((self.buf[:self.lead] == self.sentinel).all()) and bool((self.buf[self.lead + self.n:] == self.sentinel).all())

    def untouched(self):
        return bool((self.buf == self.sentinel).all())


@pytest.mark.parametrize('name', ('eight_cascades_8', 'three_patterns_16x3'))
def test_outputs_stay_inside_their_extents(dev, name):
    """labels and the grid sit 16 bytes into their buffers, the alignment the ABI asks for and no more; n_cells, lo, hi and
    n_culled at 4, 4, 12 and 4 bytes, which is all it asks of them"""
    from nerfstyle_amd import _lib as L
    C, H, bits = R.cases()[name]
    cells = C * H ** 3
    want_labels, want_stats = R.reference(name)
    want_keep = R.keep_rule(want_labels, want_stats, C, H, R.BOUND, keep_largest=1)
    grid = _grid_words(cells, seed=9)
    want_grid, want_bits, want_n = R.cull(grid, bits, want_labels, want_keep, C, H)
    assert want_n.any()
    lib, s = L.lib(), L.stream()

    labels = _Guarded(dev, cells, torch.int32, 4)
    n_cells, lo, hi = _Guarded(dev, cells, torch.int32, 1), _Guarded(dev, cells * 3, torch.int32, 1), _Guarded(dev, cells * 3, torch.int32, 3)
    n_culled = _Guarded(dev, C, torch.int32, 1)
    outs = (labels, n_cells, lo, hi, n_culled)
    assert labels.ptr() % 32 == 16 and n_cells.ptr() % 16 == 4 and lo.ptr() % 16 == 4 and hi.ptr() % 16 == 12 and n_culled.ptr() % 16 == 4
    b0 = _dev(bits, dev)
    keep = _dev(want_keep, dev)

    # refused, and nothing is written: labels 4 bytes off, C = 9, H = 4, H = 24
    b, g = _Guarded(dev, cells // 8, torch.uint8, 3, 0xA5), _Guarded(dev, cells, torch.int32, 4)
    for kw in (dict(off=4), dict(C=9), dict(H=4), dict(H=24)):
        c, h, off = kw.get('C', C), kw.get('H', H), kw.get('off', 0)
        assert lib.nsr_occ_components(b.ptr(), c, h, labels.ptr() + off, s) == INVALID, kw
        assert lib.nsr_occ_component_stats(labels.ptr() + off, c, h, n_cells.ptr(), lo.ptr(), hi.ptr(), s) == INVALID, kw
        assert lib.nsr_occ_cull(g.ptr(), b.ptr(), labels.ptr() + off, keep.data_ptr(), c, h, n_culled.ptr(), s) == INVALID, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs + (b, g))

    for _ in range(2):
        L.check(lib.nsr_occ_components(b0.data_ptr(), C, H, labels.ptr(), s), 'occ_components')
        L.check(lib.nsr_occ_component_stats(labels.ptr(), C, H, n_cells.ptr(), lo.ptr(), hi.ptr(), s), 'occ_component_stats')
        b.t.copy_(b0)
        g.t.copy_(_dev(grid.view(np.int32), dev))
        L.check(lib.nsr_occ_cull(g.ptr(), b.ptr(), labels.ptr(), keep.data_ptr(), C, H, n_culled.ptr(), s), 'occ_cull')
        torch.cuda.synchronize()
        assert all(o.bands_intact() for o in outs + (b, g))
        assert np.array_equal(_np(labels.t), want_labels) and np.array_equal(_u32(n_cells.t), want_stats['n_cells'])
        assert np.array_equal(_np(lo.t).reshape(-1, 3), want_stats['lo']) and np.array_equal(_np(hi.t).reshape(-1, 3), want_stats['hi'])
        assert np.array_equal(_u32(n_culled.t), want_n)
        assert np.array_equal(_np(b.t), want_bits) and np.array_equal(_u32(g.t), want_grid)
    assert np.array_equal(_np(b0), bits) and np.array_equal(_np(keep), want_keep)

    # without counts: the same bitfield and grid, and the counts' buffer is not written
    b2, g2 = _Guarded(dev, cells // 8, torch.uint8, 3, 0xA5), _Guarded(dev, cells, torch.int32, 4)
    b2.t.copy_(b0)
    g2.t.copy_(_dev(grid.view(np.int32), dev))
    n_culled.buf.fill_(SENTINEL)
    L.check(lib.nsr_occ_cull(g2.ptr(), b2.ptr(), labels.ptr(), keep.data_ptr(), C, H, None, s), 'occ_cull')
    torch.cuda.synchronize()
    assert torch.equal(b2.buf, b.buf) and torch.equal(g2.buf, g.buf) and n_culled.untouched()
    # bits only, with counts
    b2.t.copy_(b0)
    L.check(lib.nsr_occ_cull(None, b2.ptr(), labels.ptr(), keep.data_ptr(), C, H, n_culled.ptr(), s), 'occ_cull')
    torch.cuda.synchronize()
    assert torch.equal(b2.buf, b.buf) and np.array_equal(_u32(n_culled.t), want_n) and n_culled.bands_intact()


# ---- capture ------------------------------------------------------------------------------------------------------------------
def _padded(name, C):
    """the case in a grid of C cascades of its own H, the further ones empty -> (bits, labels, stats) of the restatement"""
    c, H, bits = R.cases()[name]
    labels, stats = R.reference(name)
    extra = (C - c) * H ** 3
    return (np.concatenate([bits, np.zeros(extra // 8, np.uint8)]), np.concatenate([labels, np.full(extra, -1, np.int32)]),
            dict(n_cells=np.concatenate([stats['n_cells'], np.zeros(extra, np.uint32)]),
                 lo=np.concatenate([stats['lo'], np.full((extra, 3), H, np.int32)]),
                 hi=np.concatenate([stats['hi'], np.full((extra, 3), -1, np.int32)])))


def test_captured_chain_replays_with_new_bits(dev):
    """components -> statistics -> cull on static buffers in one graph, a linear chain; between replays the bitfield, the grid
    and keep are refilled in place"""
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import raymarching as rm
    C, H = 3, 16
    cells = C * H ** 3
    bits_t = torch.zeros(cells // 8, dtype=torch.uint8, device=dev)
    grid_t = torch.zeros(C, H ** 3, device=dev)
    keep_t = torch.zeros(cells, dtype=torch.uint8, device=dev)
    labels_t = torch.empty(cells, dtype=torch.int32, device=dev)
    n_t, lo_t, hi_t = (torch.empty(shape, dtype=torch.int32, device=dev) for shape in ((cells,), (cells, 3), (cells, 3)))
    n_culled_t = torch.empty(C, dtype=torch.int32, device=dev)
    outs = (labels_t, n_t, lo_t, hi_t, n_culled_t)

    def body():
        lib, s = L.lib(), L.stream()
        L.check(lib.nsr_occ_components(L.p(bits_t), C, H, L.p(labels_t), s), 'occ_components')
        L.check(lib.nsr_occ_component_stats(L.p(labels_t), C, H, L.p(n_t), L.p(lo_t), L.p(hi_t), s), 'occ_component_stats')
        L.check(lib.nsr_occ_cull(L.p(grid_t), L.p(bits_t), L.p(labels_t), L.p(keep_t), C, H, L.p(n_culled_t), s), 'occ_cull')

    def fill(bits, grid, keep):
        bits_t.copy_(_dev(bits, dev))
        grid_t.copy_(_dev(grid.view(np.float32).reshape(C, H ** 3), dev))
        keep_t.copy_(_dev(keep, dev))
        for o in outs:
            o.fill_(SENTINEL)                                                  # whatever an earlier run left is gone

    inputs = []
    for i, (name, rule) in enumerate((('random_16x2', dict(min_cells=4)), ('three_patterns_16x3', dict(keep_largest=1)))):
        bits, labels, stats = _padded(name, C)
        inputs.append((name, bits, labels, stats, _grid_words(cells, seed=20 + i), R.keep_rule(labels, stats, C, H, R.BOUND, **rule)))

    fill(*[inputs[1][k] for k in (1, 4, 5)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()

    for name, bits, labels, stats, grid, keep in inputs:
        want_grid, want_bits, want_n = R.cull(grid, bits, labels, keep, C, H)
        assert want_n.any() and R.occupied(want_bits, C, H).any(), name
        fill(bits, grid, keep)
        graph.replay()
        torch.cuda.synchronize()
        # eager, on tensors of its own
        b, g = _dev(bits, dev), _dev(grid.view(np.float32).reshape(C, H ** 3), dev)
        e_labels = rm.occupancy_components(b, C, H)
        e_n, e_lo, e_hi = rm.occupancy_component_stats(e_labels, C, H)
        e_culled = rm.cull_occupancy(g, b, e_labels, _dev(keep, dev), C, H)
        for got, eager in zip(outs + (bits_t, grid_t.view(torch.int32)), (e_labels, e_n, e_lo, e_hi, e_culled, b, g.view(torch.int32))):
            assert torch.equal(got, eager), name
        assert np.array_equal(_np(labels_t), labels) and np.array_equal(_u32(n_t), stats['n_cells']), name
        assert np.array_equal(_np(lo_t), stats['lo']) and np.array_equal(_np(hi_t), stats['hi']), name
        assert np.array_equal(_u32(n_culled_t), want_n) and np.array_equal(_np(bits_t), want_bits), name
        assert np.array_equal(_u32(grid_t).reshape(-1), want_grid), name
