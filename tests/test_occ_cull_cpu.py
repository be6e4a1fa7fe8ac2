"""No GPU: the restatement the GPU tests judge the occupancy-component kernels by (tests/occ_cull_ref.py) checked on its own --
its two forms of the labels against each other, hand-checked small cases, the keep rule and the cull's algebra --, the edge
enumeration and union-find of the kernels run from 16 host threads (tests/occ_cc_host.cpp), and the argument checks of the new
entry points, which answer before anything touches a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import occ_cull_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('nsr_occ_components', 'nsr_occ_component_stats', 'nsr_occ_cull')


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _id(H, c, x, y, z):
    return c * H ** 3 + int(R.morton(x, y, z))


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.cases()))
def test_the_two_restatements_of_the_labels_agree(name):
    C, H, bits = R.cases()[name]
    a, (b, _) = R.labels_union_find(bits, C, H), R.reference(name)
    cells = C * H ** 3
    assert a.dtype == b.dtype == np.int32 and a.shape == (cells,) and np.array_equal(a, b)
    occ = R.occupied(bits, C, H)
    assert np.array_equal(a >= 0, occ) and (a[~occ] == -1).all()
    ids = np.arange(cells)
    assert (a[occ] <= ids[occ]).all() and np.array_equal(a[a[occ]], a[occ])    # a label is a root, and no larger than the cell
    assert (a[occ] // H ** 3 == ids[occ] // H ** 3).all()                      # and a cell of the same cascade


def test_morton_layout():
    assert [int(R.morton(*p)) for p in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (7, 7, 7), (511, 511, 511))] == \
        [0, 1, 2, 4, 8, 511, 2 ** 27 - 1]
    bits = R.from_cells(2, 8, [(0, 1, 0, 0), (1, 0, 0, 1)])
    assert bits[0] == 0x02 and bits[64] == 0x10 and bits.sum() == 0x12         # bit u & 7 of byte u >> 3
    xyz = R.cell_coords(8)
    assert np.array_equal(R.morton(xyz[:, 0], xyz[:, 1], xyz[:, 2]), np.arange(512))


def test_face_contact_joins_along_every_axis_and_across_block_boundaries():
    for name, (C, H, cells) in R.hand_cells().items():
        if not name.startswith('pair_'):
            continue
        labels, stats = R.reference(name)
        u, w = sorted(_id(H, *c) for c in cells)
        assert labels[u] == labels[w] == u and len(R.roots(labels)) == 1, name
        assert stats['n_cells'][u] == 2 and stats['n_cells'][w] == 0, name


def test_edge_corner_wrap_and_cascade_contact_does_not_join():
    for name in ('edge_only', 'corner_only', 'no_wrap', 'two_cascades'):
        C, H, cells = R.hand_cells()[name]
        labels, stats = R.reference(name)
        ids = sorted(_id(H, *c) for c in cells)
        if name == 'two_cascades':                                            # the two cells of cascade 1 are joined; cascade 0's is alone
            a, b, c = _id(8, 0, 3, 4, 5), _id(8, 1, 3, 4, 5), _id(8, 1, 4, 4, 5)
            assert labels[a] == a and labels[b] == labels[c] == min(b, c) and b - a == 512
            continue
        assert [int(labels[u]) for u in ids] == ids, name                      # every cell is its own component
        assert (stats['n_cells'][ids] == 1).all()


def test_L_shape_by_hand():
    labels, stats = R.reference('L_shape')
    cells = R.hand_cells()['L_shape'][2]
    ids = [_id(8, *c) for c in cells]
    r = min(ids[:6])
    assert all(labels[u] == r for u in ids[:6]) and labels[ids[6]] == ids[6]
    assert stats['n_cells'][r] == 6 and stats['lo'][r].tolist() == [1, 2, 3] and stats['hi'][r].tolist() == [4, 4, 3]
    assert stats['n_cells'][ids[6]] == 1 and stats['lo'][ids[6]].tolist() == stats['hi'][ids[6]].tolist() == [6, 6, 6]
    other = ids[1]                                                             # a cell that is no root: 0, H, -1
    assert stats['n_cells'][other] == 0 and stats['lo'][other].tolist() == [8] * 3 and stats['hi'][other].tolist() == [-1] * 3
    # bound 2, H 8, cascade 0: a cell is 0.25 wide; the box is 4 x 3 x 1 cells: diagonal^2 = 0.0625 * 26 = 1.625
    keep = lambda **rule: R.keep_rule(labels, stats, 1, 8, 2.0, **rule)
    assert keep(min_diagonal=1.27)[r] == 1 and keep(min_diagonal=1.28)[r] == 0       # 1.6129 <= 1.625 < 1.6384
    assert keep(min_cells=6)[r] == 1 and keep(min_cells=7)[r] == 0 and keep(min_cells=2)[ids[6]] == 0
    assert keep(min_diagonal=0.43)[ids[6]] == 1 and keep(min_diagonal=0.44)[ids[6]] == 0      # one cell: 0.0625 * 3 = 0.1875
    # cascade 1 of bound 2 has cells twice as wide; with bound 1 both cascades have b = 1
    two, s2 = R.reference('two_cascades')
    b = _id(8, 1, 3, 4, 5)
    assert R.keep_rule(two, s2, 2, 8, 2.0, min_diagonal=1.1)[b] == 1           # (0.5)^2 (4 + 1 + 1) = 1.5 >= 1.21
    assert R.keep_rule(two, s2, 2, 8, 1.0, min_diagonal=1.1)[b] == 0           # (0.25)^2 6 = 0.375


def test_keep_largest_ties_go_to_the_smaller_label_per_cascade():
    labels, stats = R.reference('ties')
    rts = R.roots(labels)
    c0, c1 = rts[rts < 512].tolist(), rts[rts >= 512].tolist()
    assert len(c0) == 4 and len(c1) == 2
    three = [r for r in c0 if stats['n_cells'][r] == 3]
    twos = sorted(r for r in c0 if stats['n_cells'][r] == 2)
    assert len(three) == 1 and len(twos) == 3
    kept = lambda **rule: np.flatnonzero(R.keep_rule(labels, stats, 2, 8, 2.0, **rule)).tolist()
    assert kept(keep_largest=1) == sorted([three[0], min(c1)])                # one per cascade: cascade 1's tie to the smaller label
    assert kept(keep_largest=2) == sorted([three[0], twos[0]] + c1)
    assert kept(keep_largest=3) == sorted([three[0], twos[0], twos[1]] + c1)
    assert kept(keep_largest=100) == sorted(c0 + c1)
    assert kept(min_cells=3, keep_largest=2) == three                          # the selection comes after the thresholds
    assert kept(keep_largest=1, min_cells=4) == []


@pytest.mark.parametrize('name', sorted(R.cases()))
def test_defaults_are_the_identity_and_the_cull_is_idempotent(name):
    C, H, bits = R.cases()[name]
    cells = C * H ** 3
    grid = np.random.default_rng(1).integers(0, 2 ** 32, cells, dtype=np.uint64).astype(np.uint32)
    out = R.cull_floaters(grid, bits, C, H, R.BOUND)
    assert np.array_equal(out['bits'], bits) and np.array_equal(out['grid'], grid) and not out['n_culled'].any()
    for rule in R.RULES:
        one = R.cull_floaters(grid, bits, C, H, R.BOUND, **rule)
        two = R.cull_floaters(one['grid'], one['bits'], C, H, R.BOUND, **rule)
        assert np.array_equal(two['bits'], one['bits']) and np.array_equal(two['grid'], one['grid']) and not two['n_culled'].any(), rule
        gone = R.occupied(bits, C, H) & ~R.occupied(one['bits'], C, H)
        assert np.array_equal(gone.reshape(C, -1).sum(1), one['n_culled'])
        assert (one['grid'][gone] == 0xBF800000).all() and np.array_equal(one['grid'][~gone], grid[~gone])
        assert not (R.occupied(one['bits'], C, H) & ~R.occupied(bits, C, H)).any()
        bits_only = R.cull_floaters(None, bits, C, H, R.BOUND, **rule)
        assert bits_only['grid'] is None and np.array_equal(bits_only['bits'], one['bits'])
    assert not R.occupied(R.cull_floaters(None, bits, C, H, R.BOUND, min_cells=H ** 3 + 1)['bits'], C, H).any()


def test_the_named_cases_are_what_the_issue_asks_for():
    labels, stats = R.reference('random_16x2')
    rts = R.roots(labels)
    for c in range(2):
        mine = rts[rts // 4096 == c]
        assert len(mine) >= 20, (c, len(mine))
        span = stats['hi'][mine] // 2 - stats['lo'][mine] // 2                  # in 2x2x2 blocks
        assert (span >= 1).all(axis=1).any(), c                                # one component over more than one block on every axis
    labels, stats = R.reference('snake_16')
    assert len(R.roots(labels)) == 1 and stats['n_cells'][0] == 16 * 64 + 7 * 8 + 7
    assert stats['lo'][0].tolist() == [0, 0, 0] and stats['hi'][0].tolist() == [15, 14, 14]
    labels, stats = R.reference('full_32x2')
    assert R.roots(labels).tolist() == [0, 32768] and stats['n_cells'][[0, 32768]].tolist() == [32768, 32768]
    labels, _ = R.reference('three_patterns_16x3')
    rts = R.roots(labels)
    assert [int((rts // 4096 == c).sum()) for c in (1, 2)] == [4, 8] and (rts // 4096 == 0).sum() >= 20
    for name in ('empty_8', 'full_8', 'single_cell_8', 'first_and_last_8'):
        assert len(R.roots(R.reference(name)[0])) == {'empty_8': 0, 'full_8': 1, 'single_cell_8': 1, 'first_and_last_8': 2}[name]
    assert R.roots(R.reference('first_and_last_8')[0]).tolist() == [0, 511]


def _n_culled(name, **rule):
    C, H, bits = R.cases()[name]
    labels, stats = R.reference(name)
    return R.cull(None, bits, labels, R.keep_rule(labels, stats, C, H, R.BOUND, **rule), C, H)[2].tolist()


def test_cascades_that_share_a_block_cull_different_counts():
    """H = 8: a cascade is one wave of the cull, a block spans four.  A count that lands in the wrong cascade must show"""
    C, H, bits = R.cases()['eight_cascades_8']
    assert (C, H) == (8, 8) and not bits[:64].any() and (bits[64:128] == 0xFF).all()
    n = _n_culled('eight_cascades_8', keep_largest=1)
    assert len(set(n)) > 1 and len(set(n)) >= 6, n
    assert n[0] == n[1] == 0 and len(set(n[2:])) == 6 and min(n[2:]) > 0, n    # nothing to cull in the empty and the full cascade
    C, H, bits = R.cases()['four_cascades_8']
    assert (C, H) == (4, 8) and bits.size == _kernel_constant('OC_BLOCK')      # one block exactly
    n = _n_culled('four_cascades_8', keep_largest=1)
    assert len(set(n)) == 4 and min(n) > 0, n


def _kernel_constant(name):
    src = open(os.path.join(ROOT, 'nerfstyle_amd', 'csrc', 'occ_components.hip')).read()
    found = re.findall(r'^#define\s+' + name + r'\s+(\d+)u?\b', src, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_roots_per_brick_overflow_the_statistics_table_or_fill_one_slot():
    """a block of the statistics gathers the roots of OC_BLOCK bytes, one brick, in OC_SLOTS slots of LDS; a root past them goes
    to global memory directly, and a root may reach its totals both ways.  The constants are read from the kernel's source: with
    other values these cases may no longer do what this test says they do"""
    slots, block = _kernel_constant('OC_SLOTS'), _kernel_constant('OC_BLOCK')
    assert (slots, block, _kernel_constant('OC_PROBES')) == (128, 256, 4)
    per_brick = {name: R.brick_roots(R.reference(name)[0], block) for name in ('checkerboard_16', 'random_16x2', 'full_32x2')}
    assert per_brick['checkerboard_16'].tolist() == [block * 8 // 2] * 2       # every occupied cell its own root: the most a block can meet
    assert per_brick['checkerboard_16'].max() > slots and per_brick['random_16x2'].max() > slots
    assert (per_brick['full_32x2'] == 1).all() and per_brick['full_32x2'].size == 32
    labels, stats = R.reference('checkerboard_16')
    occ = R.occupied(R.cases()['checkerboard_16'][2], 1, 16)
    assert np.array_equal(R.roots(labels), np.flatnonzero(occ)) and (stats['n_cells'][occ] == 1).all()


# ---- the closed form for large grids ------------------------------------------------------------------------------------------
def test_box_case_equals_both_restatements_at_32():
    C, H = 3, 32
    bits, labels, stats = R.box_reference(H)
    assert labels.dtype == np.int32 and labels.shape == (C * H ** 3,) and bits.shape == (C * H ** 3 // 8,)
    assert np.array_equal(labels, R.labels_propagation(bits, C, H))
    assert np.array_equal(labels, R.labels_union_find(bits, C, H))
    rts = R.roots(labels)
    assert [int((rts // H ** 3 == c).sum()) for c in range(C)] == [H // 4 + (H // 16) * (H // 8), (H // 8) ** 3, 1 + (H // 32) * (H // 16) ** 2]
    r = H ** 3 + int(R.morton(9, 17, 1))                                        # one of the two longer cubes of cascade 1
    assert stats['n_cells'][r] == 36 and stats['lo'][r].tolist() == [9, 17, 1] and stats['hi'][r].tolist() == [11, 19, 4]
    assert stats['n_cells'][0] == 2 * H * H and stats['n_cells'][2 * H ** 3] == H ** 3 // 2


def test_box_case_refuses_boxes_that_touch_or_overlap():
    R.box_case(1, 8, [(0, (0, 0, 0), (2, 2, 2)), (0, (3, 0, 0), (4, 2, 2)), (0, (2, 2, 2), (3, 3, 3))])       # a gap; a corner only
    for other in ((2, 0, 0), (0, 2, 1), (1, 1, 2), (1, 1, 1)):                  # a face along x, y, z; an overlap
        with pytest.raises(AssertionError):
            R.box_case(1, 8, [(0, (0, 0, 0), (2, 2, 2)), (0, other, tuple(v + 2 for v in other))])
    bits, labels = R.box_case(2, 8, [(0, (7, 0, 0), (8, 8, 1)), (1, (0, 0, 0), (1, 8, 1))])                  # cascades never touch
    assert np.array_equal(labels, R.labels_propagation(bits, 2, 8))


@pytest.mark.parametrize('H', (32, 128))
def test_box_layout_meets_the_conditions_of_the_large_gpu_case(H):
    """on the reference alone: what tests/test_gpu_occ_cull_edges.py::test_past_the_grid_cap relies on"""
    C = 3
    bits, labels, stats = R.box_reference(H)
    assert len(R.roots(labels)) == len(R.boxes_for(H)) <= 10000
    if H == 128:
        assert bits.size > 2048 * _kernel_constant('OC_BLOCK')                  # the grids are capped at 2048 blocks: a second trip
        assert bits.size - 2048 * 256 == bits.size // C                         # ... which is cascade 2, from blocks that began in cascade 0
    per_cascade = R.occupied(bits, C, H).reshape(C, -1).sum(1)
    for rule in R.BOX_RULES:
        keep = R.keep_rule(labels, stats, C, H, R.BOUND, **rule)
        _, _, n = R.cull(None, bits, labels, keep, C, H)
        assert ((n > 0) & (n < per_cascade)).all(), (rule, n)                   # every cascade culls something and keeps something
        assert len(set(n.tolist())) == C, (rule, n)
    keep = R.keep_rule(labels, stats, C, H, R.BOUND, min_cells=H ** 3 + 1)
    assert not keep.any() and np.array_equal(R.cull(None, bits, labels, keep, C, H)[2], per_cascade)


# ---- labels that are not this grid's ------------------------------------------------------------------------------------------
def test_foreign_labels_count_as_unoccupied_and_are_never_culled():
    C, H, cells_list = R.hand_cells()['L_shape']
    bits = R.cases()['L_shape'][2]
    labels, stats = R.reference('L_shape')
    cells = C * H ** 3
    ids = [_id(H, *c) for c in cells_list]
    r = min(ids[:6])
    for foreign in (cells, cells + 7, 0x7fffffff, -2):
        lab = np.array(labels)
        lab[ids[3]] = foreign                                                  # (4, 2, 3): the corner of the L
        lab[ids[6]] = foreign                                                  # the single cell, a root
        assert R.own_labels(lab, C, H).sum() == 5
        s = R.component_stats(lab, C, H)
        assert s['n_cells'][r] == 5 and s['lo'][r].tolist() == [1, 2, 3] and s['hi'][r].tolist() == [4, 4, 3]
        assert s['n_cells'].sum() == 5 and s['n_cells'][ids[6]] == 0 and s['lo'][ids[6]].tolist() == [H] * 3
        grid = np.arange(cells, dtype=np.uint32)
        out, out_bits, n = R.cull(grid, bits, lab, np.zeros(cells, np.uint8), C, H)          # keep nothing
        left = np.flatnonzero(R.occupied(out_bits, C, H)).tolist()
        assert left == sorted([ids[3], ids[6]]) and n.tolist() == [5]
        assert (out[[i for i in ids if i not in left]] == 0xBF800000).all() and np.array_equal(out[left], grid[left])
    lab = np.array(labels)
    lab[ids[1]] = -1                                                           # -1 on an occupied cell is no label either
    assert R.cull(None, bits, lab, np.zeros(cells, np.uint8), C, H)[2].tolist() == [6]
    # with labels of its own grid the filter changes nothing
    assert np.array_equal(R.own_labels(labels, C, H), labels >= 0)


# ---- the kernels' edge enumeration and union-find from many host threads ------------------------------------------------------
def test_labelling_core_from_sixteen_host_threads(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'occ_cc_host')
    subprocess.run([cxx, '-O2', '-std=c++17', '-pthread', os.path.join(ROOT, 'tests', 'occ_cc_host.cpp'), '-o', exe], check=True)
    C, H = 3, 8
    for name, bits in R.host_cases().items():
        path = str(tmp_path / (name + '.bin'))
        with open(path, 'wb') as f:
            f.write(np.asarray([C, H], np.uint32).tobytes() + bits.tobytes())
        want = R.labels_propagation(bits, C, H)
        assert np.array_equal(want, R.labels_union_find(bits, C, H)), name
        for _ in range(3):                                                     # the interleaving differs, the labels do not
            r = subprocess.run([exe, path, '16'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            assert r.returncode == 0, r.stdout
            got = np.asarray([int(t) for t in r.stdout.split()], np.int64)
            assert got.shape == want.shape and np.array_equal(got, want), name


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(built):
    from nerfstyle_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', hdr) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().nsr_abi_version() == _lib.ABI_VERSION == 6               # additive: the version stays


def test_invalid_arguments_answer_before_a_device_is_touched(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    INVALID = -1
    a = 0x10000                                                     # aligned, never dereferenced: the checks come first
    shapes = ((1, 24), (0, 8), (9, 8), (1, 4), (1, 1024), (2, 0))

    def comp(bits=a, C=1, H=8, labels=a):
        return L.nsr_occ_components(bits, C, H, labels, None)
    assert all(comp(C=C, H=H) == INVALID for C, H in shapes)
    assert comp(bits=None) == INVALID and comp(labels=None) == INVALID
    assert comp(labels=a + 4) == INVALID and comp(labels=a + 8) == INVALID and comp(labels=a + 1) == INVALID

    def stats(labels=a, C=1, H=8, n=a, lo=a, hi=a):
        return L.nsr_occ_component_stats(labels, C, H, n, lo, hi, None)
    assert all(stats(C=C, H=H) == INVALID for C, H in shapes)
    for k in ('labels', 'n', 'lo', 'hi'):
        assert stats(**{k: None}) == INVALID and stats(**{k: a + 2}) == INVALID, k
    assert stats(labels=a + 8) == INVALID

    def cull(grid=a, bits=a, labels=a, keep=a, C=1, H=8, n=a):
        return L.nsr_occ_cull(grid, bits, labels, keep, C, H, n, None)
    assert all(cull(C=C, H=H) == INVALID for C, H in shapes)
    for k in ('bits', 'labels', 'keep'):
        assert cull(**{k: None}) == INVALID, k
    for k, off in (('grid', 4), ('grid', 8), ('labels', 4), ('n', 2)):
        assert cull(**{k: a + off}) == INVALID, (k, off)


def test_python_layer_refuses_cpu_tensors_and_bad_input(built):
    from nerfstyle_amd import raymarching as rm
    C, H, cells = 1, 8, 512
    bits = torch.zeros(cells // 8, dtype=torch.uint8)
    labels = torch.full((cells,), -1, dtype=torch.int32)
    n, lo, hi = torch.zeros(cells, dtype=torch.int32), torch.zeros(cells, 3, dtype=torch.int32), torch.zeros(cells, 3, dtype=torch.int32)
    keep = torch.zeros(cells, dtype=torch.uint8)
    grid = torch.zeros(C, cells)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rm.occupancy_components(bits, C, H)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rm.occupancy_component_stats(labels, C, H)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rm.keep_occupancy_components(n, lo, hi, C, H, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rm.cull_occupancy(None, bits, labels, keep, C, H)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rm.cull_occupancy(grid, bits, labels, keep, C, H)
    for bad in (bits.to(torch.int32), bits[:-1], bits.numpy()):
        with pytest.raises(ValueError, match='bitfield must be a uint8'):
            rm.occupancy_components(bad, C, H)
        with pytest.raises(ValueError, match='bitfield must be a uint8'):
            rm.cull_occupancy(None, bad, labels, keep, C, H)
    for bad in (labels.to(torch.int64), labels[:-1]):
        with pytest.raises(ValueError, match='labels must be a int32'):
            rm.occupancy_component_stats(bad, C, H)
    with pytest.raises(ValueError, match='density_grid must be a float32'):
        rm.cull_occupancy(grid.double(), bits, labels, keep, C, H)
    with pytest.raises(ValueError, match='keep must be a uint8'):
        rm.cull_occupancy(None, bits, labels, keep.bool(), C, H)
    for C_, H_ in ((0, 8), (9, 8), (1, 24), (1, 4), (1, 1024)):
        with pytest.raises(ValueError, match='cascade in 1..8'):
            rm.occupancy_components(bits, C_, H_)
    for rule in (dict(min_cells=-1), dict(min_cells=1.5), dict(min_cells=2 ** 31), dict(min_diagonal=-0.5),
                 dict(min_diagonal=float('nan')), dict(keep_largest=0), dict(keep_largest=2.5)):
        with pytest.raises(ValueError, match='min_cells must be an integer|min_diagonal must be >= 0|keep_largest must be None'):
            rm.keep_occupancy_components(n, lo, hi, C, H, 1.0, **rule)
        with pytest.raises(ValueError, match='cull_floaters: '):
            rm.check_cull_rule(rule.get('min_cells', 0), rule.get('min_diagonal', 0.0), rule.get('keep_largest'), 'cull_floaters')


def test_renderer_has_the_call():
    from nerfstyle_amd.renderer import Renderer
    import inspect
    sig = inspect.signature(Renderer.cull_floaters)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ('min_cells', 0), ('min_diagonal', 0.0), ('keep_largest', None), ('permanent', True), ('return_labels', False)]
