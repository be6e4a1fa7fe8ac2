"""The large table-scatter cases (table_scatter_cases.py) judged on the reference side alone, so that
test_gpu_table_scatter_walk.py cannot pass vacuously: the launch partition each case is built for, what its walk puts on
the interior tile boundaries, the load of the table rows that the 2e-5 bar rests on, the distance of the fp64 scatter
from the oracle's fp32 encoder backward, the bincount form of the scatter against the np.add.at form, and how far a host
model of three mistakes in the walk (table_scatter_cases.walk_inputs) lands from the right result on these cases."""
import numpy as np
import pytest

import table_scatter_cases as C
from helpers import rel_l2

MIN_BOUNDARIES = 100
MAX_ROW_LOAD = 1500
ORACLE_BAR = 1e-5


@pytest.fixture(scope='module')
def censuses():
    return {name: C.census(C.walk_case(name)[0], None, C.walk_case(name)[1]) for name in C.WALK_CASES}


def test_walk_key_is_the_sort_keys_order():
    """walk_key orders as the 27-bit key of sample_order_ref.py does, and inside the box as the plain 30-bit Morton key"""
    import sample_order_ref as R
    pts, count = C.walk_case('two_tiles')
    mine = C.walk_order(pts, count)
    assert np.array_equal(mine, np.argsort(R.morton_key(pts[:count], (-2.0,) * 3, (4.0,) * 3), kind='stable'))
    q = C.blocks_of(C.unit_of(pts[:count]))
    box = np.flatnonzero(np.all(q >= 512, axis=1))
    assert box.size > 20000
    assert np.array_equal(np.argsort(C.walk_key(q[box]), kind='stable'), np.argsort(C.morton_key(q[box]), kind='stable'))


@pytest.mark.parametrize('name', C.WALK_CASES)
def test_launch_partition(censuses, name):
    pts, count = C.walk_case(name)
    lm = censuses[name]['launch']
    per, full, short, empty, end_lanes, end_tile = C.EXPECTED_LAUNCH[name]
    print(name, pts.shape[0], count, {k: v for k, v in lm.items() if k not in ('begin', 'end')})
    assert lm['nwaves'] == 16384 and lm['per'] == per
    assert lm['full'] + lm['short'] + lm['empty'] == lm['nwaves']
    assert int((lm['end'] - lm['begin']).sum()) == lm['ntiles'] and np.all(lm['begin'][1:] == lm['end'][:-1])
    if name == 'long_blocks':
        assert C.SINGLE_TILE_LIMIT < count <= 2 * C.SINGLE_TILE_LIMIT and abs(count - 270000) < 10000
    else:
        assert (lm['full'], lm['short'], lm['empty'], lm['end_lanes'], lm['end_tile_in_wave']) == (full, short, empty, end_lanes, end_tile)
    if name == 'threshold':
        assert np.array_equal(pts, C.walk_case('two_tiles')[0][:C.SINGLE_TILE_LIMIT]) and count == C.SINGLE_TILE_LIMIT
    if name == 'count_in_second_tile':
        assert pts.shape[0] == C.COUNT_CAPACITY and C.live_of(C.unit_of(pts[count:])).sum() > 30000


@pytest.mark.parametrize('name', ['two_tiles', 'long_blocks', 'three_tiles'])
def test_census_of_interior_boundaries(censuses, name):
    cs = censuses[name]
    print(name, cs['boundaries'], cs['all'], cs['by_step'])
    for k in 'abcde':
        assert cs['all'][k] >= MIN_BOUNDARIES, (name, k, cs['all'])
    if name == 'long_blocks':
        assert cs['all']['inside_long'] >= MIN_BOUNDARIES
    if name == 'three_tiles':
        assert len(cs['by_step']) == 2
        for step in cs['by_step']:
            for k in 'abc':
                assert step[k] >= MIN_BOUNDARIES, (name, k, cs['by_step'])


def test_blocks_cover_the_encoded_range_and_the_faces():
    pts, count = C.walk_case('two_tiles')
    u = C.unit_of(pts)
    live = C.live_of(u)
    q = C.blocks_of(u[live])
    for d in range(3):
        assert np.bincount(q[:, d] // 64, minlength=16).min() > 5000            # every sixteenth of every axis
    s = u[live].astype(np.float64) * 1024.0
    assert ((s == np.floor(s)).any(axis=1)).sum() > 1000                         # u exactly b / 1024
    up = np.nextafter(u[live], np.float32(2.0)).astype(np.float64) * 1024.0
    assert ((np.floor(up) > np.floor(s)).any(axis=1)).sum() > 1000               # the last fp32 u of its block
    sizes = np.bincount(np.unique(C.morton_key(q), return_inverse=True)[1])
    assert sizes.max() <= 5
    ql = C.blocks_of(C.unit_of(C.walk_case('long_blocks')[0]))
    ql = ql[C.live_of(C.unit_of(C.walk_case('long_blocks')[0]))]
    sizes = np.bincount(np.unique(C.morton_key(ql), return_inverse=True)[1])
    assert sizes.min() >= 20 and sizes.max() <= 40


@pytest.mark.parametrize('name', C.WALK_CASES)
def test_row_load(O, name):
    """no table row of any level receives more than 1 500 contributions from the walked samples"""
    pts, count = C.walk_case(name)
    u = C.unit_of(pts[:count])
    load = C.row_load(O, u, C.live_of(u), C.level_offsets(O))
    print(name, 'largest row load per level', load.tolist())
    assert load.max() <= MAX_ROW_LOAD, load


def _seeded_genc(M, seed):
    """[M, 16, 2] with the magnitudes of what the gradients-out kernel hands over in the GPU test (colour table, unit upstream
    gradients, the seeded checkpoint: mean -0.008, standard deviation 0.28 over all entries)"""
    rng = np.random.default_rng(seed)
    return (0.28 * rng.standard_normal((M, 16, 2)) - 0.008).astype(np.float32)


@pytest.mark.parametrize('name', ['two_tiles', 'long_blocks'])
def test_fp64_scatter_within_1e5_of_the_oracles_backward(O, name):
    pts, count = C.walk_case(name)
    u = C.unit_of(pts[:count])
    live = C.live_of(u)
    off = C.level_offsets(O)
    genc = _seeded_genc(count, 31)
    want = C.np_trilinear_scatter(O, u, live, genc, off, int(off[-1]))
    got = O.grid_encode_backward(genc.reshape(count, 32), u, off, int(off[-1]), 2, O.per_level_scale_from_cfg(), 16, 0, True, 0)
    r = [rel_l2(got[off[l]:off[l + 1]], want[off[l]:off[l + 1]]) for l in range(16)]
    print(name, 'oracle fp32 backward vs fp64 scatter, rel-L2 per level:', ' '.join('%.2g' % v for v in r))
    assert max(r) <= ORACLE_BAR, r


def test_bincount_scatter_equals_add_at(O):
    pts = C.SYNTHETIC['x_runs']()
    u = C.unit_of(pts)
    live = C.live_of(u)
    off = C.level_offsets(O)
    genc = _seeded_genc(pts.shape[0], 32)
    a = C.np_trilinear_scatter(O, u, live, genc, off, int(off[-1]))
    b = C.np_trilinear_scatter_add_at(O, u, live, genc, off, int(off[-1]))
    assert float(np.abs(b).sum()) > 0
    for l in range(16):
        assert rel_l2(a[off[l]:off[l + 1]], b[off[l]:off[l + 1]]) <= 1e-12
    assert np.array_equal(a == 0, b == 0)


FAULT_FLOOR = 100 * 2e-5            # a modelled mistake must miss the GPU test's bar by two orders of magnitude, on every level


def _scatter_of_walk(O, name, fault):
    pts, count = C.walk_case(name)
    p, g = C.walk_inputs(pts, _seeded_genc(pts.shape[0], 33), None, count, fault)
    u = C.unit_of(p)
    off = C.level_offsets(O)
    return C.np_trilinear_scatter(O, u, C.live_of(u), g, off, int(off[-1])), off


@pytest.fixture(scope='module')
def right_walks(O):
    return {name: _scatter_of_walk(O, name, None)[0] for name in ('two_tiles', 'three_tiles')}


@pytest.mark.parametrize('name,fault', [('two_tiles', C.WALK_FAULTS[0]), ('two_tiles', C.WALK_FAULTS[1]),
                                        ('three_tiles', C.WALK_FAULTS[0]), ('three_tiles', C.WALK_FAULTS[1]),
                                        ('three_tiles', C.WALK_FAULTS[2])])
def test_a_wrong_walk_is_far_from_the_right_one(O, right_walks, name, fault):
    """what the GPU test compares with is, on every level, at least 100 bars away from what each modelled mistake scatters"""
    got, off = _scatter_of_walk(O, name, fault)
    want = right_walks[name]
    r = [rel_l2(got[off[l]:off[l + 1]], want[off[l]:off[l + 1]]) for l in range(16)]
    print(name, fault, 'rel-L2 per level:', ' '.join('%.2g' % v for v in r))
    assert min(r) >= FAULT_FLOOR, r


def test_walk_model_without_fault_is_the_plain_scatter_and_two_ahead_needs_three_tiles(O, right_walks):
    pts, count = C.walk_case('two_tiles')
    genc = _seeded_genc(pts.shape[0], 33)
    u = C.unit_of(pts[:count])
    off = C.level_offsets(O)
    plain = C.np_trilinear_scatter(O, u, C.live_of(u), genc[:count], off, int(off[-1]))
    assert rel_l2(right_walks['two_tiles'], plain) <= 1e-12
    for name in ('two_tiles', 'long_blocks', 'count_in_second_tile', 'threshold'):
        pts, count = C.walk_case(name)
        genc = _seeded_genc(pts.shape[0], 33)
        a, b = C.walk_inputs(pts, genc, None, count, None), C.walk_inputs(pts, genc, None, count, C.WALK_FAULTS[2])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
