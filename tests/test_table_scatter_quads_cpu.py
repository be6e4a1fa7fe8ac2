"""Reference-side checks of table_scatter_quad_cases.py: the cases of test_gpu_table_scatter_quads.py put in front of the
kernel what they are meant to (no GPU)."""
import numpy as np
import pytest

import table_scatter_cases as C
import table_scatter_quad_cases as Q


@pytest.fixture(scope='module')
def O():
    from oracle import oracle
    oracle.build()
    return oracle


def test_counts_are_one_block_and_one_or_more_quads():
    for n in Q.COUNTS:
        pts = Q.one_block(n + 7)
        cen = Q.tile_census(pts, n)
        assert len(cen) == -(-n // 16) and all(not d and not c for d, c in cen)
        assert C.live_of(C.unit_of(pts)).all()                       # behind the count: live samples
        assert C.launch_model(n + 7, n)['per'] == 1
    assert {n % 4 for n in Q.COUNTS} == {0, 1, 2, 3} and {(n - 1) // 4 for n in Q.COUNTS if n <= 16} == {0, 1, 2, 3}


@pytest.mark.parametrize('form', Q.FORMS)
def test_block_change_cases(O, form):
    pts = Q.block_change(form)
    assert pts.shape[0] == 256
    cen = Q.tile_census(pts)
    assert [c for _, c in cen] == [[k] if k else [] for k in range(16)] and not any(d for d, _ in cen)
    q = C.blocks_of(C.unit_of(pts))
    for k in range(1, 16):
        a, b = q[16 * k + k - 1], q[16 * k + k]
        moved = Q.levels_that_move(O, a, b)
        if form == 'plus_x':
            assert a[0] % 2 == 0 and tuple(b - a) == (1, 0, 0)
        elif form == 'far':
            assert moved == list(range(16))
        else:
            # the finest level moves, the coarsest and at least three more do not
            assert tuple(b - a) == (0, 1, 0) and 15 in moved and 0 not in moved and len(moved) <= 12, moved


def test_two_changes_fall_inside_one_quad():
    pts, combos = Q.two_changes()
    cen = Q.tile_census(pts)
    assert len(cen) == len(combos) == 20
    for (q, i, j), (dead, change) in zip(combos, cen):
        want = [s for s in (4 * q + i, 4 * q + j) if s > 0]
        assert change == want and not dead
        assert len(want) == 1 or want[0] // 4 == want[1] // 4
    assert {q for q, _, _ in combos} == {0, 1, 2, 3}


def test_dead_sample_cases():
    pts = Q.dead_samples()
    cen = Q.tile_census(pts)
    assert len(cen) == 48
    for p in range(16):
        assert cen[p] == ([p], []) and np.isnan(pts[16 * p + p]).all()
        assert cen[16 + p] == ([p], []) and C.unit_of(pts[16 * (16 + p) + p][None])[0, 0] > 1
        # the live sample behind the dead one is the first of another block (p = 0: of the tile)
        assert cen[32 + p] == ([p], [p + 1] if 0 < p < 15 else [])          # (p = 15: the dead sample ends the tile)
    assert cen[32][0] == [0] and cen[0][0] == [0]                     # a dead sample as the first of a tile, both kinds


def test_lattice_geometry_of_the_reference_grid(O):
    res = C.level_resolutions(O)
    g = Q.lattice_geometry(res)
    assert [S for S, _ in g] == [3] * 12 + [4, 4, 5, 5]                # table_scatter.hip's head: 5^3, 5^3, 4^3, 4^3, 3^3 below
    assert sum(S ** 3 for S, _ in g) == 702


def test_no_position_reaches_the_direct_branch(O):
    """The kernel's direct-to-table branch takes a sample whose cell lies past its level's lattice.  A lattice of a group of
    w = 2^shift blocks covers floor(e) + 2 cells per axis, e = res * w / 1024, where the cells do not tile the group, and e
    where they do.  A sample of the group has u < o + w / 1024 (o the group's origin).  Not tiling: the first cell past
    the lattice begins at least 1 / 1024 of a cell behind (o + w / 1024) * res, a multiple of 1 / 1024, while the fp32 product
    u * res (< 4096) is off by at most 2^-13: out of reach.  Tiling: the cell past the lattice begins AT (o + w / 1024) * res,
    which a product that rounds up would reach -- but on this grid the only levels that tile are 16 and 4096, where the
    product is exact.  So the branch has no GPU case on the reference grid.  Below, the float32 model of the locate at the
    last fp32 position of 65 536 blocks (64 lines through the block cube that take every coordinate of every axis), and at
    the last fp32 u of every block on all three axes at once: no level fires."""
    res = C.level_resolutions(O)
    tiling = [int(r) for r, (S, sh) in zip(res, Q.lattice_geometry(res)) if (int(r) << sh) % 1024 == 0]
    assert tiling == [16, 4096]
    rng = np.random.default_rng(340)
    b = np.arange(1024)
    blocks = [np.stack([b, b, b], 1)]
    for _ in range(63):
        blocks.append(np.stack([b, np.roll(b, int(rng.integers(1024))), np.roll(b, int(rng.integers(1024)))], 1))
    pos = Q.block_end_positions(np.concatenate(blocks))
    u = C.unit_of(pos)
    assert C.live_of(u).all() and np.array_equal(C.blocks_of(u), np.concatenate(blocks))
    assert not Q.past_lattice(u, res).any()
    last_u = np.nextafter(((b + 1) / 1024.0).astype(np.float32), np.float32(0.0))
    u = np.stack([last_u, last_u, last_u], 1)
    assert np.array_equal(C.blocks_of(u)[:, 0], b)
    assert not Q.past_lattice(u, res).any()
