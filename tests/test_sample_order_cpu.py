"""The reference and the checker behind tests/test_gpu_sample_order.py, tested on their own (no GPU): the key restates the
specification independently of the kernel's mask-spread form, and check_perm rejects every kind of wrong permutation with the
condition that names it."""
import numpy as np
import pytest

import sample_order_ref as R

MN, SZ = R.BOX_MIN, R.BOX_SIZE


def _spread(v):
    """the mask-spread form the kernel and tests/test_gpu_field.py share"""
    v = v.astype(np.uint64) & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def test_morton_key_equals_mask_spread_form():
    rng = np.random.default_rng(1)
    q9 = rng.integers(0, 512, (200000, 3))
    want = _spread(q9[:, 0]) | (_spread(q9[:, 1]) << 1) | (_spread(q9[:, 2]) << 2)
    assert np.array_equal(R.interleave(q9).astype(np.uint64), want)
    assert np.array_equal(R.morton_key(R.positions_at_cells(q9, MN, SZ), MN, SZ).astype(np.uint64), want)
    assert np.array_equal(R.cells_from_key(R.interleave(q9)), q9)


def test_morton_key_axis_bits():
    """x owns bit 0, y bit 1, z bit 2 of every triple; the key grows with each coordinate"""
    one = lambda c: int(R.interleave(np.array([c]))[0])
    assert (one([1, 0, 0]), one([0, 1, 0]), one([0, 0, 1])) == (1, 2, 4)
    assert (one([2, 0, 0]), one([0, 2, 0]), one([0, 0, 2])) == (8, 16, 32)
    assert (one([256, 0, 0]), one([0, 256, 0]), one([0, 0, 256])) == (1 << 24, 1 << 25, 1 << 26)
    assert one([511, 511, 511]) == (1 << 27) - 1
    for d in range(3):
        q9 = np.zeros((512, 3), np.int64)
        q9[:, d] = np.arange(512)
        assert np.all(np.diff(R.morton_key(R.positions_at_cells(q9, MN, SZ), MN, SZ).astype(np.int64)) > 0)


def test_morton_key_clamping():
    mn, sz = np.array(MN, np.float64), np.array(SZ, np.float64)
    centre = (mn + sz / 2).astype(np.float32)                       # u = 0.75: cell 256 on every axis
    assert R.quantise(centre[None], MN, SZ).tolist() == [[256, 256, 256]]
    nan, inf = np.float32('nan'), np.float32('inf')
    for d in range(3):
        def at(v):
            p = centre.copy()
            p[d] = v
            return int(R.quantise(p[None], MN, SZ)[0, d]), int(R.morton_key(p[None], MN, SZ)[0])

        def cell(c):
            q = np.full((1, 3), 256)
            q[0, d] = c
            return c, int(R.interleave(q)[0])
        assert at(mn[d] - 0.3 * sz[d]) == cell(0)                   # below the box
        assert at(mn[d] - 10 * sz[d]) == cell(0)
        assert at(mn[d] + 1.3 * sz[d]) == cell(511)                 # above it
        assert at(mn[d] + 11 * sz[d]) == cell(511)
        assert at(nan) == cell(0)
        assert at(inf) == cell(511)
        assert at(-inf) == cell(0)
        assert at(mn[d]) == cell(0)                                 # the faces themselves: u = 0.5 and u = 1
        assert at(mn[d] + sz[d]) == cell(511)
        assert at(np.nextafter(np.float32(mn[d] + sz[d]), -inf)) == cell(511)
    # the lower half of the encoder's input range (u < 0.5) is all cell 0: only 9 bits per axis are significant
    assert R.quantise((mn - sz / 2).astype(np.float32)[None], MN, SZ).tolist() == [[0, 0, 0]]


def test_positions_at_cells_round_trip():
    rng = np.random.default_rng(2)
    q9 = rng.integers(0, 512, (300000, 3))
    q9[:4] = [[0, 0, 0], [511, 511, 511], [0, 511, 0], [511, 0, 511]]
    xyz = R.positions_at_cells(q9, MN, SZ)
    assert xyz.dtype == np.float32 and xyz.shape == q9.shape
    assert np.array_equal(R.quantise(xyz, MN, SZ), q9)
    mn, sz = np.array(MN), np.array(SZ)
    assert np.all(xyz > mn) and np.all(xyz < mn + sz)
    # cells beyond the faces keep their own position and clamp to the face cell in the key
    out = np.array([[-1, 5, 5], [512, 5, 5], [5, -5120, 5], [5, 5, 5632]])
    xo = R.positions_at_cells(out, MN, SZ)
    assert xo[0, 0] < mn[0] and xo[1, 0] > mn[0] + sz[0] and xo[2, 1] < mn[1] - 9 * sz[1] and xo[3, 2] > mn[2] + 10 * sz[2]
    assert R.quantise(xo, MN, SZ).tolist() == [[0, 5, 5], [511, 5, 5], [5, 0, 5], [5, 5, 511]]


def _case(n=20000, M=23000, seed=3, cells=12):
    """keys with many repeats (cells^3 distinct values), so that stability matters everywhere"""
    rng = np.random.default_rng(seed)
    keys = R.interleave(rng.integers(0, cells, (M, 3)) * 37)
    return keys, n, M, R.expected_perm(keys, n, M)


def _rejects(perm, keys, n, M, cond, pos=None):
    with pytest.raises(AssertionError) as e:
        R.check_perm(perm, keys, n, M)
    msg = str(e.value)
    assert msg.startswith('({})'.format(cond)), msg
    if pos is not None:
        assert 'first at position {}:'.format(pos) in msg, msg


def test_check_perm_accepts_expected():
    keys, n, M, want = _case()
    R.check_perm(want, keys, n, M)
    R.check_perm(want.astype(np.int32), keys, n, M)                 # the device tensor's dtype
    R.check_perm(want, keys[:n], n, M)
    for n2, M2 in ((0, 0), (0, 5), (1, 1), (5, 5)):
        R.check_perm(R.expected_perm(keys, n2, M2), keys, n2, M2)
    assert np.array_equal(np.sort(want), np.arange(M)) and np.array_equal(want[n:], np.arange(n, M))
    assert not np.array_equal(want[:n], np.arange(n))


def test_check_perm_rejects_duplicate():
    keys, n, M, want = _case()
    p = want.copy()
    p[777] = p[776]
    _rejects(p, keys, n, M, 'a', 777)
    p = want.copy()
    p[5] = M
    _rejects(p, keys, n, M, 'a', 5)
    p = want.astype(np.int32)
    p[9] = -1                                                       # a sentinel left in place
    _rejects(p, keys, n, M, 'a', 9)


def test_check_perm_rejects_unstable_equal_pair():
    keys, n, M, want = _case()
    along = keys[want[:n]]
    j = int(np.flatnonzero(along[1:] == along[:-1])[100]) + 1
    p = want.copy()
    p[[j - 1, j]] = p[[j, j - 1]]
    assert np.all(np.diff(keys[p[:n]].astype(np.int64)) >= 0)       # still in key order
    _rejects(p, keys, n, M, 'd', j)


def test_check_perm_rejects_inversion():
    keys, n, M, want = _case()
    along = keys[want[:n]]
    j = int(np.flatnonzero(along[1:] != along[:-1])[50]) + 1
    p = want.copy()
    p[[j - 1, j]] = p[[j, j - 1]]
    _rejects(p, keys, n, M, 'c', j)


def test_check_perm_rejects_tail():
    keys, n, M, want = _case()
    p = want.copy()
    p[[n + 10, n + 11]] = p[[n + 11, n + 10]]
    _rejects(p, keys, n, M, 'b', n + 10)
    # the tail sorted along with the rest: a bijection in key order, but not the documented one
    _rejects(np.argsort(keys, kind='stable'), keys, n, M, 'b')


def test_check_perm_rejects_tail_index_in_prefix():
    keys, n, M, want = _case()
    p = want.copy()
    p[[4321, n + 3]] = p[[n + 3, 4321]]
    _rejects(p, keys, n, M, 'b', 4321)


def test_check_perm_rejects_instability_across_a_tile_edge_only():
    """one key's run lies across position 8192 and only the two entries next to that edge are exchanged: what a lost carry
    between two tiles would look like"""
    M = n = 3 * 8192
    keys = np.empty(M, np.uint32)
    keys[:] = R.interleave(np.array([[300, 7, 7]]))[0]
    lo = np.random.default_rng(4).permutation(M)[:8000]             # 8000 smaller keys: the run of the rest begins at 8000
    keys[lo] = R.interleave(np.array([[3, 7, 7]]))[0]
    want = R.expected_perm(keys, n, M)
    assert keys[want[8191]] == keys[want[8192]]
    p = want.copy()
    p[[8191, 8192]] = p[[8192, 8191]]
    assert np.all(np.diff(keys[p].astype(np.int64)) >= 0)
    _rejects(p, keys, n, M, 'd', 8192)
    q = p.copy()
    q[[8191, 8192]] = q[[8192, 8191]]
    R.check_perm(q, keys, n, M)
