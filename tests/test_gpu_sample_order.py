"""nsr_sample_order (csrc/sample_order.hip, the hand-written three-pass LSD radix sort) called directly through the C ABI and
compared with the stable argsort of an independent restatement of its key (sample_order_ref.py), at the sizes, device counts,
key distributions and positions where a radix sort goes wrong -- and at the production shape, several tiles per block.

Every case runs the sort twice on a workspace filled with different garbage (the call must initialise every counter it
reads), between guard bands that must stay untouched, into a permutation buffer pre-filled with a sentinel.  Every comparison
is an exact integer comparison; sample_order_ref.check_perm names the violated condition -- (a) bijection, (b) identity tail,
(c) key order, (d) stability, (e) equality with the expected permutation -- and the first offending position.

The box is anisotropic and off-centre (min (-1.5, -2, 0.25), size (3, 4, 1.75)), so an exchange of two axes or a sign error in
the normalisation changes the keys.
"""
import ctypes

import numpy as np
import pytest
import torch

import sample_order_ref as R

pytestmark = pytest.mark.gpu

MN, SZ = R.BOX_MIN, R.BOX_SIZE
TILE = 8192                 # keys per tile (SO_TILE)
BLOCKS = 768                # most blocks the host launches (SO_BLOCKS_TARGET)
GUARD = 8192                # bytes on each side of the workspace
SENTINEL = -1               # 0xFFFFFFFF: never an index
NSR_OK, NSR_ERR_INVALID_ARG = 0, -1
NAN = np.float32('nan')


def _garbage(nbytes, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=g)


def _call(xyz_d, M, m_d, sort_prefix, perm_d, ws_ptr, box=(MN, SZ)):
    from nerfstyle_amd import _lib as L
    c3 = ctypes.c_float * 3
    return L.lib().nsr_sample_order(L.p(xyz_d), M, L.p(m_d), sort_prefix, c3(*box[0]), c3(*box[1]), L.p(perm_d), ws_ptr, L.stream())


def sorted_length(M, m_count, sort_prefix):
    prefix = min(sort_prefix, M)
    return prefix if m_count is None else min(max(m_count, 0), prefix)


def run_and_check(dev, xyz, m_count=None, sort_prefix=None, keys=None):
    """xyz: float32 [M,3]; m_count: None (m_dev == NULL) or the device count; sort_prefix: None = M.  The slots at and past the
    sorted length are overwritten with NaN positions here: the result must not depend on them.  Returns the permutation."""
    from nerfstyle_amd import _lib as L
    M = xyz.shape[0]
    sort_prefix = M if sort_prefix is None else sort_prefix
    n = sorted_length(M, m_count, sort_prefix)
    xyz = np.ascontiguousarray(xyz, np.float32).copy()
    xyz[n:] = NAN
    keys = R.morton_key(xyz[:n], MN, SZ) if keys is None else keys[:n]
    xyz_d = torch.as_tensor(xyz, device=dev)
    m_d = None if m_count is None else torch.tensor([m_count, 0], dtype=torch.int32, device=dev)

    nbytes = int(L.lib().nsr_sample_order_workspace_bytes(M))
    assert nbytes >= 3 * 4 * M
    buf = _garbage(nbytes + 2 * GUARD + 256, dev, 1)
    off = ((buf.data_ptr() + GUARD + 255) & ~255) - buf.data_ptr()
    assert off >= 4096 and buf.numel() - (off + nbytes) >= 4096
    lo, hi = buf[:off].clone(), buf[off + nbytes:].clone()
    perms = []
    for seed in (1, 2):
        if seed > 1:
            buf[off:off + nbytes] = _garbage(nbytes, dev, seed)
        perm_d = torch.full((M,), SENTINEL, dtype=torch.int32, device=dev)
        assert _call(xyz_d, M, m_d, sort_prefix, perm_d, buf.data_ptr() + off) == NSR_OK
        torch.cuda.synchronize()
        assert torch.equal(buf[:off], lo), 'write below the workspace'
        assert torch.equal(buf[off + nbytes:], hi), 'write past nsr_sample_order_workspace_bytes(M)'
        assert int((perm_d == SENTINEL).sum()) == 0, 'slots of perm left unwritten'
        perms.append(perm_d)
    assert torch.equal(perms[0], perms[1]), 'the result depends on what the workspace held'
    perm = perms[0].cpu().numpy()
    R.check_perm(perm, keys, n, M)
    return perm


def _random_cells(rng, n):
    return rng.integers(0, R.CELLS, (n, 3))


def _xyz(q9):
    return R.positions_at_cells(q9, MN, SZ)


# ---------------------------------------------------------------------------------------------
# sizes around a wave (64), a wave's items (1024), a tile (8192)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 8191, 8192, 8193, 16384, 3 * 8192 + 1])
def test_sizes(dev, n):
    q9 = _random_cells(np.random.default_rng(100 + n), n)
    if n >= 1024:
        q9[n // 2:] = q9[:n - n // 2]           # every key twice, a tile or more apart from 16384 on: stability is observable
    run_and_check(dev, _xyz(q9))


# ---------------------------------------------------------------------------------------------
# the device-side count and sort_prefix: sorted length min(max(m_dev[0], 0), sort_prefix), sort_prefix clamped to M
# ---------------------------------------------------------------------------------------------
M_COUNT = 20000
COUNT_CASES = ([(m, M_COUNT) for m in (0, 1, 8192, 19999, 20000, 25000, -5)]
               + [(-1, 0), (1, 0), (0, 1), (2, 1), (4999, 5000), (20000, 5000), (8191, 8192), (8193, 8192), (3000, 12345),
                  (12346, 12345)]
               + [(None, 5000), (None, 0), (None, 30000), (15000, 30000), (25000, 30000), (19999, 0xFFFFFFFF)])


def _count_population():
    q9 = _random_cells(np.random.default_rng(7), M_COUNT)
    q9[M_COUNT // 2:] = q9[:M_COUNT // 2][::-1]                      # repeats
    xyz = _xyz(q9)
    xyz.setflags(write=False)
    return xyz


@pytest.fixture(scope='module')
def count_population():
    return _count_population()


@pytest.mark.parametrize('m_count,sort_prefix', COUNT_CASES)
def test_device_count_and_prefix(dev, count_population, m_count, sort_prefix):
    n = sorted_length(M_COUNT, m_count, sort_prefix)
    perm = run_and_check(dev, count_population, m_count, sort_prefix)
    assert np.array_equal(perm[n:].astype(np.int64), np.arange(n, M_COUNT))
    if n == 0:
        assert np.array_equal(perm.astype(np.int64), np.arange(M_COUNT))


# ---------------------------------------------------------------------------------------------
# key distributions
# ---------------------------------------------------------------------------------------------
def _k_one_cell(rng, n):
    return np.full(n, R.interleave(np.array([[137, 402, 55]]))[0], np.uint32)


def _k_two_alternating(rng, n):
    lo, hi = sorted(R.interleave(np.array([[400, 3, 250], [2, 300, 77]])).tolist())
    assert lo < hi
    return np.where(np.arange(n) % 2 == 0, hi, lo).astype(np.uint32)    # the larger key first: every sample moves


def _k_one_digit(digit):
    def f(rng, n):
        const = 0x2A5A5A5 & ~(0x1FF << (9 * digit))                 # the other two digits: fixed, non-zero
        return (const | (rng.integers(0, 512, n) << (9 * digit))).astype(np.uint32)
    return f


def _k_all_bins_in_order(rng, n):
    return ((0x155 << 18) | (0x0F3 << 9) | (np.arange(n) % 512)).astype(np.uint32)


def _k_repeating(rng, n):
    return (rng.integers(0, 4096, n) * 32769).astype(np.uint32)      # 4096 distinct keys over all 27 bits, many repeats


def _k_sorted(rng, n):
    return np.sort(_k_repeating(rng, n))


def _k_reverse_sorted(rng, n):
    return np.sort(_k_repeating(rng, n))[::-1].copy()


def _k_mostly_one_cell(rng, n):
    k = R.interleave(_random_cells(rng, n))
    k[rng.random(n) < 0.9] = R.interleave(np.array([[255, 256, 1]]))[0]
    return k


def _k_run_across_slot_8192(rng, n):
    k = R.interleave(_random_cells(rng, n))
    k[8192 - 1500:8192 + 1500] = R.interleave(np.array([[31, 480, 256]]))[0]
    return k


DISTRIBUTIONS = {'one_cell': _k_one_cell, 'two_alternating': _k_two_alternating, 'digit0_only': _k_one_digit(0),
                 'digit1_only': _k_one_digit(1), 'digit2_only': _k_one_digit(2), 'all_512_bins_in_order': _k_all_bins_in_order,
                 'sorted': _k_sorted, 'reverse_sorted': _k_reverse_sorted, 'mostly_one_cell': _k_mostly_one_cell,
                 'run_across_slot_8192': _k_run_across_slot_8192}


@pytest.mark.parametrize('n', [8192 + 1000, 5 * 8192 + 17])
@pytest.mark.parametrize('name', sorted(DISTRIBUTIONS))
def test_key_distributions(dev, name, n):
    want_keys = DISTRIBUTIONS[name](np.random.default_rng(n), n)
    assert want_keys.shape == (n,) and int(want_keys.max()) < 1 << 27
    xyz = _xyz(R.cells_from_key(want_keys))
    keys = R.morton_key(xyz, MN, SZ)
    assert np.array_equal(keys, want_keys)                          # the positions carry the keys the case is about
    perm = run_and_check(dev, xyz, keys=keys)
    if name in ('one_cell', 'sorted'):
        assert np.array_equal(perm.astype(np.int64), np.arange(n))


# ---------------------------------------------------------------------------------------------
# geometry: which axis owns which bit; positions outside the box, NaN, +-inf
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_keys_differ_along_one_axis(dev, axis):
    n = 8192 + 3000
    q9 = np.empty((n, 3), np.int64)
    q9[:] = (19, 200, 511)
    q9[:, axis] = np.random.default_rng(axis).integers(0, 512, n)
    perm = run_and_check(dev, _xyz(q9))
    # the order is the stable order of that coordinate alone
    assert np.array_equal(perm.astype(np.int64), np.argsort(q9[:, axis], kind='stable'))


def test_outside_nan_and_inf_sort_with_the_faces(dev):
    """samples one cell and ten box sizes beyond each face sort exactly like the face cell (0 or 511) of that axis, NaN and -inf
    like cell 0, +inf like cell 511: each is mixed into an in-box population next to a twin IN the face cell with the same
    other two coordinates, so the two keys are equal and stability fixes their order"""
    rng = np.random.default_rng(21)
    n = 2 * 8192 + 345
    q9 = _random_cells(rng, n)
    xyz = _xyz(q9)
    want_q9 = q9.copy()
    slots = iter(rng.permutation(n)[:200].tolist())
    specials = []
    for d in range(3):
        for cell, face in ((-1, 0), (-5120, 0), (512, 511), (5632, 511), ('nan', 0), ('-inf', 0), ('+inf', 511)):
            i, twin = next(slots), next(slots)
            c = rng.integers(0, 512, 3)
            c[d] = face
            q9[twin] = want_q9[twin] = want_q9[i] = c
            xyz[twin] = _xyz(c[None])[0]
            if isinstance(cell, str):
                xyz[i] = xyz[twin]
                xyz[i, d] = {'nan': NAN, '-inf': -np.float32('inf'), '+inf': np.float32('inf')}[cell]
            else:
                c = c.copy()
                c[d] = cell
                xyz[i] = _xyz(c[None])[0]
                lo, hi = MN[d], MN[d] + SZ[d]
                assert xyz[i, d] < lo or xyz[i, d] > hi
                if abs(cell) > 600:
                    assert xyz[i, d] < lo - 9.9 * SZ[d] or xyz[i, d] > hi + 9.9 * SZ[d]
            specials.append((i, twin))
    keys = R.morton_key(xyz, MN, SZ)
    assert np.array_equal(keys, R.interleave(want_q9))
    perm = run_and_check(dev, xyz, keys=keys).astype(np.int64)
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    for i, twin in specials:                                        # next to its twin unless a third sample shares the cell
        between = perm[min(where[i], where[twin]):max(where[i], where[twin]) + 1]
        assert np.all(keys[between] == keys[i]) and (where[i] < where[twin]) == (i < twin)


# ---------------------------------------------------------------------------------------------
# continuous positions
# ---------------------------------------------------------------------------------------------
def test_continuous_positions(dev):
    """uniform fp32 positions, keys from the float64 evaluation; a position whose u * 1024 lies within 1e-3 of an integer on any
    axis is redrawn first (the kernel's fp32 expression is off by ~1e-4 there at most: 3 roundings at <= 2^-24 relative, x 1024),
    so no sample is ambiguous and none is left out"""
    n = 100000
    rng = np.random.default_rng(33)
    mn, sz = np.array(MN), np.array(SZ)
    xyz = (mn + sz * rng.random((n, 3))).astype(np.float32)

    def ambiguous(p):
        s = ((p.astype(np.float64) - mn) / sz + 1.0) / 2.0 * 1024.0
        return (np.abs(s - np.rint(s)) < 1e-3).any(axis=1) | (p < mn).any(axis=1) | (p >= mn + sz).any(axis=1)
    bad = np.flatnonzero(ambiguous(xyz))
    assert bad.size > 0
    while bad.size:
        xyz[bad] = (mn + sz * rng.random((bad.size, 3))).astype(np.float32)
        bad = bad[ambiguous(xyz[bad])]
    assert xyz.shape == (n, 3) and not ambiguous(xyz).any()
    keys = R.morton_key(xyz, MN, SZ)
    assert keys.shape == (n,) and np.unique(keys).size > n // 2
    run_and_check(dev, xyz, keys=keys)


# ---------------------------------------------------------------------------------------------
# several tiles per block: the production shape
# ---------------------------------------------------------------------------------------------
N_BIG = BLOCKS * TILE + 13 * TILE + 77


def _per(n):
    """ceil(ceil(n / 8192) / 768): tiles per block"""
    ntiles = (n + TILE - 1) // TILE
    return (ntiles + BLOCKS - 1) // BLOCKS


def _big_population():
    assert N_BIG == 6398029 and -(-N_BIG // TILE) == 782 and _per(N_BIG) == 2
    rng = np.random.default_rng(55)
    q9 = _random_cells(rng, N_BIG)
    # 20 000 equal keys across the boundary between block 5's second tile (11) and block 6's first (12) ...
    edge = (5 * 2 + 2) * TILE
    q9[edge - 10000:edge + 10000] = (300, 17, 129)
    # ... and 3000 across the common edge of block 100's two tiles (200, 201)
    edge = (100 * 2 + 1) * TILE
    q9[edge - 1500:edge + 1500] = (5, 411, 260)
    xyz = _xyz(q9)
    keys = R.morton_key(xyz, MN, SZ)
    assert np.array_equal(keys, R.interleave(q9))
    xyz.setflags(write=False)
    keys.setflags(write=False)
    return xyz, keys


@pytest.fixture(scope='module')
def big_population():
    return _big_population()


@pytest.mark.parametrize('m_count', [None, N_BIG - 5000])
def test_two_tiles_per_block(dev, big_population, m_count):
    """782 tiles on 768 blocks: blocks 0..390 walk two tiles each (the per-digit base carried from the first to the second, the
    wave counters cleared in between), the last tile is partial, blocks 391..767 own nothing; with the device count 5000 below
    (781 tiles, still two per block) the tail is NaN"""
    xyz, keys = big_population
    n = sorted_length(N_BIG, m_count, N_BIG)
    assert _per(n) == 2 and _per(N_BIG) == 2                        # tiles per block of the sorted length and of sort_prefix
    assert min(-(-N_BIG // TILE), BLOCKS) == BLOCKS                 # the host's block count
    run_and_check(dev, xyz, m_count, keys=keys)


# ---------------------------------------------------------------------------------------------
# argument checks: return before any launch
# ---------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    from nerfstyle_amd import _lib as L
    M = 1000
    xyz_d = torch.as_tensor(_xyz(_random_cells(np.random.default_rng(9), M)), device=dev)
    nbytes = int(L.lib().nsr_sample_order_workspace_bytes(M))
    assert int(L.lib().nsr_sample_order_workspace_bytes(0)) == 0
    buf = _garbage(nbytes + 512, dev, 3)
    before = buf.clone()
    ws = (buf.data_ptr() + 255) & ~255
    perm_d = torch.full((M,), SENTINEL, dtype=torch.int32, device=dev)
    assert _call(xyz_d, 0, None, 0, perm_d, ws) == NSR_OK
    assert _call(None, 0, None, 0, None, None) == NSR_OK
    for misalign in (1, 4, 128):
        assert _call(xyz_d, M, None, M, perm_d, ws + misalign) == NSR_ERR_INVALID_ARG
    assert _call(xyz_d, M, None, M, None, ws) == NSR_ERR_INVALID_ARG
    assert _call(None, M, None, M, perm_d, ws) == NSR_ERR_INVALID_ARG
    assert _call(xyz_d, M, None, M, perm_d, None) == NSR_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert int((perm_d != SENTINEL).sum()) == 0 and torch.equal(buf, before)    # nothing was launched
    assert _call(xyz_d, M, None, M, perm_d, ws) == NSR_OK
    torch.cuda.synchronize()
    R.check_perm(perm_d.cpu().numpy(), R.morton_key(xyz_d.cpu().numpy(), MN, SZ), M, M)
