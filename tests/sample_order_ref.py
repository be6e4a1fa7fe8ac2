"""Reference for nsr_sample_order (include/nsr.h, csrc/sample_order.hip): plain NumPy, no GPU, no project import.

The specification, restated:  per axis  u = ((x - bbox_min) / bbox_size + 1) / 2  (BBox.normalize, then the encoder's
(x + 1) / 2),  q = floor(clamp(u * 1024, 0, 1023))  with NaN -> 0,  q9 = max(q - 512, 0);  the key is the 27-bit interleave
of the three q9 (x in bit 0, y in bit 1, z in bit 2 of every triple).  The permutation is the STABLE ascending order of the keys
of the first n slots, n = min(max(m_dev[0], 0), sort_prefix), followed by the identity on the slots n .. M-1.

Everything here is integer-exact; check_perm reports which of its five conditions fails first, and where.
"""
import numpy as np

KEY_BITS = 9            # significant bits per axis
CELLS = 1 << KEY_BITS   # 512 cells per axis inside the box

# the anisotropic, off-centre box the tests use (every number exact in fp32)
BOX_MIN = (-1.5, -2.0, 0.25)
BOX_SIZE = (3.0, 4.0, 1.75)


def interleave(q9):
    """[n,3] cell indices in 0..511 -> uint32 [n] keys: bit b of axis d goes to key bit 3 b + d (one bit at a time)."""
    q9 = np.asarray(q9).astype(np.uint32).reshape(-1, 3)
    key = np.zeros(q9.shape[0], np.uint32)
    for b in range(KEY_BITS):
        for d in range(3):
            key |= ((q9[:, d] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + d)
    return key


def cells_from_key(key):
    """inverse of interleave: uint32 [n] keys below 2^27 -> int64 [n,3] cell indices"""
    key = np.asarray(key).astype(np.uint32).reshape(-1)
    q9 = np.zeros((key.shape[0], 3), np.int64)
    for b in range(KEY_BITS):
        for d in range(3):
            q9[:, d] |= ((key >> np.uint32(3 * b + d)) & np.uint32(1)).astype(np.int64) << b
    return q9


def quantise(xyz, bbox_min, bbox_size):
    """[n,3] positions -> int64 [n,3] q9, evaluated in float64 from the fp32 inputs the kernel sees"""
    x = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    mn = np.asarray(bbox_min, np.float32).astype(np.float64)
    sz = np.asarray(bbox_size, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        u = ((x - mn) / sz + 1.0) / 2.0
        s = u * 1024.0
        s = np.where(np.isnan(s), 0.0, np.minimum(np.maximum(s, 0.0), 1023.0))
    q = np.floor(s).astype(np.int64)
    return np.maximum(q - CELLS, 0)


def morton_key(xyz, bbox_min, bbox_size):
    """uint32 [n]: the key nsr_sample_order sorts by"""
    return interleave(quantise(xyz, bbox_min, bbox_size))


def _cell_fp32(xyz, bbox_min, bbox_size):
    """the kernel's own fp32 expression, up to floor(u * 1024) - 512 (unclamped, so cells outside the box keep their number)"""
    x = np.asarray(xyz, np.float32)
    mn, sz = np.asarray(bbox_min, np.float32), np.asarray(bbox_size, np.float32)
    u = ((x - mn) / sz + np.float32(1.0)) * np.float32(0.5)
    assert u.dtype == np.float32
    return np.floor(u * np.float32(1024.0)).astype(np.int64) - CELLS


def positions_at_cells(q9, bbox_min, bbox_size):
    """float32 [n,3]: the centre of cell 512 + q9 on every axis (q9 may lie outside 0..511: a cell beyond a face of the box).
    x = bmin + bsize (2 u - 1), u = (512 + q9 + 0.5) / 1024 in float64, rounded once.  The rounding moves a position by ~1e-7
    of the box, the centre is 5e-4 of the box away from the cell's edges: any fp32 evaluation of the key expression lands in
    the cell, which is asserted here with the kernel's."""
    q9 = np.asarray(q9, np.int64).reshape(-1, 3)
    mn = np.asarray(bbox_min, np.float32).astype(np.float64)
    sz = np.asarray(bbox_size, np.float32).astype(np.float64)
    u = (CELLS + q9 + 0.5) / 1024.0
    xyz = (mn + sz * (2.0 * u - 1.0)).astype(np.float32)
    back = _cell_fp32(xyz, bbox_min, bbox_size)
    bad = np.flatnonzero((back != q9).any(axis=1))
    if bad.size:
        raise AssertionError('positions_at_cells: sample {} lands in cell {} instead of {}'.format(bad[0], back[bad[0]], q9[bad[0]]))
    return xyz


def expected_perm(keys, n, M):
    keys = np.asarray(keys)
    return np.concatenate([np.argsort(keys[:n], kind='stable').astype(np.int64), np.arange(n, M, dtype=np.int64)])


def _fail(cond, what, pos, detail):
    raise AssertionError('({}) {}: first at position {}: {}'.format(cond, what, pos, detail))


def check_perm(perm, keys, n, M):
    """perm: integer [M] (a uint32 bit pattern read as int32 is accepted); keys: the keys of (at least) the first n slots.
    Raises AssertionError naming the first violated condition -- (a) bijection, (b) identity tail, (c) key order, (d) stability,
    (e) equality with expected_perm -- and the first position that violates it."""
    perm = np.asarray(perm).reshape(-1)
    if perm.dtype == np.int32:
        perm = perm.view(np.uint32)
    perm = perm.astype(np.int64)
    keys = np.asarray(keys).astype(np.int64)[:n]
    if perm.shape[0] != M or keys.shape[0] != n or not 0 <= n <= M:
        raise AssertionError('check_perm: {} entries for M = {}, {} keys for n = {}'.format(perm.shape[0], M, keys.shape[0], n))
    # (a) every index of 0 .. M-1 exactly once
    bad = np.flatnonzero((perm < 0) | (perm >= M))
    if bad.size:
        _fail('a', 'not a bijection of 0..{}'.format(M - 1), bad[0], 'index {} out of range'.format(perm[bad[0]]))
    seen = np.bincount(perm, minlength=M)
    if M and seen.max() > 1:
        v = int(np.flatnonzero(seen > 1)[0])
        at = np.flatnonzero(perm == v)
        missing = np.flatnonzero(seen == 0)
        _fail('a', 'not a bijection of 0..{}'.format(M - 1), at[1],
              'index {} again (first at {}); {} indices missing, the lowest {}'.format(v, at[0], missing.size, missing[0]))
    # (b) the slots at and past n keep their place, so the first n entries are the first n indices
    bad = np.flatnonzero(perm[:n] >= n)
    if bad.size:
        _fail('b', 'tail is not the identity', bad[0], 'index {} of the tail inside the sorted prefix of {}'.format(perm[bad[0]], n))
    bad = np.flatnonzero(perm[n:] != np.arange(n, M))
    if bad.size:
        _fail('b', 'tail is not the identity', n + bad[0], 'holds {}'.format(perm[n + bad[0]]))
    # (c) keys along the prefix never decrease
    along = keys[perm[:n]]
    bad = np.flatnonzero(np.diff(along) < 0)
    if bad.size:
        j = bad[0] + 1
        _fail('c', 'keys not in non-decreasing order', j, 'key {:#x} (sample {}) after key {:#x} (sample {})'.format(
            along[j], perm[j], along[j - 1], perm[j - 1]))
    # (d) inside a run of equal keys the indices ascend
    bad = np.flatnonzero((np.diff(along) == 0) & (np.diff(perm[:n]) < 0))
    if bad.size:
        j = bad[0] + 1
        _fail('d', 'not stable', j, 'sample {} after sample {}, both with key {:#x}'.format(perm[j], perm[j - 1], along[j]))
    # (e) and all of it at once
    want = expected_perm(keys, n, M)
    bad = np.flatnonzero(perm != want)
    if bad.size:
        _fail('e', 'differs from the stable argsort', bad[0], 'holds {}, expected {}'.format(perm[bad[0]], want[bad[0]]))
