"""Inputs and references for the tests of the spatially ordered table scatter (csrc/table_scatter.hip): NumPy and the CPU
oracle, no GPU.

Shared by test_gpu_table_scatter_carry.py (the small block sequences: every wave walks ONE tile), by
test_gpu_table_scatter_walk.py (batches above 262 144 samples: a wave walks two or three tiles) and by
test_table_scatter_walk_cpu.py, which checks on the reference side alone that the large cases put what they are meant
to put on the tile boundaries.

Positions.  Blocks are the sample order's keys, 1/1024 of the encoder input u per axis; x = 8 u - 6 for the +-2 box, so the
box is u in [0.5, 1] and everything down to u = 0 (x = -6) is still encoded.  Blocks are always taken from the fp32
positions (unit_of, blocks_of), never from what a builder intended.

The walk.  nsr_sample_order sorts, stably, by the Morton code (x in bit 0) of the block coordinates q = clip(u * 1024, 0,
1023), 10 bits per axis -- of max(q, 512), to be exact: the kernel drops the top bit (always set inside the box) and clamps
what lies below the box to its face (sample_order.hip, k_order_keys; tests/sample_order_ref.py).  For positions inside the
box this is the plain 30-bit key of test_gpu_field.py's `spread`; below the box, samples whose blocks differ only in
coordinates under 512 share a key and keep their buffer order.  walk_order() restates it, and the GPU tests compare the
permutation that ran with it, so census() describes the walk the kernel made.

The launch (launch_model) restates nsr_table_scatter_launch and the head of k_table_scatter: min(4096, ceil(ntiles / 4))
workgroups of 4 waves for the CAPACITY's tiles, per = ceil(tiles of the COUNT / waves) consecutive 16-sample tiles a wave.
"""
import functools

import numpy as np

TILE = 16
MAX_BLOCKS = 4096
WAVES_PER_BLOCK = 4
SINGLE_TILE_LIMIT = TILE * MAX_BLOCKS * WAVES_PER_BLOCK          # 262 144: the largest batch with one tile per wave


# ---------------------------------------------------------------------------------------------
# positions -> encoder input, block, key, walk
# ---------------------------------------------------------------------------------------------
def unit_of(pts):
    """field_unit (field_common.h) in the same fp32 operations"""
    xn = (pts.astype(np.float32) - np.float32(-2.0)) / np.float32(4.0)
    return (xn + np.float32(1.0)) / np.float32(2.0)


def live_of(u):
    return np.all((u >= 0) & (u <= 1), axis=1)


def blocks_of(u):
    """int64 [n, 3]: clip(u * 1024, 0, 1023) in fp32, truncated (NaN -> 0), as the sort and the scatter quantise"""
    with np.errstate(invalid='ignore'):
        s = np.asarray(u, np.float32) * np.float32(1024.0)
        s = np.where(np.isnan(s), np.float32(0.0), np.minimum(np.maximum(s, np.float32(0.0)), np.float32(1023.0)))
    return s.astype(np.int64)


def _spread(v):
    v = v.astype(np.uint64) & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_key(q):
    """30-bit Morton code of 10-bit block coordinates [n, 3], x in bit 0"""
    q = np.asarray(q)
    return _spread(q[:, 0]) | (_spread(q[:, 1]) << 1) | (_spread(q[:, 2]) << 2)


def walk_key(q):
    """the key nsr_sample_order sorts by, up to its constant top bits: coordinates below the box clamp to the box's face"""
    return morton_key(np.maximum(np.asarray(q), 512))


def walk_order(pts, count=None):
    """int64 [count]: buffer indices in the order the scatter walks them -- the stable argsort of walk_key"""
    n = pts.shape[0] if count is None else int(count)
    return np.argsort(walk_key(blocks_of(unit_of(pts[:n]))), kind='stable')


# ---------------------------------------------------------------------------------------------
# the launch
# ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-int(a) // int(b))


def launch_model(M, count=None):
    """capacity M, device count (default M) -> the partition of the walk over the waves.
    begin / end: every wave's tile range; full / short / empty: waves with `per` tiles, with fewer, with none;
    end_lanes: samples in the walk's last tile (1 .. 16: the count ends at that lane); end_wave / end_tile_in_wave: where
    that tile is."""
    Mc = int(M) if count is None else int(count)
    assert 0 < Mc <= M
    nblocks = max(1, min(MAX_BLOCKS, _cdiv(_cdiv(M, TILE), WAVES_PER_BLOCK)))
    nwaves = WAVES_PER_BLOCK * nblocks
    ntiles = _cdiv(Mc, TILE)
    per = _cdiv(ntiles, nwaves)
    begin = np.minimum(np.arange(nwaves, dtype=np.int64) * per, ntiles)
    end = np.minimum(begin + per, ntiles)
    n = end - begin
    end_wave = (ntiles - 1) // per
    return dict(nblocks=nblocks, nwaves=nwaves, ntiles=ntiles, per=per, begin=begin, end=end,
                full=int((n == per).sum()), short=int(((n > 0) & (n < per)).sum()), empty=int((n == 0).sum()),
                end_lanes=Mc - TILE * (ntiles - 1), end_wave=int(end_wave), end_tile_in_wave=int(ntiles - 1 - begin[end_wave]))


CLASSES = ('a', 'b', 'c', 'd', 'e', 'f')


def census(pts, M=None, count=None):
    """What the walk of pts[:count] (capacity M) meets at its INTERIOR tile boundaries: between tiles t and t + 1 of one wave.
    By the last live sample of the wave before the boundary and the first one after it:
      a  same block                                   b  the +x neighbour, y and z blocks equal (the shift-carry on the
      c  any other block change                          block-anchored levels)
    (a boundary with no live sample of its wave on one side is counted as 'open'), and by the two samples AT the boundary:
      d  lane 15 of t dead, lane 0 of t + 1 live      e  lane 0 of t + 1 dead, lane 15 of t live      f  both dead
    'inside_long': class a with both lanes live, inside a run of >= 20 live samples of one block.
    Returns {'launch': launch_model, 'boundaries': n, 'all': {class: n}, 'by_step': [{class: n} for the boundary after the
    wave's 1st, 2nd ... tile]}."""
    M = pts.shape[0] if M is None else int(M)
    n = M if count is None else int(count)
    lm = launch_model(M, n)
    per = lm['per']
    order = walk_order(pts, n)
    u = unit_of(pts[order])
    live = live_of(u)
    q = blocks_of(u)
    idx = np.arange(n, dtype=np.int64)
    prev_live = np.maximum.accumulate(np.where(live, idx, -1))
    next_live = np.minimum.accumulate(np.where(live, idx, n)[::-1])[::-1]
    lq = q[live]
    rid = np.concatenate([[0], np.cumsum(np.any(lq[1:] != lq[:-1], axis=1))]) if lq.shape[0] else np.zeros(0, np.int64)
    runlen = np.bincount(rid) if rid.size else np.zeros(0, np.int64)
    run_of = np.full(n, -1, np.int64)
    run_of[live] = rid

    t = np.arange(max(lm['ntiles'] - 1, 0), dtype=np.int64)
    wave = t // per
    t = t[(t + 1) // per == wave]
    wave = t // per
    step = t - wave * per
    p = TILE * (t + 1)
    lo, hi = TILE * wave * per, np.minimum(TILE * (wave + 1) * per, n)
    ia, ib = prev_live[p - 1], next_live[p]
    both = (ia >= lo) & (ib < hi)
    ia, ib = np.where(both, ia, 0), np.where(both, ib, 0)
    qa, qb = q[ia], q[ib]
    same = np.all(qa == qb, axis=1)
    plusx = (qb[:, 0] == qa[:, 0] + 1) & (qb[:, 1] == qa[:, 1]) & (qb[:, 2] == qa[:, 2])
    dd, de = ~live[p - 1], ~live[p]
    cls = {'a': both & same, 'b': both & plusx, 'c': both & ~same & ~plusx, 'd': dd & ~de, 'e': de & ~dd, 'f': dd & de,
           'open': ~both}
    cls['inside_long'] = cls['a'] & ~dd & ~de & (run_of[ia] == run_of[ib]) & (runlen[np.maximum(run_of[ia], 0)] >= 20)

    def count_of(sel):
        return {k: int((v & sel).sum()) for k, v in cls.items()}
    return dict(launch=lm, boundaries=int(t.size), all=count_of(np.ones(t.size, bool)),
                by_step=[count_of(step == k) for k in range(max(per - 1, 0))])


# ---------------------------------------------------------------------------------------------
# what a wrong walk would scatter
# ---------------------------------------------------------------------------------------------
WALK_FAULTS = ('refill_from_this_tile', 'positions_from_this_tile', 'no_fetch_two_ahead')


def walk_inputs(pts, genc, M=None, count=None, fault=None):
    """The samples as k_table_scatter's steps see them, in walk order: (positions [n, 3], encoder gradients [n, 16, C]).
    fault None: the kernel as it is.  Otherwise a host model of one mistake in the code that carries state from a wave's
    tile into its next one, read off the kernel's loop (idx, idx_next and idx_nn are the permutation entries of this tile,
    the next and the one after; the ring holds eight gradient rows):
      refill_from_this_tile     the ring's wrap refill reads idx, not idx_next: steps 0 .. 7 of every tile but a wave's
                                first use the gradient rows of the tile before, same lanes
      positions_from_this_tile  the next tile's positions are loaded through idx: every tile but a wave's first works on the
                                positions of the tile before, with its own gradient rows
      no_fetch_two_ahead        idx_nn is never fetched and stays idx_next: from a wave's third tile on, every tile is the
                                wave's second one again, positions and gradients (no effect below three tiles a wave)
    The count's mask is the true one in every case (it comes from the tile's number).  This is the reference side's means of
    showing that a case tells such a walk from the right one; it runs nothing on the GPU."""
    M = pts.shape[0] if M is None else int(M)
    n = M if count is None else int(count)
    lm = launch_model(M, n)
    order = walk_order(pts, n)
    i = np.arange(lm['ntiles'] * TILE, dtype=np.int64)
    tile, lane = i // TILE, i % TILE
    first = lm['begin'][tile // lm['per']]                       # the first tile of the tile's wave
    src_p = src_g = tile
    if fault == 'refill_from_this_tile':
        src_g = np.where((tile > first) & (lane < 8), tile - 1, tile)
    elif fault == 'positions_from_this_tile':
        src_p = np.where(tile > first, tile - 1, tile)
    elif fault == 'no_fetch_two_ahead':
        src_p = src_g = np.where(tile > first + 1, first + 1, tile)
    else:
        assert fault is None
    ip = order[np.minimum(src_p * TILE + lane, n - 1)][:n]       # lanes past the count read the last valid entry
    ig = order[np.minimum(src_g * TILE + lane, n - 1)][:n]
    return pts[ip], genc[ig]


# ---------------------------------------------------------------------------------------------
# the fp64 reference scatter
# ---------------------------------------------------------------------------------------------
def level_resolutions(O):
    pls = O.per_level_scale_from_cfg()
    return O.grid_resolutions(16, O.grid_S(pls), 16)


def level_offsets(O):
    """row offsets of the reference LLFF grid (16 levels, 16 .. 4096, 2^19 rows a level at the most)"""
    return O.grid_offsets(16, O.per_level_scale_from_cfg(), 16, 19, align_corners=True)


def _level_rows(O, ul, offsets, res, l):
    """the oracle's corner rows of ONE level, [n, 8] int64 relative to the level (a one-level grid of that resolution)"""
    return O.grid_corner_rows(ul, np.asarray(offsets[l:l + 2], np.int32), 1.0, int(res[l]), 0, True, 0)[0].astype(np.int64)


def _level_weights(ul, res_l):
    """fp64 corner weights [8][n]: cell and fraction from the fp32 product u * res as in nsr_grid_locate (align_corners)"""
    pos = ul * np.float32(res_l)
    c = np.minimum(np.floor(pos), np.float32(int(res_l) - 1))
    f = (pos - c).astype(np.float64)
    for i in range(8):
        w = np.ones(len(ul), np.float64)
        for d in range(3):
            w *= f[:, d] if (i >> d) & 1 else 1.0 - f[:, d]
        yield w


def np_trilinear_scatter(O, u, live, genc, offsets, n_rows):
    """fp64 scatter of genc [M, 16, C] (d loss / d encoder output) into [n_rows, C]: cell and fraction from the fp32
    product u * res as in nsr_grid_locate (align_corners), weights and sums in fp64; rows from the oracle, one level at a
    time; one np.bincount per level, corner and channel (600 000 samples: seconds, and well under 1 GB)"""
    res = level_resolutions(O)
    sel = np.flatnonzero(live)
    ul = np.ascontiguousarray(u[sel], np.float32)
    C = genc.shape[2]
    out = np.zeros((n_rows, C), np.float64)
    for l in range(16):
        a, b = int(offsets[l]), int(offsets[l + 1])
        rows = _level_rows(O, ul, offsets, res, l)
        g = genc[sel, l].astype(np.float64)
        for i, w in enumerate(_level_weights(ul, res[l])):
            r = np.ascontiguousarray(rows[:, i])
            for ch in range(C):
                out[a:b, ch] += np.bincount(r, weights=w * g[:, ch], minlength=b - a)
    return out


def np_trilinear_scatter_add_at(O, u, live, genc, offsets, n_rows):
    """the same scatter as first written: all levels' rows at once and np.add.at.  Kept as the check of the form above."""
    pls = O.per_level_scale_from_cfg()
    res = O.grid_resolutions(16, O.grid_S(pls), 16)
    rows = O.grid_corner_rows(u, offsets, pls, 16, 0, True, 0).astype(np.int64)           # [L, M, 8]: corner i has bit d set -> +1 on axis d
    out = np.zeros((n_rows, genc.shape[2]), np.float64)
    for l in range(16):
        pos = u * np.float32(res[l])
        c = np.minimum(np.floor(pos), np.float32(int(res[l]) - 1))
        f = (pos - c).astype(np.float64)
        for i in range(8):
            w = np.ones(len(u), np.float64)
            for d in range(3):
                w *= f[:, d] if (i >> d) & 1 else 1.0 - f[:, d]
            np.add.at(out, int(offsets[l]) + rows[l, live, i], w[live, None] * genc[live, l].astype(np.float64))
    return out


def row_load(O, u, live, offsets):
    """[16]: the largest number of contributions (sample corners) one table row of the level receives"""
    res = level_resolutions(O)
    ul = np.ascontiguousarray(u[live], np.float32)
    return np.array([np.bincount(_level_rows(O, ul, offsets, res, l).reshape(-1)).max() for l in range(16)], np.int64)


# ---------------------------------------------------------------------------------------------
# the small cases (test_gpu_table_scatter_carry.py): fewer than 8 000 samples, one tile a wave
# ---------------------------------------------------------------------------------------------
def _block_points(rng, blocks):
    """1 .. 5 points inside each block (bx, by, bz), block after block, as float32 positions"""
    out = []
    for b in blocks:
        n = int(rng.integers(1, 6))
        u = (np.asarray(b, np.float64)[None, :] + 0.02 + 0.96 * rng.random((n, 3))) / 1024.0
        out.append(u * 8.0 - 6.0)
    return np.concatenate(out).astype(np.float32)


def _sites(rng, n):
    """(y, z) block coordinates of n runs inside the box, all different"""
    s = set()
    while len(s) < n:
        s.add((int(rng.integers(520, 1016)), int(rng.integers(520, 1016))))
    return sorted(s)


def _x_places(k_parity):
    """first x block of a run of four: interior, touching u = 0 (outside the box, still encoded; the order's key clamps
    there, so the walk follows the buffer), touching u = 1 (block 1023: the cell of a sample at u = 1 clamps to res - 1)"""
    return [700 + k_parity, k_parity, 1020 + k_parity]


def case_x_runs(rng):
    chunks = []
    for parity in (0, 1):
        for k in _x_places(parity):
            for (y, z) in _sites(rng, 40):
                chunks.append(_block_points(rng, [(k + i, y, z) for i in range(4) if k + i < 1024]))
    pts = np.concatenate(chunks)
    pts[-1] = [2.0, 0.37, -0.81]                                # u0 == 1 exactly: the clamped cell
    return pts


def case_gaps(rng):
    chunks = []
    for gap in (2, 5):
        for k in (640, 641, 2, 3, 1016, 1017):
            for (y, z) in _sites(rng, 40):
                chunks.append(_block_points(rng, [(k, y, z), (k + gap, y, z)]))
    return np.concatenate(chunks)


def case_morton_quad(rng):
    chunks = []
    for k in (600, 602, 0, 1022):                               # even: the four blocks are consecutive Morton keys
        for (j, z) in _sites(rng, 40):
            j &= ~1
            chunks.append(_block_points(rng, [(k, j, z), (k + 1, j, z), (k, j + 1, z), (k + 1, j + 1, z)]))
    return np.concatenate(chunks)


def case_one_block(rng, n):
    u = (np.array([733.0, 801.0, 640.0])[None, :] + 0.02 + 0.96 * rng.random((n, 3))) / 1024.0
    return (u * 8.0 - 6.0).astype(np.float32)


def case_dead_between(rng):
    """dead samples (outside the encoder's range) between two x-neighbouring blocks: at x blocks 1022 | 1023, where the
    clamped key of a dead sample equals block 1023's, and below the box, where the walk is the buffer order"""
    chunks = []
    for k in (1022, 100, 101):
        for (y, z) in _sites(rng, 50):
            a = _block_points(rng, [(k, y, z)])
            b = _block_points(rng, [(k + 1, y, z)])
            nd = int(rng.integers(1, 4))
            dead = b[:1].repeat(nd, 0).copy()
            dead[:, 0] = 2.0 + 8.0 * rng.random(nd).astype(np.float32) + 0.01      # u0 > 1; y, z of block k + 1
            chunks += [a, dead, b]
    return np.concatenate(chunks)


SYNTHETIC = {
    'x_runs': lambda: case_x_runs(np.random.default_rng(101)),
    'gaps': lambda: case_gaps(np.random.default_rng(102)),
    'morton_quad': lambda: case_morton_quad(np.random.default_rng(103)),
    'one_block': lambda: case_one_block(np.random.default_rng(104), 1500),
    'one_block_16': lambda: case_one_block(np.random.default_rng(105), 16),
    'one_block_17': lambda: case_one_block(np.random.default_rng(106), 17),
    'dead_between': lambda: case_dead_between(np.random.default_rng(107)),
}


# ---------------------------------------------------------------------------------------------
# the large cases (test_gpu_table_scatter_walk.py): two and three tiles a wave
#
# A case is a list of CHUNKS in buffer order, a chunk a list of items: a block with its number of points, or a few dead
# samples.  The chunks are the small cases' generators -- an x-run of four, two blocks 2 or 5 apart, a 2 x 2 Morton group,
# dead samples between +x neighbours -- plus pairs of neighbours along one axis whose points lie ON the face between them.
# Their places are drawn over the whole encoded range 0 .. 1023 of every axis, one coarse cell (64 blocks) after the
# other in shuffled rounds, so that no row of the coarse levels collects much more than its share.
# ---------------------------------------------------------------------------------------------
def _x_of_u(u):
    return u * 8.0 - 6.0


def _face_lo(b):
    """the position whose u is exactly b / 1024 (b / 128 - 6: exact in fp32, and so is every step of unit_of)"""
    return np.float32(b / 128.0 - 6.0)


def _f32_ord(x):
    """float32 -> an integer that orders as the floats do"""
    i = int(np.float32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _f32_of_ord(k):
    return np.array([k if k >= 0 else (-k) | 0x80000000], np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def _face_hi(b):
    """the largest fp32 position whose fp32 u still lies in block b (u == 1 itself for b = 1023: the clamped cell); found by
    bisection over the fp32 numbers below the face (the block is monotonic in the position)"""
    def block(x):
        return int(blocks_of(unit_of(np.array([[x, x, x]], np.float32)))[0, 0])
    face = np.float32((b + 1) / 128.0 - 6.0)
    if block(face) == b:
        return face
    lo, hi = _f32_ord(face - np.float32(2.0 ** -10)), _f32_ord(face)      # block(lo) == b < block(hi)
    assert block(_f32_of_ord(lo)) == b
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if block(_f32_of_ord(mid)) == b:
            lo = mid
        else:
            hi = mid
    return _f32_of_ord(lo)


class _Blk:
    def __init__(self, b, n=None, face=None):
        self.b, self.n, self.face = tuple(int(v) for v in b), n, face          # face: (axis, 'lo' | 'hi') or None

    def key_block(self):
        return self.b

    def emit(self, rng):
        u = (np.asarray(self.b, np.float64)[None, :] + 0.02 + 0.96 * rng.random((self.n, 3))) / 1024.0
        p = _x_of_u(u).astype(np.float32)
        if self.face is not None:
            d, side = self.face
            p[:, d] = _face_lo(self.b[d]) if side == 'lo' else _face_hi(self.b[d])
        return p


class _Dead:
    """n samples in block `like`, moved out of the encoder's range along `axis` (side -1: below u = 0, +1: above u = 1)"""
    def __init__(self, like, axis, side, n):
        self.like, self.axis, self.side, self.n = tuple(int(v) for v in like), axis, side, n

    def key_block(self):
        b = list(self.like)
        b[self.axis] = 0 if self.side < 0 else 1023
        return tuple(b)

    def emit(self, rng):
        u = (np.asarray(self.like, np.float64)[None, :] + 0.02 + 0.96 * rng.random((self.n, 3))) / 1024.0
        p = _x_of_u(u).astype(np.float32)
        off = (0.01 + 8.0 * rng.random(self.n)).astype(np.float32)
        p[:, self.axis] = np.float32(-6.0) - off if self.side < 0 else np.float32(2.0) + off
        return p


COARSE_LEVELS = 4


@functools.lru_cache(maxsize=None)
def _coarse_cell_rows():
    """for the coarsest levels: (resolution, rows of the level, [res, res, res, 8] corner rows of every cell), asked of the
    oracle at the cells' centres -- the grid's hash and sizes are restated nowhere here"""
    from oracle import oracle as O
    O.build()
    off, res = level_offsets(O), level_resolutions(O)
    out = []
    for l in range(COARSE_LEVELS):
        r = int(res[l])
        c = (np.arange(r) + 0.5) / r
        u = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
        out.append((r, int(off[l + 1] - off[l]), _level_rows(O, u, off, res, l).reshape(r, r, r, 8)))
    return out


class _Places:
    """Block coordinates over the whole encoded range 0 .. 1023 of every axis, with a density that evens out the load of the
    coarse table rows.  With the reference's 512 style slots every level of the grid is hashed, and on the coarse levels that
    hash is far from even: level 0 puts its 17^3 corners on 2 815 of its 4 096 rows, up to six on one, and a UNIFORM cloud of
    262 144 samples loads one row of level 0 with 3 000 contributions and one of level 1 with 1 200.  So the 32^3 cells of 32
    blocks get weights, lowered step by step wherever a cell's heaviest row on one of the four coarsest levels (resolutions 16,
    23, 33, 48) is above the aim (1 100 contributions for 262 144 samples; what is reached is about 1 260), and places are
    drawn from them 4 096 at a time by systematic sampling along the cells' Morton order, so that every neighbourhood gets
    its share in every round.  The tests count the load again with the oracle's rows."""
    F = 32
    _weights = None

    @classmethod
    def weights(cls):
        if cls._weights is not None:
            return cls._weights
        F = cls.F
        cen = (np.arange(F) + 0.5) / F
        rows = []                                                   # per level [F, F, F, 8]: the corner rows of the cell a fine cell lies in
        for r, n, cr in _coarse_cell_rows():
            c = np.minimum((cen * r).astype(np.int64), r - 1)
            rows.append((cr[c[:, None, None], c[None, :, None], c[None, None, :]], n))
        w = np.full((F, F, F), 1.0 / F ** 3)
        aim = 1100.0 / SINGLE_TILE_LIMIT
        for _ in range(60):
            f = np.ones_like(w)
            for rr, n in rows:
                load = np.bincount(rr.reshape(-1), weights=np.repeat(w.reshape(-1), 8), minlength=n)
                m = load[rr].max(axis=-1)
                f = np.minimum(f, np.where(m > aim, aim / m, 1.0))
            w = w * f
            w /= w.sum()
        g = np.arange(F, dtype=np.int64)
        key = morton_key(np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3))      # key of cell (x, y, z)
        order = np.argsort(key, kind='stable')
        cls._weights = (order, np.cumsum(w.reshape(-1)[order]))
        return cls._weights

    def __init__(self, rng):
        self.rng, self.round, self.i = rng, None, 0

    def next(self):
        K = 4096
        if self.round is None or self.i == K:
            order, cum = self.weights()
            at = (np.arange(K) + self.rng.random()) / K * cum[-1]
            cells = order[np.minimum(np.searchsorted(cum, at), order.size - 1)]
            self.round, self.i = cells[self.rng.permutation(K)], 0
        c = int(self.round[self.i])
        self.i += 1
        F = self.F
        cell = np.array([c // (F * F), (c // F) % F, c % F])
        return [int(v) for v in cell * (1024 // F) + self.rng.integers(0, 1024 // F, 3)]


def _dead_pair(rng, x, y, z, nd):
    """[A, dead, B] with B the +x neighbour of A and the dead samples' key equal to B's, so that the walk meets them in
    this order: below the box along some axis the key clamps and the dead samples leave the range downwards on that axis;
    inside the box the pair moves to the face u = 1 of one axis and they leave upwards"""
    k = min(x, 1022)
    if k >= 512:
        k &= ~1                                                     # A and B are consecutive Morton keys
    c = [k + 1, y, z]
    low = [d for d in range(3) if c[d] <= 512]
    if low:
        d, side = low[int(rng.integers(len(low)))], -1
    else:
        d, side = int(rng.integers(3)), 1
        if d == 0:
            k = 1022
        elif d == 1:
            y = 1023
        else:
            z = 1023
    return [_Blk((k, y, z)), _Dead((k + 1, y, z), d, side, nd), _Blk((k + 1, y, z))]


def _face_pair(rng, x, y, z):
    """two neighbours along one axis: the first block's points at the largest u below the face, the second's exactly on it"""
    d = int(rng.integers(3))
    a = [x, y, z]
    a[d] = min(a[d], 1022)
    b = list(a)
    b[d] += 1
    return [_Blk(a, face=(d, 'hi')), _Blk(b, face=(d, 'lo'))]


def _chunk(rng, kind, x, y, z):
    if kind == 'x_run':
        k = min(x, 1020)
        return [_Blk((k + i, y, z)) for i in range(4)]
    if kind == 'gap':
        gap = (2, 5)[int(rng.integers(2))]
        k = min(x, 1023 - gap)
        return [_Blk((k, y, z)), _Blk((k + gap, y, z))]
    if kind == 'quad':
        k, j = x & ~1, y & ~1
        return [_Blk((k, j, z)), _Blk((k + 1, j, z)), _Blk((k, j + 1, z)), _Blk((k + 1, j + 1, z))]
    if kind == 'dead_pair':
        return _dead_pair(rng, x, y, z, int(rng.integers(1, 4)))
    if kind == 'pair':
        k = min(x, 1022)
        if k >= 512:
            k &= ~1
        return [_Blk((k, y, z)), _Blk((k + 1, y, z))]
    if kind == 'face_pair':
        return _face_pair(rng, x, y, z)
    if kind == 'dead_run':
        d = int(rng.integers(3))
        return [_Dead((x, y, z), d, -1 if rng.random() < 0.5 else 1, int(rng.integers(30, 121)))]
    assert kind == 'single'
    return [_Blk((x, y, z))]


class _RowLoad:
    """Contributions per table row of the three coarsest levels, counted per chunk at its first block (a chunk is at most six
    blocks long, a cell of level 2 is 31): what the weights of _Places even out on average, this keeps from piling up by chance"""
    CAP = 1300

    def __init__(self):
        self.levels = _coarse_cell_rows()[:3]
        self.load = [np.zeros(n, np.int64) for _, n, _ in self.levels]

    def rows(self, b):
        out = []
        for r, _, cr in self.levels:
            c = [min(int((v + 0.5) / 1024.0 * r), r - 1) for v in b]
            out.append(cr[c[0], c[1], c[2]])
        return out

    def over(self, rows, n):
        """by how much n more samples there take the fullest of their rows past the cap"""
        return max(int(ld[rr].max()) for ld, rr in zip(self.load, rows)) + n - self.CAP

    def add(self, rows, n):
        for ld, rr in zip(self.load, rows):
            np.add.at(ld, rr, n)


def _chunks(rng, kinds, weights, sizes, target):
    """Chunks of the given kinds until their samples reach target.  sizes(): the numbers of points of a chunk's (up to four)
    blocks, or None where _steer_sizes chooses them later (counted as 30 a block).  No block is used twice.  A chunk tries up
    to 40 places for one that keeps its coarse rows under _RowLoad.CAP and takes the least bad otherwise."""
    places, used, chunks, total, load = _Places(rng), set(), [], 0, _RowLoad()
    weights = np.asarray(weights, np.float64) / np.sum(weights)
    while total < target:
        kind = kinds[int(rng.choice(len(kinds), p=weights))]
        nl = sizes()
        best = None
        for _ in range(40):
            items = _chunk(rng, kind, *places.next())
            blocks = [it for it in items if isinstance(it, _Blk)]
            if any(it.b in used for it in blocks):
                continue
            if not blocks:
                best = (0, items, None, 0)
                break
            live = sum(nl[:len(blocks)]) if nl is not None else 30 * len(blocks)
            rows = load.rows(blocks[0].b)
            over = load.over(rows, live)
            if best is None or over < best[0]:
                best = (over, items, rows, live)
            if over <= 0:
                break
        if best is None:
            continue
        _, items, rows, live = best
        blocks = [it for it in items if isinstance(it, _Blk)]
        if rows is not None:
            load.add(rows, live)
        used.update(it.b for it in blocks)
        if nl is not None:
            for it, n in zip(blocks, nl):
                it.n = n
        chunks.append(items)
        total += live + sum(it.n for it in items if isinstance(it, _Dead))
    return chunks


def _emit(rng, chunks, M=None):
    pts = np.concatenate([it.emit(rng) for items in chunks for it in items])
    if M is not None:
        assert pts.shape[0] >= M
        pts = pts[:M]
    return np.ascontiguousarray(pts)


def _small_blocks_case(seed, M):
    """blocks of 1 .. 5 samples, M samples; one sample in five is dead (between neighbours, and in runs of 30 .. 120 that the
    sort files wherever their clamped key belongs), which keeps the live ones near 210 000 and the fullest coarse row under
    the 1 500 contributions the tests allow (see _Places)"""
    rng = np.random.default_rng(seed)
    chunks = _chunks(rng, ('x_run', 'gap', 'quad', 'dead_pair', 'face_pair', 'dead_run'), (30, 15, 20, 20, 15, 2.2),
                     lambda: [int(v) for v in rng.integers(1, 6, 4)], M)
    return _emit(rng, chunks, M)


def _steer_sizes(rng, chunks, lo, hi, per=2, share=0.45):
    """Numbers of points for the blocks that have none yet, lo .. hi each, chosen along the WALK (items by key, stably: every
    item has one key) so that a share of the block ends -- or of the ends of the dead samples behind a block, or of their
    middles -- falls on an interior tile boundary of a launch with `per` tiles a wave.  With blocks of 20 .. 40 samples only
    one boundary in thirty would meet a block change by chance."""
    items = [it for c in chunks for it in c]
    keys = walk_key(np.array([it.key_block() for it in items], np.int64))
    order = np.argsort(keys, kind='stable')
    span = TILE * per
    p = 0
    for j, i in enumerate(order):
        it = items[i]
        if it.n is None:
            n = int(rng.integers(lo, hi + 1))
            if rng.random() < share:
                nxt = items[order[j + 1]] if j + 1 < len(order) else None
                extra = [0]
                if isinstance(nxt, _Dead):
                    extra += [nxt.n] + ([1] if nxt.n >= 2 else [])
                e = extra[int(rng.integers(len(extra)))]
                fits = [m for m in range(lo, hi + 1) if (p + m + e) % TILE == 0 and (p + m + e) % span != 0]
                if fits:
                    n = fits[int(rng.integers(len(fits)))]
            it.n = n
        p += it.n
    return p


def _long_blocks_case(seed, target):
    """blocks of 20 .. 40 samples: single blocks, +x neighbour pairs, pairs with dead samples between them; runs of dead samples
    as in the other cases"""
    rng = np.random.default_rng(seed)
    chunks = _chunks(rng, ('pair', 'dead_pair', 'single', 'dead_run'), (40, 35, 25, 16), lambda: None, target)
    _steer_sizes(rng, chunks, 20, 40)
    return _emit(rng, chunks)


def _mixed_blocks_case(seed, M):
    """blocks of 1 .. 40 samples: a chunk's blocks are all small (1 .. 5) or all of 6 .. 40.  More than half of the samples are
    DEAD, in runs of 30 .. 120: 524 311 live samples would be 4.2 M contributions to level 0's 2 815 non-empty rows, 1 490 each
    if the load were perfectly even -- the 1 500 the tests allow leave room for some 250 000 live ones (see _Places)"""
    rng = np.random.default_rng(seed)

    def sizes():
        return [int(v) for v in (rng.integers(1, 6, 4) if rng.random() < 0.65 else rng.integers(6, 41, 4))]
    chunks = _chunks(rng, ('x_run', 'gap', 'quad', 'dead_pair', 'face_pair', 'pair', 'dead_run'), (18, 7, 11, 18, 7, 11, 28), sizes, M)
    return _emit(rng, chunks, M)


TWO_TILES_M = SINGLE_TILE_LIMIT + 5
THREE_TILES_M = 2 * SINGLE_TILE_LIMIT + 16 + 7
COUNT_CAPACITY, COUNT_IN_SECOND_TILE = 300000, SINGLE_TILE_LIMIT + 16 + 9

# name -> (per, waves with a full range, with a short one, with none, samples in the last tile, its place in its wave)
EXPECTED_LAUNCH = {
    'two_tiles': (2, 8192, 1, 8191, 5, 0),
    'threshold': (1, 16384, 0, 0, 16, 0),
    'long_blocks': (2, None, None, None, None, None),
    'three_tiles': (3, 10923, 1, 5460, 7, 0),
    'count_in_second_tile': (2, 8193, 0, 8191, 9, 1),
}
WALK_CASES = tuple(sorted(EXPECTED_LAUNCH))


@functools.lru_cache(maxsize=None)
def walk_case(name):
    """-> (positions float32 [M, 3], read-only; device count): built once per process, shared by the tests"""
    if name in ('two_tiles', 'threshold'):
        pts = _small_blocks_case(201, TWO_TILES_M)
        if name == 'threshold':
            pts = np.ascontiguousarray(pts[:SINGLE_TILE_LIMIT])
        count = pts.shape[0]
    elif name == 'long_blocks':
        pts = _long_blocks_case(202, 270000)
        count = pts.shape[0]
    elif name == 'three_tiles':
        pts = _mixed_blocks_case(203, THREE_TILES_M)
        count = pts.shape[0]
    else:
        assert name == 'count_in_second_tile'
        pts = _small_blocks_case(204, COUNT_CAPACITY)
        count = COUNT_IN_SECOND_TILE
    pts.setflags(write=False)
    return pts, count
