"""Inputs for the tests of the table scatter's QUAD logic (csrc/table_scatter.hip): NumPy only, no GPU.

The kernel locates the four samples of steps 4q .. 4q + 3 of a 16-sample tile in one pass (lane (level, j) takes sample 4q + j)
and every step reads its record from the lane of its quad that made it; a block change inside a quad runs the pass again
against the new anchors.  Below 262 144 samples every wave walks ONE tile (table_scatter_cases.launch_model), so a batch
whose walk is its buffer order is a row of independent 16-sample cases, one wave each.  Every builder returns positions whose
blocks' keys never decrease along the buffer -- the stable sort then leaves them where they are, which tile_census()
checks from the fp32 positions with table_scatter_cases.walk_order -- and the tests read off tile_census() what each tile
puts in front of the kernel: at which steps the block changes, which steps are dead."""
import numpy as np

import table_scatter_cases as C

TILE = C.TILE
COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)
FORMS = ('plus_x', 'far', 'same_coarse')


def _points(rng, block, n):
    """n float32 positions inside a block, as table_scatter_cases._block_points places them"""
    u = (np.asarray(block, np.float64)[None, :] + 0.02 + 0.96 * rng.random((n, 3))) / 1024.0
    return (u * 8.0 - 6.0).astype(np.float32)


def _key(b):
    return int(C.walk_key(np.asarray([b], np.int64))[0])


def one_block(n, seed=301):
    """n samples of one block: counts around a quad"""
    return _points(np.random.default_rng(seed + n), (733, 801, 640), n)


def _sites(rng, n, step_y=1):
    """n places (x even, y a multiple of step_y) in the box, all different, by key"""
    s = set()
    while len(s) < n:
        s.add((int(rng.integers(260, 508)) * 2, int(rng.integers(520 // step_y + 1, 1016 // step_y)) * step_y, int(rng.integers(520, 1016))))
    return sorted(s, key=_key)


def _far_chain(rng, n):
    """n blocks in the box by key, neighbours in the chain in different cells of the coarsest level (64 blocks wide)"""
    while True:
        b = sorted({tuple(int(v) for v in rng.integers(520, 1016, 3)) for _ in range(n)}, key=_key)
        if len(b) == n and all(any(p // 64 != q // 64 for p, q in zip(b[i], b[i + 1])) for i in range(n - 1)):
            return b


def block_change(form, seed=310):
    """16 tiles; tile k: k samples of a block A, then 16 - k of a block B (k = 0: B alone -- the change in front of step 0 is
    the wave's first anchor).  plus_x: B is A's +x neighbour, x even (the shift-carry); far: another cell of the coarsest
    level (every level re-anchors, whole flush); same_coarse: the +y neighbour inside one cell of the coarsest level and
    of most coarse ones (only the finer levels re-anchor)."""
    rng = np.random.default_rng(seed + FORMS.index(form))
    if form == 'far':
        ch = _far_chain(rng, 32)
        pairs = [(ch[2 * t], ch[2 * t + 1]) for t in range(16)]
    elif form == 'plus_x':
        pairs = [(s, (s[0] + 1, s[1], s[2])) for s in _sites(rng, 16)]
    else:
        assert form == 'same_coarse'
        # y = 64 m + 2: inside a cell of the coarsest level; the tests count the levels whose cell differs
        pairs = [((x, y + 2, z), (x, y + 3, z)) for x, y, z in _sites(rng, 16, 64)]
    out = []
    for k, (a, b) in enumerate(pairs):
        out += [_points(rng, a, k), _points(rng, b, TILE - k)]
    return np.concatenate(out)


def two_changes(seed=320):
    """per quad q and (i, j) in ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3)): blocks A | B | C = (x, x + 1, x + 2), x even, with the
    changes in front of steps 4 q + i and 4 q + j (q = 0, i = 0: A is empty)"""
    rng = np.random.default_rng(seed)
    combos = [(q, i, j) for q in range(4) for (i, j) in ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))]
    out = []
    for (q, i, j), s in zip(combos, _sites(rng, len(combos))):
        s = (min(s[0], 1012), s[1], s[2])
        na, nb = 4 * q + i, j - i
        out += [_points(rng, s, na), _points(rng, (s[0] + 1, s[1], s[2]), nb), _points(rng, (s[0] + 2, s[1], s[2]), TILE - na - nb)]
    return np.concatenate(out), combos


def dead_samples(seed=330):
    """Tiles 0 .. 15: block (512, 512, 512), the box's first key, with sample p of tile p NaN (NaN quantises to block 0, which the
    order clamps to 512 -- the same key, so the stable sort leaves it in place).  Tiles 16 .. 31: block (1023, y, z) with
    sample p outside the cube (u0 > 1 quantises to 1023 as well).  Tiles 32 .. 47: p samples of (1022, y, z), one dead sample
    with the key of (1023, y, z), then that block: a dead sample directly before a block change (p = 0: first of its tile)."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(TILE):
        t = _points(rng, (512, 512, 512), TILE)
        t[p] = np.nan
        out.append(t)
    yz = sorted({(int(rng.integers(520, 1016)), int(rng.integers(520, 1016))) for _ in range(40)}, key=lambda s: _key((1022, s[0], s[1])))
    for p in range(TILE):
        t = _points(rng, (1023, yz[p][0], yz[p][1]), TILE)
        t[p, 0] = np.float32(2.0 + 0.01 + 3.0 * rng.random())
        out.append(t)
    for p in range(TILE):
        y, z = yz[TILE + p]
        t = np.concatenate([_points(rng, (1022, y, z), p), _points(rng, (1023, y, z), TILE - p)])
        t[p, 0] = np.float32(2.0 + 0.01 + 3.0 * rng.random())
        out.append(t)
    return np.concatenate(out)


def tile_census(pts, count=None):
    """per tile of the walk of pts[:count]: (dead, change) -- the steps whose sample is dead, and the live steps whose block
    differs from the tile's live sample before them (the tile's first live step is not listed: a wave has no block before it).
    Asserts that the walk is the buffer order."""
    n = pts.shape[0] if count is None else int(count)
    assert np.array_equal(C.walk_order(pts, n), np.arange(n)), 'the walk is not the buffer order'
    u = C.unit_of(pts[:n])
    live, q = C.live_of(u), C.blocks_of(u)
    out = []
    for t0 in range(0, n, TILE):
        dead, change, last = [], [], None
        for s in range(t0, min(t0 + TILE, n)):
            if not live[s]:
                dead.append(s - t0)
                continue
            b = tuple(int(v) for v in q[s])
            if last is not None and b != last:
                change.append(s - t0)
            last = b
        out.append((dead, change))
    return out


def levels_that_move(O, a, b):
    """the levels of the reference grid on which the origins of blocks a and b lie in different cells"""
    res = C.level_resolutions(O)
    ca = [np.floor(np.asarray(a, np.float64) / 1024.0 * int(r)) for r in res]
    cb = [np.floor(np.asarray(b, np.float64) / 1024.0 * int(r)) for r in res]
    return [l for l in range(16) if np.any(ca[l] != cb[l])]


# ---------------------------------------------------------------------------------------------
# the direct-to-table branch: a float32 model of the kernel's locate, same operations, nothing contracted
# ---------------------------------------------------------------------------------------------
def lattice_geometry(res):
    """(S, shift) per level: lat_geometry of csrc/lattice.h restated"""
    def corners(r, sh):
        span = int(r) << sh
        return (span // 1024 if span % 1024 == 0 else span // 1024 + 2) + 1
    out = []
    for r in res:
        sh, S = 0, corners(r, 0)
        while sh < 10 and corners(r, sh + 1) <= max(S, 3):
            sh += 1
        out.append((max(corners(r, sh), S), sh))
    return out


def past_lattice(u, res):
    """bool [n, levels]: sample n takes the direct-to-table branch on level l.  u float32 [n, 3], live."""
    u = np.asarray(u, np.float32)
    q = C.blocks_of(u)
    out = np.zeros((u.shape[0], len(res)), bool)
    for l, (r, (S, sh)) in enumerate(zip(res, lattice_geometry(res))):
        r32, cmax = np.float32(int(r)), np.float32(int(r) - 1)
        o = ((q >> sh) << sh).astype(np.float32) * np.float32(1.0 / 1024.0)
        anchor = np.minimum(np.floor(o * r32), cmax)
        c = np.minimum(np.floor(u * r32), cmax)
        out[:, l] = np.max(c - anchor, axis=1) > np.float32(S - 2)
    return out


def block_end_positions(blocks):
    """the largest fp32 position of every block on every axis at once: the end of the block, where u * res is closest to a cell
    boundary from below"""
    return np.array([[C._face_hi(int(v)) for v in b] for b in blocks], np.float32)
