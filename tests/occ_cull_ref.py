"""CPU restatement of the occupancy-component definition in include/nsr.h ("Occupancy components"), NumPy only, for
tests/test_occ_cull_cpu.py and tests/test_gpu_occ_cull.py.

labels_union_find(bits, C, H)     the components as a sequential union-find over the cells (plain loops over coordinates)
labels_propagation(bits, C, H)    the same definition written apart from it: on the [C, x, y, z] volume, label = min over the
                                  occupied face neighbours (array shifts), iterated to a fixed point (a pointer jump
                                  label = label[label] a round only shortens the way)
component_stats(labels, C, H), keep_rule(stats, C, H, bound, ...), cull(grid_words, bits, labels, keep, C, H)
box_case(C, H, boxes)             bitfield and labels of a grid of separate boxes, by construction: for grids too large for the two
                                  above (boxes_for(H), box_reference(H): the three-cascade layout of tests/test_gpu_occ_cull_edges.py)
plus the bitfields the tests run (cases())."""
import functools

import numpy as np


def morton(x, y, z):
    """rm_morton3d on integers or integer arrays"""
    def spread(v):
        v = np.asarray(v, np.uint64)
        out = np.zeros_like(v)
        for i in range(10):
            out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
        return out
    return (spread(x) | (spread(y) << np.uint64(1)) | (spread(z) << np.uint64(2))).astype(np.int64)


@functools.lru_cache(maxsize=None)
def cell_ids(H):
    """[H,H,H] int64: ids[ix, iy, iz] = morton(ix, iy, iz)"""
    ix, iy, iz = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing='ij')
    ids = morton(ix, iy, iz)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def cell_coords(H):
    """[H^3, 3] int64: the (ix, iy, iz) of Morton index m"""
    ids = cell_ids(H)
    out = np.zeros((H ** 3, 3), np.int64)
    ix, iy, iz = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing='ij')
    out[ids.reshape(-1)] = np.stack([ix, iy, iz], -1).reshape(-1, 3)
    out.setflags(write=False)
    return out


def occupied(bits, C, H):
    """bool [C*H^3]: bit (u & 7) of byte (u >> 3)"""
    bits = np.asarray(bits, np.uint8).reshape(-1)
    assert bits.size == C * H ** 3 // 8
    return np.unpackbits(bits, bitorder='little').astype(bool)


def pack(occ):
    """bool [cells] -> the bitfield"""
    return np.packbits(np.asarray(occ, bool), bitorder='little')


def volume(bits, C, H):
    """bool [C, H, H, H] indexed [c, ix, iy, iz]"""
    return occupied(bits, C, H).reshape(C, H ** 3)[:, cell_ids(H)]


def from_volume(vol):
    """bool [C, H, H, H] -> the bitfield"""
    C, H = vol.shape[0], vol.shape[1]
    occ = np.zeros((C, H ** 3), bool)
    occ[:, cell_ids(H).reshape(-1)] = np.asarray(vol, bool).reshape(C, -1)
    return pack(occ.reshape(-1))


def labels_union_find(bits, C, H):
    occ = occupied(bits, C, H).tolist()
    H3 = H ** 3
    parent = list(range(C * H3))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def m3(x, y, z):
        out = 0
        for i in range(10):
            out |= ((x >> i) & 1) << (3 * i) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i + 2)
        return out

    for c in range(C):
        for x in range(H):
            for y in range(H):
                for z in range(H):
                    u = c * H3 + m3(x, y, z)
                    if not occ[u]:
                        continue
                    for nx, ny, nz in ((x + 1, y, z), (x, y + 1, z), (x, y, z + 1)):
                        if nx >= H or ny >= H or nz >= H:
                            continue
                        w = c * H3 + m3(nx, ny, nz)
                        if occ[w]:
                            ru, rw = find(u), find(w)
                            if ru != rw:
                                parent[max(ru, rw)] = min(ru, rw)               # the root is the tree's smallest id
    return np.asarray([find(u) if occ[u] else -1 for u in range(C * H3)], np.int32)


def labels_propagation(bits, C, H):
    vol = volume(bits, C, H)
    H3 = H ** 3
    ids = cell_ids(H)[None] + (np.arange(C) * H3)[:, None, None, None]
    BIG = C * H3                                                                 # above every id: an unoccupied cell offers nothing
    lab = np.where(vol, ids, BIG)
    flat = np.full(C * H3 + 1, BIG, np.int64)                                    # flat[u] = label of cell u; flat[BIG] = BIG
    while True:
        new = lab.copy()
        for axis in (1, 2, 3):
            a = [slice(None)] * 4
            b = [slice(None)] * 4
            a[axis], b[axis] = slice(0, H - 1), slice(1, H)
            a, b = tuple(a), tuple(b)
            both = vol[a] & vol[b]
            new[a] = np.where(both, np.minimum(new[a], lab[b]), new[a])
            new[b] = np.where(both, np.minimum(new[b], lab[a]), new[b])
        flat[ids.reshape(-1)] = new.reshape(-1)
        new = flat[new]                                                          # the label is a cell of the component: so is its label
        if np.array_equal(new, lab):
            break
        lab = new
    out = np.full(C * H3, -1, np.int64)
    out[ids[vol]] = lab[vol]
    return out.astype(np.int32)


def own_labels(labels, C, H):
    """bool [cells]: the label is a cell of this grid.  -1 is the unoccupied cell; any other label outside 0 .. cells - 1 is not
    this grid's: the statistics count such a cell as unoccupied, and the cull leaves it as it is"""
    labels = np.asarray(labels, np.int64)
    return (labels >= 0) & (labels < C * H ** 3)


def component_stats(labels, C, H):
    """-> dict(n_cells uint32 [cells], lo, hi int32 [cells,3]): 0, H, -1 at every cell that is no root"""
    labels = np.asarray(labels, np.int64)
    cells = C * H ** 3
    occ = np.flatnonzero(own_labels(labels, C, H))
    n_cells = np.bincount(labels[occ], minlength=cells).astype(np.uint32)
    xyz = cell_coords(H)[occ % H ** 3]
    lo = np.full((cells, 3), H, np.int32)
    hi = np.full((cells, 3), -1, np.int32)
    for a in range(3):
        np.minimum.at(lo[:, a], labels[occ], xyz[:, a])
        np.maximum.at(hi[:, a], labels[occ], xyz[:, a])
    return dict(n_cells=n_cells, lo=lo, hi=hi)


def roots(labels):
    labels = np.asarray(labels, np.int64)
    return np.flatnonzero(labels == np.arange(labels.size))


def keep_rule(labels, stats, C, H, bound, min_cells=0, min_diagonal=0.0, keep_largest=None):
    """-> keep uint8 [cells], set at the roots of the kept components"""
    cells, H3 = C * H ** 3, H ** 3
    keep = np.zeros(cells, np.uint8)
    passed = []
    for r in roots(labels).tolist():
        c = r // H3
        b = min(float(2 ** c), float(bound))
        unit = 2.0 * b / float(H)
        e = (stats['hi'][r].astype(np.int64) - stats['lo'][r].astype(np.int64) + 1).astype(np.float64)
        diag2 = (unit * unit) * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        if int(stats['n_cells'][r]) >= min_cells and diag2 >= float(min_diagonal) * float(min_diagonal):
            passed.append(r)
    if keep_largest is not None:
        chosen = []
        for c in range(C):
            mine = sorted((r for r in passed if r // H3 == c), key=lambda r: (-int(stats['n_cells'][r]), r))
            chosen += mine[:keep_largest]
        passed = chosen
    keep[passed] = 1
    return keep


def cull(grid_words, bits, labels, keep, C, H):
    """-> (grid words uint32 | None, bitfield, n_culled uint32 [C]); grid_words None: the bits only"""
    labels = np.asarray(labels, np.int64)
    occ = occupied(bits, C, H)
    mine = occ & own_labels(labels, C, H)                                       # a label that is not this grid's decides nothing
    gone = mine & (np.asarray(keep)[np.where(mine, labels, 0)] == 0)
    out = None
    if grid_words is not None:
        out = np.array(grid_words, np.uint32).reshape(-1)
        out[gone] = 0xBF800000
    return out, pack(occ & ~gone), gone.reshape(C, -1).sum(1).astype(np.uint32)


def cull_floaters(grid_words, bits, C, H, bound, min_cells=0, min_diagonal=0.0, keep_largest=None):
    """the whole chain -> dict(labels, stats, keep, grid, bits, n_culled)"""
    labels = labels_propagation(bits, C, H)
    stats = component_stats(labels, C, H)
    keep = keep_rule(labels, stats, C, H, bound, min_cells, min_diagonal, keep_largest)
    grid, out_bits, n_culled = cull(grid_words, bits, labels, keep, C, H)
    return dict(labels=labels, stats=stats, keep=keep, grid=grid, bits=out_bits, n_culled=n_culled)


# ---- bitfields -------------------------------------------------------------------------------------------------------------
def from_cells(C, H, cells):
    """the bitfield with exactly the cells (c, ix, iy, iz) set"""
    vol = np.zeros((C, H, H, H), bool)
    for c, x, y, z in cells:
        vol[c, x, y, z] = True
    return from_volume(vol)


def random_fill(C, H, fill, seed):
    return pack(np.random.default_rng(seed).random(C * H ** 3) < fill)


def snake(H):
    """one cascade: a one-cell-wide path that runs along x through every second row (iy even) of every second plane (iz even),
    joined at alternating ends within a plane and by one cell of the odd plane between two planes: one component whose path is
    as long as a grid of this size allows"""
    vol = np.zeros((1, H, H, H), bool)
    end = 0                                            # the x at which the path leaves the current row
    for z in range(0, H, 2):
        ys = range(0, H, 2) if (z // 2) % 2 == 0 else range(H - 2, -1, -2)
        ys = list(ys)
        for i, y in enumerate(ys):
            vol[0, :, y, z] = True
            end = H - 1 - end
            if i + 1 < len(ys):
                vol[0, end, (y + ys[i + 1]) // 2, z] = True                     # the odd row between two rows
        if z + 2 < H:
            vol[0, end, ys[-1], z + 1] = True                                   # up to the next even plane
    return from_volume(vol)


def checkerboard(H):
    """one cascade: the cells with (x + y + z) even.  No two share a face: every occupied cell is its own root"""
    ix, iy, iz = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing='ij')
    return from_volume((((ix + iy + iz) & 1) == 0)[None])


# ---- grids too large for labels_propagation: boxes, labelled by construction ----------------------------------------------------
def box_case(C, H, boxes):
    """boxes: (c, (x0, y0, z0), (x1, y1, z1)), the cells x0 <= ix < x1, ... of cascade c; no two boxes of a cascade overlap or
    share a face (asserted), so every box is one component.  -> (bitfield, labels int32 [cells]) by construction: rm_morton3d
    grows with every coordinate, so the smallest cell id of a box is that of its corner (x0, y0, z0), and every cell of the box
    gets it.  The statistics are component_stats(labels) as for every other case.

    Time on one CPU core for boxes_for(128) (C = 3, 6 291 456 cells, 2 208 155 of them occupied, 4513 boxes): box_case 0.9 s,
    component_stats 1.2 s, keep_rule and cull 0.1 s a rule: well under the ten seconds at which the np.minimum.at of the
    statistics would have to give way to box arithmetic."""
    H3 = H ** 3
    owner = np.zeros((C, H, H, H), np.int32)                                    # 1 + the index of the box that holds the cell
    lab = np.full((C, H, H, H), -1, np.int32)
    filled = 0
    for i, (c, lo, hi) in enumerate(boxes):
        assert 0 <= c < C and all(0 <= a < b <= H for a, b in zip(lo, hi)), (c, lo, hi)
        at = (c, slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
        owner[at] = i + 1
        lab[at] = c * H3 + int(morton(*lo))
        filled += (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    assert int((owner != 0).sum()) == filled                                    # no overlap
    for axis in (1, 2, 3):                                                      # no face between two boxes
        a = [slice(None)] * 4
        b = [slice(None)] * 4
        a[axis], b[axis] = slice(0, H - 1), slice(1, H)
        p, q = owner[tuple(a)], owner[tuple(b)]
        assert not ((p != 0) & (q != 0) & (p != q)).any(), axis
    labels = np.empty((C, H3), np.int32)
    labels[:, cell_ids(H).reshape(-1)] = lab.reshape(C, -1)
    return from_volume(owner != 0), labels.reshape(-1)


def boxes_for(H):
    """three cascades, a different pattern each, scaled by H (a multiple of 32):
    0  slabs two cells thick every fourth z-plane, over all of x and y: H/4 components, and a 16 x 16 x 8 brick of cells (one
       block of the statistics and the cull) holds nothing but the cells of two of them.  The plane z = H - 1 touches no slab: it
       carries single cells at period 16 in x and 8 in y
    1  3x3x3 cubes at period 8 from coordinate 1, so that each lies across a 2x2x2 block boundary on every axis: (H/8)^3
       components.  Two of them are longer along z (4 and 5 cells), so that one of 27 cells is not the largest
    2  the half x < H/2 as one box, and single cells at period 16 in the other half: one large root and many of one cell
    The single cells of cascade 0 and the two longer cubes are there for min_cells = 28: without them that rule would cull
    nothing in cascade 0 and everything in cascade 1."""
    assert H % 32 == 0
    out = [(0, (0, 0, z), (H, H, z + 2)) for z in range(0, H, 4)]
    out += [(0, (x, y, H - 1), (x + 1, y + 1, H)) for x in range(5, H, 16) for y in range(3, H, 8)]
    for x in range(1, H, 8):
        for y in range(1, H, 8):
            for z in range(1, H, 8):
                tall = {(9, 17, 1): 4, (17, 9, 9): 5}.get((x, y, z), 3)
                out.append((1, (x, y, z), (x + 3, y + 3, z + tall)))
    out.append((2, (0, 0, 0), (H // 2, H, H)))
    out += [(2, (x, y, z), (x + 1, y + 1, z + 1)) for x in range(H // 2 + 8, H, 16) for y in range(8, H, 16) for z in range(8, H, 16)]
    return out


BOX_RULES = (dict(keep_largest=1), dict(min_cells=28))     # and min_cells = H^3 + 1, which keeps nothing


@functools.lru_cache(maxsize=None)
def box_reference(H):
    """computed once per H and shared read-only: (bitfield, labels, stats) of box_case(3, H, boxes_for(H))"""
    bits, labels = box_case(3, H, boxes_for(H))
    stats = component_stats(labels, 3, H)
    for a in (bits, labels) + tuple(stats.values()):
        a.setflags(write=False)
    return bits, labels, stats


def brick_roots(labels, brick_bytes):
    """the number of distinct roots among the cells of every run of brick_bytes bitfield bytes"""
    labels = np.asarray(labels, np.int64).reshape(-1, brick_bytes * 8)
    return np.asarray([np.unique(row[row >= 0]).size for row in labels])


# the 30 % fills: the seeds were chosen on the CPU so that every cascade has at least 20 components and one component reaches over
# more than one 2x2x2 block on every axis (tests/test_occ_cull_cpu.py asserts both)
RANDOM_16_SEED = 3
# cascades 2..7 of eight_cascades_8 and the four of four_cascades_8: chosen on the CPU so that keep_largest = 1 culls a different
# number of cells in every one of these cascades (tests/test_occ_cull_cpu.py asserts it)
EIGHT_CASCADES_SEEDS = (21, 22, 23, 24, 25, 26)
FOUR_CASCADES_SEEDS = (31, 32, 33, 34)


def hand_cells():
    """name -> (C, H, [(c, ix, iy, iz)]): the hand-checked cases"""
    out = {}
    for a, name in enumerate('xyz'):
        for lo in (0, 1, 3):                           # inside a 2x2x2 block, and across the block boundaries 1|2 and 3|4
            p, q = [5, 2, 6], [5, 2, 6]
            p[a], q[a] = lo, lo + 1
            out['pair_{}_{}'.format(name, lo)] = (1, 8, [(0, *p), (0, *q)])
    out['edge_only'] = (1, 8, [(0, 1, 1, 4), (0, 2, 2, 4)])
    out['corner_only'] = (1, 8, [(0, 1, 1, 1), (0, 2, 2, 2)])
    out['no_wrap'] = (1, 8, [(0, 0, 3, 3), (0, 7, 3, 3), (0, 4, 0, 1), (0, 4, 7, 1), (0, 2, 5, 0), (0, 2, 5, 7)])
    out['two_cascades'] = (2, 8, [(0, 3, 4, 5), (1, 3, 4, 5), (1, 4, 4, 5)])
    out['L_shape'] = (1, 8, [(0, 1, 2, 3), (0, 2, 2, 3), (0, 3, 2, 3), (0, 4, 2, 3), (0, 4, 3, 3), (0, 4, 4, 3), (0, 6, 6, 6)])
    # three components of two cells and one of three in cascade 0; two of two cells in cascade 1: ties in both
    out['ties'] = (2, 8, [(0, 0, 0, 0), (0, 1, 0, 0), (0, 4, 4, 4), (0, 5, 4, 4), (0, 0, 6, 0), (0, 0, 7, 0),
                          (0, 6, 0, 6), (0, 6, 1, 6), (0, 6, 2, 6), (1, 2, 2, 2), (1, 2, 2, 3), (1, 6, 6, 6), (1, 7, 6, 6)])
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (C, H, bitfield uint8 [C*H^3/8]): the cases of the issue"""
    out = {}
    out['empty_8'] = (1, 8, np.zeros(64, np.uint8))
    out['full_8'] = (1, 8, np.full(64, 0xFF, np.uint8))
    out['single_cell_8'] = (1, 8, from_cells(1, 8, [(0, 3, 5, 2)]))
    first_last = np.zeros(64, np.uint8)
    first_last[0], first_last[-1] = 0x01, 0x80                                  # cell 0 and cell H^3 - 1
    out['first_and_last_8'] = (1, 8, first_last)
    for name, (C, H, cells) in hand_cells().items():
        out[name] = (C, H, from_cells(C, H, cells))
    out['random_16x2'] = (2, 16, random_fill(2, 16, 0.3, RANDOM_16_SEED))
    out['snake_16'] = (1, 16, snake(16))
    out['full_32x2'] = (2, 32, np.full(2 * 32 ** 3 // 8, 0xFF, np.uint8))
    # a different pattern per cascade: 30 % random, slabs two cells thick every fourth plane, a diagonal staircase of 2x2x2 cubes
    vol = np.zeros((3, 16, 16, 16), bool)
    vol[0] = volume(random_fill(1, 16, 0.3, 11), 1, 16)[0]
    vol[1, :, :, 0::4] = True
    vol[1, :, :, 1::4] = True
    for i in range(0, 16, 2):
        vol[2, i:i + 2, i:i + 2, i:i + 2] = True
    out['three_patterns_16x3'] = (3, 16, from_volume(vol))
    # H = 8: a cascade is 64 bytes, one wave, and a block of 256 threads spans four cascades.  Cascade 0 empty, cascade 1 full
    out['eight_cascades_8'] = (8, 8, np.concatenate([np.zeros(64, np.uint8), np.full(64, 0xFF, np.uint8)] +
                                                    [random_fill(1, 8, 0.3, s) for s in EIGHT_CASCADES_SEEDS]))
    out['four_cascades_8'] = (4, 8, np.concatenate([random_fill(1, 8, 0.3, s) for s in FOUR_CASCADES_SEEDS]))      # one block exactly
    out['checkerboard_16'] = (1, 16, checkerboard(16))                          # 1024 roots in each 2048-cell brick
    for _, _, b in out.values():
        b.setflags(write=False)
    return out


# host-program cases of the issue: H = 8, C = 3; empty, full, 30 % random
def host_cases():
    return {'empty': np.zeros(3 * 64, np.uint8), 'full': np.full(3 * 64, 0xFF, np.uint8), 'random': random_fill(3, 8, 0.3, 5)}


# keep rules every case is culled with (bound 2: cascade 1's cells are twice cascade 0's)
BOUND = 2.0
RULES = (dict(), dict(min_cells=2), dict(min_cells=4), dict(keep_largest=1), dict(keep_largest=3), dict(min_diagonal=0.6),
         dict(min_cells=2, min_diagonal=0.5, keep_largest=2), dict(min_cells=10 ** 6))


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per case and shared: (labels, stats)"""
    C, H, bits = cases()[name]
    labels = labels_propagation(bits, C, H)
    stats = component_stats(labels, C, H)
    labels.setflags(write=False)
    for a in stats.values():
        a.setflags(write=False)
    return labels, stats
