"""CPU model: how many gradient records / atomic requests per sample the table scatter of the field backward needs when
the samples of a DENSE ray batch (a full frame: neighbouring pixels) are processed (a) in ray order, as round 1 does,
or (b) in Morton order of their finest-level cell with a per-wave, per-level LDS lattice tile that accumulates the
corner gradients of T^3 cells and is flushed (one record per touched corner) when the wave's sample stream leaves
the tile.  Analysis tool only (uses oracle/ for marching); not imported by the product.

usage: python tools/sorted_scatter_sim.py [patch_edge_px=96] [samples_per_wave=47000]

`python tools/sorted_scatter_sim.py lattice [patch_edge_px=96] [x0=400] [y0=300] [samples_per_wave=2976]` models the shipped
kernel instead (table_scatter.hip: 10-bit block keys, per-level lattices anchored at the block or block group, flushes of
the touched corners 16 slots per atomic instruction) and counts 64-byte atomic requests per sample and level under
  (a)  a re-anchor flushes the whole lattice (the kernel before the shift-carry), with the old 16-consecutive-slots
       instruction groups and with groups of whole x-rows;
  (b)  x-carry: an anchor that moved by 0 < d <= S - 1 cells along +x only flushes the planes x < d, the rest stays;
  (c)  the same on whichever single axis moved.
A wave walks `samples_per_wave` consecutive samples (the bench frame: 48.6 M samples over 16 384 waves = 186 tiles) and
flushes everything at its end.  Not modelled: samples whose gradient is zero (they touch nothing), the rays outside
the patch that share its blocks, and the order in which the memory side sees the requests.

`python tools/sorted_scatter_sim.py gather [patch_edge_px=64] [tile_stride=4] [tiles_per_workgroup=1483]` models the forward's
lattice gather (field.hip, k_field_fwd_lat) with the same geometry on a 5 x 3 grid of dense patches over the frame: a wave
takes every `tile_stride`-th 16-sample tile of its workgroup's run, anchors every level at the block (group) of the tile's
first sample and refills a level's S^3 lattice of table rows when that anchor differs from the one it holds.  Per level and in
all: (a) rows fetched by fills per sample, (b) the share of (sample, level) pairs whose cell lies inside the lattice, (c) fills
per tile."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
from oracle import oracle as O
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid


def dense_patch_samples(edge=96, x0=400, y0=300):
    poses, intr, _ = load_room_cameras(2)
    ys, xs = np.meshgrid(np.arange(y0, y0 + edge), np.arange(x0, x0 + edge), indexing='ij')
    pix = (ys * intr.w + xs).reshape(-1)
    o, d = O.generate_rays(poses[0], intr.w, intr.h, intr.fx, intr.fy, intr.cx, intr.cy, 3, pix_indices=pix)[:2]
    grid = synthetic_density_grid(2.0, 128, n_boxes=28, seed=0)
    bits = O.packbits(grid, 0.5)
    nears, fars = O.near_far_from_aabb(o, d, np.array([-2, -2, -2, 2, 2, 2], np.float32), 0.2)
    xyzs, _, _, rays, cnt = O.march_rays_train(o, d, 2.0, bits, 2, 128, nears, fars, max_steps=1024)
    return xyzs[:int(cnt[0])], rays


def morton3(c):
    def spread(v):
        v = v.astype(np.uint64)
        v = (v | (v << 32)) & 0x1F00000000FFFF
        v = (v | (v << 16)) & 0x1F0000FF0000FF
        v = (v | (v << 8)) & 0x100F00F00F00F00F
        v = (v | (v << 4)) & 0x10C30C30C30C30C3
        v = (v | (v << 2)) & 0x1249249249249249
        return v
    return spread(c[:, 0]) | (spread(c[:, 1]) << 1) | (spread(c[:, 2]) << 2)


def level_cells(u, res):
    pos = u * np.float32(res)
    c = np.minimum(np.floor(pos), res - 1).astype(np.int64)
    return c


def lines_of(rows_sorted_by_emit):
    """requests of a record stream drained 16 per instruction under the measured merge rule"""
    n = len(rows_sorted_by_emit) // 16 * 16
    if n == 0:
        return 0
    s = rows_sorted_by_emit[:n].reshape(-1, 16)
    line = s >> 2
    # distinct lines per instruction (duplicates of the same row within an instruction are rare after merging)
    srt = np.sort(line, axis=1)
    return int((np.diff(srt, axis=1) != 0).sum() + len(srt))


def hash_row(cx, cy, cz, size, offset):
    idx = (cx.astype(np.uint64) ^ (cy.astype(np.uint64) * 2654435761 & 0xFFFFFFFF) ^ (cz.astype(np.uint64) * 805459861 & 0xFFFFFFFF)) & 0xFFFFFFFF
    return (idx % size).astype(np.int64) + offset


def lat_corners(res, shift):
    span, blocks = int(res) << shift, 1024
    cells = span // blocks if span % blocks == 0 else span // blocks + 2
    return cells + 1


def lat_geometry(res):
    """table_scatter.hip lat_geometry: (corners per axis, anchor group shift) per level"""
    out = []
    for r in res:
        shift, S = 0, lat_corners(r, 0)
        while shift < 10 and lat_corners(r, shift + 1) <= max(S, 3):
            shift += 1
        out.append((max(lat_corners(r, shift), S), shift))
    return out


def count_requests(masks, anchors, S, size, offset, rows_per_group):
    """masks [n, S^3] bool (slot = (z * S + y) * S + x), anchors [n, 3]: requests when every event's flagged slots leave
    `rows_per_group` x-rows (None: 16 consecutive slots) per atomic instruction; distinct 64-byte lines per instruction"""
    if len(masks) == 0:
        return 0
    masks, anchors = np.asarray(masks), np.asarray(anchors, np.int64)
    k = np.arange(S ** 3)
    x, y, z = k % S, (k // S) % S, k // (S * S)
    rows = hash_row(anchors[:, None, 0] + x[None], anchors[:, None, 1] + y[None], anchors[:, None, 2] + z[None], size, offset)
    line = np.where(masks, rows >> 2, -1)
    g = 16 if rows_per_group is None else rows_per_group * S
    total = 0
    for s0 in range(0, S ** 3, g):
        sub = np.sort(line[:, s0:s0 + g], axis=1)
        total += int(((np.diff(sub, axis=1) != 0) & (sub[:, 1:] >= 0)).sum() + (sub[:, 0] >= 0).sum())
    return total


def lattice_model(u, spw):
    """requests per sample and level under the rules (a) old groups, (a) row groups, (b), (c)"""
    pls = O.per_level_scale_from_cfg()
    off = O.grid_offsets(16, pls, 16, 19)
    res = [int(r) for r in O.grid_resolutions(16, O.grid_S(pls), 16)]
    geom = lat_geometry(res)
    M = len(u)
    q = np.clip(np.floor(u * np.float32(1024)), 0, 1023).astype(np.int64)
    order = np.argsort(morton3(np.maximum(q - 512, 0)), kind='stable')
    u, q = u[order], q[order]
    wave = np.arange(M) // spw
    corners = np.array([[(i >> d) & 1 for d in range(3)] for i in range(8)], np.int64)
    table = []
    for l in range(16):
        S, shift = geom[l]
        NC, size, offset = S ** 3, int(off[l + 1] - off[l]), int(off[l])
        o = ((q >> shift) << shift).astype(np.float32) * np.float32(1.0 / 1024)
        anchor = np.minimum(np.floor(o * np.float32(res[l])), res[l] - 1).astype(np.int64)
        rel = level_cells(u, res[l]) - anchor
        direct = (rel > S - 2).any(1)                       # fp32 rounding: one cell past the lattice -> straight to the table
        rel = np.minimum(rel, S - 2)
        change = np.r_[True, (np.diff(anchor, axis=0) != 0).any(1) | (np.diff(wave) != 0)]
        seg = np.cumsum(change) - 1
        nseg = int(seg[-1]) + 1
        touched = np.zeros((nseg, NC), bool)
        cc = rel[:, None, :] + corners[None]
        slot = (cc[:, :, 2] * S + cc[:, :, 1]) * S + cc[:, :, 0]
        live = ~direct
        touched[np.repeat(seg[live], 8), slot[live].reshape(-1)] = True
        first = np.flatnonzero(change)
        sa, sw = anchor[first], wave[first]
        # 8 atomic instructions (two x corners x four components) of 4 lanes with different (y, z) rows each
        extra = 32 * int(direct.sum())
        row = {'S': S, 'shift': shift, 'direct': float(direct.mean())}
        row['a_old'] = (count_requests(touched, sa, S, size, offset, None) + extra) / M
        row['a_rows'] = (count_requests(touched, sa, S, size, offset, 16 // S) + extra) / M
        for rule in ('b', 'c'):
            ev_m, ev_a = [], []
            T = np.zeros((S, S, S), bool)                   # [z, y, x]
            for i in range(nseg):
                if i > 0:
                    d = sa[i] - sa[i - 1]
                    ax = np.flatnonzero(d)
                    carry = sw[i] == sw[i - 1] and len(ax) == 1 and 0 < d[ax[0]] <= S - 1 and (rule == 'c' or ax[0] == 0)
                    if carry:
                        a, n = 2 - int(ax[0]), int(d[ax[0]])   # array axis of the moving coordinate
                        out = np.zeros_like(T)
                        sl = [slice(None)] * 3
                        sl[a] = slice(0, n)
                        out[tuple(sl)] = T[tuple(sl)]
                        T = np.roll(T, -n, axis=a)
                        sl[a] = slice(S - n, S)
                        T[tuple(sl)] = False
                    else:
                        out, T = T, np.zeros((S, S, S), bool)
                    if out.any():
                        ev_m.append(out.reshape(-1))
                        ev_a.append(sa[i - 1])
                T = T | touched[i].reshape(S, S, S)
            ev_m.append(T.reshape(-1))
            ev_a.append(sa[-1])
            row[rule] = (count_requests(ev_m, ev_a, S, size, offset, 16 // S) + extra) / M
        table.append(row)
        print('level %2d res %4d S %d shift %d  segments/sample %.3f  (a) %.3f  (a, row groups) %.3f  (b) %.3f  (c) %.3f   direct %.1e'
              % (l, res[l], S, shift, nseg / M, row['a_old'], row['a_rows'], row['b'], row['c'], row['direct']), flush=True)
    return table


def main_lattice(argv):
    edge = int(argv[0]) if len(argv) > 0 else 96
    x0, y0 = (int(argv[1]) if len(argv) > 1 else 400), (int(argv[2]) if len(argv) > 2 else 300)
    spw = int(argv[3]) if len(argv) > 3 else 2976
    xyz, _ = dense_patch_samples(edge, x0, y0)
    u = O.encoder_inputs(xyz, 2.0).astype(np.float32)
    print('rays', edge * edge, 'samples', len(u), 'per ray %.1f' % (len(u) / edge / edge), 'samples per wave', spw)
    t = lattice_model(u, spw)
    print('| level | res | S | (a) today | (a) whole x-rows per instruction | (b) x-carry | (c) any-axis carry |')
    print('|---|---|---|---|---|---|---|')
    for l, r in enumerate(t):
        print('| %d | | %d | %.3f | %.3f | %.3f | %.3f |' % (l, r['S'], r['a_old'], r['a_rows'], r['b'], r['c']))
    tot = {k: sum(r[k] for r in t) for k in ('a_old', 'a_rows', 'b', 'c')}
    print('| all | | | %.2f | %.2f | %.2f | %.2f |' % (tot['a_old'], tot['a_rows'], tot['b'], tot['c']))
    print('(c) takes a further %.1f %% of the requests (b) leaves' % (100 * (tot['b'] - tot['c']) / tot['b']))


def gather_model(u, stride, tpb):
    """per level: [rows fetched by fills, (sample, level) pairs inside the lattice, fills], and the tile count"""
    pls = O.per_level_scale_from_cfg()
    res = [int(r) for r in O.grid_resolutions(16, O.grid_S(pls), 16)]
    geom = lat_geometry(res)
    M = len(u)
    q = np.clip(np.floor(u * np.float32(1024)), 0, 1023).astype(np.int64)
    order = np.argsort(morton3(np.maximum(q - 512, 0)), kind='stable')
    u, q = u[order], q[order]
    nt = (M + 15) // 16
    tile_of = np.arange(M) // 16
    first = np.arange(nt) * 16                                  # every marched sample is live
    # the tile a wave handled before tile t: t - stride inside the same workgroup run, none at its start
    t = np.arange(nt)
    prev = np.where((t % tpb) >= stride, t - stride, -1)
    out = np.zeros((16, 3))
    for l in range(16):
        S, shift = geom[l]
        o = ((q[first] >> shift) << shift).astype(np.float32) * np.float32(1.0 / 1024)
        anchor = np.minimum(np.floor(o * np.float32(res[l])), res[l] - 1).astype(np.int64)       # [nt, 3]
        fill = (prev < 0) | (anchor != anchor[np.maximum(prev, 0)]).any(1)
        rel = level_cells(u, res[l]) - anchor[tile_of]
        inside = ((rel >= 0) & (rel < S - 1)).all(1)
        out[l] = [fill.sum() * S ** 3, inside.sum(), fill.sum()]
    return out, nt, M, geom, res


def main_gather(argv):
    edge = int(argv[0]) if len(argv) > 0 else 64
    stride = int(argv[1]) if len(argv) > 1 else 4
    tpb = int(argv[2]) if len(argv) > 2 else 1483
    tot, ntiles, samples, geom, res = np.zeros((16, 3)), 0, 0, None, None
    for j in range(3):
        for i in range(5):
            xyz, _ = dense_patch_samples(edge, (1008 - edge) * i // 4, (756 - edge) * j // 2)
            if len(xyz) < 16:
                continue
            t, nt, M, geom, res = gather_model(O.encoder_inputs(xyz, 2.0).astype(np.float32), stride, tpb)
            tot, ntiles, samples = tot + t, ntiles + nt, samples + M
    print('patches of %d^2 rays, %d samples, %d tiles, tile stride %d, %d tiles per workgroup' % (edge, samples, ntiles, stride, tpb))
    print('| level | res | S | shift | (a) rows fetched by fills / sample | (b) inside the lattice | (c) fills / tile |')
    print('|---|---|---|---|---|---|---|')
    for l in range(16):
        print('| %d | %d | %d | %d | %.3f | %.4f | %.4f |' % (l, res[l], geom[l][0], geom[l][1], tot[l, 0] / samples, tot[l, 1] / samples,
                                                            tot[l, 2] / ntiles))
    for name, lv in (('0-7', range(8)), ('8-11', range(8, 12)), ('12-15', range(12, 16)), ('all', range(16))):
        lv = list(lv)
        print('| %s | | | | %.3f | %.4f | %.4f |' % (name, tot[lv, 0].sum() / samples, tot[lv, 1].sum() / samples / len(lv),
                                                   tot[lv, 2].sum() / ntiles))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'gather':
        return main_gather(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == 'lattice':
        return main_lattice(sys.argv[2:])
    edge = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    spw = int(sys.argv[2]) if len(sys.argv) > 2 else 47000
    xyz, rays = dense_patch_samples(edge, int(sys.argv[3]) if len(sys.argv) > 3 else 0, int(sys.argv[4]) if len(sys.argv) > 4 else 0)
    M = len(xyz)
    u = O.encoder_inputs(xyz, 2.0).astype(np.float32)
    pls = O.per_level_scale_from_cfg()
    off = O.grid_offsets(16, pls, 16, 19)
    res = O.grid_resolutions(16, O.grid_S(pls), 16)
    print('rays', edge * edge, 'samples', M, 'per ray', M / edge / edge)
    fin = level_cells(u, int(res[15]))
    key = morton3(fin - fin.min(0))
    order = np.argsort(key, kind='stable')
    corners = np.array([[(i >> d) & 1 for d in range(3)] for i in range(8)], np.int64)
    tot = {}
    for name, perm in (('ray order', np.arange(M)), ('morton order', order)):
        for T in ((None, 2, 3, 4) if name == 'morton order' else (None,)):
            rec_total, req_total, low_total = 0, 0, 0
            per_level = []
            for l in range(16):
                c = level_cells(u[perm], int(res[l]))
                size = int(off[l + 1] - off[l])
                wave = np.arange(M) // spw
                if T is None:
                    # run tracker: a record per corner stream whenever the cell changes (merges only same-cell runs;
                    # the real tracker also hands runs over to the neighbouring cell: slightly optimistic/pessimistic either way)
                    change = np.r_[True, (np.diff(c, axis=0) != 0).any(1) | (np.diff(wave) != 0)]
                    seg = np.cumsum(change) - 1
                else:
                    tile = c // T
                    change = np.r_[True, (np.diff(tile, axis=0) != 0).any(1) | (np.diff(wave) != 0)]
                    seg = np.cumsum(change) - 1
                # distinct corners per segment
                cc = (c[:, None, :] + corners[None]).reshape(-1, 3)
                sg = np.repeat(seg, 8)
                k = ((sg * 4099 + cc[:, 2]) * 4099 + cc[:, 1]) * 4099 + cc[:, 0]
                uk, first = np.unique(k, return_index=True)
                rec = len(uk)
                # emit order: by segment, then z, y, x (x fastest) -> rows
                cz = (uk // 1) % 4099
                rows = hash_row(uk % 4099, (uk // 4099) % 4099, (uk // 4099 ** 2) % 4099, size, int(off[l]))
                req = lines_of(rows)
                low = len(np.unique(hash_row(cc[:, 0], cc[:, 1], cc[:, 2], size, int(off[l]))))
                rec_total += rec
                req_total += req
                low_total += low
                per_level.append((rec / M, req / M, low / M))
            tag = '{} / {}'.format(name, 'run tracker' if T is None else 'LDS tile T={} ({} corners x 16 levels = {:.1f} KB/wave)'.format(T, (T + 1) ** 3, (T + 1) ** 3 * 16 * 16 / 1024))
            print('%-78s records/sample %6.2f  requests/sample %6.2f  (distinct rows/sample %.3f)' % (tag, rec_total / M, req_total / M, low_total / M))
            print('    per level records: ' + ' '.join('%.2f' % p[0] for p in per_level))


if __name__ == '__main__':
    main()
