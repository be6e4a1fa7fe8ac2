"""Reference for the total-variation regulariser (NumPy fp64, CPU): include/nsr.h, "Total variation", restated -- the level
table and the row function of csrc/nsr_common.h, the sweep and the Philox draws (frame_batch_ref.philox), the gradient each draw
adds with what the tests' error bound needs, the value, and the loss itself in torch for autograd."""
import numpy as np

from frame_batch_ref import philox, umulhi

M32 = np.uint64(0xffffffff)
PRIMES = (np.uint64(1), np.uint64(2654435761), np.uint64(805459861))
U2 = 2.0 ** -23


def grid_S(per_level_scale):
    return float(np.float32(np.log2(per_level_scale)))


def grid_offsets(num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners=False):
    """GridEncoder.__init__'s offsets"""
    offsets, offset = [], 0
    for i in range(num_levels):
        resolution = int(np.ceil(base_resolution * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (resolution if align_corners else resolution + 1) ** 3)
        offsets.append(offset)
        offset += int(np.ceil(n / 8) * 8)
    offsets.append(offset)
    return np.array(offsets, np.int32)


def levels(offsets, S, H, gridtype=0):
    """nsr_fill_levels: per level a dict(offset, size, res, use_hash, mul)"""
    out = []
    for l in range(len(offsets) - 1):
        size = int(offsets[l + 1] - offsets[l])
        res = int(np.floor(np.exp2(np.float32(l) * np.float32(S), dtype=np.float32) * np.float32(H)))
        stride, mul = 1, [0, 0, 0]
        for d in range(3):
            if stride > size:
                break
            mul[d] = stride
            stride = (stride * (res + 1)) & 0xffffffff
        if stride <= size:                      # the style axis
            stride = (stride * 512) & 0xffffffff
        out.append(dict(offset=int(offsets[l]), size=size, res=res, use_hash=bool(gridtype == 0 and stride > size), mul=mul))
    return out


def grid_row(lv, x, y, z):
    """nsr_grid_row at style 0 on integer arrays -> int64 rows inside the level"""
    p = [np.asarray(v, np.uint64) for v in (x, y, z)]
    if lv['use_hash']:
        index = ((p[0] * PRIMES[0]) & M32) ^ ((p[1] * PRIMES[1]) & M32) ^ ((p[2] * PRIMES[2]) & M32)
    else:
        index = (p[0] * np.uint64(lv['mul'][0]) + p[1] * np.uint64(lv['mul'][1]) + p[2] * np.uint64(lv['mul'][2])) & M32
    return (index % np.uint64(lv['size'])).astype(np.int64)


def vertex_count(lv):
    return (lv['res'] + 1) ** 3


def draws(lv, level, n_samples, seed=0, seq=0, stream_id=0):
    """-> (xyz [n_l, 3] int64, swept?) of the level's n_l = min(n_samples, V_l) draws at the summed sequence `seq`"""
    side, V = lv['res'] + 1, vertex_count(lv)
    if n_samples >= V:
        i = np.arange(V, dtype=np.int64)
        return np.stack([i % side, (i // side) % side, i // (side * side)], 1), True
    r = philox(np.arange(n_samples), seq & 0xffffffff, 5, ((stream_id << 8) | level) & 0xffffffff, seed & 0xffffffff,
               (seed >> 32) & 0xffffffff)
    return np.stack([umulhi(r[k], side).astype(np.int64) for k in range(3)], 1), False


def all_vertices(lv):
    return draws(lv, 0, vertex_count(lv))[0]


def c_factor(lam, n):
    """c_{l,k} = (float)(2.0 * lambda_k / n_l) with lambda_k the float the kernel is handed"""
    return float(np.float32(2.0 * float(np.float32(lam)) / float(n)))


def level_terms(table, lv, xyz):
    """per draw, fp64 from the table's entries [rows, lanes]: the gradient sum over the neighbours inside the lattice
    [n, lanes], sum |difference| [n, lanes], the neighbour count [n], the forward squared differences [n, lanes], the rows [n]"""
    t = np.asarray(table[lv['offset']:lv['offset'] + lv['size']], np.float64)
    row = grid_row(lv, xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ta = t[row]
    g, A, fwd, nb = np.zeros_like(ta), np.zeros_like(ta), np.zeros_like(ta), np.zeros(len(row), np.int64)
    for d in range(3):
        for s in (-1, 1):
            q = xyz.copy()
            q[:, d] += s
            ok = (q[:, d] >= 0) & (q[:, d] <= lv['res'])
            q[~ok] = xyz[~ok]
            diff = (ta - t[grid_row(lv, q[:, 0], q[:, 1], q[:, 2])]) * ok[:, None]
            g += diff
            A += np.abs(diff)
            nb += ok
            if s == 1:
                fwd += diff * diff
    return g, A, nb, fwd, row


class Grad:
    """What one call adds, per touched address: rows [m] (sorted, global), grad [m, lanes] fp64 (c and scale applied),
    k [m] the number of terms (draws) added to the row, A [m, lanes] = |c scale| * sum over the row's draws of sum |difference|."""

    def __init__(self, rows, grad, k, A):
        self.rows, self.grad, self.k, self.A = rows, grad, k, A

    def bound(self, base=None):
        """(k + 4) 2^-23 |c scale| A: per draw the kernel rounds the differences (1), their pairwise sum (each difference
        passes through at most 3 adds), scale_host * scale_dev (1), c * scale (1) and the product (1), 7 half-ulps = 3.5 x 2^-23
        relative to |c scale| sum |difference|; each of the k atomic adds rounds a running sum that is at most |c scale| A in
        magnitude, half an ulp each.  base [m, lanes]: |values the gradient held before|, which every running sum includes."""
        mag = self.A if base is None else self.A + np.abs(base)
        return (self.k[:, None] + 4) * U2 * mag

    def dense(self, n_rows):
        out = np.zeros((n_rows, self.grad.shape[1]))
        out[self.rows] = self.grad
        return out


def gradient(table, offsets, S, H, lambdas, n_samples, gridtype=0, level_mask=0xffffffff, seed=0, seq=0, stream_id=0, scale=1.0):
    """the sum of what every draw of one nsr_grid_tv call adds -> Grad.  scale: the exact product scale_host * scale_dev."""
    table = np.asarray(table)
    lanes = table.shape[1]
    rows, gs, As = [], [], []
    for l, lv in enumerate(levels(offsets, S, H, gridtype)):
        if not (level_mask >> l) & 1:
            continue
        xyz, _ = draws(lv, l, n_samples, seed, seq, stream_id)
        g, A, _, _, row = level_terms(table, lv, xyz)
        cs = np.array([c_factor(lambdas[k], len(xyz)) * float(scale) for k in range(lanes)])
        rows.append(row + lv['offset'])
        gs.append(g * cs)
        As.append(A * np.abs(cs))
    rows, gs, As = np.concatenate(rows), np.concatenate(gs), np.concatenate(As)
    uniq, inv, k = np.unique(rows, return_inverse=True, return_counts=True)
    grad, A = np.zeros((len(uniq), lanes)), np.zeros((len(uniq), lanes))
    np.add.at(grad, inv, gs)
    np.add.at(A, inv, As)
    return Grad(uniq, grad, k, A)


def add(a, b):
    """two calls' contributions to one buffer"""
    uniq = np.union1d(a.rows, b.rows)
    grad, A, k = np.zeros((len(uniq), a.grad.shape[1])), np.zeros((len(uniq), a.grad.shape[1])), np.zeros(len(uniq), np.int64)
    for part in (a, b):
        at = np.searchsorted(uniq, part.rows)
        grad[at] += part.grad
        A[at] += part.A
        k[at] += part.k
    return Grad(uniq, grad, k, A)


def value(table, offsets, S, H, lambdas, n_samples, gridtype=0, level_mask=0xffffffff, seed=0, seq=0, stream_id=0):
    """-> (value [L, lanes] fp64, n [L]): (1 / n_l) sum over the draws of the forward squared differences; 0 for lanes with
    lambda_k == 0 and masked levels"""
    table = np.asarray(table)
    lvs = levels(offsets, S, H, gridtype)
    out, n = np.zeros((len(lvs), table.shape[1])), np.zeros(len(lvs), np.int64)
    on = np.array([float(np.float32(v)) != 0.0 for v in lambdas])
    for l, lv in enumerate(lvs):
        if not (level_mask >> l) & 1:
            continue
        xyz, _ = draws(lv, l, n_samples, seed, seq, stream_id)
        out[l] = level_terms(table, lv, xyz)[3].sum(0) / len(xyz) * on
        n[l] = len(xyz)
    return out, n


def tv_loss_torch(table, offsets, S, H, lambdas, gridtype=0):
    """sum_l sum_k lambda_k TV_{l,k} of a torch fp64 table [rows, lanes] (differentiable): every edge inside the lattice once"""
    import torch
    lam = torch.tensor([float(v) for v in lambdas], dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    for lv in levels(offsets, S, H, gridtype):
        xyz = all_vertices(lv)
        ra = torch.from_numpy(grid_row(lv, xyz[:, 0], xyz[:, 1], xyz[:, 2]) + lv['offset'])
        for d in range(3):
            ok = xyz[:, d] + 1 <= lv['res']
            q = xyz[ok].copy()
            q[:, d] += 1
            rb = torch.from_numpy(grid_row(lv, q[:, 0], q[:, 1], q[:, 2]) + lv['offset'])
            diff = table[ra[torch.from_numpy(ok)]] - table[rb]
            loss = loss + ((diff * diff).sum(0) * lam).sum() / vertex_count(lv)
    return loss
