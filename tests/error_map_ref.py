"""Reference for the error-map importance sampling (NumPy, CPU): the arithmetic include/nsr.h states for
nsr_error_map_accumulate, nsr_error_map_rebuild and nsr_draw_frame_batch_error, restated.  Integers (Python ints, uint64 arrays)
for everything that is integer; np.float32 with the stated operation order for err, its quantisation and the weights.  The
Philox is frame_batch_ref's."""
import numpy as np

from frame_batch_ref import philox, umulhi

F32 = np.float32
Q_CLAMP, ACC_SCALE, ACC_CLAMP = F32(2 ** 18), F32(2 ** 20), F32(2 ** 22)
PHILOX_CELL = 4


class Map:
    """the state of ErrorMap on the host: err [F,G] f32, acc_sum [F,G] u64, acc_cnt [F,G] u32, prefix [F,G] u64, frame_prefix [F] u64"""

    def __init__(self, F, w, h, cell=16, decay=0.05, uniform_mix=0.1, init=1.0, quant_scale=65536.0):
        self.F, self.w, self.h, self.cell = F, w, h, cell
        self.decay, self.uniform_mix, self.quant_scale = F32(decay), F32(uniform_mix), F32(quant_scale)
        self.gw, self.gh = -(-w // cell), -(-h // cell)
        self.G, self.P = self.gw * self.gh, w * h
        self.cw = np.minimum(cell, w - np.arange(self.gw) * cell)            # real extents of the cells' columns and rows
        self.ch = np.minimum(cell, h - np.arange(self.gh) * cell)
        self.npix = (self.ch[:, None] * self.cw[None, :]).reshape(-1).astype(np.uint64)
        self.err = np.full((F, self.G), init, F32)
        self.acc_sum = np.zeros((F, self.G), np.uint64)
        self.acc_cnt = np.zeros((F, self.G), np.uint32)
        rebuild(self)

    def cell_of(self, pix):
        pix = np.asarray(pix, np.int64)
        return (pix // self.w // self.cell) * self.gw + (pix % self.w) // self.cell


def quantise(err, quant_scale):
    """q = (u32) min(floor(err * quant_scale), 2^18) in fp32; NaN and negative products give 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.asarray(err, F32) * F32(quant_scale)
        ok = t >= 0                                                            # False for NaN
        return np.where(ok, np.minimum(np.floor(np.where(ok, t, 0)), Q_CLAMP), 0).astype(np.uint64)


def rebuild(m):
    """the fold of the accumulators into err, then prefix and frame_prefix from err"""
    hit = m.acc_cnt > 0
    if hit.any():
        mean = (m.acc_sum[hit].astype(np.float64) / m.acc_cnt[hit].astype(np.float64) * 2.0 ** -20).astype(F32)
        e = m.err[hit]
        d = (mean - e).astype(F32)
        step = (m.decay * d).astype(F32)
        m.err[hit] = (e + step).astype(F32)
        m.acc_sum[hit] = 0
        m.acc_cnt[hit] = 0
    m.q = quantise(m.err, m.quant_scale)
    m.mass = m.npix[None, :] * m.q
    m.prefix = np.cumsum(m.mass, axis=1, dtype=np.uint64)
    m.frame_prefix = np.cumsum(m.prefix[:, -1], dtype=np.uint64)


def accumulate(m, seg_frame, pix, ray_err, K):
    frame = np.repeat(np.asarray(seg_frame, np.int64), K)
    pix = np.asarray(pix, np.int64)
    e = np.asarray(ray_err, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        ok = (frame >= 0) & (frame < m.F) & (pix >= 0) & (pix < m.P) & (e >= 0)
        a = np.minimum(np.floor(np.where(ok, e, 0) * ACC_SCALE), ACC_CLAMP).astype(np.uint64)
    key = frame[ok] * m.G + m.cell_of(pix[ok])
    np.add.at(m.acc_sum.reshape(-1), key, a[ok])
    np.add.at(m.acc_cnt.reshape(-1), key, np.uint32(1))


def threshold(uniform_mix):
    return int(np.rint(np.float64(F32(uniform_mix)) * 2.0 ** 32))


def _weight(u, a, b, c):
    """1 / (u + (1 - u) * (a * b) / c) in fp32, in that order"""
    u, a, b, c = F32(u), np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    ab = (a * b).astype(F32)
    t = ((F32(1) - u) * ab).astype(F32)
    r = (t / c).astype(F32)
    with np.errstate(divide='ignore'):              # u = 0 and no mass: a pixel that is never drawn
        return (F32(1) / (u + r).astype(F32)).astype(F32)


def _mulhi64(hi, lo, m):
    """((hi * 2^32 + lo) * m) >> 64, elementwise; m an array of Python-int-valued entries"""
    return np.array([(((int(a) << 32) | int(b)) * int(c)) >> 64 for a, b, c in zip(hi, lo, m)], dtype=np.uint64)


def pixel_weights(m, f):
    """[P] f32: the pixel factor of every pixel of frame f"""
    total = int(m.prefix[f, -1])
    if total == 0:
        return np.ones(m.P, F32)
    g = m.cell_of(np.arange(m.P))
    return _weight(m.uniform_mix, m.q[f][g].astype(F32), F32(m.P), F32(np.uint64(total)))


def frame_weights(m):
    """[F] f32: the frame factor with frames_by_error"""
    grand = int(m.frame_prefix[-1])
    if grand == 0:
        return np.ones(m.F, F32)
    return _weight(m.uniform_mix, F32(m.F), m.prefix[:, -1].astype(F32), F32(np.uint64(grand)))


def pdf(m, f):
    """[P] f64: the probability of every pixel of frame f, given the frame"""
    total = int(m.prefix[f, -1])
    if total == 0:
        return np.full(m.P, 1.0 / m.P)
    u = float(m.uniform_mix)
    g = m.cell_of(np.arange(m.P))
    return u / m.P + (1.0 - u) * m.q[f][g].astype(np.float64) / total


def frame_pdf(m):
    grand = int(m.frame_prefix[-1])
    if grand == 0:
        return np.full(m.F, 1.0 / m.F)
    u = float(m.uniform_mix)
    return u / m.F + (1.0 - u) * m.prefix[:, -1].astype(np.float64) / grand


def draw(m, S, K, seed, seq, stream_id=0, fixed_frames=None, frames_by_error=False):
    """-> (seg_frame [S] i32, pix [S*K] i32, rows [S*K] i64, weights [S*K] f32, by_cell [S*K] bool, cell [S*K]): the four outputs
    of nsr_draw_frame_batch_error at the summed sequence `seq`, which rays took the cell branch, and every ray's cell"""
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    seq &= 0xffffffff
    t = threshold(m.uniform_mix)
    N = S * K
    wf = np.ones(S, F32)
    if fixed_frames is not None:
        seg = np.asarray(fixed_frames, np.int64)
    else:
        r = philox(np.arange(S), seq, 2, stream_id, k0, k1)
        seg = umulhi(r[0], m.F).astype(np.int64)
        grand = int(m.frame_prefix[-1])
        if frames_by_error and grand != 0:
            by_err = r[1].astype(np.int64) >= t
            target = _mulhi64(r[2], r[3], [grand] * S)
            seg = np.where(by_err, np.searchsorted(m.frame_prefix, target, side='right'), seg)
            wf = frame_weights(m)[seg]
    valid = (seg >= 0) & (seg < m.F)
    fr = np.repeat(np.where(valid, seg, 0), K)
    total = np.where(np.repeat(valid, K), m.prefix[fr, -1], 0).astype(np.uint64)
    r = philox(np.arange(N), seq, 3, stream_id, k0, k1)
    pix = umulhi(r[0], m.P).astype(np.int64)
    live = total != 0
    by_cell = live & (r[1].astype(np.int64) >= t)
    if by_cell.any():
        q = philox(np.arange(N), seq, PHILOX_CELL, stream_id, k0, k1)
        idx = np.flatnonzero(by_cell)
        target = _mulhi64(q[0][idx], q[1][idx], total[idx])
        g = np.array([np.searchsorted(m.prefix[f], x, side='right') for f, x in zip(fr[idx], target)], dtype=np.int64)
        gy, gx = g // m.gw, g % m.gw
        x = gx * m.cell + ((q[2][idx] * m.cw[gx].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        y = gy * m.cell + ((q[3][idx] * m.ch[gy].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        pix[idx] = y * m.w + x
    cell = m.cell_of(pix)
    wp = np.ones(N, F32)
    if live.any():
        i = np.flatnonzero(live)
        wp[i] = _weight(m.uniform_mix, m.q[fr[i], cell[i]].astype(F32), F32(m.P), total[i].astype(F32))
    weights = (wp * np.repeat(wf, K)).astype(F32)
    return seg.astype(np.int32), pix.astype(np.int32), fr * m.P + pix, weights, by_cell, cell
