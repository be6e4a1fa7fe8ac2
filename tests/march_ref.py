"""Builders and bookkeeping for the march edge tests (test_march_cpu.py, test_gpu_march_edges.py), NumPy only.

This is NOT a second oracle: the sequential C restatement (oracle/raymarching_oracle.c) stays the reference for every
sample.  What is here only builds inputs and names things:

  t_sequence    the occupancy-independent parameters a ray can visit, t_{k+1} = fl(t_k + clamp(t_k dt_gamma, dt_min, dt_max)),
                by serial fp32 additions (both branches of the reference's loop advance t by exactly that expression)
  step_indices  for one ray of the oracle's output, the index k in that sequence of every sample -- the kernels handle k in
                blocks of 64 (one wave per ray) and words of 32 (sample mask), so "a sample on lane 63" is "k % 64 == 63"
  slab_scene    occupancy set by ranges of the x cell index, so that rays running along x see chosen runs and gaps
  edge_march_rays  the rays

The scene, in cells of every cascade (`u` = H / 32 cells):
  * slabs: nx in SLABS (units of u), every ny, nz -- except the anti-diagonal band |ny + nz - (H - 1)| <= 2, which the
    `diagonal` ray runs in (its y and z are opposite), so that it meets nothing on its way;
  * the far corner nx, ny >= H - max(1, H / 16), nz < max(1, H / 16) of the TOP cascade only: all the diagonal ray samples.
The slabs leave nx in [5u, 27u) empty: 69 % of a ray along x, the gap of at least 192 steps wherever bound * max_steps >= 512.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
SQRT3 = F32(1.7320508075688772)
SLABS = ((1, 2), (3, 5), (27, 28), (29, 31))          # x cell ranges in units of H / 32
LABELS = ('oblique+x', 'oblique-x', 'inner+x', 'inner-x', 'axis', 'diagonal', 'cut', 'empty', 'miss', 'behind')
N_EDGE = 769                                          # not a multiple of 4 (rays per workgroup) or 256 (scan block)
HEAVY = (255, 256, 511, 512)                          # ray indices around the 256-ray scan blocks: sample-heavy rays


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dt_limits(max_steps, C, H):
    """(dt_min, dt_max) as the kernels and the oracle compute them in fp32 (raymarching.cu:446-447)"""
    two_s3 = F32(2) * SQRT3
    return two_s3 / F32(max_steps), two_s3 * F32(1 << (C - 1)) / F32(H)


def start_t(near, noise, dt_gamma, dt_min, dt_max):
    """raymarching.cu:452: the ray's first parameter, near plus `noise` steps"""
    near = np.asarray(near, F32)
    dt = np.clip(near * F32(dt_gamma), dt_min, dt_max).astype(F32)
    return (near + (dt * np.asarray(noise, F32)).astype(F32)).astype(F32)


def t_sequence(t0, dt_gamma, dt_min, dt_max, K):
    """f32 [K + 1, ...]: t_0 = t0 and K serial fp32 additions of clamp(t * dt_gamma, dt_min, dt_max); t0 a scalar or an array
    (one sequence per element).  NumPy keeps the product and the sum as two fp32 roundings, like the kernels with
    contraction off."""
    t = np.array(t0, F32)
    out = np.empty((K + 1,) + t.shape, F32)
    out[0] = t
    g, lo, hi = F32(dt_gamma), F32(dt_min), F32(dt_max)
    for k in range(K):
        t = (t + np.minimum(hi, np.maximum(lo, t * g))).astype(F32)
        out[k + 1] = t
    return out


def step_indices(ts, ray_o, ray_d, bound, dt_gamma, dt_min, dt_max, xyz, dt):
    """The index k of each of one ray's samples in its parameter sequence `ts` [K + 1]: xyz [c, 3] and dt [c] are the oracle's
    positions and deltas[:, 0].  A sample matches k when clamp(o + t_k d) and clamp(t_k dt_gamma) equal them bit for bit;
    every sample must match exactly one k, and the indices must increase."""
    o, d, b = np.asarray(ray_o, F32), np.asarray(ray_d, F32), F32(bound)
    pos = np.clip((o[None, :] + (ts[:, None] * d[None, :]).astype(F32)).astype(F32), -b, b)
    dts = np.minimum(F32(dt_max), np.maximum(F32(dt_min), ts * F32(dt_gamma))).astype(F32)
    ax = int(np.argmax(np.abs(d)))                     # monotone along the steepest axis
    key = pos[:, ax].astype(np.float64) * (1.0 if d[ax] > 0 else -1.0)
    assert (np.diff(key) >= 0).all()
    want = np.asarray(xyz, F32)[:, ax].astype(np.float64) * (1.0 if d[ax] > 0 else -1.0)
    lo, hi = np.searchsorted(key, want, 'left'), np.searchsorted(key, want, 'right')
    assert (hi - lo == 1).all(), 'a sample position matches {} parameters'.format(sorted(set((hi - lo).tolist())))
    k = lo
    assert np.array_equal(bits(pos[k]), bits(xyz)) and np.array_equal(bits(dts[k]), bits(dt))
    assert (np.diff(k) > 0).all()
    return k.astype(np.int64)


def _expand(v):
    v = v.astype(np.uint32)
    v = (v | (v << 16)) & 0xFF0000FF
    v = (v | (v << 8)) & 0x0F00F00F
    v = (v | (v << 4)) & 0xC30C30C3
    v = (v | (v << 2)) & 0x49249249
    return v


def slab_scene(C, H, x_ranges=None):
    """u8 bitfield [C * H^3 / 8] (bit i of byte n = cell 8 n + i, cells at cascade * H^3 + morton(nx, ny, nz)): the scene of
    the module docstring; x_ranges (in cells) replaces SLABS * H / 32."""
    assert H >= 32 and H & (H - 1) == 0
    u = H // 32
    if x_ranges is None:
        x_ranges = [(a * u, b * u) for a, b in SLABS]
    i = np.arange(H)
    in_x = np.zeros(H, bool)
    for a, b in x_ranges:
        in_x[a:b] = True
    occ = np.broadcast_to(in_x[:, None, None], (H, H, H)).copy()
    occ &= (np.abs(i[None, :, None] + i[None, None, :] - (H - 1)) > 2)
    top = occ.copy()
    m = max(1, H // 16)
    top[H - m:, H - m:, :m] = True
    nx, ny, nz = np.meshgrid(i, i, i, indexing='ij')
    mort = (_expand(nx) | (_expand(ny) << 1) | (_expand(nz) << 2)).reshape(-1)
    cells = np.zeros((C, H ** 3), bool)
    for c in range(C):
        cells[c, mort] = (top if c == C - 1 else occ).reshape(-1)
    return np.packbits(cells.reshape(-1, 8)[:, ::-1], axis=1).reshape(-1)


def floats_below(edge, n):
    """the n floats just below `edge`, ascending"""
    e = int(F32(edge).view(np.uint32))
    return np.arange(e - n, e, dtype=np.uint32).view(F32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F32)


def edge_march_rays(O, bound, C, H, max_steps, seed=0, binade_edge=None):
    """-> rays_o [N, 3], rays_d [N, 3], nears [N], fars [N] (f32) and labels (list of N names), N = N_EDGE, for slab_scene(C, H).

      oblique+x / -x   from just outside the box along +-x through the slabs, y near -0.8 bound (the top cascade all the way)
      inner+x / -x     the same through the middle of the box: every cascade
      axis             two zero direction components, one of them -0.0: along +-x through the slabs, along +y inside a slab
      diagonal         from the box edge (-b, -b, 0.99 b) to (b, b, -0.99 b) with min_near = 0, so near == 0; z stops short of
                       +-bound so that an NDC march never sees z == 1 at bound 1.  Occupied at the far corner only
      cut              along the y-z diagonal (both ways) inside the slab at 29..31 u: 2.7 bound of occupied cells
      empty            along +y inside the gap of the slabs, in the top cascade
      miss             passing beside the box: near = far = FLT_MAX
      behind           the box behind the origin: far < 0 < near = min_near
      binade           (binade_edge given; 8 of the `empty` rays otherwise) along +y inside that slab, entering the box at
                       t = binade_edge - 0.01, with `near` set to the 8 floats just below binade_edge

    nears and fars are O.near_far_from_aabb's (min_near 0.2; 0 for the diagonal), except the binade rays' nears.  Rays
    HEAVY are `cut` rays.  The reference loop `do t += dt while (t < tt)` does not end for a zero direction or a `far` that
    is neither finite nor FLT_MAX, and the step-index capacity of the kernels rests on far <= 2 sqrt(3) bound: asserted."""
    rng = np.random.default_rng(seed)
    b = float(bound)
    u = 2.0 * b / 32                                   # width of a slab unit in the top cascade
    rays = []                                          # (o, d, label, min_near)

    def along_x(label, sign, y_lo, y_hi, slope):
        x0 = -sign * (b + rng.uniform(0.05, 0.45))
        o = [x0, b * rng.uniform(y_lo, y_hi), b * rng.uniform(-0.8, -0.3) if y_hi < -0.5 else b * rng.uniform(y_lo, y_hi)]
        d = _unit([sign, rng.uniform(-slope, slope), rng.uniform(-slope, slope)])
        rays.append((o, d, label, 0.2))

    n_special = 8 + 1 + 16 + 24 + 12 + 8
    n_obl = (N_EDGE - n_special - 120) // 2
    for sign, name in ((1.0, '+x'), (-1.0, '-x')):
        for _ in range(n_obl + (1 if sign > 0 and (N_EDGE - n_special - 120) % 2 else 0)):
            along_x('oblique' + name, sign, -0.85, -0.75, 0.02)
        for _ in range(60):
            along_x('inner' + name, sign, -0.35, -0.15, 0.02)
    x_slab = -b + 30.0 * u                             # the middle of the slab at 29..31 units
    x_gap = -b + 16.3 * u
    for j in range(8):
        if j < 3:
            o, d = [-(b + 0.3), -0.8 * b + 0.01 * j, -0.41 * b], np.array([1.0, 0.0, -0.0], F32)
        elif j < 6:
            o, d = [b + 0.2, -0.33 * b, -0.77 * b + 0.01 * j], np.array([-1.0, -0.0, 0.0], F32)
        else:
            o, d = [x_slab, -(b + 0.25), -0.6 * b + 0.01 * j], np.array([-0.0, 1.0, 0.0], F32)
        rays.append((o, d, 'axis', 0.2))
    rays.append(([-b, -b, 0.99 * b], _unit([1.0, 1.0, -0.99]), 'diagonal', 0.0))
    for j in range(16):
        s = 1.0 if j % 2 == 0 else -1.0                # (0, 1, 1) from the low corner, (0, -1, -1) from the high one
        back = rng.uniform(0.05, 0.25)
        d = _unit([0.0, s, 0.9 * s])                    # |z| stays below 0.95 bound: no z == 1 for NDC at bound 1
        o = np.array([x_slab + rng.uniform(-0.3, 0.3) * u, -s * b, -s * b * rng.uniform(0.85, 0.9)]) - back * d.astype(np.float64)
        rays.append((o, d, 'cut', 0.2))
    for j in range(32):
        if j >= 24 and binade_edge is not None:
            o = [x_slab, -b - (float(binade_edge) - 0.01), -0.5 * b - 0.01 * (j - 24)]
            rays.append((o, np.array([0.0, 1.0, -0.0], F32), 'binade', 0.2))
        else:
            o = [x_gap + rng.uniform(-3, 3) * u, -(b + rng.uniform(0.05, 0.4)), b * rng.uniform(-0.82, -0.74)]
            rays.append((o, _unit([rng.uniform(-0.01, 0.01), 1.0, rng.uniform(-0.02, 0.02)]), 'empty', 0.2))
    for j in range(12):
        if j < 8:
            rays.append(([-(b + 0.5), b * (1.5 + 0.05 * j), -0.3 * b], _unit([1.0, 0.05 + 0.01 * j, 0.02]), 'miss', 0.2))
        else:
            rays.append(([b * (1.5 + 0.1 * j), b * 1.7, -b * 1.3], _unit([1.0, 0.3 + 0.01 * j, -0.2]), 'behind', 0.2))
    assert len(rays) == N_EDGE, len(rays)

    # a fixed shuffle, then the `cut` rays (the most samples) onto the indices around the scan blocks
    order = list(rng.permutation(N_EDGE))
    rays = [rays[i] for i in order]
    cuts = [i for i, r in enumerate(rays) if r[2] == 'cut' and i not in HEAVY]
    for h in HEAVY:
        if rays[h][2] != 'cut':
            c = cuts.pop()
            rays[h], rays[c] = rays[c], rays[h]
    rays_o = np.array([r[0] for r in rays], F32)
    rays_d = np.array([r[1] for r in rays], F32)
    labels = [r[2] for r in rays]
    aabb = np.array([-b, -b, -b, b, b, b], F32)
    nears, fars = O.near_far_from_aabb(rays_o, rays_d, aabb, 0.2)
    diag = [i for i, l in enumerate(labels) if l == 'diagonal']
    n0, f0 = O.near_far_from_aabb(rays_o[diag], rays_d[diag], aabb, 0.0)
    nears[diag], fars[diag] = n0, f0
    if binade_edge is not None:
        bn = [i for i, l in enumerate(labels) if l == 'binade']
        assert (nears[bn] < floats_below(binade_edge, 8)[0]).all()          # the chosen starts are inside the box
        nears[bn] = floats_below(binade_edge, 8)
    check_safe(rays_o, rays_d, nears, fars, bound)
    return rays_o, rays_d, nears, fars, labels


def check_safe(rays_o, rays_d, nears, fars, bound):
    """what the sequential reference needs to terminate and the kernels' step capacity rests on (see edge_march_rays)"""
    assert np.isfinite(rays_o).all() and np.isfinite(rays_d).all() and np.isfinite(nears).all() and np.isfinite(fars).all()
    assert (np.abs(rays_d).max(1) >= 0.1).all()
    flat = rays_d == 0
    assert (np.abs(rays_o)[flat] < bound).all()
    miss = (nears == FLT_MAX) & (fars == FLT_MAX)
    assert ((fars <= 2 * np.sqrt(3.0) * bound) | miss).all() and (nears >= 0).all()


def runs_crossing(k, period):
    """whether two consecutive step indices k, k + 1 are both samples with k + 1 a multiple of `period`"""
    k = np.asarray(k)
    return bool(((np.diff(k) == 1) & (k[1:] % period == 0)).any())


# ---- the configurations the GPU file runs (test_march_cpu.py proves the edge conditions for every one) ---------------------
# (route, bound, C, H, max_steps, dt_gamma, binade_edge).  Routes: 'replay' wave per ray with recorded blocks (N = 769),
# 'remarch' wave per ray with slot capacity 0 (bound * max_steps + 96 step indices need more than 64 records), 'mask' thread
# per ray (N = 20 481, the 769 rays tiled), 'ndc' (N = 769).
G = 1.0 / 64
CASES = [
    ('replay', 1.0, 1, 32, 1028, 0.0, 1.0),          # binade case: block starts just below 1.0
    ('replay', 1.5, 2, 64, 514, 0.0, 2.0),           # binade case: just below 2.0
    ('replay', 2.0, 2, 128, 1024, 0.0, 2.0),         # the control: a power of two has no tie
    ('replay', 4.0, 3, 64, 514, G, None),
    ('replay', 8.0, 4, 32, 64, 0.0, None),
    ('remarch', 4.0, 3, 64, 1024, 0.0, None),        # the smallest max_steps with slot capacity 0 at bound 4 ...
    ('remarch', 1.0, 1, 32, 4096, 0.0, None),        # ... and at bound 1
    ('remarch', 8.0, 4, 32, 514, G, None),
    ('remarch', 1.5, 2, 64, 4096, 0.0, None),
    ('remarch', 2.0, 2, 128, 4096, 0.0, None),
    ('mask', 1.0, 1, 32, 514, 0.0, None),
    ('mask', 1.5, 2, 64, 514, 0.0, 2.0),             # binade case
    ('mask', 2.0, 2, 128, 514, G, None),
    ('mask', 4.0, 3, 64, 64, 0.0, None),
    ('mask', 8.0, 4, 32, 64, 0.0, None),
    ('mask', 1.0, 1, 32, 1028, 0.0, 1.0),            # binade case
    ('mask', 1.0, 1, 32, 1024, 0.0, 1.0),            # control
    ('ndc', 1.0, 1, 32, 1024, 0.0, None),
    ('ndc', 1.5, 2, 64, 1028, G, None),
    ('ndc', 2.0, 2, 128, 514, 0.0, None),
    ('ndc', 4.0, 3, 64, 64, 0.0, None),
    ('ndc', 8.0, 4, 32, 1024, 0.0, None),
]
N_MASK = 20481                                        # the first batch size past the wave-per-ray limit of 20 480


def case_id(case):
    return '{}-b{:g}-C{}-H{}-s{}-g{:g}{}'.format(*case[:6], '' if case[6] is None else '-edge{:g}'.format(case[6]))


def step_capacity(bound, max_steps):
    """the step indices a ray can reach: far <= 2 sqrt(3) bound in steps of at least 2 sqrt(3) / max_steps, plus slack"""
    return int(np.ceil(max(bound, 1.0) * max_steps)) + 96


_cache = {}


def case_inputs(O, case):
    """bitfield, rays_o, rays_d, nears, fars, labels, z_hats of a case's 769 base rays; cached, treat as read-only"""
    key = case[1:]
    if key not in _cache:
        _, bound, C, H, max_steps, _, edge = case
        ro, rd, ne, fa, labels = edge_march_rays(O, bound, C, H, max_steps, binade_edge=edge)
        z_hats = np.random.default_rng(7).uniform(0.5, 2.0, len(ro)).astype(F32)
        _cache[key] = (slab_scene(C, H), ro, rd, ne, fa, labels, z_hats)
    return _cache[key]


def edge_noises(n, seed=3):
    """0, 0.5, the float below 1 and uniform random values, interleaved"""
    r = np.random.default_rng(seed).random(n).astype(F32)
    r[0::4], r[1::4], r[2::4] = 0.0, 0.5, np.nextafter(F32(1), F32(0))
    return r
