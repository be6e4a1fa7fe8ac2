"""References and seeded inputs for the inference side of csrc/raymarch_infer.hip: the single-pass composite
(nsr_composite_rays_infer), the loop step (nsr_composite_rays) and the alive-ray compaction (nsr_compact_alive).
Plain NumPy, nothing read from disk.  test_infer_composite_cpu.py proves what the builders claim, test_gpu_infer_composite.py
runs the kernels on them.

The references restate kernel_composite_rays (raymarching.cu:1133-1231) per ray, sample after sample:

    if deltas[.,0] == 0: stop                 (loop step only, :1178)
    alpha = 1 - exp(-sigma * step)            step: column 0, with is_ndc column 2
    T = 1 - weight_sum;  w = alpha * T;  weight_sum += w
    t += column 1 (with is_ndc: t_march += column 1, t += column 3);  depth += w * t;  image += w * rgb
    if T < T_thresh: stop                     (:1206, AFTER the sample that trips it)

Every ray's chain is sequential; the rays of a batch walk side by side as NumPy rows.  dtype = np.float64 is the truth (fp64
values of the fp32 inputs, np.exp); dtype = np.float32 is the same chain in the kernel's operation order and only serves to
measure how far plain fp32 sits from the truth (FLOOR below, measured by test_infer_composite_cpu.py).

Ray classes of the composite batches:
    a  transparent: every sigma 0
    b  opaque first sample: sigma * step = 200, alpha is exactly 1 in fp32 and the next T exactly 0
    c  soft: sigma in 0..60 on steps in 1e-3..5e-2, crosses T_thresh in the middle of a long run
    d  crosses exactly on its last sample: the opaque sample sits one before the last (or, for a one-slot loop step, the
       incoming weight_sum leaves T = T_thresh / 2)
    e  never crosses: density so low that T stays above 0.2.  In the T_thresh = 0 batches every ray is one, the (b) rays too
    f  loop only: terminator (deltas[.,0] == 0) in slot 0, NaN sigma, rgb and deltas behind it
    t  loop only: the terminator in a middle slot, NaN from there on
    g  single pass only: a zero step in the middle; the pass goes on, alpha = 0, t still moves by column 1
    zero, drop, keep  single pass only: no samples; offset + count == M (dropped); offset + count == M - 1 (kept)

The t columns (1 and 3), nears and incoming rays_t are multiples of 2^-10 below 16, so every t a kernel can form is exact in
fp32: rays_t has no rounding choice and is compared bit for bit.  Columns the kernels must not read (2 and 3 without NDC, all
samples no ray owns, everything behind a terminator) hold NaN.

Decision margin: a ray is redrawn while any T it tests lies within max(1e-3 * T_thresh, 2^-20) of T_thresh in fp64.  The
absolute term covers what the relative one cannot at T_thresh = 1e-4: an fp32 weight_sum near 1 has an ulp of 6e-8 and the
fast exponential moves alpha by up to 2^-21, so a T closer than a few 1e-7 to the threshold is not decided by the arithmetic
under test.  T_thresh = 0 needs no margin: alpha <= 1 keeps weight_sum <= 1 in fp32 (1 - weight_sum is exact from 0.5 on,
and fl(ws + fl(1 - ws)) rounds to 1), so T < 0 never holds.  Redraws are capped at 5 % of a batch's soft rays, or at two rays
in the batches with fewer than 40 soft rays, where 5 % is less than that; test_infer_composite_cpu.py asserts the 5 % over
all batches together (they need 0.2 %)."""
import numpy as np

F32 = np.float32
RM_BLOCK = 256
RM_MAXC = 16
SCAN_BLOCKS = 1024                                   # block totals k_scan_block_sums takes per trip
C_LIST = (1, 3, 4, 5, 8, 9, 16)
N_LIST = (1, 15, 16, 17, 63, 64, 65, 257)
N_BIG, C_BIG = 2049, (4, 8, 16)
STEP_COUNTS = (0, 1, 2, 63, 64, 65)
T_THRESHES = (1e-4, 1e-2, 0.0)
N_STEPS = (1, 2, 8, 64)
OPAQUE = 200.0
MARGIN_REL, MARGIN_ABS = 1e-3, 2.0 ** -20
EXP_ABS = 2.0 ** -21                                 # absolute error granted to the fast exponential per sample
CAP_VALUE, CAP_DEPTH = 2e-5, 2e-4                    # test_inference_march_composite_loop's bars
T_GRID = 1024.0

INFER_CLASSES = ('a', 'b', 'c', 'd', 'e', 'g', 'zero', 'drop', 'keep')
LOOP_CLASSES = ('a', 'b', 'c', 'd', 'e', 'f', 't')
SOFT = ('c', 'd', 'e', 'g', 't', 'keep')             # classes with drawn densities in front of a T test

# largest |fp32 restatement - fp64| per class over every batch of infer_cases() and loop_cases(): weights_sum and image
# absolute, depth relative to max(|depth|, 1).  Measured by test_infer_composite_cpu.py::test_fp32_floor, which fails if a
# batch exceeds them.
FLOOR = {
    'a': (0.0, 0.0), 'b': (1.2e-7, 1.3e-7), 'c': (6.7e-7, 6.7e-7), 'd': (9.3e-7, 8.8e-7), 'e': (9.5e-7, 2.3e-6), 'f': (0.0, 0.0),
    't': (7.3e-7, 6.4e-7), 'g': (3.9e-7, 6.7e-7), 'zero': (0.0, 0.0), 'drop': (0.0, 0.0), 'keep': (1.9e-7, 5.4e-7),
}


def lanes_per_ray(C):
    return 4 if C <= 4 else 8 if C <= 8 else 16


def infer_threads(N, C):
    return N * lanes_per_ray(C)


# ---- the composite chain --------------------------------------------------------------------------------------------------
def _walk(s, c, da, dt, d0, count, t, ws, d, img, T_thresh, f):
    """s, da [N, K], c [N, K, C], dt [N, K, tracks], d0 [N, K] | None (the terminator column), count [N] samples a ray owns,
    t [N, tracks], ws, d [N], img [N, C]: the state coming in.  depth steps by the last track."""
    N, K = s.shape
    s, c, da, dt = (np.asarray(a).astype(f) for a in (s, c, da, dt))
    t, ws, d, img = (np.array(a, dtype=f) for a in (t, ws, d, img))
    tt, one = f(F32(T_thresh)), f(1)
    consumed, broke = np.zeros(N, np.int64), np.zeros(N, bool)
    T_seen, w_seen = np.full((N, K), np.nan), np.zeros((N, K))
    active = count > 0
    for k in range(K):
        active = active & (k < count)
        if d0 is not None:
            z = active & (d0[:, k] == 0)
            broke |= z
            active = active & ~z
        a = np.flatnonzero(active)
        if a.size == 0:
            break
        with np.errstate(under='ignore'):
            alpha = one - np.exp(-s[a, k] * da[a, k])
        T = one - ws[a]
        w = alpha * T
        ws[a] = ws[a] + w
        t[a] = t[a] + dt[a, k]
        d[a] = d[a] + w * t[a, -1]
        img[a] = img[a] + w[:, None] * c[a, k]
        consumed[a] += 1
        T_seen[a, k], w_seen[a, k] = T, w
        stop = T < tt
        broke[a[stop]] = True
        active[a[stop]] = False
    assert ws.dtype == f and d.dtype == f and img.dtype == f and t.dtype == f
    return dict(ws=ws, d=d, img=img, t=t, consumed=consumed, broke=broke, T=T_seen, w=w_seen)


def composite_infer_ref(sig, rgb, deltas, rays, nears, M, C, T_thresh, dtype):
    """nsr_composite_rays_infer.  -> dict: weights_sum [N], depth [N], image [N, C] by ray index (a dropped or empty ray's row
    is zero), and per launch slot: live, consumed, T [N, K] (every T tested), w [N, K] (every weight added)."""
    rays = np.asarray(rays).reshape(-1, 3)
    N = len(rays)
    idx, off, cnt = (rays[:, i].astype(np.int64) for i in range(3))
    live = (cnt > 0) & (off + cnt < M)
    count = np.where(live, cnt, 0)
    K = max(int(count.max()) if N else 0, 1)
    k = np.arange(K)[None]
    pos = np.where(k < count[:, None], off[:, None] + k, 0)
    dl = np.asarray(deltas).reshape(-1, 4)[pos]
    r = _walk(np.asarray(sig)[pos], np.asarray(rgb).reshape(-1, C)[pos], dl[..., 0], dl[..., 1:2], None, count,
              np.asarray(nears)[idx][:, None], np.zeros(N), np.zeros(N), np.zeros((N, C)), T_thresh, dtype)
    out = dict(weights_sum=np.zeros(N, dtype), depth=np.zeros(N, dtype), image=np.zeros((N, C), dtype), live=live,
               consumed=r['consumed'], T=r['T'], w=r['w'])
    out['weights_sum'][idx], out['depth'][idx], out['image'][idx] = r['ws'], r['d'], r['img']
    return out


def composite_rays_ref(n_alive, n_step, rays_alive, rays_t, sig, rgb, deltas, weights_sum, depth, image, C, T_thresh, is_ndc,
                       dtype):
    """nsr_composite_rays on copies.  -> dict: rays_alive (the id kept, or -1), rays_t, weights_sum, depth, image (whole
    arrays, untouched rows as they came), and per alive slot: survived, consumed, T, w."""
    idx = np.asarray(rays_alive)[:n_alive].astype(np.int64)
    s = np.asarray(sig)[:n_alive * n_step].reshape(n_alive, n_step)
    c = np.asarray(rgb).reshape(-1, C)[:n_alive * n_step].reshape(n_alive, n_step, C)
    dl = np.asarray(deltas).reshape(-1, 4)[:n_alive * n_step].reshape(n_alive, n_step, 4)
    rt = np.array(rays_t, dtype=dtype).reshape(-1, 2 if is_ndc else 1)
    da = dl[..., 2] if is_ndc else dl[..., 0]
    dt = dl[..., [1, 3]] if is_ndc else dl[..., 1:2]
    ws, d, img = (np.array(a, dtype=dtype) for a in (weights_sum, depth, image))
    img = img.reshape(-1, C)
    r = _walk(s, c, da, dt, dl[..., 0], np.full(n_alive, n_step), rt[idx], ws[idx], d[idx], img[idx], T_thresh, dtype)
    survived = ~r['broke']
    assert (r['consumed'][survived] == n_step).all()
    alive = np.array(rays_alive, dtype=np.int32)
    alive[:n_alive] = np.where(survived, idx, -1)
    ws[idx], d[idx], img[idx] = r['ws'], r['d'], r['img']
    rt[idx[survived]] = r['t'][survived]
    return dict(rays_alive=alive, rays_t=rt.reshape(np.shape(rays_t)), weights_sum=ws, depth=d, image=img, survived=survived,
                consumed=r['consumed'], T=r['T'], w=r['w'])


def compact_ref(alive):
    alive = np.asarray(alive)
    return alive[alive >= 0]


def too_close(T, T_thresh):
    """per ray: some tested T inside the decision margin"""
    if T_thresh == 0:
        return np.zeros(len(T), bool)
    tt = float(F32(T_thresh))
    with np.errstate(invalid='ignore'):
        return (np.abs(T - tt) <= max(MARGIN_REL * tt, MARGIN_ABS)).any(1)


def bars(cls, consumed, depth64, t_max):
    """per ray: the bar on weights_sum and image (absolute) and on depth (absolute): 4 x the fp32 floor of the ray's class plus
    2^-21 per consumed sample for the fast exponential on alpha (a weight is alpha * T <= alpha, a depth term that times t <=
    t_max), capped at the bars of test_inference_march_composite_loop"""
    fv = np.array([FLOOR[c][0] for c in cls])
    fd = np.array([FLOOR[c][1] for c in cls])
    value = np.minimum(4 * fv + consumed * EXP_ABS, CAP_VALUE)
    dep = np.minimum(4 * fd * np.maximum(np.abs(depth64), 1) + consumed * EXP_ABS * t_max, CAP_DEPTH)
    return value, dep


# ---- samples of one ray -----------------------------------------------------------------------------------------------------
def _t_steps(rng, n):
    return (rng.integers(1, 65, n) / T_GRID).astype(F32)


def _ray_samples(cls, cnt, C, is_ndc, rng):
    """-> sigma [cnt], rgb [cnt, C], deltas [cnt, 4] of one ray of class cls"""
    dl = np.full((cnt, 4), np.nan, F32)
    dl[:, 1] = _t_steps(rng, cnt)
    if is_ndc:
        dl[:, 0] = rng.uniform(5, 9, cnt)                                  # non-zero and no plausible step
        dl[:, 2] = 1 - rng.uniform(0, 0.98, cnt)                           # (0, 1]
        dl[:, 3] = dl[:, 1] + _t_steps(rng, cnt)
        step, scale = dl[:, 2], 0.05
    else:
        dl[:, 0] = rng.uniform(1e-3, 5e-2, cnt)
        step, scale = dl[:, 0], 1.0
    c = rng.uniform(0, 1, (cnt, C)).astype(F32)
    hi = {'a': 0.0, 'b': 60.0, 'c': 60.0, 'd': 0.5, 'e': 0.5, 'f': 0.0, 't': 60.0, 'g': 2.0, 'drop': 60.0, 'keep': 0.5,
          'zero': 0.0}[cls]
    s = (rng.uniform(0, 1, cnt) * hi * scale).astype(F32)
    if cls == 'b':
        s[0] = F32(OPAQUE) / step[0]
    elif cls == 'd' and cnt >= 2:
        s[cnt - 2] = F32(OPAQUE) / step[cnt - 2]
    elif cls == 'g':
        dl[cnt // 2, 0] = 0
    elif cls in ('f', 't'):
        k = 0 if cls == 'f' else cnt // 2
        s[k:], c[k:], dl[k:] = np.nan, np.nan, np.nan
        dl[k, 0] = 0
    return s, c, dl


def _check_cap(redraws, n_soft):
    assert redraws <= max(2, 0.05 * n_soft), (redraws, n_soft)


def _class_list(classes, N, only, rng):
    if only is not None:
        return np.array([only] * N)
    assert N >= len(classes)
    body = [c for c in classes if c not in ('zero', 'drop', 'keep')]
    if 'zero' in classes:
        body.append('zero')
    cls = list(classes) + [body[i % len(body)] for i in range(N - len(classes))]
    return np.array(cls)[rng.permutation(N)]


# ---- single-pass batches ----------------------------------------------------------------------------------------------------
_COUNTS = {'a': (1, 2, 63, 64, 65), 'b': (2, 63, 64, 65), 'c': (65, 63, 64), 'd': (65, 2, 63, 64), 'e': (63, 1, 2, 64, 65),
           'g': (64, 65, 63), 'zero': (0,), 'drop': (1,), 'keep': (2,)}


def infer_case(C, N, T_thresh, seed=0, only=None):
    """One single-pass batch.  Launch slot n composites ray rays[n, 0], a random permutation of 0..N-1; the rays' runs lie in
    sample memory in another random order with gaps of 0..3 unowned (NaN) samples, the kept ray ends at M - 1 and the dropped
    ray owns the last sample.  only: every ray of that one class (the one-ray batch)."""
    rng = np.random.default_rng([seed, C, N, int(T_thresh * 1e6)])
    cls = _class_list(INFER_CLASSES, N, only, rng)
    seen = {}
    cnt = np.zeros(N, np.int64)
    for n, c in enumerate(cls):
        j = seen.get(c, 0)
        seen[c] = j + 1
        cnt[n] = _COUNTS[c][j % len(_COUNTS[c])]
    order = [n for n in rng.permutation(N) if cls[n] not in ('keep', 'drop')]
    order += [n for n in range(N) if cls[n] == 'keep'] + [n for n in range(N) if cls[n] == 'drop']
    off = np.zeros(N, np.int64)
    cur = int(rng.integers(0, 4))
    M = None
    for n in order:
        if cls[n] == 'drop' and M is not None:
            off[n] = M - 1
            continue
        off[n] = cur
        if cls[n] == 'keep':
            M = cur + cnt[n] + 1
            cur = M - 1
        elif cls[n] == 'drop':
            M = cur + cnt[n]
            cur = M
        else:
            cur += cnt[n] + int(rng.integers(0, 4))
    if M is None:
        M = cur + 5
    assert ((cls != 'drop') | (off + cnt == M)).all() and ((cls != 'keep') | (off + cnt == M - 1)).all()
    assert (off + cnt <= M).all()
    sig, rgb, deltas = np.full(M, np.nan, F32), np.full((M, C), np.nan, F32), np.full((M, 4), np.nan, F32)

    def fill(n):
        o, k = off[n], cnt[n]
        if cls[n] == 'drop' and (cls == 'keep').any():
            return                                                         # the kept ray's neighbour: one sample, set below
        sig[o:o + k], rgb[o:o + k], deltas[o:o + k] = _ray_samples(cls[n], k, C, False, rng)
    for n in order:
        fill(n)
    if (cls == 'drop').any() and (cls == 'keep').any():
        sig[M - 1], rgb[M - 1], deltas[M - 1] = [a[0] for a in _ray_samples('c', 1, C, False, rng)]
    rays = np.stack([rng.permutation(N), off, cnt], 1).astype(np.int32)
    nears = (rng.integers(512, 3072, N) / T_GRID).astype(F32)
    soft = np.isin(cls, SOFT)
    redraws = 0
    while True:
        ref = composite_infer_ref(sig, rgb, deltas, rays, nears, M, C, T_thresh, np.float64)
        bad = np.flatnonzero(too_close(ref['T'], T_thresh))
        if bad.size == 0:
            break
        assert soft[bad].all(), cls[bad]
        for n in bad:
            fill(n)
        redraws += bad.size
        _check_cap(redraws, int(soft.sum()))
    return dict(sig=sig, rgb=rgb, deltas=deltas, rays=rays, nears=nears, M=int(M), C=C, N=N, T_thresh=T_thresh, cls=cls,
                redraws=redraws, n_soft=int(soft.sum()), ref=ref, t_max=float(nears.max() + 65 * 64 / T_GRID))


def infer_params():
    """(C, N, T_thresh) of every single-pass batch"""
    out = []
    for C in C_LIST:
        for N in N_LIST + ((N_BIG,) if C in C_BIG else ()):
            for tt in T_THRESHES:
                out.append((C, N, tt))
    return out


def infer_batches(C, N, T_thresh):
    """the batches of one parameter set: one with every class, or for N = 1 one per class"""
    if N == 1:
        return [infer_case(C, 1, T_thresh, only=c) for c in INFER_CLASSES]
    return [infer_case(C, N, T_thresh)]


# ---- loop-step batches ------------------------------------------------------------------------------------------------------
def _loop_state(n_rays, C, is_ndc, rng):
    rt = (rng.integers(512, 3072, (n_rays, 2)) / T_GRID).astype(F32)
    rt[:, 1] = rt[:, 0] + (rng.integers(1, 512, n_rays) / T_GRID).astype(F32)
    return dict(rays_t=rt if is_ndc else rt[:, 0].copy(), weights_sum=rng.uniform(0.05, 0.5, n_rays).astype(F32),
                depth=rng.uniform(0.1, 2, n_rays).astype(F32), image=rng.uniform(0.1, 1, (n_rays, C)).astype(F32))


def loop_case(C, n_alive, n_step, is_ndc, T_thresh, seed=0, only=None, classes=LOOP_CLASSES):
    """One loop-step batch: n_alive slots over n_alive + max(3, n_alive / 4) rays, the alive ids a scrambled strict subset.
    With one slot per ray the middle terminator (t) sits in slot 0 like (f)."""
    rng = np.random.default_rng([seed, C, n_alive, n_step, int(is_ndc), int(T_thresh * 1e6)])
    cls = _class_list(classes, n_alive, only, rng)
    n_rays = n_alive + max(3, n_alive // 4)
    alive = rng.permutation(n_rays)[:n_alive].astype(np.int32)
    st = _loop_state(n_rays, C, is_ndc, rng)
    if n_step == 1 and T_thresh > 0:                                       # (d) in one slot: T = T_thresh / 2 coming in
        st['weights_sum'][alive[cls == 'd']] = F32(1 - T_thresh / 2)
    sig = np.empty((n_alive, n_step), F32)
    rgb = np.empty((n_alive, n_step, C), F32)
    deltas = np.empty((n_alive, n_step, 4), F32)

    def fill(n):
        sig[n], rgb[n], deltas[n] = _ray_samples(cls[n], n_step, C, is_ndc, rng)
    for n in range(n_alive):
        fill(n)
    soft = np.isin(cls, SOFT)
    redraws = 0
    while True:
        ref = composite_rays_ref(n_alive, n_step, alive, st['rays_t'], sig, rgb, deltas, st['weights_sum'], st['depth'],
                                 st['image'], C, T_thresh, is_ndc, np.float64)
        bad = np.flatnonzero(too_close(ref['T'], T_thresh))
        if bad.size == 0:
            break
        assert soft[bad].all(), cls[bad]
        for n in bad:
            fill(n)
        redraws += bad.size
        _check_cap(redraws, int(soft.sum()))
    t_max = float(np.max(st['rays_t']) + n_step * 128 / T_GRID)
    return dict(sig=sig.reshape(-1), rgb=rgb.reshape(-1, C), deltas=deltas.reshape(-1, 4), alive=alive, C=C, n_alive=n_alive,
                n_rays=n_rays, n_step=n_step, is_ndc=is_ndc, T_thresh=T_thresh, cls=cls, redraws=redraws,
                n_soft=int(soft.sum()), ref=ref, t_max=t_max, **st)


def loop_params():
    """(C, n_step, is_ndc, n_alive, T_thresh) of every loop-step batch: the product of the first four, T_thresh cycling so that
    every (C, n_step, is_ndc) meets each value on several batch sizes"""
    out = []
    for ic, C in enumerate(C_LIST):
        for js, n_step in enumerate(N_STEPS):
            for ndc in (False, True):
                for kn, N in enumerate(N_LIST + ((N_BIG,) if C in C_BIG else ())):
                    out.append((C, n_step, ndc, N, T_THRESHES[(ic + js + int(ndc) + kn) % 3]))
    return out


def loop_batches(C, n_step, is_ndc, n_alive, T_thresh):
    if n_alive == 1:
        return [loop_case(C, 1, n_step, is_ndc, T_thresh, only=c) for c in LOOP_CLASSES]
    return [loop_case(C, n_alive, n_step, is_ndc, T_thresh)]


CHAIN_PARAMS = [(3, 65, 2, 8, False, 1e-2), (8, 257, 8, 8, True, 1e-4), (16, 257, 1, 2, False, 1e-4), (5, 64, 2, 64, True, 0.0)]


def chain_case(C, n_alive, n1, n2, is_ndc, T_thresh, seed=0):
    """Two chained steps: `first` (n1 slots), then `sig2, rgb2, deltas2` ([n_surv * n2, ...]) for its survivors in the order the
    compaction leaves them, and the same survivors' samples concatenated (n1 + n2 slots) with the fp64 result of that one step
    from the first step's incoming state.  Margin as everywhere, on the concatenated chain."""
    first = loop_case(C, n_alive, n1, is_ndc, T_thresh, seed)
    surv = np.flatnonzero(first['ref']['survived'])
    assert 0 < surv.size < n_alive
    ids = first['alive'][surv]
    rng = np.random.default_rng([seed, 77, C, n_alive, n1, n2])
    cls2 = _class_list(LOOP_CLASSES, surv.size, None, rng)
    for attempt in range(4):
        parts = [_ray_samples(c, n2, C, is_ndc, rng) for c in cls2]
        sig2, rgb2, dl2 = (np.stack([p[i] for p in parts]) for i in range(3))
        sig_c = np.concatenate([first['sig'].reshape(n_alive, n1)[surv], sig2], 1)
        rgb_c = np.concatenate([first['rgb'].reshape(n_alive, n1, C)[surv], rgb2], 1)
        dl_c = np.concatenate([first['deltas'].reshape(n_alive, n1, 4)[surv], dl2], 1)
        ref = composite_rays_ref(surv.size, n1 + n2, ids, first['rays_t'], sig_c, rgb_c, dl_c, first['weights_sum'],
                                 first['depth'], first['image'], C, T_thresh, is_ndc, np.float64)
        if not too_close(ref['T'], T_thresh).any():
            break
    else:
        raise AssertionError('no chunk outside the decision margin')
    return dict(first=first, ids=ids, surv=surv, cls2=cls2, sig2=sig2.reshape(-1), rgb2=rgb2.reshape(-1, C), deltas2=dl2.reshape(-1, 4),
                sig_c=sig_c.reshape(-1), rgb_c=rgb_c.reshape(-1, C), deltas_c=dl_c.reshape(-1, 4), ref=ref, n2=n2,
                t_max=first['t_max'] + n2 * 128 / T_GRID)


# ---- compaction -------------------------------------------------------------------------------------------------------------
COMPACT_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 524545, 762048)
COMPACT_PATTERNS = ('all', 'none', 'alternate', 'first', 'last', 'per_block', 'dead_waves_blocks', 'rand01', 'rand50', 'rand99')
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def scan_trips(n):
    """trips of k_scan_block_sums's loop over the block totals"""
    return -(-(-(-n // RM_BLOCK)) // SCAN_BLOCKS)


def compact_keep(n, pattern, seed=0):
    i = np.arange(n)
    if pattern == 'all':
        return np.ones(n, bool)
    if pattern == 'none':
        return np.zeros(n, bool)
    if pattern == 'alternate':
        return i % 2 == 0
    if pattern == 'first':
        return i == 0
    if pattern == 'last':
        return i == n - 1
    if pattern == 'per_block':
        b = i // RM_BLOCK
        return (i % RM_BLOCK == (b * 37) % RM_BLOCK) | (i == n - 1)
    if pattern == 'dead_waves_blocks':                                     # every third wave, block 0, blocks around 1 024 and 2 048
        w, b = i // 64, i // RM_BLOCK
        dead = (w % 3 == 1) | (b == 0) | ((b >= 1020) & (b < 1028)) | ((b >= 2045) & (b < 2051))
        return ~dead
    rng = np.random.default_rng([seed, n, 5])
    return rng.uniform(0, 1, n) < {'rand01': 0.01, 'rand50': 0.5, 'rand99': 0.99}[pattern]


def compact_case(n, pattern, seed=0):
    """rays_alive [n] int32: distinct ids (0 and 2^31 - 1 among them) where the pattern keeps a ray, -1, -2 or INT32_MIN
    where it does not"""
    keep = compact_keep(n, pattern, seed)
    ids = (np.arange(n, dtype=np.int64) * 2801 + 7) % INT32_MAX            # a bijection modulo the prime 2^31 - 1
    kept = np.flatnonzero(keep)
    if kept.size >= 1:
        ids[kept[kept.size // 3]] = 0
    if kept.size >= 2:
        ids[kept[(2 * kept.size) // 3]] = INT32_MAX
    dead = np.array([-1, -2, INT32_MIN], np.int64)[np.random.default_rng([seed, n, 9]).integers(0, 3, n)]
    return np.where(keep, ids, dead).astype(np.int32)
