"""The optimiser kernels (csrc/optim.hip) and nsr_cast_f32_to_f16 (csrc/gridenc.hip) called directly through the C ABI and compared
with the fp64 restatement and the derived bounds of tests/optim_ref.py, at the shapes where elementwise kernels go wrong: scalar
tails, one element, a grid-stride trip past the 2048-block cap, every element mask, ranges that start and end inside a block.

Every buffer of a case lives in ONE device allocation (Arena) with at least 64 elements of a canary pattern on each side of it,
and every case compares the whole allocation outside the buffers with the canary: a write past an end is caught by comparison.
Nothing is launched with a pointer or a size the entry point would not accept.  Each step's reference starts from the kernel's
own previous outputs, so bounds do not compound.  The tests print the largest observed share of each derived bound (-s shows it).
"""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

NSR_OK = 0
CANARY = 0x5A695A69                 # both halves 0x5A69: the same pattern in a float (1.6e16) and in a half (205.1) buffer
CANARY16 = 0x5A69
PAD = 64                            # words between buffers (64 floats, 128 halves)
BETA1, BETA2, EPS, LR = np.float32(0.9), np.float32(0.999), 1e-15, 1e-2
SCALE = 1024.0                      # the loss scale the gradients carry
EMA_DECAY = np.float32(0.95)
BLOCK, CAP = 256, 2048
SHARE = {}                          # name of a bound -> largest observed |error| / bound


def _share(name, err, bound):
    ok = bound > 0
    if ok.any():
        SHARE[name] = max(SHARE.get(name, 0.0), float((err[ok] / bound[ok]).max()))


@pytest.fixture(scope='module', autouse=True)
def _print_shares():
    yield
    print('\nlargest observed share of each derived bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(SHARE.items())))


def _L():
    from nerfstyle_amd import _lib
    return _lib


class Arena:
    """Named buffers (float32, uint32 or float16) in one device allocation, each 256-byte aligned, PAD canary words apart."""

    def __init__(self, dev):
        self.dev, self.reg, self.words, self.t = dev, {}, PAD, None
        self.data = {}

    def add(self, name, arr, room=None):
        """`room`: elements to reserve (>= arr.size); the rest of the buffer holds the canary and must keep it"""
        arr = np.ascontiguousarray(arr)
        assert arr.dtype in (np.float32, np.uint32, np.float16) and self.t is None
        room = arr.size if room is None else room
        nw = (room * arr.dtype.itemsize + 3) // 4
        self.reg[name] = (self.words, arr.dtype, arr.size)
        self.data[name] = arr
        self.words += (nw + PAD - 1) // PAD * PAD + PAD
        return self

    def upload(self):
        img = np.full(self.words, CANARY, np.uint32)
        self.inside = np.zeros(self.words * 2, bool)                 # per half-word: belongs to a buffer
        for name, (w0, dt, n) in self.reg.items():
            img[w0:].view(dt)[:n] = self.data[name]
            self.inside[w0 * 2:w0 * 2 + n * dt.itemsize // 2] = True
        self.t = torch.from_numpy(img.view(np.int32)).to(self.dev)
        assert self.t.data_ptr() % 256 == 0
        self.data = None
        return self

    def ptr(self, name, offset=0):
        w0, dt, _ = self.reg[name]
        return self.t.data_ptr() + 4 * w0 + offset * dt.itemsize

    def view(self, name):
        """the buffer as a device tensor of int32 words (float32 / uint32 buffers), to poke values in stream order"""
        w0, dt, n = self.reg[name]
        assert dt.itemsize == 4
        return self.t[w0:w0 + n]

    def download(self):
        """-> {name: array}; asserts that everything outside the buffers still holds the canary"""
        torch.cuda.synchronize()
        img = self.t.cpu().numpy().view(np.uint32)
        spoiled = np.flatnonzero((img.view(np.uint16) != CANARY16) & ~self.inside)
        if spoiled.size:
            h = int(spoiled[0])
            near = [nm for nm, (w0, dt, n) in self.reg.items() if abs(h // 2 - w0) <= PAD + n * dt.itemsize // 4 + PAD]
            raise AssertionError('%d canary half-words overwritten, first at word %d, near %s' % (spoiled.size, h // 2, near))
        return {name: img[w0:].view(dt)[:n].copy() for name, (w0, dt, n) in self.reg.items()}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint16)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make_grads(rng, n, scale=SCALE):
    """|g| log-uniform over 1e-12 .. 1e3 times the loss scale, both signs, about one in eight exactly 0"""
    g = 10.0 ** rng.uniform(-12.0, 3.0, n) * rng.choice([-1.0, 1.0], n) * scale
    g[rng.random(n) < 0.125] = 0.0
    return g.astype(np.float32)


def make_state(rng, n, g, scale=SCALE):
    """p, m, v, ema as a previous step left them: m and v from an earlier gradient of the same spread; on a quarter of the
    elements beta1 * m is within a few percent of -(1 - beta1) * g, so the two addends of m' cancel; on half of the elements
    whose gradient is 0, m = v = 0 (the update must be exactly 0 there)"""
    gu = g.astype(np.float64) / scale
    gp = 10.0 ** rng.uniform(-12.0, 3.0, n) * rng.choice([-1.0, 1.0], n)
    m = 0.1 * gp
    v = 0.001 * gp * gp
    c = rng.random(n) < 0.25
    near = np.where(rng.random(int(c.sum())) < 0.2, 1.0, rng.uniform(0.97, 1.03, int(c.sum())))     # a fifth cancel to the last bits
    m[c] = -(0.1 / 0.9) * gu[c] * near
    v[c] = np.maximum(v[c], 0.001 * gu[c] ** 2)
    z = (g == 0) & (rng.random(n) < 0.5)
    m[z] = 0.0
    v[z] = 0.0
    p = rng.normal(0.0, 0.5, n)
    e = p + rng.normal(0.0, 0.05, n)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32), e.astype(np.float32), z


def canary_half(n):
    return np.full(n, CANARY16, np.uint16).view(np.float16)


def scaler_words(scale=SCALE, steps_taken=0, ema_n=0):
    w = np.zeros(16, np.uint32)
    w[R.SC_SCALE] = bits(np.float32(scale).reshape(1))[0]
    w[R.SC_STEP], w[R.SC_EMA_N] = steps_taken, ema_n
    w[[6, 7, 14, 15]] = (0xDEAD0006, 0xDEAD0007, 0xDEAD000E, 0xDEAD000F)     # reserved words: nothing may touch them
    return w


def scaler_update(a, name='state', growth_interval=2000, enabled=1, ema_decay_max=float(EMA_DECAY), lr_decay_steps=0.0):
    L = _L()
    assert L.lib().nsr_scaler_update(a.ptr(name), LR, lr_decay_steps, BETA1, BETA2, 2.0, 0.5, growth_interval, enabled, ema_decay_max,
                                     L.stream()) == NSR_OK


# ---- Adam, flat ---------------------------------------------------------------------------------------------------------------------
SMALL_N = [1, 2, 3, 4, 5, 7, 1023, 1025, 4 * BLOCK * 3 + 2]
LARGE_N = 4 * (CAP * BLOCK) + 4 * 300 + 3
MASKS = [0xF, 0x3, 0xC, 0x5, 0x0]
STEPS = [1, 2, 3, 100000]


def half_ns(n):
    return sorted({h for h in (0, 4, (n // 2) & ~3, n & ~3) if h <= n})


def check_adam(out, before, g, ref, name, zero_update=None):
    """the kernel's p, m, v, ema, g, half against the reference of one step"""
    tr = ref['trained']
    for k in ('p', 'm', 'v'):
        got = out[k].astype(np.float64)
        assert np.all(np.isfinite(got)), (name, k)
        err = np.abs(got - ref[k])
        _share(k, err, ref['bound_' + k])
        bad = np.flatnonzero(err > ref['bound_' + k])
        assert bad.size == 0, (name, k, int(bad[0]), float(err[bad[0]]), float(ref['bound_' + k][bad[0]]))
        assert same_bits(out[k][~tr], before[k][~tr]), (name, k, 'an untrained element changed')
    assert not bits(out['g']).any(), (name, 'gradient is not all +0.0 bits')
    if zero_update is not None and (zero_update & tr).any():
        z = zero_update & tr
        assert same_bits(out['p'][z], before['p'][z]) and not bits(out['m'][z]).any() and not bits(out['v'][z]).any(), (name, 'g = m = v = 0')
    if ref['ema'] is not None:
        err = np.abs(out['ema'].astype(np.float64) - ref['ema'])
        _share('ema', err, ref['bound_ema'])
        bad = np.flatnonzero(~(err <= ref['bound_ema']))
        assert bad.size == 0, (name, 'ema', int(bad[0]), float(err[bad[0]]), float(ref['bound_ema'][bad[0]]))
    if 'half' in out:
        hn = ref['half_n']
        assert same_bits(out['half'][:hn], R.cast_ref(out['p'][:hn])), (name, 'half copy is not the cast of p')
        assert np.all(bits(out['half'][hn:]) == CANARY16), (name, 'half copy written past half_n')


def run_flat(dev, path, n, mask, with_ema, with_half, half_n, steps, seed):
    """one buffer set, `steps` chained: each step uploads fresh gradients over the kernel's own previous outputs"""
    L = _L()
    rng = np.random.default_rng(seed)
    g = make_grads(rng, n)
    p, m, v, e, z = make_state(rng, n, g)
    cur = {'p': p, 'm': m, 'v': v}
    if with_ema:
        cur['ema'] = e
    t_prev = 0
    for step in steps:
        a = Arena(dev)
        for k in ('p', 'm', 'v'):
            a.add(k, cur[k])
        a.add('g', g)
        if with_ema:
            a.add('ema', cur['ema'])
        if with_half:
            a.add('half', canary_half(n))
        if path == 'scaled':
            a.add('state', scaler_words(steps_taken=step - 1, ema_n=t_prev))
        a.upload()
        ema_p, half_p = (a.ptr('ema') if with_ema else None), (a.ptr('half') if with_half else None)
        if path == 'host':
            assert L.lib().nsr_adam_step(a.ptr('p'), a.ptr('g'), a.ptr('m'), a.ptr('v'), ema_p, half_p, n, LR, BETA1, BETA2, EPS,
                                         np.float32(1.0 / SCALE), EMA_DECAY, step, mask, L.stream()) == NSR_OK
            ss, bc = R.host_scalars_ref(LR, BETA1, BETA2, step)
            s = R.Scalars(BETA1, BETA2, EPS, ss, bc, np.float32(1.0 / SCALE), EMA_DECAY)
            hn = n
        else:
            scaler_update(a)
            assert L.lib().nsr_adam_step_scaled(a.ptr('p'), a.ptr('g'), a.ptr('m'), a.ptr('v'), ema_p, half_p, n, half_n, BETA1, BETA2,
                                                EPS, mask, a.ptr('state'), L.stream()) == NSR_OK
            hn = half_n
        out = a.download()
        if path == 'scaled':
            dev_state = R.ScalerRef(out['state'])
            assert int(dev_state.words[R.SC_STEP]) == step and not dev_state.words[R.SC_SKIP]
            s = dev_state.scalars(BETA1, BETA2, EPS)                 # the state the kernel read, fed to the reference
            assert s.grad_scale_inv == np.float32(1.0 / SCALE)
        ref = R.adam_step_ref(cur['p'], g, cur['m'], cur['v'], cur.get('ema'), s, mask, hn)
        name = (path, n, hex(mask), with_ema, with_half, hn, step)
        check_adam(out, cur, g, ref, name, z if step == steps[0] else None)
        cur = {k: out[k] for k in cur}
        g = make_grads(rng, n)
        t_prev += 1
    return cur


@pytest.mark.parametrize('n', SMALL_N)
def test_adam_step_host_scalars(dev, n):
    case = 0
    for mask in MASKS:
        for with_ema in (False, True):
            for with_half in (False, True):
                run_flat(dev, 'host', n, mask, with_ema, with_half, n, STEPS, 1000 * n + case)
                case += 1


@pytest.mark.parametrize('n', SMALL_N)
def test_adam_step_scaled(dev, n):
    case = 0
    for mask in MASKS:
        for with_ema in (False, True):
            for with_half in (False, True):
                for half_n in (half_ns(n) if with_half else [0]):
                    run_flat(dev, 'scaled', n, mask, with_ema, with_half, half_n, STEPS, 2000 * n + case)
                    case += 1


@pytest.mark.parametrize('path,mask,half_n', [('host', 0xF, LARGE_N), ('scaled', 0xC, (LARGE_N // 2) & ~3)])
def test_adam_step_past_the_block_cap(dev, path, mask, half_n):
    """n / 4 + 1 > 2048 * 256: the grid is capped and every thread makes a second grid-stride trip, the tail behind it"""
    assert LARGE_N // 4 + 1 > CAP * BLOCK and LARGE_N & 3 == 3
    run_flat(dev, path, LARGE_N, mask, True, True, half_n, [1, 100000], 77)


@pytest.mark.parametrize('mask', [0x3, 0xC])
@pytest.mark.parametrize('n', [7, 1025])
def test_untrained_lanes_with_inf_and_nan_gradients(dev, n, mask):
    """inf / nan in gradients no trained lane reads: the trained results equal the same run without them bit for bit, and
    nothing non-finite appears anywhere (an untrained gradient is zeroed, not multiplied)"""
    L = _L()
    rng = np.random.default_rng(31 * n + mask)
    g = make_grads(rng, n)
    p, m, v, e, _ = make_state(rng, n, g)
    un = ~R.trained_mask(n, mask)
    g_bad = g.copy()
    g_bad[un] = np.resize(np.array([np.inf, -np.inf, np.nan, -np.nan], np.float32), int(un.sum()))
    outs = []
    for grad in (g, g_bad):
        a = Arena(dev).add('p', p).add('m', m).add('v', v).add('g', grad).add('ema', e).add('half', canary_half(n)).upload()
        assert L.lib().nsr_adam_step(a.ptr('p'), a.ptr('g'), a.ptr('m'), a.ptr('v'), a.ptr('ema'), a.ptr('half'), n, LR, BETA1, BETA2,
                                     EPS, np.float32(1.0 / SCALE), EMA_DECAY, 2, mask, L.stream()) == NSR_OK
        outs.append(a.download())
    for k in ('p', 'm', 'v', 'ema', 'g', 'half'):
        assert same_bits(outs[0][k], outs[1][k]), k
        assert np.all(np.isfinite(outs[1][k].astype(np.float64))), k
    assert not bits(outs[1]['g']).any()
    assert same_bits(outs[1]['p'][un], p[un]) and same_bits(outs[1]['m'][un], m[un]) and same_bits(outs[1]['v'][un], v[un])


@pytest.mark.parametrize('n', [3, 5, 1025])
def test_skipped_step(dev, n):
    """an inf found by a real nsr_grad_check -> nsr_scaler_update sets the skip word -> nsr_adam_step_scaled leaves p, m, v and
    the half copy alone, zeroes the gradient and still moves the shadow"""
    L = _L()
    rng = np.random.default_rng(500 + n)
    g = make_grads(rng, n)
    p, m, v, e, _ = make_state(rng, n, g)
    g[n - 1] = np.inf                                                # in the scalar tail
    hn = n & ~3
    a = (Arena(dev).add('p', p).add('m', m).add('v', v).add('g', g).add('ema', e).add('half', canary_half(n))
         .add('state', scaler_words(steps_taken=4, ema_n=4)).upload())
    assert L.lib().nsr_grad_check(a.ptr('g'), n, 0xF, a.ptr('state'), L.stream()) == NSR_OK
    scaler_update(a)
    assert L.lib().nsr_adam_step_scaled(a.ptr('p'), a.ptr('g'), a.ptr('m'), a.ptr('v'), a.ptr('ema'), a.ptr('half'), n, hn, BETA1, BETA2,
                                        EPS, 0xF, a.ptr('state'), L.stream()) == NSR_OK
    out = a.download()
    st = R.ScalerRef(out['state'])
    want = R.ScalerRef(scaler_words(steps_taken=4, ema_n=4))
    want.set_found()
    want.update(LR, 0.0, BETA1, BETA2, ema_decay_max=float(EMA_DECAY))
    assert np.array_equal(st.words, want.words) and st.words[R.SC_SKIP] == 1 and st.f(R.SC_SCALE) == SCALE / 2
    assert same_bits(out['p'], p) and same_bits(out['m'], m) and same_bits(out['v'], v)
    assert np.all(bits(out['half']) == CANARY16) and not bits(out['g']).any()
    ref = R.adam_step_ref(p, g, m, v, e, st.scalars(BETA1, BETA2, EPS), 0xF, hn)
    err = np.abs(out['ema'].astype(np.float64) - ref['ema'])
    _share('ema', err, ref['bound_ema'])
    assert np.all(err <= ref['bound_ema']) and not same_bits(out['ema'], e)


# ---- nsr_grad_check -----------------------------------------------------------------------------------------------------------------
BAD = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001], np.uint32)      # +inf, -inf, quiet nan, nan with the sign bit
GC_BLOCK4 = 4 * BLOCK                                                              # float4s one block covers per unrolled trip


def clean_grads(rng, n):
    """finite values that must not flag: +-FLT_MAX, subnormals, -0.0 among ordinary ones"""
    g = rng.normal(0, 1, n).astype(np.float32)
    special = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1e-45, -1e-45, 1.1e-38, -0.0, 0.0], np.float32)
    idx = rng.permutation(n)[:min(n, 4 * special.size)]
    g[idx] = np.resize(special, idx.size)
    if n >= 8:
        g[[0, n - 1, n - 2]] = special[[0, 1, 5]]
    assert np.all(np.isfinite(g))
    return g


def grad_check_ranges(n):
    """-> (stride in float4s, sorted float4 indices the 4-deep unrolled loop reads, n / 4) for nsr_grad_check's launch"""
    n4 = n // 4
    blocks = max(1, min(CAP, (n4 + GC_BLOCK4 - 1) // GC_BLOCK4))
    stride = blocks * BLOCK
    i = np.arange(stride, dtype=np.int64)
    trips = np.maximum(0, -((3 * stride + i - n4) // (4 * stride)))            # ceil((n4 - 3 stride - i) / (4 stride)), >= 0
    return stride, trips, n4


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 70])
def test_grad_check_every_position_small(dev, n):
    """one inf at every position under every mask: word [2] is set exactly when the mask selects the position"""
    L = _L()
    masks = [0xF, 0x3, 0xC, 0x1, 0x8]
    g = clean_grads(np.random.default_rng(n), n)
    a = Arena(dev)
    cases = [(pos, mask) for pos in range(n) for mask in masks] + [(None, 0xF)]
    for c, (pos, mask) in enumerate(cases):
        gc = g.copy()
        if pos is not None:
            bits(gc)[pos] = BAD[(pos + c) % 4]
        a.add('g%d' % c, gc).add('s%d' % c, scaler_words())
    a.upload()
    for c, (pos, mask) in enumerate(cases):
        assert L.lib().nsr_grad_check(a.ptr('g%d' % c), n, mask, a.ptr('s%d' % c), L.stream()) == NSR_OK
    out = a.download()
    for c, (pos, mask) in enumerate(cases):
        want = scaler_words()
        want[R.SC_FOUND] = int(pos is not None and bool(mask >> (pos & 3) & 1))
        assert np.array_equal(out['s%d' % c], want), (n, pos, hex(mask), out['s%d' % c][R.SC_FOUND])


GC_SHAPES = [4 * 2048 + 2, 4 * 1500 + 3, 4 * (CAP * 1024) + 4 * 5000 + 1]


@pytest.mark.parametrize('n', GC_SHAPES)
def test_grad_check_code_paths(dev, n):
    """one bad value at the first element, the last element of the unrolled range, the first of the remainder range, the last
    full float4, each tail element and the first element of the second trip: flagged under 0xF, not flagged under the mask
    that leaves that lane out; the clean gradient (+-FLT_MAX, subnormals, -0.0) does not flag; only word [2] changes"""
    L = _L()
    stride, trips, n4 = grad_check_ranges(n)
    unrolled = 4 * int(trips.max()) * stride if trips.max() else 0              # float4s [0, unrolled) when every thread unrolls
    if n == GC_SHAPES[0]:
        assert trips.min() == 1 and unrolled == n4                                # every thread unrolled, no remainder
    elif n == GC_SHAPES[1]:
        assert trips.max() == 0                                                   # nobody unrolled
    else:
        assert trips.min() == 1 and trips.max() == 1 and unrolled == 4 * stride == CAP * 1024 and n4 - unrolled == 5000
    pos = {0: 'first', 4 * n4 - 1: 'last full float4'}
    if unrolled:
        pos[4 * unrolled - 1] = 'last of the unrolled range'
    if unrolled < n4:
        pos[4 * unrolled] = 'first of the remainder range' if unrolled else 'first'
        pos[4 * (n4 - 1)] = 'first lane of the last full float4'
    if n4 > 4 * stride:
        pos[4 * 4 * stride] = 'first of the second trip'
    for j in range(n & 3):
        pos[4 * n4 + j] = 'tail element %d' % j
    g = clean_grads(np.random.default_rng(n), n)
    cases = [(None, 0xF, 0)] + [(q, 0xF, b) for q in sorted(pos) for b in range(4)] + [(q, 0xF ^ (1 << (q & 3)), 0) for q in sorted(pos)]
    a = Arena(dev).add('g', g)
    for c in range(len(cases)):
        a.add('s%d' % c, scaler_words())
    a.upload()
    gv = a.view('g')
    bad_i32 = BAD.view(np.int32)
    for c, (q, mask, b) in enumerate(cases):
        if q is not None:
            keep = gv[q].clone()
            gv[q] = int(bad_i32[b])
        assert L.lib().nsr_grad_check(a.ptr('g'), n, mask, a.ptr('s%d' % c), L.stream()) == NSR_OK
        if q is not None:
            gv[q] = keep
    out = a.download()
    assert same_bits(out['g'], g)
    for c, (q, mask, b) in enumerate(cases):
        want = scaler_words()
        want[R.SC_FOUND] = int(q is not None and mask == 0xF)
        assert np.array_equal(out['s%d' % c], want), (n, q, pos.get(q), hex(mask), b, out['s%d' % c][R.SC_FOUND])


# ---- nsr_scaler_update --------------------------------------------------------------------------------------------------------------
def run_scaler(dev, words, found_at, steps, **kw):
    """`steps` launches, one per step, the state copied aside after each (in stream order) -> [steps, 16] uint32"""
    a = Arena(dev).add('state', words).add('hist', np.zeros(16 * steps, np.uint32)).upload()
    st, hist = a.view('state'), a.view('hist')
    for k in range(steps):
        if k in found_at:
            st[R.SC_FOUND] = found_at[k]
        scaler_update(a, **kw)
        hist[16 * k:16 * k + 16] = st
    return a.download()['hist'].reshape(steps, 16)


def check_scaler(hist, words, found_at, ref_kw, label):
    """integer words, the scale, 1 / scale and the EMA decay exact; lr, step size and 1 / sqrt(bc2) within 1 fp32 ulp (the
    device's double pow may differ from libm in its last bits, which moves the fp32 rounding only at a near-tie)"""
    ref = R.ScalerRef(words)
    for k in range(hist.shape[0]):
        if k in found_at:
            ref.set_found(found_at[k])
        ref.update(LR, **ref_kw)
        for w in range(16):
            if w in (R.SC_STEP_SIZE, R.SC_INV_BC2, R.SC_LR):
                d = R.ulp_distance_f32(hist[k, w], ref.words[w])
                assert d <= 1, (label, k, w, hex(hist[k, w]), hex(ref.words[w]))
                SHARE['scaler ulp'] = max(SHARE.get('scaler ulp', 0.0), float(d))
            else:
                assert hist[k, w] == ref.words[w], (label, k, w, hex(hist[k, w]), hex(ref.words[w]))
        ref.words[:] = hist[k]                                       # the next step starts from the kernel's own state
    return ref


def _kw(growth_interval=2000, enabled=1, ema_decay_max=float(EMA_DECAY), lr_decay_steps=0.0):
    dev_kw = dict(growth_interval=growth_interval, enabled=enabled, ema_decay_max=ema_decay_max, lr_decay_steps=lr_decay_steps)
    ref_kw = dict(lr_decay_steps=lr_decay_steps, beta1=BETA1, beta2=BETA2, growth=2.0, backoff=0.5, growth_interval=growth_interval,
                  enabled=enabled, ema_decay_max=ema_decay_max)
    return dev_kw, ref_kw


def test_scaler_growth_interval_3(dev):
    """60 steps with infs met at tracker 0, at tracker = interval - 1, at 1, two in a row, and a flag value other than 1"""
    found_at = {0: 1, 3: 1, 9: 1, 20: 1, 21: 1, 30: 7, 44: 1}
    dev_kw, ref_kw = _kw(growth_interval=3, lr_decay_steps=50.0)
    hist = run_scaler(dev, scaler_words(), found_at, 60, **dev_kw)
    check_scaler(hist, scaler_words(), found_at, ref_kw, 'gi3')
    tracker_before = [0] + [int(x) for x in hist[:-1, R.SC_TRACKER]]
    assert {tracker_before[k] for k in found_at} == {0, 1, 2} and tracker_before[0] == 0 and tracker_before[3] == 2
    assert int(hist[-1, R.SC_SKIPPED]) == 7 and int(hist[-1, R.SC_STEP]) == 53 and int(hist[-1, R.SC_EMA_N]) == 60
    assert len(set(hist[:, R.SC_SCALE].tolist())) > 3


def test_scaler_default_interval_2005_clean_steps(dev):
    dev_kw, ref_kw = _kw(lr_decay_steps=3000.0)
    hist = run_scaler(dev, scaler_words(scale=65536.0), {}, 2005, **dev_kw)
    check_scaler(hist, scaler_words(scale=65536.0), {}, ref_kw, 'gi2000')
    scale = hist[:, R.SC_SCALE].copy().view(np.float32)
    assert np.all(scale[:1999] == 65536.0) and np.all(scale[1999:] == 131072.0)          # one growth, with the 2000th clean step
    assert int(hist[1998, R.SC_TRACKER]) == 1999 and int(hist[1999, R.SC_TRACKER]) == 0 and int(hist[-1, R.SC_TRACKER]) == 5
    assert hist[1999:, R.SC_INV_SCALE].view(np.float32)[0] == np.float32(1.0 / 65536.0)     # the scale THOSE gradients carried
    assert hist[2000:, R.SC_INV_SCALE].view(np.float32)[0] == np.float32(1.0 / 131072.0)


@pytest.mark.parametrize('label,start,found_at,steps,kw', [
    ('99999 steps taken', dict(steps_taken=99999, ema_n=123456), {2: 1}, 6, dict(lr_decay_steps=30000.0)),
    ('disabled, flag set', dict(scale=1.0), {0: 1, 3: 1}, 6, dict(enabled=0)),
    ('disabled, scale not 1', dict(scale=512.0), {1: 1}, 4, dict(enabled=0, growth_interval=1)),
    ('lr_decay_steps 0', dict(), {}, 5, dict(lr_decay_steps=0.0)),
    ('lr_decay_steps -1', dict(), {}, 5, dict(lr_decay_steps=-1.0)),
    ('lr_decay_steps 50', dict(steps_taken=70), {1: 1}, 8, dict(lr_decay_steps=50.0)),
    ('no ema', dict(ema_n=17), {1: 1}, 5, dict(ema_decay_max=-1.0)),
    ('growth_interval 1', dict(scale=2.0), {3: 1}, 8, dict(growth_interval=1)),
])
def test_scaler_settings(dev, label, start, found_at, steps, kw):
    words = scaler_words(**start)
    if label == 'no ema':
        words[R.SC_EMA_DECAY] = 0x3F000000                                     # must stay
    dev_kw, ref_kw = _kw(**kw)
    hist = run_scaler(dev, words, found_at, steps, **dev_kw)
    check_scaler(hist, words, found_at, ref_kw, label)
    last = hist[-1]
    f = lambda w: float(last[w:w + 1].copy().view(np.float32)[0])
    if label.startswith('disabled'):
        assert int(last[R.SC_SKIPPED]) == 0 and int(last[R.SC_STEP]) == steps and f(R.SC_INV_SCALE) == 1.0
        assert np.all(hist[:, R.SC_SCALE] == words[R.SC_SCALE]) and not hist[:, R.SC_FOUND].any() and not hist[:, R.SC_SKIP].any()
    if label == 'no ema':
        assert np.all(hist[:, R.SC_EMA_N] == 17) and np.all(hist[:, R.SC_EMA_DECAY] == 0x3F000000)
    if label == 'growth_interval 1':
        assert f(R.SC_SCALE) == 2.0 * 2.0 ** 3 * 0.5 * 2.0 ** 4 and not hist[:, R.SC_TRACKER].any()
    if label.startswith('lr_decay_steps') and not label.endswith('50'):
        assert np.all(hist[:, R.SC_LR] == bits(np.float32(LR).reshape(1))[0])
    if label == '99999 steps taken':
        assert int(last[R.SC_STEP]) == 99999 + 5 and f(R.SC_INV_BC2) == 1.0 and int(last[R.SC_EMA_N]) == 123456 + 6


# ---- lanes --------------------------------------------------------------------------------------------------------------------------
SMALL_ROWS = [1, 2, 255, 256, 257]
LARGE_ROWS = CAP * BLOCK + 37


def lane_ranges(rows):
    if rows == LARGE_ROWS:
        return [(0, rows), (3 * BLOCK + 101, rows - 2 * BLOCK - 59)]             # both ends inside a block
    return [r for r in dict.fromkeys(((0, rows), (1, rows - 1), (rows - 1, rows))) if r[0] <= r[1]]


@pytest.mark.parametrize('lane_mask', [0x3, 0xC])
@pytest.mark.parametrize('rows', SMALL_ROWS + [LARGE_ROWS])
def test_lanes_pack(dev, rows, lane_mask):
    L = _L()
    g = make_grads(np.random.default_rng(rows + lane_mask), 4 * rows)
    a = Arena(dev).add('g', g).add('packed', np.zeros(2 * rows, np.float32)).upload()
    assert L.lib().nsr_lanes_pack(a.ptr('g'), rows, lane_mask, a.ptr('packed'), L.stream()) == NSR_OK
    out = a.download()
    want, zero = R.lanes_pack_ref(g.reshape(rows, 4), lane_mask)
    assert same_bits(out['packed'], want.reshape(-1)) and not bits(out['g']).any()


@pytest.mark.parametrize('lane_mask', [0x3, 0xC])
@pytest.mark.parametrize('rows', SMALL_ROWS + [LARGE_ROWS])
def test_lanes_unpack(dev, rows, lane_mask):
    L = _L()
    rng = np.random.default_rng(3 * rows + lane_mask)
    arena = rng.normal(0, 1, 4 * rows).astype(np.float32)
    for lo, hi in lane_ranges(rows):
        # the gathered buffer is indexed by global row: its rows outside [lo, hi) hold values that must not arrive anywhere
        packed = rng.normal(0, 100, 2 * rows).astype(np.float32)
        for with_half in (True, False):
            a = Arena(dev).add('arena', arena).add('packed', packed)
            if with_half:
                a.add('half', canary_half(4 * rows))
            a.upload()
            assert L.lib().nsr_lanes_unpack(a.ptr('packed'), lo, hi, lane_mask, a.ptr('arena'), a.ptr('half') if with_half else None,
                                            L.stream()) == NSR_OK
            out = a.download()
            want_a, want_h = R.lanes_unpack_ref(packed.reshape(rows, 2), lo, hi, lane_mask, arena.reshape(rows, 4),
                                                canary_half(4 * rows).reshape(rows, 4) if with_half else None)
            assert same_bits(out['arena'], want_a.reshape(-1)), (rows, lo, hi)
            assert same_bits(out['packed'], packed)
            if with_half:
                assert same_bits(out['half'], want_h.reshape(-1)), (rows, lo, hi)


def expand(packed, fill, lane_mask):
    """packed [nr, 2] -> flat [4 nr]: the trained lanes from packed, the others from fill [nr, 2]"""
    l0 = R.lane0_of(lane_mask)
    x = np.empty((packed.shape[0], 4), np.float32)
    x[:, l0:l0 + 2] = packed
    x[:, 2 - l0:4 - l0] = fill
    return x.reshape(-1)


def run_lanes_adam(dev, rows, lo, hi, lane_mask, path, with_ema, with_half, alias, skip, seed):
    """nsr_lanes_adam(_scaled) on rows [lo, hi) of a table of `rows` rows, and nsr_adam_step(_scaled) with the matching
    elem_mask4 on a copy of those rows.  The shard-local buffers are given room for `hi` rows, of which the first hi - lo are
    theirs: a kernel that indexed them by global row would be caught by the canary comparison, inside the allocation."""
    L = _L()
    rng = np.random.default_rng(seed)
    nr = hi - lo
    l0 = R.lane0_of(lane_mask)
    g4 = make_grads(rng, 4 * rows)
    p4, m4, v4, e4, _ = make_state(rng, 4 * rows, g4)
    sl = slice(4 * lo, 4 * hi)
    pk = lambda x: x[sl].reshape(nr, 4)[:, l0:l0 + 2].reshape(-1).copy()
    g, m, v = pk(g4), pk(m4), pk(v4)
    ema = e4[sl].copy()
    if skip:
        g[(2 * nr) // 2] = np.inf
    words = scaler_words(steps_taken=2, ema_n=2)
    a = Arena(dev).add('arena', p4).add('g', g, 2 * hi).add('m', m, 2 * hi).add('v', v, 2 * hi).add('state', words).add('fstate', words)
    if not alias:
        a.add('out', np.zeros(2 * nr, np.float32), 2 * hi)
    if with_ema:
        a.add('ema', ema, 4 * hi).add('fema', ema)
    if with_half:
        a.add('half', canary_half(4 * rows)).add('fhalf', canary_half(4 * nr))
    # the flat twin: the same rows as a region of their own; its untrained lanes carry other gradients and moments
    other = lambda x: x[sl].reshape(nr, 4)[:, 2 - l0:4 - l0]
    a.add('fp', p4[sl]).add('fg', expand(g.reshape(nr, 2), other(g4), lane_mask)).add('fm', m4[sl]).add('fv', v4[sl])
    a.upload()
    opt = lambda name: a.ptr(name) if name in a.reg else None
    out_name = 'g' if alias else 'out'
    if nr == 0:
        null = [None] * 7
        assert L.lib().nsr_lanes_adam(*null, lo, hi, lane_mask, LR, BETA1, BETA2, EPS, 1.0, EMA_DECAY, 1, L.stream()) == NSR_OK
        out = a.download()
        assert same_bits(out['arena'], p4)
        return
    if path == 'host':
        gsi = np.float32(1.0 / SCALE)
        assert L.lib().nsr_lanes_adam(a.ptr('arena'), opt('half'), a.ptr('g'), a.ptr('m'), a.ptr('v'), opt('ema'), a.ptr(out_name), lo, hi,
                                      lane_mask, LR, BETA1, BETA2, EPS, gsi, EMA_DECAY, 3, L.stream()) == NSR_OK
        assert L.lib().nsr_adam_step(a.ptr('fp'), a.ptr('fg'), a.ptr('fm'), a.ptr('fv'), opt('fema'), opt('fhalf'), 4 * nr, LR, BETA1,
                                     BETA2, EPS, gsi, EMA_DECAY, 3, lane_mask, L.stream()) == NSR_OK
    else:
        for st, gname, gn in (('state', 'g', 2 * nr), ('fstate', 'fg', 4 * nr)):
            if skip:
                assert L.lib().nsr_grad_check(a.ptr(gname), gn, 0xF if st == 'state' else lane_mask, a.ptr(st), L.stream()) == NSR_OK
            scaler_update(a, st)
        assert L.lib().nsr_lanes_adam_scaled(a.ptr('arena'), opt('half'), a.ptr('g'), a.ptr('m'), a.ptr('v'), opt('ema'), a.ptr(out_name),
                                             lo, hi, lane_mask, BETA1, BETA2, EPS, a.ptr('state'), L.stream()) == NSR_OK
        assert L.lib().nsr_adam_step_scaled(a.ptr('fp'), a.ptr('fg'), a.ptr('fm'), a.ptr('fv'), opt('fema'), opt('fhalf'), 4 * nr, 4 * nr,
                                            BETA1, BETA2, EPS, lane_mask, a.ptr('fstate'), L.stream()) == NSR_OK
    out = a.download()
    name = (rows, lo, hi, hex(lane_mask), path, with_ema, with_half, alias, skip)
    if path == 'host':
        ss, bc = R.host_scalars_ref(LR, BETA1, BETA2, 3)
        s = R.Scalars(BETA1, BETA2, EPS, ss, bc, np.float32(1.0 / SCALE), EMA_DECAY)
    else:
        assert np.array_equal(out['state'], out['fstate']) and int(out['state'][R.SC_SKIP]) == int(skip), name
        s = R.ScalerRef(out['state']).scalars(BETA1, BETA2, EPS)
    # (1) within the reference bounds: the rows of the range as a flat region under elem_mask4 = lane_mask
    ref = R.adam_step_ref(p4[sl], expand(g.reshape(nr, 2), other(g4), lane_mask), m4[sl], v4[sl], ema if with_ema else None, s, lane_mask)
    tr = R.trained_mask(4 * nr, lane_mask)
    got = {'p': out['arena'][sl], 'm': expand(out['m'].reshape(nr, 2), other(m4), lane_mask),
           'v': expand(out['v'].reshape(nr, 2), other(v4), lane_mask)}
    for k in ('p', 'm', 'v'):
        err = np.abs(got[k].astype(np.float64) - ref[k])
        _share(k, err, ref['bound_' + k])
        assert np.all(err <= ref['bound_' + k]), (name, k)
    if with_ema:
        err = np.abs(out['ema'].astype(np.float64) - ref['ema'])
        _share('ema', err, ref['bound_ema'])
        assert np.all(err <= ref['bound_ema']), (name, 'ema')
        assert not same_bits(out['ema'], ema)
    # (2) bit-identical to the flat entry point with the matching element mask (the header's promise)
    assert same_bits(got['p'], out['fp']) and same_bits(got['m'], out['fm']) and same_bits(got['v'], out['fv']), name
    if with_ema:
        assert same_bits(out['ema'], out['fema']), name
    # (3) rows outside the range and untrained lanes inside it are untouched
    rest = np.ones(4 * rows, bool)
    rest[sl] = False
    rest[sl][~tr] = True
    rest[4 * lo:4 * hi] |= ~tr
    assert same_bits(out['arena'][rest], p4[rest]), name
    # (4) packed_out holds the lanes after the step; a separate packed_out leaves the gradient alone
    assert same_bits(out[out_name], pk(out['arena'])), name
    if not alias:
        assert same_bits(out['g'], g), name
    # (5) the half copy: all four lanes of the rows in range, the canary elsewhere
    if with_half:
        inr = np.zeros(4 * rows, bool)
        inr[sl] = not skip
        assert same_bits(out['half'][inr], R.cast_ref(out['arena'][inr])), name
        assert np.all(bits(out['half'][~inr]) == CANARY16), name
        assert same_bits(out['half'][sl], out['fhalf']), name
    if skip:
        assert same_bits(out['arena'], p4) and same_bits(out['m'], m) and same_bits(out['v'], v), name
        assert same_bits(out[out_name], pk(p4)), name


@pytest.mark.parametrize('lane_mask', [0x3, 0xC])
@pytest.mark.parametrize('rows', SMALL_ROWS)
def test_lanes_adam(dev, rows, lane_mask):
    case = 0
    for lo, hi in lane_ranges(rows):
        for path in ('host', 'scaled'):
            for with_ema in (False, True):
                for with_half in (False, True):
                    for alias in (True, False):
                        run_lanes_adam(dev, rows, lo, hi, lane_mask, path, with_ema, with_half, alias, False, 10000 * rows + case)
                        case += 1
        if hi > lo:
            for alias in (True, False):
                run_lanes_adam(dev, rows, lo, hi, lane_mask, 'scaled', True, True, alias, True, 10000 * rows + 500 + case)
                case += 1


@pytest.mark.parametrize('lane_mask,path,alias', [(0x3, 'host', True), (0xC, 'scaled', False)])
def test_lanes_adam_past_the_block_cap(dev, lane_mask, path, alias):
    for k, (lo, hi) in enumerate(lane_ranges(LARGE_ROWS)):
        assert hi - lo > CAP * BLOCK or k == 1
        run_lanes_adam(dev, LARGE_ROWS, lo, hi, lane_mask, path, True, True, alias, False, 99 + k)


# ---- nsr_cast_f32_to_f16 ------------------------------------------------------------------------------------------------------------
def cast_inputs():
    """every f16 value, the midpoint of every adjacent finite pair and its two fp32 neighbours, the overflow threshold, half
    of the smallest subnormal and its neighbours, +-0"""
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    pos = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)           # 0 .. 65504 ascending
    mid = (pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)                   # exact in fp32
    mid = mid.astype(np.float32)
    up, down = np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))
    tiny = np.float32(2.0 ** -25)
    extra = np.array([65504.0, 65519.996, 65520.0, 1e30, tiny, np.nextafter(tiny, np.float32(1)), np.nextafter(tiny, np.float32(0)),
                      0.0, -0.0, np.finfo(np.float32).max, 1e-45], np.float32)
    one = np.concatenate([mid, up, down, extra])
    return np.concatenate([allh, one, -one]).astype(np.float32)


@pytest.fixture(scope='module')
def cast_set():
    x = cast_inputs()
    x.setflags(write=False)
    return x


CAST_LARGE = 8 * (CAP * BLOCK) + 8 * 11 + 5


@pytest.mark.parametrize('n', ['set', 1, 7, 8, 9, CAST_LARGE])
def test_cast_f32_to_f16(dev, cast_set, n):
    L = _L()
    if n == 'set':
        x = cast_set
    elif n == CAST_LARGE:
        x = np.resize(cast_set, n)
    else:
        x = cast_set[65536 + 1000:][:n]                              # midpoints: rounding matters in the tail too
    n = x.size
    a = Arena(dev).add('src', x).add('dst', canary_half(n)).upload()
    assert L.lib().nsr_cast_f32_to_f16(a.ptr('src'), a.ptr('dst'), n, L.stream()) == NSR_OK
    out = a.download()
    want = R.cast_ref(x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out['dst']), nan)
    bad = np.flatnonzero((bits(out['dst']) != bits(want)) & ~nan)
    assert bad.size == 0, (int(bad[0]), float(x[bad[0]]), hex(bits(out['dst'])[bad[0]]), hex(bits(want)[bad[0]]))
    assert same_bits(out['src'], x)
