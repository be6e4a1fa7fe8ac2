"""NumPy fp64 restatement of the optimiser kernels (csrc/optim.hip) and of nsr_cast_f32_to_f16 (csrc/gridenc.hip): one fused Adam
step with its unscale, element mask, EMA shadow and zeroed gradient; the bookkeeping of k_scaler_update word by word; the lane
pack / unpack data movement; the f16 cast -- and the error bounds tests/test_gpu_optim.py holds the fp32 kernels to.

One element of one step, as adam_one / ema_move write it (every value fp32, u = 2^-24 the unit roundoff of one fp32 operation):

    gs = g * grad_scale_inv                               1 rounding
    m' = beta1 * m + (1 - beta1) * gs                     3 roundings: beta1 * m, (1 - beta1) * gs, the sum
    v' = beta2 * v + (1 - beta2) * gs * gs                4 roundings: beta2 * v, (1 - beta2) * gs, ... * gs, the sum
    denom = sqrt(v') * inv_sqrt_bc2 + eps                 3 roundings (sqrtf and / are correctly rounded: -O3, no fast-math)
    p' = p - step_size * (m' / denom)                     3 roundings: the quotient, the product, the difference
    e' = e - k * (e - p'),  k = 1 - ema_decay             3 roundings: the inner difference, the product, the outer difference

beta1, beta2, 1 - beta and k are formed in fp32 exactly as the kernel forms them, so they carry no error against the kernel.
The compiler may contract a product and a sum into one FMA, which drops a rounding; the counts are those of the uncontracted
expression, the larger number.  To first order in u, with A(x) the bound of x:

    m':  the first addend carries 1 rounding, the second 2 (gs, the product), the sum 1 over both:
             |dm| <= u (2 |beta1 m| + 3 |(1 - beta1) gs|)  <=  3 u S_m,        S_m = |beta1 m| + |(1 - beta1) gs|
         S_m, not |m'|: the two addends cancel when the gradient turns against the momentum.
    v':  addends 1 and 4 roundings (gs enters twice), the sum 1, every addend >= 0 so S_v = v':
             |dv| <= u (2 beta2 v + 5 (1 - beta2) gs^2)  <=  5 u v'
    p':  denom: sqrt halves v's 5 u and rounds (3.5 u), the product (4.5 u), the sum of two positive terms (5.5 u);
         q = step_size * (m' / denom) inherits dm / denom absolutely, 5.5 u from denom, and 2 roundings of its own:
             |dq| <= step_size * 3 u S_m / denom + 7.5 u |q|;          |dp| <= u |p'| + |dq|
    e':  the kernel's shadow follows the kernel's p', so p's bound enters with weight k; the inner difference rounds once on
         |e - p'| <= |e| + |p'|, the product once more, the outer difference once on |e'|:
             |de| <= u |e'| + 2 u k (|e| + |p'|) + k A(p')

Every constant above is doubled in the bounds returned here (SAFETY = 2): the second-order terms and a denom whose eps share
rounds differently are far below that.  An intermediate that underflows loses at most the smallest normal number, flushed or not;
TINY = 4 * 2^-126 is added to every bound for it.  The bounds do not hold for inputs that overflow fp32 (the tests stay below).

Scalars.  A field of `Scalars` given as numpy.float32 is the kernel's own fp32 value, and 1 - x is then formed in fp32 as the kernel
forms it; a Python float is taken as it is (tests/test_optim_cpu.py compares with torch in fp64 that way)."""
import collections
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 2.0
TINY = 4.0 * 2.0 ** -126
C_M, C_V, C_DENOM, C_Q = 3.0, 5.0, 5.5, 7.5       # the counts derived in the module docstring

Scalars = collections.namedtuple('Scalars', 'beta1 beta2 eps step_size inv_sqrt_bc2 grad_scale_inv ema_decay skip')
Scalars.__new__.__defaults__ = (False,)


def one_minus(x):
    """1 - x as the kernel forms it: in fp32 when x is the kernel's fp32 value, else in fp64"""
    if isinstance(x, np.float32):
        return float(np.float32(1.0) - x)
    return 1.0 - float(x)


def trained_mask(n, mask4):
    """bool [n]: element i is trained <=> bit (i & 3) of mask4"""
    return ((int(mask4) >> (np.arange(n) & 3)) & 1).astype(bool)


def host_scalars_ref(lr, beta1, beta2, step):
    """(step_size, inv_sqrt_bc2) as host_scalars forms them: betas are the fp32 values widened, the powers and the quotients
    are taken in double, the results rounded to fp32 once"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    bc1, bc2 = 1.0 - math.pow(b1, float(step)), 1.0 - math.pow(b2, float(step))
    return np.float32(float(np.float32(lr)) / bc1), np.float32(1.0 / math.sqrt(bc2))


def adam_step_ref(p, g, m, v, ema, scalars, mask4, half_n=0, u=U32):
    """One step in fp64 from the fp32 (or fp64) inputs -> dict of fp64 arrays p, m, v, ema (None without a shadow), g (all zero),
    their bounds bound_p, bound_m, bound_v, bound_ema for unit roundoff u, `trained` (bool) and `half_n`.  On a skipped step
    (scalars.skip) p, m, v stay, the gradient is zeroed and the shadow still moves.  The f16 copy is not restated here: it is the
    cast of the kernel's own p on [0, half_n), cast_ref."""
    s = scalars
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    n = p.size
    tr = trained_mask(n, mask4) & (not s.skip)
    b1, b2 = float(s.beta1), float(s.beta2)
    k1, k2 = one_minus(s.beta1), one_minus(s.beta2)
    gs = np.where(tr, g, 0.0) * float(s.grad_scale_inv)            # an untrained gradient is zeroed, whatever it holds
    a1, a2 = b1 * m, k1 * gs
    m1 = a1 + a2
    v1 = b2 * v + k2 * gs * gs
    denom = np.sqrt(v1) * float(s.inv_sqrt_bc2) + float(s.eps)
    q = float(s.step_size) * (m1 / denom)
    p1 = p - q
    s_m = np.abs(a1) + np.abs(a2)
    bm = SAFETY * C_M * u * s_m + TINY
    bv = SAFETY * C_V * u * v1 + TINY
    bp = SAFETY * (u * np.abs(p1) + float(s.step_size) * C_M * u * s_m / denom + C_Q * u * np.abs(q)) + TINY
    res = {'p': np.where(tr, p1, p), 'm': np.where(tr, m1, m), 'v': np.where(tr, v1, v), 'g': np.zeros(n),
           'bound_p': np.where(tr, bp, 0.0), 'bound_m': np.where(tr, bm, 0.0), 'bound_v': np.where(tr, bv, 0.0),
           'trained': tr, 'half_n': int(half_n), 'ema': None, 'bound_ema': None}
    if ema is not None:
        e = np.asarray(ema, np.float64)
        k = one_minus(s.ema_decay)
        res['ema'] = e - k * (e - res['p'])
        res['bound_ema'] = SAFETY * (u * np.abs(res['ema']) + 2.0 * u * k * (np.abs(e) + np.abs(res['p']))) + k * res['bound_p'] + TINY
    return res


# ---- k_scaler_update, word by word ------------------------------------------------------------------------------------------------
SC_SCALE, SC_TRACKER, SC_FOUND, SC_STEP, SC_SKIPPED, SC_EMA_N = 0, 1, 2, 3, 4, 5
SC_SKIP, SC_STEP_SIZE, SC_INV_BC2, SC_INV_SCALE, SC_LR, SC_EMA_DECAY = 8, 9, 10, 11, 12, 13
SC_FLOAT_WORDS = (SC_SCALE, SC_STEP_SIZE, SC_INV_BC2, SC_INV_SCALE, SC_LR, SC_EMA_DECAY)


def _f2u(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _u2f(w):
    return np.array([w], np.uint32).view(np.float32)[0]


class ScalerRef:
    """The 16-word state of nsr_scaler_update and its policy.  `words` is a uint32 array laid out as include/nsr.h describes;
    update() is one launch.  fp32 arithmetic (the scale, 1 / scale, the EMA decay) is done in numpy.float32, double arithmetic
    (LambdaLR, the bias corrections) in Python floats with libm's pow, rounded to fp32 once as the kernel rounds."""

    def __init__(self, words=None, scale=65536.0):
        self.words = np.zeros(16, np.uint32) if words is None else np.array(words, np.uint32).copy()
        if words is None:
            self.words[SC_SCALE] = _f2u(scale)

    def f(self, i):
        return _u2f(self.words[i])

    def set_found(self, found=1):
        self.words[SC_FOUND] = found

    def update(self, lr_base, lr_decay_steps, beta1, beta2, growth=2.0, backoff=0.5, growth_interval=2000, enabled=1,
               ema_decay_max=-1.0):
        w = self.words
        f32 = np.float32
        lr_base, lr_decay_steps, beta1, beta2 = f32(lr_base), f32(lr_decay_steps), f32(beta1), f32(beta2)
        if f32(ema_decay_max) >= 0.0:
            n = (int(w[SC_EMA_N]) + 1) & 0xFFFFFFFF
            w[SC_EMA_N] = n
            w[SC_EMA_DECAY] = _f2u(min(f32(ema_decay_max), (f32(1.0) + f32(n)) / (f32(10.0) + f32(n))))
        scale = self.f(SC_SCALE)
        inf = bool(enabled) and w[SC_FOUND] != 0
        w[SC_FOUND] = 0
        w[SC_INV_SCALE] = _f2u(f32(1.0) / scale if enabled else f32(1.0))
        w[SC_SKIP] = 1 if inf else 0
        if inf:
            w[SC_SKIPPED] = (int(w[SC_SKIPPED]) + 1) & 0xFFFFFFFF
            w[SC_SCALE] = _f2u(scale * f32(backoff))
            w[SC_TRACKER] = 0
            return self
        t = (int(w[SC_STEP]) + 1) & 0xFFFFFFFF
        w[SC_STEP] = t
        lr = float(lr_base) * math.pow(0.1, float(t - 1) / float(lr_decay_steps)) if lr_decay_steps > 0.0 else float(lr_base)
        bc1, bc2 = 1.0 - math.pow(float(beta1), float(t)), 1.0 - math.pow(float(beta2), float(t))
        w[SC_LR] = _f2u(lr)
        w[SC_STEP_SIZE] = _f2u(lr / bc1)
        w[SC_INV_BC2] = _f2u(1.0 / math.sqrt(bc2))
        if enabled:
            tr = (int(w[SC_TRACKER]) + 1) & 0xFFFFFFFF
            if tr >= growth_interval:
                w[SC_SCALE] = _f2u(scale * f32(growth))
                w[SC_TRACKER] = 0
            else:
                w[SC_TRACKER] = tr
        return self

    def scalars(self, beta1, beta2, eps):
        """this step's Scalars as nsr_adam_step_scaled reads them from the state"""
        return Scalars(np.float32(beta1), np.float32(beta2), float(eps), self.f(SC_STEP_SIZE), self.f(SC_INV_BC2),
                       self.f(SC_INV_SCALE), self.f(SC_EMA_DECAY), bool(self.words[SC_SKIP]))


def ulp_distance_f32(a_words, b_words):
    """distance in fp32 steps between two finite fp32 values of one sign given as bit patterns"""
    return abs(int(a_words) - int(b_words))


# ---- pure data movement: exact ------------------------------------------------------------------------------------------------------
def lane0_of(lane_mask):
    return {0x3: 0, 0xC: 2}[lane_mask]


def lanes_pack_ref(grad_rows, lane_mask):
    """grad_rows [rows, 4] -> (packed [rows, 2] = the trained lanes, grad_rows afterwards = all zero)"""
    g = np.asarray(grad_rows)
    l0 = lane0_of(lane_mask)
    return g[:, l0:l0 + 2].copy(), np.zeros_like(g)


def lanes_unpack_ref(packed, row_lo, row_hi, lane_mask, arena_rows, half_rows=None):
    """packed [>= row_hi, 2] indexed by global row; arena_rows [rows, 4] f32; half_rows [rows, 4] f16 or None ->
    (arena_rows, half_rows) afterwards: trained lanes of rows [row_lo, row_hi) replaced, all four lanes of those rows cast"""
    a = np.array(arena_rows, np.float32)
    l0 = lane0_of(lane_mask)
    a[row_lo:row_hi, l0:l0 + 2] = np.asarray(packed, np.float32)[row_lo:row_hi]
    h = None
    if half_rows is not None:
        h = np.array(half_rows, np.float16)
        h[row_lo:row_hi] = cast_ref(a[row_lo:row_hi])
    return a, h


def cast_ref(x):
    """fp32 -> f16, round to nearest even, overflow to inf, gradual underflow: NumPy's cast"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(x, np.float32).astype(np.float16)
