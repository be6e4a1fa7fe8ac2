"""tests/optim_ref.py, the reference tests/test_gpu_optim.py judges the optimiser kernels by, tied to torch on the CPU; and the
argument checks of the optimiser entry points, which run before any launch and need no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_ref as R

B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))      # the kernel's fp32 betas, widened
EPS = 1e-15
NSR_OK, NSR_ERR_INVALID_ARG = 0, -1


def _grads(rng, n):
    g = rng.uniform(1e-3, 1.0, n) * rng.choice([-1.0, 1.0], n)
    g[::8] = 0.0
    return g


def test_adam_step_ref_equals_torch_adam_fp64():
    """Five chained steps of adam_step_ref against torch.optim.Adam on float64 tensors with the same betas, the bias
    corrections in double as torch forms them (nothing rounded to fp32).
    Tolerance: both sides make at most the roundings optim_ref counts (torch's lerp and addcdiv make no more), now with
    u = 2^-53: 2 sides.  An error carried in m, v or p enters the next step with a factor <= 1 (beta1, beta2, 1), so after k
    steps k single-step bounds have added up; p also inherits the carried error of m and v through m / denom, another factor
    k.  2 * k * k = 50 at k = 5 times the single-step bound (which holds SAFETY = 2 already): a few tens of fp64 roundings of
    the addends' magnitudes, against a formula error that would show at 1e-8 and more."""
    rng = np.random.default_rng(0)
    n, lr = 257, 1e-2
    p = rng.normal(0, 0.1, n)
    m, v = np.zeros(n), np.zeros(n)
    pt = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([pt], lr=lr, betas=(B1, B2), eps=EPS)
    for t in range(1, 6):
        g = _grads(rng, n)
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
        s = R.Scalars(B1, B2, EPS, lr / bc1, 1.0 / math.sqrt(bc2), 1.0, 0.0)
        r = R.adam_step_ref(p, g, m, v, None, s, 0xF, u=R.U64)
        st = opt.state[pt]
        tol = 2.0 * t * t
        for name, got in (('p', pt.detach().numpy()), ('m', st['exp_avg'].numpy()), ('v', st['exp_avg_sq'].numpy())):
            err = np.abs(r[name] - got)
            assert np.all(err <= tol * r['bound_' + name]), (t, name, float((err / r['bound_' + name]).max()))
        assert np.all(r['g'] == 0.0)
        p, m, v = r['p'], r['m'], r['v']
    assert float(np.abs(p - pt.detach().numpy()).max()) < 1e-15


def test_known_difference_from_torch_with_its_own_betas():
    """torch.optim.Adam(betas=(0.9, 0.999)) holds the betas as doubles; the kernel receives floats.  1 - 0.999f =
    0.00099998713, so after one step from v = 0 the second moment is smaller than torch's by 1.287e-5 relative.  The same
    1 - 0.999f is the bias correction of step 1, so the difference cancels in sqrt(v) / sqrt(bc2) and the parameters agree
    as closely as eps = 1e-15 against |g| >= 1e-3 allows (1e-12 relative to the update, which is lr)."""
    rng = np.random.default_rng(1)
    n, lr = 64, 1e-2
    p = rng.normal(0, 0.1, n)
    g = rng.uniform(1e-3, 1.0, n) * rng.choice([-1.0, 1.0], n)
    pt = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([pt], lr=lr, betas=(0.9, 0.999), eps=EPS)
    pt.grad = torch.tensor(g, dtype=torch.float64)
    opt.step()
    s = R.Scalars(B1, B2, EPS, lr / (1.0 - B1), 1.0 / math.sqrt(1.0 - B2), 1.0, 0.0)
    r = R.adam_step_ref(p, g, np.zeros(n), np.zeros(n), None, s, 0xF)
    rel_v = r['v'] / opt.state[pt]['exp_avg_sq'].numpy() - 1.0
    want = (1.0 - B2) / 0.001 - 1.0
    assert -1.30e-5 < want < -1.28e-5
    assert np.all(np.abs(rel_v - want) < 1e-12)
    rel_m = r['m'] / opt.state[pt]['exp_avg'].numpy() - 1.0           # 1 - 0.9f against 0.1: 2.4e-7 the other way
    assert np.all(np.abs(rel_m - ((1.0 - B1) / (1.0 - 0.9) - 1.0)) < 1e-12)
    assert float(np.abs(r['p'] - pt.detach().numpy()).max()) < 1e-10 * lr


def test_untrained_lanes_and_skipped_step_of_the_reference():
    rng = np.random.default_rng(2)
    n = 11
    p, m, v, e = (rng.normal(0, 1, n).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    g = rng.normal(0, 1, n).astype(np.float32)
    g[1] = np.inf
    g[3] = np.nan                                                   # lanes 1 and 3 are untrained under 0x5
    ss, bc = R.host_scalars_ref(1e-2, 0.9, 0.999, 3)
    s = R.Scalars(np.float32(0.9), np.float32(0.999), EPS, ss, bc, np.float32(0.5), np.float32(0.95))
    r = R.adam_step_ref(p, g, m, v, e, s, 0x5)
    un = ~R.trained_mask(n, 0x5)
    assert list(un[:5]) == [False, True, False, True, False]
    for name, x in (('p', p), ('m', m), ('v', v)):
        assert np.array_equal(r[name][un], x[un].astype(np.float64)) and np.all(r['bound_' + name][un] == 0.0)
        assert np.all(r[name][~un] != x[~un]) and np.all(np.isfinite(r[name]))
    k = float(np.float32(1.0) - np.float32(0.95))
    assert np.array_equal(r['ema'], e - k * (e.astype(np.float64) - r['p']))
    assert np.all(r['ema'] != e)                                    # the shadow of an untrained element moves too
    sk = R.adam_step_ref(p, g, m, v, e, s._replace(skip=True), 0xF)
    assert np.array_equal(sk['p'], p) and np.array_equal(sk['m'], m) and np.array_equal(sk['v'], v) and np.all(sk['g'] == 0)
    assert np.array_equal(sk['ema'], e - k * (e.astype(np.float64) - p))


def test_host_scalars_ref():
    ss, bc = R.host_scalars_ref(1e-2, 0.9, 0.999, 1)
    assert ss == np.float32(float(np.float32(1e-2)) / (1.0 - B1)) and bc == np.float32(1.0 / math.sqrt(1.0 - B2))
    ss, bc = R.host_scalars_ref(1e-2, 0.9, 0.999, 100000)            # both corrections are 1 to the last bit by then
    assert ss == np.float32(1e-2) and bc == np.float32(1.0)
    assert ss.dtype == np.float32 and bc.dtype == np.float32


def test_ema_of_the_reference_is_torch_emas_formula():
    """torch_ema (utils/__init__.py:116-142), restated as tests/test_gpu_render.py restates it: num_updates += 1;
    decay = min(decay, (1 + num_updates) / (10 + num_updates)); shadow.sub_((1 - decay) * (shadow - param)) -- in torch
    float64 against adam_step_ref's shadow with ScalerRef's decay schedule.  ScalerRef holds the decay in fp32 as the kernel
    does: the two agree to the fp32 rounding of the decay (2^-24 of |shadow - param| per step), and exactly when the
    reference is given torch's double."""
    rng = np.random.default_rng(3)
    n = 40
    p = rng.normal(0, 1, n)
    shadow = torch.tensor(p.copy(), dtype=torch.float64)
    e64, e32 = p.copy(), p.copy()
    sc = R.ScalerRef()
    zero = np.zeros(n)
    for it in range(1, 181):                                      # the schedule reaches its cap at update 170
        p = p + rng.normal(0, 0.05, n)
        decay = min(0.95, (1 + it) / (10 + it))
        shadow.sub_((1.0 - decay) * (shadow - torch.tensor(p)))
        s = R.Scalars(B1, B2, EPS, 0.0, 1.0, 1.0, decay, True)        # skip: the parameters are given, only the shadow moves
        e64 = R.adam_step_ref(p, zero, zero, zero, e64, s, 0xF)['ema']
        assert float(np.abs(e64 - shadow.numpy()).max()) <= 4 * R.U64 * 4.0, it
        sc.update(1e-2, 0.0, 0.9, 0.999, ema_decay_max=0.95)
        assert int(sc.words[R.SC_EMA_N]) == it and sc.f(R.SC_EMA_DECAY) == np.float32(decay)
        before = e32
        e32 = R.adam_step_ref(p, zero, zero, zero, e32, sc.scalars(0.9, 0.999, EPS), 0xF)['ema']
        want = before - (1.0 - decay) * (before - p)
        assert np.all(np.abs(e32 - want) <= 2.0 * R.U32 * np.abs(before - p) + 1e-15), it
    assert sc.f(R.SC_EMA_DECAY) == np.float32(0.95)


# 40 steps: infs at tracker 0, at tracker = interval - 1, two in a row, and long clean runs (growth_interval 3)
KINDS = ['ok', 'ok', 'inf', 'inf', 'ok', 'ok', 'ok', 'inf', 'ok', 'ok', 'inf', 'ok', 'ok', 'ok', 'ok', 'ok', 'ok', 'inf', 'ok', 'inf',
         'inf', 'inf', 'ok', 'ok', 'ok', 'ok', 'ok', 'ok', 'ok', 'ok', 'ok', 'inf', 'ok', 'ok', 'inf', 'ok', 'ok', 'ok', 'ok', 'ok']


def test_scaler_ref_equals_lambdalr_adam_and_gradscaler():
    """ScalerRef driven as the trainer drives torch (trainers/base.py:420-426: scaler.step, scaler.update, scheduler.step only
    if the scale did not drop): the LambdaLR value, Adam's step count and bias corrections, and torch.amp.GradScaler's scale
    and growth tracker on CPU tensors (checked where the installed torch runs its GradScaler on the CPU)."""
    assert len(KINDS) == 40
    lr0, decay_steps, gi = 1e-2, 50.0, 3
    lr0_32 = float(np.float32(lr0))
    pt = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    # the kernel receives lr_base as a float: the torch side starts from the same number
    topt = torch.optim.Adam([pt], lr=lr0_32, betas=(B1, B2), eps=EPS)
    sched = torch.optim.lr_scheduler.LambdaLR(topt, lambda it: 0.1 ** (it / decay_steps))
    try:
        tsc = torch.amp.GradScaler('cpu', init_scale=1024.0, growth_interval=gi)
        tsc.scale(torch.zeros(1))
    except Exception:                                               # a torch whose GradScaler needs a device: policy checked below
        tsc = None
    sc = R.ScalerRef(scale=1024.0)
    scale, tracker, steps, skipped = 1024.0, 0, 0, 0
    for it, kind in enumerate(KINDS):
        grad = torch.full((4,), 0.5, dtype=torch.float64)
        if kind == 'inf':
            grad[it % 4] = float('inf') if it % 2 else float('nan')
            sc.set_found()
        pt.grad = grad
        lr_now = sched.get_last_lr()[0]
        if tsc is not None:
            tsc.step(topt)
            old = tsc.get_scale()
            tsc.update()
            took = old <= tsc.get_scale()
        else:
            took = kind != 'inf'
            if took:
                topt.step()
        if took:
            sched.step()
        sc.update(lr0, decay_steps, 0.9, 0.999, 2.0, 0.5, gi, 1, -1.0)
        # GradScaler's policy, restated (torch/amp/grad_scaler.py: _amp_update_scale_)
        if kind == 'inf':
            scale, tracker, skipped = scale * 0.5, 0, skipped + 1
        else:
            steps, tracker = steps + 1, tracker + 1
            if tracker == gi:
                scale, tracker = scale * 2.0, 0
        assert took == (kind != 'inf')
        assert sc.f(R.SC_SCALE) == scale and int(sc.words[R.SC_TRACKER]) == tracker, it
        assert int(sc.words[R.SC_STEP]) == steps and int(sc.words[R.SC_SKIPPED]) == skipped and int(sc.words[R.SC_FOUND]) == 0
        assert int(sc.words[R.SC_SKIP]) == (kind == 'inf')
        if tsc is not None:
            assert tsc.get_scale() == scale and tsc.state_dict()['_growth_tracker'] == tracker, it
        assert int(topt.state[pt]['step']) == steps if steps else True
        if took:
            t = steps
            assert sc.f(R.SC_LR) == np.float32(lr_now), it
            assert sc.f(R.SC_STEP_SIZE) == np.float32(lr_now / (1.0 - B1 ** t)), it
            assert sc.f(R.SC_INV_BC2) == np.float32(1.0 / math.sqrt(1.0 - B2 ** t)), it
    assert skipped == KINDS.count('inf') and steps == 40 - skipped
    assert sc.f(R.SC_INV_SCALE) * sc.f(R.SC_SCALE) in (0.5, 1.0, 2.0)      # 1 / the scale the last gradients carried


def test_scaler_ref_disabled_and_constant_lr():
    sc = R.ScalerRef(scale=1.0)
    sc.set_found()
    sc.update(1e-2, 0.0, 0.9, 0.999, enabled=0, ema_decay_max=-1.0)
    assert sc.f(R.SC_SCALE) == 1.0 and sc.f(R.SC_INV_SCALE) == 1.0 and not sc.words[R.SC_SKIP] and not sc.words[R.SC_FOUND]
    assert int(sc.words[R.SC_STEP]) == 1 and int(sc.words[R.SC_TRACKER]) == 0 and int(sc.words[R.SC_EMA_N]) == 0
    assert sc.f(R.SC_LR) == np.float32(1e-2)
    sc.update(1e-2, -1.0, 0.9, 0.999, enabled=0)
    assert sc.f(R.SC_LR) == np.float32(1e-2) and int(sc.words[R.SC_STEP]) == 2


def test_pack_unpack_and_cast_refs():
    g = np.arange(12, dtype=np.float32).reshape(3, 4)
    pk, z = R.lanes_pack_ref(g, 0xC)
    assert pk.tolist() == [[2, 3], [6, 7], [10, 11]] and not z.any()
    assert R.lanes_pack_ref(g, 0x3)[0].tolist() == [[0, 1], [4, 5], [8, 9]]
    a, h = R.lanes_unpack_ref(-pk, 1, 3, 0x3, g, np.full((3, 4), 7, np.float16))
    assert a.tolist() == [[0, 1, 2, 3], [-6, -7, 6, 7], [-10, -11, 10, 11]]
    assert h.tolist() == [[7, 7, 7, 7], [-6, -7, 6, 7], [-10, -11, 10, 11]]
    x = np.array([2049.0, 2051.0, 65519.996, 65520.0, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), -0.0], np.float32)
    c = R.cast_ref(x)
    assert c[:2].tolist() == [2048.0, 2052.0] and c[2] == 65504.0 and np.isinf(c[3])              # ties to even, overflow
    assert c[4] == 0.0 and c[5] == np.float16(2.0 ** -24) and np.signbit(c[6])                       # subnormal tie, its neighbour


# ---- refusals at the C boundary: argument checks run before any launch ------------------------------------------------------------
@pytest.fixture(scope='module')
def L():
    from nerfstyle_amd import build, _lib
    build.build()
    return _lib.lib()


A = 0x7F0000001000        # a 4096-aligned address nothing dereferences: every call below returns before a launch


def _adam_step(L, ptrs, n=8, step=1, mask=0xF):
    return L.nsr_adam_step(*ptrs, n, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, step, mask, None)


def test_adam_step_refuses_misaligned_pointers_and_step_zero(L):
    good = [A, A + 0x1000, A + 0x2000, A + 0x3000, A + 0x4000, A + 0x5000]
    for slot in range(6):
        ptrs = list(good)
        ptrs[slot] += 4
        assert _adam_step(L, ptrs) == NSR_ERR_INVALID_ARG, slot
    for slot in range(4):                                           # the four required pointers
        ptrs = list(good)
        ptrs[slot] = None
        assert _adam_step(L, ptrs) == NSR_ERR_INVALID_ARG, slot
    assert _adam_step(L, good, step=0) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_adam(A, None, A, A, A, None, A, 0, 4, 0x3, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 0, None) == NSR_ERR_INVALID_ARG


def test_scaled_step_refuses_bad_half_n_and_state(L):
    def call(n, half_n, state=A + 0x6000):
        return L.nsr_adam_step_scaled(A, A, A, A, None, A, n, half_n, 0.9, 0.999, EPS, 0xF, state, None)
    assert call(8, 12) == NSR_ERR_INVALID_ARG                       # half_n > n
    assert call(8, 6) == NSR_ERR_INVALID_ARG                        # half_n & 3
    assert call(7, 8) == NSR_ERR_INVALID_ARG
    for odd in (1, 2, 3):
        assert call(8, 8, A + 0x6000 + odd) == NSR_ERR_INVALID_ARG
        assert L.nsr_grad_check(A, 8, 0xF, A + 0x6000 + odd, None) == NSR_ERR_INVALID_ARG
        assert L.nsr_scaler_update(A + 0x6000 + odd, 1e-2, 0.0, 0.9, 0.999, 2.0, 0.5, 2000, 1, 0.95, None) == NSR_ERR_INVALID_ARG
        assert L.nsr_lanes_adam_scaled(A, None, A, A, A, None, A, 0, 4, 0x3, 0.9, 0.999, EPS, A + 0x6000 + odd, None) == NSR_ERR_INVALID_ARG
    assert call(8, 8, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_scaler_update(None, 1e-2, 0.0, 0.9, 0.999, 2.0, 0.5, 2000, 1, 0.95, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_scaler_update(A, 1e-2, 0.0, 0.9, 0.999, 2.0, 0.5, 0, 1, 0.95, None) == NSR_ERR_INVALID_ARG       # growth_interval 0
    assert L.nsr_grad_check(A + 4, 8, 0xF, A + 0x6000, None) == NSR_ERR_INVALID_ARG


@pytest.mark.parametrize('mask', [0x0, 0x5, 0xF])
def test_lanes_refuse_masks_that_are_no_table(L, mask):
    assert L.nsr_lanes_pack(A, 4, mask, A + 0x1000, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_adam(A, None, A, A, A, None, A, 0, 4, mask, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_adam_scaled(A, None, A, A, A, None, A, 0, 4, mask, 0.9, 0.999, EPS, A + 0x6000, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_unpack(A, 0, 4, mask, A + 0x1000, None, None) == NSR_ERR_INVALID_ARG


def test_lanes_refuse_reversed_ranges_and_misalignment(L):
    assert L.nsr_lanes_adam(A, None, A, A, A, None, A, 5, 4, 0x3, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_adam_scaled(A, None, A, A, A, None, A, 5, 4, 0xC, 0.9, 0.999, EPS, A + 0x6000, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_unpack(A, 5, 4, 0x3, A + 0x1000, None, None) == NSR_ERR_INVALID_ARG
    # arena and ema 16-byte, the packed buffers and the half copy 8-byte
    assert L.nsr_lanes_adam(A + 8, None, A, A, A, None, A, 0, 4, 0x3, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_adam(A, None, A, A, A, A + 8, A, 0, 4, 0x3, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, None) == NSR_ERR_INVALID_ARG
    for slot in (1, 2, 3, 4, 6):
        args = [A, None, A, A, A, None, A]
        args[slot] = A + 4
        assert L.nsr_lanes_adam(*args, 0, 4, 0x3, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, None) == NSR_ERR_INVALID_ARG, slot
    assert L.nsr_lanes_pack(A + 8, 4, 0x3, A, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_pack(A, 4, 0x3, A + 4, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_lanes_unpack(A + 4, 0, 4, 0x3, A, None, None) == NSR_ERR_INVALID_ARG
    assert L.nsr_cast_f32_to_f16(A + 8, A, 8, None) == NSR_ERR_INVALID_ARG


def test_empty_work_is_ok_with_null_pointers(L):
    assert L.nsr_adam_step(None, None, None, None, None, None, 0, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1, 0xF, None) == NSR_OK
    assert L.nsr_adam_step_scaled(None, None, None, None, None, None, 0, 0, 0.9, 0.999, EPS, 0xF, None, None) == NSR_OK
    assert L.nsr_grad_check(None, 0, 0xF, None, None) == NSR_OK
    assert L.nsr_cast_f32_to_f16(None, None, 0, None) == NSR_OK
    assert L.nsr_lanes_pack(None, 0, 0x3, None, None) == NSR_OK
    for lo in (0, 7):
        assert L.nsr_lanes_adam(None, None, None, None, None, None, None, lo, lo, 0xC, 1e-2, 0.9, 0.999, EPS, 1.0, 0.95, 1,
                                None) == NSR_OK
        assert L.nsr_lanes_adam_scaled(None, None, None, None, None, None, None, lo, lo, 0xC, 0.9, 0.999, EPS, None, None) == NSR_OK
        assert L.nsr_lanes_unpack(None, lo, lo, 0x3, None, None, None) == NSR_OK
