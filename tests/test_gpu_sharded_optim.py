"""GPU: ShardedFusedAdam (nerfstyle_amd/sharded_optim.py) against FusedAdam + parallel.sync_gradients, rehearsed on ONE
card: fresh processes (gloo rendezvous, all on cuda:0), each holding two copies of the model fed identical gradients
(seeded per rank and step, copied into both gradient arenas before any reduction).  One copy steps with the all-reduce +
FusedAdam path, the other with the sharded optimiser.

Child processes are started with subprocess (never a re-exec of a process that has touched the GPU)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, SCALE = 1e-2, 1024.0

CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["NSR_ROOT"])
import torch
from nerfstyle_amd import parallel as P
torch.cuda.set_device(0)
os.environ["NSR_BENCH_DEVICE"] = "0"
rank, local_rank, world = P.init(backend="gloo", seed=11)
dev = torch.device("cuda", 0)
from nerfstyle_amd import checkpoint as C
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.optim import FusedAdam, LossScaler
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_room_cameras
from nerfstyle_amd.sharded_optim import ShardedFusedAdam
from nerfstyle_amd.style_nerf import StyleTCNerf
E = os.environ
kw = None if E["NSR_SET"] == "recon" else ["x_color_embedder"]
tdt = None if E["NSR_TDT"] == "f16" else torch.float32
scaled = E["NSR_PATH"] == "scaler"
mode = E.get("NSR_MODE", "compare")
steps = [int(s) for s in E["NSR_STEPS"].split(",")]
inf_step, inf_rank = int(E.get("NSR_INF_STEP", -1)), int(E.get("NSR_INF_RANK", -1))
LR, SCALE, DECAY = 1e-2, 1024.0, 500.0
_, intr, _ = load_room_cameras()

def make():
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=tdt, use_dir=False).to(dev)
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=8, samples_per_ray_cap=256).to(dev)
    return m, r

def grad_of(step, rk, n):
    # rank- and step-keyed: a resumed run regenerates the same gradients
    g = torch.Generator(device=dev).manual_seed(1000 * step + rk)
    x = torch.randn(n, generator=g, device=dev) * (torch.rand(n, generator=g, device=dev) < 0.5)
    return x * (1e-3 * SCALE)

def snapshot(m, opt, sc):
    half = m.half_tables().detach().cpu().clone() if m.table_dtype == torch.float16 else None
    sd = opt.state_dict()                                         # collective for the sharded optimiser
    return {"arena": m.arena.detach().cpu().clone(), "half": half, "exp_avg": sd["exp_avg"].cpu(), "exp_avg_sq": sd["exp_avg_sq"].cpu(),
            "ema": sd["ema"].cpu(), "step": torch.tensor(sd["step"]), "ema_updates": torch.tensor(sd["ema_updates"]),
            "scaler": sc.state.cpu().clone() if sc is not None else None}

def run_steps(pairs, todo):
    zero = []
    for it in todo:
        g = grad_of(it, rank, pairs[0][0].arena.numel())
        if it == inf_step and rank == inf_rank:
            g[4 * 3 + 2] = float("inf")      # colour lane of row 3: rank 0's shard in both sets -- it reaches rank 0 via the reduction
        for (m, r, opt, sc) in pairs:
            m._ensure_grad().copy_(g)
        for (m, r, opt, sc) in pairs:
            if isinstance(opt, FusedAdam):
                P.sync_gradients(m, optimizer=opt)
            elif it % 2:
                opt.reduce_gradients_async().wait()
            if scaled:
                opt.step(scaler=sc, lr_decay_steps=DECAY)
            else:
                opt.step(grad_scale=SCALE)
        zero.append(all(bool((m.grad_arena == 0).all()) for (m, _, _, _) in pairs))
    return zero

out = {}
if mode == "compare" or mode == "ckpt":
    ma, ra = make()
    ms, rs = make()
    init = ma.arena.detach().cpu().clone()
    oa = FusedAdam(ma, lr=LR, keywords=kw, ema_decay=0.95)
    os_ = ShardedFusedAdam(ms, lr=LR, keywords=kw, ema_decay=0.95)
    pairs = [(ma, ra, oa, LossScaler(init_scale=SCALE) if scaled else None), (ms, rs, os_, LossScaler(init_scale=SCALE) if scaled else None)]
    if mode == "ckpt":
        zero = run_steps(pairs, steps[:-1])
        gathered = os_.gathered()                                 # collective: every rank
        if rank == 0:
            C.save_checkpoint(E["NSR_OUT"] + ".all_reduce.ckpt", ra, optim=oa, scaler=pairs[0][3], iter_ctr=7)
            C.save_checkpoint(E["NSR_OUT"] + ".sharded.ckpt", rs, optim=gathered, scaler=pairs[1][3], iter_ctr=7)
        zero += run_steps(pairs, steps[-1:])
    else:
        zero = run_steps(pairs, steps)
    out = {"a": snapshot(ma, oa, pairs[0][3]), "s": snapshot(ms, os_, pairs[1][3]), "init": init, "zero": torch.tensor(zero),
           "exp_avg_numel": torch.tensor(os_.exp_avg.numel()), "chunk": torch.tensor(os_.geo.chunk)}
elif mode == "resume":
    ms, rs = make()
    os_ = ShardedFusedAdam(ms, lr=LR, keywords=kw, ema_decay=0.95)
    sc = LossScaler(init_scale=SCALE)
    assert C.restore(C.load_checkpoint(E["NSR_CKPT"]), rs, optim=os_, scaler=sc) == 7
    zero = run_steps([(ms, rs, os_, sc)], steps)
    out = {"s": snapshot(ms, os_, sc), "zero": torch.tensor(zero)}
elif mode == "resume_fused":
    # world 1: the sharded run's file into a plain FusedAdam; its step on the summed gradients of both ranks
    ma, ra = make()
    oa = FusedAdam(ma, lr=LR, keywords=kw, ema_decay=0.95)
    sc = LossScaler(init_scale=SCALE)
    sd = C.load_checkpoint(E["NSR_CKPT"])
    assert C.restore(sd, ra, optim=oa, scaler=sc) == 7
    loaded = snapshot(ma, oa, None)
    for it in steps:
        n = ma.arena.numel()
        ma._ensure_grad().copy_(grad_of(it, 0, n) + grad_of(it, 1, n))
        oa.step(scaler=sc, lr_decay_steps=DECAY)
    out = {"loaded": loaded, "a": snapshot(ma, oa, sc)}
torch.cuda.synchronize()
torch.save(out, E["NSR_OUT"])
P.barrier()
print("CHILD_OK", rank, world)
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(tmp_path, world, tag, **env):
    script = tmp_path / 'child_sharded.py'
    script.write_text(CHILD)
    port = _free_port()
    procs = []
    for rank in range(world):
        e = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                 MASTER_PORT=str(port), NSR_ROOT=ROOT, NSR_OUT=str(tmp_path / '{}_{}.pt'.format(tag, rank)), OMP_NUM_THREADS='2',
                 **{k: str(v) for k, v in env.items()})
        procs.append(subprocess.Popen([sys.executable, str(script)], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out[-3000:]
        assert 'CHILD_OK {} {}'.format(rank, world) in out
    return [torch.load(tmp_path / '{}_{}.pt'.format(tag, rank), weights_only=True) for rank in range(world)]


KEYS = ('arena', 'half', 'exp_avg', 'exp_avg_sq', 'ema', 'step', 'ema_updates', 'scaler')


def _equal(x, y, keys=KEYS):
    for k in keys:
        if x[k] is None or y[k] is None:
            assert x[k] is None and y[k] is None, k
        else:
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize('tdt', ['f16', 'f32'])
@pytest.mark.parametrize('path', ['scaler', 'host'])
@pytest.mark.parametrize('which', ['recon', 'style'])
def test_world_one_equals_fused_adam_bitwise(tmp_path, which, path, tdt):
    (d,) = _run(tmp_path, 1, 'w1', NSR_SET=which, NSR_TDT=tdt, NSR_PATH=path, NSR_STEPS='0,1,2')
    _equal(d['a'], d['s'])
    assert bool(d['zero'].all())
    assert not torch.equal(d['s']['arena'], d['init'])                   # the steps did train
    assert int(d['exp_avg_numel']) == int(d['chunk'])


def _world_two(tmp_path, which):
    a, b = _run(tmp_path, 2, which, NSR_SET=which, NSR_TDT='f16', NSR_PATH='scaler', NSR_STEPS='0,1,2,3', NSR_INF_STEP=2,
                NSR_INF_RANK=1)
    for d in (a, b):
        _equal(d['s'], d['a'])                                          # = the all-reduce copy (two addends: order-free)
        assert bool(d['zero'].all())                                    # gradient arena all zero after every step
        assert int(d['s']['scaler'][4]) == 1 and int(d['s']['scaler'][3]) == 3      # both ranks skipped step 2, took 3 steps
    _equal(a['s'], b['s'])                                              # replicas bit-identical
    return a, b


def test_world_two_reconstruction_set_with_inf_on_one_rank(tmp_path):
    a, _ = _world_two(tmp_path, 'recon')
    assert int(a['chunk']) * 2 >= a['s']['arena'].numel() and int(a['exp_avg_numel']) == int(a['chunk'])
    assert int(a['chunk']) < a['s']['arena'].numel()


def test_world_two_stylisation_set_with_inf_on_one_rank(tmp_path):
    a, _ = _world_two(tmp_path, 'style')
    te = a['init'].numel() - 15360
    t0, t1 = a['init'][:te].view(-1, 2, 2), a['s']['arena'][:te].view(-1, 2, 2)
    assert torch.equal(t0[:, 0], t1[:, 0])                              # density lanes untouched
    assert torch.equal(a['init'][te:], a['s']['arena'][te:])            # MLP parameters untouched
    assert not torch.equal(t0[:, 1], t1[:, 1])
    assert int(a['exp_avg_numel']) == int(a['chunk']) and int(a['chunk']) * 2 >= 2 * (te // 4)


def test_world_three_uneven_padded_shards(tmp_path):
    ds = _run(tmp_path, 3, 'w3', NSR_SET='recon', NSR_TDT='f16', NSR_PATH='scaler', NSR_STEPS='0,1,2')
    for d in ds[1:]:
        _equal(ds[0]['s'], d['s'])                                      # replicas bit-identical
    n = ds[0]['s']['arena'].numel()
    c = int(ds[0]['chunk'])
    assert c % 16 == 0 and 3 * c >= n and 3 * c - n < 48
    for d in ds:
        assert int(d['exp_avg_numel']) == c and bool(d['zero'].all())
    # against the all-reduce copy: three addends, fp32 summation order (gloo's all-reduce and reduce-scatter may add in
    # different orders); Adam's sign-like steps on ~0 gradients are the only large differences
    s, r = ds[0]['s'], ds[0]['a']
    assert torch.equal(s['step'], r['step']) and torch.equal(s['scaler'], r['scaler'])
    d = (s['arena'] - r['arena']).abs()
    f6, f3 = float((d > 1e-6).float().mean()), float((d > 1e-3).float().mean())
    rel = float(d.double().norm() / (r['arena'] - ds[0]['init']).double().norm())
    print('world 3 vs all-reduce: frac>1e-6 {:.2e}, frac>1e-3 {:.2e}, rel-L2 of the update {:.2e}'.format(f6, f3, rel))
    assert f6 < 1e-3 and f3 < 1e-4 and rel < 1e-3, (f6, f3, rel)
    for k in ('exp_avg', 'exp_avg_sq', 'ema'):
        dk = (s[k] - r[k]).abs()
        assert float(dk.max()) <= 1e-4 * float(r[k].abs().max()) + 1e-6, k


def test_checkpoint_through_gathered_and_restore(tmp_path):
    a, b = _run(tmp_path, 2, 'ck', NSR_SET='recon', NSR_TDT='f16', NSR_PATH='scaler', NSR_STEPS='0,1,2', NSR_MODE='ckpt')
    _equal(a['s'], a['a'])
    base = str(tmp_path / 'ck_0.pt')
    fs = torch.load(base + '.sharded.ckpt', weights_only=True)
    fa = torch.load(base + '.all_reduce.ckpt', weights_only=True)

    def same(x, y, where):
        assert type(x) is type(y), where
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and torch.equal(x, y), where
        elif isinstance(x, dict):
            assert x.keys() == y.keys(), where
            for k in x:
                same(x[k], y[k], where + '.' + k)
        elif isinstance(x, (list, tuple)):
            assert len(x) == len(y), where
            for i, (u, v) in enumerate(zip(x, y)):
                same(u, v, '{}[{}]'.format(where, i))
        else:
            assert x == y, where
    same(fs, fa, 'ckpt')
    assert fs['optim']['exp_avg'].numel() == a['s']['arena'].numel() and fs['ema']['shadow'].numel() == a['s']['arena'].numel()
    # a fresh world-2 sharded run restored from the file, one step: equals the uninterrupted run bit for bit
    ra, rb = _run(tmp_path, 2, 'rs', NSR_SET='recon', NSR_TDT='f16', NSR_PATH='scaler', NSR_STEPS='2', NSR_MODE='resume',
                  NSR_CKPT=base + '.sharded.ckpt')
    for d in (ra, rb):
        _equal(d['s'], a['s'])
        assert bool(d['zero'].all())
    # the same file into a world-1 FusedAdam: the state it loads is the file's, and its step equals the world-2 run's
    (w1,) = _run(tmp_path, 1, 'f1', NSR_SET='recon', NSR_TDT='f16', NSR_PATH='scaler', NSR_STEPS='2', NSR_MODE='resume_fused',
                 NSR_CKPT=base + '.sharded.ckpt')
    for k in ('exp_avg', 'exp_avg_sq', 'ema'):
        assert torch.equal(w1['loaded'][k], fs['optim'][k]), k
    _equal(w1['a'], a['s'])
