"""Timing of the drawn rollouts (include/bsig_sim_draws.h, csrc/sim.h with csrc/sim_draws.h) for
profiles/sim_draws_NOTES.md, by the method of tools/sim_policy_timing.py: HIP events for launches (a warm-up, median
and range of REPS repeats of INNER launches between two events, the variants of a comparison alternating in one
process, no read-back), the wall clock around a synchronised call for whole calls (median and range of WALL
repeats).

    python tools/sim_draws_timing.py [--parent PATH/libbsig_hip.so] [--quick]

Per task (Pendulum, CartPole), N = 32 000 and 100 000, T = 50 and 200:
  1. the RandomState path, ``cartpole_pairs`` / ``pendulum_pairs(device='cuda')``, whole and split: the host draws
     (the calls of that function on ``RandomState``, in its order; closed loop for CartPole: replace marks,
     replacement actions and the Gaussian, three [N, T] double arrays), their copy to the device, and the double
     launch on the copied arrays with the two roundings to fp32 behind it.  ``pendulum_pairs`` steps on the host:
     its whole call is the host loop; the split restates its draws in front of the device rollout.
  2. ``draw_pairs`` for the same shape (one fp32 launch, nothing drawn or copied), whole, and the
     ``rollout_drawn`` call inside it between two events: the launch with its five output allocations and the
     binding (the launch alone on preallocated buffers is the `drawn` column of 3).
  3. the drawn launch against ``bsig_sim_rollout_policy`` (without a policy: ``bsig_sim_rollout``) fed that
     launch's own recordings, already on the device: the kernel-only cost or gain of drawing in registers instead
     of loading; fp32 and double; no policy, the linear feedback () and a (64,) tanh policy; frac_rnd 0.3,
     noise_std 0.3, terminate off.  The outputs are compared bit for bit first.
  4. ``--parent``: the library built from the PARENT commit (BSIG_OUT_DIR=... ./build.sh in a checkout of it), loaded
     next to this commit's in the same process: its ``bsig_sim_rollout*`` and ``bsig_sim_rollout_policy*`` against
     this commit's on the same inputs, outputs compared bit for bit first, with the run-to-run spread,
     (max - min) / median of the parent's launches, beside the ratio.
``--quick``: N = 32 000 and T = 50 only."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed
from tools.sim_policy_timing import seeded_policy

INNER = 4
WALL = 5
COUNTS = (32000, 100000)
STEPS = (50, 200)
FRAC, STD, SEED = 0.3, 0.3, 7
F32, F64 = torch.float32, torch.float64


def parent_library(path):
    """The parent commit's build with the prototypes of the entry points it shares with this commit."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for header in ('bsig_sim.h', 'bsig_sim_policy.h'):
        for name, (res, args) in B._lib.HEADERS[header].items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(lib, 'bsig_sim_rollout_drawn'), 'this is not the parent commit: it has the drawn entry points'
    return lib


def wall(fn, reps=WALL):
    """(median, min, max) ms of a call with the device idle before and after."""
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), min(times), max(times)


def task_bounds(task):
    lows, highs, init_lows, init_highs, act_low, act_high = B.pairs._DRAW_PAIRS[task]
    if task == 'cartpole':
        lows, highs = lows + (1.0,), highs + (1.0,)
    return dict(lows=lows, highs=highs, init_lows=init_lows, init_highs=init_highs, act_low=act_low, act_high=act_high)


def host_path(task, n, steps, policy):
    """1: the RandomState path, whole and split.  -> the lines' numbers, in ms."""
    pairs = B.pairs

    def draws():
        rs = np.random.RandomState(SEED)
        if task == 'pendulum':
            theta = rs.uniform(np.array([0.01, 0.01]), np.array([2.0, 2.0]), size=(n, 2))
            init = np.column_stack([rs.uniform(-np.pi, np.pi, size=n), rs.uniform(-1.0, 1.0, size=n)])
            acts = np.stack([rs.rand(n) for _ in range(steps)], axis=1)
            return theta, init, acts[:, :, None], None
        theta = rs.uniform(np.array([0.1, 0.1]), np.array([2.0, 2.0]), size=(n, 2))
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
        replace = rs.uniform(size=(n, steps)) < FRAC
        instead = rs.uniform(-1.0, 1.0, size=(n, steps))
        acts = np.where(replace, instead, STD * rs.standard_normal((n, steps)))
        return np.column_stack([theta, np.full(n, 1.0)]), init, acts[:, :, None], replace

    arrays = draws()
    to_dev = lambda: [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
                      for a in arrays]
    on_dev = to_dev()

    def launch():
        s, a, l = pairs.rollout(task, on_dev[0], on_dev[1], on_dev[2], n_steps=steps, dtype=F64,
                                policy=policy if task == 'cartpole' else None, replace=on_dev[3])
        return on_dev[0].float(), s.float(), a.float()
    if task == 'pendulum':
        whole = lambda: pairs.pendulum_pairs(n, steps, seed=SEED, device=DEV)      # noqa: E731
    else:
        whole = lambda: pairs.cartpole_pairs(n, steps, policy=policy, seed=SEED, device=DEV, frac_rnd=FRAC,      # noqa: E731
                                             noise_std=STD)
    return dict(whole=wall(whole), draws=wall(draws), copy=wall(to_dev), launch=wall(launch))


def drawn_path(task, n, steps, policy):
    """2: draw_pairs whole, and the rollout_drawn call inside it (events; allocations and binding included)."""
    pairs = B.pairs
    kw = dict(policy=policy, frac_rnd=FRAC, noise_std=STD) if task == 'cartpole' else {}
    whole = wall(lambda: pairs.draw_pairs(task, n, steps, SEED, device=DEV, **kw))
    draws = pairs.EpisodeDraws(SEED, frac_rnd=FRAC if kw else 0.0, noise_std=STD if kw else 0.0, **task_bounds(task))
    fn = lambda: pairs.rollout_drawn(task, n, steps, draws, policy=kw.get('policy'), device=DEV)      # noqa: E731
    res = timed({'launch': lambda: [fn() for _ in range(INNER)]})
    return whole, tuple(v / INNER / 1e3 for v in res['launch'])


def kernel_variants(task, n, steps, dtype, policy, parent):
    """3 and 4: {name: launch()} on preallocated buffers, and the outputs by name."""
    _lib, lib = B._lib, B._lib.load()
    prec = _lib.F64 if dtype == F64 else _lib.F32
    pd, idim, sd = B.pairs.SIM_DIMS[task]
    ptr, st, tid = _lib.ptr, _lib.stream(), _lib.SIM_TASKS[task]
    draws = B.pairs.EpisodeDraws(SEED, frac_rnd=FRAC, noise_std=STD, **task_bounds(task))
    theta, init, _, _, _, explore, replace = B.pairs.rollout_drawn(task, n, steps, draws, policy=policy, dtype=dtype,
                                                                   device=DEV, record=True)
    dbl = lambda v: (_lib.f64 * len(v))(*np.asarray(v, dtype=np.float64).tolist())      # noqa: E731
    bounds = [dbl(b) for b in (draws.lows, draws.highs, draws.init_lows, draws.init_highs)]
    hidden = (policy.hidden if policy is not None else ()) + (0, 0)
    packed = None if policy is None else ptr(policy.packed_on(DEV))
    act = _lib.SIM_ACTIVATIONS[policy.activation] if policy is not None else 0
    outs, fns = {}, {}

    def buffers(name, extra=False):
        outs[name] = [torch.empty(n, steps + 1, sd, dtype=dtype, device=DEV),
                      torch.empty(n, steps + 1, 1, dtype=dtype, device=DEV),
                      torch.empty(n, dtype=torch.int32, device=DEV)]
        more = [torch.empty(n, pd, dtype=dtype, device=DEV), torch.empty(n, idim, dtype=dtype, device=DEV)] if extra else []
        outs[name + '/theta'] = more
        return [ptr(x) for x in more + outs[name]]

    po, io, s, a, l = buffers('drawn', True)
    fns['drawn'] = lambda: prec.sim_rollout_drawn(tid, None, None, *bounds, draws.act_low, draws.act_high, FRAC, STD,
                                                  SEED, 0, packed, len(hidden) - 2, hidden[0], hidden[1], act, po, io,
                                                  s, a, l, None, None, n, steps, 0, None, st)

    def fed(which, name):
        s, a, l = buffers(name)
        suffix = '_f64' if prec.itemsize == 8 else ''
        if policy is None:
            fn = getattr(which, 'bsig_sim_rollout' + suffix)
            return lambda: _lib.check(fn(tid, ptr(theta), ptr(init), ptr(explore), s, a, l, n, steps, steps, 0, None, st))
        fn = getattr(which, 'bsig_sim_rollout_policy' + suffix)
        return lambda: _lib.check(fn(tid, ptr(theta), ptr(init), ptr(explore), ptr(replace), packed, len(hidden) - 2,
                                     hidden[0], hidden[1], act, s, a, l, n, steps, steps, 0, None, st))
    fns['fed'] = fed(lib, 'fed')
    if parent is not None:
        fns['parent'] = fed(parent, 'parent')
    keep = (theta, init, explore, replace, bounds, policy)
    return fns, outs, keep


def main(argv):
    parent = parent_library(argv[argv.index('--parent') + 1]) if '--parent' in argv else None
    counts, steps_list = ((COUNTS[:1], STEPS[:1]) if '--quick' in argv else (COUNTS, STEPS))
    print('# csrc: %s' % csrc_hash())
    print('# %s; launches: %d repeats of %d, us per launch, median (min .. max); whole calls: %d repeats, ms'
          % (torch.cuda.get_device_name(0), REPS, INNER, WALL))
    fmt = '%.2f (%.2f .. %.2f)'
    for task in ('pendulum', 'cartpole'):
        balance = B.pairs.linear_feedback(B.pairs.CARTPOLE_BALANCE_GAINS).to(DEV) if task == 'cartpole' else None
        for n in counts:
            for steps in steps_list:
                head = '%s N %d T %d' % (task, n, steps)
                host = host_path(task, n, steps, balance)
                whole, launch = drawn_path(task, n, steps, balance)
                print('%s: RandomState path, ms: whole %s = host draws %s + copy %s + launch and rounding %s'
                      % ((head,) + tuple(fmt % host[k] for k in ('whole', 'draws', 'copy', 'launch'))), flush=True)
                print('    draw_pairs, ms: whole %s, the rollout_drawn call in it %s; whole / RandomState whole %.4f'
                      % (fmt % whole, fmt % launch, whole[0] / host['whole'][0]), flush=True)
                for dtype in (F32, F64):
                    for name, policy in (('open', None), ('()', seeded_policy(task, ())),
                                         ('(64,)', seeded_policy(task, (64,)))):
                        fns, outs, keep = kernel_variants(task, n, steps, dtype, policy, parent)
                        for fn in fns.values():
                            fn()
                        torch.cuda.synchronize()
                        same = all(torch.equal(x, y) for x, y in zip(outs['drawn'], outs['fed']))
                        res = timed({k: (lambda fn=fn: [fn() for _ in range(INNER)]) for k, fn in fns.items()})
                        res = {k: tuple(v / INNER for v in r) for k, r in res.items()}
                        line = ('    %s %-5s us: drawn %.1f (%.1f .. %.1f), fed %.1f (%.1f .. %.1f), drawn / fed %.3f, '
                                'bitwise equal: %s' % (('fp64' if dtype == F64 else 'fp32', name) + res['drawn']
                                                       + res['fed'] + (res['drawn'][0] / res['fed'][0], same)))
                        if parent is not None:
                            par = res['parent']
                            same = all(torch.equal(x, y) for x, y in zip(outs['parent'], outs['fed']))
                            line += ('; parent %.1f (%.1f .. %.1f), spread %.1f %%, fed / parent %.3f, bitwise equal: %s'
                                     % (par + (100.0 * (par[2] - par[1]) / par[0], res['fed'][0] / par[0], same)))
                        print(line, flush=True)
                        del fns, outs, keep
                        torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1:])
