"""Timing of the closed-loop rollout kernel (include/bsig_sim_policy.h, csrc/sim.h with csrc/sim_policy.h) for
profiles/sim_policy_NOTES.md, by the method of tools/ragged_timing.py: HIP events, a warm-up, median and range of
REPS repeats of INNER launches between two events, the variants of a comparison alternating in one process; no
read-back in any of them.

    python tools/sim_policy_timing.py [--parent PATH/libbsig_hip.so] [--quick]

Per task (Pendulum, CartPole), N = 32 000 and 100 000, T = 50 and 200 (Ta = T), fp32 and double data, on the same
seeded inputs:
  open      bsig_sim_rollout*, the open-loop launch;
  copy      bsig_copy_rows* moving the bytes the rollout reads and writes (params, init, actions in; states,
            actions_out, lengths out): a copy of half of them, read once and written once;
  () / (64,) / (64, 64)   bsig_sim_rollout_policy* under a seeded tanh policy of that hidden shape, e = the
            actions scaled by 0.1, no replace marks, terminate 0 (every thread evaluates every step).
Per policy launch the table gives the time, its ratio to the open-loop launch, and the double multiplies and adds
the definition asks for (2 per term and one add, counted from the shapes by ``policy_ops``) per second.

``--parent``: the library built from the PARENT commit (BSIG_OUT_DIR=... ./build.sh in a checkout of it), loaded
next to this commit's in the same process: its bsig_sim_rollout* against this commit's on the same inputs,
outputs compared bit for bit first, with the run-to-run spread, (max - min) / median of the parent's launches,
beside the ratio.  ``--quick``: N = 32 000 and T = 50 only."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

INNER = 4
COUNTS = (32000, 100000)
STEPS = (50, 200)
HIDDEN = ((), (64,), (64, 64))


def policy_ops(sd, hidden):
    """The double operations of one evaluation of a_t = pi(o_t) + e_t: a multiply and an add per term, one add."""
    widths = (sd,) + tuple(hidden) + (1,)
    return 2 * sum(a * b for a, b in zip(widths[:-1], widths[1:])) + 1


def parent_library(path):
    """The parent commit's build with the prototypes of the two open-loop entry points."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ('bsig_sim_rollout', 'bsig_sim_rollout_f64'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = B._lib.HEADERS['bsig_sim.h'][name]
    assert not hasattr(lib, 'bsig_sim_rollout_policy'), 'this is not the parent commit: it has the policy entry points'
    return lib


def seeded_policy(task, hidden):
    rs = np.random.RandomState(0)
    widths = (B.pairs.SIM_DIMS[task][2],) + tuple(hidden) + (1,)
    weights = [rs.uniform(-1, 1, size=(b, a)) / np.sqrt(a) for a, b in zip(widths[:-1], widths[1:])]
    biases = [rs.uniform(-0.1, 0.1, size=b) for b in widths[1:]]
    return B.pairs.MLPPolicy(weights, biases, 'tanh').to(DEV)


def variants(task, n, steps, dtype, parent):
    """{name: launch()}, the outputs by name, the bytes a rollout moves, what the launches share."""
    _lib, lib = B._lib, B._lib.load()
    prec = _lib.F64 if dtype == torch.float64 else _lib.F32
    pd, idim, sd = B.pairs.SIM_DIMS[task]
    rs = np.random.RandomState(1)
    params = torch.from_numpy(rs.uniform(0.1, 2.0, size=(n, pd))).to(dtype).to(DEV)
    if task == 'pendulum':
        init = np.column_stack([rs.uniform(-np.pi, np.pi, n), rs.uniform(-1.0, 1.0, n)])
    else:
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
    init = torch.from_numpy(init).to(dtype).to(DEV)
    actions = torch.from_numpy(rs.uniform(-1.0, 1.0, size=(n, steps, 1))).to(dtype).to(DEV)
    noise = (0.1 * actions).contiguous()
    ptr, st, tid = _lib.ptr, _lib.stream(), _lib.SIM_TASKS[task]
    outs, fns = {}, {}

    def buffers(name):
        outs[name] = (torch.empty(n, steps + 1, sd, dtype=dtype, device=DEV),
                      torch.empty(n, steps + 1, 1, dtype=dtype, device=DEV),
                      torch.empty(n, dtype=torch.int32, device=DEV))
        return [ptr(x) for x in outs[name]]

    def open_loop(which, name):
        fn = getattr(which, 'bsig_sim_rollout' + ('_f64' if prec.itemsize == 8 else ''))
        s, a, l = buffers(name)
        return lambda: _lib.check(fn(tid, ptr(params), ptr(init), ptr(actions), s, a, l, n, steps, steps, 0, None, st))

    fns['open'] = open_loop(lib, 'open')
    if parent is not None:
        fns['parent'] = open_loop(parent, 'parent')
    nbytes = prec.itemsize * n * (pd + idim + steps + (steps + 1) * (sd + 1)) + 4 * n
    cols = nbytes // (2 * prec.itemsize * n)
    src = torch.zeros(n, cols, dtype=dtype, device=DEV)
    dst = torch.empty_like(src)
    fns['copy'] = lambda: prec.copy_rows(ptr(src), cols, None, ptr(dst), cols, n, cols, st)
    policies = []
    for hidden in HIDDEN:
        policy = seeded_policy(task, hidden)
        widths = tuple(hidden) + (0, 0)
        s, a, l = buffers(hidden)
        fns[hidden] = (lambda policy=policy, widths=widths, nh=len(hidden), s=s, a=a, l=l:
                       prec.sim_rollout_policy(tid, ptr(params), ptr(init), ptr(noise), None,
                                               ptr(policy.packed_on(DEV)), nh, widths[0], widths[1],
                                               _lib.SIM_ACTIVATIONS['tanh'], s, a, l, n, steps, steps, 0, None, st))
        policies.append(policy)
    keep = (params, init, actions, noise, src, dst, policies)
    return fns, outs, nbytes, keep


def main(argv):
    parent = parent_library(argv[argv.index('--parent') + 1]) if '--parent' in argv else None
    counts, steps_list = ((COUNTS[:1], STEPS[:1]) if '--quick' in argv else (COUNTS, STEPS))
    print('# csrc: %s' % csrc_hash())
    print('# %s, %d repeats of %d launches; us per launch: median (min .. max)'
          % (torch.cuda.get_device_name(0), REPS, INNER))
    for task in ('pendulum', 'cartpole'):
        sd = B.pairs.SIM_DIMS[task][2]
        for n in counts:
            for steps in steps_list:
                for dtype in (torch.float32, torch.float64):
                    fns, outs, nbytes, keep = variants(task, n, steps, dtype, parent)
                    for fn in fns.values():
                        fn()
                    torch.cuda.synchronize()
                    assert all(torch.isfinite(o[0]).all() for o in outs.values())
                    res = timed({k: (lambda fn=fn: [fn() for _ in range(INNER)]) for k, fn in fns.items()})
                    res = {k: tuple(v / INNER for v in r) for k, r in res.items()}
                    head = '%s N %d T %d %s' % (task, n, steps, 'fp64' if dtype == torch.float64 else 'fp32')
                    print('%s: open %.1f (%.1f .. %.1f); copy of the same %.1f MB %.1f (%.1f .. %.1f), %.2f TB/s'
                          % ((head,) + res['open'] + (nbytes / 1e6,) + res['copy'] + (nbytes / res['copy'][0] / 1e6,)),
                          flush=True)
                    if parent is not None:
                        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
                                   for x, y in zip(outs['parent'], outs['open']))
                        par = res['parent']
                        print('    parent %.1f (%.1f .. %.1f), spread %.1f %%; open / parent %.3f; bitwise equal: %s'
                              % (par + (100.0 * (par[2] - par[1]) / par[0], res['open'][0] / par[0], same)), flush=True)
                    for hidden in HIDDEN:
                        med = res[hidden][0]
                        ops = policy_ops(sd, hidden) * float(n) * steps
                        print('    policy %-9s %.1f (%.1f .. %.1f), %.2f x open, %d operations a thread-step, '
                              '%.2f T double operations/s'
                              % ((str(hidden),) + res[hidden] + (med / res['open'][0], policy_ops(sd, hidden),
                                                                 ops / med / 1e6)), flush=True)
                    del fns, outs, keep
                    torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1:])
