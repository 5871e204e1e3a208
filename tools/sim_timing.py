"""Timing of the rollout kernel (include/bsig_sim.h, csrc/sim.h) for profiles/sim_NOTES.md, by the method of
tools/signature_ex_timing.py: HIP events, a warm-up, median and range of REPS repeats, the kernels of a comparison
alternating in one process.  N = 32 000 and 100 000 episodes, T = 20, 50, 200, both tasks, fp32 and double outputs.
  (i)  the rollout launch (bsig_sim_rollout / _f64 on buffers made once, terminate = 0, no flag) next to
       (a) copy_rows writing the same output bytes, N rows of (T + 1) (sd + 1) elements, in the same process: the
           floor the stores can reach (it reads as many bytes as it writes; the rollout reads almost none);
       (b) what a user does without the kernel: the host path of pairs.rollout on the same draws (numpy, double,
           a Python loop over the steps) plus the copy of its three outputs to the device; wall clock, the median
           of HOST_REPS runs.
  (ii) --one TASK fp32|fp64 N T: that launch alone, five times, for a profiler run."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

COUNTS = (32000, 100000)
STEPS = (20, 50, 200)
HOST_REPS = 3


def draws(task, n, steps):
    """fp32 parameters in [0.1, 2], the task's own initial states, actions in [-1, 1), as cartpole_pairs and
    pendulum_pairs draw them."""
    rs = np.random.RandomState(0)
    pd = B.pairs.SIM_DIMS[task][0]
    params = rs.uniform(0.1, 2.0, size=(n, pd))
    if task == 'pendulum':
        init = np.column_stack([rs.uniform(-np.pi, np.pi, n), rs.uniform(-1.0, 1.0, n)])
    else:
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
    actions = rs.uniform(-1.0, 1.0, size=(n, steps, 1))
    return [torch.from_numpy(x).float() for x in (params, init, actions)]


def launcher(task, host, steps, dtype):
    """The one library call on buffers made once -> (fn, output elements per episode)."""
    prec = B._lib.F64 if dtype == torch.float64 else B._lib.F32
    n, sd = host[0].shape[0], B.pairs.SIM_DIMS[task][2]
    params, init, actions = (x.to(DEV).to(dtype).contiguous() for x in host)
    states = torch.empty(n, steps + 1, sd, dtype=dtype, device=DEV)
    acts = torch.empty(n, steps + 1, 1, dtype=dtype, device=DEV)
    lengths = torch.empty(n, dtype=torch.int32, device=DEV)
    keep = (params, init, actions, states, acts, lengths)

    def fn(keep=keep):
        prec.sim_rollout(B._lib.SIM_TASKS[task], *(B._lib.ptr(x) for x in keep), n, steps, steps, 0, None,
                         B._lib.stream())
    return fn, (steps + 1) * (sd + 1), prec


def host_then_copy(task, host, steps, dtype):
    times = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = B.pairs.rollout(task, *host, n_steps=steps, dtype=dtype)
        on_device = [x.to(DEV) for x in out]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
        del on_device
    return float(np.median(times))


def kernel_times():
    print('us: median (min .. max) of %d repeats; host + copy: median of %d' % (REPS, HOST_REPS))
    for task in ('pendulum', 'cartpole'):
        for n in COUNTS:
            for steps in STEPS:
                host = draws(task, n, steps)
                for dtype in (torch.float32, torch.float64):
                    fn, per_episode, prec = launcher(task, host, steps, dtype)
                    quad = 16 // prec.itemsize
                    cols = B._lib.round_up(per_episode, quad)
                    src = torch.randn(n, cols, device=DEV).to(dtype)
                    dst = torch.empty_like(src)
                    res = timed({'rollout': fn,
                                 'copy': lambda: prec.copy_rows(B._lib.ptr(src), cols, None, B._lib.ptr(dst), cols, n,
                                                                cols, B._lib.stream())})
                    slow = host_then_copy(task, host, steps, dtype)
                    nbytes = float(per_episode) * prec.itemsize * n
                    print('  %s N=%d T=%d %s: %.1f MB out: rollout %.0f (%.0f .. %.0f) = %.3f TB/s written, '
                          '%.1f M steps/s; copy_rows %.0f (%.0f .. %.0f); host + copy %.0f; rollout / copy = %.1f, '
                          'host / rollout = %.0f'
                          % ((task, n, steps, 'fp64' if prec.itemsize == 8 else 'fp32', nbytes / 1e6) + res['rollout']
                             + (nbytes / res['rollout'][0] / 1e6, n * steps / res['rollout'][0]) + res['copy']
                             + (slow, res['rollout'][0] / res['copy'][0], slow / res['rollout'][0])), flush=True)
                    del fn, src, dst
                    torch.cuda.empty_cache()


def one_shape(task, precision, n, steps):
    fn, _, _ = launcher(task, draws(task, n, steps), steps, torch.float64 if precision == 'fp64' else torch.float32)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()


def main(argv):
    print('# csrc: %s' % csrc_hash())
    print('# %s' % torch.cuda.get_device_name(0))
    if '--one' in argv:
        task, precision, n, steps = argv[argv.index('--one') + 1:][:4]
        one_shape(task, precision, int(n), int(steps))
    else:
        kernel_times()


if __name__ == '__main__':
    main(sys.argv[1:])
