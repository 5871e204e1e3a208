"""Timing of the least-squares dynamics kernel (include/bsig_sysid.h, csrc/sysid.h) for profiles/sysid_NOTES.md, by
the method of tools/signature_ex_timing.py: HIP events, a warm-up, median and range of REPS repeats, the kernels of
a comparison alternating in one process, N = 32 000 trajectories.
  (i)  kernel time in fp32 and in double (where covered) for Pendulum (3, 1, T 21), Ant (60, 8) at T 50 and T 100
       and ShadowHand (211, 20, T 50), each next to two yardsticks on the same trajectories: copy_rows moving the
       kernel's algorithmic bytes (trajectories in, rows out: half of them read, half written), the HBM bound; and
       summary_xcorr at lag 0.  No read-back in any of them (check_finite=False).
  (ii) --fit: pairs per second of BayesSim.fit (wall clock around the whole call, summaries included) on FIT_PAIRS
       Ant-shaped synthetic pairs with summary_sysid (4200 inputs) and with summary_xcorr (K 0, 600 inputs),
       alternating, and what bsig_fit_is_persistent answers for each model's plan.
  (iii) --one TASK fp32|fp64: the sysid launch of one shape of (i) alone, five times, for a profiler run."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

N = 32000
FIT_PAIRS = 32000
FIT_REPS = 3
WIDE_RIDGE = 1e-1
SHAPES = (('Pendulum', 3, 1, 21, 1e-3), ('Ant', 60, 8, 50, WIDE_RIDGE), ('Ant100', 60, 8, 100, WIDE_RIDGE),
          ('ShadowHand', 211, 20, 50, WIDE_RIDGE))


def _trajectories(sd, ad, length, dtype):
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV).to(dtype)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV).to(dtype)
    return states, actions


def kernel_times():
    print('(i) N = %d; us: median (min .. max) of %d repeats; bytes: trajectories in + rows out' % (N, REPS))
    lib = B._lib.load()
    for task, sd, ad, length, ridge in SHAPES:
        for dtype in (torch.float32, torch.float64):
            prec = B._lib.F64 if dtype == torch.float64 else B._lib.F32
            name = '%s %s' % (task, 'fp64' if prec.itemsize == 8 else 'fp32')
            if lib.bsig_sysid_fits(length, length, sd, ad, prec.itemsize) != B._lib.BSIG_OK:
                print('  %s: not covered (%s)' % (name, lib.bsig_last_error().decode()))
                continue
            states, actions = _trajectories(sd, ad, length, dtype)
            quad = 16 // prec.itemsize
            width = B.sysid_dim(sd, ad)
            out = torch.empty(N, B._lib.round_up(width, quad), dtype=dtype, device=DEV)
            x_out = torch.empty(N, B._lib.round_up(B.xcorr_dim(sd, ad, 0), quad), dtype=dtype, device=DEV)
            elems = length * (sd + ad) - ad + width           # T sd + (T - 1) ad read, the row written
            half = B._lib.round_up((elems + 1) // 2, quad)
            src = torch.randn(N, half, device=DEV).to(dtype)
            dst = torch.empty_like(src)
            fns = {
                'sysid': lambda: B.summary_sysid(states, actions, ridge=ridge, out=out, check_finite=False,
                                                 dtype=dtype),
                'copy': lambda: prec.copy_rows(B._lib.ptr(src), half, None, B._lib.ptr(dst), half, N, half,
                                               B._lib.stream()),
                'xcorr': lambda: B.summary_xcorr(states, actions, out=x_out, check_finite=False, dtype=dtype),
            }
            res = timed(fns)
            nbytes = float(elems) * prec.itemsize * N
            group = lib.bsig_sysid_group(length, length, sd, ad, prec.itemsize)
            dual = length - 1 < 1 + sd + ad
            print('  %s: width %d, %s system of order %d, %d a workgroup, %.1f MB: sysid %.0f (%.0f .. %.0f) = '
                  '%.3f TB/s; copy_rows %.0f (%.0f .. %.0f); summary_xcorr K 0 %.0f (%.0f .. %.0f); '
                  'sysid / copy = %.1f, sysid / xcorr = %.1f'
                  % ((name, width, 'dual' if dual else 'primal', min(length - 1, 1 + sd + ad), group, nbytes / 1e6)
                     + res['sysid'] + (nbytes / res['sysid'][0] / 1e6,) + res['copy'] + res['xcorr'] +
                     (res['sysid'][0] / res['copy'][0], res['sysid'][0] / res['xcorr'][0])), flush=True)
            del states, actions, out, x_out, src, dst
            torch.cuda.empty_cache()


def one_shape(task, precision):
    sd, ad, length, ridge = {name: rest for name, *rest in SHAPES}[task]
    dtype = torch.float64 if precision == 'fp64' else torch.float32
    states, actions = _trajectories(sd, ad, length, dtype)
    out = torch.empty(N, B._lib.round_up(B.sysid_dim(sd, ad), 16 // states.element_size()), dtype=dtype, device=DEV)
    for _ in range(5):
        B.summary_sysid(states, actions, ridge=ridge, out=out, check_finite=False, dtype=dtype)
    torch.cuda.synchronize()


def fit_throughput():
    sd, ad, length = 60, 8, 50
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    B.MDNN.VERBOSE = False
    models = {}
    for name, keys in (('summary_sysid', {'sysidRidge': WIDE_RIDGE}), ('summary_xcorr', {})):
        cfg = dict({'modelClass': 'MDNN', 'summarizerFxn': name, 'trainTrajLen': length, 'components': 5,
                    'hiddenLayers': (128, 128), 'lr': 1e-3}, **keys)
        torch.manual_seed(11)
        models[name] = B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2,
                                  params_lows=np.array([0.01, 0.01]), params_highs=np.array([2.0, 2.0]),
                                  prior=None, device=DEV)
    times = {name: [] for name in models}
    for rep in range(FIT_REPS + 1):                    # the first round warms up (plans, graphs)
        for name, bs in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = bs.fit(theta, states, actions)
            torch.cuda.synchronize()
            if rep:
                times[name].append(FIT_PAIRS / (time.perf_counter() - t0))
            assert np.isfinite(logs[-1]['train_loss']).all()
    print('(ii) BayesSim.fit on %d Ant-shaped synthetic pairs (sd 60, ad 8, T 50), MDNN (128, 128), 5 components: '
          'pairs per second, median and range of %d fits, alternating' % (FIT_PAIRS, FIT_REPS))
    for name, bs in models.items():
        model = bs.model
        code = int(model._plan_prec.is_persistent(model._plan)) if model._plan is not None else -1
        v = times[name]
        print('  %s, %d inputs: %.0f pairs/s (%.0f .. %.0f); bsig_fit_is_persistent: %d'
              % (name, model.input_dim, float(np.median(v)), min(v), max(v), code))
    a, b = (float(np.median(times[k])) for k in ('summary_sysid', 'summary_xcorr'))
    print('  sysid / xcorr = %.2f' % (a / b))


def main(argv):
    print('# csrc: %s' % csrc_hash())
    print('# %s' % torch.cuda.get_device_name(0))
    if '--one' in argv:
        task, precision = argv[argv.index('--one') + 1:][:2]
        one_shape(task, precision)
    elif '--fit' in argv:
        fit_throughput()
    else:
        kernel_times()


if __name__ == '__main__':
    main(sys.argv[1:])
