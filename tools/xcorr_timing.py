"""Timing of the time-lagged cross-correlation kernel (include/bsig_xcorr.h, csrc/xcorr.h) for
profiles/xcorr_NOTES.md, by the method of tools/signature_ex_timing.py: HIP events, a warm-up, median and range of
REPS repeats, the kernels of a comparison alternating in one process, N = 32 000 trajectories.
  (i)  kernel time in fp32 and in double for Pendulum (3, 1, T 21) at K 0 and 4, Ant (60, 8, T 50) at K 0 and 4
       and ShadowHand (211, 20, T 50) at K 0 and 1, each next to two yardsticks on the same trajectories:
       copy_rows moving the kernel's algorithmic bytes (trajectories in, rows out: half of them read, half
       written), the HBM bound; and summary_corrdiff, which this summary is an alternative to.  No read-back in
       any of them (check_finite=False).
  (ii) --fit: pairs per second of BayesSim.fit (wall clock around the whole call, summaries included) on
       FIT_PAIRS Ant-shaped synthetic pairs with summary_xcorr (K 0, 600 inputs) and with summary_corrdiff
       (11 802 inputs), alternating, and what bsig_fit_is_persistent answers for each model's plan.
  (iii) --pmc TASK K fp32|fp64: the xcorr launch of one shape of (i) alone, five times, for a counter pass
       (tools/pmc_pass.sh runs it once per counter)."""
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
SHAPES = (('Pendulum', 3, 1, 21, (0, 4)), ('Ant', 60, 8, 50, (0, 4)), ('ShadowHand', 211, 20, 50, (0, 1)))


def kernel_times():
    print('(i) N = %d; us: median (min .. max) of %d repeats; bytes: trajectories in + rows out' % (N, REPS))
    for task, sd, ad, length, lags in SHAPES:
        for dtype in (torch.float32, torch.float64):
            prec = B._lib.F64 if dtype == torch.float64 else B._lib.F32
            gen = torch.Generator().manual_seed(0)
            states = torch.randn(N, length, sd, generator=gen).to(DEV).to(dtype)
            actions = torch.rand(N, length, ad, generator=gen).to(DEV).to(dtype)
            quad = 16 // prec.itemsize
            corr_w = B.summarizers.summary_dim('summary_corrdiff', length, sd, ad)
            corr_out = torch.empty(N, B._lib.round_up(corr_w, quad), dtype=dtype, device=DEV)
            for k in lags:
                width = B.xcorr_dim(sd, ad, k)
                out = torch.empty(N, B._lib.round_up(width, quad), dtype=dtype, device=DEV)
                elems = length * (sd + ad) - ad + width           # T sd + (T - 1) ad read, the row written
                half = B._lib.round_up((elems + 1) // 2, quad)
                src = torch.randn(N, half, device=DEV).to(dtype)
                dst = torch.empty_like(src)
                fns = {
                    'xcorr': lambda: B.summary_xcorr(states, actions, max_lag=k, out=out, check_finite=False,
                                                     dtype=dtype),
                    'copy': lambda: prec.copy_rows(B._lib.ptr(src), half, None, B._lib.ptr(dst), half, N, half,
                                                   B._lib.stream()),
                    'corrdiff': lambda: B.summary_corrdiff(states, actions, out=corr_out, check_finite=False,
                                                           dtype=dtype),
                }
                res = timed(fns)
                nbytes = float(elems) * prec.itemsize * N
                group = B._lib.load().bsig_xcorr_group(length, length, sd, ad, k, 1, prec.itemsize)
                print('  %s K %d %s: width %d, %d a workgroup, %.1f MB: xcorr %.0f (%.0f .. %.0f) = %.2f TB/s; '
                      'copy_rows %.0f (%.0f .. %.0f); summary_corrdiff (width %d) %.0f (%.0f .. %.0f); '
                      'xcorr / copy = %.2f, xcorr / corrdiff = %.3f'
                      % ((task, k, 'fp64' if prec.itemsize == 8 else 'fp32', width, group, nbytes / 1e6) +
                         res['xcorr'] + (nbytes / res['xcorr'][0] / 1e6,) + res['copy'] + (corr_w,) +
                         res['corrdiff'] + (res['xcorr'][0] / res['copy'][0], res['xcorr'][0] / res['corrdiff'][0])))
                del out, src, dst
            del states, actions, corr_out
            torch.cuda.empty_cache()


def one_shape(task, k, precision):
    sd, ad, length = {name: (sd, ad, length) for name, sd, ad, length, _ in SHAPES}[task]
    dtype = torch.float64 if precision == 'fp64' else torch.float32
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV).to(dtype)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV).to(dtype)
    out = torch.empty(N, B._lib.round_up(B.xcorr_dim(sd, ad, k), 16 // states.element_size()), dtype=dtype, device=DEV)
    for _ in range(5):
        B.summary_xcorr(states, actions, max_lag=k, out=out, check_finite=False, dtype=dtype)
    torch.cuda.synchronize()


def fit_throughput():
    sd, ad, length = 60, 8, 50
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    B.MDNN.VERBOSE = False
    models = {}
    for name in ('summary_xcorr', 'summary_corrdiff'):
        cfg = {'modelClass': 'MDNN', 'summarizerFxn': name, 'trainTrajLen': length, 'components': 5,
               'hiddenLayers': (128, 128), 'lr': 1e-3}
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
    a, b = (float(np.median(times[k])) for k in ('summary_xcorr', 'summary_corrdiff'))
    print('  xcorr / corrdiff = %.2f' % (a / b))


def main(argv):
    print('# csrc: %s' % csrc_hash())
    print('# %s' % torch.cuda.get_device_name(0))
    if '--pmc' in argv:
        task, k, precision = argv[argv.index('--pmc') + 1:][:3]
        one_shape(task, int(k), precision)
    elif '--fit' in argv:
        fit_throughput()
    else:
        kernel_times()


if __name__ == '__main__':
    main(sys.argv[1:])
