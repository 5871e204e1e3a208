"""Timing of the log-signature kernel (include/bsig_logsignature.h, csrc/logsignature.h) for
profiles/logsignature_NOTES.md, by the method of tools/signature_ex_timing.py: HIP events, a warm-up, median and
range of REPS repeats, the kernels of a comparison alternating in one process, N = 100 000 trajectories, fp32.
  (i)  the epilogue's cost: summary_logsignature next to summary_signatory on the general kernel (the identity
       channel list) at (L = 21, d = 6, depth 4), (L = 21, d = 5, depth 5) and (L = 11, d = 22, depth 3);
  (ii) the effect on the fit: us per update of BayesSim.fit (wall clock around the whole call, summaries
       included, FIT_PAIRS synthetic pairs) at d = 10, depth 4 with summary_signatory (11 110 inputs) and with
       summary_logsignature (2 860 inputs), alternating, and whether each model's plan is a persistent kernel."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, N, REPS, timed

FIT_PAIRS = 4000
FIT_REPS = 5


def shape(length, sd, ad, depth):
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV)
    d = 1 + sd + ad
    widths = B.summarizers.signature_dim(d, depth), B.summarizers.logsignature_dim(d, depth)
    outs = [torch.empty(N, B._lib.round_up(w, 4), device=DEV) for w in widths]
    return states, actions, outs, widths


def epilogue_cost():
    print('(i) summary_logsignature against summary_signatory on the general kernel (identity list)')
    for length, sd, ad, depth in ((21, 4, 1, 4), (21, 3, 1, 5), (11, 17, 4, 3)):
        states, actions, outs, widths = shape(length, sd, ad, depth)
        ident = list(range(sd + ad))
        res = timed({'sig': lambda: B.summary_signatory(states, actions, depth=depth, channels=ident, out=outs[0]),
                     'log': lambda: B.summary_logsignature(states, actions, depth=depth, channels=ident,
                                                           out=outs[1])})
        print('  L = %d, d = %d, depth %d: signature (%d terms) %.0f us (%.0f .. %.0f), log-signature (%d words) '
              '%.0f us (%.0f .. %.0f), log / signature = %.3f'
              % ((length, 1 + sd + ad, depth, widths[0]) + res['sig'] + (widths[1],) + res['log'] +
                 (res['log'][0] / res['sig'][0],)))
        del states, actions, outs


def fit_effect():
    sd, ad, length, depth = 7, 2, 11, 4
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    models = {}
    for name in ('summary_signatory', 'summary_logsignature'):
        cfg = {'modelClass': 'MDNN', 'summarizerFxn': name, 'trainTrajLen': length, 'components': 3,
               'hiddenLayers': (64, 64), 'lr': 1e-3, 'sigDepth': depth}
        torch.manual_seed(11)
        models[name] = B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2,
                                  params_lows=np.array([0.01, 0.01]), params_highs=np.array([2.0, 2.0]),
                                  prior=None, device=DEV)
    B.MDNN.VERBOSE = False
    updates = -(-FIT_PAIRS // B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH) * B.BayesSim.NUM_GRAD_UPDATES
    times = {name: [] for name in models}
    for rep in range(FIT_REPS + 1):                    # the first round warms up (plans, graphs)
        for name, bs in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = bs.fit(theta, states, actions)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e6 / updates)
            assert np.isfinite(logs[-1]['train_loss']).all()
    print('(ii) BayesSim.fit on %d synthetic pairs, d = 10, depth 4, hidden (64, 64): us per update, median '
          'and range of %d fits, alternating' % (FIT_PAIRS, FIT_REPS))
    for name, bs in models.items():
        model = bs.model
        persistent = bool(model._plan_prec.is_persistent(model._plan)) if model._plan is not None else None
        v = times[name]
        print('  %s, %d inputs: %.1f us (%.1f .. %.1f); plan: %s'
              % (name, model.input_dim, float(np.median(v)), min(v), max(v),
                 {True: 'persistent update kernel', False: 'per-phase kernels', None: 'none'}[persistent]))
    a, b = (float(np.median(times[k])) for k in ('summary_signatory', 'summary_logsignature'))
    print('  log-signature / signature = %.3f' % (b / a))


def main():
    print('# csrc: %s' % csrc_hash())
    print('# %s, N = %d, %d repeats' % (torch.cuda.get_device_name(0), N, REPS))
    epilogue_cost()
    fit_effect()


if __name__ == '__main__':
    main()
