"""Timing of the median bandwidth (include/bsig_rff_bandwidth.h, csrc/rff_bandwidth.h) for
profiles/rff_bandwidth_NOTES.md, by the method of tools/input_norm_timing.py: HIP events, a warm-up, median and
range of REPS repeats, the calls of a comparison alternating in one process.
  (i)   the one-off launches (pair distances, 8 selection passes, the finish, and bsig_rff_coeff_dev) on the first
        chunk's 800 training rows at widths 2310 and 11 802, fp32 and double rows, next to the yardstick: one
        rff.to_features of a block of BLOCK_ROWS rows of the same width (fp32, 200 features);
  (ii)  BayesSim.fit on FIT_PAIRS synthetic pairs, 'MDRFF_RBF_median' against 'MDRFF_RBF_4.0' on summary_start,
        wall clock around the whole call, alternating.
Arguments: any of 'launches', 'fit' (default: both)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

N_ROWS = 800
WIDTHS = (2310, 11802)
N_FEAT = 200
BLOCK_ROWS = 32000
FIT_PAIRS = 32000
FIT_REPS = 5


def launches():
    print('(i) the bandwidth of %d rows (pair distances + selection) and the coefficient, next to one '
          'rff.to_features of %d rows, %d features' % (N_ROWS, BLOCK_ROWS, N_FEAT))
    lib = _lib.load()
    for width in WIDTHS:
        ld = _lib.round_up(width, 4)
        block = torch.randn(BLOCK_ROWS, ld, device=DEV)
        np.random.seed(0)
        rff = B.RFF(N_FEAT, width, 4.0, quasi_random=False, device=DEV)
        freqs = rff.freqs.contiguous()
        sigma = torch.ones((), dtype=torch.float64, device=DEV)
        coeff = torch.empty(N_FEAT // 2, ld, device=DEV)
        need = int(lib.bsig_rff_bandwidth_workspace_bytes(N_ROWS, width))
        ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
        x64 = block[:N_ROWS].double().contiguous()
        st = _lib.stream()
        res = timed({
            'fp32': lambda: _lib.F32.rff_bandwidth_median(_lib.ptr(block), ld, N_ROWS, width, 1.0, _lib.ptr(sigma),
                                                          _lib.ptr(ws), need, st),
            'f64': lambda: _lib.F64.rff_bandwidth_median(_lib.ptr(x64), ld, N_ROWS, width, 1.0, _lib.ptr(sigma),
                                                         _lib.ptr(ws), need, st),
            'coeff': lambda: _lib.F32.rff_coeff_dev(_lib.ptr(freqs), _lib.ptr(sigma), _lib.ptr(coeff), N_FEAT // 2,
                                                    width, ld, st),
            'project': lambda: rff.to_features(block[:, :width])})
        flop = 3.0 * (N_ROWS * (N_ROWS - 1) // 2) * width            # a subtraction and an fma per pair and column
        print('  width %5d: fp32 rows %.0f us (%.0f .. %.0f) = %.2f fp64 TFLOP/s, double rows %.0f us (%.0f .. %.0f), '
              'coeff_dev %.1f us (%.1f .. %.1f); to_features of %d rows %.0f us (%.0f .. %.0f); bandwidth / '
              'projection = %.3f' % ((width,) + res['fp32'] + (flop / res['fp32'][0] * 1e-6,) + res['f64'] +
                                     res['coeff'] + (BLOCK_ROWS,) + res['project'] +
                                     (res['fp32'][0] / res['project'][0],)))
        print('    sigma %.6g (standard normal rows: sqrt(2 x %d) = %.6g)' % (float(sigma), width, (2 * width) ** 0.5))
        del block, x64


def fit_effect():
    sd, ad, length = 7, 2, 11
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    B.MDNN.VERBOSE = False
    models = {}
    for name in ('MDRFF_RBF_4.0', 'MDRFF_RBF_median'):
        cfg = dict(modelClass=name, summarizerFxn='summary_start', nFeat=N_FEAT, hiddenLayers=[], trainTrajLen=length,
                   components=5, lr=1e-3)
        torch.manual_seed(11), np.random.seed(11)
        models[name] = B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2,
                                  params_lows=np.array([0.01, 0.01]), params_highs=np.array([2.0, 2.0]),
                                  prior=None, device=DEV)
    times, first, last = {key: [] for key in models}, {}, {}
    for rep in range(FIT_REPS + 1):                    # the first round warms up (plans, graphs) and makes the bandwidth
        for key, bs in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = bs.fit(theta, states, actions)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                times[key].append(ms)
            else:
                first[key], last[key] = ms, logs[-1]['test_loss'][-1]
            assert np.isfinite(logs[-1]['train_loss']).all()
    print('(ii) BayesSim.fit on %d synthetic pairs, summary_start (%d inputs): ms per fit, median and range of %d '
          'fits, alternating' % (FIT_PAIRS, models['MDRFF_RBF_median'].model.input_dim, FIT_REPS))
    for key, v in times.items():
        print('  %s: %.1f ms (%.1f .. %.1f); the first fit (plans, graphs, and the bandwidth where it is made) %.1f '
              'ms; held-out NLL of the last chunk after the first fit %.3f'
              % (key, float(np.median(v)), min(v), max(v), first[key], last[key]))
    print('  median / 4.0 = %.3f; sigma = %.6g' % (
        float(np.median(times['MDRFF_RBF_median'])) / float(np.median(times['MDRFF_RBF_4.0'])),
        float(models['MDRFF_RBF_median'].model.state_dict()['rff_bandwidth.sigma'])))


def main(argv):
    what = argv or ['launches', 'fit']
    print('# csrc: %s' % csrc_hash())
    print('# %s, %d repeats' % (torch.cuda.get_device_name(0), REPS))
    if 'launches' in what:
        launches()
    if 'fit' in what:
        fit_effect()


if __name__ == '__main__':
    main(sys.argv[1:])
