"""Timing of the input standardisation (include/bsig_input_norm.h, csrc/input_norm.h) for
profiles/input_norm_NOTES.md, by the method of tools/logsignature_timing.py: HIP events, a warm-up, median and
range of REPS repeats, the kernels of a comparison alternating in one process.
  (i)   the apply against the copy it replaces in the chunk staging: bsig_input_norm_apply next to bsig_copy_rows,
        fp32, a block of 32 000 x 11 110 (1.4 GB a side: beyond the 256 MiB Infinity Cache) and a chunk of
        1 000 x 11 110, out of place, pitches rounded up to 16 bytes; the apply in place too;
  (ii)  the statistics: GB/s of rows read at 800 x 11 110 and at 32 000 x 11 110, next to a read-only torch sum
        over the same buffer (the read rate tools/hbm_peak.py reports, at this size);
  (iii) BayesSim.fit with 'inputNorm' on against off: FIT_PAIRS synthetic pairs, an MDNN on summary_signatory
        depth 3 and an MDRFF on summary_start, wall clock around the whole call, alternating.
Arguments: any of 'apply', 'stats', 'fit' (default: all three)."""
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

WIDTH = 11110
FIT_PAIRS = 32000
FIT_REPS = 5


def rows(n, width=WIDTH):
    ld = _lib.round_up(width, 4)
    x = torch.randn(n, ld, device=DEV)
    x[:, 0] = torch.arange(n, device=DEV)          # not every column centred
    return x, ld


def stats_of(x, ld, n, width=WIDTH):
    mean = torch.empty(width, dtype=torch.float64, device=DEV)
    inv = torch.empty(width, dtype=torch.float64, device=DEV)
    need = int(_lib.load().bsig_input_norm_workspace_bytes(n, width))
    ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)

    def run():
        _lib.F32.input_norm_stats(_lib.ptr(x), ld, n, width, _lib.ptr(mean), _lib.ptr(inv), _lib.ptr(ws), need,
                                  _lib.stream())
    return mean, inv, run


def apply_against_copy():
    print('(i) bsig_input_norm_apply against bsig_copy_rows, fp32, width %d, pitch %d' % (WIDTH, _lib.round_up(WIDTH, 4)))
    for n in (32000, 1000):
        x, ld = rows(n)
        out = torch.empty_like(x)
        mean, inv, run = stats_of(x, ld, n)
        run()
        st = _lib.stream()
        res = timed({
            'copy': lambda: _lib.F32.copy_rows(_lib.ptr(x), ld, None, _lib.ptr(out), ld, n, WIDTH, st),
            'apply': lambda: _lib.F32.input_norm_apply(_lib.ptr(x), ld, _lib.ptr(mean), _lib.ptr(inv), _lib.ptr(out),
                                                       ld, n, WIDTH, st),
            'in_place': lambda: _lib.F32.input_norm_apply(_lib.ptr(out), ld, _lib.ptr(mean), _lib.ptr(inv),
                                                          _lib.ptr(out), ld, n, WIDTH, st)})
        gb = 2 * 4 * n * WIDTH / 1e9            # read + write
        print('  %6d rows (%.2f GB moved): copy_rows %.0f us (%.0f .. %.0f) = %.2f TB/s, apply %.0f us (%.0f .. %.0f) '
              '= %.2f TB/s, apply / copy = %.3f; in place %.0f us (%.0f .. %.0f)'
              % ((n, gb) + res['copy'] + (gb / res['copy'][0] * 1e3,) + res['apply'] +
                 (gb / res['apply'][0] * 1e3, res['apply'][0] / res['copy'][0]) + res['in_place']))
        del x, out


def statistics_rate():
    print('(ii) bsig_input_norm_stats (slab pass + finishing pass), fp32, width %d' % WIDTH)
    for n in (800, 32000):
        x, ld = rows(n)
        _, _, run = stats_of(x, ld, n)
        res = timed({'stats': run, 'sum': lambda: x.sum()})
        gb = 4 * n * WIDTH / 1e9
        print('  %6d rows (%.3f GB read): stats %.0f us (%.0f .. %.0f) = %.2f TB/s; torch sum of the buffer %.0f us '
              '= %.2f TB/s' % ((n, gb) + res['stats'] + (gb / res['stats'][0] * 1e3, res['sum'][0],
                                                       4 * x.numel() / 1e9 / res['sum'][0] * 1e3)))
        del x


def fit_effect():
    sd, ad, length = 7, 2, 11
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    kinds = {'MDNN on summary_signatory depth 3': {'modelClass': 'MDNN', 'summarizerFxn': 'summary_signatory',
                                                   'sigDepth': 3, 'hiddenLayers': (128, 128)},
             'MDRFF on summary_start': {'modelClass': 'MDRFF', 'summarizerFxn': 'summary_start', 'nFeat': 200,
                                        'hiddenLayers': []}}
    B.MDNN.VERBOSE = False
    models = {}
    for kind, extra in kinds.items():
        for on in (False, True):
            cfg = dict(extra, trainTrajLen=length, components=5, lr=1e-3, inputNorm=on)
            torch.manual_seed(11), np.random.seed(11)
            models[kind, on] = B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2,
                                          params_lows=np.array([0.01, 0.01]), params_highs=np.array([2.0, 2.0]),
                                          prior=None, device=DEV)
    times, last = {key: [] for key in models}, {}
    for rep in range(FIT_REPS + 1):                    # the first round warms up (plans, graphs, the statistics)
        for key, bs in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = bs.fit(theta, states, actions)
            torch.cuda.synchronize()
            if rep:
                times[key].append((time.perf_counter() - t0) * 1e3)
            assert np.isfinite(logs[-1]['train_loss']).all()
            if rep == 0:
                last[key] = logs[-1]['test_loss'][-1]      # after one pass over the pairs
    print("(iii) BayesSim.fit on %d synthetic pairs with 'inputNorm' off / on: ms per fit, median and range of %d "
          "fits, alternating" % (FIT_PAIRS, FIT_REPS))
    for kind in kinds:
        off, on = times[kind, False], times[kind, True]
        print('  %s, %d inputs: off %.1f ms (%.1f .. %.1f), on %.1f ms (%.1f .. %.1f), on / off = %.3f; held-out '
              'NLL of the last chunk after the first fit: off %.3f, on %.3f'
              % (kind, models[kind, True].model.input_dim, float(np.median(off)), min(off), max(off),
                 float(np.median(on)), min(on), max(on), float(np.median(on)) / float(np.median(off)),
                 last[kind, False], last[kind, True]))


def main(argv):
    what = argv or ['apply', 'stats', 'fit']
    print('# csrc: %s' % csrc_hash())
    print('# %s, %d repeats' % (torch.cuda.get_device_name(0), REPS))
    if 'apply' in what:
        apply_against_copy()
    if 'stats' in what:
        statistics_rate()
    if 'fit' in what:
        fit_effect()


if __name__ == '__main__':
    main(sys.argv[1:])
