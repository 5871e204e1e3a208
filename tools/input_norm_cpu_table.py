"""Why the estimator's inputs want standardising (profiles/input_norm_NOTES.md, the README's table), measured on
the CPU with the oracle alone: pairs.pendulum_pairs(5000, 20, seed=0), summaries from oracle.summarize, estimators
from oracle.estimators, nothing from the GPU.
  table: per summary its width, max |x|, largest column std, number of constant columns, and the share of the
         units of a Linear(width, 128) + tanh at torch's default init with |h| > 0.999 on the first 2000 rows, raw
         and standardised (mean / std of the first 800 rows, constant columns zeroed);
  --fit: final held-out NLL of an OracleMDRFF (200 features, sigma 4, RBF) and an OracleMDNN (trunk [128, 128]),
         lr 1e-3, 5 components, 5 chunks of 1000 pairs with 100 updates of 100 each, seeds 0 and 1, on the raw and
         on the standardised depth-3 signature."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from oracle import summarize as osum


def standardised(x, n_stats=800):
    mean, std = x[:n_stats].double().mean(0), x[:n_stats].double().std(0, unbiased=False)
    flat = std <= 8 * 2.0 ** -23 * mean.abs()
    inv = torch.where(flat, torch.zeros_like(std), 1.0 / torch.where(flat, torch.ones_like(std), std))
    return ((x.double() - mean) * inv).float()


def saturation(x):
    torch.manual_seed(0)
    layer = torch.nn.Linear(x.shape[1], 128)
    with torch.no_grad():
        return float((torch.tanh(layer(x[:2000])).abs() > 0.999).float().mean())


def final_nll(cls, x, theta, seed, **kw):
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = cls(input_dim=x.shape[1], output_dim=2, output_lows=np.array([0.01, 0.01]),
                output_highs=np.array([2.0, 2.0]), n_gaussians=5, full_covariance=False, lr=1e-3,
                activation=torch.nn.Tanh, **kw)
    for lo in range(0, 5000, 1000):
        logs = model.run_training(x[lo:lo + 1000], theta[lo:lo + 1000], 100, 100)
    return logs['test_loss'][-1]


def main(argv):
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    summaries = [('summary_start', osum.summary_start(states, actions)),
                 ('summary_corrdiff', osum.summary_corrdiff(states, actions)),
                 ('summary_signatory, depth 3', osum.summary_signatory(states, actions, depth=3)),
                 ('summary_signatory, depth 4', osum.summary_signatory(states, actions, depth=4))]
    print('| summary | width | max abs x | largest column std | constant columns | saturated raw / standardised |')
    for name, x in summaries:
        x = x.float()
        std = x.double().std(0, unbiased=False)
        print('| %s | %d | %.2g | %.3g | %d | %.3f / %.3f |' % (name, x.shape[1], float(x.abs().max()), float(std.max()),
                                                             int((std == 0).sum()), saturation(x),
                                                             saturation(standardised(x))))
    if '--fit' in argv:
        x = summaries[2][1].float()
        freqs = oest.draw_rff_freqs('RBF', 100, x.shape[1])
        for label, cls, kw in (('OracleMDRFF', oest.OracleMDRFF, dict(n_feat=200, sigma=4.0, kernel='RBF', freqs=freqs)),
                               ('OracleMDNN', oest.OracleMDNN, dict(hidden_layers=(128, 128)))):
            raw = [final_nll(cls, x, theta, seed, **kw) for seed in (0, 1)]
            std = [final_nll(cls, standardised(x), theta, seed, **kw) for seed in (0, 1)]
            print('%s on the depth-3 signature, final held-out NLL, seeds 0 / 1: raw %.2f / %.2f, standardised '
                  '%.2f / %.2f' % (label, raw[0], raw[1], std[0], std[1]))


if __name__ == '__main__':
    main(sys.argv[1:])
