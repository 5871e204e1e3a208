"""What the kernel mean embedding summary buys the estimator (profiles/kme_NOTES.md, the README's table), measured
on the CPU with the oracle and numpy alone, under the protocol of tools/xcorr_cpu_table.py:
pairs.pendulum_pairs(5000, 20, seed=0), the embedding from the definition of include/bsig_kme.h restated below in
numpy (double, rounded to fp32 rows), one frequency draw (RandomState(0)), the per-column scale from the first 800
trajectories' transitions, an OracleMDNN with trunk [128, 128], 5 components, lr 1e-3, 5 chunks of 1000 pairs with
100 updates of 100 rows -- ``final_nll`` and ``standardised`` of tools/input_norm_cpu_table.py.  Per summary: its
width and the final held-out NLL at seeds 0 / 1, on the raw rows and on the rows standardised by the first 800.  One
task, one draw, on the CPU: nothing here says anything about the GPU or about wide tasks."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from oracle import summarize as osum
from tools.input_norm_cpu_table import final_nll, standardised
from tools.xcorr_cpu_table import xcorr

N_SCALE = 800      # the trajectories whose transitions give the per-column scale


def transitions(states, actions, diff=True, time=False):
    """The rows x_t = [tau? | s | a | ds?] of include/bsig_kme.h, [N, M, d] in double."""
    s, a = states.double().numpy(), actions.double().numpy()
    m = s.shape[1] - (1 if diff else 0)
    parts = []
    if time:
        parts.append(np.broadcast_to((np.arange(m) / max(m - 1, 1))[None, :, None], (s.shape[0], m, 1)))
    parts += [s[:, :m], a[:, np.minimum(np.arange(m), a.shape[1] - 1)]]
    if diff:
        parts.append(s[:, 1:] - s[:, :-1])
    return np.concatenate(parts, axis=2)


def embedding(states, actions, n_feat, c, diff=True, time=False, seed=0):
    """[a/M sum_t cos z_t | a/M sum_t sin z_t], z = x . (freqs / (c std sqrt(d))), a = sqrt(2 / n_feat)."""
    x = transitions(states, actions, diff, time)
    d, m = x.shape[2], n_feat // 2
    std = x[:N_SCALE].reshape(-1, d).std(axis=0)
    inv_std = np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)
    freqs = np.random.RandomState(seed).standard_normal((m, d)).astype(np.float32).astype(np.float64)
    z = np.einsum('ntk,jk->ntj', x, freqs * inv_std[None, :] / (c * np.sqrt(d)))
    row = np.concatenate([np.cos(z).mean(axis=1), np.sin(z).mean(axis=1)], axis=1) * np.sqrt(1.0 / m)
    return torch.from_numpy(row).float()


def main():
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    summaries = [('`summary_start`', osum.summary_start(states, actions)),
                 ('`summary_xcorr`, lag 0', xcorr(states, actions, 0, True))]
    for n_feat in (64, 256):
        for c in (0.5, 1.0, 2.0):
            summaries.append(('mean embedding, %d features, c = %g' % (n_feat, c),
                              embedding(states, actions, n_feat, c)))
    summaries.append(('mean embedding, 256 features, c = 1, time=True', embedding(states, actions, 256, 1.0, time=True)))
    summaries.append(('mean embedding, 256 features, c = 1, diff=False', embedding(states, actions, 256, 1.0, diff=False)))
    print('| summary | width | raw | standardised (first 800 rows) |')
    print('|---|---|---|---|')
    for name, x in summaries:
        x = x.float()
        kw = dict(hidden_layers=(128, 128))
        raw = [final_nll(oest.OracleMDNN, x, theta, seed, **kw) for seed in (0, 1)]
        std = [final_nll(oest.OracleMDNN, standardised(x), theta, seed, **kw) for seed in (0, 1)]
        print('| %s | %d | %.2f / %.2f | %.2f / %.2f |' % (name, x.shape[1], raw[0], raw[1], std[0], std[1]), flush=True)


if __name__ == '__main__':
    main()
