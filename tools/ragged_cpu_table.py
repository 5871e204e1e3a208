"""What per-trajectory lengths buy the estimator on episodes that end early (profiles/ragged_NOTES.md, the README's
paragraph), measured on the CPU with the oracle and numpy alone, under the protocol of tools/xcorr_cpu_table.py and
tools/kme_cpu_table.py: pairs.pendulum_pairs(5000, 20, seed=0), an OracleMDNN with trunk [128, 128], 5 components,
lr 1e-3, 5 chunks of 1000 pairs with 100 updates of 100 rows, the inputs standardised by the first 800 rows, the
final held-out NLL at seeds 0 / 1.

The episodes are ended at lengths drawn once, uniformly in 6..21 states, from a generator of their own
(``pairs.end_episodes``: the recorder's tail, the last state repeated).  Two summaries, ``summary_xcorr`` at lag 0
and ``summary_kme`` with 256 features and c = 1, each
  (a) on the padded episodes, without lengths: what a user could compute before;
  (b) with lengths: the definitions of include/bsig_ragged.h, restated below in numpy, in double;
and, for reference, on the untruncated episodes.  One task, one draw of lengths, on the CPU: nothing here says
anything about the GPU or about another task."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from tools.input_norm_cpu_table import final_nll, standardised
from tools.kme_cpu_table import N_SCALE, transitions

LENGTHS_SEED, SHORTEST = 7, 6


def valid_steps(lengths, steps):
    """[N, M] in double: 1 where step t is one of the trajectory's own M_n = L_n - 1, else 0."""
    return (np.arange(steps)[None, :] < (np.asarray(lengths) - 1)[:, None]).astype(np.float64)


def xcorr_lag0(states, actions, lengths):
    """[c_0 | mu | sigma] of include/bsig_xcorr.h with T = L_n in every formula, in double."""
    s, a = states.double().numpy(), actions.double().numpy()
    f = s[:, 1:] - s[:, :-1]
    n, m, _ = f.shape
    a = a[:, np.minimum(np.arange(m), a.shape[1] - 1)]
    on = valid_steps(lengths, m)[:, :, None]
    count = on.sum(axis=1)
    c0 = np.einsum('nti,ntj->nij', f * on, a).reshape(n, -1) / count
    mu = (f * on).sum(axis=1) / count
    sigma = np.sqrt((((f - mu[:, None, :]) ** 2) * on).sum(axis=1) / count)
    return torch.from_numpy(np.concatenate([c0, mu, sigma], axis=1)).float()


def embedding(states, actions, lengths, n_feat=256, c=1.0, seed=0):
    """[a/M_n sum_t cos z_t | a/M_n sum_t sin z_t] over the trajectory's own steps, the per-column scale from the
    valid rows of the first N_SCALE trajectories (include/bsig_kme.h with T = L_n)."""
    x = transitions(states, actions)
    d, m = x.shape[2], n_feat // 2
    on = valid_steps(lengths, x.shape[1])
    std = x[:N_SCALE][on[:N_SCALE] > 0].std(axis=0)
    inv_std = np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)
    freqs = np.random.RandomState(seed).standard_normal((m, d)).astype(np.float32).astype(np.float64)
    z = np.einsum('ntk,jk->ntj', x, freqs * inv_std[None, :] / (c * np.sqrt(d)))
    count = on.sum(axis=1)[:, None]
    row = np.concatenate([(np.cos(z) * on[:, :, None]).sum(axis=1) / count,
                          (np.sin(z) * on[:, :, None]).sum(axis=1) / count], axis=1) * np.sqrt(1.0 / m)
    return torch.from_numpy(row).float()


def main():
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    whole = np.full(5000, states.shape[1])
    lengths = np.random.RandomState(LENGTHS_SEED).randint(SHORTEST, states.shape[1] + 1, size=5000)
    ended_s, ended_a = pairs.end_episodes(states, actions, lengths)
    print('lengths: uniform in %d..%d, mean %.2f; %d of 5000 episodes run to the end'
          % (SHORTEST, states.shape[1], lengths.mean(), int((lengths == states.shape[1]).sum())))
    print('| summary | width | untruncated | (a) padded, no lengths | (b) with lengths |')
    print('|---|---|---|---|---|')
    for name, fn in (('`summary_xcorr`, lag 0', xcorr_lag0), ('`summary_kme`, 256 features, c = 1', embedding)):
        cells = []
        for s, a, lens in ((states, actions, whole), (ended_s, ended_a, whole), (ended_s, ended_a, lengths)):
            x = standardised(fn(s, a, lens))
            nll = [final_nll(oest.OracleMDNN, x, theta, seed, hidden_layers=(128, 128)) for seed in (0, 1)]
            cells.append('%.2f / %.2f' % (nll[0], nll[1]))
        print('| %s | %d | %s |' % (name, x.shape[1], ' | '.join(cells)), flush=True)


if __name__ == '__main__':
    main()
