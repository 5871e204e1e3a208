"""What the paper's time-lagged cross-correlation summary buys the estimator (profiles/xcorr_NOTES.md, the README's
table), measured on the CPU with the oracle and numpy alone: pairs.pendulum_pairs(5000, 20, seed=0), the
reference's summaries from oracle.summarize, the time-lagged ones from the definition of include/bsig_xcorr.h
restated below in numpy (double, rounded to fp32 rows), an OracleMDNN with trunk [128, 128], 5 components, lr 1e-3,
5 chunks of 1000 pairs with 100 updates of 100 rows -- ``final_nll`` and ``standardised`` of
tools/input_norm_cpu_table.py.  Per summary: its width and the final held-out NLL at seeds 0 / 1, on the raw rows
and on the rows standardised by the first 800.  One task, on the CPU: nothing here says anything about the GPU or
about wide tasks."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from oracle import summarize as osum
from tools.input_norm_cpu_table import final_nll, standardised


def xcorr(states, actions, max_lag=0, state_diff=True):
    """[c_0 | ... | c_max_lag | mu | sigma] of include/bsig_xcorr.h, in double."""
    s, a = states.double().numpy(), actions.double().numpy()
    f = s[:, 1:] - s[:, :-1] if state_diff else s
    n, m, _ = f.shape
    a = a[:, np.minimum(np.arange(m), a.shape[1] - 1)]
    parts = [(np.einsum('nti,ntj->nij', f[:, tau:], a[:, :m - tau]) / (m - tau)).reshape(n, -1)
             for tau in range(max_lag + 1)]
    mu = f.mean(axis=1)
    sigma = np.sqrt(((f - mu[:, None, :]) ** 2).mean(axis=1))
    return torch.from_numpy(np.concatenate(parts + [mu, sigma], axis=1)).float()


def main():
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    summaries = [('`summary_start`', osum.summary_start(states, actions)),
                 ('`summary_corrdiff`', osum.summary_corrdiff(states, actions)),
                 ("time-lagged, temporal diffs, lag 0 (the paper's)", xcorr(states, actions, 0, True)),
                 ('time-lagged, temporal diffs, lags 0..4', xcorr(states, actions, 4, True)),
                 ('time-lagged, temporal diffs, lags 0..9', xcorr(states, actions, 9, True)),
                 ('time-lagged, raw states, lags 0..4', xcorr(states, actions, 4, False))]
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
