"""What the least-squares dynamics summary buys the estimator (profiles/sysid_NOTES.md, the README's table),
measured on the CPU with the oracle and numpy alone, by the protocol of tools/xcorr_cpu_table.py:
pairs.pendulum_pairs(5000, 20, seed=0), the summary from the definition of include/bsig_sysid.h restated below in
numpy (double, rounded to fp32 rows), an OracleMDNN with trunk [128, 128], 5 components, lr 1e-3, 5 chunks of
1000 pairs with 100 updates of 100 rows -- ``final_nll`` and ``standardised`` of tools/input_norm_cpu_table.py.
Per row: the width and the final held-out NLL at seeds 0 / 1, on the raw rows and on the rows standardised by the
first 800.  The row without the residuals is for reference only: the library has no such option.  One task, on
the CPU: nothing here says anything about the GPU or about wide tasks."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from tools.input_norm_cpu_table import final_nll, standardised
from tools.xcorr_cpu_table import xcorr


def sysid(states, actions, ridge=1e-3, residual=True):
    """[W row-major | r] of include/bsig_sysid.h, in double."""
    s, a = states.double().numpy(), actions.double().numpy()
    n, ts, sd = s.shape
    m = ts - 1
    phi = np.concatenate([np.ones((n, m, 1)), s[:, :m], a[:, np.minimum(np.arange(m), a.shape[1] - 1)]], axis=2)
    y = s[:, 1:] - s[:, :-1]
    p = phi.shape[2]
    gram = np.einsum('nti,ntj->nij', phi, phi) / m
    cross = np.einsum('nti,ntj->nij', phi, y) / m
    rho = ridge * np.trace(gram, axis1=1, axis2=2) / p
    w = np.linalg.solve(gram + rho[:, None, None] * np.eye(p), cross)
    parts = [w.reshape(n, -1)]
    if residual:
        e = y - np.einsum('nti,nij->ntj', phi, w)
        parts.append(np.sqrt((e * e).mean(axis=1)))
    return torch.from_numpy(np.concatenate(parts, axis=1)).float()


def main():
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    summaries = [('`summary_xcorr`, lag 0', xcorr(states, actions, 0, True))]
    summaries += [('dynamics fit, ridge %g' % ridge, sysid(states, actions, ridge))
                  for ridge in (1e-6, 1e-4, 1e-3, 1e-2)]
    summaries += [('dynamics fit, ridge 1e-3, no residual (reference only)', sysid(states, actions, 1e-3, False))]
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
