"""Why an MDRFF's bandwidth wants relating to its rows (profiles/rff_bandwidth_NOTES.md, the README's table),
measured on the CPU with the oracle alone, by the construction of tools/input_norm_cpu_table.py:
pairs.pendulum_pairs(5000, 20, seed=0), summaries from oracle.summarize, OracleMDRFF (200 features, RBF, 5
components, lr 1e-3), 5 chunks of 1000 pairs with 100 updates of 100 rows each, nothing from the GPU.  Per summary,
raw and standardised: the median pairwise distance of the first 800 rows (include/bsig_rff_bandwidth.h, restated
in numpy) and the final held-out NLL at seeds 0 / 1 with sigma = 4, the median, half of it and twice it.  The
frequencies are drawn once per summary with oracle.estimators.draw_rff_freqs('RBF', 100, width)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from oracle import summarize as osum
from tools.input_norm_cpu_table import final_nll, standardised

N_ROWS = 800


def median_distance(x, n_rows=N_ROWS):
    """The lower median of the pairwise distances of the first ``n_rows`` rows, in double."""
    x = x[:n_rows].double().numpy()
    d2 = np.concatenate([((x[i + 1:] - x[i]) ** 2).sum(axis=1) for i in range(x.shape[0] - 1)])
    return float(np.sqrt(np.sort(d2)[(d2.size - 1) // 2]))


def main(argv):
    theta, states, actions = pairs.pendulum_pairs(5000, 20, seed=0)
    summaries = [('`summary_start`', osum.summary_start(states, actions)),
                 ('`summary_corrdiff`', osum.summary_corrdiff(states, actions)),
                 ('signature depth 3', osum.summary_signatory(states, actions, depth=3))]
    print('| summary (width) | rows | median distance | sigma = 4 | sigma = median | median / 2 | median x 2 |')
    print('|---|---|---|---|---|---|---|')
    for name, x in summaries:
        x = x.float()
        np.random.seed(0)
        freqs = oest.draw_rff_freqs('RBF', 100, x.shape[1])
        for rows, xr in (('raw', x), ('standardised', standardised(x, N_ROWS))):
            med = median_distance(xr)
            cells = []
            for sigma in (4.0, med, med / 2, med * 2):
                nll = [final_nll(oest.OracleMDRFF, xr, theta, seed, n_feat=200, sigma=sigma, kernel='RBF', freqs=freqs)
                       for seed in (0, 1)]
                cells.append('%.2f / %.2f' % tuple(nll))
            print('| %s (%d) | %s | %.3g | %s |' % (name, x.shape[1], rows, med, ' | '.join(cells)), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
