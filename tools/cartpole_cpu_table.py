"""The second task's tables (profiles/sim_NOTES.md, the README's paragraph): what every summary the table tools
restate in numpy buys the estimator on CartPole, measured on the CPU with the oracle and numpy alone, under the
protocol of tools/sysid_cpu_table.py -- an OracleMDNN with trunk [128, 128], 5 components, lr 1e-3, 5 chunks of
1000 pairs with 100 updates of 100 rows, ``final_nll`` and ``standardised`` of tools/input_norm_cpu_table.py (whose
output box [0.01, 2]^2 holds CartPole's [0.1, 2]^2), the final held-out NLL at seeds 0 / 1.

  (1) pairs.cartpole_pairs(5000, 20, seed=0): no episode ends.  Per summary: its width, the NLL on the raw rows
      and on the rows standardised by the first 800.
  (2) pairs.cartpole_pairs(5000, 50, seed=0, terminate=True): episodes end by the task's own rule.  The three
      columns of tools/ragged_cpu_table.py, standardised rows: on the untruncated episodes (the same draws
      without ``terminate``), on the ended episodes without lengths, and with lengths -- for the two summaries
      that take them (``summary_xcorr`` at lag 0 and ``summary_kme``; the others have no such form).

Every summary is an existing restatement, imported: oracle.summarize, tools/xcorr_cpu_table.py,
tools/kme_cpu_table.py, tools/sysid_cpu_table.py, tools/ragged_cpu_table.py.  The rollouts run on the host path
of pairs.rollout.  One more task, the oracle, the CPU: nothing here says anything about the GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from bayes_sim_ig_amd import pairs
from oracle import estimators as oest
from oracle import summarize as osum
from tools import ragged_cpu_table as ragged
from tools.input_norm_cpu_table import final_nll, standardised
from tools.kme_cpu_table import embedding
from tools.sysid_cpu_table import sysid
from tools.xcorr_cpu_table import xcorr

# name -> (the fixed-length restatement, the one with lengths or None)
SUMMARIES = (
    ('`summary_start`', osum.summary_start, None),
    ('`summary_corrdiff`', osum.summary_corrdiff, None),
    ('`summary_signatory`, depth 3', lambda s, a: osum.summary_signatory(s, a, depth=3), None),
    ('`summary_xcorr`, lag 0', lambda s, a: xcorr(s, a, 0, True), ragged.xcorr_lag0),
    ('`summary_xcorr`, lags 0..4', lambda s, a: xcorr(s, a, 4, True), None),
    ('`summary_kme`, 256 features, c = 1', lambda s, a: embedding(s, a, 256, 1.0), ragged.embedding),
    ('`summary_sysid`, ridge 1e-3', lambda s, a: sysid(s, a, 1e-3), None),
)


def nll_pair(x, theta):
    nll = [final_nll(oest.OracleMDNN, x.float(), theta, seed, hidden_layers=(128, 128)) for seed in (0, 1)]
    return '%.2f / %.2f' % (nll[0], nll[1])


def fixed_length_table():
    theta, states, actions, lengths = pairs.cartpole_pairs(5000, 20, seed=0, terminate=True)
    print('(1) cartpole_pairs(5000, 20, seed=0): %d of 5000 episodes would end early under the end rule; the table '
          'is on the untruncated episodes' % int((lengths < 21).sum()))
    theta, states, actions = pairs.cartpole_pairs(5000, 20, seed=0)
    print('| summary | width | raw | standardised (first 800 rows) |')
    print('|---|---|---|---|')
    for name, fn, _ in SUMMARIES:
        x = fn(states, actions).float()
        print('| %s | %d | %s | %s |' % (name, x.shape[1], nll_pair(x, theta), nll_pair(standardised(x), theta)),
              flush=True)


def ended_table():
    theta, ended_s, ended_a, lengths = pairs.cartpole_pairs(5000, 50, seed=0, terminate=True)
    _, states, actions = pairs.cartpole_pairs(5000, 50, seed=0)
    lengths = lengths.numpy()
    print('(2) cartpole_pairs(5000, 50, seed=0, terminate=True): %d of 5000 episodes end early, mean length %.2f '
          'states, shortest %d' % (int((lengths < 51).sum()), lengths.mean(), lengths.min()))
    print('| summary | width | untruncated | (a) ended, no lengths | (b) with lengths |')
    print('|---|---|---|---|---|')
    for name, fn, with_lengths in SUMMARIES:
        cells = [nll_pair(standardised(fn(states, actions).float()), theta),
                 nll_pair(standardised(fn(ended_s, ended_a).float()), theta)]
        x = fn(ended_s, ended_a)
        if with_lengths is None:
            cells.append('no such form')
        else:
            x = with_lengths(ended_s, ended_a, lengths)
            assert np.isfinite(x.numpy()).all()
            cells.append(nll_pair(standardised(x.float()), theta))
        print('| %s | %d | %s |' % (name, x.shape[1], ' | '.join(cells)), flush=True)


def main(argv):
    if '--ended' not in argv:
        fixed_length_table()
    if '--fixed' not in argv:
        ended_table()


if __name__ == '__main__':
    main(sys.argv[1:])
