"""What rolling out under a stabilising policy buys the estimator on CartPole (profiles/sim_policy_NOTES.md, the
README's paragraph), measured on the CPU with the oracle and numpy alone under the protocol of
tools/cartpole_cpu_table.py: an OracleMDNN with trunk [128, 128], 5 components, lr 1e-3, 5 chunks of 1000 pairs
with 100 updates of 100 rows, rows standardised by the first 800, the final held-out NLL at seeds 0 / 1.

  (1) The share of episodes that end, pairs.cartpole_pairs(4000, T, ..., seed=0, terminate=True) at T = 50 and
      200, theta in [0.1, 2]^2, cart mass 1, initial state U[-0.05, 0.05)^4: under random actions, under
      ``linear_feedback(CARTPOLE_BALANCE_GAINS)``, and under it with ``frac_rnd`` = 0.1 and 0.3 of the actions
      replaced by U[-1, 1] (the measurement in the comment of pairs.CARTPOLE_BALANCE_GAINS).
  (2) Per T and policy, on cartpole_pairs(5000, T, ..., seed=0, terminate=True): ``summary_start``,
      ``summary_xcorr`` at lag 0 and ``summary_kme`` (256 features, c = 1), both WITH the lengths, and
      ``summary_sysid`` (ridge 1e-3; it has no form with lengths) on the ended episodes.

Every summary is an existing restatement, imported.  The rollouts run on the host path of pairs.rollout.  The
oracle, the CPU: nothing here says anything about the GPU.  ``--shares``: (1) alone."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from bayes_sim_ig_amd import pairs
from oracle import summarize as osum
from tools import ragged_cpu_table as ragged
from tools.cartpole_cpu_table import nll_pair
from tools.input_norm_cpu_table import standardised
from tools.sysid_cpu_table import sysid

STEPS = (50, 200)
BALANCE = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
POLICIES = (('random', dict(policy='random')),
            ('balance gains', dict(policy=BALANCE)),
            ('balance gains, frac_rnd 0.1', dict(policy=BALANCE, frac_rnd=0.1)),
            ('balance gains, frac_rnd 0.3', dict(policy=BALANCE, frac_rnd=0.3)))
SUMMARIES = (('`summary_start`', lambda s, a, lengths: osum.summary_start(s, a)),
             ('`summary_xcorr`, lag 0, with lengths', ragged.xcorr_lag0),
             ('`summary_kme`, 256 features, c = 1, with lengths', ragged.embedding),
             ('`summary_sysid`, ridge 1e-3', lambda s, a, lengths: sysid(s, a, 1e-3)))


def shares():
    print('(1) the share of 4000 episodes that end (seed 0)')
    print('| policy | T = 50 | T = 200 |')
    print('|---|---|---|')
    for name, kw in POLICIES:
        cells = []
        for steps in STEPS:
            lengths = pairs.cartpole_pairs(4000, steps, seed=0, terminate=True, **kw)[3].numpy()
            ended = int((lengths < steps + 1).sum())
            cells.append('%d (%.2f %%), mean length %.1f' % (ended, 100.0 * ended / 4000, lengths.mean()))
        print('| %s | %s |' % (name, ' | '.join(cells)), flush=True)


def table():
    for steps in STEPS:
        print('(2) T = %d: final held-out NLL at seeds 0 / 1, standardised rows' % steps)
        data = []
        for name, kw in POLICIES:
            theta, states, actions, lengths = pairs.cartpole_pairs(5000, steps, seed=0, terminate=True, **kw)
            lengths = lengths.numpy()
            print('    %s: %d of 5000 end early, mean length %.1f' % (name, int((lengths < steps + 1).sum()),
                                                                     lengths.mean()))
            data.append((theta, states, actions, lengths))
        print('| summary | width | %s |' % ' | '.join(name for name, _ in POLICIES))
        print('|---|---|%s' % ('---|' * len(POLICIES)))
        for name, fn in SUMMARIES:
            cells = []
            for theta, states, actions, lengths in data:
                x = fn(states, actions, lengths)
                assert np.isfinite(x.numpy()).all()
                cells.append(nll_pair(standardised(x.float()), theta))
            print('| %s | %d | %s |' % (name, x.shape[1], ' | '.join(cells)), flush=True)


def main(argv):
    shares()
    if '--shares' not in argv:
        table()


if __name__ == '__main__':
    main(sys.argv[1:])
