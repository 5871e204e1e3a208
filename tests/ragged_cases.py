"""The shared cases of the two summaries with per-trajectory lengths (include/bsig_ragged.h) and their definition
restated in numpy, in double, THROUGH the fixed-length restatements of tests/xcorr_cases.py and tests/kme_cases.py:
row i is what those give for ``states[i:i + 1, :L_i]`` and the whole ``actions[i:i + 1]``.  Nothing here touches the
library or the GPU.

The bounds are therefore the derived bounds of those two modules, evaluated per trajectory at its own length: no
new number.  A lag block with no term (``tau >= M_i``) is 0 with bound 0: the test asks for exactly +0.
"""
import numpy as np

import kme_cases as KC
import xcorr_cases as XC

# The cases, by the parents' names: the smallest shapes on which each kernel path can go wrong.  name -> n, the
# trajectories (None: the row counts around G of the parent's ``group_counts``).  Where the parent's n could not
# hold the lengths a case is about, it is a little larger here.
XCORR = {
    'pendulum_k4': None,          # 8 trajectories a workgroup with different M
    'pendulum_raw_k20': 37,       # L = 1: sigma exactly 0; most lags empty
    'ta_t_minus_1': 21, 'ta_1': 21, 'ta_above_t': 21,      # the padded action count depends on M_i
    'odd_width': 13,
    'ant': 6,                     # runs per column: seg_len per trajectory; vector stores
    'shadowhand': 5,              # whole columns a thread
    'shadowhand_t50': 4,          # in double: 512 threads
    'odd_ad_wide': 5,             # the mixed word
    'two_a_workgroup': None,
}
XCORR_IN_DOUBLE_ONLY = ('shadowhand_t50',)
KME = {
    'pendulum': None,
    'm100_time': 37,              # r per trajectory
    'm1_raw_time': 19,
    'edge_ts66': 7,               # M_i in {1, 31, 32, 33, 64, 65}
    'edge_ts65_raw': 7,
    'ta_1': 21, 'ta_above_t': 21,
    'ant': 5,
    'shadowhand_long': 4,         # 1, 2 and 4 blocks
    'five_tiles_two_blocks': 4,
    'constant_action': 9,
}
# lengths a case is about, in front of the seeded ones
_FIRST = {
    ('kme', 'edge_ts66'): [2, 32, 33, 34, 65, 66, 3],
    ('kme', 'edge_ts65_raw'): [1, 31, 32, 33, 64, 65, 2],
    ('kme', 'shadowhand_long'): [120, 2, 3, 60],
    ('kme', 'five_tiles_two_blocks'): [40, 2, 3, 33],
}


def shape_of(kind, name):
    """(ts, ta, sd, ad, diff) of a case, and Lmin."""
    if kind == 'xcorr':
        _, ts, ta, sd, ad, _, diff = XC.CASES[name]
    else:
        _, ts, ta, sd, ad, _, diff, _ = KC.CASES[name]
    return ts, ta, sd, ad, bool(diff), (2 if diff else 1)


def lengths_for(name, n, kind='xcorr'):
    """Seeded lengths of a case at ``n`` trajectories, int64 numpy: they always contain Lmin, ts and Lmin + 1 (in
    that order, as far as n and ts allow), for xcorr a length with M_i = K <= K (and Lmin's M_i = 1), and they
    alternate between the shorter and the longer half of Lmin..ts, so every group of two or more consecutive
    trajectories -- every workgroup's -- mixes short and long."""
    ts, _, _, _, diff, lmin = shape_of(kind, name)
    rng = np.random.RandomState(9176 + 131 * n + 17 * ts + (1 if kind == 'kme' else 0))
    mid = (lmin + ts) // 2
    short = rng.randint(lmin, mid + 1, size=n)
    long_ = rng.randint(min(mid + 1, ts), ts + 1, size=n)
    out = np.where(np.arange(n) % 2 == 0, short, long_).astype(np.int64)
    first = list(_FIRST.get((kind, name), [lmin, ts, min(lmin + 1, ts)]))
    if kind == 'xcorr' and XC.CASES[name][5] >= 1:
        first.append(min(XC.CASES[name][5] + (1 if diff else 0), ts))       # M_i = K: the last lag has no term
    out[:min(n, len(first))] = first[:n]
    assert ((out >= lmin) & (out <= ts)).all()
    return out


def steps_of(lengths, diff):
    return np.asarray(lengths, dtype=np.int64) - (1 if diff else 0)


def _place(small, k_i, k, sd, ad):
    """A row of k_i + 1 lag blocks in the layout of k + 1: the missing blocks are 0."""
    row = np.zeros(XC.width(sd, ad, k))
    cross = (k_i + 1) * sd * ad
    row[:cross] = small[:cross]
    row[-2 * sd:] = small[cross:]
    return row


def _xcorr_rows(fn, states, actions, lengths, k, diff):
    sd, ad = states.shape[2], actions.shape[2]
    rows = []
    for i, (length, m_i) in enumerate(zip(lengths, steps_of(lengths, diff))):
        k_i = int(min(k, m_i - 1))
        rows.append(_place(fn(states[i:i + 1, :length], actions[i:i + 1], k_i)[0], k_i, k, sd, ad))
    return np.stack(rows) if rows else np.zeros((0, XC.width(sd, ad, k)))


def xcorr_reference(states, actions, lengths, k, diff):
    """The rows of the definition with lengths, [N, width] in double."""
    return _xcorr_rows(lambda s, a, k_i: XC.reference(s, a, k_i, diff), states, actions, lengths, k, diff)


def xcorr_bounds(states, actions, lengths, k, diff, u):
    """Per output element the bound on |got - reference|: XC.bounds of every trajectory at its own length."""
    return _xcorr_rows(lambda s, a, k_i: XC.bounds(s, a, k_i, diff, u), states, actions, lengths, k, diff)


def kme_reference(states, actions, lengths, coeff, diff, time):
    return np.concatenate([KC.reference(states[i:i + 1, :length], actions[i:i + 1], coeff, diff, time)
                           for i, length in enumerate(lengths)], axis=0)


def kme_bounds(states, actions, lengths, coeff, diff, time, itemsize):
    return np.concatenate([KC.bounds(states[i:i + 1, :length], actions[i:i + 1], coeff, diff, time, itemsize)
                           for i, length in enumerate(lengths)], axis=0)


def kme_rows_compacted(states, actions, lengths, diff, time, dtype=np.float64, header_tau=False):
    """The valid rows only, trajectory after trajectory, [sum_i M_i, d] in ``dtype``: bsig_kme_rows_ragged's.
    ``header_tau``: in double too the time column is the header's t times the rounded reciprocal (two roundings,
    what the kernels form), not the definition's quotient."""
    d = KC.row_dim(states.shape[2], actions.shape[2], diff, time)
    parts = []
    for i, length in enumerate(lengths):
        x = KC.rows(states[i:i + 1, :length], actions[i:i + 1], diff, time, dtype).reshape(-1, d).copy()
        if time and header_tau:
            x[:, 0] = np.arange(x.shape[0], dtype=dtype) * (dtype(1) / dtype(max(x.shape[0] - 1, 1)))
        parts.append(x)
    return np.concatenate(parts, axis=0)


def end_episodes(states, actions, lengths):
    """pairs.end_episodes restated: the states from L_i on repeat state L_i - 1, the actions from step
    M_i = L_i - 1 on the last valid action."""
    lengths = np.asarray(lengths)
    t_s = np.minimum(np.arange(states.shape[1])[None, :], lengths[:, None] - 1)
    t_a = np.minimum(np.arange(actions.shape[1])[None, :], lengths[:, None] - 2)
    return states[np.arange(len(lengths))[:, None], t_s], actions[np.arange(len(lengths))[:, None], t_a]
