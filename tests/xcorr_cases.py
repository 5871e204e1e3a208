"""The shared cases of the time-lagged cross-correlation summary (include/bsig_xcorr.h) and its definition
restated in numpy, in double: what tests/test_xcorr_host.py and tests/test_gpu_xcorr.py compare with.  Nothing
here touches the library or the GPU.

The definition.  states [N, Ts, sd], actions [N, Ta, ad], T = Ts.
  a_t = actions[min(t, Ta - 1)] for t < T;
  f_t = s_(t+1) - s_t, M = T - 1 (state_diff) or f_t = s_t, M = T;
  c_tau[i, j] = 1/(M - tau) sum_{t < M - tau} f_(t+tau),i a_t,j for tau = 0..K;
  mu_i = 1/M sum_t f_t,i;  sigma_i = sqrt(1/M sum_t (f_t,i - mu_i)^2), two passes;
  row = [c_0 | ... | c_K | mu | sigma], each c_tau flattened with i major.

The error bounds of ``bounds`` (u: the unit roundoff of the output precision; gamma(k) = k u / (1 - k u), the
usual constant for k roundings in a row, so nothing is dropped as "second order").  The kernel runs one fma
chain per output over ascending t and multiplies by a rounded reciprocal at the end; its inputs here are
exactly representable in the precision it computes in.
  * cross term, m = M - tau steps.  Each f is one rounded difference (exact without state_diff: d = 0
    roundings, else d = 1); the chain is m fmas, each one rounding of a partial sum that is at most the sum of
    the |products| (the first adds to zero and is exact: counted all the same); the reciprocal is one rounding
    and its multiply another.  With every factor (1 + delta), |delta| <= u, collected per term:
        |got - ref| <= gamma(m + d + 2) * (1/m) sum_t |f_(t+tau),i| |a_t,j|.
    (The issue counts m + 4 with and m + 3 without the difference: one more than this.  ``bounds`` uses the
    issue's count, which is the looser of the two and therefore holds as well.)
  * mu, M steps: the same chain with a_t = 1:  E_mu = gamma(M + d + 2) * (1/M) sum_t |f_t,i|.
  * sigma.  The thread forms d^_t = fl(f^_t - mu^): |d^_t - d_t| <= e_t with
        e_t = u |f_t| d + E_mu + u (|d_t| + u |f_t| d + E_mu)
    (the error of f^_t, of mu^, and the subtraction's own rounding of a value that is at most |d_t| plus the
    two).  The chain sums d^_t^2: |d^_t^2 - d_t^2| <= 2 |d_t| e_t + e_t^2, and its M roundings, the
    reciprocal and the multiply act on a sum of squares that is at most sum_t (|d_t| + e_t)^2:
        Dv = (1/M) sum_t (2 |d_t| e_t + e_t^2) + gamma(M + 2) (1/M) sum_t (|d_t| + e_t)^2
    bounds the error of the variance v^ against v = sigma^2.  |sqrt(v^) - sqrt(v)| is at most Dv / sigma (the
    two roots sum to sigma or more) and at most sqrt(Dv) (whatever sigma, a constant column included); the
    root itself is one more rounding of a value that is at most sigma plus that:
        |got - ref| <= E + u (sigma + E),  E = min(Dv / sigma, sqrt(Dv)).
    For M = 1 everything above is zero: d^_0 = fl(f^_0 - fl(f^_0 * 1)) = 0 and the test asks for exactly 0.
Every bound scales with the magnitudes that enter it (|f|, |a|, |d|), none with the result.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53

# name -> (n, Ts, Ta, sd, ad, max_lag, state_diff).  n = None: the row counts around the trajectories per
# workgroup, G, that the library answers for the shape (test_gpu_xcorr.py asks bsig_xcorr_group).
CASES = {
    # Pendulum: 9 outputs (16 trajectories a workgroup), 21 (8 a workgroup); K 19 is M - 1, a one-term lag
    'pendulum_k0': (None, 21, 21, 3, 1, 0, True),
    'pendulum_k4': (None, 21, 21, 3, 1, 4, True),
    'pendulum_k19': (37, 21, 21, 3, 1, 19, True),
    'pendulum_raw_k20': (37, 21, 21, 3, 1, 20, False),
    # M = 1: sigma is exactly 0
    'm1_diff': (19, 2, 2, 3, 1, 0, True),
    'm1_raw': (19, 1, 1, 3, 2, 0, False),
    # the actions' padding: n + 1 states and n actions, one action, more actions than states
    'ta_t_minus_1': (21, 21, 20, 3, 1, 4, True),
    'ta_t_minus_1_raw': (21, 21, 20, 3, 2, 4, False),
    'ta_1': (21, 12, 1, 4, 2, 3, True),
    'ta_above_t': (21, 12, 17, 4, 2, 3, False),
    # a width that is no multiple of 4 (nor of 2): 3 * 9 + 6 = 33
    'odd_width': (13, 9, 9, 3, 3, 2, True),
    # a trajectory takes the whole workgroup; the vector stores (2520 outputs); columns cut into runs (60 < 256)
    'ant': (5, 50, 50, 60, 8, 4, True),
    'ant_k0': (5, 50, 49, 60, 8, 0, True),
    # wider than a workgroup has threads: whole columns a thread (211 < 256), 8862 outputs; and sd above 256
    'shadowhand': (3, 10, 10, 211, 20, 1, True),
    'sd_above_threads': (3, 6, 6, 300, 2, 1, True),
    # a trajectory beyond half a CU's LDS in double (92 KB): the workgroup of 512 threads
    'shadowhand_t50': (3, 50, 50, 211, 20, 1, True),
    # 16-byte words of outputs whose chains do not share their state (ad 5), one word that holds the last cross
    # terms and the first means (615 cross terms), one that holds the last means and the first deviations (sd 41)
    'odd_ad_wide': (4, 8, 8, 41, 5, 2, True),
    # two and four trajectories a workgroup (65..128 and 33..64 outputs)
    'two_a_workgroup': (None, 15, 15, 10, 4, 1, True),
    'four_a_workgroup': (None, 15, 14, 6, 3, 1, False),
}


def group_counts(g):
    """Row counts around G trajectories a workgroup: 1, G - 1, G, G + 1, 3 G + 2."""
    return sorted({1, max(g - 1, 1), g, g + 1, 3 * g + 2})


def width(sd, ad, max_lag):
    return (max_lag + 1) * sd * ad + 2 * sd


def trajectories(n, ts, ta, sd, ad, seed=0):
    """Seeded fp32-representable trajectories as float32 numpy arrays (states ~ N(0, 1) + a per-trajectory
    offset, so the columns' means are not all near zero; actions in [-1, 1))."""
    rng = np.random.RandomState(1000003 * seed + 7919 * n + 101 * ts + 13 * sd + ad)
    states = (rng.standard_normal((n, ts, sd)) + 2.0 * rng.standard_normal((n, 1, sd))).astype(np.float32)
    actions = (2.0 * rng.random_sample((n, ta, ad)) - 1.0).astype(np.float32)
    return states, actions


def features(states, actions, state_diff):
    """(f [N, M, sd], a [N, M, ad]) in double."""
    s, a = np.asarray(states, dtype=np.float64), np.asarray(actions, dtype=np.float64)
    t, ta = s.shape[1], a.shape[1]
    f = s[:, 1:] - s[:, :-1] if state_diff else s
    m = f.shape[1]
    assert m >= 1
    return f, a[:, np.minimum(np.arange(m), ta - 1)]


def reference(states, actions, max_lag=0, state_diff=True):
    """The rows of the definition, [N, width] in double."""
    f, a = features(states, actions, state_diff)
    n, m, sd = f.shape
    assert 0 <= max_lag <= m - 1
    parts = []
    for tau in range(max_lag + 1):
        c = np.einsum('nti,ntj->nij', f[:, tau:], a[:, :m - tau]) / (m - tau)
        parts.append(c.reshape(n, -1))
    mu = f.sum(axis=1) / m
    sigma = np.sqrt(((f - mu[:, None, :]) ** 2).sum(axis=1) / m)
    return np.concatenate(parts + [mu, sigma], axis=1)


def _gamma(k, u):
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def bounds(states, actions, max_lag, state_diff, u):
    """Per output element the bound on |got - reference| of the module's docstring, [N, width] in double."""
    f, a = features(states, actions, state_diff)
    n, m, sd = f.shape
    d = 1 if state_diff else 0
    fa, aa = np.abs(f), np.abs(a)
    parts = []
    for tau in range(max_lag + 1):
        cnt = m - tau
        mag = np.einsum('nti,ntj->nij', fa[:, tau:], aa[:, :cnt]) / cnt
        parts.append((_gamma(cnt + 3 + d, u) * mag).reshape(n, -1))      # the issue's m + 4 / m + 3
    e_mu = _gamma(m + d + 2, u) * fa.sum(axis=1) / m
    mu = f.sum(axis=1) / m
    dev = np.abs(f - mu[:, None, :])
    sigma = np.sqrt((dev ** 2).sum(axis=1) / m)
    e_t = u * d * fa + e_mu[:, None, :]
    e_t = e_t + u * (dev + e_t)
    dv = (2.0 * dev * e_t + e_t ** 2).sum(axis=1) / m + _gamma(m + 2, u) * ((dev + e_t) ** 2).sum(axis=1) / m
    with np.errstate(divide='ignore', invalid='ignore'):
        by_sigma = np.where(sigma > 0, dv / sigma, np.inf)
    e = np.minimum(by_sigma, np.sqrt(dv))
    e_sigma = e + u * (sigma + e)
    if m == 1:
        e_sigma = np.zeros_like(e_sigma)
    return np.concatenate(parts + [e_mu, e_sigma], axis=1)
