"""The shared cases of the random-feature kernel mean embedding summary (include/bsig_kme.h) and its definition
restated in numpy, in double: what tests/test_kme_host.py and tests/test_gpu_kme.py compare with.  Nothing here
touches the library or the GPU.

The definition.  states [N, Ts, sd], actions [N, Ta, ad], T = Ts.
  a_t = actions[min(t, Ta - 1)];
  x_t = [tau_t? | s_t | a_t | s_(t+1) - s_t], t = 0..T-2, M = T - 1 (diff) or x_t = [tau_t? | s_t | a_t], M = T;
  tau_t = t / max(M - 1, 1) (time);   d = the width of x_t;
  z_t,j = sum_k x_t,k coeff_j,k for the m rows of coeff [m, d];
  row = [a/M sum_t cos z_t,j (j < m) | a/M sum_t sin z_t,j (j < m)], a = sqrt(1/m).
The coefficients: coeff[j, k] = round(((double)freqs[j, k] * inv_std[k]) * kappa), kappa = 1 / (scale sqrt(d)).

The error bound of ``bounds`` (u: the unit roundoff of the output precision; gamma(k) = k u / (1 - k u)).  The
inputs here are exactly representable in the precision the kernel computes in, and the reference takes the
coefficients as the kernel gets them (already rounded), so they carry no error.
  * x^_t,k.  A difference is one rounding; tau^_t = fl(t * fl(1 / max(M - 1, 1))) two; s and a none.
  * z^_t,j is a chain of d fmas in some order (the zero padding adds exact zeros): d roundings on top of its
    term's own, so |z^ - z| <= gamma(d + 2) sum_k |x_t,k| |coeff_j,k|.  The issue counts d + 3 (chain,
    difference and both roundings of the time product, although no term has all of them): ``bounds`` uses the
    issue's count, the looser one.  Call it E_t,j.
  * |cos z^ - cos z| <= |z^ - z|, and the computed cosine is within S of cos z^: S = 3e-6 in fp32, the
    figure tests/test_gpu_matmul.py holds the same sincosf epilogue to, and 8 u in double
    (test_rff_map_in_double).  The same for the sine.
  * The sum over t in any order puts at most M - 1 roundings on a term; the constant a/M is made in double
    (a division, a root, a division) and rounded, and multiplied in: M + 3 in all, the issue's count, on terms
    that are at most 1 + S + E in magnitude.
        |got - ref| <= a [ (1/M) sum_t (E_t,j + S) + gamma(M + 3) (1 + S + max_t E_t,j) ].
    The issue's form has gamma(M + 3) alone; the factor beside it keeps the second-order terms and makes this
    count the looser of the two by a relative 1e-5 or so.
The bound scales with the magnitudes that enter it and was not fitted to what the kernel gave.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
SINCOS = {4: 3e-6, 8: 8 * U64}       # the allowance for the sine and cosine themselves, by itemsize
BLOCK_ROWS = 32                      # BSIG_KME_BLOCK_ROWS

# name -> (n, Ts, Ta, sd, ad, m, diff, time).  n = None: the row counts around the trajectories per workgroup, G,
# that the library answers for the shape (test_gpu_kme.py asks bsig_kme_group).
CASES = {
    # Pendulum: M = 20 in one partial block, odd d = 7
    'pendulum': (None, 21, 21, 3, 1, 128, 1, 0),
    # the reference's 200 features: no multiple of a column tile; the time column
    'm100_time': (37, 21, 21, 3, 1, 100, 1, 1),
    'm2': (19, 5, 5, 3, 1, 2, 1, 0),
    # M = 1, tau = 0
    'm1_diff_time': (19, 2, 2, 3, 1, 32, 1, 1),
    'm1_raw_time': (19, 1, 1, 3, 2, 32, 0, 1),
    # block edges: M = 31, 32, 33, 64, 65 (d = 10: a partial group of 8 columns), and M = 65 without differences
    'edge_ts32': (7, 32, 32, 4, 2, 33, 1, 0),
    'edge_ts33': (7, 33, 33, 4, 2, 33, 1, 0),
    'edge_ts34': (7, 34, 34, 4, 2, 33, 1, 0),
    'edge_ts65': (7, 65, 65, 4, 2, 33, 1, 0),
    'edge_ts66': (7, 66, 66, 4, 2, 33, 1, 0),
    'edge_ts65_raw': (7, 65, 65, 4, 2, 33, 0, 0),
    # the actions' padding: n + 1 states and n actions, one action, more actions than states
    'ta_t_minus_1': (21, 21, 20, 3, 1, 16, 1, 0),
    'ta_1': (21, 12, 1, 4, 2, 16, 1, 1),
    'ta_above_t': (21, 12, 17, 4, 2, 16, 0, 0),
    # d = 128, two blocks
    'ant': (5, 50, 49, 60, 8, 128, 1, 0),
    # d = 442: a 56 KB block; and a trajectory that is longer than a workgroup's LDS as a whole (four blocks)
    'shadowhand': (3, 40, 40, 211, 20, 64, 1, 0),
    'shadowhand_long': (2, 120, 120, 211, 20, 64, 1, 0),
    # more column tiles than wavefronts: the items of one block, and a second walk over a longer trajectory
    'five_tiles_one_block': (None, 9, 9, 3, 1, 160, 1, 0),
    'five_tiles_two_blocks': (3, 40, 40, 4, 2, 150, 1, 1),
    # a constant action column: inv_std = 0, a zero coefficient column, a finite output
    'constant_action': (9, 21, 21, 3, 2, 16, 1, 0),
}
CONSTANT_ACTION = ('constant_action',)
IN_DOUBLE = ('pendulum', 'm100_time', 'edge_ts32', 'edge_ts33', 'edge_ts34', 'edge_ts65', 'edge_ts66',
             'edge_ts65_raw', 'shadowhand', 'shadowhand_long')


def group_counts(g):
    """Row counts around G trajectories a workgroup: 1, G - 1, G, G + 1, 2 G + 1."""
    return sorted({1, max(g - 1, 1), g, g + 1, 2 * g + 1})


def row_dim(sd, ad, diff, time):
    return (2 if diff else 1) * sd + ad + (1 if time else 0)


def steps(ts, diff):
    return ts - 1 if diff else ts


def trajectories(n, ts, ta, sd, ad, seed=0, constant_action=False):
    """Seeded fp32-representable trajectories as float32 numpy arrays (states ~ N(0, 1) + a per-trajectory
    offset, actions in [-1, 1); ``constant_action``: action column 0 is 0.5 everywhere)."""
    rng = np.random.RandomState(1000003 * seed + 7919 * n + 101 * ts + 13 * sd + ad)
    states = (rng.standard_normal((n, ts, sd)) + 2.0 * rng.standard_normal((n, 1, sd))).astype(np.float32)
    actions = (2.0 * rng.random_sample((n, ta, ad)) - 1.0).astype(np.float32)
    if constant_action:
        actions[:, :, 0] = 0.5
    return states, actions


def rows(states, actions, diff, time, dtype=np.float64):
    """The rows x_t, [N, M, d], in ``dtype``: in double they are the definition's (exact for fp32 data, tau the
    rounded quotient); in float32 every difference and tau = t * (1 / max(M - 1, 1)) is rounded as the kernels
    round it, so they are bsig_kme_rows' bit for bit."""
    s, a = np.asarray(states, dtype=dtype), np.asarray(actions, dtype=dtype)
    n, ts, _ = s.shape
    m = steps(ts, diff)
    assert m >= 1
    at = a[:, np.minimum(np.arange(m), a.shape[1] - 1)]
    parts = []
    if time:
        t = np.arange(m, dtype=dtype)
        if dtype == np.float64:
            tau = t / max(m - 1, 1)
        else:
            tau = t * (dtype(1) / dtype(max(m - 1, 1)))
        parts.append(np.broadcast_to(tau.astype(dtype)[None, :, None], (n, m, 1)))
    parts += [s[:, :m], at]
    if diff:
        parts.append(s[:, 1:] - s[:, :-1])
    out = np.concatenate(parts, axis=2)
    assert out.dtype == dtype and out.shape[2] == row_dim(s.shape[2], a.shape[2], diff, time)
    return out


def flat_rule_inv_std(x, u=2.0 ** -23):
    """inv_std of the columns of rows x [R, d] by the rule of include/bsig_input_norm.h (population form)."""
    mean, std = x.mean(axis=0), x.std(axis=0)
    flat = std <= 8.0 * u * np.abs(mean)
    return np.where(flat, 0.0, 1.0 / np.where(flat, 1.0, std))


def kappa(scale, d):
    return 1.0 / (scale * np.sqrt(float(d)))


def coefficients(freqs, inv_std, kap, dtype):
    """bsig_kme_coeff restated: two double multiplications, left to right, one rounding to ``dtype``."""
    first = np.asarray(freqs, dtype=np.float64) * np.asarray(inv_std, dtype=np.float64)[None, :]
    return (first * np.float64(kap)).astype(dtype)


def case_inputs(name, n):
    """(states, actions, freqs fp32 [m, d], inv_std double [d]) of a case at ``n`` rows: the coefficients are
    standard normal x inv_std / sqrt(d), so |z| stays below about 8."""
    _, ts, ta, sd, ad, m, diff, time = CASES[name]
    states, actions = trajectories(n, ts, ta, sd, ad, constant_action=name in CONSTANT_ACTION)
    d = row_dim(sd, ad, diff, time)
    freqs = np.random.RandomState(17 + m + d).standard_normal((m, d)).astype(np.float32)
    inv_std = flat_rule_inv_std(rows(states, actions, diff, time).reshape(-1, d))
    return states, actions, freqs, inv_std


def reference(states, actions, coeff, diff, time):
    """The rows of the definition, [N, 2 m] in double, for coefficients as the kernel gets them."""
    x = rows(states, actions, diff, time)
    c = np.asarray(coeff, dtype=np.float64)
    z = np.einsum('ntk,jk->ntj', x, c)
    a_over_m = np.sqrt(1.0 / c.shape[0]) / x.shape[1]
    return np.concatenate([np.cos(z).sum(axis=1), np.sin(z).sum(axis=1)], axis=1) * a_over_m


def _gamma(k, u):
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def bounds(states, actions, coeff, diff, time, itemsize):
    """Per output element the bound on |got - reference| of the module's docstring, [N, 2 m] in double."""
    u, s_allow = (U64, SINCOS[8]) if itemsize == 8 else (U32, SINCOS[4])
    x = rows(states, actions, diff, time)
    c = np.asarray(coeff, dtype=np.float64)
    m_steps, d = x.shape[1], x.shape[2]
    e = _gamma(d + 3, u) * np.einsum('ntk,jk->ntj', np.abs(x), np.abs(c))
    half = np.sqrt(1.0 / c.shape[0]) * ((e + s_allow).mean(axis=1) +
                                        _gamma(m_steps + 3, u) * (1.0 + s_allow + e.max(axis=1)))
    return np.concatenate([half, half], axis=1)
