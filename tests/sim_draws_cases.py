"""What the drawn-rollout tests (tests/test_sim_draws_host.py, tests/test_gpu_sim_draws.py) share: the known
answers of Philox4x32-10, the case tables, seeded bounds, and the bounds of the checks.  The tasks' steps, the
policies and the step-by-step criterion are tests/sim_cases.py's and tests/sim_policy_cases.py's, unchanged.

The Gaussian bound.  z = sqrt(-2 log(u1)) cos(2 pi u2).  The device and numpy evaluate log and cos on BITWISE
identical arguments (u1, u2 and 6.283185307179586 u2 are exact or one shared rounding), so what separates them is
the libraries' documented error and the roundings of the root and the product on each side, in ulps of the value:
  device (OpenCL full profile, which the device library documents): log 3 ulp, halved by the root: 1.5; the
    correctly rounded root 0.5; cos 4; the product 0.5: 6.5;
  numpy (glibc: 1 ulp each): log 1, halved: 0.5; the root 0.5; cos 1; the product 0.5: 2.5.
Together 9 ulp; with a noise_std other than 1 the product noise_std z adds one rounding of 0.5 ulp a side: 10.
The bound is GAUSS_ULPS = 10 units of 2^-52 of the reference value (an ulp is at most 2^-52 of the value), whatever
noise_std.  Nothing here was fitted to what a kernel gave.

The distribution conditions of SANITY_N step draws of SANITY_SEED (5 standard errors each) are asserted on
``pairs.episode_draws`` by the host tests before any device test relies on them:
  |mean(v) - (lo + hi) / 2| <= 5 (hi - lo) / sqrt(12 n),  |mean(z)| <= 5 / sqrt(n),
  |mean(z^2) - 1| <= 5 sqrt(2 / n),  |mean(r) - frac| <= 5 sqrt(frac (1 - frac) / n).
"""
import numpy as np

KNOWN_ANSWERS = (       # counter, key, output (Random123's known-answer vectors of philox4x32_10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

TASKS = ('pendulum', 'cartpole')
COUNTS = (1, 63, 64, 65, 194)          # around one wavefront per workgroup
STEPS = (1, 7, 8, 9, 17)               # around the 8-step staging block
HIDDEN = (None, (), (5,), (16, 4))     # no policy, and the policies
EXACT_ACTIVATIONS = ('identity', 'relu')      # where bitwise equality is claimed
FRACS = (0.0, 0.3, 1.0)
STDS = (0.0, 1.0, 0.3)
GAUSS_ULPS = 10.0
SANITY_N, SANITY_SEED, SANITY_FRAC = 65536, 7, 0.3
SEED = 0x9E3779B97F4A7C15              # both words of the key in use
FIRST = 2 ** 32 - 70                   # the global index crosses 2^32 inside a launch of 194


def hidden_id(hidden):
    return 'open' if hidden is None else 'h' + ('x'.join(str(h) for h in hidden) or '0')


def bounds(task, wide=False):
    """Keyword bounds of an EpisodeDraws for ``task``: theta in [0.1, 2] (CartPole's cart mass the constant 1),
    the initial state as the task's collection draws it (``wide``: CartPole states from which episodes end at
    every step, as sim_cases.draws(wide=True)), actions in [-1, 1]."""
    if task == 'pendulum':
        return dict(lows=(0.1, 0.1), highs=(2.0, 2.0), init_lows=(-np.pi, -1.0), init_highs=(np.pi, 1.0),
                    act_low=-1.0, act_high=1.0)
    span = (2.3, 2.0, 0.2, 2.0) if wide else (0.05,) * 4
    return dict(lows=(0.1, 0.1, 1.0), highs=(2.0, 2.0, 1.0), init_lows=tuple(-s for s in span), init_highs=span,
                act_low=-1.0, act_high=1.0)


def sanity(v, z, r, lo, hi, frac):
    """The four conditions of the module's docstring: name -> (|statistic|, its limit)."""
    n = v.size
    assert n == z.size == r.size == SANITY_N
    return {'mean v': (abs(v.mean() - 0.5 * (lo + hi)), 5 * (hi - lo) / np.sqrt(12 * n)),
            'mean z': (abs(z.mean()), 5 / np.sqrt(n)),
            'mean z^2': (abs((z * z).mean() - 1.0), 5 * np.sqrt(2.0 / n)),
            'mean r': (abs(r.mean() - frac), 5 * np.sqrt(frac * (1 - frac) / n))}


def case_grid():
    """(task, hidden, activation, n, steps, frac, std, terminate): every N, T, hidden shape, frac_rnd, noise_std
    and both terminate values occur with each task; the tables are walked together, not multiplied."""
    cases = []
    for ti, task in enumerate(TASKS):
        i = 0
        for hidden in HIDDEN:
            for steps in STEPS:
                for n in COUNTS:
                    if hidden is not None or (i % 2 == 0):
                        cases.append((task, hidden, EXACT_ACTIVATIONS[(i + ti) % 2], n, steps,
                                      FRACS[i % 3], STDS[(i // 3) % 3], bool((i // 2 + ti) % 2)))
                    i += 1
    return cases
