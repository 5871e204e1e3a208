"""What the closed-loop rollout tests (tests/test_sim_policy_host.py, tests/test_gpu_sim_policy.py) share: the
policy of include/bsig_sim_policy.h restated unit by unit in numpy (not from bayes_sim_ig_amd/pairs.py), seeded
policies with fp32-representable weights, the case tables, and the bound of the action check.  The steps, the
draws and the step-by-step check are tests/sim_cases.py's, unchanged.

The action check.  The numpy policy below is applied to the kernel's OWN double state t (the observation the
kernel's thread held, stored unrounded by the double entry point) and e_t, and compared with its
actions_out[t].  Both sides run the SAME sequence of correctly rounded double operations (z_j = b_j, then for k
ascending z_j = z_j + W_jk x_k; nothing contracted), so with the identity or relu, or without a hidden layer, they
agree BITWISE and are compared so.  With tanh they differ by their libraries' tanh: each is allowed
sigma = 8 u in absolute value, the project's allowance for a double library function (sim_cases.SINCOS, whose
form this is: |tanh| <= 1 as |sin| <= 1), so two values that each carry it differ by dt = 2 sigma.  With
gamma(k) = k u / (1 - k u) and a formula of k operations costing gamma(k) of its absolute form on EACH side,
2 gamma(k), as in sim_cases:
  layer 1:  z1_j from the same bits on both sides: no difference.       d_h1_j = dt;
  layer 2:  z2_j = b_j + sum_k W_jk h1_k, 2 h0 operations:
            d_z2_j = sum_k |W_jk| d_h1_k + 2 gamma(2 h0) (|b_j| + sum_k |W_jk| |h1_k|);
            h2_j = tanh(z2_j), |tanh'| <= 1:                            d_h2_j = d_z2_j + dt;
  output:   y = b + sum_j W_j h_j over the last hidden layer h (width h), 2 h operations:
            d_y = sum_j |W_j| d_h_j + 2 gamma(2 h) (|b| + sum_j |W_j| |h_j|);
  action:   a = y + e, one operation:                                   d_a = d_y + 2 gamma(1) (|y| + |e|).
Every magnitude is evaluated from the numpy reference, per element; no constant was fitted to what a kernel gave.
"""
import numpy as np

import sim_cases as SC

UNITS = 4                  # BSIG_SIM_POLICY_UNITS: the units of a layer the kernel forms side by side
MAX_WIDTH = 64             # BSIG_SIM_POLICY_MAX_WIDTH
ACTIVATIONS = ('identity', 'relu', 'tanh')
STEPS = (1, 7, 8, 9, 17)   # around the step block B = 8 (T + 1 states are walked in blocks of B)
# the issue's hidden shapes, and the widths just below, at and above UNITS in either layer
HIDDEN = ((), (1,), (UNITS - 1,), (UNITS,), (UNITS + 1,), (16,), (64,), (3, 64), (64, 1), (UNITS, UNITS + 1),
          (UNITS + 1, UNITS), (64, 64))
TANH = 8 * SC.U64          # the allowance for a double tanh: sim_cases.SINCOS' form


def hidden_id(hidden):
    return 'h' + ('x'.join(str(h) for h in hidden) or '0')


def make_policy(task, hidden, seed=0, scale=1.0):
    """(weights, biases) of a policy on ``task``'s observation: float64 arrays of fp32-representable values,
    W_l uniform in [-1, 1] / sqrt(in_l) times ``scale``, b_l uniform in [-0.1, 0.1]."""
    rs = np.random.RandomState(1000 + seed)
    widths = (SC.DIMS[task][2],) + tuple(hidden) + (1,)
    weights, biases = [], []
    for fan_in, fan_out in zip(widths[:-1], widths[1:]):
        w = rs.uniform(-1.0, 1.0, size=(fan_out, fan_in)) * (scale / np.sqrt(fan_in))
        weights.append(w.astype(np.float32).astype(np.float64))
        biases.append(rs.uniform(-0.1, 0.1, size=fan_out).astype(np.float32).astype(np.float64))
    return weights, biases


def activate(z, activation):
    if activation == 'relu':
        return np.where(z < 0, 0.0, z)
    return np.tanh(z) if activation == 'tanh' else z


def layer(w, b, x):
    """[..., in] -> [..., out], one unit at a time: z_j = b_j, then k ascending z_j = z_j + W_jk x_k."""
    out = np.empty(x.shape[:-1] + (w.shape[0],))
    for j in range(w.shape[0]):
        z = np.full(x.shape[:-1], b[j])
        for k in range(w.shape[1]):
            z = z + w[j, k] * x[..., k]
        out[..., j] = z
    return out


def policy_ref(weights, biases, activation, obs):
    """pi(obs) by the definition, obs [..., in] double -> [...]."""
    x = np.asarray(obs, dtype=np.float64)
    with np.errstate(all='ignore'):
        for l, (w, b) in enumerate(zip(weights, biases)):
            x = layer(w, b, x)
            if l + 1 < len(weights):
                x = activate(x, activation)
    return x[..., 0]


def action_bound(weights, biases, activation, obs, e):
    """(pi(obs) + e, the bound d_a of the module's docstring), per element.  The bound is 0 -- compare bitwise
    -- unless the activation is tanh and there is a hidden layer."""
    x = np.asarray(obs, dtype=np.float64)
    ref = policy_ref(weights, biases, activation, x) + e
    if activation != 'tanh' or len(weights) == 1:
        return ref, np.zeros_like(ref)
    dt = 2.0 * TANH
    h = np.tanh(layer(weights[0], biases[0], x))
    d_h = np.full(h.shape, dt)
    for w, b in zip(weights[1:-1], biases[1:-1]):
        k = w.shape[1]
        d_z = d_h @ np.abs(w).T + 2 * SC.gamma(2 * k) * (np.abs(b) + np.abs(h) @ np.abs(w).T)
        h = np.tanh(layer(w, b, h))
        d_h = d_z + dt
    w, b = weights[-1], biases[-1]
    k = w.shape[1]
    y = layer(w, b, h)[..., 0]
    d_y = (d_h @ np.abs(w).T)[..., 0] + 2 * SC.gamma(2 * k) * (np.abs(b[0]) + (np.abs(h) @ np.abs(w).T)[..., 0])
    return ref, d_y + 2 * SC.gamma(1) * (np.abs(y) + np.abs(e))


def replace_marks(n, ta, seed=0, frac=0.3):
    """uint8 [n, ta]: a mixed mask, about ``frac`` ones."""
    return (np.random.RandomState(2000 + seed).uniform(size=(n, ta)) < frac).astype(np.uint8)


def closed_loop_by_steps(task, weights, biases, activation, params, init, actions, replace, steps):
    """The definition of include/bsig_sim_policy.h step by step, without ends: (states [n, T + 1, sd],
    actions_out [n, T + 1, 1]) in double, from sim_cases' own steps and the policy above."""
    params, init = params.astype(np.float64), init.astype(np.float64)
    actions = actions.astype(np.float64)
    n, ta = actions.shape[:2]
    sd = SC.DIMS[task][2]
    states, acts = np.empty((n, steps + 1, sd)), np.empty((n, steps + 1, 1))
    state = init
    with np.errstate(all='ignore'):
        for t in range(steps + 1):
            if task == 'pendulum':
                obs = np.stack([np.cos(state[:, 0]), np.sin(state[:, 0]), state[:, 1]], axis=1)
            else:
                obs = state
            states[:, t] = obs
            if t == steps:
                break
            i = min(t, ta - 1)
            e = actions[:, i, 0]
            a = policy_ref(weights, biases, activation, obs) + e
            if replace is not None:
                a = np.where(replace[:, i] != 0, e, a)
            acts[:, t, 0] = a
            if task == 'pendulum':
                r = SC.pendulum_parts(params, state[:, 0], state[:, 1], a)
                state = np.stack([r['th1'], r['thdot1']], axis=1)
            else:
                state = SC.cartpole_parts(params, state, a)['new']
    acts[:, steps] = acts[:, steps - 1]
    return states, acts


def ends_case(steps):
    """The case of the ends under a policy (CartPole, terminate): the `wide` draws of 3 W + 2 episodes with T
    actions, a seeded (16,) tanh policy's (weights, biases), e the drawn actions.  tests/test_sim_policy_host.py
    asserts on the HOST path that lengths from 2 upward occur, and every length in 2..T + 1 for T = 9 and 17."""
    params, init, actions = SC.draws('cartpole', SC.COUNTS[-1], steps, seed=steps, wide=True)
    weights, biases = make_policy('cartpole', (16,), seed=steps)
    return params, init, actions, weights, biases
