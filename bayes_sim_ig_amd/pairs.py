"""(theta, trajectory) pair front end — what replaces Isaac Gym on this path.

The reference obtains training pairs from ``collect_trajectories`` over a
closed simulator (utils/collect_trajectories.py:15-93); its output contract is
``params [N, D]``, ``states [N, T+1, sd]``, ``actions [N, T+1, ad]`` (fp32).
This module produces tensors with that contract from

  * recorded pairs in the reference's regression-test ``.npz`` layout
    (``params`` [N, D], ``data`` [N, (T)*(sd+ad)] with [s_t | a_t] per step:
    bayes_sim_ig/tests/regression_tests.py:31-43), and
  * a vectorised restatement of the reference's numpy Pendulum
    (sim/openai_env_wrappers.py:77-93 reset, :153-177 dynamics; parameters
    (length, mass) ~ U[0.01, 2]^2 as in cfg/pendulum.yaml:36-50) driven by the
    reference's collection policies ``policy_random`` / ``policy_ones``
    (collect_trajectories.py:96-101), and
  * open-loop rollouts of the two analytic tasks, Pendulum and CartPole, with real episode ends
    (``rollout``, ``cartpole_pairs``; include/bsig_sim.h): on the device the tensors live on -- the HIP kernel
    for GPU tensors, its numpy restatement in double for CPU tensors; and the same rollouts closed loop, under
    an ``MLPPolicy`` evaluated step by step inside the kernel (``rollout(policy=, replace=)``,
    ``cartpole_pairs(policy=<MLPPolicy>)``; include/bsig_sim_policy.h): the reference's ``policy_rl`` and
    ``policy_rl_randomized`` (collect_trajectories.py) for an actor of up to two hidden layers; and
  * the same rollouts with every number -- theta, the initial state, the marks, the replacement actions, the
    exploration noise -- drawn inside the kernel by a counter-based generator (``rollout_drawn``, ``draw_pairs``;
    include/bsig_sim_draws.h): an episode is a function of (seed, global episode index) alone, and nothing is
    drawn on the host or copied.

The loaders and ``pendulum_pairs`` are host-side data preparation (numpy); not part of the accelerated path.
"""
import operator

import numpy as np
import torch

from . import _lib


def load_pairs_npz(path, state_dim, act_dim=1, device='cpu'):
    """-> (params [N,D], states [N,T,sd], actions [N,T,ad]) float32 tensors."""
    loaded = np.load(path)
    params = torch.from_numpy(np.asarray(loaded['params'])).float()
    data = torch.from_numpy(np.asarray(loaded['data'])).float()
    if params.dim() == 1:                      # a single recorded trajectory
        params, data = params.reshape(1, -1), data.reshape(1, -1)
    step = state_dim + act_dim
    assert data.shape[1] % step == 0, 'row width is not a multiple of state_dim + act_dim'
    sa = data.reshape(params.shape[0], -1, step)
    return (params.to(device), sa[:, :, :state_dim].contiguous().to(device),
            sa[:, :, state_dim:].contiguous().to(device))


def save_pairs_npz(path, params, states, actions):
    """Inverse of load_pairs_npz (same layout as the reference's test data)."""
    sa = torch.cat([states, actions], dim=-1).reshape(states.shape[0], -1)
    np.savez_compressed(path, params=params.detach().cpu().numpy().astype(np.float64),
                        data=sa.detach().cpu().numpy().astype(np.float64))


def pendulum_pairs(n, traj_len, policy='random', lows=(0.01, 0.01), highs=(2.0, 2.0),
                   params=None, seed=None, device='cpu'):
    """n Pendulum episodes of ``traj_len`` actions -> the collect_trajectories
    contract: params [n,2] = (length, mass), states [n, traj_len+1, 3] =
    (cos th, sin th, thdot), actions [n, traj_len+1, 1] in [-1,1] (the last
    action repeated, as pad_states_actions does).

    Dynamics (openai_env_wrappers.py:162-172): dt = 0.05, g = 10,
    torque u = clip(2*a, -2, 2);
      thdot' = thdot + (-3g/(2l) sin(th+pi) + 3/(m l^2) u) dt;  th' = th + thdot' dt;
      thdot' clipped to [-8, 8] after th' is formed.
    Initial state th ~ U[-pi, pi], thdot ~ U[-1, 1] (:85-90)."""
    rs = np.random.RandomState(seed) if seed is not None else np.random
    lows, highs = np.asarray(lows, dtype=np.float64), np.asarray(highs, dtype=np.float64)
    if params is None:
        theta = rs.uniform(lows, highs, size=(n, 2))
    else:
        theta = np.broadcast_to(np.asarray(params, dtype=np.float64), (n, 2)).copy()
    length, mass = theta[:, 0], theta[:, 1]
    th = rs.uniform(-np.pi, np.pi, size=n)
    thdot = rs.uniform(-1.0, 1.0, size=n)
    max_speed, max_torque, dt, g = 8.0, 2.0, 0.05, 10.0
    states = np.empty((n, traj_len + 1, 3))
    actions = np.empty((n, traj_len + 1, 1))
    states[:, 0] = np.column_stack([np.cos(th), np.sin(th), thdot])
    for t in range(traj_len):
        if policy in ('random', 'policy_random'):
            act = rs.rand(n)                                    # torch.rand_like: U[0,1)
        elif policy in ('ones', 'policy_ones'):
            act = np.ones(n)
        else:
            raise ValueError('unknown collection policy %r' % (policy,))
        u = np.clip(act * max_torque, -max_torque, max_torque)
        newthdot = thdot + (-3 * g / (2 * length) * np.sin(th + np.pi) +
                            3.0 / (mass * length ** 2) * u) * dt
        th = th + newthdot * dt
        thdot = np.clip(newthdot, -max_speed, max_speed)
        actions[:, t, 0] = act
        states[:, t + 1] = np.column_stack([np.cos(th), np.sin(th), thdot])
    actions[:, traj_len] = actions[:, traj_len - 1]             # pad (summarizers.py:52-58)
    to = lambda a: torch.from_numpy(a).float().to(device)      # noqa: E731
    return to(theta), to(states), to(actions)


def end_episodes(states, actions, lengths):
    """Copies of ``states`` [N, T, sd] and ``actions`` [N, Ta, ad] as a recorder leaves episodes that ended
    early: trajectory n's states from ``lengths[n]`` on repeat state ``lengths[n] - 1`` and its actions from step
    ``lengths[n] - 1`` on repeat the last valid action, ``lengths[n] - 2`` (``pad_states_actions``' rule at the
    episode's own end).  ``lengths``: N integers in 2..T, the valid STATES -- what ``summary_xcorr`` and
    ``summary_kme`` take as ``lengths=``."""
    lens = lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths))
    lens = lens.to(device=states.device, dtype=torch.int64)
    assert lens.shape == (states.shape[0],) and int(lens.min()) >= 2 and int(lens.max()) <= states.shape[1]
    t_s = torch.arange(states.shape[1], device=states.device)[None, :].minimum(lens[:, None] - 1)
    t_a = torch.arange(actions.shape[1], device=states.device)[None, :].minimum(lens[:, None] - 2)
    rows = torch.arange(states.shape[0], device=states.device)[:, None]
    return states[rows, t_s].clone(), actions[rows, t_a].clone()


# ---------------------------------------------------------------- rollouts of the analytic tasks (include/bsig_sim.h)
SIM_DIMS = {'pendulum': (2, 2, 3), 'cartpole': (3, 4, 4)}        # task -> (pd, id, sd): what bsig_sim_dims answers
CARTPOLE_X_LIMIT = 2.4
CARTPOLE_TH_LIMIT = 12 * 2 * np.pi / 360


def _pendulum_step(params, state, act):
    """One step of ``pendulum_pairs``' loop, operation for operation: (th, thdot) -> (th', thdot')."""
    length, mass = params[:, 0], params[:, 1]
    th, thdot = state[:, 0], state[:, 1]
    max_speed, max_torque, dt, g = 8.0, 2.0, 0.05, 10.0
    u = np.clip(act * max_torque, -max_torque, max_torque)
    newthdot = thdot + (-3 * g / (2 * length) * np.sin(th + np.pi) +
                        3.0 / (mass * length ** 2) * u) * dt
    th = th + newthdot * dt
    return np.stack([th, np.clip(newthdot, -max_speed, max_speed)], axis=1)


def _pendulum_observe(state):
    return np.stack([np.cos(state[..., 0]), np.sin(state[..., 0]), state[..., 1]], axis=-1)


def _cartpole_step(params, state, act):
    """One Euler step of the frictionless cart and pole (Barto, Sutton and Anderson 1983), every operation in
    the order include/bsig_sim.h writes it."""
    mp, l, mt = params[:, 0], params[:, 1], params[:, 0] + params[:, 2]
    x, xdot, th, thdot = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
    g, dt = 9.8, 0.02
    force = 10.0 * np.clip(act, -1.0, 1.0)
    s, c = np.sin(th), np.cos(th)
    mpl = mp * l
    tmp = (force + (mpl * (thdot * thdot)) * s) / mt
    tha = (g * s - c * tmp) / (l * (4.0 / 3.0 - (mp * (c * c)) / mt))
    xa = tmp - ((mpl * tha) * c) / mt
    return np.stack([x + dt * xdot, xdot + dt * xa, th + dt * thdot, thdot + dt * tha], axis=1)


def cartpole_ended(states):
    """The end condition of CartPole on observations ``[..., 4]`` (numpy, double): ``|x| > 2.4`` or
    ``|th| > 12 * 2 * pi / 360``."""
    return (np.abs(states[..., 0]) > CARTPOLE_X_LIMIT) | (np.abs(states[..., 2]) > CARTPOLE_TH_LIMIT)


_HOST_TASKS = {'pendulum': (_pendulum_step, _pendulum_observe, None),
               'cartpole': (_cartpole_step, lambda state: state, cartpole_ended)}


class MLPPolicy:
    """The policy of include/bsig_sim_policy.h: an MLP with 0, 1 or 2 hidden layers of 1..64 units, ONE output
    without an activation, and one activation ('identity', 'relu' or 'tanh') on every hidden layer.
    ``weights[l]`` is ``[out_l, in_l]`` and ``biases[l]`` ``[out_l]`` (arrays or tensors; kept as doubles, fp32
    values widened exactly).  The input width is checked against the task by ``rollout``.

    ``policy(obs)`` is the definition in numpy, double, on ``obs [..., in]``: ``z_j = b_j``, then for k ascending
    ``z_j = z_j + W_jk * x_k`` (two roundings a term); ``relu(z) = where(z < 0, 0, z)``.  ``to(device)`` packs the
    weights once per device (``W_0, b_0, W_1, b_1, ...``, one double tensor) and keeps them there.
    ValueError for anything that does not fit; the message names it."""
    ACTIVATIONS = ('identity', 'relu', 'tanh')

    def __init__(self, weights, biases, activation='tanh'):
        self._set(weights, biases, activation)

    def _set(self, weights, biases, activation):
        as_array = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)  # noqa: E731
        weights, biases = [as_array(w) for w in weights], [as_array(b) for b in biases]
        if len(weights) < 1 or len(weights) != len(biases):
            raise ValueError('weights and biases must hold one entry per layer, at least one, got %d and %d'
                             % (len(weights), len(biases)))
        if len(weights) - 1 > _lib.SIM_POLICY_MAX_HIDDEN:
            raise ValueError('weights: %d hidden layers, more than %d' % (len(weights) - 1, _lib.SIM_POLICY_MAX_HIDDEN))
        for l, (w, b) in enumerate(zip(weights, biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],) or (l == 0 and w.shape[1] < 1):
                raise ValueError('weights[%d] must be [out, in] and biases[%d] [out], got %r and %r'
                                 % (l, l, w.shape, b.shape))
            if l and w.shape[1] != weights[l - 1].shape[0]:
                raise ValueError('weights[%d] takes %d inputs, the layer before has %d units'
                                 % (l, w.shape[1], weights[l - 1].shape[0]))
        for l, w in enumerate(weights[:-1]):
            if not 1 <= w.shape[0] <= _lib.SIM_POLICY_MAX_WIDTH:
                raise ValueError('weights[%d]: a hidden width of %d is outside 1..%d'
                                 % (l, w.shape[0], _lib.SIM_POLICY_MAX_WIDTH))
        if weights[-1].shape[0] != 1:
            raise ValueError('weights[%d]: the policy has one output, got %d' % (len(weights) - 1, weights[-1].shape[0]))
        if activation not in self.ACTIVATIONS:
            raise ValueError('activation must be one of %r, got %r' % (self.ACTIVATIONS, activation))
        self.weights, self.biases, self.activation = weights, biases, activation
        self.in_dim = weights[0].shape[1]
        self.hidden = tuple(w.shape[0] for w in weights[:-1])
        self._packed = {}

    @classmethod
    def from_module(cls, module):
        """From a ``torch.nn.Sequential`` of ``Linear`` layers with ``Tanh``, ``ReLU`` or ``Identity`` between
        them (one kind throughout; none behind the last ``Linear``)."""
        nn = torch.nn
        kinds = {nn.Tanh: 'tanh', nn.ReLU: 'relu', nn.Identity: 'identity'}
        weights, biases, behind = [], [], []          # behind[l]: the activation behind Linear l
        for i, layer in enumerate(module):
            if isinstance(layer, nn.Linear):
                if layer.bias is None:
                    raise ValueError('module[%d]: a Linear without a bias' % i)
                weights.append(layer.weight), biases.append(layer.bias), behind.append('identity')
            elif type(layer) is nn.Identity:
                continue
            elif type(layer) in kinds and weights and behind[-1] == 'identity':
                behind[-1] = kinds[type(layer)]
            else:
                raise ValueError('module[%d]: %s where a Linear, or one Tanh / ReLU / Identity behind one, belongs'
                                 % (i, type(layer).__name__))
        if behind and behind[-1] != 'identity':
            raise ValueError('module: the last Linear is the output, no %s behind it' % behind[-1])
        if len(set(behind[:-1])) > 1:
            raise ValueError('module: one activation for all hidden layers, got %s' % sorted(set(behind[:-1])))
        return cls(weights, biases, behind[0] if len(behind) > 1 else 'identity')

    def packed(self):
        """The packed policy: one double array, ``W_0`` (row-major), ``b_0``, ``W_1``, ``b_1``, ..."""
        return np.concatenate([part.ravel() for w, b in zip(self.weights, self.biases) for part in (w, b)])

    def to(self, device):
        """Pack the weights on ``device`` (once: kept for later launches); returns ``self``."""
        self.packed_on(device)
        return self

    def packed_on(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._packed:
            self._packed[device] = torch.from_numpy(self.packed()).to(device)
        return self._packed[device]

    def __call__(self, obs):
        x = np.asarray(obs, dtype=np.float64)
        if x.shape[-1] != self.in_dim:
            raise ValueError('obs must be [..., %d], got %r' % (self.in_dim, x.shape))
        with np.errstate(all='ignore'):
            for l, (w, b) in enumerate(zip(self.weights, self.biases)):
                z = np.broadcast_to(b, x.shape[:-1] + b.shape).copy()
                for k in range(w.shape[1]):
                    z = z + w[:, k] * x[..., k:k + 1]
                if l + 1 < len(self.weights):
                    if self.activation == 'relu':
                        z = np.where(z < 0, 0.0, z)
                    elif self.activation == 'tanh':
                        z = np.tanh(z)
                x = z
        return x[..., 0]

    def state_dict(self):
        return {'weights': [w.copy() for w in self.weights], 'biases': [b.copy() for b in self.biases],
                'activation': self.activation}

    def load_state_dict(self, state):
        self._set(state['weights'], state['biases'], state['activation'])
        return self


def linear_feedback(gains, bias=0.0):
    """``a = gains . o + bias``: the policy without a hidden layer."""
    return MLPPolicy([np.asarray(gains, dtype=np.float64).reshape(1, -1)], [np.array([float(bias)])], 'identity')


# A feedback on (x, xdot, th, thdot) that keeps CartPole up.  Measured by tools/closed_loop_cpu_table.py --shares
# (host path, cartpole_pairs(4000, T, seed=0, terminate=True): theta in [0.1, 2]^2, cart mass 1, initial state
# U[-0.05, 0.05)^4): under it 0 of 4000 episodes end in 50 steps and 10 (0.25 %) in 200; under random actions
# 3069 (76.7 %) and 3999 (99.97 %, mean length 39.4 states); with frac_rnd = 0.1 of the actions replaced by
# U[-1, 1] 0 and 71 (1.8 %); with frac_rnd = 0.3, 6 (0.15 %) and 459 (11.5 %).
CARTPOLE_BALANCE_GAINS = (0.2, 0.5, 8.0, 1.5)


def _host_rollout(task, params, init, actions, n_steps, terminate, policy=None, replace=None):
    """The definition of include/bsig_sim.h (and, with a policy, of include/bsig_sim_policy.h) in numpy, double:
    (states, actions_out, lengths)."""
    step, observe, ended = _HOST_TASKS[task]
    n, ta = params.shape[0], actions.shape[1]
    states = np.empty((n, n_steps + 1, SIM_DIMS[task][2]))
    acts = np.empty((n, n_steps + 1, 1))
    lengths = np.full(n, n_steps + 1, dtype=np.int32)
    state = init
    states[:, 0] = observe(state)
    with np.errstate(all='ignore'):
        for t in range(n_steps):
            act = actions[:, min(t, ta - 1), 0]
            if policy is not None:                      # a_t = e_t where replaced, else pi(o_t) + e_t
                closed = policy(states[:, t]) + act
                act = closed if replace is None else np.where(replace[:, min(t, ta - 1)] != 0, act, closed)
            state = step(params, state, act)
            acts[:, t, 0] = act
            states[:, t + 1] = observe(state)
    acts[:, n_steps] = acts[:, n_steps - 1]
    if terminate and ended is not None and n:
        done = ended(states[:, 1:])                      # of states 1..T
        lengths = np.where(done.any(axis=1), done.argmax(axis=1) + 2, n_steps + 1).astype(np.int32)
        rows, t = np.arange(n)[:, None], np.arange(n_steps + 1)[None, :]
        states = states[rows, np.minimum(t, lengths[:, None] - 1)]
        acts = acts[rows, np.minimum(t, lengths[:, None] - 2)]
    return states, acts, lengths


def rollout(task, params, init, actions, n_steps=None, terminate=False, dtype=None, nonfinite=None, policy=None,
            replace=None):
    """Rollouts of ``task`` ('pendulum' or 'cartpole'), the definition of include/bsig_sim.h:
    ``params`` [N, pd], ``init`` [N, id] (the initial INTERNAL state), ``actions`` [N, Ta, 1] ->
    ``(states [N, T + 1, sd], actions_out [N, T + 1, 1], lengths [N] int32)``, T = ``n_steps``.

    Pendulum (pd 2: length, mass; id 2: th, thdot; sd 3: cos th, sin th, thdot) is exactly the loop of
    ``pendulum_pairs``: dt 0.05, g 10, ``u = clip(2 a, -2, 2)``,
    ``w = thdot + (-3 g / (2 l) sin(th + pi) + 3 / (m l^2) u) dt``, ``th' = th + w dt``, ``thdot' = clip(w, -8, 8)``;
    it never terminates.  CartPole (pd 3: pole mass m_p, pole half-length l, cart mass m_c; id and sd 4: x, xdot,
    th, thdot) is the frictionless cart and pole of Barto, Sutton and Anderson (1983) in Euler steps, g 9.8,
    dt 0.02: ``F = 10 clip(a, -1, 1)``, ``tmp = (F + m_p l thdot^2 sin th) / (m_p + m_c)``,
    ``tha = (g sin th - cos th tmp) / (l (4/3 - m_p cos^2 th / (m_p + m_c)))``,
    ``xa = tmp - m_p l tha cos th / (m_p + m_c)``, then x, xdot, th, thdot all step from the OLD values; it ends
    when the NEW state has ``|x| > 2.4`` or ``|th| > 12 * 2 * pi / 360``.

    The action of step t is ``actions[:, min(t, Ta - 1)]``; ``n_steps`` defaults to ``Ta - 1``, for actions that
    come padded as ``pendulum_pairs`` returns them.  With ``terminate`` an episode whose state j (1 <= j <= T) is
    the first to meet the end condition has length j + 1 (the terminal state is recorded), its states from there
    on repeat the terminal one and its actions from step j on repeat action j - 1: ``end_episodes``' rule, so
    ``lengths`` is what ``traj_lengths=`` / ``lengths=`` take.  Without it (and for Pendulum) the physics goes
    on, ``lengths`` are all T + 1 and ``actions_out[:, T]`` repeats step T - 1; the first ``lengths[n]`` states
    are bitwise the same either way.

    The state and every operation are double.  ``dtype`` follows the summarizers: ``None`` / ``torch.float32``
    takes the inputs as fp32 (a float64 input is narrowed) and returns the doubles rounded once;
    ``torch.float64`` widens the inputs and returns the doubles.  Tensors on a GPU launch the HIP kernel on
    their device (csrc/sim.h); CPU tensors run the numpy restatement on the host and never touch a GPU.  The
    two differ by the sine and cosine of their libraries alone.  ``nonfinite``: an optional 1-element int32
    tensor on the same device, set to 1 where a state is not finite (nothing is repaired or read back).
    ValueError, before any GPU call, for a shape, a device or an argument that does not fit; it names it.

    Closed loop (include/bsig_sim_policy.h).  With ``policy`` (an ``MLPPolicy`` whose input width is the task's
    sd) ``actions`` holds the exploration terms e and the action of step t is ``pi(o_t) + e_t``, one add, with
    ``o_t`` the observation in double before any rounding; where ``replace`` (optional, uint8 or bool ``[N, Ta]``
    on the same device, indexed like the actions) is not 0 it is ``e_t`` alone.  That action is what the step
    takes and what ``actions_out`` records; ends and fills are as above.  The policy is evaluated inside the
    kernel for GPU tensors and by ``policy(obs)`` on the host for CPU tensors; the two differ by their libraries'
    sine, cosine and tanh alone.  ``policy=None, replace=None`` is the open-loop call, unchanged."""
    if task not in SIM_DIMS:
        raise ValueError("task must be 'pendulum' or 'cartpole', got %r" % (task,))
    pd, idim, sd = SIM_DIMS[task]
    if dtype is None or dtype == torch.float32:
        prec = _lib.F32
    elif dtype == torch.float64:
        prec = _lib.F64
    else:
        raise ValueError('rollout stores torch.float32 or torch.float64, got dtype=%r' % (dtype,))
    for name, t in (('params', params), ('init', init), ('actions', actions)):
        if not torch.is_tensor(t) or not t.dtype.is_floating_point:
            raise ValueError('%s must be a floating-point tensor' % name)
    if params.dim() != 2 or params.shape[1] != pd:
        raise ValueError('params must be [N, %d] for %s, got %r' % (pd, task, tuple(params.shape)))
    n = params.shape[0]
    if tuple(init.shape) != (n, idim):
        raise ValueError('init must be [%d, %d] for %s, got %r' % (n, idim, task, tuple(init.shape)))
    if actions.dim() != 3 or actions.shape[0] != n or actions.shape[1] < 1 or actions.shape[2] != 1:
        raise ValueError('actions must be [%d, Ta >= 1, 1], got %r' % (n, tuple(actions.shape)))
    if init.device != params.device or actions.device != params.device:
        raise ValueError('params, init and actions must live on one device, got %s, %s, %s'
                         % (params.device, init.device, actions.device))
    ta = actions.shape[1]
    if n_steps is None:
        if ta < 2:
            raise ValueError('n_steps defaults to Ta - 1, which needs 2 actions or more, got %d' % ta)
        n_steps = ta - 1
    try:
        steps = None if isinstance(n_steps, bool) else operator.index(n_steps)
    except TypeError:
        steps = None
    if steps is None or not 1 <= steps < 2 ** 28:
        raise ValueError('n_steps must be an int >= 1, got %r' % (n_steps,))
    n_steps = steps
    if not isinstance(terminate, (bool, np.bool_)):
        raise ValueError('terminate must be a bool, got %r' % (terminate,))
    dev = params.device
    if nonfinite is not None and not (torch.is_tensor(nonfinite) and nonfinite.dtype == torch.int32
                                      and nonfinite.numel() == 1 and nonfinite.device == dev):
        raise ValueError('nonfinite must be a 1-element int32 tensor on %s' % (dev,))
    if policy is None:
        if replace is not None:
            raise ValueError('replace marks the steps that do not follow the policy: it needs policy=')
    else:
        if not isinstance(policy, MLPPolicy):
            raise ValueError('policy must be an MLPPolicy, got %r' % (type(policy).__name__,))
        if policy.in_dim != sd:
            raise ValueError('policy takes %d inputs, %s observes %d' % (policy.in_dim, task, sd))
        if replace is not None:
            if not torch.is_tensor(replace) or replace.dtype not in (torch.uint8, torch.bool) \
                    or tuple(replace.shape) != (n, ta):
                raise ValueError('replace must be a uint8 or bool tensor [%d, %d], got %s'
                                 % (n, ta, (replace.dtype, tuple(replace.shape)) if torch.is_tensor(replace)
                                    else type(replace).__name__))
            if replace.device != dev:
                raise ValueError('replace must live on %s with params, init and actions, got %s'
                                 % (dev, replace.device))
            replace = replace.detach().to(torch.uint8).contiguous()
    p, s0, a = (t.detach().to(prec.dtype).contiguous() for t in (params, init, actions))
    if not dev.type == 'cuda':
        states, acts, lengths = _host_rollout(task, p.double().numpy(), s0.double().numpy(), a.double().numpy(),
                                              n_steps, bool(terminate), policy,
                                              None if replace is None else replace.numpy())
        if nonfinite is not None and not np.isfinite(states).all():
            nonfinite.fill_(1)
        return (torch.from_numpy(states).to(prec.dtype), torch.from_numpy(acts).to(prec.dtype),
                torch.from_numpy(lengths))
    _lib.require_gpu()
    with _lib.device_stream(dev) as stream:
        states = torch.empty((n, n_steps + 1, sd), dtype=prec.dtype, device=dev)
        acts = torch.empty((n, n_steps + 1, 1), dtype=prec.dtype, device=dev)
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
        if policy is not None:
            hidden = policy.hidden + (0, 0)
            prec.sim_rollout_policy(_lib.SIM_TASKS[task], _lib.ptr(p), _lib.ptr(s0), _lib.ptr(a), _lib.ptr(replace),
                                    _lib.ptr(policy.packed_on(dev)), len(policy.hidden), hidden[0], hidden[1],
                                    _lib.SIM_ACTIVATIONS[policy.activation], _lib.ptr(states), _lib.ptr(acts),
                                    _lib.ptr(lengths), n, n_steps, ta, int(bool(terminate)), _lib.ptr(nonfinite),
                                    stream)
            return states, acts, lengths
        prec.sim_rollout(_lib.SIM_TASKS[task], _lib.ptr(p), _lib.ptr(s0), _lib.ptr(a), _lib.ptr(states),
                         _lib.ptr(acts), _lib.ptr(lengths), n, n_steps, ta, int(bool(terminate)),
                         _lib.ptr(nonfinite), stream)
    return states, acts, lengths


def cartpole_pairs(n, traj_len, policy='random', lows=(0.1, 0.1), highs=(2.0, 2.0), cart_mass=1.0,
                   params=None, seed=None, device='cpu', terminate=False, frac_rnd=0.0, noise_std=0.0):
    """n CartPole episodes of ``traj_len`` actions in ``pendulum_pairs``' contract: theta [n, 2] = (pole mass,
    pole half-length) with the cart's mass the constant ``cart_mass``, or, with three bounds, theta [n, 3] with
    the cart's mass drawn as well; states [n, traj_len + 1, 4] = (x, xdot, th, thdot); actions
    [n, traj_len + 1, 1] in [-1, 1], the last repeated; fp32 on ``device``.  With ``terminate=True`` also
    ``lengths`` [n] int32, and the episodes end as ``rollout`` states it.

    Every draw is made on the host from ``RandomState(seed)``, in this order: theta
    ``uniform(lows, highs, (n, 2 or 3))`` (none with ``params=``, which is broadcast to that shape), the initial
    state ``uniform(-0.05, 0.05, (n, 4))``, the actions ``uniform(-1, 1, (n, traj_len))`` for ``'random'`` (none
    for ``'ones'``: every action is 1).  The rollout then runs on ``device`` in double --
    ``rollout('cartpole', ..., dtype=torch.float64)`` on the draws as they are -- and is rounded once.

    With ``policy`` an ``MLPPolicy`` (4 inputs) the episodes run closed loop, as ``rollout(policy=, replace=)``
    states it, and the returned actions are the ones taken.  After theta and the initial state the draws are, in
    this order and each only if it is used: ``replace = uniform(size=(n, traj_len)) < frac_rnd`` (only if
    ``frac_rnd > 0``), ``uniform(-1, 1, (n, traj_len))`` (only if ``frac_rnd > 0``: the actions where replaced)
    and ``standard_normal((n, traj_len))`` (only if ``noise_std > 0``: times ``noise_std``, the exploration term
    elsewhere).  ``frac_rnd = noise_std = 0`` is the policy alone (the reference's policy_rl), ``frac_rnd > 0``
    its policy_rl_randomized.  Both must be 0 with ``'random'`` / ``'ones'``, whose draws are unchanged."""
    rs = np.random.RandomState(seed) if seed is not None else np.random
    lows, highs = np.asarray(lows, dtype=np.float64), np.asarray(highs, dtype=np.float64)
    if lows.shape != highs.shape or lows.shape not in ((2,), (3,)):
        raise ValueError('lows and highs must both hold 2 or 3 bounds, got %r and %r'
                         % (tuple(lows.shape), tuple(highs.shape)))
    k = lows.shape[0]
    if params is None:
        theta = rs.uniform(lows, highs, size=(n, k))
    else:
        theta = np.broadcast_to(np.asarray(params, dtype=np.float64), (n, k)).copy()
    init = rs.uniform(-0.05, 0.05, size=(n, 4))
    closed, replace = isinstance(policy, MLPPolicy), None
    if not 0.0 <= frac_rnd <= 1.0 or not noise_std >= 0.0:
        raise ValueError('frac_rnd must lie in [0, 1] and noise_std be >= 0, got %r and %r' % (frac_rnd, noise_std))
    if not closed and (frac_rnd or noise_std) and policy in ('random', 'policy_random', 'ones', 'policy_ones'):
        raise ValueError('frac_rnd and noise_std belong to an MLPPolicy, not to policy=%r' % (policy,))
    if closed:
        if frac_rnd > 0:
            replace = rs.uniform(size=(n, traj_len)) < frac_rnd
            instead = rs.uniform(-1.0, 1.0, size=(n, traj_len))
        acts = noise_std * rs.standard_normal((n, traj_len)) if noise_std > 0 else np.zeros((n, traj_len))
        if frac_rnd > 0:
            acts = np.where(replace, instead, acts)
    elif policy in ('random', 'policy_random'):
        acts = rs.uniform(-1.0, 1.0, size=(n, traj_len))
    elif policy in ('ones', 'policy_ones'):
        acts = np.ones((n, traj_len))
    else:
        raise ValueError('unknown collection policy %r' % (policy,))
    full = theta if k == 3 else np.column_stack([theta, np.full(n, float(cart_mass))])
    to = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(device)      # noqa: E731
    states, actions, lengths = rollout('cartpole', to(full), to(init), to(acts[:, :, None]), n_steps=traj_len,
                                       terminate=terminate, dtype=torch.float64,
                                       policy=policy if closed else None,
                                       replace=None if replace is None else to(replace))
    out = (to(theta).float(), states.float(), actions.float())
    return out + (lengths,) if terminate else out


# ---------------------------------------------------------------- draws on the device (include/bsig_sim_draws.h)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_TWO_PI = 6.283185307179586
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(counters, key):
    """Philox4x32-10 (Salmon et al., SC 2011) in numpy: ``counters`` ``[..., 4]`` and ``key = (k0, k1)`` (integers
    below 2^32, the key's words scalars or arrays that broadcast against ``[...]``) -> uint32 ``[..., 4]``.  Ten
    rounds of ``c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))``, the key bumped by
    (0x9E3779B9, 0xBB67AE85) after each."""
    c = np.asarray(counters)
    if c.ndim < 1 or c.shape[-1] != 4 or c.dtype.kind not in 'iu':
        raise ValueError('counters must be an integer array [..., 4], got %s %r' % (c.dtype, c.shape))
    c = c.astype(np.uint64)
    if (c > _MASK32).any():
        raise ValueError('counters must be below 2^32')
    if len(key) != 2:
        raise ValueError('key must be (k0, k1), got %r' % (key,))
    k0, k1 = (np.asarray(k).astype(np.uint64) & _MASK32 for k in key)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    shift = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2              # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> shift) ^ c1 ^ k0, p1 & _MASK32, (p0 >> shift) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _MASK32, (k1 + np.uint64(PHILOX_W1)) & _MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


class EpisodeDraws:
    """What the draws of include/bsig_sim_draws.h are made from: ``seed`` and ``first_episode`` (integers in
    0..2^64 - 1; episode n of a call is the global episode ``first_episode + n``), theta's bounds ``lows`` /
    ``highs`` (pd entries; ``low == high`` is a constant), the initial internal state's ``init_lows`` /
    ``init_highs`` (id entries), the replacement action's ``act_low`` / ``act_high``, the share ``frac_rnd`` of
    the steps that take it instead of the policy's action, and the standard deviation ``noise_std`` of the
    Gaussian exploration term of the others.  A pair of bounds may be left ``None`` when ``rollout_drawn`` is given
    that array.  Everything is checked here, before any GPU call; a ValueError names its argument."""

    def __init__(self, seed, first_episode=0, lows=None, highs=None, init_lows=None, init_highs=None,
                 act_low=-1.0, act_high=1.0, frac_rnd=0.0, noise_std=0.0):
        self.seed = self._word64('seed', seed)
        self.first_episode = self._word64('first_episode', first_episode)
        self.lows, self.highs = self._bounds('lows', 'highs', lows, highs, 3)
        self.init_lows, self.init_highs = self._bounds('init_lows', 'init_highs', init_lows, init_highs, 4)
        (self.act_low,), (self.act_high,) = self._bounds('act_low', 'act_high', [act_low], [act_high], 1)
        self.frac_rnd, self.noise_std = self._real('frac_rnd', frac_rnd), self._real('noise_std', noise_std)
        if not 0.0 <= self.frac_rnd <= 1.0:
            raise ValueError('frac_rnd must lie in [0, 1], got %r' % (frac_rnd,))
        if not (np.isfinite(self.noise_std) and self.noise_std >= 0.0):
            raise ValueError('noise_std must be finite and >= 0, got %r' % (noise_std,))

    @staticmethod
    def _word64(name, value):
        try:
            word = None if isinstance(value, (bool, np.bool_)) else operator.index(value)
        except TypeError:
            word = None
        if word is None or not 0 <= word < 2 ** 64:
            raise ValueError('%s must be an int in 0..2^64 - 1, got %r' % (name, value))
        return word

    @staticmethod
    def _real(name, value):
        try:
            return float(value)
        except (TypeError, ValueError):
            raise ValueError('%s must be a number, got %r' % (name, value)) from None

    @staticmethod
    def _bounds(lo_name, hi_name, lo, hi, most):
        if lo is None and hi is None:
            return None, None
        if lo is None or hi is None:
            raise ValueError('%s and %s come together, got %r and %r' % (lo_name, hi_name, lo, hi))
        try:
            lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('%s and %s must be numbers, got %r and %r' % (lo_name, hi_name, lo, hi)) from None
        if lo.ndim != 1 or lo.shape != hi.shape or not 1 <= lo.shape[0] <= most:
            raise ValueError('%s and %s must both hold 1..%d bounds, got %r and %r'
                             % (lo_name, hi_name, most, tuple(lo.shape), tuple(hi.shape)))
        if not np.isfinite(lo).all():
            raise ValueError('%s must be finite, got %r' % (lo_name, lo.tolist()))
        if not np.isfinite(hi).all():
            raise ValueError('%s must be finite, got %r' % (hi_name, hi.tolist()))
        if (lo > hi).any():
            raise ValueError('%s must not exceed %s, got %r and %r' % (lo_name, hi_name, lo.tolist(), hi.tolist()))
        return lo, hi

    @property
    def thresh(self):
        """``floor(frac_rnd * 2^32)``, in 0..2^32: step t is marked where ``x0 < thresh``."""
        return int(np.floor(self.frac_rnd * 4294967296.0))

    def key(self):
        return self.seed & 0xFFFFFFFF, self.seed >> 32

    def for_task(self, task, need_theta=True, need_init=True):
        """ValueError unless the bounds that will be used hold ``task``'s pd and id entries."""
        pd, idim, _ = SIM_DIMS[task]
        for names, lo, width, need in ((('lows', 'highs', 'params'), self.lows, pd, need_theta),
                                       (('init_lows', 'init_highs', 'init'), self.init_lows, idim, need_init)):
            if need and lo is None:
                raise ValueError('%s and %s are needed where no %s is given' % names)
            names = names[:2]
            if need and lo.shape[0] != width:
                raise ValueError('%s and %s must hold %d bounds for %s, got %d' % (names + (width, task, lo.shape[0])))
        return self


def _np_dtype(dtype):
    if dtype is None or dtype in (torch.float32, np.float32):
        return np.float32
    if dtype in (torch.float64, np.float64):
        return np.float64
    raise ValueError('the draws are stored as float32 or float64, got dtype=%r' % (dtype,))


def _philox_words(draws, n, t, purpose):
    """The words of global episodes first_episode .. + n - 1 at the steps ``t`` ([T] or a scalar): [n, (T,) 4]."""
    g = np.uint64(draws.first_episode) + np.arange(n, dtype=np.uint64)          # (mod 2^64)
    t = np.asarray(t, dtype=np.uint64)
    shape = (n,) + t.shape
    counters = np.empty(shape + (4,), dtype=np.uint64)
    lead = (slice(None),) + (None,) * t.ndim
    counters[..., 0] = (g & _MASK32)[lead]
    counters[..., 1] = (g >> np.uint64(32))[lead]
    counters[..., 2] = t
    counters[..., 3] = purpose
    return philox4x32(counters, draws.key())


def episode_draws(task, draws, n, n_steps, policy_on=False, dtype=np.float64):
    """The definition of include/bsig_sim_draws.h in numpy: the draws of episodes ``draws.first_episode`` ..
    ``+ n - 1`` -> ``(theta [n, pd], init [n, id], explore [n, T], replace [n, T] uint8)``, every real formed in
    double by the header's operations and rounded once to ``dtype`` (float32 or float64).  ``theta`` / ``init`` is
    ``None`` where ``draws`` holds no bounds for it.  ``explore`` is ``e_t = r_t ? v_t : noise_std z_t`` and
    ``replace`` ``r_t`` with ``policy_on``; without it every step counts as marked: ``v_t`` and 1.  The ends of
    episodes are not known here: every step is drawn."""
    if task not in SIM_DIMS:
        raise ValueError("task must be 'pendulum' or 'cartpole', got %r" % (task,))
    if not isinstance(draws, EpisodeDraws):
        raise ValueError('draws must be an EpisodeDraws, got %r' % (type(draws).__name__,))
    draws.for_task(task, draws.lows is not None, draws.init_lows is not None)
    pd, idim, _ = SIM_DIMS[task]
    store = _np_dtype(dtype)
    unit = lambda x: x.astype(np.float64) * 2.0 ** -32      # noqa: E731  (exact)
    theta = init = None
    if draws.lows is not None:
        x = unit(_philox_words(draws, n, 0, _lib.SIM_DRAW_THETA)[:, :pd])
        theta = (draws.lows + ((draws.highs - draws.lows) * x)).astype(store)
    if draws.init_lows is not None:
        x = unit(_philox_words(draws, n, 0, _lib.SIM_DRAW_INIT)[:, :idim])
        init = (draws.init_lows + ((draws.init_highs - draws.init_lows) * x)).astype(store)
    w = _philox_words(draws, n, np.arange(n_steps), _lib.SIM_DRAW_STEP)
    v = draws.act_low + ((draws.act_high - draws.act_low) * unit(w[..., 1]))
    if not policy_on:
        return theta, init, v.astype(store), np.ones((n, n_steps), dtype=np.uint8)
    replace = w[..., 0].astype(np.uint64) < np.uint64(draws.thresh)
    if draws.noise_std != 0.0:
        u1, u2 = (w[..., 2].astype(np.float64) + 1.0) * 2.0 ** -32, unit(w[..., 3])
        z = np.sqrt(-2.0 * np.log(u1)) * np.cos(_TWO_PI * u2)
        e = np.where(replace, v, draws.noise_std * z)
    else:
        e = np.where(replace, v, 0.0)
    return theta, init, e.astype(store), replace.astype(np.uint8)


def rollout_drawn(task, n, n_steps, draws, policy=None, params=None, init=None, terminate=False, dtype=None,
                  device='cpu', nonfinite=None, record=False):
    """``n`` episodes of ``task`` over ``n_steps`` steps with every number drawn by the counter-based generator of
    include/bsig_sim_draws.h from ``draws`` (an ``EpisodeDraws``): episode i is the global episode
    ``draws.first_episode + i`` of ``draws.seed``, the same bits whatever ``n``, the launch or the device's
    neighbours.  -> ``(theta [n, pd], init [n, id], states [n, T + 1, sd], actions_out [n, T + 1, 1],
    lengths [n] int32)``, and with ``record`` also ``explore [n, T]`` and ``replace [n, T]`` uint8.

    ``policy=None``: every action is the uniform draw ``v_t`` in ``[act_low, act_high)``.  With an ``MLPPolicy``
    the action is ``v_t`` where the step is marked (a share ``frac_rnd``) and ``pi(o_t) + noise_std z_t``
    elsewhere: the rule of ``rollout(policy=, replace=)``.  ``params`` / ``init`` (tensors ``[n, pd]`` / ``[n, id]``
    on ``device``) are used as given instead of a draw.  Ends, fills, ``lengths``, ``dtype`` and ``nonfinite`` are
    ``rollout``'s; every draw is rounded once to ``dtype`` before it is used, so ``rollout`` fed the returned
    ``theta``, ``init``, ``explore`` and ``replace`` gives the same states bit for bit.  An ended episode draws
    nothing more: its ``explore`` and ``replace`` from step ``lengths - 1`` on are 0.

    On a CUDA ``device`` this is ONE launch of the HIP kernel, which reads no ``[n, T]`` array at all; on the CPU
    it is ``episode_draws`` followed by the numpy rollout, and never touches a GPU.  The two differ by their
    libraries' sine, cosine, tanh, logarithm alone.  ValueError, before any GPU call, for what does not fit."""
    if task not in SIM_DIMS:
        raise ValueError("task must be 'pendulum' or 'cartpole', got %r" % (task,))
    pd, idim, sd = SIM_DIMS[task]
    if dtype is None or dtype == torch.float32:
        prec = _lib.F32
    elif dtype == torch.float64:
        prec = _lib.F64
    else:
        raise ValueError('rollout_drawn stores torch.float32 or torch.float64, got dtype=%r' % (dtype,))
    counts = []
    for name, value, top in (('n', n, 2 ** 62), ('n_steps', n_steps, 2 ** 28)):
        try:
            count = None if isinstance(value, (bool, np.bool_)) else operator.index(value)
        except TypeError:
            count = None
        if count is None or not (name == 'n' or count >= 1) or not 0 <= count < top:
            raise ValueError('%s must be an int >= %d, got %r' % (name, name != 'n', value))
        counts.append(count)
    n, n_steps = counts
    if not isinstance(draws, EpisodeDraws):
        raise ValueError('draws must be an EpisodeDraws, got %r' % (type(draws).__name__,))
    if not isinstance(terminate, (bool, np.bool_)):
        raise ValueError('terminate must be a bool, got %r' % (terminate,))
    if policy is not None:
        if not isinstance(policy, MLPPolicy):
            raise ValueError('policy must be an MLPPolicy, got %r' % (type(policy).__name__,))
        if policy.in_dim != sd:
            raise ValueError('policy takes %d inputs, %s observes %d' % (policy.in_dim, task, sd))
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None and torch.cuda.is_available():
        dev = torch.device('cuda', torch.cuda.current_device())
    given = {}
    for name, t, width in (('params', params, pd), ('init', init, idim)):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.dtype.is_floating_point or tuple(t.shape) != (n, width):
            raise ValueError('%s must be a floating-point tensor [%d, %d] for %s' % (name, n, width, task))
        if t.device != dev:
            raise ValueError('%s must live on %s, got %s' % (name, dev, t.device))
        given[name] = t.detach().to(prec.dtype).contiguous()
    draws.for_task(task, 'params' not in given, 'init' not in given)
    if nonfinite is not None and not (torch.is_tensor(nonfinite) and nonfinite.dtype == torch.int32
                                      and nonfinite.numel() == 1 and nonfinite.device == dev):
        raise ValueError('nonfinite must be a 1-element int32 tensor on %s' % (dev,))
    if dev.type != 'cuda':
        theta, s0, explore, replace = episode_draws(task, draws, n, n_steps, policy is not None, prec.np_dtype)
        theta = given['params'].numpy() if 'params' in given else theta
        s0 = given['init'].numpy() if 'init' in given else s0
        states, acts, lengths = _host_rollout(task, theta.astype(np.float64), s0.astype(np.float64),
                                              explore.astype(np.float64)[:, :, None], n_steps, bool(terminate),
                                              policy, replace if policy is not None else None)
        if nonfinite is not None and not np.isfinite(states).all():
            nonfinite.fill_(1)
        over = np.arange(n_steps)[None, :] >= lengths[:, None] - 1          # an ended episode draws nothing more
        explore, replace = np.where(over, 0, explore).astype(explore.dtype), np.where(over, 0, replace).astype(np.uint8)
        out = (torch.from_numpy(np.ascontiguousarray(theta)), torch.from_numpy(np.ascontiguousarray(s0)),
               torch.from_numpy(states).to(prec.dtype), torch.from_numpy(acts).to(prec.dtype),
               torch.from_numpy(lengths))
        return out + (torch.from_numpy(explore), torch.from_numpy(replace)) if record else out
    _lib.require_gpu()
    as_doubles = lambda b: None if b is None else (_lib.f64 * len(b))(*b.tolist())      # noqa: E731
    bounds = [as_doubles(b) for b in (draws.lows, draws.highs, draws.init_lows, draws.init_highs)]
    hidden = (policy.hidden if policy is not None else ()) + (0, 0)
    with _lib.device_stream(dev) as stream:
        theta = torch.empty((n, pd), dtype=prec.dtype, device=dev)
        s0 = torch.empty((n, idim), dtype=prec.dtype, device=dev)
        states = torch.empty((n, n_steps + 1, sd), dtype=prec.dtype, device=dev)
        acts = torch.empty((n, n_steps + 1, 1), dtype=prec.dtype, device=dev)
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
        explore = torch.empty((n, n_steps), dtype=prec.dtype, device=dev) if record else None
        replace = torch.empty((n, n_steps), dtype=torch.uint8, device=dev) if record else None
        prec.sim_rollout_drawn(_lib.SIM_TASKS[task], _lib.ptr(given.get('params')), _lib.ptr(given.get('init')),
                               bounds[0], bounds[1], bounds[2], bounds[3], draws.act_low, draws.act_high,
                               draws.frac_rnd, draws.noise_std, draws.seed, draws.first_episode,
                               None if policy is None else _lib.ptr(policy.packed_on(dev)),
                               len(hidden) - 2, hidden[0], hidden[1],
                               _lib.SIM_ACTIVATIONS[policy.activation] if policy is not None else 0,
                               _lib.ptr(theta), _lib.ptr(s0), _lib.ptr(states), _lib.ptr(acts), _lib.ptr(lengths),
                               _lib.ptr(explore), _lib.ptr(replace), n, n_steps, int(bool(terminate)),
                               _lib.ptr(nonfinite), stream)
    out = (theta, s0, states, acts, lengths)
    return out + (explore, replace) if record else out


_DRAW_PAIRS = {     # task -> theta's default bounds, the initial state's bounds, the actions' (pendulum_pairs, cartpole_pairs)
    'pendulum': ((0.01, 0.01), (2.0, 2.0), (-np.pi, -1.0), (np.pi, 1.0), 0.0, 1.0),
    'cartpole': ((0.1, 0.1), (2.0, 2.0), (-0.05,) * 4, (0.05,) * 4, -1.0, 1.0),
}


def draw_pairs(task, n, traj_len, seed, policy='random', lows=None, highs=None, cart_mass=1.0, frac_rnd=0.0,
               noise_std=0.0, terminate=False, first_episode=0, device='cpu'):
    """``n`` episodes of ``task`` with ``traj_len`` actions in the contract of ``pendulum_pairs`` and
    ``cartpole_pairs`` -- fp32 ``(theta, states [n, traj_len + 1, sd], actions [n, traj_len + 1, 1])`` on
    ``device``, and ``lengths`` [n] int32 with ``terminate=True`` -- with every number drawn by
    ``rollout_drawn``: on a CUDA device one launch and no host draw or copy at all.  Episode i is the global
    episode ``first_episode + i`` of ``seed``, so shards, ranks and later rounds make disjoint or identical
    episodes by their indices alone.

    The defaults follow those functions.  Pendulum: theta = (length, mass) ~ U[0.01, 2)^2, th ~ U[-pi, pi),
    thdot ~ U[-1, 1), actions ~ U[0, 1).  CartPole: theta = (pole mass, pole half-length) ~ U[0.1, 2)^2 with the
    cart's mass the constant ``cart_mass`` (or three bounds: drawn as well, theta [n, 3]), the initial state
    ~ U[-0.05, 0.05)^4, actions ~ U[-1, 1).  ``policy='random'`` draws every action; an ``MLPPolicy`` runs closed
    loop with ``frac_rnd`` and ``noise_std`` as in ``cartpole_pairs``, and the returned actions are the ones
    taken.  The launch is the fp32 one: the returned theta is exactly what each episode ran with.  These are not
    the ``RandomState`` draws of ``pendulum_pairs`` / ``cartpole_pairs``, which are unchanged."""
    if task not in _DRAW_PAIRS:
        raise ValueError("task must be 'pendulum' or 'cartpole', got %r" % (task,))
    d_lows, d_highs, init_lows, init_highs, act_low, act_high = _DRAW_PAIRS[task]
    lows = np.asarray(d_lows if lows is None else lows, dtype=np.float64)
    highs = np.asarray(d_highs if highs is None else highs, dtype=np.float64)
    widths = ((2,), (3,)) if task == 'cartpole' else ((2,),)
    if lows.shape != highs.shape or lows.shape not in widths:
        raise ValueError('lows and highs must both hold %s bounds for %s, got %r and %r'
                         % (' or '.join(str(w[0]) for w in widths), task, tuple(lows.shape), tuple(highs.shape)))
    k = lows.shape[0]
    if task == 'cartpole' and k == 2:
        try:
            mass = float(cart_mass)
        except (TypeError, ValueError):
            raise ValueError('cart_mass must be a number, got %r' % (cart_mass,)) from None
        lows, highs = np.append(lows, mass), np.append(highs, mass)
    closed = isinstance(policy, MLPPolicy)
    if not closed:
        if policy not in ('random', 'policy_random'):
            raise ValueError("policy must be 'random' or an MLPPolicy, got %r" % (policy,))
        if frac_rnd or noise_std:
            raise ValueError('frac_rnd and noise_std belong to an MLPPolicy, not to policy=%r' % (policy,))
    draws = EpisodeDraws(seed, first_episode, lows, highs, init_lows, init_highs, act_low, act_high, frac_rnd,
                         noise_std)
    theta, _, states, actions, lengths = rollout_drawn(task, n, traj_len, draws, policy=policy if closed else None,
                                                       terminate=terminate, dtype=torch.float32, device=device)
    out = (theta[:, :k].contiguous(), states, actions)
    return out + (lengths,) if terminate else out
