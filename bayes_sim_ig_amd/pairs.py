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
    for GPU tensors, its numpy restatement in double for CPU tensors.

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


def _host_rollout(task, params, init, actions, n_steps, terminate):
    """The definition of include/bsig_sim.h in numpy, double: (states, actions_out, lengths)."""
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


def rollout(task, params, init, actions, n_steps=None, terminate=False, dtype=None, nonfinite=None):
    """Open-loop rollouts of ``task`` ('pendulum' or 'cartpole'), the definition of include/bsig_sim.h:
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
    ValueError, before any GPU call, for a shape, a device or an argument that does not fit; it names it."""
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
    p, s0, a = (t.detach().to(prec.dtype).contiguous() for t in (params, init, actions))
    if not dev.type == 'cuda':
        states, acts, lengths = _host_rollout(task, p.double().numpy(), s0.double().numpy(), a.double().numpy(),
                                              n_steps, bool(terminate))
        if nonfinite is not None and not np.isfinite(states).all():
            nonfinite.fill_(1)
        return (torch.from_numpy(states).to(prec.dtype), torch.from_numpy(acts).to(prec.dtype),
                torch.from_numpy(lengths))
    _lib.require_gpu()
    with _lib.device_stream(dev) as stream:
        states = torch.empty((n, n_steps + 1, sd), dtype=prec.dtype, device=dev)
        acts = torch.empty((n, n_steps + 1, 1), dtype=prec.dtype, device=dev)
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
        prec.sim_rollout(_lib.SIM_TASKS[task], _lib.ptr(p), _lib.ptr(s0), _lib.ptr(a), _lib.ptr(states),
                         _lib.ptr(acts), _lib.ptr(lengths), n, n_steps, ta, int(bool(terminate)),
                         _lib.ptr(nonfinite), stream)
    return states, acts, lengths


def cartpole_pairs(n, traj_len, policy='random', lows=(0.1, 0.1), highs=(2.0, 2.0), cart_mass=1.0,
                   params=None, seed=None, device='cpu', terminate=False):
    """n CartPole episodes of ``traj_len`` actions in ``pendulum_pairs``' contract: theta [n, 2] = (pole mass,
    pole half-length) with the cart's mass the constant ``cart_mass``, or, with three bounds, theta [n, 3] with
    the cart's mass drawn as well; states [n, traj_len + 1, 4] = (x, xdot, th, thdot); actions
    [n, traj_len + 1, 1] in [-1, 1], the last repeated; fp32 on ``device``.  With ``terminate=True`` also
    ``lengths`` [n] int32, and the episodes end as ``rollout`` states it.

    Every draw is made on the host from ``RandomState(seed)``, in this order: theta
    ``uniform(lows, highs, (n, 2 or 3))`` (none with ``params=``, which is broadcast to that shape), the initial
    state ``uniform(-0.05, 0.05, (n, 4))``, the actions ``uniform(-1, 1, (n, traj_len))`` for ``'random'`` (none
    for ``'ones'``: every action is 1).  The rollout then runs on ``device`` in double --
    ``rollout('cartpole', ..., dtype=torch.float64)`` on the draws as they are -- and is rounded once."""
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
    if policy in ('random', 'policy_random'):
        acts = rs.uniform(-1.0, 1.0, size=(n, traj_len))
    elif policy in ('ones', 'policy_ones'):
        acts = np.ones((n, traj_len))
    else:
        raise ValueError('unknown collection policy %r' % (policy,))
    full = theta if k == 3 else np.column_stack([theta, np.full(n, float(cart_mass))])
    to = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(device)      # noqa: E731
    states, actions, lengths = rollout('cartpole', to(full), to(init), to(acts[:, :, None]), n_steps=traj_len,
                                       terminate=terminate, dtype=torch.float64)
    out = (to(theta).float(), states.float(), actions.float())
    return out + (lengths,) if terminate else out
