"""What the rollout tests (tests/test_sim_host.py, tests/test_gpu_sim.py) share: the two tasks' steps restated
in numpy, in double, from the definition of include/bsig_sim.h (not from bayes_sim_ig_amd/pairs.py); seeded
draws of fp32-representable values; the case tables; and the bound of the step-by-step check.

The step-by-step check.  A launch's double outputs are taken as they are: for every episode and every t with
t + 1 below its length, the numpy step below is applied to the kernel's OWN state t and compared with its state
t + 1.  Whole trajectories are never compared: for a small l the Pendulum map amplifies an ulp by up to
1 + 3 g dt^2 / (2 l) a step, and a step-by-step check cannot hide behind that.

The bound of ``step_bounds``.  u = U64 is the unit roundoff of double, gamma(k) = k u / (1 - k u) (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1).  The kernel and numpy run the SAME sequence
of correctly rounded double operations on the same operands (the header states every operation; nothing is
contracted), so where no sine or cosine enters, the two agree BITWISE and are compared so.  They differ by their
libraries' sine and cosine: each is allowed sigma = 8 u in absolute value, the project's own allowance
(tests/kme_cases.py SINCOS[8]); two values that each carry it differ by ds = 2 sigma.  A formula evaluated in k
operations from operands that differ by d on the two sides gives results that differ by the formula's first-order
change (the second-order products are carried too) plus gamma(k) of its absolute form on EACH side: 2 gamma(k).
Every magnitude is evaluated from the numpy reference, per element; no constant was fitted to what a kernel gave.

CartPole (the state is observed, so both sides start from the same bits).  With mt = m_p + m_c, mpl = m_p l,
q = mpl thdot^2:
  tmp = (F + q s) / mt              8 operations:  tmp_abs = (|F| + |q s|) / mt,
                                    d_tmp = |q| ds / mt + 2 gamma(8) tmp_abs;
  num = g s - c tmp                 2 more:        num_abs = g |s| + |c| tmp_abs,
                                    d_num = g ds + (tmp_abs + d_tmp) ds + |c| d_tmp + 2 gamma(10) num_abs;
  den = l (4/3 - m_p c^2 / mt)      6 operations:  den_abs = l (4/3 + m_p c^2 / mt); den >= l / 3 > 0,
                                    d_den = l m_p (2 |c| ds + ds^2) / mt + 2 gamma(6) den_abs;
  tha = num / den                   d_tha = (d_num + |tha| d_den) / (|den| - d_den) + 2 gamma(1) |tha|;
  xa  = tmp - (mpl tha c) / mt      5 operations on top of tmp and tha:
                                    d_xa = d_tmp + mpl (|c| d_tha + (|tha| + d_tha) ds) / mt
                                           + 2 gamma(5) (tmp_abs + mpl |tha c| / mt);
  x' = x + dt xdot, th' = th + dt thdot:   no sine: compared bitwise (bound 0);
  xdot'  = xdot + dt xa:            d = dt d_xa  + 2 gamma(2) (|xdot| + dt |xa|);
  thdot' = thdot + dt tha:          d = dt d_tha + 2 gamma(2) (|thdot| + dt |tha|).

Pendulum (the angle is NOT observed).  From the observed (c^, s^, thdot) of state t the check forms
th_r = atan2(s^, c^) in (-pi, pi]; the kernel's own angle theta is th_r + 2 pi k + e with
  |e| <= E = (|c^| + |s^|) sigma / (1 - 4 sigma) + gamma(2) pi
(c^ and s^ are within sigma of cos theta, sin theta; numpy's atan2 is taken as 1 ulp).  |theta| itself is bounded
by Theta_t = |th_0| + sum_(k<t) |w_k| dt, evaluated from the reference's w (times 1 + 1e-6 for the difference
between the two sides' w, which the bound below keeps many orders smaller).  With k_s = -3 g / (2 l) and
k_u = 3 / (m l^2), which both sides form by the same operations (they agree bitwise):
  A = theta + pi: the kernel rounds at |theta| <= Theta_t, numpy at |th_r| <= pi:
                                    d_A = E + u (Theta_t + pi) + u 2 pi;
  S = sin A                         d_S = d_A + 2 sigma;
  w = thdot + (k_s S + k_u u_t) dt  5 operations:  w_abs = |thdot| + (|k_s S| + |k_u u_t|) dt,
                                    d_w = |k_s| dt d_S + 2 gamma(5) w_abs   -- it scales with 3 g / (2 l); k_u
                                    enters w_abs;
  thdot' = clip(w, -8, 8)           d = d_w (a clip does not spread two values);
  th' = theta + w dt (mod 2 pi)     d_th = E + dt d_w + gamma(2) (Theta_t + |w| dt) + gamma(2) (pi + |w| dt);
  cos th', sin th'                  d = d_th + 2 sigma.
Only cos, sin of th' and thdot' are compared.
"""
import numpy as np

U64 = 2.0 ** -53
SINCOS = 8 * U64                       # the allowance for a double sine or cosine (tests/kme_cases.py SINCOS[8])
EPISODES, STEP_BLOCK, GRID_CAP = 64, 8, 2048      # BSIG_SIM_EPISODES, _STEP_BLOCK, _GRID_CAP
TASK_IDS = {'pendulum': 0, 'cartpole': 1}
DIMS = {'pendulum': (2, 2, 3), 'cartpole': (3, 4, 4)}      # pd, id, sd
X_LIMIT = 2.4
TH_LIMIT = 12 * 2 * np.pi / 360

W, B = EPISODES, STEP_BLOCK
# the episode counts around a workgroup's W, and the step counts around the step block B (T + 1 states are
# walked in blocks of B, so T = B - 1 is one full block, T = B one more state, 2 B + 1 two blocks and two)
COUNTS = (1, W - 1, W, W + 1, 3 * W + 2)
STEPS = (1, 2, B - 1, B, B + 1, 2 * B + 1, 20, 200)


def ta_of(steps):
    """The action counts of a case: one action, T, T + 1 (padded), T + 4 (more than are used)."""
    return (1, steps, steps + 1, steps + 4)


def gamma(k, u=U64):
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def draws(task, n, ta, seed=0, corner=False, wide=False):
    """params [n, pd], init [n, id], actions [n, ta, 1] as float32 arrays (so both entry points take them
    exactly): parameters uniform in [0.1, 2] (``corner``: Pendulum's l = m = 0.01, the prior's corner), the
    initial state as the task's own collection draws it -- Pendulum th in [-pi, pi], thdot in [-1, 1]; CartPole
    in [-0.05, 0.05]^4, or ``wide``: x in [-2.3, 2.3], xdot in [-2, 2], th in [-0.2, 0.2], thdot in [-2, 2], so
    that episodes end at every step -- and actions in [-1, 1]."""
    rs = np.random.RandomState(seed)
    pd, idim, _ = DIMS[task]
    params = rs.uniform(0.1, 2.0, size=(n, pd))
    if corner:
        params[:] = 0.01
    if task == 'pendulum':
        init = np.column_stack([rs.uniform(-np.pi, np.pi, n), rs.uniform(-1.0, 1.0, n)])
    elif wide:
        init = rs.uniform(-1.0, 1.0, size=(n, 4)) * np.array([2.3, 2.0, 0.2, 2.0])
    else:
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
    actions = rs.uniform(-1.0, 1.0, size=(n, ta, 1))
    return params.astype(np.float32), init.astype(np.float32), actions.astype(np.float32)


def _clip(v, lo, hi):
    return np.clip(v, lo, hi)


def pendulum_parts(params, th, thdot, act):
    """One Pendulum step from the angle: everything the bound reads."""
    l, m = params[..., 0], params[..., 1]
    g, dt = 10.0, 0.05
    u = _clip(2.0 * act, -2.0, 2.0)
    k_s = -3 * g / (2 * l)
    k_u = 3.0 / (m * (l * l))
    sin_a = np.sin(th + np.pi)
    w = thdot + (k_s * sin_a + k_u * u) * dt
    th1 = th + w * dt
    return dict(u=u, k_s=k_s, k_u=k_u, sin_a=sin_a, w=w, th1=th1, thdot1=_clip(w, -8.0, 8.0), dt=dt)


def cartpole_parts(params, state, act):
    """One CartPole step from the state [..., 4]: everything the bound reads."""
    mp, l, mt = params[..., 0], params[..., 1], params[..., 0] + params[..., 2]
    x, xdot, th, thdot = (state[..., i] for i in range(4))
    g, dt = 9.8, 0.02
    force = 10.0 * _clip(act, -1.0, 1.0)
    s, c = np.sin(th), np.cos(th)
    mpl = mp * l
    q = mpl * (thdot * thdot)
    tmp = (force + q * s) / mt
    den = l * (4.0 / 3.0 - (mp * (c * c)) / mt)
    tha = (g * s - c * tmp) / den
    xa = tmp - ((mpl * tha) * c) / mt
    new = np.stack([x + dt * xdot, xdot + dt * xa, th + dt * thdot, thdot + dt * tha], axis=-1)
    return dict(mp=mp, l=l, mt=mt, mpl=mpl, force=force, s=s, c=c, q=q, tmp=tmp, den=den, tha=tha, xa=xa,
                new=new, g=g, dt=dt, xdot=xdot, thdot=thdot)


def ended(states):
    """CartPole's end condition on observations [..., 4]."""
    return (np.abs(states[..., 0]) > X_LIMIT) | (np.abs(states[..., 2]) > TH_LIMIT)


def lengths_by_scan(task, states, terminate=True):
    """The valid states of every episode by a direct scan of states [n, T + 1, sd] by the end condition."""
    n, ts = states.shape[:2]
    if task == 'pendulum' or not terminate:
        return np.full(n, ts, dtype=np.int32)
    done = ended(states[:, 1:])
    return np.where(done.any(axis=1), done.argmax(axis=1) + 2, ts).astype(np.int32)


def filled(states, actions_all, lengths):
    """The fill rule applied to untruncated states [n, T + 1, sd] and per-state actions [n, T + 1, 1]."""
    n, ts = states.shape[:2]
    rows, t = np.arange(n)[:, None], np.arange(ts)[None, :]
    lens = np.asarray(lengths, dtype=np.int64)[:, None]
    return states[rows, np.minimum(t, lens - 1)], actions_all[rows, np.minimum(t, lens - 2)]


def step_actions(actions, steps):
    """actions [n, Ta, 1] -> the action of every state index 0..T, [n, T + 1, 1]: step t takes
    actions[min(t, Ta - 1)], state T repeats step T - 1."""
    t = np.minimum(np.minimum(np.arange(steps + 1), steps - 1), actions.shape[1] - 1)
    return actions[:, t]


def step_check(task, params, init, actions, states, lengths):
    """The step-by-step check of the module's docstring on a launch's double ``states`` [n, T + 1, sd]: the worst
    |kernel - numpy| / bound over the elements with a positive bound (a dict by component), after asserting
    bitwise equality where the bound is 0."""
    params, init = params.astype(np.float64), init.astype(np.float64)
    n, ts, _ = states.shape
    steps = ts - 1
    act = step_actions(actions.astype(np.float64), steps)[:, :steps, 0]            # [n, T]
    valid = (np.arange(steps)[None, :] + 1) < np.asarray(lengths)[:, None]          # state t + 1 is a valid one
    cur, nxt = states[:, :-1], states[:, 1:]
    p = params[:, None, :]
    ds = 2.0 * SINCOS
    with np.errstate(all='ignore'):
        if task == 'cartpole':
            r = cartpole_parts(p, cur, act)
            mt, mpl, l, mp = r['mt'], r['mpl'], r['l'], r['mp']
            s, c, dt, g = r['s'], r['c'], r['dt'], r['g']
            tmp_abs = (np.abs(r['force']) + np.abs(r['q'] * s)) / mt
            d_tmp = np.abs(r['q']) * ds / mt + 2 * gamma(8) * tmp_abs
            num_abs = g * np.abs(s) + np.abs(c) * tmp_abs
            d_num = g * ds + (tmp_abs + d_tmp) * ds + np.abs(c) * d_tmp + 2 * gamma(10) * num_abs
            den_abs = l * (4.0 / 3.0 + mp * c * c / mt)
            d_den = l * mp * (2 * np.abs(c) * ds + ds * ds) / mt + 2 * gamma(6) * den_abs
            tha = np.abs(r['tha'])
            d_tha = (d_num + tha * d_den) / (np.abs(r['den']) - d_den) + 2 * gamma(1) * tha
            d_xa = (d_tmp + mpl * (np.abs(c) * d_tha + (tha + d_tha) * ds) / mt
                    + 2 * gamma(5) * (tmp_abs + mpl * tha * np.abs(c) / mt))
            zero = np.zeros_like(d_xa)
            bound = np.stack([zero, dt * d_xa + 2 * gamma(2) * (np.abs(r['xdot']) + dt * np.abs(r['xa'])),
                              zero, dt * d_tha + 2 * gamma(2) * (np.abs(r['thdot']) + dt * tha)], axis=-1)
            ref, names = r['new'], ('x', 'xdot', 'th', 'thdot')
        else:
            c_hat, s_hat, thdot = cur[..., 0], cur[..., 1], cur[..., 2]
            th_r = np.arctan2(s_hat, c_hat)
            r = pendulum_parts(p, th_r, thdot, act)
            dt, w = r['dt'], np.abs(r['w'])
            e = (np.abs(c_hat) + np.abs(s_hat)) * SINCOS / (1.0 - 4.0 * SINCOS) + gamma(2) * np.pi
            travelled = np.cumsum(w * dt, axis=1) * (1.0 + 1e-6)
            theta = np.abs(init[:, :1]) + np.concatenate([np.zeros((n, 1)), travelled[:, :-1]], axis=1)
            d_a = e + U64 * (theta + np.pi) + U64 * 2 * np.pi
            d_s = d_a + 2 * SINCOS
            w_abs = np.abs(thdot) + (np.abs(r['k_s'] * r['sin_a']) + np.abs(r['k_u'] * r['u'])) * dt
            d_w = np.abs(r['k_s']) * dt * d_s + 2 * gamma(5) * w_abs
            d_th = e + dt * d_w + gamma(2) * (theta + w * dt) + gamma(2) * (np.pi + w * dt)
            bound = np.stack([d_th + 2 * SINCOS, d_th + 2 * SINCOS, d_w], axis=-1)
            ref = np.stack([np.cos(r['th1']), np.sin(r['th1']), r['thdot1']], axis=-1)
            names = ('cos', 'sin', 'thdot')
    worst = {}
    for i, name in enumerate(names):
        got, want, lim = nxt[..., i][valid], ref[..., i][valid], bound[..., i][valid]
        assert np.isfinite(want).all() and np.isfinite(lim).all(), name
        exact = lim == 0
        assert np.array_equal(got[exact], want[exact]), '%s: not bitwise where no sine enters' % name
        rest = ~exact
        worst[name] = float((np.abs(got[rest] - want[rest]) / lim[rest]).max()) if rest.any() else 0.0
    return worst


# ---- the cases of the episode ends (CartPole, terminate).  `wide` initial states at T = 20: 21 states walked in the
# blocks [0..7], [8..15], [16..20].  ENDS_SEED was chosen on the HOST path (tests/test_sim_host.py asserts it) so
# that the 3 W + 2 episodes hold every kind the end-of-episode code can go wrong on:
#   'first'     L = 2: the first state formed is terminal;
#   'mid'       the terminal state lies inside a block (its index j = L - 1 has 0 < j % B < B - 1);
#   'edge'      the terminal state is the last of a block (j % B == B - 1) or the first of one (j % B == 0);
#   'last'      the terminal state is state T itself (L = T + 1, as for an episode that never ends);
#   'never'     no state meets the end condition.
ENDS_STEPS, ENDS_COUNT, ENDS_SEED = 20, 3 * W + 2, 0
END_KINDS = ('first', 'mid', 'edge', 'last', 'never')


def end_kinds(states, lengths):
    """kind -> the number of episodes of that kind (see above), from terminated states and their lengths."""
    ts = states.shape[1]
    j = np.asarray(lengths, dtype=np.int64) - 1
    at_end = ended(states[np.arange(states.shape[0]), j])
    stopped = at_end & (j < ts - 1)
    return {'first': int((stopped & (j == 1)).sum()),
            'mid': int((stopped & (j % B > 0) & (j % B < B - 1)).sum()),
            'edge': int((stopped & ((j % B == 0) | (j % B == B - 1))).sum()),
            'last': int((at_end & (j == ts - 1)).sum()),
            'never': int((~at_end).sum())}
