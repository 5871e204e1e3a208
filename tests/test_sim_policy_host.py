"""CPU-side checks of the closed-loop rollouts (include/bsig_sim_policy.h, bayes_sim_ig_amd/pairs.py):
``MLPPolicy`` against the unit-by-unit restatement of tests/sim_policy_cases.py (bitwise) and against the same
``nn.Sequential`` in torch double (within gamma of the layer sizes), its packing and its state dict, every
ValueError before any launch, the draw order of ``cartpole_pairs`` (the ``'random'`` and ``'ones'`` outputs
unchanged), the host path of ``rollout`` with a policy against the step-by-step definition, the episode ends
under a policy on the host path, the binding's table and the argument checks of the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sim_cases as SC
import sim_policy_cases as PC
from conftest import ROOT
from bayes_sim_ig_amd import _lib, pairs

F32, F64 = torch.float32, torch.float64
FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
TASKS = ('pendulum', 'cartpole')


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _policy(task, hidden, activation='tanh', seed=0, scale=1.0):
    weights, biases = PC.make_policy(task, hidden, seed, scale)
    return pairs.MLPPolicy(weights, biases, activation), weights, biases


# ------------------------------------------------------------------ MLPPolicy
@pytest.mark.parametrize('activation', PC.ACTIVATIONS)
@pytest.mark.parametrize('hidden', PC.HIDDEN, ids=PC.hidden_id)
def test_policy_call_is_the_definition_bitwise(hidden, activation):
    for task in TASKS:
        policy, weights, biases = _policy(task, hidden, activation)
        obs = np.random.RandomState(5).uniform(-2.0, 2.0, size=(3, 11, SC.DIMS[task][2]))
        got = policy(obs)
        assert got.shape == (3, 11) and got.dtype == np.float64
        assert np.array_equal(got, PC.policy_ref(weights, biases, activation, obs))
        assert policy.hidden == tuple(hidden) and policy.in_dim == SC.DIMS[task][2]
        # the packing: W_0 row-major, b_0, W_1, b_1, ...; the library counts the same doubles
        packed = policy.packed()
        want = np.concatenate([x.ravel() for w, b in zip(weights, biases) for x in (w, b)])
        assert packed.dtype == np.float64 and np.array_equal(packed, want)
        widths = tuple(hidden) + (0, 0)
        assert _lib.load().bsig_sim_policy_size(SC.TASK_IDS[task], len(hidden), widths[0], widths[1]) == packed.size
    # a NaN passes the relu, as it passes the clip
    if activation == 'relu' and hidden:
        assert np.isnan(policy(np.full((1, policy.in_dim), np.nan))).all()


@pytest.mark.parametrize('activation', PC.ACTIVATIONS)
@pytest.mark.parametrize('hidden', PC.HIDDEN, ids=PC.hidden_id)
def test_policy_call_against_torch_double(hidden, activation):
    """The same nn.Sequential in torch double sums in another order: per layer gamma(2 in) of the absolute form on
    each side, carried through the layers (|act'| <= 1), and a library tanh on each side (PC.TANH)."""
    nn = torch.nn
    act = {'identity': nn.Identity, 'relu': nn.ReLU, 'tanh': nn.Tanh}[activation]
    policy, weights, biases = _policy('cartpole', hidden, activation)
    layers = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        lin = nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
        layers += [lin] + ([act()] if l + 1 < len(weights) else [])
    module = nn.Sequential(*layers)
    obs = np.random.RandomState(6).uniform(-2.0, 2.0, size=(50, 4))
    with torch.no_grad():
        want = module(torch.from_numpy(obs)).numpy()[:, 0]
    x, d = obs, np.zeros_like(obs)
    for l, (w, b) in enumerate(zip(weights, biases)):
        k = w.shape[1]
        d = d @ np.abs(w).T + 2 * SC.gamma(2 * k) * (np.abs(b) + np.abs(x) @ np.abs(w).T)
        x = PC.layer(w, b, x)
        if l + 1 < len(weights):
            x = PC.activate(x, activation)
            d = d + (2 * PC.TANH if activation == 'tanh' else 0.0)
    err = np.abs(policy(obs) - want)
    print('%s %s: worst |numpy - torch| / bound %.3g' % (PC.hidden_id(hidden), activation, (err / d[:, 0]).max()))
    assert (err <= d[:, 0]).all()
    # from_module reads the same policy back; fp32 modules are widened exactly
    back = pairs.MLPPolicy.from_module(module)
    assert back.activation == (activation if hidden else 'identity') and back.hidden == tuple(hidden)
    assert np.array_equal(back.packed(), policy.packed())
    single = pairs.MLPPolicy.from_module(module.float())
    assert np.array_equal(single.packed(), policy.packed())      # (the weights are fp32-representable)


def test_policy_state_dict_device_cache_and_linear_feedback():
    policy, weights, biases = _policy('cartpole', (5, 4), 'relu')
    state = policy.state_dict()
    assert sorted(state) == ['activation', 'biases', 'weights'] and state['activation'] == 'relu'
    other, _, _ = _policy('cartpole', (), 'tanh', seed=1)
    assert other.load_state_dict(state) is other
    assert other.hidden == (5, 4) and other.activation == 'relu' and np.array_equal(other.packed(), policy.packed())
    state['weights'][0][:] = 0                              # a copy: the policy keeps its own
    assert np.array_equal(policy.weights[0], weights[0])
    assert policy.to('cpu') is policy
    packed = policy.packed_on('cpu')
    assert packed is policy.packed_on(torch.device('cpu')) and packed.dtype == F64
    assert np.array_equal(packed.numpy(), policy.packed())
    lin = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS, bias=0.25)
    assert lin.hidden == () and lin.in_dim == 4 and pairs.CARTPOLE_BALANCE_GAINS == (0.2, 0.5, 8.0, 1.5)
    obs = np.array([[1.0, 2.0, 3.0, 4.0]])
    assert lin(obs)[0] == (((0.25 + 0.2 * 1.0) + 0.5 * 2.0) + 8.0 * 3.0) + 1.5 * 4.0


def test_from_module_refuses_what_is_not_the_policy():
    nn = torch.nn
    for module in (nn.Sequential(nn.Linear(4, 3), nn.Tanh(), nn.Linear(3, 3), nn.ReLU(), nn.Linear(3, 1)),
                   nn.Sequential(nn.Linear(4, 3), nn.Sigmoid(), nn.Linear(3, 1)),
                   nn.Sequential(nn.Linear(4, 3), nn.Tanh(), nn.Linear(3, 1), nn.Tanh()),
                   nn.Sequential(nn.Tanh(), nn.Linear(4, 1)),
                   nn.Sequential(nn.Linear(4, 3, bias=False), nn.Tanh(), nn.Linear(3, 1))):
        with pytest.raises(ValueError, match='module'):
            pairs.MLPPolicy.from_module(module)


# ------------------------------------------------------------------ every ValueError
def test_policy_shape_errors_name_the_argument():
    w = lambda out, fan_in: np.zeros((out, fan_in))      # noqa: E731
    b = lambda out: np.zeros(out)                        # noqa: E731
    with pytest.raises(ValueError, match=r'weights\[0\]: the policy has one output, got 2'):
        pairs.MLPPolicy([w(2, 4)], [b(2)])
    with pytest.raises(ValueError, match='hidden layers, more than 2'):
        pairs.MLPPolicy([w(3, 4), w(3, 3), w(3, 3), w(1, 3)], [b(3), b(3), b(3), b(1)])
    with pytest.raises(ValueError, match=r'weights\[0\]: a hidden width of 65 is outside 1..64'):
        pairs.MLPPolicy([w(65, 4), w(1, 65)], [b(65), b(1)])
    with pytest.raises(ValueError, match=r'weights\[1\]: a hidden width of 0 is outside 1..64'):
        pairs.MLPPolicy([w(3, 4), w(0, 3), w(1, 0)], [b(3), b(0), b(1)])
    with pytest.raises(ValueError, match='activation must be one of'):
        pairs.MLPPolicy([w(1, 4)], [b(1)], activation='gelu')
    with pytest.raises(ValueError, match=r'weights\[1\] takes 2 inputs, the layer before has 3'):
        pairs.MLPPolicy([w(3, 4), w(1, 2)], [b(3), b(1)])
    with pytest.raises(ValueError, match=r'biases\[0\]'):
        pairs.MLPPolicy([w(1, 4)], [b(2)])
    with pytest.raises(ValueError, match='one entry per layer'):
        pairs.MLPPolicy([w(1, 4)], [])
    with pytest.raises(ValueError, match='activation must be one of'):
        pairs.MLPPolicy([w(1, 4)], [b(1)]).load_state_dict({'weights': [w(1, 4)], 'biases': [b(1)],
                                                            'activation': 'sigmoid'})


def test_rollout_errors_come_before_any_launch():
    n, ta = 5, 3
    params, init, actions = _t(*SC.draws('cartpole', n, ta))
    good = pairs.linear_feedback((1.0, 1.0, 1.0, 1.0))
    marks = torch.zeros(n, ta, dtype=torch.uint8)

    def call(**kw):
        return pairs.rollout('cartpole', params, init, actions, n_steps=4, **kw)
    with pytest.raises(ValueError, match='policy takes 3 inputs, cartpole observes 4'):
        call(policy=pairs.linear_feedback((1.0, 1.0, 1.0)))
    pend = _t(*SC.draws('pendulum', n, ta))
    with pytest.raises(ValueError, match='policy takes 4 inputs, pendulum observes 3'):
        pairs.rollout('pendulum', *pend, n_steps=4, policy=good)
    with pytest.raises(ValueError, match='policy must be an MLPPolicy'):
        call(policy=torch.nn.Linear(4, 1))
    with pytest.raises(ValueError, match='replace .* needs policy='):
        call(replace=marks)
    for bad in (marks.float(), marks[:, :2], marks[:4], marks[:, :, None], marks.numpy()):
        with pytest.raises(ValueError, match=r'replace must be a uint8 or bool tensor \[5, 3\]'):
            call(policy=good, replace=bad)
    with pytest.raises(ValueError, match='replace must live on cpu'):
        call(policy=good, replace=marks.to('meta'))
    # what fits: uint8 and bool marks are the same call
    a = call(policy=good, replace=marks)
    b = call(policy=good, replace=marks.bool())
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bsig_sim_policy.h')).read()
    define = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1))      # noqa: E731
    assert {k: define('BSIG_SIM_ACT_' + k.upper()) for k in PC.ACTIVATIONS} == _lib.SIM_ACTIVATIONS
    assert (define('BSIG_SIM_POLICY_MAX_HIDDEN'), define('BSIG_SIM_POLICY_MAX_WIDTH'), define('BSIG_SIM_POLICY_UNITS')) \
        == (_lib.SIM_POLICY_MAX_HIDDEN, _lib.SIM_POLICY_MAX_WIDTH, _lib.SIM_POLICY_UNITS) == (2, PC.MAX_WIDTH, PC.UNITS)
    table = _lib.HEADERS['bsig_sim_policy.h']
    assert table['bsig_sim_rollout_policy'] == table['bsig_sim_rollout_policy_f64']
    assert _lib.F32.symbol('sim_rollout_policy') == 'bsig_sim_rollout_policy'
    assert _lib.F64.symbol('sim_rollout_policy') == 'bsig_sim_rollout_policy_f64'
    assert lib.bsig_sim_policy_size(1, 0, 0, 0) == 5 and lib.bsig_sim_policy_size(0, 1, 64, 99) == 3 * 64 + 64 + 65
    for bad in ((2, 0, 0, 0), (1, 3, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 65, 1), (1, 2, 64, 0), (1, 2, 64, 65)):
        assert lib.bsig_sim_policy_size(*bad) < 0, bad
    for fn in (lib.bsig_sim_rollout_policy, lib.bsig_sim_rollout_policy_f64):
        def call(task=1, replace=None, policy=FAKE, nh=2, h0=8, h1=8, act=2, n=3, steps=4, ta=2, terminate=0):
            return fn(task, FAKE, FAKE, FAKE, replace, policy, nh, h0, h1, act, FAKE, FAKE, FAKE, n, steps, ta,
                      terminate, None, None)
        assert call(n=0) == _lib.BSIG_OK
        for kw, word in ((dict(policy=None), 'null policy'), (dict(nh=3), 'n_hidden 3'), (dict(nh=-1), 'n_hidden -1'),
                         (dict(h0=0), 'h0 0'), (dict(h0=65), 'h0 65'), (dict(h1=0), 'h1 0'), (dict(h1=65), 'h1 65'),
                         (dict(act=3), 'unknown activation 3'), (dict(act=-1), 'unknown activation -1'),
                         (dict(task=2), 'unknown task 2'), (dict(steps=0), 'T 0'), (dict(ta=0), 'Ta 0'),
                         (dict(terminate=2), 'terminate 2'), (dict(n=-1), 'bad n')):
            assert call(**kw) == _lib.BSIG_EINVAL, kw
            assert word in lib.bsig_last_error().decode(), (kw, lib.bsig_last_error().decode())


# ------------------------------------------------------------------ the draws of cartpole_pairs
def test_cartpole_pairs_draw_order():
    n, steps, seed = 40, 12, 9
    # 'random' and 'ones': theta, the initial state, the actions -- as before the policies came
    for name in ('random', 'ones'):
        rs = np.random.RandomState(seed)
        theta = rs.uniform(np.array([0.1, 0.1]), np.array([2.0, 2.0]), size=(n, 2))
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
        acts = rs.uniform(-1.0, 1.0, size=(n, steps)) if name == 'random' else np.ones((n, steps))
        full = np.column_stack([theta, np.ones(n)])
        want = pairs.rollout('cartpole', *_t(full, init, acts[:, :, None]), n_steps=steps, terminate=True, dtype=F64)
        got = pairs.cartpole_pairs(n, steps, policy=name, seed=seed, terminate=True)
        assert torch.equal(got[0], torch.from_numpy(theta).float())
        assert torch.equal(got[1], want[0].float()) and torch.equal(got[2], want[1].float())
        assert torch.equal(got[3], want[2]) and len(pairs.cartpole_pairs(n, steps, policy=name, seed=seed)) == 3
        with pytest.raises(ValueError, match='frac_rnd and noise_std belong to an MLPPolicy'):
            pairs.cartpole_pairs(n, steps, policy=name, seed=seed, frac_rnd=0.1)
    with pytest.raises(ValueError, match='unknown collection policy'):
        pairs.cartpole_pairs(n, steps, policy='rl', seed=seed)
    with pytest.raises(ValueError, match='unknown collection policy'):
        pairs.cartpole_pairs(n, steps, policy='rl', seed=seed, frac_rnd=0.5)
    # a policy object: replace, the actions where replaced, the noise -- each drawn only if used
    policy = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
    for frac, std in ((0.0, 0.0), (0.3, 0.0), (0.0, 0.5), (0.3, 0.5)):
        rs = np.random.RandomState(seed)
        theta = rs.uniform(np.array([0.1, 0.1]), np.array([2.0, 2.0]), size=(n, 2))
        init = rs.uniform(-0.05, 0.05, size=(n, 4))
        replace = rs.uniform(size=(n, steps)) < frac if frac > 0 else None
        instead = rs.uniform(-1.0, 1.0, size=(n, steps)) if frac > 0 else None
        e = std * rs.standard_normal((n, steps)) if std > 0 else np.zeros((n, steps))
        if frac > 0:
            e = np.where(replace, instead, e)
        full = np.column_stack([theta, np.ones(n)])
        want = pairs.rollout('cartpole', *_t(full, init, e[:, :, None]), n_steps=steps, terminate=True, dtype=F64,
                             policy=policy, replace=None if replace is None else torch.from_numpy(replace))
        got = pairs.cartpole_pairs(n, steps, policy=policy, seed=seed, terminate=True, frac_rnd=frac, noise_std=std)
        assert torch.equal(got[1], want[0].float()) and torch.equal(got[2], want[1].float())
        assert torch.equal(got[3], want[2]) and got[1].dtype == F32
        if frac > 0:        # where replaced, the action taken is the uniform draw
            assert np.array_equal(got[2][:, :steps, 0].numpy()[replace], instead[replace].astype(np.float32))
    with pytest.raises(ValueError, match='frac_rnd must lie in'):
        pairs.cartpole_pairs(n, steps, policy=policy, frac_rnd=1.5)


# ------------------------------------------------------------------ the host path of rollout
@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('hidden', ((), (5,), (3, 64)), ids=PC.hidden_id)
def test_host_rollout_with_a_policy_is_the_definition_step_by_step(task, hidden):
    n, steps = SC.EPISODES + 1, 9
    for activation in PC.ACTIVATIONS:
        policy, weights, biases = _policy(task, hidden, activation)
        for ta in SC.ta_of(steps):
            params, init, actions = SC.draws(task, n, ta, seed=steps)
            for marks in (None, PC.replace_marks(n, ta)):
                want = PC.closed_loop_by_steps(task, weights, biases, activation, params, init, actions, marks, steps)
                got = pairs.rollout(task, *_t(params, init, actions), n_steps=steps, dtype=F64, policy=policy,
                                    replace=None if marks is None else torch.from_numpy(marks))
                assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
                assert (got[2] == steps + 1).all()
                # fp32: the doubles rounded once
                g32 = pairs.rollout(task, *_t(params, init, actions), n_steps=steps, policy=policy,
                                    replace=None if marks is None else torch.from_numpy(marks))
                assert g32[0].dtype == F32 and torch.equal(g32[0], got[0].float()) and torch.equal(g32[1], got[1].float())
                if marks is not None:
                    t = np.minimum(np.arange(steps), ta - 1)
                    on = marks[:, t] != 0
                    assert np.array_equal(got[1].numpy()[:, :steps, 0][on], actions.astype(np.float64)[:, t, 0][on])
    # replace all ones is the open-loop call; policy=None is the call it always was
    ones = torch.ones(n, ta, dtype=torch.uint8)
    open_loop = pairs.rollout(task, *_t(params, init, actions), n_steps=steps, dtype=F64)
    same = pairs.rollout(task, *_t(params, init, actions), n_steps=steps, dtype=F64, policy=policy, replace=ones)
    assert all(torch.equal(x, y) for x, y in zip(open_loop, same))


@pytest.mark.parametrize('steps', PC.STEPS)
def test_ends_with_a_policy_on_the_host_path(steps):
    params, init, actions, weights, biases = PC.ends_case(steps)
    policy = pairs.MLPPolicy(weights, biases, 'tanh')
    args = _t(params, init, actions)
    states, acts, lengths = pairs.rollout('cartpole', *args, n_steps=steps, terminate=True, dtype=F64, policy=policy)
    free = pairs.rollout('cartpole', *args, n_steps=steps, dtype=F64, policy=policy)
    lens = lengths.numpy()
    seen = sorted(set(lens.tolist()))
    print('T=%d: lengths seen %s' % (steps, seen))
    assert seen[0] == 2 and (steps == 1 or len(seen) > 1)
    if steps in (9, 17):
        assert seen == list(range(2, steps + 2))
    assert np.array_equal(lens, SC.lengths_by_scan('cartpole', free[0].numpy())) and (free[2] == steps + 1).all()
    want = SC.filled(free[0].numpy(), free[1].numpy(), lens)
    assert np.array_equal(states.numpy(), want[0]) and np.array_equal(acts.numpy(), want[1])


def test_balance_gains_keep_the_pole_up_on_the_host_path():
    policy = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
    held = pairs.cartpole_pairs(256, 50, policy=policy, frac_rnd=0.1, seed=0, terminate=True)
    rand = pairs.cartpole_pairs(256, 50, seed=0, terminate=True)
    assert (held[3] == 51).all() and int((rand[3] < 51).sum()) > 128
