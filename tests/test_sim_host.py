"""CPU-side checks of the rollouts (include/bsig_sim.h, bayes_sim_ig_amd/pairs.py): the host path of
``pairs.rollout`` against ``pendulum_pairs`` (bitwise) and against known answers, ``cartpole_pairs``' contract,
the binding's table and the precision seam's pair, every argument check of the launch entry points before any
launch, the Python mirror's ValueErrors -- and the yardstick of tests/sim_cases.py itself: its restatement of the
steps agrees with the host path bitwise, its bound is small enough to prove something and refuses a perturbed
state, and the seed of the episode-end cases holds every kind of end."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sim_cases as SC
from conftest import ROOT
from bayes_sim_ig_amd import _lib, pairs

FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsig_last_error().decode()


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


# ------------------------------------------------------------------ the host path
def test_pendulum_on_the_host_is_pendulum_pairs_bitwise():
    """The draws of pendulum_pairs(64, 20, seed=3) in its documented order: theta, th, thdot, then the actions of
    every step."""
    rs = np.random.RandomState(3)
    theta = rs.uniform(np.array([0.01, 0.01]), np.array([2.0, 2.0]), size=(64, 2))
    th = rs.uniform(-np.pi, np.pi, size=64)
    thdot = rs.uniform(-1.0, 1.0, size=64)
    acts = np.stack([rs.rand(64) for _ in range(20)], axis=1)[:, :, None]
    want_theta, want_states, want_actions = pairs.pendulum_pairs(64, 20, seed=3)
    assert torch.equal(torch.from_numpy(theta).float(), want_theta)
    params, init, actions = _t(theta, np.column_stack([th, thdot]), acts)
    states, actions_out, lengths = pairs.rollout('pendulum', params, init, actions, n_steps=20, dtype=F64)
    assert states.dtype == F64 and actions_out.dtype == F64 and lengths.dtype == torch.int32
    assert tuple(states.shape) == (64, 21, 3) and tuple(actions_out.shape) == (64, 21, 1)
    assert torch.equal(states.float(), want_states) and torch.equal(actions_out.float(), want_actions)
    assert (lengths == 21).all()
    # terminate changes nothing on Pendulum; padded actions give the default n_steps
    again = pairs.rollout('pendulum', params, init, actions_out, terminate=True, dtype=F64)
    assert all(torch.equal(x, y) for x, y in zip(again, (states, actions_out, lengths)))
    # dtype=None: the inputs as fp32, the doubles rounded once
    s32, a32, l32 = pairs.rollout('pendulum', params, init, actions, n_steps=20)
    want = pairs.rollout('pendulum', params.float(), init.float(), actions.float(), n_steps=20, dtype=F64)
    assert s32.dtype == F32 and torch.equal(s32, want[0].float()) and torch.equal(a32, want[1].float())


def test_pendulum_with_ones_reaches_the_speed_limit_exactly():
    n, steps = 8, 30
    params = torch.full((n, 2), 0.5, dtype=F64)
    init = torch.zeros(n, 2, dtype=F64)
    states, actions_out, _ = pairs.rollout('pendulum', params, init, torch.ones(n, 1, 1, dtype=F64), n_steps=steps,
                                           dtype=F64)
    thdot = states[:, :, 2]
    assert (thdot == 8.0).any(dim=1).all() and float(thdot.abs().max()) == 8.0
    assert (actions_out == 1.0).all()
    np.testing.assert_allclose((states[:, :, 0] ** 2 + states[:, :, 1] ** 2).numpy(), 1.0, rtol=0, atol=4 * SC.U64)


@pytest.mark.parametrize('dtype', [None, F64])
def test_cartpole_known_answers(dtype):
    n, steps = 5, 12
    params = torch.tensor([[0.1, 0.5, 1.0]] * n, dtype=F64)
    zeros = pairs.rollout('cartpole', params, torch.zeros(n, 4, dtype=F64), torch.zeros(n, 3, 1, dtype=F64),
                          n_steps=steps, terminate=True, dtype=dtype)
    assert (zeros[0] == 0).all() and (zeros[1] == 0).all() and (zeros[2] == steps + 1).all()
    assert not torch.signbit(zeros[0]).any()
    # |th| already beyond 12 degrees: state 1 is terminal, L = 2, the tail repeats it and action 0
    init = torch.zeros(n, 4, dtype=F64)
    init[:, 2] = torch.tensor([0.5, -0.5, 0.3, -0.25, 0.0])
    actions = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, size=(n, steps, 1)))
    states, actions_out, lengths = pairs.rollout('cartpole', params, init, actions, n_steps=steps, terminate=True,
                                                 dtype=dtype)
    assert lengths[:4].tolist() == [2, 2, 2, 2] and int(lengths[4]) > 2
    free = pairs.rollout('cartpole', params, init, actions, n_steps=steps, dtype=dtype)
    assert (free[2] == steps + 1).all()
    for i in range(4):
        assert torch.equal(states[i, :2], free[0][i, :2])
        assert (states[i, 2:] == states[i, 1]).all() and (actions_out[i, 1:] == actions_out[i, 0]).all()
        assert torch.equal(actions_out[i, 0], actions[i, 0].to(actions_out.dtype))
    assert torch.equal(free[1][:, :steps], actions.to(free[1].dtype)) and torch.equal(free[1][:, steps],
                                                                                      free[1][:, steps - 1])
    # a short action array is padded with its last action
    short = pairs.rollout('cartpole', params, init, actions[:, :3], n_steps=steps, dtype=dtype)
    padded = pairs.rollout('cartpole', params, init, torch.cat([actions[:, :3]] + [actions[:, 2:3]] * 6, dim=1),
                           n_steps=steps, dtype=dtype)
    assert all(torch.equal(x, y) for x, y in zip(short, padded))


def test_a_nonfinite_state_raises_the_flag_and_nothing_else():
    params, init, actions = _t(*SC.draws('cartpole', 6, 5, seed=2))
    flag = torch.zeros(1, dtype=torch.int32)
    clean = pairs.rollout('cartpole', params, init, actions, n_steps=9, dtype=F64, nonfinite=flag)
    assert int(flag) == 0
    bad = params.clone()
    bad[3, 1] = float('nan')
    got = pairs.rollout('cartpole', bad, init, actions, n_steps=9, dtype=F64, nonfinite=flag)
    assert int(flag) == 1
    keep = [0, 1, 2, 4, 5]
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.isnan(got[0][3, 1:]).any()
    assert torch.equal(got[0][3, 0], clean[0][3, 0])


def test_the_host_path_never_asks_for_a_gpu(monkeypatch):
    def no_gpu():
        raise RuntimeError('asked for a GPU')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    out = pairs.rollout('cartpole', *_t(*SC.draws('cartpole', 3, 4)), n_steps=4)
    assert all(x.device.type == 'cpu' for x in out)
    assert pairs.cartpole_pairs(3, 4, seed=0)[1].device.type == 'cpu'


# ------------------------------------------------------------------ cartpole_pairs
def test_cartpole_pairs_contract():
    theta, states, actions = pairs.cartpole_pairs(40, 20, seed=5)
    assert tuple(theta.shape) == (40, 2) and tuple(states.shape) == (40, 21, 4) and tuple(actions.shape) == (40, 21, 1)
    assert theta.dtype == states.dtype == actions.dtype == F32
    assert float(theta.min()) >= 0.1 and float(theta.max()) <= 2.0
    assert float(states[:, 0].abs().max()) <= 0.05 and float(actions.abs().max()) <= 1.0
    assert torch.equal(actions[:, 20], actions[:, 19])
    again = pairs.cartpole_pairs(40, 20, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(again, (theta, states, actions)))
    assert not torch.equal(pairs.cartpole_pairs(40, 20, seed=6)[1], states)
    # the documented order of the draws
    rs = np.random.RandomState(5)
    th = rs.uniform(np.array([0.1, 0.1]), np.array([2.0, 2.0]), size=(40, 2))
    init = rs.uniform(-0.05, 0.05, size=(40, 4))
    acts = rs.uniform(-1.0, 1.0, size=(40, 20))
    assert torch.equal(theta, torch.from_numpy(th).float())
    assert torch.equal(states[:, 0], torch.from_numpy(init).float())
    assert torch.equal(actions[:, :20, 0], torch.from_numpy(acts).float())
    full = torch.from_numpy(np.column_stack([th, np.ones(40)]))
    want = pairs.rollout('cartpole', full, *_t(init, acts[:, :, None]), n_steps=20, dtype=F64)
    assert torch.equal(states, want[0].float())
    # three bounds: the cart's mass is drawn too
    theta3, states3, _ = pairs.cartpole_pairs(40, 20, lows=(0.1, 0.1, 0.5), highs=(2.0, 2.0, 1.5), seed=5)
    assert tuple(theta3.shape) == (40, 3) and 0.5 <= float(theta3[:, 2].min()) <= float(theta3[:, 2].max()) <= 1.5
    # 'ones', a fixed theta, another cart
    theta1, _, ones = pairs.cartpole_pairs(4, 6, policy='ones', params=(0.3, 0.7), cart_mass=2.0, seed=1)
    assert (ones == 1).all() and torch.equal(theta1, torch.tensor([[0.3, 0.7]] * 4))
    with pytest.raises(ValueError, match='unknown collection policy'):
        pairs.cartpole_pairs(4, 6, policy='greedy', seed=1)
    with pytest.raises(ValueError, match='2 or 3 bounds'):
        pairs.cartpole_pairs(4, 6, lows=(0.1,), highs=(2.0,), seed=1)


def test_cartpole_pairs_with_episode_ends():
    theta, states, actions, lengths = pairs.cartpole_pairs(300, 50, seed=0, terminate=True)
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (300,)
    theta_f, states_f, actions_f = pairs.cartpole_pairs(300, 50, seed=0)
    assert torch.equal(theta, theta_f)
    assert int(lengths.min()) >= 2 and int(lengths.max()) == 51 and int((lengths < 51).sum()) > 100
    # a direct scan of the returned states by the end condition
    assert np.array_equal(SC.lengths_by_scan('cartpole', states.double().numpy()), lengths.numpy())
    # pairs.end_episodes applied to the untruncated rollout
    want_states, want_actions = pairs.end_episodes(states_f, actions_f, lengths)
    assert torch.equal(states, want_states) and torch.equal(actions, want_actions)


# ------------------------------------------------------------------ the binding
def test_the_headers_table_the_constants_and_the_seam(lib):
    assert sorted(_lib.HEADERS['bsig_sim.h']) == ['bsig_sim_dims', 'bsig_sim_rollout', 'bsig_sim_rollout_f64']
    assert _lib.Precision.OPS['sim_rollout'] == ('bsig_sim_rollout', 'bsig_sim_rollout_f64')
    assert _lib.HEADERS['bsig_sim.h']['bsig_sim_rollout'] == _lib.HEADERS['bsig_sim.h']['bsig_sim_rollout_f64']
    with open(os.path.join(ROOT, 'include', 'bsig_sim.h')) as f:
        header = f.read()
    define = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1))      # noqa: E731
    assert (define('BSIG_SIM_PENDULUM'), define('BSIG_SIM_CARTPOLE')) == (0, 1) \
        == (_lib.SIM_PENDULUM, _lib.SIM_CARTPOLE) == (SC.TASK_IDS['pendulum'], SC.TASK_IDS['cartpole'])
    assert _lib.SIM_TASKS == SC.TASK_IDS
    assert (define('BSIG_SIM_EPISODES'), define('BSIG_SIM_STEP_BLOCK'), define('BSIG_SIM_GRID_CAP')) \
        == (_lib.SIM_EPISODES, _lib.SIM_STEP_BLOCK, _lib.SIM_GRID_CAP) == (SC.EPISODES, SC.STEP_BLOCK, SC.GRID_CAP)
    # 32 000 episodes put a wavefront on every CU
    assert -(-32000 // SC.EPISODES) >= 256


def test_dims(lib):
    for task, want in SC.DIMS.items():
        got = [C.c_int(-1) for _ in range(3)]
        assert lib.bsig_sim_dims(SC.TASK_IDS[task], *[C.byref(g) for g in got]) == _lib.BSIG_OK
        assert tuple(g.value for g in got) == want == pairs.SIM_DIMS[task]
        assert lib.bsig_sim_dims(SC.TASK_IDS[task], None, None, None) == _lib.BSIG_OK
    for bad in (-1, 2, 7):
        assert lib.bsig_sim_dims(bad, None, None, None) == _lib.BSIG_EINVAL and 'task %d' % bad in err(lib)


@pytest.mark.parametrize('fn', ['bsig_sim_rollout', 'bsig_sim_rollout_f64'])
def test_launch_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = fn[len('bsig_'):]
    six = (FAKE,) * 6
    # (task, params, init, actions, states, actions_out, lengths, n, T, Ta, terminate, nonfinite, stream)
    for task in (-1, 2):
        rc = call(task, *six, 4, 20, 20, 0, None, None)
        assert rc == _lib.BSIG_EINVAL and 'unknown task %d' % task in err(lib) and err(lib).startswith(what + ':')
    for steps in (0, -3):
        rc = call(0, *six, 4, steps, 20, 0, None, None)
        assert rc == _lib.BSIG_EINVAL and 'T %d' % steps in err(lib) and err(lib).startswith(what + ':')
    for ta in (0, -1):
        rc = call(1, *six, 4, 20, ta, 0, None, None)
        assert rc == _lib.BSIG_EINVAL and 'Ta %d' % ta in err(lib)
    rc = call(1, *six, -1, 20, 20, 0, None, None)
    assert rc == _lib.BSIG_EINVAL and 'n=-1' in err(lib)
    for terminate in (2, -1):
        rc = call(1, *six, 4, 20, 20, terminate, None, None)
        assert rc == _lib.BSIG_EINVAL and 'terminate %d' % terminate in err(lib)
    for hole in range(6):
        args = [FAKE] * 6
        args[hole] = None
        rc = call(1, *args, 4, 20, 20, 1, FAKE, None)
        assert rc == _lib.BSIG_EINVAL and 'null' in err(lib)
    # an empty batch is fine and touches nothing, whatever else is passed
    assert call(0, *six, 0, 20, 20, 0, None, None) == _lib.BSIG_OK
    assert call(1, None, None, None, None, None, None, 0, 20, 20, 1, None, None) == _lib.BSIG_OK
    assert call(5, None, None, None, None, None, None, 0, 0, 0, 3, None, None) == _lib.BSIG_OK


# ------------------------------------------------------------------ the Python mirror
def test_rollouts_value_errors_name_the_argument():
    params, init, actions = _t(*SC.draws('cartpole', 4, 6))
    ok = dict(n_steps=5)
    with pytest.raises(ValueError, match="task must be 'pendulum' or 'cartpole'"):
        pairs.rollout('acrobot', params, init, actions, **ok)
    with pytest.raises(ValueError, match=r'params must be \[N, 3\] for cartpole'):
        pairs.rollout('cartpole', params[:, :2], init, actions, **ok)
    with pytest.raises(ValueError, match=r'params must be \[N, 2\] for pendulum'):
        pairs.rollout('pendulum', params, init, actions, **ok)
    with pytest.raises(ValueError, match=r'init must be \[4, 4\] for cartpole'):
        pairs.rollout('cartpole', params, init[:3], actions, **ok)
    with pytest.raises(ValueError, match=r'init must be \[4, 2\] for pendulum'):
        pairs.rollout('pendulum', params[:, :2], init, actions, **ok)
    for bad in (actions[:, :, 0], actions[:3], actions[:, :0], actions.repeat(1, 1, 2)):
        with pytest.raises(ValueError, match=r'actions must be \[4, Ta >= 1, 1\]'):
            pairs.rollout('cartpole', params, init, bad, **ok)
    with pytest.raises(ValueError, match='params must be a floating-point tensor'):
        pairs.rollout('cartpole', params.numpy(), init, actions, **ok)
    with pytest.raises(ValueError, match='init must be a floating-point tensor'):
        pairs.rollout('cartpole', params, init.long(), actions, **ok)
    for bad in (0, -1, 2.5, '3', True):
        with pytest.raises(ValueError, match='n_steps must be an int >= 1'):
            pairs.rollout('cartpole', params, init, actions, n_steps=bad)
    with pytest.raises(ValueError, match='n_steps defaults to Ta - 1'):
        pairs.rollout('cartpole', params, init, actions[:, :1])
    with pytest.raises(ValueError, match='terminate must be a bool'):
        pairs.rollout('cartpole', params, init, actions, terminate=1, **ok)
    with pytest.raises(ValueError, match='torch.float32 or torch.float64'):
        pairs.rollout('cartpole', params, init, actions, dtype=torch.float16, **ok)
    with pytest.raises(ValueError, match='nonfinite must be a 1-element int32 tensor'):
        pairs.rollout('cartpole', params, init, actions, nonfinite=torch.zeros(1), **ok)
    assert pairs.rollout('cartpole', params, init, actions)[0].shape[1] == 6      # n_steps = Ta - 1
    empty = pairs.rollout('cartpole', params[:0], init[:0], actions[:0], **ok)
    assert [tuple(x.shape) for x in empty] == [(0, 6, 4), (0, 6, 1), (0,)]


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize('task,corner', [('pendulum', False), ('pendulum', True), ('cartpole', False)])
def test_the_step_check_passes_the_host_path_and_refuses_a_perturbed_state(task, corner):
    params, init, actions = SC.draws(task, 70, 5, seed=1, corner=corner, wide=True)
    states, _, lengths = pairs.rollout(task, *_t(params, init, actions), n_steps=40, terminate=True, dtype=F64)
    states, lengths = states.numpy(), lengths.numpy()
    worst = SC.step_check(task, params, init, actions, states, lengths)
    print(task, corner, worst)
    assert all(q <= 1.0 for q in worst.values())
    if task == 'cartpole':       # the same numpy operations: the restatement and the host path agree bitwise
        assert all(q == 0.0 for q in worst.values())
        assert np.array_equal(lengths, SC.lengths_by_scan(task, states))
    # one state moved by 1e-9 of its size (or 1e-9): millions of ulps, and yet far below any whole-trajectory
    # comparison's tolerance -- the check must refuse it
    n, t = 11, 1
    assert lengths[n] > t + 1
    col = 2 if task == 'pendulum' and not corner else (0 if task == 'pendulum' else 3)
    moved = states.copy()
    moved[n, t + 1, col] += 1e-9 * max(1.0, abs(moved[n, t + 1, col]))
    try:
        refused = any(q > 1.0 for q in SC.step_check(task, params, init, actions, moved, lengths).values())
    except AssertionError:
        refused = True
    assert refused


def test_the_episode_end_cases_hold_every_kind():
    params, init, actions = SC.draws('cartpole', SC.ENDS_COUNT, SC.ENDS_STEPS, seed=SC.ENDS_SEED, wide=True)
    states, actions_out, lengths = pairs.rollout('cartpole', *_t(params, init, actions), n_steps=SC.ENDS_STEPS,
                                                 terminate=True, dtype=F64)
    kinds = SC.end_kinds(states.numpy(), lengths.numpy())
    print(kinds)
    assert set(kinds) == set(SC.END_KINDS) and all(count >= 1 for count in kinds.values())
    free = pairs.rollout('cartpole', *_t(params, init, actions), n_steps=SC.ENDS_STEPS, dtype=F64)
    want = SC.filled(free[0].numpy(), SC.step_actions(actions.astype(np.float64), SC.ENDS_STEPS), lengths.numpy())
    assert np.array_equal(states.numpy(), want[0]) and np.array_equal(actions_out.numpy(), want[1])
