"""GPU checks of the rollout kernel (include/bsig_sim.h, csrc/sim.h) through ``pairs.rollout`` and
``pairs.cartpole_pairs`` on GPU tensors.

What is compared with: tests/sim_cases.py -- the two tasks' steps restated in numpy, in double, applied step by
step to the kernel's OWN double states (never whole trajectories against the host path), within the bound its
docstring derives from the step's operation counts and the project's allowance for a double sine; bitwise where
no sine enters.  The fp32 outputs are compared bitwise with the double ones rounded; the episode ends with a scan
of the double outputs by the end condition, the fill rule and the launch without ends.

The shapes: N around the workgroup's W = 64 episodes, T around the step block B = 8 (T + 1 states are walked in
blocks of B) plus 20 and 200, Ta in {1, T, T + 1, T + 4}, one launch beyond the grid cap.  Parameters, initial
states and actions are fp32-representable, so both entry points take them exactly.  Every comparison with a bound
prints its worst |error| / bound."""
import functools

import numpy as np
import pytest
import torch

import sim_cases as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TASKS = ('pendulum', 'cartpole')
N_MAX = SC.COUNTS[-1]


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@functools.lru_cache(maxsize=None)
def _draws(task, steps, corner=False, wide=False):
    """(params, init, actions) float32 arrays for 3 W + 2 episodes with T + 4 actions: made once per shape, cut
    to fewer episodes and fewer actions by the tests, never modified."""
    return SC.draws(task, N_MAX, steps + 4, seed=steps, corner=corner, wide=wide)


def _dev(arrays, n, ta, dtype=None):
    params, init, actions = arrays
    out = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (params[:n], init[:n], actions[:n, :ta])]
    return [x.to(dtype) for x in out] if dtype is not None else out


def _rollout(B, task, arrays, n, ta, steps, dtype, terminate=False, **kw):
    out = B.pairs.rollout(task, *_dev(arrays, n, ta), n_steps=steps, terminate=terminate, dtype=dtype, **kw)
    states, actions_out, lengths = out
    sd = SC.DIMS[task][2]
    assert states.dtype == actions_out.dtype == dtype and lengths.dtype == torch.int32
    assert tuple(states.shape) == (n, steps + 1, sd) and tuple(actions_out.shape) == (n, steps + 1, 1)
    assert tuple(lengths.shape) == (n,) and all(x.device.type == 'cuda' and x.is_contiguous() for x in out)
    return out


SHAPES = pytest.mark.parametrize('task,steps', [(task, steps) for task in TASKS for steps in SC.STEPS],
                                 ids=['%s-T%d' % (task, steps) for task in TASKS for steps in SC.STEPS])


# ------------------------------------------------------------------ 1. the recurrence, 2. the fp32 outputs
@SHAPES
def test_every_step_is_the_definitions_and_fp32_is_the_doubles_rounded(B, task, steps):
    arrays = _draws(task, steps)
    worst = {}
    for n in SC.COUNTS:
        for ta in SC.ta_of(steps):
            params, init, actions = (x[:n] for x in arrays)
            actions = actions[:, :ta]
            s64, a64, l64 = _rollout(B, task, arrays, n, ta, steps, F64)
            s32, a32, l32 = _rollout(B, task, arrays, n, ta, steps, F32)
            # 2. bitwise the doubles rounded once
            assert torch.equal(s32, s64.float()) and torch.equal(a32, a64.float()) and torch.equal(l32, l64)
            states = s64.cpu().numpy()
            assert np.isfinite(states).all() and (l64 == steps + 1).all()
            assert np.array_equal(a64.cpu().numpy(), SC.step_actions(actions.astype(np.float64), steps))
            # state 0 is the observation of the initial state
            if task == 'cartpole':
                assert np.array_equal(states[:, 0], init.astype(np.float64))
            else:
                assert np.array_equal(states[:, 0, 2], init[:, 1].astype(np.float64))
                want = np.stack([np.cos(init[:, 0].astype(np.float64)), np.sin(init[:, 0].astype(np.float64))], 1)
                assert np.abs(states[:, 0, :2] - want).max() <= 2 * SC.SINCOS
            # 1. every step
            for name, q in SC.step_check(task, params, init, actions, states, l64.cpu().numpy()).items():
                worst[name] = max(worst.get(name, 0.0), q)
    print('%s T=%d: worst |kernel - numpy step| / bound: %s'
          % (task, steps, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert all(q <= 1.0 for q in worst.values()), worst


@pytest.mark.parametrize('steps', [SC.STEP_BLOCK + 1, 20])
def test_pendulum_at_the_priors_corner(B, steps):
    """l = m = 0.01: 3 g / (2 l) = 1500 and 3 / (m l^2) = 3e6, the largest gains of the map."""
    arrays = _draws('pendulum', steps, corner=True)
    n, ta = SC.EPISODES + 1, steps
    s64, _, l64 = _rollout(B, 'pendulum', arrays, n, ta, steps, F64)
    s32, _, _ = _rollout(B, 'pendulum', arrays, n, ta, steps, F32)
    assert torch.equal(s32, s64.float())
    worst = SC.step_check('pendulum', arrays[0][:n], arrays[1][:n], arrays[2][:n, :ta], s64.cpu().numpy(),
                          l64.cpu().numpy())
    print('corner T=%d: worst |kernel - numpy step| / bound: %s' % (steps, worst))
    assert all(q <= 1.0 for q in worst.values()), worst
    assert float(s64[:, :, 2].abs().max()) == 8.0


def test_ones_on_pendulum_reaches_the_speed_limit_exactly(B):
    n = 5
    params = torch.full((n, 2), 0.5, device=DEV)
    states, actions_out, _ = B.pairs.rollout('pendulum', params, torch.zeros(n, 2, device=DEV),
                                             torch.ones(n, 1, 1, device=DEV), n_steps=30, dtype=F64)
    assert (states[:, :, 2] == 8.0).any(dim=1).all() and float(states[:, :, 2].abs().max()) == 8.0
    assert (actions_out == 1.0).all()
    zeros = B.pairs.rollout('cartpole', torch.full((n, 3), 0.5, device=DEV), torch.zeros(n, 4, device=DEV),
                            torch.zeros(n, 2, 1, device=DEV), n_steps=30, terminate=True)
    assert (zeros[0] == 0).all() and (zeros[1] == 0).all() and (zeros[2] == 31).all()


# ------------------------------------------------------------------ 3. the ends
def _check_ends(B, steps, n, ta, dtype):
    arrays = _draws('cartpole', steps, wide=True)
    states, actions_out, lengths = _rollout(B, 'cartpole', arrays, n, ta, steps, dtype, terminate=True)
    free = _rollout(B, 'cartpole', arrays, n, ta, steps, dtype)
    s64, _, l64 = _rollout(B, 'cartpole', arrays, n, ta, steps, F64, terminate=True)
    assert (free[2] == steps + 1).all() and torch.equal(lengths, l64)
    lens = lengths.cpu().numpy()
    # the lengths are a scan of the double outputs by the end condition
    assert np.array_equal(lens, SC.lengths_by_scan('cartpole', s64.cpu().numpy()))
    assert lens.min() >= 2 and lens.max() <= steps + 1
    # the tails follow the fill rule, and the first L_n states are bitwise those of the launch without ends
    want = SC.filled(free[0].cpu().numpy(), free[1].cpu().numpy(), lens)
    assert np.array_equal(states.cpu().numpy(), want[0]) and np.array_equal(actions_out.cpu().numpy(), want[1])
    both = B.pairs.end_episodes(free[0], free[1], lengths)
    assert torch.equal(states, both[0]) and torch.equal(actions_out, both[1])
    return s64.cpu().numpy(), lens


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_episode_ends_of_every_kind(B, dtype):
    """The case of tests/sim_cases.py (ENDS_*): ends at L = 2, inside a block, at a block's edge, at state T, and
    episodes that never end, all in one launch of 3 W + 2 episodes."""
    assert N_MAX == SC.ENDS_COUNT
    arrays = SC.draws('cartpole', SC.ENDS_COUNT, SC.ENDS_STEPS, seed=SC.ENDS_SEED, wide=True)
    steps = SC.ENDS_STEPS
    states, actions_out, lengths = _rollout(B, 'cartpole', arrays, N_MAX, steps, steps, dtype, terminate=True)
    free = _rollout(B, 'cartpole', arrays, N_MAX, steps, steps, dtype)
    s64, _, l64 = _rollout(B, 'cartpole', arrays, N_MAX, steps, steps, F64, terminate=True)
    lens = lengths.cpu().numpy()
    assert torch.equal(lengths, l64) and np.array_equal(lens, SC.lengths_by_scan('cartpole', s64.cpu().numpy()))
    kinds = SC.end_kinds(s64.cpu().numpy(), lens)
    print('ends: %s' % kinds)
    assert all(kinds[kind] >= 1 for kind in SC.END_KINDS)
    want = SC.filled(free[0].cpu().numpy(), free[1].cpu().numpy(), lens)
    assert np.array_equal(states.cpu().numpy(), want[0]) and np.array_equal(actions_out.cpu().numpy(), want[1])
    worst = SC.step_check('cartpole', *arrays, s64.cpu().numpy(), lens)
    assert all(q <= 1.0 for q in worst.values()), worst


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('steps', SC.STEPS)
def test_episode_ends_at_every_shape(B, steps, dtype):
    seen = set()
    for n in SC.COUNTS:
        for ta in SC.ta_of(steps):
            _, lens = _check_ends(B, steps, n, ta, dtype)
            seen.update(lens.tolist())
    print('T=%d: lengths seen %s' % (steps, sorted(seen)))
    assert 2 in seen and (steps == 1 or len(seen) > 1)


# ------------------------------------------------------------------ the grid stride
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', TASKS)
def test_workgroups_stride_over_more_episodes_than_the_grid_holds(B, task, dtype):
    """2 cap W + 5 episodes at T = 3: every workgroup takes a second batch, some a third, the last one partly
    empty.  The rows are those of the same episodes in a batch the grid holds."""
    steps, ta = 3, 3
    arrays = _draws(task, steps, wide=True)
    small = _rollout(B, task, arrays, N_MAX, ta, steps, dtype, terminate=True)
    n = 2 * SC.GRID_CAP * SC.EPISODES + 5
    reps = -(-n // N_MAX)
    params, init, actions = (x.repeat(*([reps] + [1] * (x.dim() - 1)))[:n] for x in _dev(arrays, N_MAX, ta))
    got = B.pairs.rollout(task, params, init, actions, n_steps=steps, terminate=True, dtype=dtype)
    assert tuple(got[0].shape) == (n, steps + 1, SC.DIMS[task][2]) and tuple(got[2].shape) == (n,)
    assert torch.equal(got[0], small[0].repeat(reps, 1, 1)[:n])
    assert torch.equal(got[1], small[1].repeat(reps, 1, 1)[:n])
    assert torch.equal(got[2], small[2].repeat(reps)[:n])


# ------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', TASKS)
def test_bits_repeat_rows_permute_and_a_nan_stays_in_its_episode(B, task, dtype):
    steps, ta, n = 20, 21, N_MAX
    arrays = _draws(task, steps, wide=True)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    first = _rollout(B, task, arrays, n, ta, steps, dtype, terminate=True, nonfinite=flag)
    again = _rollout(B, task, arrays, n, ta, steps, dtype, terminate=True, nonfinite=flag)
    assert all(torch.equal(x, y) for x, y in zip(first, again)) and int(flag.item()) == 0
    # a permutation of the episodes permutes the rows; fewer episodes are the first rows
    perm = torch.from_numpy(np.random.RandomState(7).permutation(n)).to(DEV)
    params, init, actions = _dev(arrays, n, ta)
    moved = B.pairs.rollout(task, params[perm], init[perm], actions[perm], n_steps=steps, terminate=True,
                            dtype=dtype)
    assert all(torch.equal(x[perm], y) for x, y in zip(first, moved))
    fewer = _rollout(B, task, arrays, SC.EPISODES + 1, ta, steps, dtype, terminate=True)
    assert all(torch.equal(x[:SC.EPISODES + 1], y) for x, y in zip(first, fewer))
    # a NaN parameter: the flag, that episode's states from state 1 on, and nothing else
    for victim in (0, SC.EPISODES - 1, SC.EPISODES + 2, n - 1):
        bad = params.clone()
        bad[victim, 1] = float('nan')
        flag.zero_()
        got = B.pairs.rollout(task, bad, init, actions, n_steps=steps, terminate=True, dtype=dtype, nonfinite=flag)
        assert int(flag.item()) == 1
        keep = torch.arange(n, device=DEV) != victim
        assert all(torch.equal(x[keep], y[keep]) for x, y in zip(first, got))
        assert torch.isnan(got[0][victim, 1:]).any(dim=1).all() and torch.isfinite(got[0][victim, 0]).all()
    # no flag asked for: the same outputs
    flag.zero_()
    quiet = B.pairs.rollout(task, bad, init, actions, n_steps=steps, terminate=True, dtype=dtype)
    assert int(flag.item()) == 0 and torch.equal(torch.nan_to_num(quiet[0]), torch.nan_to_num(got[0]))


def test_nothing_is_written_beyond_the_outputs(B):
    """The C entry points on buffers with a guard band behind every output, at a T whose last block is partial."""
    _lib = B._lib
    for task in TASKS:
        for prec, dtype in ((_lib.F32, F32), (_lib.F64, F64)):
            n, steps, ta = SC.EPISODES + 3, SC.STEP_BLOCK + 2, 4
            pd, idim, sd = SC.DIMS[task]
            params, init, actions = _dev(_draws(task, steps, wide=True), n, ta, dtype)
            sizes = (n * (steps + 1) * sd, n * (steps + 1), n)
            bufs = [torch.full((size + 64,), -9.0, dtype=dtype, device=DEV) for size in sizes[:2]]
            bufs.append(torch.full((n + 64,), -9, dtype=torch.int32, device=DEV))
            prec.sim_rollout(SC.TASK_IDS[task], _lib.ptr(params), _lib.ptr(init), _lib.ptr(actions),
                             _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), n, steps, ta, 1, None,
                             _lib.stream())
            want = B.pairs.rollout(task, params, init, actions, n_steps=steps, terminate=True, dtype=dtype)
            for buf, size, ref in zip(bufs, sizes, want):
                assert torch.equal(buf[:size], ref.reshape(-1)) and (buf[size:] == -9).all()
            # outputs that start off a 16-byte boundary take the element stores: the same values
            off = [torch.full((size + 65,), -9.0, dtype=dtype, device=DEV) for size in sizes[:2]]
            prec.sim_rollout(SC.TASK_IDS[task], _lib.ptr(params), _lib.ptr(init), _lib.ptr(actions),
                             _lib.ptr(off[0][1:]), _lib.ptr(off[1][1:]), _lib.ptr(bufs[2]), n, steps, ta, 1, None,
                             _lib.stream())
            for buf, size, ref in zip(off, sizes, want):
                assert torch.equal(buf[1:size + 1], ref.reshape(-1)) and buf[0] == -9 and (buf[size + 1:] == -9).all()


# ------------------------------------------------------------------ 5. end to end
CFG = {'modelClass': 'MDNN', 'trainTrajLen': 51, 'components': 3, 'hiddenLayers': (16, 16), 'lr': 1e-3,
       'inputNorm': True}
SUMMARIES = {'summary_kme': {'kmeFeatures': 64}, 'summary_xcorr': {'xcorrLags': 4}}


@pytest.mark.parametrize('name', sorted(SUMMARIES))
def test_cartpole_pairs_on_the_device_train_an_estimator_with_lengths(B, name):
    theta, states, actions, lengths = B.pairs.cartpole_pairs(2000, 50, seed=0, device=DEV, terminate=True)
    assert all(x.device.type == 'cuda' for x in (theta, states, actions, lengths))
    assert theta.dtype == states.dtype == actions.dtype == F32 and lengths.dtype == torch.int32
    assert tuple(theta.shape) == (2000, 2) and tuple(states.shape) == (2000, 51, 4)
    assert tuple(actions.shape) == (2000, 51, 1) and tuple(lengths.shape) == (2000,)
    ended = int((lengths < 51).sum())
    print('%d of 2000 episodes end early, mean length %.1f' % (ended, float(lengths.float().mean())))
    assert 1000 < ended < 2000 and int(lengths.min()) >= 2
    # the draws are the host's: the same theta, initial states and actions as on the CPU
    host = B.pairs.cartpole_pairs(2000, 50, seed=0, terminate=True)
    assert torch.equal(theta.cpu(), host[0]) and torch.equal(states[:, 0].cpu(), host[1][:, 0])

    def bayes_sim():
        torch.manual_seed(11)
        cfg = dict(CFG, summarizerFxn=name, **SUMMARIES[name])
        return B.BayesSim(model_cfg=cfg, obs_dim=4, act_dim=1, params_dim=2, params_lows=np.array([0.1, 0.1]),
                          params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)
    bs = bayes_sim()
    np.random.seed(31), torch.manual_seed(32)
    logs = bs.fit(theta, states, actions, traj_lengths=lengths)
    assert len(logs) == 2
    for chunk in logs:
        for key in ('train_loss', 'test_loss'):
            assert len(chunk[key]) > 0 and np.isfinite(chunk[key]).all()
    i = int(torch.nonzero(lengths < 51)[0])
    mog = bs.predict(states[i:i + 1], actions[i:i + 1], lengths=[int(lengths[i])])
    assert isinstance(mog, B.pdf.MoG) and np.isfinite(mog.a).all() and abs(float(np.sum(mog.a)) - 1.0) <= 1e-6
    assert np.isfinite(mog.eval(theta[:8].cpu().numpy().astype(np.float64))).all()
    # the same pairs without lengths give other summaries
    rows = bs._summarize(states, actions, lengths=lengths)
    assert torch.isfinite(rows).all() and not torch.equal(rows, bs._summarize(states, actions))
