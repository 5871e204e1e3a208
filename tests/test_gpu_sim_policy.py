"""GPU checks of the closed-loop rollouts (include/bsig_sim_policy.h, csrc/sim.h with csrc/sim_policy.h) through
``pairs.rollout(policy=, replace=)`` and ``pairs.cartpole_pairs(policy=)`` on GPU tensors.

What is compared with: the kernel's OWN outputs and tests/sim_policy_cases.py.  The closed-loop states against an
OPEN-loop launch fed the closed-loop launch's recorded actions (bitwise); the recorded action of step t against
the numpy policy applied to the kernel's own double state t (bitwise for the identity and relu, within the bound
of sim_policy_cases' docstring for tanh); the next state by the unchanged ``sim_cases.step_check`` with the
recorded actions as the open-loop ones; the fp32 outputs against the doubles rounded once; the degenerate
policies against the open-loop launch; the ends by a scan of the double outputs, the fill rule and the launch
without ends.  Whole trajectories are never compared with the host path.

The shapes: N in sim_cases.COUNTS (around the workgroup's 64 episodes), T in (1, 7, 8, 9, 17) (around the step
block 8), Ta in ta_of(T); per policy and T every N and every Ta occur (N_i with Ta_(i + T) % 4), the whole
product for three policies; one launch beyond the grid cap.  Hidden shapes: sim_policy_cases.HIDDEN, with the
widths below, at and above the 4 units the kernel forms side by side.  Every draw is fp32-representable."""
import functools

import numpy as np
import pytest
import torch

import sim_cases as SC
import sim_policy_cases as PC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TASKS = ('pendulum', 'cartpole')
N_MAX = SC.COUNTS[-1]
WHOLE_PRODUCT = ((), (PC.UNITS + 1,), (3, 64))       # the policies that see every (N, Ta) of every T


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@functools.lru_cache(maxsize=None)
def _draws(task, steps):
    """(params, init, actions) float32 arrays for 3 W + 2 episodes with T + 4 actions (CartPole: the `wide`
    initial states, so that episodes end): made once per shape, cut by the tests, never modified."""
    return SC.draws(task, N_MAX, steps + 4, seed=steps, wide=True)


@functools.lru_cache(maxsize=None)
def _weights(task, hidden, seed=0):
    return PC.make_policy(task, hidden, seed)


def _policy(B, task, hidden, activation, seed=0):
    weights, biases = _weights(task, hidden, seed)
    return B.pairs.MLPPolicy(weights, biases, activation).to(DEV), weights, biases


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _rollout(B, task, arrays, n, ta, steps, dtype, terminate=False, policy=None, marks=None, actions=None, **kw):
    params, init, acts = arrays
    acts = acts[:n, :ta] if actions is None else actions
    out = B.pairs.rollout(task, _dev(params[:n]), _dev(init[:n]), _dev(acts), n_steps=steps, terminate=terminate,
                          dtype=dtype, policy=policy, replace=_dev(marks), **kw)
    sd = SC.DIMS[task][2]
    assert out[0].dtype == out[1].dtype == dtype and out[2].dtype == torch.int32
    assert tuple(out[0].shape) == (n, steps + 1, sd) and tuple(out[1].shape) == (n, steps + 1, 1)
    assert tuple(out[2].shape) == (n,) and all(x.device.type == 'cuda' and x.is_contiguous() for x in out)
    return out


def _shapes(hidden, steps):
    tas = SC.ta_of(steps)
    if hidden in WHOLE_PRODUCT:
        return [(n, ta) for n in SC.COUNTS for ta in tas]
    return [(n, tas[(i + steps) % len(tas)]) for i, n in enumerate(SC.COUNTS)]


CASES = [(task, hidden, activation) for task in TASKS for hidden in PC.HIDDEN for activation in PC.ACTIVATIONS]


# ------------------------------------------------------------------ 1. own actions, 2. the action, 3. fp32
@pytest.mark.parametrize('task,hidden,activation', CASES,
                         ids=['%s-%s-%s' % (t, PC.hidden_id(h), a) for t, h, a in CASES])
def test_closed_loop_against_its_own_actions_the_definition_and_fp32(B, task, hidden, activation):
    policy, weights, biases = _policy(B, task, hidden, activation)
    worst, worst_step, count = 0.0, {}, 0
    for steps in PC.STEPS:
        arrays = _draws(task, steps)
        for i, (n, ta) in enumerate(_shapes(hidden, steps)):
            marks = PC.replace_marks(n, ta, seed=steps) if i % 2 else None
            terminate = bool((i // 2) % 2) if hidden in WHOLE_PRODUCT else bool(i % 3 == 0)
            params, init, e_in = arrays[0][:n], arrays[1][:n], arrays[2][:n, :ta]
            s64, a64, l64 = _rollout(B, task, arrays, n, ta, steps, F64, terminate, policy, marks)
            # 3. fp32 is the doubles rounded once
            s32, a32, l32 = _rollout(B, task, arrays, n, ta, steps, F32, terminate, policy, marks)
            assert torch.equal(s32, s64.float()) and torch.equal(a32, a64.float()) and torch.equal(l32, l64)
            # 1. an open-loop launch fed the recorded actions: the same states and lengths, bit for bit
            fed = a64[:, :steps].contiguous()
            o64 = B.pairs.rollout(task, _dev(params), _dev(init), fed, n_steps=steps, terminate=terminate, dtype=F64)
            assert torch.equal(o64[0], s64) and torch.equal(o64[2], l64) and torch.equal(o64[1], a64)
            states, acts, lens = s64.cpu().numpy(), a64.cpu().numpy(), l64.cpu().numpy()
            assert np.isfinite(states).all()
            assert np.array_equal(lens, SC.lengths_by_scan(task, states, terminate))
            # 2. the recorded action of step t is the definition's on the kernel's own state t
            t = np.arange(steps)
            e = SC.step_actions(e_in.astype(np.float64), steps)[:, :steps, 0]
            ref, bound = PC.action_bound(weights, biases, activation, states[:, :steps], e)
            if marks is not None:
                on = marks[:, np.minimum(t, ta - 1)] != 0
                ref, bound = np.where(on, e, ref), np.where(on, 0.0, bound)
            valid = t[None, :] < (lens[:, None] - 1)
            got, exact = acts[:, :steps, 0], (bound == 0) & valid
            assert np.array_equal(got[exact], ref[exact]), 'not bitwise where no tanh enters'
            rest = valid & ~exact
            if rest.any():
                assert np.isfinite(bound[rest]).all()
                worst = max(worst, float((np.abs(got[rest] - ref[rest]) / bound[rest]).max()))
            assert np.array_equal(acts[:, steps], acts[:, steps - 1])
            # ... and the next state is the step's, by the unchanged check of the open-loop tests
            for name, q in SC.step_check(task, params, init, acts[:, :steps], states, lens).items():
                worst_step[name] = max(worst_step.get(name, 0.0), q)
            count += 1
    print('%s %s %s: %d shapes, worst |action - numpy| / bound %.3g; steps: %s'
          % (task, PC.hidden_id(hidden), activation, count, worst,
             ', '.join('%s %.3g' % kv for kv in sorted(worst_step.items()))))
    assert worst <= 1.0 and all(q <= 1.0 for q in worst_step.values()), (worst, worst_step)


# ------------------------------------------------------------------ 4. the degenerate cases
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', TASKS)
def test_degenerate_policies_are_the_open_loop_launch(B, task, dtype):
    for hidden in ((), (PC.UNITS + 1,), (64, 64)):
        for steps in (PC.STEPS[0], PC.STEPS[3], PC.STEPS[4]):
            arrays = _draws(task, steps)
            assert not any((np.signbit(x) & (x == 0)).any() for x in arrays)          # no -0 in the draws
            n, ta = N_MAX, steps + 1
            open_loop = _rollout(B, task, arrays, n, ta, steps, dtype, terminate=True)
            # an all-zero policy adds 0 to every e_t
            weights, biases = _weights(task, hidden)
            zero = B.pairs.MLPPolicy([np.zeros_like(w) for w in weights], [np.zeros_like(b) for b in biases], 'tanh')
            got = _rollout(B, task, arrays, n, ta, steps, dtype, True, zero)
            assert torch.equal(got[0], open_loop[0]) and torch.equal(got[2], open_loop[2])
            # every step replaced: the policy is never asked
            policy, _, _ = _policy(B, task, hidden, 'tanh')
            ones = np.ones((n, ta), dtype=np.uint8)
            got = _rollout(B, task, arrays, n, ta, steps, dtype, True, policy, ones)
            assert all(torch.equal(x, y) for x, y in zip(got, open_loop))
            # a mixed mask: e where replaced, and not e where the policy answers (its bias is not 0)
            marks = PC.replace_marks(n, ta, seed=steps)
            got = _rollout(B, task, arrays, n, ta, steps, dtype, False, policy, marks)
            free = _rollout(B, task, arrays, n, ta, steps, dtype)
            on = _dev(marks[:, np.minimum(np.arange(steps), ta - 1)] != 0)
            assert torch.equal(got[1][:, :steps, 0][on], free[1][:, :steps, 0][on])
            assert not torch.equal(got[1][:, :steps, 0][~on], free[1][:, :steps, 0][~on])
            # bool marks are the same launch
            again = B.pairs.rollout(task, *(_dev(x[:n]) for x in arrays[:2]), _dev(arrays[2][:n, :ta]), n_steps=steps,
                                    dtype=dtype, policy=policy, replace=_dev(marks).bool())
            assert all(torch.equal(x, y) for x, y in zip(got, again))


# ------------------------------------------------------------------ 5. the ends with the policy
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('steps', PC.STEPS)
def test_ends_with_the_policy(B, steps, dtype):
    params, init, actions, weights, biases = PC.ends_case(steps)
    arrays = (params, init, actions)
    # on the host path first: lengths from 2 upward, every length for T = 9 and 17
    host = B.pairs.rollout('cartpole', *(torch.from_numpy(x) for x in arrays), n_steps=steps, terminate=True,
                           dtype=F64, policy=B.pairs.MLPPolicy(weights, biases, 'tanh'))
    seen = sorted(set(host[2].tolist()))
    assert seen[0] == 2 and (steps == 1 or len(seen) > 1)
    assert steps not in (9, 17) or seen == list(range(2, steps + 2))
    policy = B.pairs.MLPPolicy(weights, biases, 'tanh').to(DEV)
    n = N_MAX
    states, acts, lengths = _rollout(B, 'cartpole', arrays, n, steps, steps, dtype, True, policy)
    free = _rollout(B, 'cartpole', arrays, n, steps, steps, dtype, False, policy)
    s64, _, l64 = _rollout(B, 'cartpole', arrays, n, steps, steps, F64, True, policy)
    lens = lengths.cpu().numpy()
    print('T=%d: lengths on the device %s' % (steps, sorted(set(lens.tolist()))))
    assert (free[2] == steps + 1).all() and torch.equal(lengths, l64)
    assert np.array_equal(lens, SC.lengths_by_scan('cartpole', s64.cpu().numpy()))
    assert lens.min() >= 2 and lens.max() <= steps + 1 and len(set(lens.tolist())) == len(seen)
    # the first L_n states are bitwise those without ends, and the tails follow the fill rule
    want = SC.filled(free[0].cpu().numpy(), free[1].cpu().numpy(), lens)
    assert np.array_equal(states.cpu().numpy(), want[0]) and np.array_equal(acts.cpu().numpy(), want[1])
    both = B.pairs.end_episodes(free[0], free[1], lengths)
    assert torch.equal(states, both[0]) and torch.equal(acts, both[1])


# ------------------------------------------------------------------ the grid stride
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', TASKS)
def test_workgroups_stride_over_more_episodes_than_the_grid_holds(B, task, dtype):
    """2 cap W + 5 episodes at T = 2 under a (3,) policy: every workgroup takes a second batch with the weights
    it staged once, some a third, the last one partly empty."""
    steps, ta = 2, 2
    arrays = _draws(task, steps)
    policy, _, _ = _policy(B, task, (3,), 'tanh')
    marks = PC.replace_marks(N_MAX, ta)
    small = _rollout(B, task, arrays, N_MAX, ta, steps, dtype, True, policy, marks)
    n = 2 * SC.GRID_CAP * SC.EPISODES + 5
    reps = -(-n // N_MAX)
    rep = lambda x: x.repeat(*([reps] + [1] * (x.dim() - 1)))[:n]      # noqa: E731
    params, init, actions = (rep(_dev(x)) for x in (arrays[0], arrays[1], arrays[2][:, :ta]))
    got = B.pairs.rollout(task, params, init, actions, n_steps=steps, terminate=True, dtype=dtype, policy=policy,
                          replace=rep(_dev(marks)))
    assert tuple(got[0].shape) == (n, steps + 1, SC.DIMS[task][2]) and tuple(got[2].shape) == (n,)
    assert all(torch.equal(x, rep(y)) for x, y in zip(got, small))


# ------------------------------------------------------------------ 6. rows, repeats and bounds
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', TASKS)
def test_bits_repeat_rows_permute_and_a_nan_stays_in_its_episode(B, task, dtype):
    steps, ta, n = 17, 18, N_MAX
    arrays = _draws(task, steps)
    policy, _, _ = _policy(B, task, (16,), 'tanh')
    marks = PC.replace_marks(n, ta)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    first = _rollout(B, task, arrays, n, ta, steps, dtype, True, policy, marks, nonfinite=flag)
    again = _rollout(B, task, arrays, n, ta, steps, dtype, True, policy, marks, nonfinite=flag)
    assert all(torch.equal(x, y) for x, y in zip(first, again)) and int(flag.item()) == 0
    perm = np.random.RandomState(7).permutation(n)
    moved = _rollout(B, task, tuple(x[perm] for x in arrays), n, ta, steps, dtype, True, policy, marks[perm])
    assert all(torch.equal(x[_dev(perm)], y) for x, y in zip(first, moved))
    fewer = _rollout(B, task, arrays, SC.EPISODES + 1, ta, steps, dtype, True, policy, marks[:SC.EPISODES + 1])
    assert all(torch.equal(x[:SC.EPISODES + 1], y) for x, y in zip(first, fewer))
    # a NaN in one episode's initial state: the flag, that episode, and nothing else
    for victim in (0, SC.EPISODES - 1, SC.EPISODES + 2, n - 1):
        init = arrays[1].copy()
        init[victim, 1] = np.nan
        flag.zero_()
        got = _rollout(B, task, (arrays[0], init, arrays[2]), n, ta, steps, dtype, True, policy, marks, nonfinite=flag)
        assert int(flag.item()) == 1
        keep = torch.arange(n, device=DEV) != victim
        assert all(torch.equal(x[keep], y[keep]) for x, y in zip(first, got))
        assert torch.isnan(got[0][victim]).any(dim=1).all()
    flag.zero_()
    quiet = _rollout(B, task, (arrays[0], init, arrays[2]), n, ta, steps, dtype, True, policy, marks)
    assert int(flag.item()) == 0 and torch.equal(torch.nan_to_num(quiet[0]), torch.nan_to_num(got[0]))


def test_nothing_is_written_beyond_the_outputs(B):
    """The C entry points on buffers with a guard band behind every output, at a T whose last block is partial,
    with the outputs on a 16-byte boundary and off one; the widest policy, so that the LDS limit is raised."""
    _lib = B._lib
    for task in TASKS:
        for hidden in ((PC.UNITS + 1,), (64, 64)):
            policy, _, _ = _policy(B, task, hidden, 'tanh')
            widths = hidden + (0, 0)
            for prec, dtype in ((_lib.F32, F32), (_lib.F64, F64)):
                n, steps, ta = SC.EPISODES + 3, SC.STEP_BLOCK + 2, 4
                sd = SC.DIMS[task][2]
                arrays = _draws(task, steps)
                params, init, actions = (_dev(x).to(dtype) for x in (arrays[0][:n], arrays[1][:n], arrays[2][:n, :ta]))
                marks = _dev(PC.replace_marks(n, ta))
                want = B.pairs.rollout(task, params, init, actions, n_steps=steps, terminate=True, dtype=dtype,
                                       policy=policy, replace=marks)
                sizes = (n * (steps + 1) * sd, n * (steps + 1), n)
                for shift in (0, 1):
                    bufs = [torch.full((size + 65,), -9.0, dtype=dtype, device=DEV) for size in sizes[:2]]
                    bufs.append(torch.full((n + 65,), -9, dtype=torch.int32, device=DEV))
                    prec.sim_rollout_policy(SC.TASK_IDS[task], _lib.ptr(params), _lib.ptr(init), _lib.ptr(actions),
                                            _lib.ptr(marks), _lib.ptr(policy.packed_on(DEV)), len(hidden), widths[0],
                                            widths[1], _lib.SIM_ACTIVATIONS['tanh'], _lib.ptr(bufs[0][shift:]),
                                            _lib.ptr(bufs[1][shift:]), _lib.ptr(bufs[2][shift:]), n, steps, ta, 1,
                                            None, _lib.stream())
                    for buf, size, ref in zip(bufs, sizes, want):
                        assert torch.equal(buf[shift:size + shift], ref.reshape(-1))
                        assert (buf[:shift] == -9).all() and (buf[size + shift:] == -9).all()


# ------------------------------------------------------------------ 7. end to end
def test_cartpole_pairs_under_the_balance_gains_train_an_estimator(B):
    pairs = B.pairs
    policy = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
    # the host path first: no episode ends
    host = pairs.cartpole_pairs(256, 50, policy=policy, frac_rnd=0.1, seed=0, terminate=True)
    assert (host[3] == 51).all()
    theta, states, actions, lengths = pairs.cartpole_pairs(256, 50, policy=policy, frac_rnd=0.1, seed=0, device=DEV,
                                                           terminate=True)
    assert all(x.device.type == 'cuda' for x in (theta, states, actions, lengths))
    assert theta.dtype == states.dtype == actions.dtype == F32 and lengths.dtype == torch.int32
    assert tuple(states.shape) == (256, 51, 4) and tuple(actions.shape) == (256, 51, 1)
    assert torch.equal(lengths.cpu(), host[3]) and torch.equal(theta.cpu(), host[0])
    assert torch.equal(states[:, 0].cpu(), host[1][:, 0])
    cfg = {'modelClass': 'MDNN', 'trainTrajLen': 51, 'components': 3, 'hiddenLayers': (16, 16), 'lr': 1e-3,
           'inputNorm': True, 'summarizerFxn': 'summary_sysid'}
    torch.manual_seed(11)
    bs = B.BayesSim(model_cfg=cfg, obs_dim=4, act_dim=1, params_dim=2, params_lows=np.array([0.1, 0.1]),
                    params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)
    np.random.seed(31), torch.manual_seed(32)
    logs = bs.fit(theta, states, actions)
    assert len(logs) >= 1
    for chunk in logs:
        for key in ('train_loss', 'test_loss'):
            assert len(chunk[key]) > 0 and np.isfinite(chunk[key]).all()
