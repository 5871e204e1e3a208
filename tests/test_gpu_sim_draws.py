"""GPU checks of the drawn rollouts (include/bsig_sim_draws.h, csrc/sim.h with csrc/sim_draws.h) through
``pairs.rollout_drawn`` and ``pairs.draw_pairs`` on a GPU, and of the generator through ``bsig_philox4x32_10``.

What is compared with: ``pairs.episode_draws`` (the definition in numpy, which tests/test_sim_draws_host.py holds
against a one-counter-at-a-time restatement) for the draws -- bitwise but for the Gaussian entries, which are held
to the bound tests/sim_draws_cases.py derives -- and the kernel's OWN outputs for the rest: the existing entry
points fed a drawn launch's recordings (bitwise), the fp32 launch against the double one, the launch without
ends, other launches of the same global episodes.  Whole trajectories are never compared with the host path.

The shapes: sim_draws_cases.case_grid() -- N around one wavefront, T around the 8-step staging block, both tasks,
fp32 and double, no policy and the policies (), (5,), (16, 4) under the identity and relu, frac_rnd in (0, 0.3, 1),
noise_std in (0, 1, 0.3), terminate on and off."""
import numpy as np
import pytest
import torch

import sim_cases as SC
import sim_draws_cases as DC
import sim_policy_cases as PC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


def _draws(B, task, seed=DC.SEED, first=DC.FIRST, frac=0.0, std=0.0, wide=True):
    return B.pairs.EpisodeDraws(seed, first, frac_rnd=frac, noise_std=std, **DC.bounds(task, wide))


def _policy(B, task, hidden, activation):
    if hidden is None:
        return None
    return B.pairs.MLPPolicy(*PC.make_policy(task, hidden), activation).to(DEV)


def _drawn(B, task, n, steps, draws, policy, terminate, dtype, **kw):
    out = B.pairs.rollout_drawn(task, n, steps, draws, policy=policy, terminate=terminate, dtype=dtype, device=DEV,
                                record=True, **kw)
    pd, idim, sd = SC.DIMS[task]
    shapes = ((n, pd), (n, idim), (n, steps + 1, sd), (n, steps + 1, 1), (n,), (n, steps), (n, steps))
    assert [tuple(x.shape) for x in out] == list(shapes)
    assert [x.dtype for x in out] == [dtype] * 4 + [torch.int32, dtype, torch.uint8]
    assert all(x.device.type == 'cuda' and x.is_contiguous() for x in out)
    return out


# ------------------------------------------------------------------ (a) the generator
def test_philox_on_the_device(B):
    lib = B._lib.load()

    def device_words(counters, key):
        packed = torch.from_numpy(counters.astype(np.uint32).view(np.int32)).to(DEV).contiguous()
        out = torch.full_like(packed, -1)
        B._lib.check(lib.bsig_philox4x32_10(B._lib.ptr(packed), key[0], key[1], B._lib.ptr(out), packed.shape[0],
                                            B._lib.stream()))
        return out.cpu().numpy().view(np.uint32)
    for counter, key, want in DC.KNOWN_ANSWERS:
        got = device_words(np.array([counter], dtype=np.uint64), key)
        assert got.tolist() == [list(want)], ['%08x' % x for x in got[0]]
    rs = np.random.RandomState(11)
    counters = rs.randint(0, 2 ** 32, size=(4096, 4), dtype=np.uint64)
    key = (int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(0, 2 ** 32, dtype=np.uint64)))
    assert np.array_equal(device_words(counters, key), B.pairs.philox4x32(counters, key))


# ------------------------------------------------------------------ (b) the draws, (c) the equivalence
@pytest.mark.parametrize('task', DC.TASKS)
@pytest.mark.parametrize('hidden', DC.HIDDEN, ids=DC.hidden_id)
def test_draws_are_the_definition_and_the_launch_is_the_existing_one_on_them(B, task, hidden):
    pairs = B.pairs
    worst, count, ended = 0.0, 0, 0
    for case in DC.case_grid():
        if case[0] != task or case[1] != hidden:
            continue
        _, _, activation, n, steps, frac, std, terminate = case
        policy = _policy(B, task, hidden, activation)
        draws = _draws(B, task, frac=frac, std=std)
        d64 = _drawn(B, task, n, steps, draws, policy, terminate, F64)
        d32 = _drawn(B, task, n, steps, draws, policy, terminate, F32)
        lens = d64[4].cpu().numpy()
        ended += int((lens < steps + 1).sum())
        drawn = lambda out: np.arange(steps)[None, :] < out[4].cpu().numpy()[:, None] - 1      # noqa: E731
        for out, store in ((d64, np.float64), (d32, np.float32)):
            theta, init, explore, replace = pairs.episode_draws(task, draws, n, steps, policy is not None, store)
            got_e, got_r = out[5].cpu().numpy(), out[6].cpu().numpy()
            live = drawn(out)                # the steps this launch drew: an ended episode draws nothing more
            # (b) theta, the initial state, the marks and the uniform entries: bitwise
            assert np.array_equal(out[0].cpu().numpy(), theta) and np.array_equal(out[1].cpu().numpy(), init)
            assert np.array_equal(got_r[live], replace[live]) and (got_r[~live] == 0).all()
            assert (got_e[~live] == 0).all() and not np.signbit(got_e[~live]).any()
            uniform = live & (replace != 0)
            assert np.array_equal(got_e[uniform], explore[uniform])
            gauss = live & (replace == 0)
            if std == 0.0:
                assert (got_e[gauss] == 0).all() and not np.signbit(got_e[gauss]).any()
            elif store is np.float64 and gauss.any():
                limit = DC.GAUSS_ULPS * 2.0 ** -52 * np.abs(explore[gauss])
                err = np.abs(got_e[gauss] - explore[gauss])
                worst = max(worst, float((err / np.maximum(limit, 1e-300)).max()))
                assert (err <= limit).all()
        # (b) the fp32 launch's recordings are the double launch's rounded once (where both episodes live)
        both = torch.from_numpy(drawn(d32) & drawn(d64)).to(DEV)
        assert torch.equal(d32[5][both], d64[5].float()[both]) and torch.equal(d32[6][both], d64[6][both])
        assert torch.equal(d32[0], d64[0].float()) and torch.equal(d32[1], d64[1].float())
        # (c) the existing entry point fed the launch's own recordings: bitwise, in either type
        for out, dtype in ((d64, F64), (d32, F32)):
            fed = pairs.rollout(task, out[0], out[1], out[5][:, :, None], n_steps=steps, terminate=terminate,
                                dtype=dtype, policy=policy, replace=out[6] if policy is not None else None)
            assert torch.equal(fed[0], out[2]) and torch.equal(fed[1], out[3]) and torch.equal(fed[2], out[4])
            assert torch.isfinite(out[2]).all()
        # (c) the first lengths[n] states are those of the launch without ends
        if terminate:
            free = _drawn(B, task, n, steps, draws, policy, False, F64)
            assert (free[4] == steps + 1).all()
            want = SC.filled(free[2].cpu().numpy(), free[3].cpu().numpy(), lens)
            assert np.array_equal(d64[2].cpu().numpy(), want[0]) and np.array_equal(d64[3].cpu().numpy(), want[1])
            assert np.array_equal(lens, SC.lengths_by_scan(task, d64[2].cpu().numpy()))
        count += 1
    print('%s %s: %d cases, %d episodes ended early, worst Gaussian |device - numpy| / bound %.3g'
          % (task, DC.hidden_id(hidden), count, ended, worst))
    assert count >= 12 and (task == 'pendulum' or ended > 0)


# ------------------------------------------------------------------ (d) a function of (seed, global index)
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', DC.TASKS)
def test_an_episode_is_a_function_of_seed_and_global_index(B, task, dtype):
    steps = 17
    for hidden in (None, (16, 4)):
        policy = _policy(B, task, hidden, 'relu')
        kw = dict(frac=0.3, std=0.3)
        whole = _drawn(B, task, 194, steps, _draws(B, task, **kw), policy, True, dtype)
        again = _drawn(B, task, 194, steps, _draws(B, task, **kw), policy, True, dtype)
        assert all(torch.equal(a, b) for a, b in zip(whole, again))
        head = _drawn(B, task, 64, steps, _draws(B, task, **kw), policy, True, dtype)
        tail = _drawn(B, task, 130, steps, _draws(B, task, first=DC.FIRST + 64, **kw), policy, True, dtype)
        assert all(torch.equal(w, torch.cat([h, t])) for w, h, t in zip(whole, head, tail))
        for other in (dict(seed=DC.SEED ^ 1), dict(seed=DC.SEED ^ (1 << 32)), dict(first=DC.FIRST + 1),
                      dict(first=DC.FIRST + 2 ** 32)):
            moved = _drawn(B, task, 194, steps, _draws(B, task, **dict(kw, **other)), policy, True, dtype)
            assert not any(torch.equal(a, b) for a, b in zip(whole[:4], moved[:4])), other
            assert not torch.equal(whole[5], moved[5])
        # record=False is the same launch without the recordings
        plain = B.pairs.rollout_drawn(task, 194, steps, _draws(B, task, **kw), policy=policy, terminate=True,
                                      dtype=dtype, device=DEV)
        assert len(plain) == 5 and all(torch.equal(a, b) for a, b in zip(plain, whole))


# ------------------------------------------------------------------ (e) given params and init
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', DC.TASKS)
def test_given_params_and_init_are_used_verbatim(B, task, dtype):
    n, steps = 65, 9
    policy = _policy(B, task, (5,), 'identity')
    draws = _draws(B, task, frac=0.3, std=1.0)
    whole = _drawn(B, task, n, steps, draws, policy, False, dtype)
    params, init, _ = (torch.from_numpy(x).to(DEV) for x in SC.draws(task, n, 1, seed=3, wide=True))
    for given in (dict(params=params), dict(init=init), dict(params=params, init=init)):
        got = _drawn(B, task, n, steps, draws, policy, False, dtype, **given)
        assert torch.equal(got[0], params.to(dtype) if 'params' in given else whole[0])
        assert torch.equal(got[1], init.to(dtype) if 'init' in given else whole[1])
        assert torch.equal(got[5], whole[5]) and torch.equal(got[6], whole[6])
        fed = B.pairs.rollout(task, got[0], got[1], got[5][:, :, None], n_steps=steps, dtype=dtype, policy=policy,
                              replace=got[6])
        assert torch.equal(fed[0], got[2]) and torch.equal(fed[1], got[3])
        assert not torch.equal(got[2], whole[2])
    bare = B.pairs.EpisodeDraws(DC.SEED, DC.FIRST, frac_rnd=0.3, noise_std=1.0)
    got = _drawn(B, task, n, steps, bare, policy, False, dtype, params=params, init=init)
    assert torch.equal(got[0], params.to(dtype)) and torch.equal(got[1], init.to(dtype))
    # a NaN in a given initial state: the flag, and that episode alone
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = _drawn(B, task, n, steps, draws, policy, False, dtype, init=init, nonfinite=flag)
    assert int(flag.item()) == 0
    broken = init.clone()
    broken[7, 1] = float('nan')
    got = _drawn(B, task, n, steps, draws, policy, False, dtype, init=broken, nonfinite=flag)
    keep = torch.arange(n, device=DEV) != 7
    assert int(flag.item()) == 1 and torch.equal(got[2][keep], ok[2][keep]) and torch.isnan(got[2][7]).any()


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('task', DC.TASKS)
def test_the_widest_policy_under_the_draws(B, task, dtype):
    """(64, 64), the policy's maximum widths: the dynamic LDS is above 64 KB, so the drawn instantiation raises its
    own limit, on top of the static rows the recordings add.  Two workgroups, the second partly empty; a last step
    block of two states."""
    n, steps = SC.EPISODES + 1, SC.STEP_BLOCK + 1
    for activation in DC.EXACT_ACTIVATIONS:
        policy = _policy(B, task, (PC.MAX_WIDTH, PC.MAX_WIDTH), activation)
        draws = _draws(B, task, frac=0.3, std=0.3)
        got = _drawn(B, task, n, steps, draws, policy, True, dtype)
        theta, init, explore, replace = B.pairs.episode_draws(task, draws, n, steps, True, got[0].cpu().numpy().dtype)
        assert np.array_equal(got[0].cpu().numpy(), theta) and np.array_equal(got[1].cpu().numpy(), init)
        live = np.arange(steps)[None, :] < got[4].cpu().numpy()[:, None] - 1
        assert np.array_equal(got[6].cpu().numpy()[live], replace[live])
        uniform = live & (replace != 0)
        assert np.array_equal(got[5].cpu().numpy()[uniform], explore[uniform])
        fed = B.pairs.rollout(task, got[0], got[1], got[5][:, :, None], n_steps=steps, terminate=True, dtype=dtype,
                              policy=policy, replace=got[6])
        assert torch.equal(fed[0], got[2]) and torch.equal(fed[1], got[3]) and torch.equal(fed[2], got[4])
        assert torch.isfinite(got[2]).all()
        tail = _drawn(B, task, 1, steps, _draws(B, task, first=DC.FIRST + n - 1, frac=0.3, std=0.3), policy, True, dtype)
        assert all(torch.equal(a[n - 1:], b) for a, b in zip(got, tail))


def test_nothing_is_written_beyond_the_outputs(B):
    """The C entry points on buffers with a guard band behind every output, at a T whose last block is partial,
    with the outputs on a 16-byte boundary and off one."""
    _lib = B._lib
    dbl = lambda v: (_lib.f64 * len(v))(*v)      # noqa: E731
    for task in DC.TASKS:
        for hidden in (None, (16, 4)):
            policy = _policy(B, task, hidden, 'relu')
            widths = (hidden or ()) + (0, 0)
            for prec, dtype in ((_lib.F32, F32), (_lib.F64, F64)):
                for steps in (SC.STEP_BLOCK + 2, 2 * SC.STEP_BLOCK):
                    n = SC.EPISODES + 3
                    pd, idim, sd = SC.DIMS[task]
                    draws = _draws(B, task, frac=0.3, std=0.3)
                    want = _drawn(B, task, n, steps, draws, policy, True, dtype)
                    sizes = (n * pd, n * idim, n * (steps + 1) * sd, n * (steps + 1), n, n * steps, n * steps)
                    kinds = [dtype] * 4 + [torch.int32, dtype, torch.uint8]
                    for shift in (0, 1):
                        bufs = [torch.full((size + 65,), 9, dtype=kind, device=DEV) for size, kind in zip(sizes, kinds)]
                        ptrs = [_lib.ptr(buf[shift:]) for buf in bufs]
                        prec.sim_rollout_drawn(SC.TASK_IDS[task], None, None, dbl(draws.lows), dbl(draws.highs),
                                               dbl(draws.init_lows), dbl(draws.init_highs), draws.act_low,
                                               draws.act_high, draws.frac_rnd, draws.noise_std, draws.seed,
                                               draws.first_episode,
                                               None if policy is None else _lib.ptr(policy.packed_on(DEV)),
                                               len(widths) - 2, widths[0], widths[1], _lib.SIM_ACTIVATIONS['relu'],
                                               *ptrs, n, steps, 1, None, _lib.stream())
                        for buf, size, ref in zip(bufs, sizes, want):
                            assert torch.equal(buf[shift:size + shift], ref.reshape(-1))
                            assert (buf[:shift] == 9).all() and (buf[size + shift:] == 9).all()


# ------------------------------------------------------------------ (f) the distributions
def test_the_distributions_of_the_device_draws(B):
    n, steps = 1024, DC.SANITY_N // 1024
    policy = _policy(B, 'cartpole', (), 'identity')

    def recorded(**kw):
        draws = _draws(B, 'cartpole', seed=DC.SANITY_SEED, first=0, wide=False, **kw)
        return _drawn(B, 'cartpole', n, steps, draws, policy, False, F64)
    v = recorded(frac=1.0)[5].cpu().numpy()
    z = recorded(std=1.0)[5].cpu().numpy()
    r = recorded(frac=DC.SANITY_FRAC)[6].cpu().numpy().astype(np.float64)
    for name, (got, limit) in DC.sanity(v, z, r, -1.0, 1.0, DC.SANITY_FRAC).items():
        print('%s: %.3g <= %.3g' % (name, got, limit))
        assert got <= limit, name


# ------------------------------------------------------------------ (g) draw_pairs on the device and on the host
@pytest.mark.parametrize('task', DC.TASKS)
def test_draw_pairs_on_the_device_against_the_host(B, task):
    pairs = B.pairs
    n, steps = 194, 17
    dev = pairs.draw_pairs(task, n, steps, seed=5, terminate=True, first_episode=DC.FIRST, device=DEV)
    host = pairs.draw_pairs(task, n, steps, seed=5, terminate=True, first_episode=DC.FIRST)
    assert len(dev) == 4 and all(x.device.type == 'cuda' for x in dev)
    assert [x.dtype for x in dev] == [F32, F32, F32, torch.int32]
    assert tuple(dev[0].shape) == (n, 2) and tuple(dev[1].shape) == (n, steps + 1, SC.DIMS[task][2])
    # theta and the open-loop actions: bitwise (an ended episode repeats its last action: compare the steps taken)
    assert torch.equal(dev[0].cpu(), host[0])
    taken = torch.arange(steps + 1)[None, :] < torch.minimum(dev[3].cpu(), host[3])[:, None] - 1
    assert torch.equal(dev[2].cpu()[:, :, 0][taken], host[2][:, :, 0][taken])
    if task == 'cartpole':
        assert torch.equal(dev[1][:, 0].cpu(), host[1][:, 0])
    # the states: the step-by-step criterion of sim_cases on the double launch of the same episodes
    d_lows, d_highs, init_lows, init_highs, act_low, act_high = pairs._DRAW_PAIRS[task]
    lows, highs = (d_lows + (1.0,), d_highs + (1.0,)) if task == 'cartpole' else (d_lows, d_highs)
    draws = pairs.EpisodeDraws(5, DC.FIRST, lows, highs, init_lows, init_highs, act_low, act_high)
    d64 = _drawn(B, task, n, steps, draws, None, True, F64)
    h64 = pairs.rollout_drawn(task, n, steps, draws, terminate=True, dtype=F64, record=True)
    assert torch.equal(d64[0].cpu(), h64[0]) and torch.equal(d64[1].cpu(), h64[1])
    worst = SC.step_check(task, d64[0].cpu().numpy(), d64[1].cpu().numpy(), d64[5].cpu().numpy()[:, :, None],
                          d64[2].cpu().numpy(), d64[4].cpu().numpy())
    print('%s: worst |kernel - numpy step| / bound: %s' % (task, worst))
    assert all(q <= 1.0 for q in worst.values()), worst
    # closed loop: the same contract
    if task == 'cartpole':
        policy = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
        held = pairs.draw_pairs(task, 256, 50, seed=0, policy=policy, frac_rnd=0.1, terminate=True, device=DEV)
        assert (held[3] == 51).all() and tuple(held[2].shape) == (256, 51, 1)


# ------------------------------------------------------------------ (h) end to end
def test_draw_pairs_train_an_estimator(B):
    theta, states, actions, lengths = B.pairs.draw_pairs('cartpole', 2000, 20, seed=0, terminate=True, device=DEV)
    assert int(lengths.min()) >= 2 and int((lengths < 21).sum()) > 0
    cfg = {'modelClass': 'MDNN', 'trainTrajLen': 21, 'components': 3, 'hiddenLayers': (16, 16), 'lr': 1e-3,
           'inputNorm': True, 'summarizerFxn': 'summary_xcorr', 'xcorrLags': 4}
    torch.manual_seed(11)
    bs = B.BayesSim(model_cfg=cfg, obs_dim=4, act_dim=1, params_dim=2, params_lows=np.array([0.1, 0.1]),
                    params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)
    np.random.seed(31), torch.manual_seed(32)
    logs = bs.fit(theta, states, actions, traj_lengths=lengths)
    assert len(logs) >= 1
    for chunk in logs:
        for key in ('train_loss', 'test_loss'):
            assert len(chunk[key]) > 0 and np.isfinite(chunk[key]).all()
    i = int(torch.nonzero(lengths < 21)[0])
    mog = bs.predict(states[i:i + 1], actions[i:i + 1], lengths=[int(lengths[i])])
    assert isinstance(mog, B.pdf.MoG) and np.isfinite(mog.a).all() and abs(float(np.sum(mog.a)) - 1.0) <= 1e-6
    assert np.isfinite(mog.eval(theta[:8].cpu().numpy().astype(np.float64))).all()
