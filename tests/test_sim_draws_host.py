"""CPU-side checks of the drawn rollouts (include/bsig_sim_draws.h, bayes_sim_ig_amd/pairs.py): ``philox4x32``
against the known answers, ``episode_draws`` against a one-counter-at-a-time restatement, its ranges, its
exact constants and the conditions on its distributions, every ValueError of ``EpisodeDraws``, ``rollout_drawn``
and ``draw_pairs``, the host path of ``rollout_drawn`` against ``_host_rollout`` on ``episode_draws``' arrays
(bitwise), an episode as a function of (seed, global index), the binding's table and every BSIG_EINVAL of the entry
points before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sim_cases as SC
import sim_draws_cases as DC
import sim_policy_cases as PC
from conftest import ROOT
from bayes_sim_ig_amd import _lib, pairs

F32, F64 = torch.float32, torch.float64
FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first


def _draws(task, seed=DC.SEED, first=0, frac=0.0, std=0.0, wide=False, **kw):
    return pairs.EpisodeDraws(seed, first, frac_rnd=frac, noise_std=std, **dict(DC.bounds(task, wide), **kw))


def _policy(task, hidden, activation='relu'):
    return pairs.MLPPolicy(*PC.make_policy(task, hidden), activation)


# ------------------------------------------------------------------ the generator
def test_philox_known_answers():
    for counter, key, want in DC.KNOWN_ANSWERS:
        got = pairs.philox4x32(np.array(counter, dtype=np.uint64), key)
        assert got.dtype == np.uint32 and got.tolist() == list(want)
    counters = np.array([k[0] for k in DC.KNOWN_ANSWERS], dtype=np.uint32).reshape(3, 1, 4)
    keys = tuple(np.array([k[1][i] for k in DC.KNOWN_ANSWERS]).reshape(3, 1) for i in range(2))
    assert pairs.philox4x32(counters, keys)[:, 0].tolist() == [list(k[2]) for k in DC.KNOWN_ANSWERS]
    for bad in (np.zeros(4), np.zeros((2, 3), dtype=np.uint32), np.array([0, 0, 0, 2 ** 32], dtype=np.uint64)):
        with pytest.raises(ValueError, match='counters'):
            pairs.philox4x32(bad, (0, 0))
    with pytest.raises(ValueError, match='key'):
        pairs.philox4x32(np.zeros(4, dtype=np.uint32), (0,))


def _philox_scalar(c, k):
    """One counter in Python integers, from the header's round."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize('task', DC.TASKS)
def test_episode_draws_is_the_definition_one_counter_at_a_time(task):
    n, steps, first = 5, 3, DC.FIRST + 67         # the global index crosses 2^32
    draws = _draws(task, first=first, frac=0.3, std=0.3)
    pd, idim, _ = SC.DIMS[task]
    for policy_on in (False, True):
        theta, init, explore, replace = pairs.episode_draws(task, draws, n, steps, policy_on, np.float64)
        assert theta.shape == (n, pd) and init.shape == (n, idim) and explore.shape == replace.shape == (n, steps)
        assert replace.dtype == np.uint8 and explore.dtype == np.float64
        key = (DC.SEED & 0xFFFFFFFF, DC.SEED >> 32)
        for i in range(n):
            g = first + i
            x = _philox_scalar((g & 0xFFFFFFFF, g >> 32, 0, 1), key)
            for c in range(pd):
                assert theta[i, c] == draws.lows[c] + ((draws.highs[c] - draws.lows[c]) * (x[c] * 2.0 ** -32))
            x = _philox_scalar((g & 0xFFFFFFFF, g >> 32, 0, 2), key)
            for c in range(idim):
                lo, hi = draws.init_lows[c], draws.init_highs[c]
                assert init[i, c] == lo + ((hi - lo) * (x[c] * 2.0 ** -32))
            for t in range(steps):
                x = _philox_scalar((g & 0xFFFFFFFF, g >> 32, t, 0), key)
                r = x[0] < draws.thresh or not policy_on
                v = -1.0 + (2.0 * (x[1] * 2.0 ** -32))
                z = np.sqrt(-2.0 * np.log((x[2] + 1) * 2.0 ** -32)) * np.cos(6.283185307179586 * (x[3] * 2.0 ** -32))
                assert replace[i, t] == r and explore[i, t] == (v if r else 0.3 * z)
        # float32: the doubles rounded once
        single = pairs.episode_draws(task, draws, n, steps, policy_on, np.float32)
        assert all(a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32))
                   for a, b in zip(single[:3], (theta, init, explore)))
        assert np.array_equal(single[3], replace)
        assert np.array_equal(pairs.episode_draws(task, draws, n, steps, policy_on, F32)[2], single[2])


def test_episode_draws_ranges_constants_and_switches():
    n, steps = 300, 40
    for task in DC.TASKS:
        b = DC.bounds(task)
        for dtype in (np.float64, np.float32):
            theta, init, explore, replace = pairs.episode_draws(task, _draws(task, frac=0.3, std=1.0), n, steps, True,
                                                                dtype)
            lo, hi = np.asarray(b['lows']), np.asarray(b['highs'])
            assert (theta >= lo.astype(dtype)).all() and (theta <= hi.astype(dtype)).all()
            ilo, ihi = np.asarray(b['init_lows']), np.asarray(b['init_highs'])
            assert (init >= ilo.astype(dtype)).all() and (init <= ihi.astype(dtype)).all()
            if task == 'cartpole':
                assert (theta[:, 2] == 1.0).all()                   # low == high is exact
            on = replace != 0
            assert set(np.unique(replace).tolist()) == {0, 1} and 0.2 < on.mean() < 0.4
            assert (explore[on] >= -1.0).all() and (explore[on] <= 1.0).all() and np.isfinite(explore).all()
            assert np.abs(explore[~on]).max() > 1.0                  # a Gaussian, not a uniform
    # low == high at values that are not fp32 numbers, in both types
    exact = pairs.EpisodeDraws(3, lows=(0.1, 1 / 3), highs=(0.1, 1 / 3), init_lows=(-0.7, 0.3), init_highs=(-0.7, 0.3),
                               act_low=0.25, act_high=0.25, frac_rnd=1.0)
    theta, init, explore, replace = pairs.episode_draws('pendulum', exact, 50, 9, True)
    assert (theta == np.array([0.1, 1 / 3])).all() and (init == np.array([-0.7, 0.3])).all()
    assert (explore == 0.25).all() and (replace == 1).all()
    # frac_rnd 0 never marks, 1 always; noise_std 0 leaves +0 where unmarked; no policy: all marked, v_t
    never = pairs.episode_draws('pendulum', _draws('pendulum', frac=0.0, std=0.0), 50, 9, True)
    assert (never[3] == 0).all() and (never[2] == 0).all() and not np.signbit(never[2]).any()
    always = pairs.episode_draws('pendulum', _draws('pendulum', frac=1.0, std=1.0), 50, 9, True)
    open_loop = pairs.episode_draws('pendulum', _draws('pendulum', frac=0.3, std=1.0), 50, 9, False)
    assert (always[3] == 1).all() and (open_loop[3] == 1).all() and np.array_equal(always[2], open_loop[2])
    # thresh
    assert [pairs.EpisodeDraws(0, frac_rnd=f).thresh for f in (0.0, 0.5, 1.0, 2.0 ** -33)] == [0, 2 ** 31, 2 ** 32, 0]
    # no bounds, no draw
    assert pairs.episode_draws('pendulum', pairs.EpisodeDraws(0), 4, 2)[:2] == (None, None)


def test_the_distributions_of_the_sanity_seed():
    """The conditions the GPU test asserts on the device's draws hold for the definition with that seed."""
    n, steps = 1024, DC.SANITY_N // 1024
    v = pairs.episode_draws('cartpole', _draws('cartpole', seed=DC.SANITY_SEED, frac=1.0), n, steps, True)[2]
    z = pairs.episode_draws('cartpole', _draws('cartpole', seed=DC.SANITY_SEED, std=1.0), n, steps, True)[2]
    r = pairs.episode_draws('cartpole', _draws('cartpole', seed=DC.SANITY_SEED, frac=DC.SANITY_FRAC), n, steps, True)[3]
    for name, (got, limit) in DC.sanity(v, z, r.astype(np.float64), -1.0, 1.0, DC.SANITY_FRAC).items():
        print('%s: %.3g <= %.3g' % (name, got, limit))
        assert got <= limit, name


# ------------------------------------------------------------------ every ValueError
def test_episode_draws_errors_name_the_argument():
    E = pairs.EpisodeDraws
    for name in ('seed', 'first_episode'):
        for bad in (-1, 2 ** 64, 1.5, True, None, 'x'):
            with pytest.raises(ValueError, match='^%s must be an int' % name):
                E(**dict({'seed': 0}, **{name: bad}))
        assert getattr(E(**dict({'seed': 0}, **{name: 2 ** 64 - 1})), name) == 2 ** 64 - 1
    for lo_name, hi_name, most in (('lows', 'highs', 3), ('init_lows', 'init_highs', 4)):
        ok = (0.0,) * most
        with pytest.raises(ValueError, match='%s and %s come together' % (lo_name, hi_name)):
            E(0, **{lo_name: ok})
        with pytest.raises(ValueError, match='%s and %s must both hold 1..%d bounds' % (lo_name, hi_name, most)):
            E(0, **{lo_name: ok, hi_name: ok[:-1]})
        with pytest.raises(ValueError, match='%s and %s must both hold 1..%d bounds' % (lo_name, hi_name, most)):
            E(0, **{lo_name: ok + (0.0,), hi_name: ok + (0.0,)})
        with pytest.raises(ValueError, match='^%s must be finite' % lo_name):
            E(0, **{lo_name: (np.nan,) + ok[1:], hi_name: ok})
        with pytest.raises(ValueError, match='^%s must be finite' % hi_name):
            E(0, **{lo_name: ok, hi_name: (np.inf,) + ok[1:]})
        with pytest.raises(ValueError, match='^%s must not exceed %s' % (lo_name, hi_name)):
            E(0, **{lo_name: (1.0,) + ok[1:], hi_name: ok})
        with pytest.raises(ValueError, match='%s and %s must be numbers' % (lo_name, hi_name)):
            E(0, **{lo_name: ('a',), hi_name: ('b',)})
    with pytest.raises(ValueError, match='^act_low must not exceed act_high'):
        E(0, act_low=1.0, act_high=-1.0)
    with pytest.raises(ValueError, match='^act_high must be finite'):
        E(0, act_high=np.inf)
    with pytest.raises(ValueError, match='^act_low must be finite'):
        E(0, act_low=np.nan)
    for bad in (-0.1, 1.1, np.nan):
        with pytest.raises(ValueError, match='^frac_rnd must lie in'):
            E(0, frac_rnd=bad)
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='^noise_std must be finite and >= 0'):
            E(0, noise_std=bad)
    with pytest.raises(ValueError, match='^noise_std must be a number'):
        E(0, noise_std='x')
    with pytest.raises(ValueError, match='^frac_rnd must be a number'):
        E(0, frac_rnd=None)


def test_rollout_drawn_and_draw_pairs_errors_come_before_any_launch():
    good = _draws('cartpole')

    def call(task='cartpole', n=4, steps=3, draws=good, **kw):
        return pairs.rollout_drawn(task, n, steps, draws, **kw)
    with pytest.raises(ValueError, match='task must be'):
        call(task='acrobot')
    with pytest.raises(ValueError, match='rollout_drawn stores'):
        call(dtype=torch.float16)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match='^n must be an int'):
            call(n=bad)
    for bad in (0, -1, 2.0, False, 2 ** 28):
        with pytest.raises(ValueError, match='^n_steps must be an int'):
            call(steps=bad)
    with pytest.raises(ValueError, match='draws must be an EpisodeDraws'):
        call(draws={'seed': 0})
    with pytest.raises(ValueError, match='terminate must be a bool'):
        call(terminate=1)
    with pytest.raises(ValueError, match='policy must be an MLPPolicy'):
        call(policy=torch.nn.Linear(4, 1))
    with pytest.raises(ValueError, match='policy takes 3 inputs, cartpole observes 4'):
        call(policy=pairs.linear_feedback((1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match='lows and highs must hold 2 bounds for pendulum, got 3'):
        call(task='pendulum')
    with pytest.raises(ValueError, match='init_lows and init_highs must hold 2 bounds for pendulum, got 4'):
        call(task='pendulum', params=torch.zeros(4, 2))
    with pytest.raises(ValueError, match='lows and highs are needed where no params is given'):
        call(draws=pairs.EpisodeDraws(0, init_lows=(0,) * 4, init_highs=(0,) * 4))
    with pytest.raises(ValueError, match='init_lows and init_highs are needed where no init is given'):
        call(draws=pairs.EpisodeDraws(0), params=torch.zeros(4, 3))
    for bad in (torch.zeros(4, 2), torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.int32), np.zeros((4, 3))):
        with pytest.raises(ValueError, match=r'^params must be a floating-point tensor \[4, 3\]'):
            call(params=bad)
    with pytest.raises(ValueError, match=r'^init must be a floating-point tensor \[4, 4\]'):
        call(init=torch.zeros(4, 3))
    with pytest.raises(ValueError, match='^params must live on cpu'):
        call(params=torch.zeros(4, 3, device='meta'))
    with pytest.raises(ValueError, match='nonfinite must be a 1-element int32 tensor'):
        call(nonfinite=torch.zeros(1))
    assert tuple(call(n=0)[2].shape) == (0, 4, 4)
    # draw_pairs
    with pytest.raises(ValueError, match='task must be'):
        pairs.draw_pairs('acrobot', 4, 3, 0)
    with pytest.raises(ValueError, match="policy must be 'random' or an MLPPolicy"):
        pairs.draw_pairs('cartpole', 4, 3, 0, policy='ones')
    with pytest.raises(ValueError, match='frac_rnd and noise_std belong to an MLPPolicy'):
        pairs.draw_pairs('cartpole', 4, 3, 0, frac_rnd=0.1)
    with pytest.raises(ValueError, match='lows and highs must both hold 2 bounds for pendulum'):
        pairs.draw_pairs('pendulum', 4, 3, 0, lows=(0.1,) * 3, highs=(1.0,) * 3)
    with pytest.raises(ValueError, match='lows and highs must both hold 2 or 3 bounds for cartpole'):
        pairs.draw_pairs('cartpole', 4, 3, 0, lows=(0.1,), highs=(1.0,))
    with pytest.raises(ValueError, match='^lows must not exceed highs'):
        pairs.draw_pairs('cartpole', 4, 3, 0, lows=(3.0, 0.1))
    with pytest.raises(ValueError, match='^seed must be an int'):
        pairs.draw_pairs('cartpole', 4, 3, -1)
    with pytest.raises(ValueError, match='^frac_rnd must lie in'):
        pairs.draw_pairs('cartpole', 4, 3, 0, policy=pairs.linear_feedback((1.0,) * 4), frac_rnd=2.0)
    with pytest.raises(ValueError, match='cart_mass must be a number'):
        pairs.draw_pairs('cartpole', 4, 3, 0, cart_mass='heavy')


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bsig_sim_draws.h')).read()
    define = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1))      # noqa: E731
    assert (define('BSIG_SIM_DRAW_STEP'), define('BSIG_SIM_DRAW_THETA'), define('BSIG_SIM_DRAW_INIT')) \
        == (_lib.SIM_DRAW_STEP, _lib.SIM_DRAW_THETA, _lib.SIM_DRAW_INIT) == (0, 1, 2)
    for word in ('D2511F53', 'CD9E8D57', '9E3779B9', 'BB67AE85'):
        assert word in header
    assert (pairs.PHILOX_M0, pairs.PHILOX_M1, pairs.PHILOX_W0, pairs.PHILOX_W1) \
        == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
    table = _lib.HEADERS['bsig_sim_draws.h']
    assert table['bsig_sim_rollout_drawn'] == table['bsig_sim_rollout_drawn_f64']
    assert _lib.F32.symbol('sim_rollout_drawn') == 'bsig_sim_rollout_drawn'
    assert _lib.F64.symbol('sim_rollout_drawn') == 'bsig_sim_rollout_drawn_f64'
    # the generator
    assert lib.bsig_philox4x32_10(None, 0, 0, None, 0, None) == _lib.BSIG_OK
    for args, word in (((FAKE, 0, 0, FAKE, -1, None), 'bad n'), ((None, 0, 0, FAKE, 1, None), 'null counters'),
                       ((FAKE, 0, 0, None, 1, None), 'null counters or out'),
                       ((C.c_void_p(4100), 0, 0, FAKE, 1, None), '16 bytes')):
        assert lib.bsig_philox4x32_10(*args) == _lib.BSIG_EINVAL, word
        assert word in lib.bsig_last_error().decode()
    # the drawn rollouts
    dbl = lambda *v: (C.c_double * len(v))(*v)      # noqa: E731
    nan, inf = float('nan'), float('inf')
    for fn in (lib.bsig_sim_rollout_drawn, lib.bsig_sim_rollout_drawn_f64):
        def call(task=1, params=None, init=None, lows=dbl(0, 0, 1), highs=dbl(1, 1, 1), ilows=dbl(0, 0, 0, 0),
                 ihighs=dbl(1, 1, 1, 1), act=(-1.0, 1.0), frac=0.3, std=0.5, policy=FAKE, nh=2, h0=8, h1=8, fn_act=1,
                 params_out=FAKE, init_out=FAKE, states=FAKE, actions_out=FAKE, lengths=FAKE, explore=None,
                 replace=None, n=3, steps=4, terminate=0):
            return fn(task, params, init, lows, highs, ilows, ihighs, act[0], act[1], frac, std, 7, 2 ** 63, policy,
                      nh, h0, h1, fn_act, params_out, init_out, states, actions_out, lengths, explore, replace, n,
                      steps, terminate, None, None)
        assert call(n=0) == _lib.BSIG_OK
        assert call(n=0, states=None, lows=None) == _lib.BSIG_OK
        cases = [(dict(task=2), 'unknown task 2'), (dict(steps=0), 'T 0'), (dict(terminate=2), 'terminate 2'),
                 (dict(n=-1), 'bad n'),
                 (dict(nh=3), 'n_hidden 3'), (dict(nh=-1), 'n_hidden -1'), (dict(h0=0), 'h0 0'), (dict(h0=65), 'h0 65'),
                 (dict(h1=0), 'h1 0'), (dict(h1=65), 'h1 65'), (dict(fn_act=3), 'unknown activation 3'),
                 (dict(fn_act=-1), 'unknown activation -1'),
                 (dict(lows=None), 'null lows or highs'), (dict(highs=None), 'null lows or highs'),
                 (dict(ilows=None), 'null init_lows or init_highs'), (dict(ihighs=None), 'null init_lows or init_highs'),
                 (dict(lows=dbl(0, nan, 1)), 'lows and highs must be finite'),
                 (dict(highs=dbl(1, inf, 1)), 'lows and highs must be finite'),
                 (dict(lows=dbl(0, 2, 1)), 'lows and highs must be finite with low <= high'),
                 (dict(ilows=dbl(0, 0, 0, -inf)), 'init_lows and init_highs must be finite'),
                 (dict(ihighs=dbl(1, 1, -1, 1)), 'init_lows and init_highs must be finite with low <= high'),
                 (dict(act=(nan, 1.0)), 'act_low'), (dict(act=(-1.0, inf)), 'act_high'),
                 (dict(act=(1.0, -1.0)), 'act_low 1 and act_high -1'),
                 (dict(frac=-0.1), 'frac_rnd -0.1 outside'), (dict(frac=1.5), 'frac_rnd 1.5 outside'),
                 (dict(frac=nan), 'frac_rnd nan outside'),
                 (dict(std=-1.0), 'noise_std -1 is negative'), (dict(std=inf), 'noise_std inf is negative or not finite'),
                 (dict(std=nan), 'noise_std nan'),
                 (dict(params_out=None), 'null params_out'), (dict(init_out=None), 'null init_out'),
                 (dict(states=None), 'null states'), (dict(actions_out=None), 'null actions_out'),
                 (dict(lengths=None), 'null lengths')]
        for kw, word in cases:
            assert call(**kw) == _lib.BSIG_EINVAL, kw
            assert word in lib.bsig_last_error().decode(), (kw, lib.bsig_last_error().decode())
        # without a policy its arguments are not read; bounds of a draw that is not made are not read
        for kw in (dict(policy=None, nh=9, steps=0), dict(params=FAKE, lows=None, highs=None, steps=0),
                   dict(init=FAKE, ilows=None, ihighs=dbl(nan, 0, 0, 0), steps=0)):
            assert call(**kw) == _lib.BSIG_EINVAL
            assert 'T 0' in lib.bsig_last_error().decode(), kw


# ------------------------------------------------------------------ the host path of rollout_drawn
@pytest.mark.parametrize('task', DC.TASKS)
@pytest.mark.parametrize('hidden', DC.HIDDEN, ids=DC.hidden_id)
def test_host_rollout_drawn_is_host_rollout_on_episode_draws(task, hidden):
    policy = None if hidden is None else _policy(task, hidden)
    for i, (n, steps) in enumerate(zip(DC.COUNTS, DC.STEPS)):
        frac, std, terminate = DC.FRACS[i % 3], DC.STDS[(i + 1) % 3], bool(i % 2)
        draws = _draws(task, first=DC.FIRST, frac=frac, std=std, wide=True)
        for dtype, store in ((F64, np.float64), (F32, np.float32)):
            theta, init, explore, replace = pairs.episode_draws(task, draws, n, steps, policy is not None, store)
            want = pairs._host_rollout(task, theta.astype(np.float64), init.astype(np.float64),
                                       explore.astype(np.float64)[:, :, None], steps, terminate, policy,
                                       replace if policy is not None else None)
            got = pairs.rollout_drawn(task, n, steps, draws, policy=policy, terminate=terminate, dtype=dtype, record=True)
            assert len(got) == 7 and [x.dtype for x in got] == [dtype] * 4 + [torch.int32, dtype, torch.uint8]
            assert np.array_equal(got[0].numpy(), theta) and np.array_equal(got[1].numpy(), init)
            assert np.array_equal(got[2].numpy(), want[0].astype(store))
            assert np.array_equal(got[3].numpy(), want[1].astype(store)) and np.array_equal(got[4].numpy(), want[2])
            live = np.arange(steps)[None, :] < want[2][:, None] - 1
            assert np.array_equal(got[5].numpy()[live], explore[live]) and (got[5].numpy()[~live] == 0).all()
            assert np.array_equal(got[6].numpy()[live], replace[live]) and (got[6].numpy()[~live] == 0).all()
            # the existing entry point fed the recordings is the same rollout
            fed = pairs.rollout(task, got[0], got[1], got[5][:, :, None], n_steps=steps, terminate=terminate,
                                dtype=dtype, policy=policy, replace=got[6] if policy is not None else None)
            assert all(torch.equal(a, b) for a, b in zip(fed, got[2:5]))
            plain = pairs.rollout_drawn(task, n, steps, draws, policy=policy, terminate=terminate, dtype=dtype)
            assert len(plain) == 5 and all(torch.equal(a, b) for a, b in zip(plain, got))


def test_host_episodes_are_functions_of_seed_and_global_index_and_given_arrays_are_used():
    task, steps = 'cartpole', 9
    policy = _policy(task, (5,))
    kw = dict(policy=policy, terminate=True, dtype=F64, record=True)
    whole = pairs.rollout_drawn(task, 194, steps, _draws(task, first=DC.FIRST, frac=0.3, std=0.3, wide=True), **kw)
    head = pairs.rollout_drawn(task, 64, steps, _draws(task, first=DC.FIRST, frac=0.3, std=0.3, wide=True), **kw)
    tail = pairs.rollout_drawn(task, 130, steps, _draws(task, first=DC.FIRST + 64, frac=0.3, std=0.3, wide=True), **kw)
    assert all(torch.equal(w, torch.cat([h, t])) for w, h, t in zip(whole, head, tail))
    assert len(set(whole[4].tolist())) > 3
    for other in (dict(seed=DC.SEED ^ 1), dict(seed=DC.SEED ^ (1 << 32)), dict(first=DC.FIRST + 1)):
        moved = pairs.rollout_drawn(task, 194, steps, _draws(task, **dict(dict(first=DC.FIRST, frac=0.3, std=0.3,
                                                                            wide=True), **other)), **kw)
        assert not any(torch.equal(a, b) for a, b in zip(whole[:4], moved[:4]))
    # given params and / or init: used verbatim, the other still drawn as before
    params, init, _ = (torch.from_numpy(x) for x in SC.draws(task, 194, 1, seed=3, wide=True))
    draws = _draws(task, first=DC.FIRST, frac=0.3, std=0.3, wide=True)
    for given in (dict(params=params), dict(init=init), dict(params=params, init=init)):
        got = pairs.rollout_drawn(task, 194, steps, draws, **dict(kw, **given))
        assert torch.equal(got[0], params.double() if 'params' in given else whole[0])
        assert torch.equal(got[1], init.double() if 'init' in given else whole[1])
        assert torch.equal(got[5][:, 0], whole[5][:, 0]) and not torch.equal(got[2], whole[2])
    none = pairs.EpisodeDraws(DC.SEED, DC.FIRST, frac_rnd=0.3, noise_std=0.3)
    got = pairs.rollout_drawn(task, 194, steps, none, **dict(kw, params=params, init=init))
    assert torch.equal(got[0], params.double()) and torch.equal(got[1], init.double())


def test_draw_pairs_on_the_host():
    for task, sd in (('pendulum', 3), ('cartpole', 4)):
        theta, states, actions = pairs.draw_pairs(task, 70, 12, seed=5)
        assert theta.dtype == states.dtype == actions.dtype == F32
        assert tuple(theta.shape) == (70, 2) and tuple(states.shape) == (70, 13, sd) and tuple(actions.shape) == (70, 13, 1)
        lo, hi = (0.0, 1.0) if task == 'pendulum' else (-1.0, 1.0)
        assert float(actions.min()) >= lo and float(actions.max()) <= hi and float(actions.min()) < lo + 0.05
        assert torch.equal(actions[:, 12], actions[:, 11])
        low = 0.01 if task == 'pendulum' else 0.1
        assert float(theta.min()) >= np.float32(low) and float(theta.max()) <= 2.0
        # shards: the second half by its first_episode
        part = pairs.draw_pairs(task, 35, 12, seed=5, first_episode=35)
        assert all(torch.equal(a[35:], b) for a, b in zip((theta, states, actions), part))
    out = pairs.draw_pairs('cartpole', 300, 50, seed=0, terminate=True)
    assert len(out) == 4 and out[3].dtype == torch.int32 and int((out[3] < 51).sum()) > 150
    assert torch.equal(out[1][:, 0].abs().max(dim=1).values <= 0.05, torch.ones(300, dtype=torch.bool))
    three = pairs.draw_pairs('cartpole', 20, 5, seed=0, lows=(0.1, 0.1, 0.5), highs=(2.0, 2.0, 1.5))
    assert tuple(three[0].shape) == (20, 3) and float(three[0][:, 2].min()) >= 0.5
    heavy = pairs.draw_pairs('cartpole', 20, 5, seed=0, cart_mass=3.0)
    assert torch.equal(heavy[0], out[0][:20]) and not torch.equal(heavy[1], out[1][:20, :6])
    policy = pairs.linear_feedback(pairs.CARTPOLE_BALANCE_GAINS)
    held = pairs.draw_pairs('cartpole', 256, 50, seed=0, policy=policy, frac_rnd=0.1, terminate=True)
    assert (held[3] == 51).all()
