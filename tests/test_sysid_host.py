"""CPU-side checks of the least-squares dynamics summary (include/bsig_sysid.h): the width, the cover and the
group queries are host arithmetic; every argument check of the launch entry points comes before any launch; the
Python mirror validates ``ridge`` and the shapes before it asks for a GPU; BayesSim sizes its first layer by
``sysid_dim`` and validates its one key.  And the yardstick of tests/sysid_cases.py itself: the fp64 reference
against a literal least-squares solve, the bound small enough on every case to prove something, and the kernel's
own form restated in fp32 numpy inside it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import sysid_cases as SC
from bayes_sim_ig_amd import _lib, summarizers
from bayes_sim_ig_amd.summarizer_table import SUMMARIZERS

FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_sysid', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsig_last_error().decode()


@functools.lru_cache(maxsize=None)
def _case(name):
    n, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    states, actions = SC.trajectories(n or 5, ts, ta, sd, ad)
    return states, actions, SC.reference(states, actions, ridge), SC.bounds(states, actions, ridge, SC.U32)


# ------------------------------------------------------------------ the binding
def test_the_headers_table_and_the_seam(lib):
    assert sorted(_lib.HEADERS['bsig_sysid.h']) == ['bsig_sysid', 'bsig_sysid_dim', 'bsig_sysid_f64',
                                                    'bsig_sysid_fits', 'bsig_sysid_group']
    assert _lib.Precision.OPS['sysid'] == ('bsig_sysid', 'bsig_sysid_f64')
    assert _lib.HEADERS['bsig_sysid.h']['bsig_sysid'] == _lib.HEADERS['bsig_sysid.h']['bsig_sysid_f64']
    assert _lib.HEADERS['bsig_sysid.h']['bsig_sysid'][1][8] is C.c_double          # the ridge, in both


@pytest.mark.parametrize('sd,ad,want', [(3, 1, 18), (60, 8, 4200), (211, 20, 49163), (1, 1, 4), (7, 3, 84)])
def test_width_is_the_closed_form(lib, sd, ad, want):
    assert SC.width(sd, ad) == want == (1 + sd + ad) * sd + sd
    assert lib.bsig_sysid_dim(sd, ad) == want
    assert summarizers.sysid_dim(sd, ad) == want == B.sysid_dim(sd, ad)


def test_width_refuses_bad_arguments(lib):
    for sd, ad in ((0, 1), (1, 0), (-2, 1), (50000, 50000)):
        assert lib.bsig_sysid_dim(sd, ad) == -1
        with pytest.raises(ValueError, match='dynamics-fit row'):
            summarizers.sysid_dim(sd, ad)
    assert lib.bsig_sysid_dim(40000, 1) == 40002 * 40000 + 40000
    for bad in (1.5, '2', None):
        with pytest.raises(ValueError, match='must be ints'):
            summarizers.sysid_dim(bad, 1)


def test_fits_codes_and_messages(lib):
    ok, einval, eunsup = _lib.BSIG_OK, _lib.BSIG_EINVAL, _lib.BSIG_EUNSUPPORTED
    # (ts, ta, sd, ad, itemsize): what the issue asks to cover
    for ts, sd, ad, sizes in ((21, 3, 1, (4, 8)), (50, 60, 8, (4, 8)), (100, 60, 8, (4, 8)), (50, 211, 20, (4,))):
        for itemsize in sizes:
            assert lib.bsig_sysid_fits(ts, ts, sd, ad, itemsize) == ok
    # ShadowHand at 50 states in double: 16 + 50 * 233 * 8 + 49 * 49 * 8 + 49 * 211 * 8, each part rounded up to
    # 16, = 195 152 B > 163 840 B
    assert lib.bsig_sysid_fits(50, 50, 211, 20, 8) == eunsup
    assert 'LDS' in err(lib) and '195152 B' in err(lib) and err(lib).startswith('sysid_f64:')
    assert lib.bsig_sysid_fits(300, 300, 211, 20, 4) == eunsup and 'LDS' in err(lib)
    assert lib.bsig_sysid_fits(2, 1, 3, 1, 4) == ok                       # M = 1
    assert lib.bsig_sysid_fits(1, 1, 3, 1, 4) == einval and 'ts 1' in err(lib)
    assert lib.bsig_sysid_fits(21, 0, 3, 1, 4) == einval and 'ta' in err(lib)
    assert lib.bsig_sysid_fits(21, 21, 0, 1, 4) == einval and 'sd' in err(lib)
    assert lib.bsig_sysid_fits(21, 21, 3, 0, 4) == einval and 'ad' in err(lib)
    assert lib.bsig_sysid_fits(21, 21, 3, 1, 2) == einval and 'itemsize' in err(lib)


def test_trajectories_per_workgroup_and_the_numpy_plan(lib):
    assert lib.bsig_sysid_group(21, 21, 3, 1, 4) == 16 == lib.bsig_sysid_group(21, 21, 3, 1, 8)
    assert lib.bsig_sysid_group(50, 50, 60, 8, 4) == 1
    assert lib.bsig_sysid_group(50, 50, 211, 20, 8) == _lib.BSIG_EUNSUPPORTED
    assert lib.bsig_sysid_group(1, 1, 3, 1, 4) == _lib.BSIG_EINVAL
    # 16 Pendulum trajectories of 3000 states are 960 KB: 1 fits 64 KiB
    assert lib.bsig_sysid_group(3000, 3000, 3, 1, 4) == 1
    shapes = [case[1:5] for case in SC.CASES.values()] + [(3000, 3000, 3, 1), (50, 50, 211, 20), (9, 9, 1, 1)]
    for ts, ta, sd, ad in shapes:
        for itemsize in (4, 8):
            g, mine = lib.bsig_sysid_group(ts, ta, sd, ad, itemsize), SC.plan(ts, sd, ad, itemsize)
            assert (mine is None and g == _lib.BSIG_EUNSUPPORTED) or mine[2] == g, (ts, sd, ad, itemsize)
    for name, case in SC.CASES.items():
        assert case[0] is not None or lib.bsig_sysid_group(*case[1:5], 4) > 1, name
    # which system: a function of the shape only
    assert [SC.plan(ts, 3, 1, 4)[:2] for ts in (2, 5, 6, 7)] == [(True, 1), (True, 4), (False, 5), (False, 5)]
    assert SC.plan(50, 60, 8, 4)[:2] == (True, 49) and SC.plan(100, 60, 8, 8)[:2] == (False, 69)
    assert SC.plan(50, 211, 20, 4)[:2] == (True, 49)


@pytest.mark.parametrize('fn', ['bsig_sysid', 'bsig_sysid_f64'])
def test_launch_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = 'sysid_f64' if fn.endswith('f64') else 'sysid'
    # (states, actions, out, n, ts, ta, sd, ad, ridge, ld_out, nonfinite, stream)
    rc = call(FAKE, FAKE, FAKE, 4, 1, 1, 3, 1, 1e-3, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ts 1' in err(lib) and err(lib).startswith(what + ':')
    rc = call(FAKE, FAKE, FAKE, 4, 21, 0, 3, 1, 1e-3, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ta' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 0, 1, 1e-3, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'sd' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 0, 1e-3, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ad' in err(lib)
    for ridge in (0.0, -1e-3, float('nan'), float('inf')):
        rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, ridge, 64, None, None)
        assert rc == _lib.BSIG_EINVAL and 'ridge' in err(lib)
    if not fn.endswith('f64'):      # positive in double, zero in fp32
        rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 1e-60, 64, None, None)
        assert rc == _lib.BSIG_EINVAL and 'ridge' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 1e-3, 17, None, None)             # width 18
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        rc = call(*args, 4, 21, 21, 3, 1, 1e-3, 20, None, None)
        assert rc == _lib.BSIG_EINVAL and 'null' in err(lib)
    rc = call(FAKE, FAKE, FAKE, -1, 21, 21, 3, 1, 1e-3, 20, None, None)
    assert rc == _lib.BSIG_EINVAL and 'n=' in err(lib)
    if fn.endswith('f64'):       # (in fp32 this shape is covered: it would launch)
        rc = call(FAKE, FAKE, FAKE, 4, 50, 50, 211, 20, 1e-1, 1 << 20, None, None)
        assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 300, 300, 211, 20, 1e-1, 1 << 20, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
    message = err(lib)
    assert lib.bsig_sysid_fits(300, 300, 211, 20, 8 if fn.endswith('f64') else 4) == _lib.BSIG_EUNSUPPORTED
    assert err(lib) == message                                    # the launch's own code and message
    # an empty batch is fine and touches nothing, whatever else is passed
    assert call(None, None, None, 0, 21, 21, 3, 1, 1e-3, 20, None, None) == _lib.BSIG_OK
    assert call(None, None, None, 0, 1, 0, 3, 1, -1.0, 0, None, None) == _lib.BSIG_OK


# ------------------------------------------------------------------ the Python mirror
def test_the_summarizers_value_errors_come_before_any_gpu_call(monkeypatch):
    def no_gpu():
        raise RuntimeError('asked for a GPU')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    states, actions = torch.zeros(4, 21, 3), torch.zeros(4, 21, 1)
    for bad in (0.0, -1e-3, 1, True, None, '1e-3', float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError) as caught:
            B.summary_sysid(states, actions, ridge=bad)
        assert str(caught.value) == 'ridge must be a positive float, got %r' % (bad,)
    with pytest.raises(ValueError, match='needs 2 states or more, got 1'):
        B.summary_sysid(states[:, :1], actions)
    with pytest.raises(ValueError, match='needs 1 action or more, got 0'):
        B.summary_sysid(states, actions[:, :0])
    with pytest.raises(ValueError, match='float32 or torch.float64'):
        B.summary_sysid(states, actions, dtype=torch.float16)
    with pytest.raises(AssertionError):
        B.summary_sysid(states[0], actions)
    with pytest.raises(RuntimeError, match='asked for a GPU'):       # valid arguments get as far as the GPU
        B.summary_sysid(states, actions)


def _bayes_sim(obs_dim=3, act_dim=1, **keys):
    return B.BayesSim(model_cfg=dict(CFG, **keys), obs_dim=obs_dim, act_dim=act_dim, **KW)


def test_the_table_entry():
    entry = SUMMARIZERS['summary_sysid']
    assert entry.fxn is B.summary_sysid is summarizers.summary_sysid
    assert entry.keys == {'sysidRidge': 'summary_sysid'}
    assert entry.check_finite and not entry.lazy and entry.embedding is None and not entry.ragged
    assert [name for name, other in SUMMARIZERS.items() if 'sysidRidge' in other.keys] == ['summary_sysid']


def test_bayessim_sizes_the_model_and_validates_the_key():
    bs = _bayes_sim()
    assert bs.model.input_dim == 18 and bs.summarizer_fxn is B.summary_sysid and bs.embedding is None
    assert bs.summary_kwargs == {'ridge': 1e-3}
    assert _bayes_sim(sysidRidge=1e-1).summary_kwargs == {'ridge': 1e-1}
    assert _bayes_sim(60, 8, trainTrajLen=100, sysidRidge=0.1).model.input_dim == 4200
    assert 'sysid' not in ''.join(bs.model.state_dict())
    for bad in (0.0, -1.0, 1, True, None, 'small', float('nan'), float('inf')):
        with pytest.raises(ValueError) as caught:
            _bayes_sim(sysidRidge=bad)
        assert str(caught.value) == "model_cfg['sysidRidge'] must be a positive float, got %r" % (bad,)
    with pytest.raises(ValueError, match=r"model_cfg\['trainTrajLen'\] = 1 leaves no step"):
        _bayes_sim(trainTrajLen=1)
    for name in sorted(set(SUMMARIZERS) - {'summary_sysid'}):
        with pytest.raises(ValueError) as caught:
            B.BayesSim(model_cfg=dict(CFG, summarizerFxn=name, sysidRidge=1e-3), obs_dim=3, act_dim=1, **KW)
        assert str(caught.value) == "model_cfg['sysidRidge'] applies to 'summary_sysid', not to '%s'" % name
    for key, value in (('xcorrLags', 0), ('kmeFeatures', 256), ('sigChannels', [0])):
        with pytest.raises(ValueError, match='applies to'):
            _bayes_sim(**{key: value})
    # ShadowHand at 50 states: fits in fp32, refused in double with bsig_sysid_fits' message
    assert _bayes_sim(211, 20, trainTrajLen=50).model.input_dim == 49163
    with pytest.raises(NotImplementedError, match='sysid_f64: 195152 B of LDS'):
        _bayes_sim(211, 20, trainTrajLen=50, dtype='float64', summaryDtype='float64')
    with pytest.raises(ValueError, match="lengths apply to 'summary_xcorr' and 'summary_kme', not to 'summary_sysid'"):
        bs.predict(torch.zeros(2, 21, 3), torch.zeros(2, 21, 1), lengths=[21, 21])


def test_the_arguments_that_reach_the_summarizer():
    """In the manner of tests/test_summarizer_table_host.py: the keyword arguments of the one summarizer call."""
    states, actions, flag = torch.zeros(2, 21, 3), torch.zeros(2, 21, 1), torch.zeros(1, dtype=torch.int32)

    def recorded(bs, *args, **kwargs):
        calls = []
        bs.summarizer_fxn = lambda *a, **kw: (calls.append((a, kw)), torch.zeros(2, bs.model.input_dim))[1]
        out = bs._summarize(states, actions, *args, **kwargs)
        assert tuple(out.shape) == (2, 18) and len(calls) == 1
        (a, kw), = calls
        assert a[0] is states and a[1] is actions
        return a[2:], kw
    fixed = {'ridge': 1e-2}
    checked = dict(fixed, check_finite=flag)
    bs = _bayes_sim(sysidRidge=1e-2)
    assert recorded(bs) == ((), fixed)
    assert recorded(bs, flag) == ((), checked)
    assert recorded(bs, flag, lazy=True) == ((), checked)
    assert recorded(bs, None, lazy=True) == ((), fixed)
    bs._lazy_summaries = lambda: True
    assert recorded(bs, flag, lazy=True) == ((), checked)            # not lazy: no factor rows
    double = _bayes_sim(sysidRidge=1e-2, dtype='float64', summaryDtype='float64')
    assert recorded(double) == ((), dict(fixed, dtype=torch.float64))
    assert recorded(double, flag) == ((), dict(checked, dtype=torch.float64))


# ------------------------------------------------------------------ the yardstick
def test_the_reference_is_the_least_squares_fit():
    """Against numpy.linalg.lstsq on the augmented system [Phi; sqrt(M rho) I] W = [Y; 0], another algorithm."""
    for name in ('pendulum', 'boundary_m4', 'odd', 'ta_1', 'ta_t_minus_1', 'ta_above_t'):
        n, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
        states, actions, ref, _ = _case(name)
        phi, y = SC.regressors(states, actions)
        m, p = phi.shape[1:]
        assert ref.shape == (states.shape[0], SC.width(sd, ad))
        for i in range(states.shape[0]):
            rho = ridge * np.trace(phi[i].T @ phi[i] / m) / p
            w = np.linalg.lstsq(np.concatenate([phi[i], np.sqrt(m * rho) * np.eye(p)]),
                                np.concatenate([y[i], np.zeros((p, sd))]), rcond=None)[0]
            r = np.sqrt(((y[i] - phi[i] @ w) ** 2).mean(axis=0))
            np.testing.assert_allclose(ref[i], np.concatenate([w.reshape(-1), r]), rtol=1e-9, atol=1e-11)
    # the padding: one action is every step's action; an action from step M on enters nothing
    states, actions, ref, _ = _case('ta_1')
    assert np.array_equal(ref, SC.reference(states, np.repeat(actions, 20, axis=1), 1e-2))
    states, actions, ref, _ = _case('ta_above_t')
    assert np.array_equal(ref, SC.reference(states, actions[:, :20], SC.DEFAULT_RIDGE))
    # a constant trajectory: W and r are zero
    ref = SC.reference(np.full((2, 9, 3), 1.5, dtype=np.float32), np.full((2, 9, 1), -0.5, dtype=np.float32))
    assert (ref == 0).all()


@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_the_fp32_bound_proves_something_and_holds_the_kernels_form(name):
    n, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    states, actions, ref, (d_w, d_r) = _case(name)
    w, _ = SC.split(ref, sd, ad)
    relative = float((d_w / np.linalg.norm(w, axis=1)).max())
    q_w, q_r = SC.ratios(SC.kernel_form(states, actions, ridge), ref, d_w, d_r, sd, ad)
    print('%s: bound / ||W_:j|| = %.3g; the fp32 restatement: worst |err| / bound W %.3g, r %.3g'
          % (name, relative, q_w, q_r))
    assert relative <= 1e-2
    assert 0 < q_w <= 1.0 and 0 < q_r <= 1.0


def test_the_ill_conditioned_cases_are_for_double():
    """ridge 1e-6 on Ant: the fp32 bound says nothing (the factorisation's perturbation alone is of the order of
    the smallest eigenvalue), the fp64 bound is small."""
    for name, (n, ts, ta, sd, ad, ridge) in SC.ILL.items():
        states, actions = SC.trajectories(n, ts, ta, sd, ad)
        ref = SC.reference(states, actions, ridge)
        w, _ = SC.split(ref, sd, ad)
        d_w, _ = SC.bounds(states, actions, ridge, SC.U64)
        assert float((d_w / np.linalg.norm(w, axis=1)).max()) <= 1e-6
        p = 1 + sd + ad
        assert p * p * SC.U32 / ridge > 0.1          # the header's p^2 u / ridge
