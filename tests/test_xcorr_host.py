"""CPU-side checks of the time-lagged cross-correlation summary (include/bsig_xcorr.h): the width, the cover
and the group queries are host arithmetic; every argument check of the launch entry points comes before any
launch (the pattern of tests/test_cabi_errors.py); the Python mirror validates ``max_lag`` before it asks for
a GPU; BayesSim sizes its first layer by ``xcorr_dim`` and validates its two keys.  The numpy restatement of
the definition (tests/xcorr_cases.py) is checked against a literal triple loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import xcorr_cases as XC
from bayes_sim_ig_amd import _lib, summarizers

FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_xcorr', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsig_last_error().decode()


@pytest.mark.parametrize('sd,ad,k', [(3, 1, 0), (3, 1, 4), (3, 1, 19), (60, 8, 0), (60, 8, 4), (211, 20, 0),
                                     (211, 20, 1), (24, 12, 0), (1, 1, 0)])
def test_width_is_the_closed_form(lib, sd, ad, k):
    want = (k + 1) * sd * ad + 2 * sd
    assert XC.width(sd, ad, k) == want
    assert lib.bsig_xcorr_dim(sd, ad, k) == want
    assert summarizers.xcorr_dim(sd, ad, k) == want == B.xcorr_dim(sd, ad, max_lag=k)
    assert summarizers.xcorr_dim(sd, ad) == sd * ad + 2 * sd


def test_the_issues_widths(lib):
    # Pendulum, Ant, Anymal, ShadowHand-more at lag 0
    assert [lib.bsig_xcorr_dim(*dims, 0) for dims in ((3, 1), (60, 8), (48, 12), (211, 20))] == [9, 600, 672, 4642]


def test_width_refuses_bad_arguments(lib):
    for sd, ad, k in ((0, 1, 0), (1, 0, 0), (3, 1, -1), (-2, 1, 0), (50000, 50000, 0), (1000, 1000, 3000)):
        assert lib.bsig_xcorr_dim(sd, ad, k) == -1
        with pytest.raises(ValueError, match='cross-correlation row'):
            summarizers.xcorr_dim(sd, ad, k)
    assert lib.bsig_xcorr_dim(1000, 1000, 2000) == 2001 * 10 ** 6 + 2000
    for bad in (1.5, '2', None, True):
        with pytest.raises(ValueError, match='max_lag'):
            summarizers.xcorr_dim(3, 1, bad)


def test_fits_codes_and_messages(lib):
    ok, einval, eunsup = _lib.BSIG_OK, _lib.BSIG_EINVAL, _lib.BSIG_EUNSUPPORTED
    # (length, ta, sd, ad, max_lag, state_diff, itemsize)
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, 19, 1, 4) == ok            # max_lag = M - 1
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, 20, 1, 4) == einval and 'max_lag' in err(lib)      # = M
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, 20, 0, 8) == ok            # M = T without the difference
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, 21, 0, 8) == einval and 'max_lag' in err(lib)
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, -1, 1, 4) == einval and 'max_lag' in err(lib)
    assert lib.bsig_xcorr_fits(1, 1, 3, 1, 0, 1, 4) == einval and 'M = 0' in err(lib) and 'ts' in err(lib)
    assert lib.bsig_xcorr_fits(1, 1, 3, 1, 0, 0, 4) == ok               # one state, no difference: M = 1
    assert lib.bsig_xcorr_fits(2, 1, 3, 1, 0, 1, 4) == ok
    assert lib.bsig_xcorr_fits(0, 1, 3, 1, 0, 0, 4) == einval and 'ts' in err(lib)
    assert lib.bsig_xcorr_fits(21, 0, 3, 1, 0, 1, 4) == einval and 'ta' in err(lib)
    assert lib.bsig_xcorr_fits(21, 21, 0, 1, 0, 1, 4) == einval and 'sd' in err(lib)
    assert lib.bsig_xcorr_fits(21, 21, 3, 0, 0, 1, 4) == einval and 'ad' in err(lib)
    assert lib.bsig_xcorr_fits(21, 21, 3, 1, 0, 1, 2) == einval and 'itemsize' in err(lib)
    # Pendulum, Ant, Anymal and ShadowHand at 50 steps, both precisions (ShadowHand in double: 92 KB)
    for sd, ad in ((3, 1), (60, 8), (48, 12), (211, 20)):
        for itemsize in (4, 8):
            assert lib.bsig_xcorr_fits(50, 50, sd, ad, 4, 1, itemsize) == ok
    # a shape refused for LDS in double and accepted in fp32: ShadowHand at 100 steps
    # (100 * 211 + 99 * 20) * 8 = 184 640 B > 163 840 B; * 4 = 92 320 B
    assert lib.bsig_xcorr_fits(100, 100, 211, 20, 0, 1, 4) == ok
    assert lib.bsig_xcorr_fits(100, 100, 211, 20, 0, 1, 8) == eunsup and 'LDS' in err(lib)
    # the header's limits: 88 steps in double, 177 in fp32
    assert lib.bsig_xcorr_fits(88, 88, 211, 20, 0, 1, 8) == ok
    assert lib.bsig_xcorr_fits(89, 89, 211, 20, 0, 1, 8) == eunsup and 'LDS' in err(lib)
    assert lib.bsig_xcorr_fits(177, 177, 211, 20, 0, 1, 4) == ok
    assert lib.bsig_xcorr_fits(178, 178, 211, 20, 0, 1, 4) == eunsup and 'LDS' in err(lib)
    # the reciprocals travel with the launch
    assert lib.bsig_xcorr_fits(400, 400, 3, 1, 255, 1, 4) == ok
    assert lib.bsig_xcorr_fits(400, 400, 3, 1, 256, 1, 4) == eunsup and 'max_lag 256' in err(lib)


def test_trajectories_per_workgroup(lib):
    """G: 256 / max(16, outputs rounded up to a power of two), halved until the trajectories take 64 KiB."""
    assert lib.bsig_xcorr_group(21, 21, 3, 1, 0, 1, 4) == 16             # 9 outputs
    assert lib.bsig_xcorr_group(21, 21, 3, 1, 4, 1, 4) == 8              # 21
    assert lib.bsig_xcorr_group(21, 21, 3, 1, 19, 1, 8) == 2             # 66
    assert lib.bsig_xcorr_group(15, 15, 10, 4, 1, 1, 4) == 2             # 100
    assert lib.bsig_xcorr_group(15, 14, 6, 3, 1, 0, 8) == 4              # 48
    assert lib.bsig_xcorr_group(50, 50, 60, 8, 0, 1, 4) == 1             # 600
    assert lib.bsig_xcorr_group(50, 50, 211, 20, 0, 1, 8) == 1
    # 9 outputs would share a workgroup among 16, but 16 trajectories of 3 * 2000 floats are 384 KB: 2 fit 64 KiB
    assert lib.bsig_xcorr_group(2000, 2000, 3, 1, 0, 1, 4) == 2
    assert lib.bsig_xcorr_group(21, 21, 3, 1, 20, 1, 4) == _lib.BSIG_EINVAL
    assert lib.bsig_xcorr_group(100, 100, 211, 20, 0, 1, 8) == _lib.BSIG_EUNSUPPORTED
    for name, (n, ts, ta, sd, ad, k, diff) in XC.CASES.items():
        for itemsize in (4, 8):
            g = lib.bsig_xcorr_group(ts, ta, sd, ad, k, int(diff), itemsize)
            assert g in (1, 2, 4, 8, 16), name
            assert n is not None or g > 1, name      # the cases that ask for row counts around G share workgroups


@pytest.mark.parametrize('fn', ['bsig_xcorr', 'bsig_xcorr_f64'])
def test_launch_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = 'xcorr_f64' if fn.endswith('f64') else 'xcorr'
    # (states, actions, out, n, ts, ta, sd, ad, max_lag, state_diff, ld_out, nonfinite, stream)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 20, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'max_lag' in err(lib) and err(lib).startswith(what + ':')
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, -1, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'max_lag' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 1, 1, 3, 1, 0, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'M = 0' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 0, 1, 3, 1, 0, 0, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ts' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 0, 3, 1, 0, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ta' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 0, 1, 0, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'sd' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 0, 0, 1, 64, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ad' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 0, 1, 8, None, None)              # width 9
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 4, 1, 20, None, None)             # width 21
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        rc = call(*args, 4, 21, 21, 3, 1, 0, 1, 12, None, None)
        assert rc == _lib.BSIG_EINVAL and 'null' in err(lib)
    rc = call(FAKE, FAKE, FAKE, -1, 21, 21, 3, 1, 0, 1, 12, None, None)
    assert rc == _lib.BSIG_EINVAL and 'n=' in err(lib)
    if fn.endswith('f64'):       # (in fp32 this shape is covered: it would launch)
        rc = call(FAKE, FAKE, FAKE, 4, 100, 100, 211, 20, 0, 1, 1 << 20, None, None)
        assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 200, 200, 211, 20, 0, 1, 1 << 20, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 4, 400, 400, 3, 1, 256, 1, 1 << 20, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'max_lag 256' in err(lib)
    # an empty batch is fine and touches nothing, whatever else is passed
    assert call(None, None, None, 0, 21, 21, 3, 1, 0, 1, 12, None, None) == _lib.BSIG_OK
    assert call(None, None, None, 0, 1, 1, 3, 1, 7, 1, 0, None, None) == _lib.BSIG_OK


def test_the_seam_routes_xcorr(lib):
    assert _lib.Precision.OPS['xcorr'] == ('bsig_xcorr', 'bsig_xcorr_f64')
    assert _lib.F32.symbol('xcorr') == 'bsig_xcorr' and _lib.F64.symbol('xcorr') == 'bsig_xcorr_f64'
    assert set(_lib.HEADERS['bsig_xcorr.h']) == {'bsig_xcorr_dim', 'bsig_xcorr_fits', 'bsig_xcorr_group',
                                                 'bsig_xcorr', 'bsig_xcorr_f64'}
    assert _lib.HEADERS['bsig_xcorr.h']['bsig_xcorr'] == _lib.HEADERS['bsig_xcorr.h']['bsig_xcorr_f64']


def test_summary_xcorr_validates_before_it_asks_for_a_gpu():
    states, actions = torch.zeros(2, 21, 3), torch.zeros(2, 21, 1)
    for lag, diff in ((20, True), (21, False), (-1, True), (10 ** 12, True)):
        with pytest.raises(ValueError, match='max_lag %d' % lag):
            summarizers.summary_xcorr(states, actions, max_lag=lag, state_diff=diff)
    for bad in (1.5, '2', None, True):
        with pytest.raises(ValueError, match='max_lag must be an int'):
            summarizers.summary_xcorr(states, actions, max_lag=bad)
    with pytest.raises(AssertionError):
        summarizers.summary_xcorr(states[:, :1], actions)            # one state leaves no difference
    with pytest.raises(AssertionError):
        summarizers.summary_xcorr(states[0], actions)
    with pytest.raises(ValueError, match='float32 or torch.float64'):
        summarizers.summary_xcorr(states, actions, dtype=torch.float16)
    assert B.summary_xcorr is summarizers.summary_xcorr and B.bayes_sim.summary_xcorr is B.summary_xcorr
    import bayes_sim_ig_amd.compat as compat
    compat.install()
    from bayes_sim_ig.utils.summarizers import summary_xcorr, xcorr_dim
    assert summary_xcorr is B.summary_xcorr and xcorr_dim is B.xcorr_dim


def test_the_numpy_reference_is_the_definition():
    """tests/xcorr_cases.reference against the sums written out, on a shape with padding and two lags."""
    states, actions = XC.trajectories(2, 6, 3, 2, 2, seed=5)
    for diff in (True, False):
        ref = XC.reference(states, actions, max_lag=2, state_diff=diff)
        s, a = states.astype(np.float64), actions.astype(np.float64)
        m = 5 if diff else 6
        assert ref.shape == (2, 3 * 4 + 4)
        for r in range(2):
            f = [[(s[r, t + 1, i] - s[r, t, i]) if diff else s[r, t, i] for i in range(2)] for t in range(m)]
            act = [[a[r, min(t, 2), j] for j in range(2)] for t in range(m)]
            want = []
            for tau in range(3):
                for i in range(2):
                    for j in range(2):
                        want.append(sum(f[t + tau][i] * act[t][j] for t in range(m - tau)) / (m - tau))
            mu = [sum(f[t][i] for t in range(m)) / m for i in range(2)]
            sig = [np.sqrt(sum((f[t][i] - mu[i]) ** 2 for t in range(m)) / m) for i in range(2)]
            np.testing.assert_allclose(ref[r], np.array(want + mu + sig), rtol=1e-13, atol=1e-15)
        bound = XC.bounds(states, actions, 2, diff, XC.U32)
        assert bound.shape == ref.shape and (bound > 0).all() and (bound < 1e-4).all()
    one = XC.reference(states[:, :2], actions, 0, True)
    assert (one[:, -2:] == 0).all() and (XC.bounds(states[:, :2], actions, 0, True, XC.U32)[:, -2:] == 0).all()


def _bayes_sim(cfg, obs_dim=3, act_dim=1):
    return B.BayesSim(model_cfg=cfg, obs_dim=obs_dim, act_dim=act_dim, **KW)


def test_bayessim_sizes_its_first_layer_by_xcorr_dim():
    assert _bayes_sim(CFG).model.input_dim == 9
    assert _bayes_sim(dict(CFG, xcorrLags=4)).model.input_dim == 21
    assert _bayes_sim(dict(CFG, xcorrLags=4, xcorrStateDiff=False)).model.input_dim == 21
    assert _bayes_sim(dict(CFG, xcorrStateDiff=False, xcorrLags=20)).model.input_dim == 69
    assert _bayes_sim(dict(CFG, trainTrajLen=50), obs_dim=60, act_dim=8).model.input_dim == 600
    assert _bayes_sim(dict(CFG, trainTrajLen=50, xcorrLags=1), obs_dim=211, act_dim=20).model.input_dim == 8862
    bs = _bayes_sim(dict(CFG, xcorrLags=19))
    assert bs.model.input_dim == 66 and bs.summarizer_fxn is B.summary_xcorr
    assert bs.summarizer_name == 'summary_xcorr' and bs.summary_kwargs['max_lag'] == 19
    assert bs.summary_kwargs['state_diff'] is True
    assert 'summary_xcorr' not in bs.model.state_dict() and not any('xcorr' in k for k in bs.model.state_dict())


def test_bayessim_validates_the_xcorr_keys():
    for lags in (-1, 1.0, '1', None, True, 20):            # 20 = M with trainTrajLen 21 and the difference
        with pytest.raises(ValueError, match='xcorrLags'):
            _bayes_sim(dict(CFG, xcorrLags=lags))
    with pytest.raises(ValueError, match='xcorrLags'):
        _bayes_sim(dict(CFG, xcorrLags=21, xcorrStateDiff=False))
    for diff in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='xcorrStateDiff'):
            _bayes_sim(dict(CFG, xcorrStateDiff=diff))
    for other in ('summary_start', 'summary_corrdiff', 'summary_signatory', 'summary_logsignature'):
        with pytest.raises(ValueError, match="xcorrLags.*applies to 'summary_xcorr'"):
            _bayes_sim(dict(CFG, summarizerFxn=other, xcorrLags=0))
        with pytest.raises(ValueError, match="xcorrStateDiff.*applies to 'summary_xcorr'"):
            _bayes_sim(dict(CFG, summarizerFxn=other, xcorrStateDiff=True))
    with pytest.raises(NameError, match="name 'summary_xcor' is not defined"):
        _bayes_sim(dict(CFG, summarizerFxn='summary_xcor'))
    # a trajectory beyond a workgroup's LDS: in double only
    long = dict(CFG, trainTrajLen=100)
    assert _bayes_sim(long, obs_dim=211, act_dim=20).model.input_dim == 4642
    with pytest.raises(NotImplementedError, match='LDS'):
        _bayes_sim(dict(long, dtype='float64', summaryDtype='float64'), obs_dim=211, act_dim=20)


def test_the_other_summarizers_keep_their_widths():
    for name, want in (('summary_start', 40), ('summary_corrdiff', 202)):
        assert _bayes_sim(dict(CFG, summarizerFxn=name)).model.input_dim == want
