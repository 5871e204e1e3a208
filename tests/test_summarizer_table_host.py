"""CPU-side checks of what BayesSim takes from the summarizer table (bayes_sim_ig_amd/summarizer_table.py): every
``model_cfg`` key that one summarizer owns is refused for every other, with the owner's name in the message;
``sigDepth`` belongs to nobody; the widths at Pendulum's dimensions; and the positional and keyword arguments that
reach the summarizer on every path of ``_summarize``.  The expected values were recorded from the constructor's
``if / elif`` chain that the table replaced."""
import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B

CFG = {'modelClass': 'MDNN', 'trainTrajLen': 21, 'components': 3, 'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2),
          prior=None)
WIDTHS = {'summary_start': 40, 'summary_waypts': 40, 'summary_corr': 202, 'summary_corrdiff': 202,
          'summary_signatory': 155, 'summary_logsignature': 55, 'summary_xcorr': 9, 'summary_kme': 256}
NAMES = sorted(WIDTHS)
# key -> (a valid value, the name the message prints, the names that own the key)
OWNED = {'sigChannels': ([0, 3], 'summary_signatory', ('summary_signatory', 'summary_logsignature')),
         'xcorrLags': (0, 'summary_xcorr', ('summary_xcorr',)),
         'xcorrStateDiff': (True, 'summary_xcorr', ('summary_xcorr',)),
         'kmeFeatures': (256, 'summary_kme', ('summary_kme',)),
         'kmeScale': (1.0, 'summary_kme', ('summary_kme',)),
         'kmeSeed': (0, 'summary_kme', ('summary_kme',)),
         'kmeDiff': (True, 'summary_kme', ('summary_kme',)),
         'kmeTime': (False, 'summary_kme', ('summary_kme',))}
SIGNATURES = ('summary_signatory', 'summary_logsignature')


def _bayes_sim(name, **keys):
    return B.BayesSim(model_cfg=dict(CFG, summarizerFxn=name, **keys), **KW)


@pytest.mark.parametrize('key', sorted(OWNED))
def test_an_owned_key_is_refused_for_every_other_summarizer(key):
    value, owner, owners = OWNED[key]
    for name in NAMES:
        if name in owners:
            assert _bayes_sim(name, **{key: value}).summarizer_name == name
            continue
        with pytest.raises(ValueError) as err:
            _bayes_sim(name, **{key: value})
        assert str(err.value) == "model_cfg['%s'] applies to '%s', not to '%s'" % (key, owner, name)


def test_sig_depth_belongs_to_nobody():
    assert _bayes_sim('summary_start', sigDepth=2).model.input_dim == 40
    for name in NAMES:
        with pytest.raises(ValueError, match=r"model_cfg\['sigDepth'\] must be in 1\.\.6, got 7"):
            _bayes_sim(name, sigDepth=7)
    # 'sigChannels': None is every channel, whoever summarises
    assert _bayes_sim('summary_start', sigChannels=None).model.input_dim == 40


@pytest.mark.parametrize('name', NAMES)
def test_the_widths_at_pendulums_dimensions(name):
    bs = _bayes_sim(name)
    assert bs.model.input_dim == WIDTHS[name] and bs.summarizer_fxn is getattr(B, name)
    assert (bs.embedding is not None) == (name == 'summary_kme')


def _recorded(bs, *args, **kwargs):
    """(positional arguments after the trajectories, keyword arguments) of the one summarizer call behind
    ``bs._summarize(states, actions, *args, **kwargs)``."""
    states, actions, calls = torch.zeros(2, 21, 3), torch.zeros(2, 21, 1), []

    def recorder(*a, **kw):
        calls.append((a, kw))
        return torch.zeros(2, bs.model.input_dim)
    bs.summarizer_fxn = recorder
    out = bs._summarize(states, actions, *args, **kwargs)
    assert tuple(out.shape) == (2, bs.model.input_dim) and len(calls) == 1
    (a, kw), = calls
    assert a[0] is states and a[1] is actions
    return a[2:], kw


@pytest.mark.parametrize('name', NAMES)
def test_the_arguments_that_reach_the_summarizer(name):
    flag = torch.zeros(1, dtype=torch.int32)
    fixed = {'max_lag': 0, 'state_diff': True} if name == 'summary_xcorr' else {}
    checked = dict(fixed, check_finite=flag) if name in ('summary_corr', 'summary_corrdiff', 'summary_xcorr',
                                                         'summary_kme') else fixed
    bs = _bayes_sim(name)
    extra = (bs.embedding,) if name == 'summary_kme' else ()
    assert bs.summary_kwargs == fixed
    assert _recorded(bs) == (extra, fixed)
    assert _recorded(bs, flag) == (extra, checked)
    assert _recorded(bs, flag, lazy=True) == (extra, checked)       # a CPU model takes no factor rows
    assert _recorded(bs, None, lazy=True) == (extra, fixed)
    bs._lazy_summaries = lambda: True
    lazy = dict(checked, lazy=True) if name in ('summary_corr', 'summary_corrdiff') else checked
    assert _recorded(bs, flag, lazy=True) == (extra, lazy)
    assert _recorded(bs, flag) == (extra, checked)                  # nobody asked
    double = _bayes_sim(name, dtype='float64', summaryDtype='float64')
    extra = (double.embedding,) if name == 'summary_kme' else ()
    assert _recorded(double) == (extra, dict(fixed, dtype=torch.float64))
    assert _recorded(double, flag) == (extra, dict(checked, dtype=torch.float64))


@pytest.mark.parametrize('name', SIGNATURES)
def test_a_signature_gets_depth_and_channels_only_when_the_config_set_one(name):
    flag = torch.zeros(1, dtype=torch.int32)
    assert _recorded(_bayes_sim(name), flag, lazy=True) == ((), {})
    assert _recorded(_bayes_sim(name, sigChannels=None)) == ((), {})
    for keys, want in ((dict(sigDepth=2), {'depth': 2, 'channels': None}),
                       (dict(sigChannels=[0, 3]), {'depth': None, 'channels': (0, 3)}),
                       (dict(sigDepth=4, sigChannels=np.array([3, 0, 0])), {'depth': 4, 'channels': (3, 0, 0)})):
        bs = _bayes_sim(name, **keys)
        assert bs.summary_kwargs == want
        assert _recorded(bs) == ((), want) and _recorded(bs, flag, lazy=True) == ((), want)
        double = _bayes_sim(name, dtype='float64', summaryDtype='float64', **keys)
        assert _recorded(double) == ((), dict(want, dtype=torch.float64))
    for other in ('summary_start', 'summary_corrdiff'):
        assert _recorded(_bayes_sim(other, sigDepth=2)) == ((), {})


def test_xcorr_gets_its_lags_and_its_difference():
    bs = _bayes_sim('summary_xcorr', xcorrLags=4, xcorrStateDiff=False)
    assert bs.model.input_dim == 21 and _recorded(bs) == ((), {'max_lag': 4, 'state_diff': False})
