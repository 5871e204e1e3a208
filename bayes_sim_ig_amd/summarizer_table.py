"""What BayesSim knows about each ``'summarizerFxn'``: one entry per name, nothing else anywhere.  A new
summarizer is one ``configure`` function and one line of ``SUMMARIZERS``.

An entry (``Summarizer``) holds:

- ``fxn``: the summarizer.
- ``keys``: the ``model_cfg`` keys it owns -> the name the "applies to" message prints for that key.
- ``configure``: ``(model_cfg, obs_dim, act_dim, itemsize) -> (the summary width, the keyword arguments of every
  call)``; it validates the entry's own keys and asks the library whether the shape fits a workgroup.
- ``check_finite``: it takes ``check_finite=`` (the isfinite assert of summarizers.py:120, deferred with the logs).
- ``lazy``: it takes ``lazy=True`` (summarizers.CrossCorrFactors).
- ``embedding``: None, or ``(model_cfg, obs_dim, act_dim, device) ->`` the module it is called with as its third
  positional argument (``model_cfg`` has been through ``configure``).
- ``ragged``: it takes ``lengths=``, the valid states of every trajectory (include/bsig_ragged.h).
"""
from collections import namedtuple

import numpy as np

from . import _lib
from . import summarizers as _summ
from .kme import KernelMeanEmbedding

Summarizer = namedtuple('Summarizer', 'fxn keys configure check_finite lazy embedding ragged',
                        defaults=(False, False, None, False))


def given(model_cfg, key):
    """Whether the config sets ``key`` (``'sigChannels': None`` is every channel: as without the key)."""
    return key in model_cfg and not (key == 'sigChannels' and model_cfg[key] is None)


def _plain(name):
    """The reference's summarizers: the width is a closed form (``sigDepth``, range-checked for every name, is
    handed on as it always was)."""
    def configure(model_cfg, obs_dim, act_dim, itemsize):
        return _summ.summary_dim(name, model_cfg['trainTrajLen'], obs_dim, act_dim,
                                 model_cfg.get('sigDepth') or 0), {}
    return configure


def _signature_path(model_cfg, obs_dim, act_dim):
    """``sigDepth`` and ``sigChannels`` as (the path's width, the depth in force, the keyword arguments):
    ``depth`` / ``channels`` are passed only where the config gave one of them."""
    depth, channels = model_cfg.get('sigDepth'), model_cfg.get('sigChannels')
    if channels is not None:
        channels = _summ.signature_channels(channels, obs_dim, act_dim)
    path_dim = 1 + (obs_dim + act_dim if channels is None else len(channels))
    kwargs = {'depth': depth, 'channels': channels} if depth or channels is not None else {}
    return path_dim, depth or _summ.signature_depth(path_dim), kwargs


def _signatory(model_cfg, obs_dim, act_dim, itemsize):
    path_dim, depth, kwargs = _signature_path(model_cfg, obs_dim, act_dim)
    if kwargs.get('channels') is None and depth <= 3:      # the call it always was: the reference's width
        return _plain('summary_signatory')(model_cfg, obs_dim, act_dim, itemsize)[0], kwargs
    # include/bsig_signature.h: the general kernel; whether it covers the shape is host arithmetic
    width = _summ.signature_dim(path_dim, depth)
    _lib.check(_lib.load().bsig_signature_ex_fits(path_dim, model_cfg['trainTrajLen'], depth, itemsize))
    return width, kwargs


def _logsignature(model_cfg, obs_dim, act_dim, itemsize):
    # include/bsig_logsignature.h: the same kernel's LDS at every depth but 1 (level 1 needs none)
    path_dim, depth, kwargs = _signature_path(model_cfg, obs_dim, act_dim)
    width = _summ.logsignature_dim(path_dim, depth)
    if depth > 1:
        _lib.check(_lib.load().bsig_signature_ex_fits(path_dim, model_cfg['trainTrajLen'], depth, itemsize))
    return width, kwargs


def _xcorr(model_cfg, obs_dim, act_dim, itemsize):
    # include/bsig_xcorr.h: the keys, the lags against the feature steps, then the trajectory against the LDS
    lags, state_diff = model_cfg.get('xcorrLags', 0), model_cfg.get('xcorrStateDiff', True)
    if isinstance(lags, bool) or not isinstance(lags, int) or lags < 0:
        raise ValueError("model_cfg['xcorrLags'] must be an int >= 0, got %r" % (lags,))
    if not isinstance(state_diff, bool):
        raise ValueError("model_cfg['xcorrStateDiff'] must be a bool, got %r" % (state_diff,))
    length = model_cfg['trainTrajLen']
    steps = length - (1 if state_diff else 0)
    if lags > steps - 1:
        raise ValueError("model_cfg['xcorrLags'] = %d is outside 0..%d: trainTrajLen = %d leaves %d "
                         "feature steps" % (lags, steps - 1, length, steps))
    width = _summ.xcorr_dim(obs_dim, act_dim, lags)
    _lib.check(_lib.load().bsig_xcorr_fits(length, length, obs_dim, act_dim, lags, 1 if state_diff else 0,
                                           itemsize))
    return width, {'max_lag': lags, 'state_diff': state_diff}


def _kme_arguments(model_cfg):
    """The keys of ``'summarizerFxn': 'summary_kme'`` as KernelMeanEmbedding's arguments; ValueError on a value
    of the wrong kind."""
    n_feat = model_cfg.get('kmeFeatures', 256)
    if isinstance(n_feat, bool) or not isinstance(n_feat, int) or n_feat < 2 or n_feat % 2:
        raise ValueError("model_cfg['kmeFeatures'] must be an even int >= 2, got %r" % (n_feat,))
    scale = model_cfg.get('kmeScale', 1.0)
    if not isinstance(scale, float) or not (np.isfinite(scale) and scale > 0.0):
        raise ValueError("model_cfg['kmeScale'] must be a positive float, got %r" % (scale,))
    seed = model_cfg.get('kmeSeed', 0)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError("model_cfg['kmeSeed'] must be an int in 0..2^32 - 1, got %r" % (seed,))
    flags = {}
    for key, default in (('kmeDiff', True), ('kmeTime', False)):
        flags[key] = model_cfg.get(key, default)
        if not isinstance(flags[key], bool):
            raise ValueError("model_cfg[%r] must be a bool, got %r" % (key, flags[key]))
    return {'n_feat': n_feat, 'scale': scale, 'seed': seed, 'diff': flags['kmeDiff'], 'time': flags['kmeTime']}


def _kme(model_cfg, obs_dim, act_dim, itemsize):
    # include/bsig_kme.h: the keys, then a block of rows against the LDS
    args = _kme_arguments(model_cfg)
    length = model_cfg['trainTrajLen']
    if length - (1 if args['diff'] else 0) < 1:
        raise ValueError("model_cfg['trainTrajLen'] = %d leaves no transition row" % (length,))
    _summ.kme_row_dim(obs_dim, act_dim, args['diff'], args['time'])
    _lib.check(_lib.load().bsig_kme_fits(length, length, obs_dim, act_dim, args['n_feat'] // 2,
                                         int(args['diff']), int(args['time']), itemsize))
    return args['n_feat'], {}


def _kme_embedding(model_cfg, obs_dim, act_dim, device):
    return KernelMeanEmbedding(obs_dim, act_dim, device=device, **_kme_arguments(model_cfg))


def _sysid(model_cfg, obs_dim, act_dim, itemsize):
    # include/bsig_sysid.h: the key, then the trajectory and the system it solves against the LDS
    ridge = _summ.sysid_ridge(model_cfg.get('sysidRidge', 1e-3), "model_cfg['sysidRidge']")
    length = model_cfg['trainTrajLen']
    if length < 2:
        raise ValueError("model_cfg['trainTrajLen'] = %d leaves no step to fit" % (length,))
    width = _summ.sysid_dim(obs_dim, act_dim)
    _lib.check(_lib.load().bsig_sysid_fits(length, length, obs_dim, act_dim, itemsize))
    return width, {'ridge': ridge}


_SIG_KEYS = {'sigChannels': 'summary_signatory'}
_XCORR_KEYS = dict.fromkeys(('xcorrLags', 'xcorrStateDiff'), 'summary_xcorr')
_KME_KEYS = dict.fromkeys(('kmeFeatures', 'kmeScale', 'kmeSeed', 'kmeDiff', 'kmeTime'), 'summary_kme')

SUMMARIZERS = {
    'summary_start': Summarizer(_summ.summary_start, {}, _plain('summary_start')),
    'summary_waypts': Summarizer(_summ.summary_waypts, {}, _plain('summary_waypts')),
    'summary_corr': Summarizer(_summ.summary_corr, {}, _plain('summary_corr'), check_finite=True, lazy=True),
    'summary_corrdiff': Summarizer(_summ.summary_corrdiff, {}, _plain('summary_corrdiff'), check_finite=True,
                                   lazy=True),
    'summary_signatory': Summarizer(_summ.summary_signatory, _SIG_KEYS, _signatory),
    'summary_logsignature': Summarizer(_summ.summary_logsignature, _SIG_KEYS, _logsignature),
    'summary_xcorr': Summarizer(_summ.summary_xcorr, _XCORR_KEYS, _xcorr, check_finite=True, ragged=True),
    'summary_kme': Summarizer(_summ.summary_kme, _KME_KEYS, _kme, check_finite=True, embedding=_kme_embedding,
                              ragged=True),
    'summary_sysid': Summarizer(_summ.summary_sysid, {'sysidRidge': 'summary_sysid'}, _sysid, check_finite=True),
}
