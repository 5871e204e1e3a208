"""CPU-side checks of the general signature entry points (include/bsig_signature.h: depth up to 6, a chosen
subset of channels): the width and cover queries are host arithmetic, the argument checks come before any
launch, and the Python mirror validates a channel list and a depth before it asks for a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib, summarizers

CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_signatory', 'trainTrajLen': 11, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)
# (depth, widest d, longest path) include/bsig_signature.h promises in both precisions
COVERED = [(4, 10, 64), (5, 6, 64), (6, 4, 64), (3, 22, 64), (2, 110, 32), (1, 232, 1000), (1, 100000, 2)]


def _err():
    return _lib.load().bsig_last_error().decode()


@pytest.mark.parametrize('d,depth,width', [(3, 4, 120), (6, 4, 1554), (5, 5, 3905), (10, 4, 11110),
                                           (22, 3, 11154), (2, 6, 126)])
def test_width_of_a_signature_row(d, depth, width):
    assert width == sum(d ** k for k in range(1, depth + 1))
    assert _lib.load().bsig_signature_ex_dim(d, depth) == width
    assert summarizers.signature_dim(d, depth) == width


@pytest.mark.parametrize('d,depth', [(1, 3), (3, 0), (3, 7), (100000, 2), (2 ** 31 - 1, 2)])
def test_no_width_for_a_bad_path_dim_depth_or_an_int32_overflow(d, depth):
    assert _lib.load().bsig_signature_ex_dim(d, depth) == -1
    with pytest.raises(ValueError):
        summarizers.signature_dim(d, depth)


def test_binding_lists_the_entry_points_and_the_seam_routes_them():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py)"""
    names = _lib.exported_symbols('bsig_signature.h')
    assert names == sorted(['bsig_signature_ex', 'bsig_signature_ex_dim', 'bsig_signature_ex_f64',
                            'bsig_signature_ex_fits'])
    assert _lib.F32.symbol('signature_ex') == 'bsig_signature_ex'
    assert _lib.F64.symbol('signature_ex') == 'bsig_signature_ex_f64'
    assert _lib.SIGNATURE_MAX_DEPTH == 6


@pytest.mark.parametrize('itemsize', [4, 8])
@pytest.mark.parametrize('depth,dmax,length', COVERED)
def test_the_cover_table_fits(depth, dmax, length, itemsize):
    lib = _lib.load()
    for d in sorted({2, 3, dmax - 1, dmax}):
        for ln in (2, length):
            assert lib.bsig_signature_ex_fits(d, ln, depth, itemsize) == _lib.BSIG_OK, (d, ln, _err())


@pytest.mark.parametrize('itemsize', [4, 8])
def test_what_does_not_fit_is_refused_with_the_lds_named(itemsize):
    lib = _lib.load()
    assert lib.bsig_signature_ex_fits(7, 11, 6, itemsize) == _lib.BSIG_EUNSUPPORTED       # 7^6 terms
    assert 'LDS' in _err()
    assert lib.bsig_signature_ex_fits(10, 4000, 4, itemsize) == _lib.BSIG_EUNSUPPORTED    # the increments
    assert 'LDS' in _err()
    assert lib.bsig_signature_ex_fits(300, 2, 2, itemsize) == _lib.BSIG_EUNSUPPORTED
    assert 'LDS' in _err()
    # depth <= 0: the reference's rule (d = 5: depth 3)
    assert lib.bsig_signature_ex_fits(5, 20, 0, itemsize) == _lib.BSIG_OK
    for bad in ((1, 5, 2, itemsize), (3, 1, 2, itemsize), (3, 5, 7, itemsize), (3, 5, 2, 2)):
        assert lib.bsig_signature_ex_fits(*bad) == _lib.BSIG_EINVAL, bad


@pytest.mark.parametrize('name', ['bsig_signature_ex', 'bsig_signature_ex_f64'])
def test_c_abi_argument_errors(name):
    """The BSIG_REQUIRE checks come before any launch: no GPU needed.  Arguments: states, actions, channels,
    n_channels, out, n, length, sd, ad, depth, ld_out, stream."""
    fn = getattr(_lib.load(), name)
    one = ctypes.c_void_p(8)          # never dereferenced on the host
    assert fn(one, one, None, 0, one, 1, 5, 2, 1, 7, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'depth' in _err()
    assert fn(one, one, one, 3, one, 1, 5, 2, 1, 7, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'depth' in _err()
    assert fn(one, one, None, 0, one, 1, 1, 2, 1, 4, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'length' in _err()
    assert fn(one, one, None, 0, one, 1, 5, 2, 1, 4, 339, None) == _lib.BSIG_EINVAL          # width 340
    assert 'ld_out' in _err()
    assert fn(one, one, one, 3, one, 1, 5, 2, 1, 3, 83, None) == _lib.BSIG_EINVAL            # width 84
    assert 'ld_out' in _err()
    assert fn(one, one, None, 0, one, 1, 5, 2, 1, 3, 83, None) == _lib.BSIG_EINVAL           # (the old entry point's)
    assert 'ld_out' in _err()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert fn(args[0], args[1], None, 0, args[2], 1, 5, 2, 1, 4, 340, None) == _lib.BSIG_EINVAL
        assert 'null pointer' in _err()
    assert fn(one, one, one, 0, one, 1, 5, 2, 1, 4, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'n_channels' in _err()
    # refused, not spilled
    assert fn(one, one, None, 0, one, 1, 5, 5, 1, 6, 1 << 20, None) == _lib.BSIG_EUNSUPPORTED
    assert 'LDS' in _err()
    # the old refusals still come through the delegation: a forced depth 3 on a wide path
    assert fn(one, one, None, 0, one, 1, 4, 30, 3, 3, 1 << 20, None) == _lib.BSIG_EUNSUPPORTED
    assert 'path dim' in _err()
    # n = 0: nothing to do, nothing looked at
    assert fn(None, None, None, 0, None, 0, 1, 0, 0, 9, 0, None) == _lib.BSIG_OK


def test_the_old_entry_points_still_refuse_depth_4():
    lib = _lib.load()
    one = ctypes.c_void_p(8)
    assert lib.bsig_signature(one, one, one, 1, 4, 2, 1, 4, 100000, None) == _lib.BSIG_EINVAL
    assert lib.bsig_signature_f64(one, one, one, 1, 4, 2, 1, 4, 100000, None) == _lib.BSIG_EINVAL


@pytest.mark.parametrize('dtype', [None, torch.float64])
def test_python_refuses_a_bad_channel_list_or_depth_before_it_asks_for_a_gpu(dtype, monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    states, actions = torch.zeros(2, 5, 3), torch.zeros(2, 5, 2)
    for bad in ([5], [-1], [0, 5], [], (), [0.5], ['a'], 3):
        with pytest.raises(ValueError):
            summarizers.summary_signatory(states, actions, channels=bad, dtype=dtype)
    with pytest.raises(ValueError, match='depth'):
        summarizers.summary_signatory(states, actions, depth=7, dtype=dtype)
    with pytest.raises(ValueError, match='depth'):
        summarizers.summary_signatory(states, actions, depth=7, channels=[0], dtype=dtype)
    assert summarizers.signature_channels(np.array([4, 0, 0]), 3, 2) == (4, 0, 0)


def test_bayessim_takes_sig_depth_and_sig_channels():
    picked = [0, 210, 211, 230] + list(range(5, 22))
    assert len(picked) == 21
    hand = B.BayesSim(model_cfg=dict(CFG, sigChannels=picked, sigDepth=3), obs_dim=211, act_dim=20, **KW)
    assert hand.model.input_dim == 11154 and hand.summary_kwargs['channels'] == tuple(picked)
    assert B.BayesSim(model_cfg=dict(CFG, sigChannels=picked), obs_dim=211, act_dim=20, **KW).model.input_dim == 11154
    pend = dict(obs_dim=3, act_dim=1, **KW)
    assert B.BayesSim(model_cfg=dict(CFG, sigDepth=4, sigChannels=[0, 1, 3]), **pend).model.input_dim == 340
    assert B.BayesSim(model_cfg=dict(CFG, sigDepth=5), **pend).model.input_dim == 3905
    assert B.BayesSim(model_cfg=dict(CFG, sigDepth=2), **pend).model.input_dim == 30            # as before
    assert B.BayesSim(model_cfg=CFG, **pend).model.input_dim == 155
    both = dict(CFG, sigDepth=4, dtype='float64', summaryDtype='float64')
    assert B.BayesSim(model_cfg=both, **pend).model.input_dim == 780
    with pytest.raises(ValueError, match='sigChannels'):
        B.BayesSim(model_cfg=dict(CFG, summarizerFxn='summary_start', sigChannels=[0]), **pend)
    for bad in ([4], [], [0.5]):
        with pytest.raises(ValueError):
            B.BayesSim(model_cfg=dict(CFG, sigChannels=bad), **pend)
    for bad in (7, 0, -1):
        with pytest.raises(ValueError, match='sigDepth'):
            B.BayesSim(model_cfg=dict(CFG, sigDepth=bad), **pend)
    # refused at construction, not at the first fit: 7^6 terms do not fit a workgroup's LDS
    with pytest.raises(NotImplementedError, match='LDS'):
        B.BayesSim(model_cfg=dict(CFG, sigDepth=6), obs_dim=5, act_dim=1, **KW)
