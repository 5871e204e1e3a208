"""CPU-side checks of the log-signature entry points (include/bsig_logsignature.h): the width and the words
table are host arithmetic, checked against Witt's formula and against the Lyndon words enumerated by their
definition (tests/logsig_cases.py: no Duval there); the argument checks come before any launch; the Python
mirror validates a channel list and a depth before it asks for a GPU; BayesSim sizes its first layer by the
log-signature's width."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import logsig_cases as LC
from bayes_sim_ig_amd import _lib, summarizers

CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_logsignature', 'trainTrajLen': 11, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)


def _err():
    return _lib.load().bsig_last_error().decode()


def _table(d, depth, capacity=None):
    width = _lib.load().bsig_logsignature_dim(d, depth)
    buf = (ctypes.c_int32 * max(width, 1))()
    rc = _lib.load().bsig_logsignature_words(d, depth, buf, width if capacity is None else capacity)
    return rc, list(buf)[:max(width, 0)]


@pytest.mark.parametrize('d,depth,sig,width', [(10, 4, 11110, 2860), (22, 3, 11154, 3795), (6, 5, 9330, 1960),
                                               (4, 6, 5460, 964), (2, 6, 126, 23), (110, 2, 12210, 6105)])
def test_width_is_witts_formula(d, depth, sig, width):
    assert LC.witt(d, depth) == width
    assert _lib.load().bsig_logsignature_dim(d, depth) == width
    assert summarizers.logsignature_dim(d, depth) == width
    assert summarizers.signature_dim(d, depth) == sig


def test_the_helper_knows_the_words_of_the_header():
    words = [''.join(map(str, w)) for w in LC.lyndon_words(2, 4)]
    assert words == ['0', '1', '01', '001', '011', '0001', '0011', '0111']


@pytest.mark.parametrize('d,depth', [(2, 6), (3, 4), (4, 6), (10, 4), (22, 3), (5, 1), (7, 2)])
def test_words_table_is_the_independent_enumeration(d, depth):
    words = LC.lyndon_words(d, depth)
    assert len(words) == LC.witt(d, depth)
    rc, table = _table(d, depth)
    assert rc == _lib.BSIG_OK, _err()
    assert table == [LC.word_offset(w, d) for w in words]
    assert summarizers.lyndon_words(d, depth) == words
    assert 0 <= min(table) and max(table) < summarizers.signature_dim(d, depth)


def test_a_short_capacity_and_bad_arguments_are_refused():
    lib = _lib.load()
    rc, _ = _table(3, 4, capacity=31)            # 32 words
    assert rc == _lib.BSIG_EINVAL and 'capacity' in _err()
    buf = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.bsig_logsignature_words(3, 4, buf, 4) == _lib.BSIG_EINVAL and list(buf) == [7] * 4     # untouched
    assert lib.bsig_logsignature_words(3, 4, None, 100) == _lib.BSIG_EINVAL
    for d, depth in [(1, 3), (3, 0), (3, 7), (100000, 2), (2 ** 31 - 1, 2)]:
        assert lib.bsig_signature_ex_dim(d, depth) == -1
        assert lib.bsig_logsignature_dim(d, depth) == -1
        assert lib.bsig_logsignature_words(d, depth, buf, 1 << 40) == _lib.BSIG_EINVAL
        with pytest.raises(ValueError):
            summarizers.logsignature_dim(d, depth)
        with pytest.raises(ValueError):
            summarizers.lyndon_words(d, depth)


def test_binding_lists_the_entry_points_and_the_seam_routes_them():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py)"""
    names = _lib.exported_symbols('bsig_logsignature.h')
    assert names == sorted(['bsig_logsignature', 'bsig_logsignature_dim', 'bsig_logsignature_f64',
                            'bsig_logsignature_words'])
    assert _lib.F32.symbol('logsignature') == 'bsig_logsignature'
    assert _lib.F64.symbol('logsignature') == 'bsig_logsignature_f64'
    assert B.summary_logsignature is summarizers.summary_logsignature
    assert B.logsignature_dim is summarizers.logsignature_dim and B.lyndon_words is summarizers.lyndon_words


@pytest.mark.parametrize('name', ['bsig_logsignature', 'bsig_logsignature_f64'])
def test_c_abi_argument_errors(name):
    """The BSIG_REQUIRE checks come before any launch: no GPU needed.  Arguments: states, actions, channels,
    n_channels, words, out, n, length, sd, ad, depth, ld_out, stream."""
    fn = getattr(_lib.load(), name)
    one = ctypes.c_void_p(8)          # never dereferenced on the host
    assert fn(one, one, None, 0, one, one, 1, 5, 2, 1, 7, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'depth' in _err()
    assert fn(one, one, None, 0, one, one, 1, 1, 2, 1, 4, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'length' in _err()
    assert fn(one, one, None, 0, None, one, 1, 5, 2, 1, 4, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'words' in _err()
    assert fn(one, one, None, 0, None, one, 1, 5, 2, 1, 0, 1 << 20, None) == _lib.BSIG_EINVAL   # d = 4: depth 3
    assert 'words' in _err()
    assert fn(one, one, None, 0, one, one, 1, 5, 2, 1, 4, 89, None) == _lib.BSIG_EINVAL          # width 90
    assert 'ld_out' in _err()
    assert fn(one, one, one, 3, one, one, 1, 5, 2, 1, 3, 29, None) == _lib.BSIG_EINVAL           # width 30
    assert 'ld_out' in _err()
    assert fn(one, one, one, 3, None, one, 1, 5, 2, 1, 1, 3, None) == _lib.BSIG_EINVAL           # depth 1: width 4
    assert 'ld_out' in _err()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert fn(args[0], args[1], None, 0, one, args[2], 1, 5, 2, 1, 4, 90, None) == _lib.BSIG_EINVAL
        assert 'null pointer' in _err()
    assert fn(one, one, one, 0, one, one, 1, 5, 2, 1, 4, 1 << 20, None) == _lib.BSIG_EINVAL
    assert 'n_channels' in _err()
    # refused, not spilled: 7^6 terms, the general signature kernel's answer
    assert fn(one, one, None, 0, one, one, 1, 5, 5, 1, 6, 1 << 20, None) == _lib.BSIG_EUNSUPPORTED
    assert 'LDS' in _err()
    assert _lib.load().bsig_signature_ex_fits(7, 5, 6, 4) == _lib.BSIG_EUNSUPPORTED
    # n = 0: nothing to do, nothing looked at
    assert fn(None, None, None, 0, None, None, 0, 1, 0, 0, 9, 0, None) == _lib.BSIG_OK


@pytest.mark.parametrize('dtype', [None, torch.float64])
def test_python_refuses_a_bad_channel_list_or_depth_before_it_asks_for_a_gpu(dtype, monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    states, actions = torch.zeros(2, 5, 3), torch.zeros(2, 5, 2)
    for bad in ([5], [-1], [0, 5], [], (), [0.5], ['a'], 3):
        with pytest.raises(ValueError):
            summarizers.summary_logsignature(states, actions, channels=bad, dtype=dtype)
    with pytest.raises(ValueError, match='depth'):
        summarizers.summary_logsignature(states, actions, depth=7, dtype=dtype)
    with pytest.raises(ValueError, match='depth'):
        summarizers.summary_logsignature(states, actions, depth=7, channels=[0], dtype=dtype)
    with pytest.raises(ValueError, match='float'):
        summarizers.summary_logsignature(states, actions, dtype=torch.float16)


def test_bayessim_sizes_its_first_layer_by_the_log_signature():
    pend = dict(obs_dim=3, act_dim=1, **KW)
    bs = B.BayesSim(model_cfg=dict(CFG, sigDepth=4, sigChannels=[0, 1, 3]), **pend)
    assert bs.model.input_dim == 90 == LC.witt(4, 4) and bs.summary_kwargs['channels'] == (0, 1, 3)
    assert bs.summarizer_fxn is B.summary_logsignature
    assert B.BayesSim(model_cfg=dict(CFG, sigDepth=5), **pend).model.input_dim == LC.witt(5, 5) == 829
    assert B.BayesSim(model_cfg=CFG, **pend).model.input_dim == LC.witt(5, 3) == 55           # default depth 3
    assert B.BayesSim(model_cfg=dict(CFG, sigDepth=1), **pend).model.input_dim == 5
    both = dict(CFG, sigDepth=4, dtype='float64', summaryDtype='float64')
    assert B.BayesSim(model_cfg=both, **pend).model.input_dim == LC.witt(5, 4) == 205
    picked = [0, 210, 211, 230] + list(range(5, 22))
    hand = B.BayesSim(model_cfg=dict(CFG, sigChannels=picked), obs_dim=211, act_dim=20, **KW)
    assert hand.model.input_dim == 3795
    # the whole ShadowHand path: depth 1 by the reference's rule, no LDS asked for, however long the path
    long = dict(CFG, trainTrajLen=100000)
    assert B.BayesSim(model_cfg=long, obs_dim=211, act_dim=20, **KW).model.input_dim == 232
    with pytest.raises(ValueError, match="applies to 'summary_signatory', not to 'summary_start'"):
        B.BayesSim(model_cfg=dict(CFG, summarizerFxn='summary_start', sigChannels=[0]), **pend)
    for bad in ([4], [], [0.5]):
        with pytest.raises(ValueError):
            B.BayesSim(model_cfg=dict(CFG, sigChannels=bad), **pend)
    for bad in (7, 0, -1):
        with pytest.raises(ValueError, match='sigDepth'):
            B.BayesSim(model_cfg=dict(CFG, sigDepth=bad), **pend)
    # refused at construction, by the general signature kernel's LDS arithmetic
    with pytest.raises(NotImplementedError, match='LDS'):
        B.BayesSim(model_cfg=dict(CFG, sigDepth=6), obs_dim=5, act_dim=1, **KW)
    with pytest.raises(NotImplementedError, match='LDS'):
        B.BayesSim(model_cfg=dict(CFG, sigDepth=4, trainTrajLen=4000), obs_dim=7, act_dim=2, **KW)


def test_the_series_of_the_helper_against_known_logs():
    """The helper's own footing, in exact rationals: a straight line's log-signature is its increment (every
    longer word 0), and two segments e_0 then e_1 give the Baker-Campbell-Hausdorff coefficients
    1/2, 1/12, 1/12, 0, 1/24, 0 at the words 01, 001, 011, 0001, 0011, 0111."""
    f = lambda rows: np.array([[[Fraction(v) for v in r] for r in rows]], dtype=object)
    line = LC.chen(f([[3, -2, 5]]), 4)
    got = LC.logsignature(line, 3, 4)[0]
    assert list(got[:3]) == [3, -2, 5] and all(v == 0 for v in got[3:])
    two = LC.chen(f([[1, 0], [0, 1]]), 4)
    assert list(LC.logsignature(two, 2, 4)[0]) == [1, 1, Fraction(1, 2), Fraction(1, 12), Fraction(1, 12), 0,
                                                   Fraction(1, 24), 0]
    # and the per-word sum over cuts -- what the kernel evaluates -- is the same number
    words = LC.lyndon_words(2, 4)
    for col, w in enumerate(words):
        total = Fraction(0)
        for pieces in LC.cuts(w):
            prod = Fraction(1)
            for u in pieces:
                prod *= two[0, LC.word_offset(u, 2)]
            total += prod * Fraction((-1) ** (len(pieces) + 1), len(pieces))
        assert total == LC.logsignature(two, 2, 4)[0, col], w
