"""CPU-side checks of the per-trajectory lengths of ``summary_xcorr`` and ``summary_kme`` (include/bsig_ragged.h):
the header's table and the seam's pairs; every argument check of the six entry points comes before any launch (the
pattern of tests/test_cabi_errors.py); Python validates ``lengths`` before a GPU is asked for; ``pairs.end_episodes``
against its numpy restatement; and the numpy references of tests/ragged_cases.py against a direct loop on
hand-sized trajectories, one of them with an empty lag block."""
import ctypes as C

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import kme_cases as KC
import ragged_cases as RC
import xcorr_cases as XC
from bayes_sim_ig_amd import _lib, summarizers
from bayes_sim_ig_amd.summarizer_table import SUMMARIZERS

FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
SYMBOLS = {'bsig_xcorr_ragged', 'bsig_xcorr_ragged_f64', 'bsig_kme_ragged', 'bsig_kme_ragged_f64',
           'bsig_kme_rows_ragged', 'bsig_kme_rows_ragged_f64'}
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_xcorr', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsig_last_error().decode()


# ------------------------------------------------------------------ the header, the seam
def test_the_headers_table_is_the_six_symbols_and_the_seam_routes_them(lib):
    table = _lib.HEADERS['bsig_ragged.h']
    assert set(table) == SYMBOLS == set(_lib.exported_symbols('bsig_ragged.h'))
    for op in ('xcorr_ragged', 'kme_ragged', 'kme_rows_ragged'):
        assert _lib.Precision.OPS[op] == ('bsig_' + op, 'bsig_%s_f64' % op)
        assert _lib.F32.symbol(op) == 'bsig_' + op and _lib.F64.symbol(op) == 'bsig_%s_f64' % op
        assert table['bsig_' + op] == table['bsig_%s_f64' % op]
        assert hasattr(lib, 'bsig_' + op) and hasattr(lib, 'bsig_%s_f64' % op)
    # the parents' argument lists with the lengths (and the offsets) behind the trajectories
    vp = _lib.vp
    xc, km, rows = (_lib.HEADERS[h][n][1] for h, n in (('bsig_xcorr.h', 'bsig_xcorr'), ('bsig_kme.h', 'bsig_kme'),
                                                      ('bsig_kme.h', 'bsig_kme_rows')))
    assert table['bsig_xcorr_ragged'][1] == xc[:2] + [vp] + xc[2:]
    assert table['bsig_kme_ragged'][1] == km[:2] + [vp] + km[2:]
    assert table['bsig_kme_rows_ragged'][1] == rows[:2] + [vp, vp] + rows[2:]
    assert [SUMMARIZERS[name].ragged for name in sorted(SUMMARIZERS)] == \
        [name in ('summary_xcorr', 'summary_kme') for name in sorted(SUMMARIZERS)]


# ------------------------------------------------------------------ the C ABI's argument checks
@pytest.mark.parametrize('fn', ['bsig_xcorr_ragged', 'bsig_xcorr_ragged_f64'])
def test_xcorr_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = fn[5:]
    # (states, actions, lengths, out, n, ts, ta, sd, ad, max_lag, state_diff, ld_out, nonfinite, stream)
    rc = call(FAKE, FAKE, FAKE, FAKE, 4, 1, 1, 3, 1, 0, 1, 12, None, None)
    assert rc == _lib.BSIG_EINVAL and 'M = 0' in err(lib) and err(lib).startswith(what + ':')
    assert call(FAKE, FAKE, FAKE, FAKE, 4, 0, 1, 3, 1, 0, 0, 12, None, None) == _lib.BSIG_EINVAL and 'ts' in err(lib)
    assert call(FAKE, FAKE, FAKE, FAKE, 4, 21, 0, 3, 1, 0, 1, 12, None, None) == _lib.BSIG_EINVAL and 'ta' in err(lib)
    assert call(FAKE, FAKE, FAKE, FAKE, 4, 21, 21, 0, 1, 0, 1, 12, None, None) == _lib.BSIG_EINVAL and 'sd' in err(lib)
    assert call(FAKE, FAKE, FAKE, FAKE, 4, 21, 21, 3, 0, 0, 1, 12, None, None) == _lib.BSIG_EINVAL and 'ad' in err(lib)
    # max_lag against the M of ts: 20 under state_diff
    for lag in (-1, 20):
        rc = call(FAKE, FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, lag, 1, 80, None, None)
        assert rc == _lib.BSIG_EINVAL and 'max_lag' in err(lib) and '0..19' in err(lib)
    rc = call(FAKE, FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 0, 1, 8, None, None)                       # width 9
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    for args in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, FAKE, None)):
        rc = call(*args, 4, 21, 21, 3, 1, 0, 1, 12, None, None)
        assert rc == _lib.BSIG_EINVAL and 'null pointer' in err(lib)
    rc = call(FAKE, FAKE, None, FAKE, 4, 21, 21, 3, 1, 0, 1, 12, None, None)
    assert rc == _lib.BSIG_EINVAL and 'null lengths' in err(lib) and err(lib).startswith(what + ':')
    assert call(FAKE, FAKE, FAKE, FAKE, -1, 21, 21, 3, 1, 0, 1, 12, None, None) == _lib.BSIG_EINVAL and 'n=' in err(lib)
    # the cover is that of the fixed-length launch at ts: the same code and message
    itemsize = 8 if fn.endswith('f64') else 4
    for ts in (88, 89, 177, 178):
        want = lib.bsig_xcorr_fits(ts, ts, 211, 20, 1, 1, itemsize)
        message = err(lib) if want else ''
        rc = call(FAKE if want else None, FAKE, FAKE, FAKE, 4, ts, ts, 211, 20, 1, 1, 8864, None, None)
        if want:
            assert rc == want == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
            assert err(lib).split(':', 1)[1] == message.split(':', 1)[1]
        else:
            assert rc == _lib.BSIG_EINVAL and 'null pointer' in err(lib)      # covered: the next check speaks
    rc = call(FAKE, FAKE, FAKE, FAKE, 4, 600, 600, 3, 1, 256, 1, 1040, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'max_lag' in err(lib)
    # an empty batch is fine and touches nothing, whatever else is passed
    assert call(None, None, None, None, 0, 21, 21, 3, 1, 0, 1, 12, None, None) == _lib.BSIG_OK
    assert call(None, None, None, None, 0, 1, 1, 3, 1, 5, 1, 0, None, None) == _lib.BSIG_OK


@pytest.mark.parametrize('fn', ['bsig_kme_ragged', 'bsig_kme_ragged_f64'])
def test_kme_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = fn[5:]
    # (states, actions, lengths, coeff, ld_coeff, out, n, ts, ta, sd, ad, m, diff, time, ld_out, nonfinite, stream)
    rc = call(FAKE, FAKE, FAKE, FAKE, 8, FAKE, 4, 1, 1, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'M = 0' in err(lib) and err(lib).startswith(what + ':')
    for bad, word in (((0, 1, 3, 1, 16, 0), 'ts'), ((21, 0, 3, 1, 16, 1), 'ta'), ((21, 21, 0, 1, 16, 1), 'sd'),
                      ((21, 21, 3, 0, 16, 1), 'ad'), ((21, 21, 3, 1, 0, 1), 'm 0')):
        rc = call(FAKE, FAKE, FAKE, FAKE, 8, FAKE, 4, *bad, 0, 32, None, None)
        assert rc == _lib.BSIG_EINVAL and word in err(lib), bad
    rc = call(FAKE, FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 21, 3, 1, 16, 1, 0, 31, None, None)             # width 32
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    rc = call(FAKE, FAKE, FAKE, FAKE, 6, FAKE, 4, 21, 21, 3, 1, 16, 1, 0, 32, None, None)             # d = 7
    assert rc == _lib.BSIG_EINVAL and 'ld_coeff' in err(lib)
    for args in ((None, FAKE, FAKE, FAKE, 8, FAKE), (FAKE, None, FAKE, FAKE, 8, FAKE),
                 (FAKE, FAKE, FAKE, None, 8, FAKE), (FAKE, FAKE, FAKE, FAKE, 8, None)):
        rc = call(*args, 4, 21, 21, 3, 1, 16, 1, 0, 32, None, None)
        assert rc == _lib.BSIG_EINVAL and 'null pointer' in err(lib)
    rc = call(FAKE, FAKE, None, FAKE, 8, FAKE, 4, 21, 21, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'null lengths' in err(lib) and err(lib).startswith(what + ':')
    rc = call(FAKE, FAKE, FAKE, FAKE, 8, FAKE, -1, 21, 21, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'n=' in err(lib)
    # the cover is bsig_kme_fits': one block beyond the LDS, the same message
    itemsize = 8 if fn.endswith('f64') else 4
    assert lib.bsig_kme_fits(50, 50, 800, 73, 16, 1, 0, itemsize) == _lib.BSIG_EUNSUPPORTED
    message = err(lib)
    rc = call(FAKE, FAKE, FAKE, FAKE, 2048, FAKE, 4, 50, 50, 800, 73, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib) and err(lib).split(':', 1)[1] == message.split(':', 1)[1]
    assert call(None, None, None, None, 0, None, 0, 21, 21, 3, 1, 16, 1, 0, 32, None, None) == _lib.BSIG_OK
    assert call(None, None, None, None, 0, None, 0, 1, 1, 3, 1, 0, 1, 0, 0, None, None) == _lib.BSIG_OK


@pytest.mark.parametrize('fn', ['bsig_kme_rows_ragged', 'bsig_kme_rows_ragged_f64'])
def test_rows_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = fn[5:]
    # (states, actions, lengths, offsets, rows, n, ts, ta, sd, ad, diff, time, ld_rows, stream)
    rc = call(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 1, 1, 3, 1, 1, 0, 8, None)
    assert rc == _lib.BSIG_EINVAL and 'M = 0' in err(lib) and err(lib).startswith(what + ':')
    for bad, word in (((0, 1, 3, 1, 0), 'ts'), ((21, 0, 3, 1, 1), 'ta'), ((21, 21, 0, 1, 1), 'sd'),
                      ((21, 21, 3, 0, 1), 'ad')):
        assert call(FAKE, FAKE, FAKE, FAKE, FAKE, 4, *bad, 0, 8, None) == _lib.BSIG_EINVAL and word in err(lib), bad
    rc = call(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 1, 0, 6, None)
    assert rc == _lib.BSIG_EINVAL and 'ld_rows' in err(lib)
    for args in ((None, FAKE, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE, FAKE), (FAKE, FAKE, FAKE, FAKE, None)):
        assert call(*args, 4, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'null pointer' in err(lib)
    rc = call(FAKE, FAKE, None, FAKE, FAKE, 4, 21, 21, 3, 1, 1, 0, 8, None)
    assert rc == _lib.BSIG_EINVAL and 'null lengths' in err(lib)
    rc = call(FAKE, FAKE, FAKE, None, FAKE, 4, 21, 21, 3, 1, 1, 0, 8, None)
    assert rc == _lib.BSIG_EINVAL and 'null offsets' in err(lib)
    assert call(FAKE, FAKE, FAKE, FAKE, FAKE, -1, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'n=' in err(lib)
    assert call(None, None, None, None, None, 0, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_OK


# ------------------------------------------------------------------ Python: before a GPU is asked for
def _calls():
    """Every way lengths reach a summarizer directly: (what, call(lengths), Lmin)."""
    states, actions = torch.zeros(5, 21, 3), torch.zeros(5, 21, 1)
    emb = B.KernelMeanEmbedding(3, 1, n_feat=16).set_scale(np.ones(7))
    raw = B.KernelMeanEmbedding(3, 1, n_feat=16, diff=False).set_scale(np.ones(4))
    return [
        ('xcorr', lambda lengths: B.summary_xcorr(states, actions, max_lag=2, lengths=lengths), 2),
        ('xcorr raw', lambda lengths: B.summary_xcorr(states, actions, state_diff=False, lengths=lengths), 1),
        ('kme', lambda lengths: B.summary_kme(states, actions, emb, lengths=lengths), 2),
        ('kme raw', lambda lengths: raw(states, actions, lengths=lengths), 1),
        ('kme rows', lambda lengths: emb.rows(states, actions, lengths=lengths), 2),
        ('kme fit_scale', lambda lengths: emb.fit_scale(states, actions, lengths=lengths), 2),
    ]


def test_lengths_are_validated_before_any_gpu_call():
    for what, call, lmin in _calls():
        for bad in ([21] * 4, [21] * 6, [[21] * 5], np.full((5, 1), 21), torch.full((1, 5), 21), 21):
            with pytest.raises(ValueError, match=r'one value per trajectory, shape \(5,\)'):
                call(bad)
        for bad in ([21.0] * 5, np.full(5, 21.0), torch.full((5,), 21.0), np.full(5, True), torch.full((5,), 21,
                                                                                                     dtype=torch.int16)):
            with pytest.raises(ValueError, match='must hold integers'):
                call(bad)
        # on the host: the range, the first index outside named
        for kind in (list, np.asarray, lambda v: torch.tensor(v, dtype=torch.int32),
                     lambda v: torch.tensor(v, dtype=torch.int64)):
            with pytest.raises(ValueError, match=r'lengths\[2\] = 22 is outside %d\.\.21' % lmin):
                call(kind([21, lmin, 22, 0, 21]))
            with pytest.raises(ValueError, match=r'lengths\[1\] = %d is outside %d\.\.21' % (lmin - 1, lmin)):
                call(kind([21, lmin - 1, 22, 0, 21]))
            with pytest.raises(ValueError, match=r'lengths\[4\] = -3 is outside'):
                call(kind([21, lmin, 20, 5, -3]))


def test_check_lengths_returns_what_the_kernels_take():
    got = summarizers.check_lengths([21, 2, 3], 3, 21, True)
    assert got.dtype == torch.int32 and got.tolist() == [21, 2, 3] and not got.is_cuda
    assert summarizers.check_lengths(np.array([1, 5], dtype=np.uint8), 2, 5, False).tolist() == [1, 5]
    assert summarizers.check_lengths(torch.tensor([4, 5]), 2, 5, True).dtype == torch.int32
    assert tuple(summarizers.check_lengths([], 0, 5, True).shape) == (0,)      # an empty batch
    with pytest.raises(ValueError, match=r'traj_lengths\[0\]'):
        summarizers.check_lengths([1], 1, 5, True, name='traj_lengths')


def _bayes_sim(cfg):
    return B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, **KW)


def test_bayessim_refuses_lengths_for_a_summarizer_that_takes_none():
    theta, states, actions = torch.zeros(5, 2), torch.zeros(5, 21, 3), torch.zeros(5, 21, 1)
    lengths = [21] * 5
    for name in sorted(set(SUMMARIZERS) - {'summary_xcorr', 'summary_kme'}):
        bs = _bayes_sim(dict(CFG, summarizerFxn=name))
        message = "lengths apply to 'summary_xcorr' and 'summary_kme', not to '%s'" % name
        for call in (lambda: bs.fit(theta, states, actions, traj_lengths=lengths),
                     lambda: bs.fit(theta, states, actions, lengths),
                     lambda: bs.run_training(theta, states, actions, traj_lengths=lengths),
                     lambda: bs.predict(states, actions, lengths=lengths),
                     lambda: bs.predict(states, actions, 0.005, lengths)):
            with pytest.raises(ValueError) as caught:
                call()
            assert str(caught.value) == message
    bs = _bayes_sim(dict(CFG, summarizerFxn='summary_start', inputNorm=True))
    with pytest.raises(ValueError, match='lengths apply to'):
        bs.fit_input_norm(states, actions, lengths=lengths)
    bs = _bayes_sim(dict(CFG, summarizerFxn='summary_start', modelClass='MDRFF_RBF_median'))
    with pytest.raises(ValueError, match='lengths apply to'):
        bs.fit_rff_bandwidth(states, actions, lengths=lengths)


@pytest.mark.parametrize('name', ['summary_xcorr', 'summary_kme'])
def test_bayessim_validates_lengths_and_hands_them_on_only_when_given(name):
    theta, states, actions = torch.zeros(5, 2), torch.zeros(5, 21, 3), torch.zeros(5, 21, 1)
    bs = _bayes_sim(dict(CFG, summarizerFxn=name))
    if bs.embedding is not None:
        bs.embedding.set_scale(np.ones(7))
    for call in (lambda v: bs.fit(theta, states, actions, traj_lengths=v),
                 lambda v: bs.run_training(theta, states, actions, traj_lengths=v),
                 lambda v: bs.predict(states, actions, lengths=v)):
        with pytest.raises(ValueError, match=r'shape \(5,\)'):
            call([21] * 4)
        with pytest.raises(ValueError, match='must hold integers'):
            call([21.0] * 5)
        with pytest.raises(ValueError, match=r'lengths\[3\] = 1 is outside 2\.\.21'):
            call([21, 2, 3, 1, 21])
    if bs.embedding is not None:
        with pytest.raises(ValueError, match=r'lengths\[0\] = 22'):
            bs.fit_embedding_scale(states, actions, lengths=[22] * 5)
    # what reaches the summarizer: lengths=None is the call it always was, no new keyword
    calls = []
    bs.summarizer_fxn = lambda *args, **kw: (calls.append(kw), torch.zeros(5, bs.model.input_dim))[1]
    bs._summarize(states, actions)
    bs._summarize(states, actions, lengths=None)
    bs._summarize(states, actions, lengths=[21, 2, 3, 4, 5])
    assert 'lengths' not in calls[0] and calls[0] == calls[1] == bs.summary_kwargs
    assert calls[2]['lengths'].tolist() == [21, 2, 3, 4, 5] and calls[2]['lengths'].dtype == torch.int32
    assert {k: v for k, v in calls[2].items() if k != 'lengths'} == calls[0]


# ------------------------------------------------------------------ end_episodes
def test_end_episodes_is_its_numpy_restatement():
    states, actions = XC.trajectories(6, 9, 8, 3, 2)
    lengths = np.array([9, 2, 3, 8, 5, 9])
    got_s, got_a = B.pairs.end_episodes(torch.from_numpy(states), torch.from_numpy(actions), lengths)
    want_s, want_a = RC.end_episodes(states, actions, lengths)
    assert np.array_equal(got_s.numpy(), want_s) and np.array_equal(got_a.numpy(), want_a)
    assert got_s.data_ptr() != torch.from_numpy(states).data_ptr()      # copies
    for i, length in enumerate(lengths):
        assert np.array_equal(want_s[i, :length], states[i, :length])
        assert (want_s[i, length:] == states[i, length - 1]).all()
        assert np.array_equal(want_a[i, :min(length - 1, 8)], actions[i, :min(length - 1, 8)])
        assert (want_a[i, length - 1:] == actions[i, length - 2]).all()
    same = B.pairs.end_episodes(torch.from_numpy(states), torch.from_numpy(actions), torch.tensor([9] * 6))
    assert np.array_equal(same[0].numpy(), states) and np.array_equal(same[1].numpy(), actions)
    with pytest.raises(AssertionError):
        B.pairs.end_episodes(torch.from_numpy(states), torch.from_numpy(actions), [1] * 6)


# ------------------------------------------------------------------ the numpy references
def _xcorr_by_hand(states, actions, length, k, diff):
    s = np.asarray(states, dtype=np.float64)[:length]
    a = np.asarray(actions, dtype=np.float64)
    f = s[1:] - s[:-1] if diff else s
    m, sd, ad = f.shape[0], s.shape[1], a.shape[1]
    row = []
    for tau in range(k + 1):
        for i in range(sd):
            for j in range(ad):
                terms = [f[t + tau, i] * a[min(t, a.shape[0] - 1), j] for t in range(m - tau)]
                row.append(sum(terms) / (m - tau) if terms else 0.0)
    mu = [sum(f[:, i]) / m for i in range(sd)]
    sigma = [np.sqrt(sum((f[:, i] - mu[i]) ** 2) / m) for i in range(sd)]
    return np.array(row + mu + sigma)


def test_the_xcorr_reference_agrees_with_a_direct_loop_and_an_empty_lag_block_is_zero():
    states, actions = XC.trajectories(2, 6, 3, 2, 2)
    lengths, k = np.array([6, 3]), 2                       # the second: M = 2, lag 2 has no term
    for diff in (True, False):
        ref = RC.xcorr_reference(states, actions, lengths, k, diff)
        bound = RC.xcorr_bounds(states, actions, lengths, k, diff, XC.U32)
        assert ref.shape == bound.shape == (2, XC.width(2, 2, k))
        for i in range(2):
            np.testing.assert_allclose(ref[i], _xcorr_by_hand(states[i], actions[i], lengths[i], k, diff),
                                       rtol=1e-13, atol=1e-15)
        full = XC.reference(states[:1], actions[:1], k, diff)
        assert np.array_equal(ref[0], full[0])              # L = ts: the fixed-length row
    ref = RC.xcorr_reference(states, actions, lengths, k, True)
    bound = RC.xcorr_bounds(states, actions, lengths, k, True, XC.U32)
    assert (ref[1, 8:12] == 0).all() and (bound[1, 8:12] == 0).all()        # c_2 of the short one
    assert (ref[1, :8] != 0).all() and (bound[1, :8] > 0).all() and (bound[0] > 0).all()
    # padding changes the statistic: the summary of the padded episode is not the summary at its length
    padded = RC.end_episodes(states, actions, lengths)
    assert not np.allclose(XC.reference(padded[0][1:], padded[1][1:], 1, True)[0, -4:], ref[1, -4:])


def test_the_kme_reference_agrees_with_a_direct_loop():
    states, actions = KC.trajectories(2, 5, 2, 2, 1)
    lengths = np.array([5, 3])
    coeff = np.random.RandomState(3).standard_normal((3, 6))           # [tau | s s | a | ds ds]
    ref = RC.kme_reference(states, actions, lengths, coeff, True, True)
    bound = RC.kme_bounds(states, actions, lengths, coeff, True, True, 4)
    assert ref.shape == bound.shape == (2, 6) and (bound > 0).all() and (bound < 1e-5).all()
    for i, length in enumerate(lengths):
        s, a = states[i].astype(np.float64), actions[i].astype(np.float64)
        m = length - 1
        cs, sn = np.zeros(3), np.zeros(3)
        for t in range(m):
            x = np.concatenate([[t / max(m - 1, 1)], s[t], a[min(t, 1)], s[t + 1] - s[t]])
            cs += np.cos(coeff @ x)
            sn += np.sin(coeff @ x)
        np.testing.assert_allclose(ref[i], np.concatenate([cs, sn]) * np.sqrt(1.0 / 3) / m, rtol=1e-13)
    rows = RC.kme_rows_compacted(states, actions, lengths, True, True)
    assert rows.shape == (4 + 2, 6)
    assert np.array_equal(rows[:4], KC.rows(states[:1], actions[:1], True, True)[0])
    assert rows[4:, 0].tolist() == [0.0, 1.0]                           # tau runs to 1 at the episode's own end
    assert RC.kme_rows_compacted(states, actions, lengths, True, True, np.float32).dtype == np.float32


def test_the_seeded_lengths_hold_what_a_case_is_about():
    for kind, cases in (('xcorr', RC.XCORR), ('kme', RC.KME)):
        for name, n in cases.items():
            ts, _, _, _, diff, lmin = RC.shape_of(kind, name)
            n = 11 if n is None else n
            lengths = RC.lengths_for(name, n, kind)
            assert np.array_equal(lengths, RC.lengths_for(name, n, kind)) and lengths.shape == (n,)
            assert lengths.min() >= lmin and lengths.max() <= ts
            assert {lmin, ts, min(lmin + 1, ts)} <= set(lengths.tolist()), (kind, name)
            if kind == 'xcorr' and XC.CASES[name][5] >= 1:
                assert (RC.steps_of(lengths, diff) <= XC.CASES[name][5]).any(), name
            if ts - lmin >= 4 and (kind, name) not in RC._FIRST:
                mid = (lmin + ts) // 2
                for i in range(4, n - 1):
                    assert (lengths[i] <= mid) != (lengths[i + 1] <= mid), (kind, name, i)
    steps = set(RC.steps_of(RC.lengths_for('edge_ts66', 7, 'kme'), True).tolist())
    assert {1, 31, 32, 33, 64, 65} <= steps
    blocks = {-(-m // 32) for m in RC.steps_of(RC.lengths_for('shadowhand_long', 4, 'kme'), True)}
    assert blocks == {1, 2, 4}
