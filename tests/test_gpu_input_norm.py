"""GPU checks of the input standardisation (include/bsig_input_norm.h, MDNN(input_norm=True),
model_cfg['inputNorm']): the statistics kernels against the long-double two-pass definition of
tests/input_norm_cases.py within bounds derived from Welford's recurrence in double, the apply kernel against the
header's arithmetic bit for bit, and the model / BayesSim layers against a plain model on hand-standardised rows
and against the oracle.

Bounds of the statistics (not measured: Welford in double adds at most a few roundings of 2^-53 per row to a
column's mean and M2, Chan's merge a few per slab):
    |mean - ref| <= 4 n 2^-53 (|mean| + max_i |x_i|),     |std - ref| <= 8 n 2^-53 (std + |mean|)
where std is 1 / inv_std of a kept column; a flat column has inv_std == 0 exactly."""
import contextlib

import numpy as np
import pytest
import torch

import input_norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@pytest.fixture(autouse=True)
def _eps_guard():
    import bayes_sim_ig_amd as pkg
    old = pkg.MDNN.EPS_NOISE
    yield
    pkg.MDNN.EPS_NOISE = old


@contextlib.contextmanager
def default_f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _prec(B, dtype):
    return B._lib.F64 if np.dtype(dtype) == np.float64 else B._lib.F32


def _bits(t):
    """A device tensor's bit patterns on the host (NaN paddings compare equal to themselves)."""
    t = t.contiguous().cpu()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32).numpy()


def _pitched(x, ld):
    """x[n, width] in a device buffer of pitch ld whose padding columns are NaN."""
    dtype = torch.float64 if x.dtype == np.float64 else torch.float32
    buf = torch.full((x.shape[0], ld), NAN, dtype=dtype, device=DEV)
    buf[:, :x.shape[1]] = torch.from_numpy(x.copy()).to(DEV)
    return buf


def _device_stats(B, buf, ld, n, width, dtype):
    """(mean, inv_std) of the kernel: double [width + 3] with NaN behind the width."""
    _lib = B._lib
    mean = torch.full((width + 3,), NAN, dtype=torch.float64, device=DEV)
    inv = torch.full((width + 3,), NAN, dtype=torch.float64, device=DEV)
    need = int(_lib.load().bsig_input_norm_workspace_bytes(n, width))
    ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    _prec(B, dtype).input_norm_stats(_lib.ptr(buf), ld, n, width, _lib.ptr(mean), _lib.ptr(inv), _lib.ptr(ws),
                                     need, _lib.stream())
    return mean, inv


# ------------------------------------------------------------------ 1. statistics
@pytest.mark.parametrize('width', NC.WIDTH_CASES)
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_statistics_against_the_long_double_definition(B, dtype, width):
    for n in NC.N_CASES:
        x = NC.rows(n, width, dtype)
        ref_mean, ref_std, ref_flat = NC.reference(n, width, dtype)
        assert NC.clear_of_the_threshold(x, ref_mean, ref_std, ref_flat), (n, width)
        x_max = np.abs(x).max(axis=0).astype(np.longdouble)
        mean_bound = 4 * n * NC.U53 * (np.abs(ref_mean) + x_max)
        std_bound = 8 * n * NC.U53 * (ref_std + np.abs(ref_mean))
        first = None
        for kind in NC.PITCH_CASES:
            ld = NC.pitch(kind, width, dtype)
            buf = _pitched(x, ld)
            mean, inv = _device_stats(B, buf, ld, n, width, dtype)
            again = _device_stats(B, buf, ld, n, width, dtype)
            what = (dtype, n, width, kind)
            assert np.array_equal(_bits(mean), _bits(again[0])) and np.array_equal(_bits(inv), _bits(again[1])), what
            mean, inv = mean.cpu().numpy(), inv.cpu().numpy()
            assert np.isnan(mean[width:]).all() and np.isnan(inv[width:]).all(), what      # nothing behind the width
            mean, inv = mean[:width], inv[:width]
            err = np.abs(mean.astype(np.longdouble) - ref_mean)
            some = mean_bound > 0
            print('%s: max mean error / bound %.3g' % (what, float((err[some] / mean_bound[some]).max()) if some.any() else 0.0))
            assert (err <= mean_bound).all(), (what, 'mean', int(np.argmax(err - mean_bound)))
            assert np.array_equal(inv == 0.0, ref_flat), (what, 'flat', np.nonzero((inv == 0.0) != ref_flat)[0][:8])
            kept = ~ref_flat
            assert np.isfinite(inv).all() and (inv[kept] > 0).all(), what
            err = np.abs(1.0 / inv[kept].astype(np.longdouble) - ref_std[kept])
            assert (err <= std_bound[kept]).all(), (what, 'std')
            # the pitch decides the path (16-byte groups or single elements), not the result: one chain per column
            if first is None:
                first = (mean, inv)
            assert np.array_equal(mean, first[0]) and np.array_equal(inv, first[1]), what


# ------------------------------------------------------------------ 2. apply
def _apply(B, src, ld_x, mean, inv, dst, ld_out, n, width, dtype):
    _lib = B._lib
    _prec(B, dtype).input_norm_apply(_lib.ptr(src), ld_x, _lib.ptr(mean), _lib.ptr(inv), _lib.ptr(dst), ld_out,
                                     n, width, _lib.stream())


def _check_apply(B, x, dtype, pitch_x, pitch_out):
    """Out of place (pitch_out a pitch kind) or in place (pitch_out None), against numpy on the kernel's own
    statistics, bit for bit; paddings untouched."""
    n, width = x.shape
    ld_x = NC.pitch(pitch_x, width, dtype)
    src = _pitched(x, ld_x)
    mean, inv = _device_stats(B, src, ld_x, n, width, dtype)
    want = NC.apply(x, mean[:width].cpu().numpy(), inv[:width].cpu().numpy())
    flat = inv[:width].cpu().numpy() == 0.0
    what = (dtype, n, width, pitch_x, pitch_out)
    if pitch_out is None:
        dst, ld_out = src, ld_x
    else:
        ld_out = NC.pitch(pitch_out, width, dtype)
        dst = torch.full((n, ld_out), NAN, dtype=src.dtype, device=DEV)
        before = _bits(src)
    _apply(B, src, ld_x, mean, inv, dst, ld_out, n, width, dtype)
    got = dst.cpu().numpy()
    assert np.array_equal(_bits(dst[:, :width]), want.view(np.int64 if want.itemsize == 8 else np.int32)), what
    assert (got[:, :width][:, flat] == 0).all(), what
    assert np.isnan(got[:, width:]).all(), what                     # the row padding of out: as it was
    if pitch_out is not None:
        assert np.array_equal(_bits(src), before), what            # x: read only


@pytest.mark.parametrize('width', NC.WIDTH_CASES)
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_apply_is_the_stated_arithmetic_bit_for_bit(B, dtype, width):
    for n in (1, 2, NC.SLAB + 3, 800):
        x = NC.rows(n, width, dtype)
        for pitch_x, pitch_out in (('tight', 'tight'), ('aligned', 'aligned'), ('odd', 'odd'), ('aligned', 'odd'),
                                   ('odd', 'aligned'), ('tight', None), ('aligned', None), ('odd', None)):
            _check_apply(B, x, dtype, pitch_x, pitch_out)


@pytest.mark.parametrize('width,pitch', [(4, 'aligned'), (5, 'aligned'), (5, 'odd')])
def test_apply_strides_over_more_rows_than_it_has_workgroups(B, width, pitch):
    """One column tile: the launch has at most 8192 row lanes, and a lane takes its rows in groups of four, the
    next group loaded while the current one is converted.  13 * 8192 + 3 rows give every lane three whole groups
    (the pipelined loop runs twice) and the first three lanes one more row."""
    x = NC.rows(13 * 8192 + 3, width, 'float32')
    _check_apply(B, x, 'float32', pitch, pitch)
    _check_apply(B, x, 'float32', pitch, None)


def test_apply_refuses_overlap_and_takes_no_rows(B):
    x = _pitched(NC.rows(8, 5, 'float32'), 8)
    mean, inv = _device_stats(B, x, 8, 8, 5, 'float32')
    before = _bits(x)
    with pytest.raises(AssertionError, match='overlaps'):
        _apply(B, x, 8, mean, inv, x[1:], 8, 7, 5, 'float32')
    _apply(B, x, 8, mean, inv, x, 8, 0, 5, 'float32')               # n == 0
    assert np.array_equal(_bits(x), before)


# ------------------------------------------------------------------ 3. the model
N_PAIRS, N_TRAIN, N_UPDATES, BATCH = 1000, 800, 20, 50
CASES = {                                   # summarizer, keywords, state_dim, action_dim
    'start': ('summary_start', {}, 5, 2),
    'sig3': ('summary_signatory', {'depth': 3}, 3, 1),
    'sig3_wide': ('summary_signatory', {'depth': 3}, 4, 1),
    'corrdiff': ('summary_corrdiff', {}, 4, 1),
}
IDS = np.random.RandomState(5).randint(0, N_TRAIN, (N_UPDATES, BATCH))


def _pairs(sd, ad, n=N_PAIRS, t=11, d=2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    theta = torch.rand(n, d, generator=gen)
    states = torch.randn(n, t, sd, generator=gen) * 0.3 + theta[:, None, :1]
    actions = torch.rand(n, t, ad, generator=gen)
    return theta, states, actions


def _summaries(B, case, dtype=None):
    name, kw, sd, ad = CASES[case]
    theta, states, actions = _pairs(sd, ad)
    if dtype == torch.float64:
        kw = dict(kw, dtype=dtype)
        states, actions = states.double(), actions.double()
    return getattr(B, name)(states.to(DEV), actions.to(DEV), **kw).contiguous(), theta.to(DEV)


def _model(B, kind, width, input_norm, seed=7):
    kw = dict(input_dim=width, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
              full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, device=DEV)
    if input_norm:
        kw['input_norm'] = True
    torch.manual_seed(seed)
    if kind.startswith('mdrff'):
        freqs = np.random.RandomState(9).randn(32, width).astype(np.float32)
        m = B.MDRFF(n_feat=64, sigma=4.0, kernel='RBF', freqs=freqs, **kw)
    else:
        m = B.MDNN(hidden_layers=(16, 16), **kw)
    return m.double() if kind.endswith('f64') else m


def _train(m, x, theta):
    return m.run_training(x, theta, N_UPDATES, BATCH, ids_table=IDS)


@pytest.mark.parametrize('kind', ['mdnn', 'mdrff', 'mdnn_f64', 'mdrff_f64'])
@pytest.mark.parametrize('case', ['start', 'sig3'])
def test_the_model_standardises_what_it_says(B, case, kind):
    B.MDNN.EPS_NOISE = 0.0
    x, theta = _summaries(B, case, torch.float64 if kind.endswith('f64') else None)
    width = x.shape[1]
    # (a) input_norm on x == a plain model of the same initialisation on normalize_inputs(x)
    a = _model(B, kind, width, True)
    assert not a.input_norm_ready
    logs_a = _train(a, x, theta)
    assert a.input_norm_ready and int(a.input_norm.count) == N_TRAIN
    xn = a.normalize_inputs(x)
    assert xn.dtype == x.dtype and xn.shape == x.shape
    plain = _model(B, kind, width, False)
    logs_plain = _train(plain, xn, theta)
    assert np.isfinite(logs_a['train_loss'] + logs_a['test_loss']).all()
    assert logs_a == logs_plain and torch.equal(a._flat, plain._flat)
    # the statistics are those of the call's training rows, nothing else; a second call does not refit
    c = _model(B, kind, width, True).fit_input_norm(x[:N_TRAIN])
    for name in ('mean', 'inv_std', 'count'):
        assert torch.equal(getattr(c.input_norm, name), getattr(a.input_norm, name)), name
    # they are the definition's: the long-double statistics of those rows, by the bounds at the top
    ref_mean, ref_std, ref_flat = NC.reference_stats(x[:N_TRAIN].cpu().numpy())
    mean, inv = a.input_norm.mean.cpu().numpy(), a.input_norm.inv_std.cpu().numpy()
    assert np.array_equal(inv == 0.0, ref_flat)
    assert (np.abs(mean - ref_mean) <= 4 * N_TRAIN * NC.U53 * 2 * np.abs(x[:N_TRAIN].cpu().numpy()).max(axis=0)).all()
    # forward / predict_MoGs standardise too: the plain model on xn
    fa, fp = a.forward(x[N_TRAIN:N_TRAIN + 3]), plain.forward(xn[N_TRAIN:N_TRAIN + 3])
    c.load_state_dict(a.state_dict())
    fc = c.forward(x[N_TRAIN:N_TRAIN + 3])
    for u, v, w in zip(fa, fp, fc):
        assert (u is None and v is None) or (torch.equal(u, v) and torch.equal(u, w))
    # a later call, on other training rows, does not refit
    before = [getattr(a.input_norm, name).clone() for name in ('mean', 'inv_std', 'count')]
    _train(a, x.flip(0).contiguous(), theta.flip(0).contiguous())
    for u, name in zip(before, ('mean', 'inv_std', 'count')):
        assert torch.equal(u, getattr(a.input_norm, name)), name
    # (b) set_input_norm(zeros, ones) is the plain model on x
    b = _model(B, kind, width, True).set_input_norm(np.zeros(width), np.ones(width))
    logs_b = _train(b, x, theta)
    raw = _model(B, kind, width, False)
    logs_raw = _train(raw, x, theta)
    assert logs_b == logs_raw and torch.equal(b._flat, raw._flat)
    assert logs_b != logs_a


def test_crosscorr_factor_rows_are_materialised_for_a_model_that_standardises(B):
    B.MDNN.EPS_NOISE = 0.0
    name, kw, sd, ad = CASES['corrdiff']
    theta, states, actions = _pairs(sd, ad)
    lazy = B.summary_corrdiff(states.to(DEV), actions.to(DEV), lazy=True)
    x = B.summary_corrdiff(states.to(DEV), actions.to(DEV))
    a, b = _model(B, 'mdnn', x.shape[1], True), _model(B, 'mdnn', x.shape[1], True)
    logs_a, logs_b = _train(a, lazy, theta.to(DEV)), _train(b, x, theta.to(DEV))
    assert logs_a == logs_b and torch.equal(a._flat, b._flat)
    assert torch.equal(a.input_norm.mean, b.input_norm.mean)


# ------------------------------------------------------------------ 4. parity with the oracle
def _oracle(B, kind, model, width, freqs_perm=None, perm=None, double=False):
    from oracle import estimators as oest
    kw = dict(input_dim=width, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
              full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, eps_noise=0.0)
    w0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if not k.startswith('input_norm.')}
    if double:
        w0 = {k: v.double() for k, v in w0.items()}
    if kind.startswith('mdrff'):
        freqs = model.rff.freqs.cpu().numpy()
        o = oest.OracleMDRFF(n_feat=64, sigma=4.0, kernel='RBF', freqs=freqs if perm is None else freqs[:, perm], **kw)
        if double:
            o.rff.freqs, o.rff.sigma = o.rff.freqs.double(), o.rff.sigma.double()
    else:
        o = oest.OracleMDNN(hidden_layers=(16, 16), **kw)
        if perm is not None:
            w0['net.fcon0.weight'] = w0['net.fcon0.weight'][:, perm].contiguous()
    o.load_state_dict(w0)
    return o


@pytest.mark.parametrize('kind', ['mdnn', 'mdrff'])
@pytest.mark.parametrize('case', ['sig3_wide', 'corrdiff'])
def test_fp32_chunk_matches_the_oracle_on_hand_standardised_rows(B, case, kind):
    B.MDNN.EPS_NOISE = 0.0
    x, theta = _summaries(B, case)
    m = _model(B, kind, x.shape[1], True)
    o = _oracle(B, kind, m, x.shape[1])
    xn = NC.standardize(x.cpu().numpy(), N_TRAIN)                     # long-double statistics, rounded to fp32
    assert xn.dtype == np.float32
    got = _train(m, x, theta)
    ref = o.run_training(torch.from_numpy(xn), theta.cpu(), N_UPDATES, BATCH, ids_table=IDS)
    for key in ('test_loss', 'train_loss'):                           # tests/test_gpu_fit.py: a reference chunk
        print(case, kind, key, np.max(np.abs(np.array(got[key]) / np.array(ref[key]) - 1)))
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-4, atol=1e-5)


N_ORDERS = 8


@pytest.mark.parametrize('kind', ['mdnn_f64', 'mdrff_f64'])
@pytest.mark.parametrize('case', ['sig3_wide', 'corrdiff'])
def test_fp64_chunk_matches_the_oracle_on_hand_standardised_rows(B, case, kind):
    """The rule of tests/test_gpu_f64.py for a chunk: the fp64 oracle in eight input-column orders; the device
    run within 8 x their spread + 1e-11 |ref|, where that spread itself is <= 1e-8 relative."""
    B.MDNN.EPS_NOISE = 0.0
    x, theta = _summaries(B, case, torch.float64)
    width = x.shape[1]
    m = _model(B, kind, width, True)
    xn = torch.from_numpy(NC.standardize(x.cpu().numpy(), N_TRAIN))
    assert xn.dtype == torch.float64
    runs = []
    with default_f64():
        for i in range(N_ORDERS):
            perm = None if i == 0 else np.random.RandomState(100 + i).permutation(width)
            o = _oracle(B, kind, m, width, perm=perm, double=True)
            logs = o.run_training(xn if perm is None else xn[:, perm].contiguous(), theta.cpu().double(), N_UPDATES,
                                  BATCH, ids_table=IDS)
            runs.append({k: np.asarray(v, np.float64) for k, v in logs.items()})
    hip = {k: np.asarray(v, np.float64) for k, v in _train(m, x, theta).items()}
    ref = runs[0]
    for key in ('train_loss', 'test_loss'):
        spread = np.max([np.abs(r[key] - ref[key]) for r in runs[1:]], axis=0)
        rel = (spread / np.abs(ref[key])).max()
        dev = np.abs(hip[key] - ref[key])
        print('%s %s %s: oracle spread %.3g, HIP deviation %.3g' % (case, kind, key, rel,
                                                                    (dev / np.abs(ref[key])).max()))
        assert rel <= 1e-8, 'condition broken: shorten the chunk (%s: %.3g)' % (key, rel)
        assert (dev <= 8 * spread + 1e-11 * np.abs(ref[key])).all(), (key, dev, spread)


# ------------------------------------------------------------------ 5. - 7. BayesSim
SIM = {
    'mdnn_sig': (dict(modelClass='MDNN', summarizerFxn='summary_signatory', sigDepth=3, hiddenLayers=(16, 16)), 3, 1),
    'mdrff_start': (dict(modelClass='MDRFF', summarizerFxn='summary_start', nFeat=64, hiddenLayers=[]), 5, 2),
}


def _sim(B, tag, seed=77, **extra):
    cfg, sd, ad = SIM[tag]
    cfg = dict(cfg, trainTrajLen=11, components=3, lr=1e-3, inputNorm=True, **extra)
    torch.manual_seed(seed)
    np.random.seed(seed)
    return B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2, params_lows=np.zeros(2),
                      params_highs=np.ones(2), prior=None, proposal=None, device=DEV)


def _sim_pairs(tag, n=3500):
    _, sd, ad = SIM[tag]
    theta, states, actions = _pairs(sd, ad, n=n, seed=3)
    return theta.to(DEV), states.to(DEV), actions.to(DEV)


def _stats_bits(model):
    return [_bits(getattr(model.input_norm, name)) for name in ('mean', 'inv_std', 'count')]


@pytest.mark.parametrize('tag', list(SIM))
def test_fit_and_the_chunk_loop_use_the_same_statistics(B, tag):
    theta, states, actions = _sim_pairs(tag)
    fit = _sim(B, tag)
    np.random.seed(11), torch.manual_seed(12)
    logs_fit = fit.fit(theta, states, actions)
    loop = _sim(B, tag)
    np.random.seed(11), torch.manual_seed(12)
    logs_loop = [loop.run_training(theta[i:i + 1000], states[i:i + 1000], actions[i:i + 1000])
                 for i in range(0, 3500, 1000)]
    assert len(logs_fit) == len(logs_loop) == 4
    assert int(fit.model.input_norm.count) == 800 == int(loop.model.input_norm.count)
    for u, v in zip(_stats_bits(fit.model), _stats_bits(loop.model)):
        assert np.array_equal(u, v)
    # ... the first chunk's 800 training rows, not the block and not the held-out rows
    hand = _sim(B, tag)
    hand.fit_input_norm(states[:800], actions[:800])
    for u, v in zip(_stats_bits(fit.model), _stats_bits(hand.model)):
        assert np.array_equal(u, v)
    for x, y in zip(logs_fit, logs_loop):       # tests/test_gpu_fit.py::test_fit_projects_blocks_of_chunks_at_once
        np.testing.assert_allclose(x['train_loss'], y['train_loss'], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(x['test_loss'], y['test_loss'], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(fit.model._flat, loop.model._flat, rtol=1e-5, atol=1e-6)
    before = _stats_bits(fit.model)
    fit.fit(theta[1000:2500], states[1000:2500], actions[1000:2500])
    for u, v in zip(before, _stats_bits(fit.model)):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('tag', list(SIM))
def test_predict_standardises_like_fit(B, tag):
    B.MDNN.EPS_NOISE = 0.0
    theta, states, actions = _sim_pairs(tag, n=1000)
    bs = _sim(B, tag)
    bs.run_training(theta, states, actions)
    mog = bs.predict(states[900:901], actions[900:901])
    # the plain model with the same weights on the hand-standardised summary
    summ = bs._summarize(states[900:901], actions[900:901])
    xn = NC.apply(summ.cpu().numpy(), bs.model.input_norm.mean.cpu().numpy(), bs.model.input_norm.inv_std.cpu().numpy())
    cfg = dict(SIM[tag][0], trainTrajLen=11, components=3, lr=1e-3)
    torch.manual_seed(77), np.random.seed(77)      # (an MDRFF draws its frequencies: the same ones)
    plain = B.BayesSim(model_cfg=cfg, obs_dim=SIM[tag][1], act_dim=SIM[tag][2], params_dim=2,
                       params_lows=np.zeros(2), params_highs=np.ones(2), prior=None, device=DEV)
    weights = {k: v for k, v in bs.model.state_dict().items() if not k.startswith('input_norm.')}
    plain.model.load_state_dict(weights)
    want = plain.model.predict_MoGs(torch.from_numpy(xn).to(DEV))[0]
    fresh = _sim(B, tag)
    assert not fresh.model.input_norm_ready
    fresh.model.load_state_dict(bs.model.state_dict())
    again = fresh.predict(states[900:901], actions[900:901])
    for got in (mog, again):
        assert np.array_equal(got.a, want.a)
        for u, v in zip(got.xs, want.xs):
            assert np.array_equal(u.m, v.m) and np.array_equal(u.S, v.S)


@pytest.mark.parametrize('row', [5, 1500])          # a row the statistics are made from; a later chunk's training row
@pytest.mark.parametrize('tag', list(SIM))
def test_a_nan_trajectory_is_the_assertion_error_it_always_was(B, tag, row):
    theta, states, actions = _sim_pairs(tag, n=2000)
    states = states.clone()
    states[row, 2, 0] = NAN
    with pytest.raises(AssertionError):
        _sim(B, tag).fit(theta, states, actions)
    bs = _sim(B, tag)
    with pytest.raises(AssertionError, match='non-finite'):
        bs.fit_input_norm(states, actions)
    assert not bs.model.input_norm_ready and int(bs.model.input_norm.count) == 0


def test_data_parallel_needs_the_statistics_first(B):
    """The refusal comes before anything is enqueued (here: before the model even looks at its rows)."""
    m = _model(B, 'mdnn', 6, True)
    m._dp = object()                   # (what enable_data_parallel leaves behind; no process group needed)
    try:
        with pytest.raises(ValueError, match='fit_input_norm'):
            m.run_training(None, None, 5, 10)
    finally:
        m._dp = None
