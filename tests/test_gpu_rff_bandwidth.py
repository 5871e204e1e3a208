"""GPU checks of the median bandwidth (include/bsig_rff_bandwidth.h, MDRFF(sigma='median'),
'MDRFF_<kernel>_median'): the selection stage bit for bit against numpy's sort, the distances bit for bit where
they are exact and within a derived bound elsewhere, and the model / BayesSim layers against the numpy restatement
of tests/rff_bandwidth_cases.py and against the oracle.

The bound of the general rows (derived, not measured): every term of a squared distance is non-negative, so the
chain of ``width`` fma -- one rounding each, on top of the one rounding of each difference -- is within
(width + 2) 2^-53 relative of the exact sum; an order statistic moves by no more than its elements; the square root
and the multiplication by ``scale`` add one rounding each to sigma, two to its square:
    |sigma^2 - ref^2| <= (width + 4) 2^-53 ref^2,
with ref^2 summed in long double (RC.sigma2_ref)."""
import functools
import os

import numpy as np
import pytest
import torch

import rff_bandwidth_cases as RC

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
def _guards():
    import bayes_sim_ig_amd as pkg
    old = pkg.MDNN.EPS_NOISE
    consts = {k: getattr(pkg.BayesSim, k) for k in ('NUM_TRAIN_TRAJ_PER_BATCH', 'NUM_GRAD_UPDATES', 'MINIBATCH_SIZE')}
    yield
    pkg.MDNN.EPS_NOISE = old
    for k, v in consts.items():
        setattr(pkg.BayesSim, k, v)
    os.environ.pop('BSIG_NO_FIT_PREPROJECT', None)


def _bits(v):
    return np.asarray(v, dtype=np.float64).reshape(-1).view(np.uint64)


# ------------------------------------------------------------------ 1. selection
def _select(B, values):
    """The device's lower median of ``values`` (numpy float64), as a numpy float64 scalar."""
    L = B._lib
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(DEV)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(RC.SELECT_WORKSPACE_BYTES // 8, dtype=torch.float64, device=DEV)
    L.check(L.load().bsig_rff_bandwidth_select(L.ptr(v), v.numel(), L.ptr(out), L.ptr(ws), ws.numel() * 8,
                                               L.stream()))
    return out.cpu().numpy()[0]


@pytest.mark.parametrize('pattern', RC.SELECT_PATTERNS)
def test_select_is_the_lower_median_bit_for_bit(B, pattern):
    for count in RC.SELECT_COUNTS:
        v = RC.select_values(pattern, count)
        want = np.sort(v)[(count - 1) // 2]
        got, again = _select(B, v), _select(B, v)
        assert _bits(got)[0] == _bits(want)[0], (pattern, count, got, want)
        assert _bits(again)[0] == _bits(got)[0], (pattern, count)


@pytest.mark.parametrize('bad', [float('inf'), NAN, -NAN])
def test_select_gives_nan_for_one_non_finite_value_anywhere(B, bad):
    for count in (1, 2, 65, 1025, 4097):
        for at in sorted({0, count // 2, count - 1}):
            v = RC.select_values('uniform', count)
            v[at] = bad
            assert np.isnan(_select(B, v)), (count, at)
    # the largest finite double is a value like any other
    v = RC.select_values('uniform', 65)
    v[:40] = np.finfo(np.float64).max
    assert _select(B, v) == np.finfo(np.float64).max


# ------------------------------------------------------------------ 2. distances
def _device_rows(x, kind):
    """x[n, width] on the device with NaN in every padding column.  'vec': a 16-byte aligned base and pitch (the
    16-byte loads); 'elem': pitch width + 3 and a base one element past a 256-byte boundary (element by element)."""
    n, width = x.shape
    dtype = torch.float64 if x.dtype == np.float64 else torch.float32
    per16 = 16 // x.dtype.itemsize
    ld = (width + 3 + per16 - 1) // per16 * per16 if kind == 'vec' else width + 3
    off = 0 if kind == 'vec' else 1
    flat = torch.full((off + n * ld,), NAN, dtype=dtype, device=DEV)
    buf = flat[off:].view(n, ld)
    buf[:, :width] = torch.from_numpy(np.array(x)).to(DEV)
    assert (buf.data_ptr() % 16 == 0) == (kind == 'vec')
    return buf, ld


def _sigma(B, x, scale=1.0, kind='elem', n=None):
    L = B._lib
    buf, ld = _device_rows(x, kind)
    n, width = x.shape[0] if n is None else n, x.shape[1]
    prec = L.F64 if x.dtype == np.float64 else L.F32
    need = int(L.load().bsig_rff_bandwidth_workspace_bytes(n, width))
    ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    prec.rff_bandwidth_median(L.ptr(buf), ld, n, width, scale, L.ptr(out), L.ptr(ws), need, L.stream())
    return out.cpu().numpy()[0]


@pytest.mark.parametrize('dtype,n_max', [('float64', 33), ('float32', 15)])
def test_rows_on_a_line_give_the_numpy_bits(B, dtype, n_max):
    """All d2 are distinct and each is one rounded square: sigma must be numpy's, bit for bit; a dropped or doubled
    pair would move the median to another element."""
    for n in sorted({2, 3, 4, 5, 8, n_max - 1, n_max}):
        for width, column in ((1, 0), (5, 3), (130, 77)):
            x = RC.line_rows(n, width, dtype, column)
            for scale in (1.0, 0.5):
                want = RC.sigma_ref(x, scale, work=np.float64)
                for kind in ('vec', 'elem'):
                    got = _sigma(B, x, scale, kind)
                    assert _bits(got)[0] == _bits(want)[0], (dtype, n, width, scale, kind, got, want)


@functools.lru_cache(maxsize=None)
def _general(n, width, dtype):
    rng = np.random.RandomState(1000 * n + width)
    x = (rng.randn(n, width) * np.exp(rng.randn(1, width))).astype(dtype)
    x.setflags(write=False)
    return x, RC.sigma2_ref(x, 1.0)


@pytest.mark.parametrize('width', [1, 3, 4, 7, 40, 130, 1026])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_general_rows_within_the_derived_bound(B, dtype, width):
    for n in (2, 3, 5, 33, 64, 65, 130):
        x, ref2 = _general(n, width, dtype)
        bound = (width + 4) * RC.U53 * ref2
        first = None
        for kind in ('vec', 'elem'):
            got = _sigma(B, x, 1.0, kind)
            err = abs(np.longdouble(got) ** 2 - ref2)
            print('%s n %d width %d %s: error / bound %.3g' % (dtype, n, width, kind, float(err / bound)))
            assert np.isfinite(got) and err <= bound, (dtype, n, width, kind, got)
            # the pitch decides how the rows are loaded, not the result: one chain per pair
            first = got if first is None else first
            assert _bits(got)[0] == _bits(first)[0] and _bits(_sigma(B, x, 1.0, kind))[0] == _bits(got)[0]
        half = _sigma(B, x, 0.5, 'elem')
        assert half == 0.5 * first                      # one multiplication, exact for a power of two


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_cap_and_degenerate_rows(B, dtype):
    rng = np.random.RandomState(5)
    x = rng.randn(1500, 6).astype(dtype)
    capped = _sigma(B, x, 1.0, 'elem')
    assert _bits(capped)[0] == _bits(_sigma(B, x[:RC.MAX_ROWS].copy(), 1.0, 'elem'))[0]
    assert _bits(capped)[0] == _bits(_sigma(B, x, 1.0, 'vec'))[0] and np.isfinite(capped) and capped > 0
    assert _bits(capped)[0] != _bits(_sigma(B, x[:1000].copy(), 1.0, 'elem'))[0]
    # a NaN behind the cap is never read; one in a used row gives NaN
    bad = x.copy()
    bad[RC.MAX_ROWS:, 2] = NAN
    assert _bits(_sigma(B, bad, 1.0, 'elem'))[0] == _bits(capped)[0]
    for row in (0, 517, RC.MAX_ROWS - 1):
        bad = x.copy()
        bad[row, 4] = NAN
        assert np.isnan(_sigma(B, bad, 1.0, 'elem')), row
    bad = x[:70].copy()
    bad[69, 0] = np.inf
    assert np.isnan(_sigma(B, bad, 1.0, 'vec'))
    # rows that coincide carry no scale: exactly 1.0, whatever the scale
    for n in (2, 65, 200):
        same = np.repeat(rng.randn(1, 9), n, axis=0).astype(dtype)
        assert _sigma(B, same, 1.0, 'elem') == 1.0 and _sigma(B, same, 0.25, 'vec') == 1.0
    # ... also where only most of them do (the median pair coincides)
    most = np.repeat(rng.randn(1, 9), 40, axis=0).astype(dtype)
    most[:5] += 1.0
    assert _sigma(B, most, 3.0, 'elem') == 1.0


# ------------------------------------------------------------------ 3. the model
WIDTH, N_FEAT, N_PAIRS, N_TRAIN, N_UPDATES, BATCH = 130, 16, 60, 48, 12, 16
IDS = np.random.RandomState(2).randint(0, N_TRAIN, (N_UPDATES, BATCH))
FREQS = np.random.RandomState(9).randn(N_FEAT // 2, WIDTH).astype(np.float32)


def _rows(seed=0, double=False):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N_PAIRS, WIDTH, generator=gen) * (1.0 + 5.0 * torch.rand(1, WIDTH, generator=gen)) + 2.0
    theta = torch.rand(N_PAIRS, 2, generator=gen)
    return (x.double() if double else x).to(DEV), theta.to(DEV)


def _model(B, sigma='median', input_norm=False, double=False, scale=1.0, seed=7):
    kw = dict(input_dim=WIDTH, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
              full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, device=DEV, n_feat=N_FEAT, sigma=sigma,
              freqs=FREQS)
    if input_norm:
        kw['input_norm'] = True
    if sigma == 'median':
        kw['sigma_scale'] = scale
    torch.manual_seed(seed)
    m = B.MDRFF(**kw)
    return m.double() if double else m


def _features_f64(x, sigma, n_feat=N_FEAT, freqs=FREQS):
    inner = np.asarray(x, np.float64) @ (freqs.astype(np.float64) / float(sigma)).T
    return np.sqrt(2.0 / n_feat) * np.concatenate([np.cos(inner), np.sin(inner)], axis=1)


@pytest.mark.parametrize('variant', ['fp32', 'input_norm', 'double', 'double_input_norm'])
def test_run_training_makes_the_bandwidth_once_from_its_training_rows(B, variant):
    B.MDNN.EPS_NOISE = 0.0
    double, inorm = variant.startswith('double'), variant.endswith('input_norm')
    x, theta = _rows(0, double)
    m = _model(B, input_norm=inorm, double=double, scale=0.5)
    assert not m.rff_bandwidth_ready
    with pytest.raises(RuntimeError, match='fit_rff_bandwidth'):
        m.rff.to_features(x)
    logs = m.run_training(x, theta, N_UPDATES, BATCH, ids_table=IDS)
    assert np.isfinite(logs['train_loss'] + logs['test_loss']).all()
    sd = m.state_dict()
    assert m.rff_bandwidth_ready and int(sd['rff_bandwidth.count']) == N_TRAIN
    sigma = sd['rff_bandwidth.sigma'].cpu().numpy().reshape(())
    # the rows the estimator saw: the model's own standardisation of them (bit for bit what the staging copy
    # writes, tests/test_gpu_input_norm.py), else the rows themselves
    seen = (m.normalize_inputs(x) if inorm else x)
    assert RC.within_bound(sigma, seen[:N_TRAIN].cpu().numpy(), 0.5, WIDTH), (variant, sigma)
    assert not RC.within_bound(sigma, seen.cpu().numpy(), 0.5, WIDTH)      # not the held-out rows too
    assert (m.rff.sigma.cpu().numpy() == np.float32(sigma)).all() and m.rff.sigma.shape == (1, WIDTH)
    # the explicit form on the same rows gives the same bits
    c = _model(B, input_norm=inorm, double=double, scale=0.5)
    if inorm:
        c.input_norm.load_state_dict(m.input_norm.state_dict())
        c.input_norm.ready = True
    c.fit_rff_bandwidth(x[:N_TRAIN])
    assert _bits(c.state_dict()['rff_bandwidth.sigma'].cpu().numpy())[0] == _bits(sigma)[0]
    # the features are those of the definition at that sigma
    feats = m.rff.to_features(seen.float()).cpu().numpy()
    np.testing.assert_allclose(feats, _features_f64(seen.float().cpu().numpy(), sigma), rtol=0, atol=3e-6)
    # a second call on other rows leaves it as it is
    x2, theta2 = _rows(1, double)
    m.run_training(x2 * 3.0, theta2, N_UPDATES, BATCH, ids_table=IDS)
    assert _bits(m.state_dict()['rff_bandwidth.sigma'].cpu().numpy())[0] == _bits(sigma)[0]
    assert int(m.state_dict()['rff_bandwidth.count']) == N_TRAIN
    # forward and predict_MoGs use it; a state_dict carries it over
    fresh = _model(B, input_norm=inorm, double=double)
    fresh.load_state_dict(m.state_dict())
    for u, v in zip(m.forward(x[N_TRAIN:N_TRAIN + 3]), fresh.forward(x[N_TRAIN:N_TRAIN + 3])):
        assert (u is None and v is None) or torch.equal(u, v)
    assert len(m.predict_MoGs(x[:2])) == 2
    # set_rff_bandwidth replaces it, and what was derived from it
    before = m.rff.to_features(seen.float())
    m.set_rff_bandwidth(2.0 * float(sigma))
    after = m.rff.to_features(seen.float()).cpu().numpy()
    assert not np.array_equal(after, before.cpu().numpy())
    np.testing.assert_allclose(after, _features_f64(seen.float().cpu().numpy(), 2.0 * float(sigma)), rtol=0, atol=3e-6)


@pytest.mark.parametrize('input_norm', [False, True])
def test_chunk_matches_the_oracle_at_the_device_made_sigma(B, input_norm):
    """OracleMDRFF with the model's frequencies and the device-made sigma, read back: the 6 + 6 logs at the 1e-4
    of the reference chunks of tests/test_gpu_fit.py."""
    from oracle import estimators as oest
    B.MDNN.EPS_NOISE = 0.0
    n_updates = 20
    ids = np.random.RandomState(3).randint(0, N_TRAIN, (n_updates, BATCH))
    x, theta = _rows(0)
    m = _model(B, input_norm=input_norm)
    w0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()
          if not k.startswith(('input_norm.', 'rff_bandwidth.'))}
    got = m.run_training(x, theta, n_updates, BATCH, ids_table=ids)
    assert len(got['train_loss']) == len(got['test_loss']) == 6
    sigma = float(m.state_dict()['rff_bandwidth.sigma'])
    o = oest.OracleMDRFF(input_dim=WIDTH, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2),
                         n_gaussians=3, full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, eps_noise=0.0,
                         n_feat=N_FEAT, sigma=sigma, kernel='RBF', freqs=FREQS)
    o.load_state_dict(w0)
    seen = (m.normalize_inputs(x) if input_norm else x).cpu()
    ref = o.run_training(seen, theta.cpu(), n_updates, BATCH, ids_table=ids)
    for key in ('test_loss', 'train_loss'):
        print(input_norm, key, np.max(np.abs(np.array(got[key]) / np.array(ref[key]) - 1)))
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ 4. BayesSim
def _sim(B, extra=None):
    cfg = {'modelClass': 'MDRFF_RBF_median', 'summarizerFxn': 'summary_start', 'trainTrajLen': 11, 'components': 3,
           'hiddenLayers': (16, 16), 'lr': 1e-3, 'nFeat': 64}
    cfg.update(extra or {})
    torch.manual_seed(77)
    np.random.seed(78)
    return B.BayesSim(model_cfg=cfg, obs_dim=5, act_dim=2, params_dim=2, params_lows=np.array([0.0] * 2),
                      params_highs=np.array([1.0] * 2), prior=None, device=DEV)


def _sim_pairs(n=100, seed=0):
    gen = torch.Generator().manual_seed(seed)
    theta = torch.rand(n, 2, generator=gen)
    states = torch.randn(n, 11, 5, generator=gen) * 0.3 + theta[:, None, :1]
    actions = torch.rand(n, 11, 2, generator=gen)
    return theta.to(DEV), states.to(DEV), actions.to(DEV)


@pytest.mark.parametrize('extra', [{}, {'inputNorm': True, 'rffSigmaScale': 2.0}, {'dtype': 'float64'}])
def test_fit_block_path_and_chunk_path_make_the_same_bits(B, extra):
    """Two chunks of 50 pairs (40 training rows): the block path against BSIG_NO_FIT_PREPROJECT=1.  sigma bit for
    bit; the logs as tests/test_gpu_fit.py holds these two paths to each other."""
    B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH, B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 50, 7, 16
    theta, states, actions = _sim_pairs()
    out = []
    for env in ('0', '1'):
        os.environ['BSIG_NO_FIT_PREPROJECT'] = env
        try:
            bs = _sim(B, extra)
            np.random.seed(11)
            torch.manual_seed(12)
            logs = bs.fit(theta, states, actions)
            out.append((bs, logs))
        finally:
            os.environ.pop('BSIG_NO_FIT_PREPROJECT', None)
    (a, la), (b, lb) = out
    assert len(la) == len(lb) == 2 and a.model.rff_bandwidth_ready and b.model.rff_bandwidth_ready
    sa, sb = (m.model.state_dict()['rff_bandwidth.sigma'].cpu().numpy() for m in (a, b))
    assert _bits(sa)[0] == _bits(sb)[0] and np.isfinite(sa) and sa > 0
    assert int(a.model.state_dict()['rff_bandwidth.count']) == int(b.model.state_dict()['rff_bandwidth.count']) == 40
    # ... and it is the definition's, of the first chunk's training rows as the projection sees them
    summ = a._summarize(states[:50], actions[:50])
    if a.model._f64:
        summ = summ.double()
    seen = a.model.normalize_inputs(summ) if a.model._inorm is not None else summ
    scale = extra.get('rffSigmaScale', 1.0)
    assert RC.within_bound(sa.reshape(()), seen[:40].cpu().numpy(), scale, seen.shape[1])
    for x, y in zip(la, lb):
        np.testing.assert_allclose(x['train_loss'], y['train_loss'], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(x['test_loss'], y['test_loss'], rtol=1e-6, atol=1e-6)
    # a fresh model that loads the state projects the same bits
    fresh = _sim(B, extra)
    assert not fresh.model.rff_bandwidth_ready
    fresh.model.load_state_dict(a.model.state_dict())
    assert torch.equal(fresh.model.rff.to_features(seen.float()), a.model.rff.to_features(seen.float()))
    # the explicit form: all given rows up to the cap, and frozen against a later fit
    c = _sim(B, extra)
    if c.model._inorm is not None:
        c.fit_input_norm(states[:40], actions[:40])
    c.fit_rff_bandwidth(states[:40], actions[:40])
    assert _bits(c.model.state_dict()['rff_bandwidth.sigma'].cpu().numpy())[0] == _bits(sa)[0]


def test_fit_reports_non_finite_rows(B):
    B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH, B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 50, 7, 16
    theta, states, actions = _sim_pairs()
    bad = states.clone()
    bad[3, 0, 1] = NAN
    bs = _sim(B)
    with pytest.raises(AssertionError):
        bs.fit_rff_bandwidth(bad, actions)
    assert not bs.model.rff_bandwidth_ready and int(bs.model.rff_bandwidth.count) == 0
    with pytest.raises(AssertionError):
        _sim(B).fit(theta, bad, actions)


# ------------------------------------------------------------------ 5. off
def test_a_numeric_sigma_model_is_what_the_untouched_entry_points_give(B):
    """sigma = 4.0: the coefficient the model binds and its features are bit for bit those of bsig_rff_coeff +
    bsig_rff_project called here, and a chunk's logs are bit for bit those of the same model driven with these
    features handed over; no bandwidth exists, none of its launches is made."""
    B.MDNN.EPS_NOISE = 0.0
    L = B._lib
    lib = L.load()
    x, theta = _rows(0)
    m = _model(B, sigma=4.0)
    assert m._rffbw is None and m.rff.bandwidth is None and 'rff_bandwidth.sigma' not in m.state_dict()
    fr = torch.from_numpy(FREQS).to(DEV)
    sg = torch.full((1, WIDTH), 4.0, dtype=torch.float32, device=DEV)
    ld = L.round_up(WIDTH, 4)
    co = torch.full((N_FEAT // 2, ld), NAN, dtype=torch.float32, device=DEV)
    L.check(lib.bsig_rff_coeff(L.ptr(fr), L.ptr(sg), L.ptr(co), N_FEAT // 2, WIDTH, ld, L.stream()))
    feats = torch.empty((N_PAIRS, N_FEAT), dtype=torch.float32, device=DEV)
    need = int(lib.bsig_gemm_workspace_bytes(N_PAIRS, N_FEAT // 2, WIDTH))
    ws = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
    L.check(lib.bsig_rff_project(L.ptr(x), x.stride(0), None, L.ptr(co), ld, None, L.ptr(feats), N_FEAT, N_PAIRS,
                                 WIDTH, N_FEAT // 2, float(m.rff.a), 0, L.ptr(ws), ws.numel() * 4, L.stream()))
    assert torch.equal(m._rff_args()[0], co) and torch.equal(m.rff.coeff(), co)
    assert torch.equal(m.rff.to_features(x), feats)
    logs = m.run_training(x, theta, N_UPDATES, BATCH, ids_table=IDS)
    handed = _model(B, sigma=4.0)
    ref = handed.run_training(x, theta, N_UPDATES, BATCH, ids_table=IDS, _feats=feats)
    assert logs == ref and torch.equal(m._flat, handed._flat)
    assert 'rffbw_ws' not in m._bufs and not m.rff_bandwidth_ready
    assert (m.rff.sigma == 4.0).all()
