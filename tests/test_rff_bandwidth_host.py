"""CPU-side checks of the median bandwidth (include/bsig_rff_bandwidth.h, MDRFF(sigma='median'),
'MDRFF_<kernel>_median'): the binding lists the entry points, the workspace size is host arithmetic, the argument
checks come before any launch, the model class and ``model_cfg['rffSigmaScale']`` are parsed and validated, the
bandwidth is part of ``state_dict`` of such a model (and of no other), a default model draws what it drew, and a
model without its bandwidth says so before it asks for a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import rff_bandwidth_cases as RC
from bayes_sim_ig_amd import _lib

RFF_KW = dict(input_dim=5, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
              full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, n_feat=64)
FREQS = np.random.RandomState(0).randn(32, 5).astype(np.float32)
CFG = {'modelClass': 'MDRFF_RBF_median', 'summarizerFxn': 'summary_start', 'trainTrajLen': 11, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3, 'nFeat': 64}
SIM_KW = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
              params_highs=np.array([2.0] * 2), prior=None)
NAMES = ['bsig_rff_bandwidth_median', 'bsig_rff_bandwidth_median_f64', 'bsig_rff_bandwidth_select',
         'bsig_rff_bandwidth_workspace_bytes', 'bsig_rff_coeff_dev', 'bsig_rff_coeff_dev_f64']
EXTRA = ['rff_bandwidth.sigma', 'rff_bandwidth.count']


@pytest.fixture(autouse=True)
def _quiet():
    old, B.MDNN.VERBOSE = B.MDNN.VERBOSE, False
    yield
    B.MDNN.VERBOSE = old


def _err():
    return _lib.load().bsig_last_error().decode()


def test_binding_lists_the_entry_points_and_the_seam_routes_them():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py, which
    is parametrized over _lib.HEADERS and so covers this header too)"""
    assert _lib.exported_symbols('bsig_rff_bandwidth.h') == NAMES
    for op in ('rff_bandwidth_median', 'rff_coeff_dev'):
        assert _lib.F32.symbol(op) == 'bsig_' + op and _lib.F64.symbol(op) == 'bsig_' + op + '_f64'
    assert _lib.RFF_BANDWIDTH_MAX_ROWS == RC.MAX_ROWS
    assert _lib.RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES == RC.SELECT_WORKSPACE_BYTES
    with open(_lib.HEADER_PATH.replace('bsig.h', 'bsig_rff_bandwidth.h')) as f:
        text = f.read()
    assert '#define BSIG_RFF_BANDWIDTH_MAX_ROWS %d\n' % RC.MAX_ROWS in text
    assert '#define BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES %d\n' % RC.SELECT_WORKSPACE_BYTES in text


def test_workspace_bytes():
    ws = _lib.load().bsig_rff_bandwidth_workspace_bytes
    for n in (2, 3, 64, 65, 800, 1023, 1024, 1025, 32000):
        m = min(n, RC.MAX_ROWS)
        for width in (1, 7, 11802):
            assert ws(n, width) == 8 * (m * (m - 1) // 2) + RC.SELECT_WORKSPACE_BYTES, (n, width)
    for n, width in ((1, 5), (0, 5), (-1, 5), (5, 0), (5, -3)):
        assert ws(n, width) == -1


@pytest.mark.parametrize('suffix', ['', '_f64'])
def test_c_abi_argument_errors(suffix):
    """The checks come before any launch: no GPU needed, no pointer is dereferenced on the host."""
    lib = _lib.load()
    median = getattr(lib, 'bsig_rff_bandwidth_median' + suffix)
    coeff = getattr(lib, 'bsig_rff_coeff_dev' + suffix)
    one = ctypes.c_void_p(1 << 20)
    need = lib.bsig_rff_bandwidth_workspace_bytes(10, 4)
    # median(x, ld, n, width, scale, sigma_out, workspace, workspace_bytes, stream)
    for k, name in ((0, 'x'), (5, 'sigma_out'), (6, 'workspace')):
        args = [one, 4, 10, 4, 1.0, one, one, need, None]
        args[k] = None
        assert median(*args) == _lib.BSIG_EINVAL and 'null pointer ' + name in _err()
    assert median(one, 3, 10, 4, 1.0, one, one, need, None) == _lib.BSIG_EINVAL and 'ld' in _err()
    assert median(one, 4, 10, 4, 1.0, one, one, need - 1, None) == _lib.BSIG_EINVAL and 'workspace_bytes' in _err()
    assert median(one, 4, 10, 4, 1.0, one, ctypes.c_void_p((1 << 20) + 4), need, None) == _lib.BSIG_EINVAL
    assert 'aligned' in _err()
    for n in (1, 0, -2):
        assert median(one, 4, n, 4, 1.0, one, one, need, None) == _lib.BSIG_EINVAL and 'n = %d' % n in _err()
    assert median(one, 4, 10, 0, 1.0, one, one, need, None) == _lib.BSIG_EINVAL and 'width' in _err()
    for scale in (0.0, -1.0, float('inf'), float('nan')):
        assert median(one, 4, 10, 4, scale, one, one, need, None) == _lib.BSIG_EINVAL and 'scale' in _err()
    # coeff(freqs, sigma_dev, coeff, m, d, ld, stream)
    for k, name in ((0, 'freqs'), (1, 'sigma_dev'), (2, 'coeff')):
        args = [one, one, one, 3, 5, 8, None]
        args[k] = None
        assert coeff(*args) == _lib.BSIG_EINVAL and 'null pointer ' + name in _err()
    assert coeff(one, one, one, 3, 5, 4, None) == _lib.BSIG_EINVAL and 'ld' in _err()
    assert coeff(one, one, one, 3, 0, 4, None) == _lib.BSIG_EINVAL and 'd = 0' in _err()
    assert coeff(one, one, one, -1, 5, 8, None) == _lib.BSIG_EINVAL and 'm = -1' in _err()
    assert coeff(None, None, None, 0, 5, 8, None) == _lib.BSIG_OK


def test_select_argument_errors():
    select = _lib.load().bsig_rff_bandwidth_select
    one, need = ctypes.c_void_p(1 << 20), RC.SELECT_WORKSPACE_BYTES
    # select(values, count, out, workspace, workspace_bytes, stream)
    for k, name in ((0, 'values'), (2, 'out'), (3, 'workspace')):
        args = [one, 10, one, one, need, None]
        args[k] = None
        assert select(*args) == _lib.BSIG_EINVAL and 'null pointer ' + name in _err()
    for count in (0, -1, 2 ** 31):
        assert select(one, count, one, one, need, None) == _lib.BSIG_EINVAL and 'count' in _err()
    assert select(one, 10, one, one, need - 1, None) == _lib.BSIG_EINVAL and 'workspace_bytes' in _err()


def test_model_class_and_scale_are_parsed_and_validated():
    bs = B.BayesSim(model_cfg=CFG, **SIM_KW)
    bw = bs.model._rffbw
    assert isinstance(bs.model, B.MDRFF) and bw is not None and bw.scale == 1.0 and not bs.model.rff_bandwidth_ready
    assert bs.model.rff.bandwidth is bw
    assert B.BayesSim(model_cfg=dict(CFG, rffSigmaScale=0.5), **SIM_KW).model._rffbw.scale == 0.5
    # the kernel of the name is kept: Matern32 consumes the chi-square stream too (width > 100: the numpy draw)
    wide = dict(SIM_KW, obs_dim=60, act_dim=45)
    np.random.seed(4)
    mat = B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF_Matern32_median'), **wide)
    after = np.random.get_state()[1].copy()
    np.random.seed(4)
    num = B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF_Matern32_2.5'), **wide)
    assert mat.model._rffbw is not None and num.model._rffbw is None
    assert torch.equal(mat.model.rff.freqs, num.model.rff.freqs) and np.array_equal(after, np.random.get_state()[1])
    np.random.seed(4)
    rbf = B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF_RBF_median'), **wide)
    assert not torch.equal(rbf.model.rff.freqs, mat.model.rff.freqs)
    # the numeric forms are what they were
    assert num.model.rff.sigma.tolist() == [[2.5] * num.model.input_dim]
    assert B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF'), **SIM_KW).model.rff.sigma[0, 0].item() == 4.0
    for bad in (0.0, -1.0, 1, 2, True, '1.0', None, [1.0], float('inf'), float('nan')):
        with pytest.raises(ValueError, match='rffSigmaScale'):
            B.BayesSim(model_cfg=dict(CFG, rffSigmaScale=bad), **SIM_KW)
    for other in ('MDNN', 'MDRFF', 'MDRFF_RBF_4.0'):
        with pytest.raises(ValueError, match='rffSigmaScale'):
            B.BayesSim(model_cfg=dict(CFG, modelClass=other, rffSigmaScale=1.0), **SIM_KW)
    with pytest.raises(ValueError):
        B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF_RBF_mean'), **SIM_KW)      # float('mean'), as before
    assert B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW)._rffbw.scale == 1.0
    assert B.MDRFF(sigma='median', sigma_scale=2, freqs=FREQS, **RFF_KW)._rffbw.scale == 2.0
    for kw in (dict(sigma='mean'), dict(sigma='median', sigma_scale=0.0), dict(sigma='median', sigma_scale='1'),
               dict(sigma=4.0, sigma_scale=2.0)):
        with pytest.raises(ValueError):
            B.MDRFF(freqs=FREQS, **dict(RFF_KW, **kw))


def test_a_default_model_is_untouched():
    """No rff_bandwidth.* key, the same frequency draw, the same numpy RNG state afterwards; sigma as it was."""
    wide = dict(RFF_KW, input_dim=130)
    states = []
    for sigma in (4.0, 'median'):
        np.random.seed(21)
        torch.manual_seed(3)
        m = B.MDRFF(sigma=sigma, **wide)
        states.append((m, np.random.get_state()[1].copy()))
    (num, rng_num), (med, rng_med) = states
    np.random.seed(21)
    assert np.array_equal(num.rff.freqs.numpy(), np.random.normal(0.0, 1.0, (32, 130)).astype(np.float32))
    assert np.array_equal(rng_num, np.random.get_state()[1]) and np.array_equal(rng_num, rng_med)
    assert torch.equal(num.rff.freqs, med.rff.freqs)
    keys = list(num.state_dict())
    assert not [k for k in keys if k.startswith('rff_bandwidth')] and num._rffbw is None and not num.rff_bandwidth_ready
    assert list(med.state_dict()) == keys + EXTRA
    for k in keys:
        assert torch.equal(num.state_dict()[k], med.state_dict()[k]), k
    assert num.rff.sigma.shape == (1, 130) and num.rff.sigma.dtype == torch.float32 and (num.rff.sigma == 4.0).all()
    per_dim = B.MDRFF(sigma=[1.0, 2.0, 3.0, 4.0, 5.0], freqs=FREQS, **RFF_KW)
    assert per_dim.rff.sigma.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]] and per_dim._rffbw is None
    for call in (lambda m: m.set_rff_bandwidth(2.0), lambda m: m.fit_rff_bandwidth(torch.zeros(3, 130))):
        with pytest.raises(RuntimeError, match="sigma='median'"):
            call(num)
    assert B.MDNN(hidden_layers=(8,), **{k: v for k, v in RFF_KW.items() if k != 'n_feat'})._rffbw is None


def test_state_dict_round_trip_restores_ready():
    model = B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW)
    sd = model.state_dict()
    assert [sd[k].dtype for k in EXTRA] == [torch.float64, torch.int64] and [sd[k].shape for k in EXTRA] == [(), ()]
    assert int(sd['rff_bandwidth.count']) == 0 and not model.rff_bandwidth_ready
    for conv in (lambda m: m.double(), lambda m: m.float()):
        assert [conv(model).state_dict()[k].dtype for k in EXTRA] == [torch.float64, torch.int64]
    model.set_rff_bandwidth(12.75)
    assert model.rff_bandwidth_ready and float(model.state_dict()['rff_bandwidth.sigma']) == 12.75
    assert int(model.state_dict()['rff_bandwidth.count']) == 1
    # the reference's attribute is filled from the buffer when read
    assert model.rff.sigma.shape == (1, 5) and (model.rff.sigma == 12.75).all()
    fresh = B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW)
    assert not fresh.rff_bandwidth_ready
    version = fresh._rffbw.version
    fresh.load_state_dict(model.state_dict())
    assert fresh.rff_bandwidth_ready and fresh._rffbw.version > version
    for k, v in model.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v) and fresh.state_dict()[k].dtype == v.dtype, k
    # a state without a bandwidth leaves the model without one
    blank = B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW)
    blank.load_state_dict(B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW).state_dict())
    assert not blank.rff_bandwidth_ready
    # the bandwidth is part of the model: a numeric-sigma model refuses it, and the other way round
    with pytest.raises(RuntimeError):
        B.MDRFF(sigma=4.0, freqs=FREQS, **RFF_KW).load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError):
        B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW).load_state_dict(B.MDRFF(sigma=4.0, freqs=FREQS, **RFF_KW).state_dict())
    for bad in (0.0, -3.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='set_rff_bandwidth'):
            model.set_rff_bandwidth(bad)


@pytest.mark.parametrize('input_norm', [False, True])
def test_a_model_without_its_bandwidth_says_so_before_it_asks_for_a_gpu(input_norm, monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    model = B.MDRFF(sigma='median', freqs=FREQS, **dict(RFF_KW, **({'input_norm': True} if input_norm else {})))
    if input_norm:
        model.set_input_norm(np.zeros(5), np.ones(5))
    x, y = torch.zeros(4, 5), torch.zeros(4, 2)
    for call in (lambda: model.forward(x), lambda: model(x), lambda: model.predict_MoGs(x),
                 lambda: model.loss_and_grad(x, y), lambda: model.rff.to_features(x), lambda: model.rff.coeff(),
                 lambda: model._rff_args(), lambda: model.double()._rff_args(), lambda: model.rff.sigma):
        with pytest.raises(RuntimeError, match='fit_rff_bandwidth'):
            call()


def test_a_data_parallel_model_needs_its_bandwidth_first():
    """The refusal comes before anything is enqueued (here: before the model even looks at its rows)."""
    model = B.MDRFF(sigma='median', freqs=FREQS, **RFF_KW)
    model._dp = object()               # (what enable_data_parallel leaves behind; no process group needed)
    try:
        with pytest.raises(ValueError, match='fit_rff_bandwidth'):
            model.run_training(None, None, 5, 10)
        bs = B.BayesSim(model_cfg=CFG, **SIM_KW)
        bs.model._dp = model._dp
        try:
            with pytest.raises(ValueError, match='fit_rff_bandwidth'):
                bs._fit_once(torch.zeros(4, 2), None, None)
        finally:
            bs.model._dp = None
    finally:
        model._dp = None
