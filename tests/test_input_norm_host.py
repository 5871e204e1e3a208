"""CPU-side checks of the input standardisation (include/bsig_input_norm.h): the binding lists the entry points,
the workspace size is host arithmetic, the argument checks come before any launch, ``model_cfg['inputNorm']`` is
validated, the statistics are part of ``state_dict`` (and of nothing else), and a model without statistics says
so before it asks for a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import input_norm_cases as NC
from bayes_sim_ig_amd import _lib
from oracle import estimators as oest

KW = dict(input_dim=5, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
          full_covariance=False, hidden_layers=(16, 16), activation=torch.nn.Tanh, lr=1e-3)
RFF_KW = dict(input_dim=5, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2), n_gaussians=3,
              full_covariance=False, activation=torch.nn.Tanh, lr=1e-3, n_feat=64, sigma=4.0,
              freqs=np.random.RandomState(0).randn(32, 5).astype(np.float32))
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 11, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
SIM_KW = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
              params_highs=np.array([2.0] * 2), prior=None)
NAMES = ['bsig_input_norm_apply', 'bsig_input_norm_apply_f64', 'bsig_input_norm_stats',
         'bsig_input_norm_stats_f64', 'bsig_input_norm_workspace_bytes']


@pytest.fixture(autouse=True)
def _quiet():
    old, B.MDNN.VERBOSE = B.MDNN.VERBOSE, False
    yield
    B.MDNN.VERBOSE = old


def _err():
    return _lib.load().bsig_last_error().decode()


def test_binding_lists_the_entry_points_and_the_seam_routes_them():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py)"""
    assert _lib.exported_symbols('bsig_input_norm.h') == NAMES
    for op in ('input_norm_stats', 'input_norm_apply'):
        assert _lib.F32.symbol(op) == 'bsig_' + op and _lib.F64.symbol(op) == 'bsig_' + op + '_f64'
    assert _lib.INPUT_NORM_SLAB_ROWS == NC.SLAB
    with open(_lib.HEADER_PATH.replace('bsig.h', 'bsig_input_norm.h')) as f:
        assert '#define BSIG_INPUT_NORM_SLAB_ROWS %d\n' % NC.SLAB in f.read()


def test_workspace_bytes():
    ws = _lib.load().bsig_input_norm_workspace_bytes
    slab = NC.SLAB
    for n, slabs in ((1, 1), (slab - 1, 1), (slab, 1), (slab + 1, 2), (3 * slab + 5, 4)):
        for width in (1, 7, 11110):
            assert ws(n, width) == 2 * slabs * width * 8, (n, width)      # (mean, M2) per slab and column
    for n, width in ((0, 5), (-1, 5), (5, 0), (5, -3), (0, 0)):
        assert ws(n, width) == -1
    assert ws(2 ** 62, 2 ** 40) == -1          # a size that no int64 holds


@pytest.mark.parametrize('suffix', ['', '_f64'])
def test_c_abi_argument_errors(suffix):
    """The checks come before any launch: no GPU needed, no pointer is dereferenced on the host."""
    lib = _lib.load()
    stats, apply = getattr(lib, 'bsig_input_norm_stats' + suffix), getattr(lib, 'bsig_input_norm_apply' + suffix)
    size = 8 if suffix else 4
    one, two = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)      # far apart: no overlap
    need = lib.bsig_input_norm_workspace_bytes(10, 4)
    # stats(x, ld, n, width, mean, inv_std, workspace, workspace_bytes, stream)
    for k, name in ((0, 'x'), (4, 'mean'), (5, 'inv_std'), (6, 'workspace')):
        args = [one, 4, 10, 4, one, one, one, need, None]
        args[k] = None
        assert stats(*args) == _lib.BSIG_EINVAL and 'null pointer ' + name in _err()
    assert stats(one, 3, 10, 4, one, one, one, need, None) == _lib.BSIG_EINVAL and 'ld' in _err()
    assert stats(one, 4, 10, 4, one, one, one, need - 1, None) == _lib.BSIG_EINVAL and 'workspace_bytes' in _err()
    assert stats(one, 4, 0, 4, one, one, one, need, None) == _lib.BSIG_EINVAL and 'n = 0' in _err()
    assert stats(one, 4, 10, 0, one, one, one, need, None) == _lib.BSIG_EINVAL and 'width' in _err()
    # apply(x, ld_x, mean, inv_std, out, ld_out, n, width, stream)
    for k, name in ((0, 'x'), (2, 'mean'), (3, 'inv_std'), (4, 'out')):
        args = [one, 4, one, one, two, 4, 10, 4, None]
        args[k] = None
        assert apply(*args) == _lib.BSIG_EINVAL and 'null pointer ' + name in _err()
    assert apply(one, 3, one, one, two, 4, 10, 4, None) == _lib.BSIG_EINVAL and 'ld_x' in _err()
    assert apply(one, 4, one, one, two, 3, 10, 4, None) == _lib.BSIG_EINVAL and 'ld_out' in _err()
    assert apply(one, 4, one, one, two, 4, -1, 4, None) == _lib.BSIG_EINVAL and 'n = -1' in _err()
    # partial overlap, decided from the pointer ranges: the rows of x end at x + ((n - 1) ld + width) elements
    x0 = 1 << 20
    span = (9 * 6 + 4) * size
    for off in (size, span - size, -size, -(span - size)):
        assert apply(ctypes.c_void_p(x0), 6, one, one, ctypes.c_void_p(x0 + off), 6, 10, 4, None) == \
            _lib.BSIG_EINVAL and 'overlaps' in _err(), off
    # the same start with another pitch is an overlap too
    assert apply(ctypes.c_void_p(x0), 6, one, one, ctypes.c_void_p(x0), 8, 10, 4, None) == _lib.BSIG_EINVAL
    assert 'overlaps' in _err()
    # n == 0: nothing to do, nothing looked at
    assert apply(None, 0, None, None, None, 0, 0, 0, None) == _lib.BSIG_OK


def test_model_cfg_input_norm_is_validated():
    assert B.BayesSim(model_cfg=CFG, **SIM_KW).model._inorm is None
    assert B.BayesSim(model_cfg=dict(CFG, inputNorm=False), **SIM_KW).model._inorm is None
    bs = B.BayesSim(model_cfg=dict(CFG, inputNorm=True), **SIM_KW)
    assert bs.model._inorm is not None and bs.model._inorm.width == bs.model.input_dim and not bs.model.input_norm_ready
    rff = B.BayesSim(model_cfg=dict(CFG, modelClass='MDRFF', nFeat=64, inputNorm=True), **SIM_KW)
    assert rff.model._inorm.width == rff.model.input_dim == bs.model.input_dim       # the summary's width
    for bad in (1, 0, 'yes', 'True', None, [True], 1.0):
        with pytest.raises(ValueError, match='inputNorm'):
            B.BayesSim(model_cfg=dict(CFG, inputNorm=bad), **SIM_KW)


def test_state_dict_keys_and_dtypes():
    torch.manual_seed(3)
    plain = B.MDNN(**KW)
    torch.manual_seed(3)
    oracle = oest.OracleMDNN(**KW)
    torch.manual_seed(3)
    model = B.MDNN(input_norm=True, **KW)
    keys = list(oracle.state_dict())
    assert list(plain.state_dict()) == keys and not plain.input_norm_ready
    assert list(B.MDNN(input_norm=False, **KW).state_dict()) == keys
    extra = ['input_norm.mean', 'input_norm.inv_std', 'input_norm.count']
    assert list(model.state_dict()) == keys + extra
    # nothing drawn from the RNG: the same initialisation
    for k in keys:
        assert torch.equal(model.state_dict()[k], plain.state_dict()[k]) and \
            torch.equal(plain.state_dict()[k], oracle.state_dict()[k]), k
    for conv in (lambda m: m, lambda m: m.double(), lambda m: m.float()):
        sd = conv(model).state_dict()
        assert [sd[k].dtype for k in extra] == [torch.float64, torch.float64, torch.int64]
        assert sd['input_norm.mean'].shape == sd['input_norm.inv_std'].shape == (5,) and sd['input_norm.count'].shape == ()
    assert int(model.state_dict()['input_norm.count']) == 0 and not model.input_norm_ready
    rff = B.MDRFF(input_norm=True, **RFF_KW)
    assert list(rff.state_dict()) == list(B.MDRFF(**RFF_KW).state_dict()) + extra
    assert rff.state_dict()['input_norm.mean'].shape == (5,)


def test_set_input_norm_stores_the_flat_rule_and_state_dict_round_trips():
    model = B.MDNN(input_norm=True, **KW)
    u = 2.0 ** -23
    mean = np.array([1.0, -2.0, 1000.0, 1000.0, 0.0])
    std = np.array([2.0, 0.0, 7.9 * u * 1000.0, 8.1 * u * 1000.0, 0.0])      # kept, zero, below, above, zero
    model.set_input_norm(mean, std, count=800)
    sd = model.state_dict()
    assert sd['input_norm.mean'].tolist() == mean.tolist()
    assert sd['input_norm.inv_std'].tolist() == [0.5, 0.0, 0.0, 1.0 / std[3], 0.0]
    assert int(sd['input_norm.count']) == 800 and model.input_norm_ready
    # a double model's rows have u = 2^-52: the two columns near the fp32 threshold are kept
    model.double().set_input_norm(torch.from_numpy(mean), torch.from_numpy(std))
    assert model.state_dict()['input_norm.inv_std'].tolist() == [0.5, 0.0, 1.0 / std[2], 1.0 / std[3], 0.0]
    model.float().set_input_norm(mean, std, count=800)
    fresh = B.MDNN(input_norm=True, **KW)
    assert not fresh.input_norm_ready
    fresh.load_state_dict(model.state_dict())
    assert fresh.input_norm_ready
    for k, v in model.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v) and fresh.state_dict()[k].dtype == v.dtype, k
    # the statistics are part of the model: a default model refuses them, and the other way round
    with pytest.raises(RuntimeError):
        B.MDNN(**KW).load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError):
        B.MDNN(input_norm=True, **KW).load_state_dict(B.MDNN(**KW).state_dict())
    for bad in ((mean[:4], std[:4]), (mean, -std - 1.0)):
        with pytest.raises(ValueError):
            model.set_input_norm(*bad)
    for call in (lambda m: m.set_input_norm(mean, std), lambda m: m.fit_input_norm(torch.zeros(3, 5)),
                 lambda m: m.normalize_inputs(torch.zeros(3, 5))):
        with pytest.raises(RuntimeError, match='input_norm=True'):
            call(B.MDNN(**KW))


@pytest.mark.parametrize('cls', ['MDNN', 'MDRFF'])
def test_a_model_without_statistics_says_so_before_it_asks_for_a_gpu(cls, monkeypatch):
    """forward, predict_MoGs, loss_and_grad and normalize_inputs check for the statistics FIRST: the
    RuntimeError comes on a machine without a GPU too."""
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    model = getattr(B, cls)(input_norm=True, **(KW if cls == 'MDNN' else RFF_KW))
    x, y = torch.zeros(4, 5), torch.zeros(4, 2)
    for call in (lambda: model.forward(x), lambda: model(x), lambda: model.predict_MoGs(x),
                 lambda: model.loss_and_grad(x, y), lambda: model.normalize_inputs(x)):
        with pytest.raises(RuntimeError, match='statistics'):
            call()
