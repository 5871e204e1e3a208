"""CPU-side checks of the matmul precision (include/bsig_matmul.h, MDNN.set_matmul_precision): the library
exports and the binding declares every prototype of the new header, the Python switches validate their
values, a fresh model is 'float32' and creates its plan with flags 0, and bsig_debug_gemm_path names the
split-bf16 kernel exactly where the mode was asked for and the kernel covers the call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_precision_seam import FakeLib, P

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib

SPLIT = _lib.GEMM_PATH_SPLIT_BF16
EPI_ADAM = 100


def _model(cls='MDNN', **kw):
    args = dict(input_dim=40, output_dim=3, output_lows=np.array([0.1, 0.2, 0.3]),
                output_highs=np.array([1.0, 2.0, 3.0]), n_gaussians=4, full_covariance=True,
                activation=torch.nn.Tanh, lr=1e-3)
    args.update(kw)
    torch.manual_seed(0)
    if cls == 'MDRFF':
        return B.MDRFF(n_feat=16, sigma=4.0, freqs=np.random.RandomState(0).randn(8, 40), **args)
    return B.MDNN(hidden_layers=(24, 24), **args)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, '_lib', lib)
    monkeypatch.setattr(_lib, 'F32', P(torch.float32))
    monkeypatch.setattr(_lib, 'F64', P(torch.float64))
    return lib


def test_library_exports_every_matmul_symbol():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py)"""
    header = open(os.path.join(ROOT, 'include', 'bsig_matmul.h')).read()
    assert set(_lib.exported_symbols('bsig_matmul.h')) == {'bsig_gemm_f32_ex', 'bsig_rff_project_ex',
                                                           'bsig_debug_gemm_path'}
    # the _ex prototypes: the plain ones plus one int
    matmul = _lib.HEADERS['bsig_matmul.h']
    for name in ('bsig_gemm_f32', 'bsig_rff_project'):
        assert matmul[name + '_ex'][1] == _lib.HEADERS['bsig.h'][name][1] + [ctypes.c_int]
        assert list(getattr(_lib.load(), name + '_ex').argtypes) == matmul[name + '_ex'][1]
    consts = dict(re.findall(r'#define (BSIG_[A-Z0-9_]+) (\d+)', header))
    assert consts == {'BSIG_MATMUL_FP32': '0', 'BSIG_MATMUL_SPLIT_BF16': '1', 'BSIG_PLAN_SPLIT_BF16': '2',
                      'BSIG_GEMM_PATH_SPLIT_BF16': '10'}
    assert (_lib.MATMUL_FP32, _lib.MATMUL_SPLIT_BF16, _lib.PLAN_SPLIT_BF16, SPLIT) == (0, 1, 2, 10)
    # include/bsig.h is untouched by the new ABI
    assert 'matmul' not in open(os.path.join(ROOT, 'include', 'bsig.h')).read().lower()


def test_setter_validates(monkeypatch):
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    m = _model()
    assert m.matmul_precision == 'float32'
    with pytest.raises(AttributeError):
        m.matmul_precision = 'split_bf16'             # read-only
    assert m.set_matmul_precision('split_bf16') is m and m.matmul_precision == 'split_bf16'
    for bad in ('bf16', 'high', 'float64', None, 1):
        with pytest.raises(ValueError):
            m.set_matmul_precision(bad)
    assert m.matmul_precision == 'split_bf16'
    with pytest.raises(ValueError):                    # .double() on a model set to split_bf16
        m.double()
    assert not m._f64 and m._flat.dtype == torch.float32 and m.pi.weight.dtype == torch.float32
    m.set_matmul_precision('float32').double()
    with pytest.raises(ValueError):                    # a double model takes no matmul precision
        m.set_matmul_precision('split_bf16')
    assert m.set_matmul_precision('float32').matmul_precision == 'float32'


def test_rff_follows_its_model(monkeypatch):
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    m = _model('MDRFF')
    assert m.rff.matmul_precision == 'float32'
    m.set_matmul_precision('split_bf16')
    assert m.rff.matmul_precision == 'split_bf16'
    m.set_matmul_precision('float32')
    assert m.rff.matmul_precision == 'float32'
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'split_bf16')
    assert _model('MDRFF').rff.matmul_precision == 'split_bf16'


def test_environment_default(monkeypatch):
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    assert _model().matmul_precision == 'float32'
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'split_bf16')
    m = _model()
    assert m.matmul_precision == 'split_bf16'
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'float32')
    assert _model().matmul_precision == 'float32' and m.matmul_precision == 'split_bf16'   # read at construction
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'tf32')
    with pytest.raises(ValueError):
        _model()


def test_environment_default_does_not_break_double_models(monkeypatch):
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'split_bf16')
    for cls in ('MDNN', 'MDRFF'):
        m = _model(cls)
        assert m.matmul_precision == 'split_bf16'
        m.double()                                     # only the process default: left behind
        assert m._f64 and m.matmul_precision == 'float32'
        assert m.rff is None or m.rff.matmul_precision == 'float32'
        m = _model(cls).set_matmul_precision('split_bf16')   # chosen explicitly: refused
        with pytest.raises(ValueError):
            m.double()
    cfg = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 10, 'components': 3,
           'hiddenLayers': (16, 16), 'lr': 1e-3, 'fullCovariance': True, 'dtype': 'float64'}
    bs = B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
                    params_highs=np.array([2.0] * 2), prior=None)
    assert bs.model._f64 and bs.model.matmul_precision == 'float32'


def test_bayessim_matmul_key(monkeypatch):
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    cfg = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 10, 'components': 3,
           'hiddenLayers': (16, 16), 'lr': 1e-3, 'fullCovariance': True}
    kw = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
              params_highs=np.array([2.0] * 2), prior=None)
    assert B.BayesSim(model_cfg=cfg, **kw).model.matmul_precision == 'float32'
    assert B.BayesSim(model_cfg=dict(cfg, matmulPrecision='split_bf16'), **kw).model.matmul_precision == 'split_bf16'
    assert B.BayesSim(model_cfg=dict(cfg, matmulPrecision='float32'), **kw).model.matmul_precision == 'float32'
    with pytest.raises(ValueError):
        B.BayesSim(model_cfg=dict(cfg, matmulPrecision='bfloat16'), **kw)
    with pytest.raises(ValueError):
        B.BayesSim(model_cfg=dict(cfg, matmulPrecision='split_bf16', dtype='float64'), **kw)
    assert B.BayesSim(model_cfg=dict(cfg, matmulPrecision='float32', dtype='float64'), **kw).model._f64


def test_plan_flags(fake, monkeypatch):
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    m = _model()
    cfg = m._cfg()
    m._ensure_plan(cfg, 10, 48, 12, 5)
    assert fake.calls[-1][0] == 'bsig_fit_create_ex' and fake.calls[-1][1][5] == 0      # a fresh model: flags 0
    first = m._plan
    m.set_matmul_precision('split_bf16')                                                # drops the plan
    assert m._plan is None and fake.calls[-1][0] == 'bsig_fit_destroy' and fake.calls[-1][1][0] is first
    m._ensure_plan(cfg, 10, 48, 12, 5)
    assert fake.calls[-1][0] == 'bsig_fit_create_ex' and fake.calls[-1][1][5] == _lib.PLAN_SPLIT_BF16
    m._no_persistent = True
    m._drop_plan()
    m._ensure_plan(cfg, 10, 48, 12, 5)
    assert fake.calls[-1][1][5] == _lib.PLAN_SPLIT_BF16 | _lib.PLAN_NO_PERSISTENT
    # the fp64 seam refuses the flag
    with pytest.raises(NotImplementedError):
        _lib.F64.fit_create('cfg', 'hyper', 10, 48, 12, 5, _lib.PLAN_SPLIT_BF16)


def _path(m, n, k, akm=0, bkm=0, gathered=0, epi=0, ws=0, matmul=0):
    out = (ctypes.c_int32 * 8)()
    rc = _lib.load().bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, ws, matmul, out)
    assert rc == 0, _lib.load().bsig_last_error()
    return dict(zip(('kernel', 'tile_m', 'tile_n', 'splits', 'k_chunk', 'workgroups', 'declined'), list(out)[:7]))


SHAPES = [(1, 1, 1), (33, 17, 50), (130, 70, 257), (64, 260, 1040), (100, 128, 128), (800, 1024, 2310),
          (32000, 1024, 2310), (8192, 260, 4096), (260, 4096, 8192)]


@pytest.mark.parametrize('shape', SHAPES)
def test_gemm_path(shape):
    m, n, k = shape
    big = 1 << 32
    for akm in (0, 1):
        for bkm in (0, 1):
            for ws in (0, big):
                for gathered in (0, 1):
                    off = _path(m, n, k, akm, bkm, gathered, ws=ws, matmul=0)
                    assert off['kernel'] != SPLIT and off['declined'] == 0          # matmul = 0 never names it
                    on = _path(m, n, k, akm, bkm, gathered, ws=ws, matmul=1)
                    if (m, n, k, akm, bkm) in ((8192, 260, 4096, 0, 0), (260, 4096, 8192, 1, 1)):
                        # the documented rule: the head products of a large minibatch stay on the fp32 kernels
                        assert on['declined'] == 2 and {**on, 'declined': 0} == off
                        continue
                    assert on['kernel'] == SPLIT and on['declined'] == 0            # all four layout pairs
                    assert on['tile_m'] == on['tile_n'] and on['tile_m'] in (64, 128)
                    tiles = -(-m // on['tile_m']) * -(-n // on['tile_n'])
                    assert on['workgroups'] == tiles * on['splits']
                    assert on['k_chunk'] % 32 == 0 and on['k_chunk'] * on['splits'] >= k
                    assert on['k_chunk'] * (on['splits'] - 1) < max(k, 1)           # no empty slice
                    if ws == 0:
                        assert on['splits'] == 1
    # every epilogue the kernel applies itself needs no workspace
    for epi in range(6):
        assert _path(m, n, k, 0, 1, epi=epi, ws=0, matmul=1)['kernel'] == SPLIT


def test_gemm_path_large_minibatch_rule():
    """Head-shaped products against thousands of rows were measured slower in the split mode: they keep the
    fp32 kernels, and the path query says why; the same head at a smaller minibatch takes the split kernel."""
    big = 1 << 32
    for nh in (260, 270):
        assert _path(8192, nh, 4096, ws=big, matmul=1)['declined'] == 2
        assert _path(nh, 4096, 8192, 1, 1, 1, EPI_ADAM, big, 1)['declined'] == 2
        assert _path(4096, nh, 1024, ws=big, matmul=1)['kernel'] != SPLIT
        fwd, grad = _path(2048, nh, 1024, 0, 0, 1, 1, big, 1), _path(nh, 1024, 2048, 1, 1, 1, EPI_ADAM, big, 1)
        assert fwd['kernel'] == SPLIT and grad['kernel'] == SPLIT and fwd['declined'] == grad['declined'] == 0
    assert _path(32000, 2048, 2310, ws=big, matmul=1)['kernel'] == SPLIT       # the projection is not head-shaped


def test_gemm_path_workspace_too_small_for_the_slabs():
    """A fused Adam step leaves the split kernel through slabs: without room for one, the call runs the fp32
    kernel it runs with matmul = 0; K slices beyond what the workspace holds are not taken."""
    m, n, k = 260, 4096, 2048
    slab = 4 * m * n
    for ws in (0, slab - 4):
        got = _path(m, n, k, 1, 1, 1, EPI_ADAM, ws, 1)
        assert got['kernel'] != SPLIT and got['declined'] == 1
        want = _path(m, n, k, 1, 1, 1, EPI_ADAM, ws, 0)
        assert {**got, 'declined': 0} == want
    assert _path(m, n, k, 1, 1, 1, EPI_ADAM, slab, 1)['kernel'] == SPLIT
    assert _path(m, n, k, 1, 1, 1, EPI_ADAM, slab, 1)['splits'] == 1
    two = _path(m, n, k, 1, 1, 1, EPI_ADAM, 2 * slab, 1)
    assert two['kernel'] == SPLIT and two['splits'] == 2 and two['k_chunk'] == 1024
    many = _path(m, n, k, 1, 1, 1, EPI_ADAM, 64 * slab, 1)
    assert many['kernel'] == SPLIT and many['splits'] >= 2
    # (64, 260, 1040): a workspace of one slab forces one slice, a larger one allows a ragged last slice
    one = _path(64, 260, 1040, ws=4 * 64 * 260, matmul=1)
    more = _path(64, 260, 1040, ws=64 * 4 * 64 * 260, matmul=1)
    assert one['splits'] == 1 and more['splits'] >= 2 and 1040 % more['k_chunk'] != 0


def test_gemm_path_bad_arguments():
    out = (ctypes.c_int32 * 8)()
    lib = _lib.load()
    assert lib.bsig_debug_gemm_path(4, 4, 4, 0, 0, 0, 0, 0, 2, out) == _lib.BSIG_EINVAL
    assert lib.bsig_debug_gemm_path(4, 4, 4, 0, 0, 0, 7, 0, 1, out) == _lib.BSIG_EINVAL
    assert lib.bsig_debug_gemm_path(0, 4, 4, 0, 0, 0, 0, 0, 1, out) == _lib.BSIG_EINVAL
    assert lib.bsig_debug_gemm_path(4, 4, 4, 0, 0, 0, 0, 0, 1, None) == _lib.BSIG_EINVAL
