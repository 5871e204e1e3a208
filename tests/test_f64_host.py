"""CPU-side checks of the fp64 mode (include/bsig_f64.h, MDNN.double()): the library exports and the
binding declares every prototype of the new header, casting re-flattens the model's buffers, and a
double model still refuses to compute without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib

NO_GPU = not torch.cuda.is_available()


def _model(full=True, cls='MDNN'):
    kw = dict(input_dim=40, output_dim=3, output_lows=np.array([0.1, 0.2, 0.3]),
              output_highs=np.array([1.0, 2.0, 3.0]), n_gaussians=4, full_covariance=full,
              activation=torch.nn.Tanh, lr=1e-3)
    torch.manual_seed(0)
    if cls == 'MDRFF':
        return B.MDRFF(n_feat=16, sigma=4.0, freqs=np.random.RandomState(0).randn(8, 40), **kw)
    return B.MDNN(hidden_layers=(24, 24), **kw)


def test_library_exports_every_f64_symbol():
    """(header == binding, every name resolves, no overlap with another header: tests/test_headers_host.py)"""
    declared = _lib.exported_symbols('bsig_f64.h')
    assert len(declared) >= 19
    for name in ('bsig_gemm_f64', 'bsig_rff_project_f64', 'bsig_mdn_head_forward_f64',
                 'bsig_mdn_loss_grad_f64', 'bsig_mdn_head_nll_f64', 'bsig_adam_flat_f64',
                 'bsig_normalize_rows_f64', 'bsig_fit64_create', 'bsig_fit64_destroy',
                 'bsig_fit64_workspace_bytes', 'bsig_fit64_bind', 'bsig_fit64_begin', 'bsig_fit64_run',
                 'bsig_fit64_pack_logs'):
        assert name in declared, name
    assert ctypes.sizeof(_lib.F64Hyper) == 64


def test_f64_sources_are_outside_the_kernel_source_hash():
    """tools/csrc_hash.py (the stamp of the committed profiles) covers csrc/* only: the fp64 mode's
    sources live one level down and leave it alone."""
    src = os.path.join(ROOT, 'bayes_sim_ig_amd', 'csrc')
    assert os.path.isdir(os.path.join(src, 'f64'))
    assert not [f for f in os.listdir(src) if 'f64' in f and os.path.isfile(os.path.join(src, f))]


@pytest.mark.parametrize('cls', ['MDNN', 'MDRFF'])
def test_double_and_back(cls):
    m = _model(cls=cls)
    keys = list(m.state_dict())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m._exp_avg.fill_(0.25)
    assert m.double() is m
    assert m._f64 and m._flat.dtype == torch.float64
    for t in (m._flat_grad, m._exp_avg, m._exp_avg_sq, m.output_lows, m.output_highs):
        assert t.dtype == torch.float64
    assert torch.equal(m._exp_avg, torch.full_like(m._exp_avg, 0.25))      # the moments travel
    assert list(m.state_dict()) == keys
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float64 and torch.equal(v, before[k].double()), k
    for p in m.parameters():          # views of the flat buffer, gradients too
        assert p.data_ptr() >= m._flat.data_ptr() and p.grad.dtype == torch.float64
    with torch.no_grad():
        m.pi.bias.add_(1.0)
    assert float(m._flat.sum()) == pytest.approx(float(sum(v.sum() for v in before.values())) + 4.0)
    with torch.no_grad():
        m.pi.bias.sub_(1.0)
    m.float()
    assert not m._f64 and m._flat.dtype == torch.float32 and m.output_lows.dtype == torch.float32
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, before[k]), k
    m.to(torch.float64)
    assert m._f64
    with pytest.raises(NotImplementedError):
        m.half()


@pytest.mark.skipif(not NO_GPU, reason='needs a machine without a GPU')
def test_double_model_has_no_cpu_fallback():
    m = _model().double()
    x, y = torch.zeros(4, 40), torch.zeros(4, 3)
    for call in (lambda: m(x), lambda: m.loss_and_grad(x, y), lambda: m.run_training(x, y, 2, 2),
                 lambda: m.predict_MoGs(x), lambda: m.adam_step(1), lambda: m.normalize_samples(y)):
        with pytest.raises(RuntimeError, match='no CPU fallback|needs a ROCm GPU'):
            call()


def test_double_model_refuses_data_parallel():
    m = _model()
    m._dp = object()          # a data-parallel group is attached
    with pytest.raises(NotImplementedError, match='data-parallel'):
        m.double()
    assert not m._f64 and m._flat.dtype == torch.float32 and m.pi.weight.dtype == torch.float32   # left as it was
    m = _model().double()
    with pytest.raises(NotImplementedError, match='data-parallel'):
        m.enable_data_parallel(group=None)
    m._dp = object()
    with pytest.raises(NotImplementedError, match='data-parallel'):
        m.run_training(torch.zeros(4, 40), torch.zeros(4, 3), 2, 2)


def test_bayessim_dtype_key():
    cfg = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 10, 'components': 3,
           'hiddenLayers': (16, 16), 'lr': 1e-3, 'fullCovariance': True}
    kw = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
              params_highs=np.array([2.0] * 2), prior=None)
    assert not B.BayesSim(model_cfg=cfg, **kw).model._f64
    bs = B.BayesSim(model_cfg=dict(cfg, dtype='float64'), **kw)
    assert bs.model._f64 and not bs._lazy_summaries()
    with pytest.raises(ValueError):
        B.BayesSim(model_cfg=dict(cfg, dtype='float16'), **kw)
