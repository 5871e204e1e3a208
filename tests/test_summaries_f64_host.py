"""CPU-side checks of the summarizers' fp64 mode (the ``dtype`` keyword of bayes_sim_ig_amd/summarizers.py,
BayesSim's ``'summaryDtype'``): what is refused is refused before anything touches a GPU, the binding lists the
new entry points, the precision seam routes them, and a float64 call still has no CPU fallback."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib, summarizers

NO_GPU = not torch.cuda.is_available()
SUMMARIZERS = ('summary_start', 'summary_waypts', 'cross_correlation', 'summary_corr', 'summary_corrdiff',
               'summary_signatory')
NEW_SYMBOLS = ('bsig_summary_start_f64', 'bsig_crosscorr_f64', 'bsig_signature_f64')
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 10, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2),
          prior=None)


def _traj():
    return torch.zeros(2, 12, 3), torch.zeros(2, 12, 1)


@pytest.mark.parametrize('name', SUMMARIZERS)
def test_every_summarizer_takes_dtype_and_refuses_other_dtypes(name):
    fn = getattr(summarizers, name)
    assert inspect.signature(fn).parameters['dtype'].default is None
    for bad in (torch.float16, torch.bfloat16, torch.int32, 'float64'):
        with pytest.raises(ValueError, match='float32 or torch.float64'):
            fn(*_traj(), dtype=bad)


@pytest.mark.parametrize('name', ['cross_correlation', 'summary_corr', 'summary_corrdiff'])
def test_lazy_rows_do_not_exist_in_double(name):
    with pytest.raises(NotImplementedError, match='factor rows.*fp64 fit'):
        getattr(summarizers, name)(*_traj(), lazy=True, dtype=torch.float64)


def test_bayessim_summary_dtype_key():
    assert B.BayesSim(model_cfg=CFG, **KW)._summary_dtype is None
    assert B.BayesSim(model_cfg=dict(CFG, dtype='float64'), **KW)._summary_dtype is None
    assert B.BayesSim(model_cfg=dict(CFG, dtype='float64', summaryDtype='float32'), **KW)._summary_dtype is None
    bs = B.BayesSim(model_cfg=dict(CFG, dtype='float64', summaryDtype='float64'), **KW)
    assert bs._summary_dtype == torch.float64 and bs.model._f64 and not bs._lazy_summaries()
    with pytest.raises(ValueError, match='summaryDtype'):       # double summaries for an fp32 estimator
        B.BayesSim(model_cfg=dict(CFG, summaryDtype='float64'), **KW)
    with pytest.raises(ValueError, match='summaryDtype'):
        B.BayesSim(model_cfg=dict(CFG, dtype='float32', summaryDtype='float64'), **KW)
    for bad in ('float16', 'double', torch.float64):
        with pytest.raises(ValueError, match='summaryDtype'):
            B.BayesSim(model_cfg=dict(CFG, dtype='float64', summaryDtype=bad), **KW)


def test_block_rows_count_eight_bytes_per_double_summary_value(monkeypatch):
    """input_dim = 40: 160 000 bytes of fp32 summaries per chunk of 1000 pairs, 320 000 of double ones."""
    monkeypatch.setattr(B.BayesSim, 'FIT_BLOCK_BYTES', 3200000)
    f32 = B.BayesSim(model_cfg=dict(CFG, dtype='float64'), **KW)
    f64 = B.BayesSim(model_cfg=dict(CFG, dtype='float64', summaryDtype='float64'), **KW)
    assert f32.model.input_dim == 40
    assert f32._block_rows() == 20 * 1000 and f64._block_rows() == 10 * 1000


def test_binding_lists_the_new_entry_points_and_the_seam_routes_them():
    names = _lib.exported_symbols('bsig_f64.h')
    for name in NEW_SYMBOLS:
        assert name in names, name
        # the argument list of the fp32 namesake, pointer for pointer
        assert _lib.HEADERS['bsig_f64.h'][name] == _lib.HEADERS['bsig.h'][name[:-4]]
    for op, name in zip(('summary_start', 'crosscorr', 'signature'), NEW_SYMBOLS):
        assert _lib.F64.symbol(op) == name and _lib.F32.symbol(op) == name[:-4]
    assert summarizers._precision(None) is _lib.F32 and summarizers._precision(torch.float32) is _lib.F32
    assert summarizers._precision(torch.float64) is _lib.F64


def test_c_abi_argument_errors_of_the_double_entry_points():
    """The BSIG_REQUIRE checks come before any launch: no GPU needed."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)          # never dereferenced on the host
    err = lambda: lib.bsig_last_error().decode()
    assert lib.bsig_summary_start_f64(None, one, one, 1, 3, 3, 1, 1, 4, 8, None) == _lib.BSIG_EINVAL
    assert 'null pointer' in err()
    assert lib.bsig_summary_start_f64(one, one, one, 1, 3, 3, 1, 1, 4, 7, None) == _lib.BSIG_EINVAL
    assert 'ld_out' in err()
    assert lib.bsig_crosscorr_f64(one, one, one, 1, 1, 1, 3, 1, 0, 100, None, None) == _lib.BSIG_EINVAL
    assert 'traj_len' in err()                                            # summarizers.py:94
    assert lib.bsig_crosscorr_f64(one, one, one, 1, 12, 12, 3, 1, 0, 201, None, None) == _lib.BSIG_EINVAL
    assert 'ld_out' in err()
    assert lib.bsig_signature_f64(one, one, one, 1, 1, 2, 1, 0, 100, None) == _lib.BSIG_EINVAL
    assert lib.bsig_signature_f64(one, one, one, 1, 4, 2, 1, 4, 100000, None) == _lib.BSIG_EINVAL
    assert 'depth' in err()
    # refused, not spilled: a forced depth 3 beyond d = 22, and a path that does not fit the LDS of a workgroup
    assert lib.bsig_signature_f64(one, one, one, 1, 4, 19, 3, 3, 1 << 20, None) == _lib.BSIG_EUNSUPPORTED
    assert 'path dim' in err()
    assert lib.bsig_signature_f64(one, one, one, 1, 240, 18, 3, 3, 1 << 20, None) == _lib.BSIG_EUNSUPPORTED
    assert 'LDS' in err()
    # n = 0: nothing to do
    for rc in (lib.bsig_summary_start_f64(None, None, None, 0, 3, 3, 1, 1, 4, 8, None),
               lib.bsig_crosscorr_f64(None, None, None, 0, 12, 12, 3, 1, 0, 0, None, None),
               lib.bsig_signature_f64(None, None, None, 0, 4, 2, 1, 0, 0, None)):
        assert rc == _lib.BSIG_OK


@pytest.mark.skipif(not NO_GPU, reason='needs a machine without a GPU')
@pytest.mark.parametrize('name', SUMMARIZERS)
def test_double_summarizers_have_no_cpu_fallback(name):
    states, actions = torch.zeros(2, 12, 3, dtype=torch.float64), torch.zeros(2, 12, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        getattr(summarizers, name)(states, actions, dtype=torch.float64)
