"""Every summarizer, the embedding and the RFF map launch on the device their rows live on, whichever device is
current (``_lib.device_stream``): with cuda:0 current and the trajectories (for ``summary_kme`` the embedding
too) on cuda:1, every call below returns rows on cuda:1 that are, bit for bit, the rows of the same call made
entirely on cuda:0, and leaves cuda:0 current.  Needs two GPUs; skipped on a machine that shows one.

The shapes are the smallest that reach every kernel: N = 5, T = 6, sd = 3, ad = 1."""
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')]
F32, F64 = torch.float32, torch.float64
N, T, SD, AD = 5, 6, 3, 1
LENGTHS = [6, 5, 4, 3, 2]


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _trajectories():
    gen = torch.Generator().manual_seed(11)
    return torch.randn(N, T, SD, generator=gen), torch.rand(N, T, AD, generator=gen)


def _kme(B, s, a, dtype, **kwargs):
    emb = B.KernelMeanEmbedding(SD, AD, n_feat=8, device=s.device)
    emb.set_scale(torch.ones(emb.row_dim))
    return B.summary_kme(s, a, emb, dtype=dtype, **kwargs)


def _rff(B, s, a, dtype):
    x = torch.randn(N, 4, generator=torch.Generator().manual_seed(12)).to(s.device)
    return B.RFF(8, 4, 1.5, device=s.device).to_features(x)


# name -> the call, from the package, the trajectories on the device under test and the dtype
CALLS = {
    'summary_start': lambda B, s, a, dt: B.summary_start(s, a, dtype=dt),
    'summary_corr': lambda B, s, a, dt: B.summary_corr(s, a, dtype=dt),
    'summary_corrdiff': lambda B, s, a, dt: B.summary_corrdiff(s, a, dtype=dt),
    'summary_corrdiff_lazy': lambda B, s, a, dt: B.summary_corrdiff(s, a, lazy=True).materialize(),
    'summary_signatory': lambda B, s, a, dt: B.summary_signatory(s, a, dtype=dt),
    'summary_signatory_depth4': lambda B, s, a, dt: B.summary_signatory(s, a, depth=4, channels=[0, 1, 3], dtype=dt),
    'summary_logsignature': lambda B, s, a, dt: B.summary_logsignature(s, a, depth=2, dtype=dt),
    'summary_xcorr': lambda B, s, a, dt: B.summary_xcorr(s, a, max_lag=2, dtype=dt),
    'summary_xcorr_lengths': lambda B, s, a, dt: B.summary_xcorr(s, a, max_lag=2, dtype=dt, lengths=LENGTHS),
    'summary_sysid': lambda B, s, a, dt: B.summary_sysid(s, a, dtype=dt),
    'summary_kme': _kme,
    'summary_kme_lengths': lambda B, s, a, dt: _kme(B, s, a, dt, lengths=LENGTHS),
    'rff_to_features': _rff,
}
FP32_ONLY = ('summary_corrdiff_lazy', 'rff_to_features')
CASES = [pytest.param(name, dt, id='%s-%s' % (name, 'fp32' if dt == F32 else 'fp64'))
         for name in CALLS for dt in (F32, F64) if dt == F32 or name not in FP32_ONLY]


@pytest.mark.parametrize('name,dtype', CASES)
def test_a_call_runs_on_the_device_of_its_rows_not_on_the_current_one(B, name, dtype):
    states, actions = _trajectories()
    with torch.cuda.device(0):
        want = CALLS[name](B, states.to('cuda:0'), actions.to('cuda:0'), dtype)
        got = CALLS[name](B, states.to('cuda:1'), actions.to('cuda:1'), dtype)
        assert torch.cuda.current_device() == 0
    assert want.device == torch.device('cuda:0') and got.device == torch.device('cuda:1')
    assert got.dtype == want.dtype == dtype and got.shape == want.shape and got.shape[0] == N
    assert torch.equal(got.cpu(), want.cpu())
