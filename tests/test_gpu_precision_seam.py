"""The staging that fp32 and fp64 share in MDNN.run_training (row capacity, y_stage at the pitch round_up(D, 4),
the id buffer, the plan's capacities) at the smallest shapes where it can go wrong: one model fits 60 rows, then
90 (everything grows), then 60 again (everything is larger than needed), and every call must give, bit for bit,
what a fresh model started from the same parameters gives.  No tolerance: the same arithmetic on the same values
-- only buffer addresses, capacities and pitches differ."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_UPDATES, BATCH = 5, 10


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@pytest.fixture(autouse=True)
def _eps_guard():
    import bayes_sim_ig_amd as pkg
    old, pkg.MDNN.EPS_NOISE = pkg.MDNN.EPS_NOISE, 0.0
    yield
    pkg.MDNN.EPS_NOISE = old


def _model(B, dtype, box):
    torch.manual_seed(0)
    m = B.MDNN(input_dim=40, output_dim=3, output_lows=np.array([0.1, 0.2, 0.3]) if box else None,
               output_highs=np.array([1.0, 2.0, 3.0]) if box else None, n_gaussians=4, full_covariance=True,
               hidden_layers=(24, 24), activation=torch.nn.Tanh, lr=1e-3, device=DEV)
    return m.double() if dtype == torch.float64 else m


@pytest.mark.parametrize('box', [True, False], ids=['normalised', 'copied'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['float64', 'float32'])
def test_reused_and_grown_staging_is_bitwise_a_fresh_models(B, dtype, box):
    r = np.random.RandomState(7)
    calls = []
    for n in (60, 90, 60):
        n_train = n - int(n * 0.2)
        calls.append((torch.from_numpy(r.randn(n, 40).astype(np.float32) * 0.3).to(DEV),
                      torch.from_numpy((0.3 + 0.5 * r.rand(n, 3)).astype(np.float32)).to(DEV),
                      r.randint(0, n_train, (N_UPDATES, BATCH))))
    one = _model(B, dtype, box)
    for i, (x, y, ids) in enumerate(calls):
        start = {k: v.clone() for k, v in one.state_dict().items()}
        logs = one.run_training(x, y, N_UPDATES, BATCH, ids_table=ids)
        fresh = _model(B, dtype, box)
        fresh.load_state_dict(start)
        ref = fresh.run_training(x, y, N_UPDATES, BATCH, ids_table=ids)
        assert np.isfinite(logs['train_loss']).all() and np.isfinite(logs['test_loss']).all()
        assert logs == ref, (i, logs, ref)
        got, want = one.state_dict(), fresh.state_dict()
        for k in want:
            assert got[k].dtype == dtype and torch.equal(got[k], want[k]), (i, k)
            assert not torch.equal(got[k], start[k]), (i, k)          # (the call did train)
    assert one._bufs['cap_rows'] == 90 and one._bufs['y_stage'].dtype == dtype
    assert one._bufs['y_stage'].numel() >= 90 * 4                     # the shared pitch round_up(3, 4)
