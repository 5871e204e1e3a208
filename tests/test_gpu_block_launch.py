"""A block of chunks in ONE launch of the persistent update kernel (bsig_fit_run_block) against the same fit
with one launch per chunk (BSIG_FIT_CHUNK_PER_LAUNCH=1): per-chunk logs, parameters and both Adam moment
buffers bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


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
    os.environ.pop('BSIG_FIT_CHUNK_PER_LAUNCH', None)


def _fit(B, d, k, n_feat, n, per_chunk, eps=None):
    import bench
    os.environ.pop('BSIG_FIT_CHUNK_PER_LAUNCH', None)
    if per_chunk:
        os.environ['BSIG_FIT_CHUNK_PER_LAUNCH'] = '1'
    if eps is not None:
        B.MDNN.EPS_NOISE = eps
    cfg = dict(task='synthetic', model='MDRFF', summarizer='summary_start', t=11, sd=5, ad=2, d=d, k=k,
               hidden=[], n_feat=n_feat, pairs=n)
    theta, states, actions = bench.synth_pairs(cfg, n, 3, DEV)
    bs = bench.build_gpu_model(B, cfg, DEV, 77)
    np.random.seed(5)
    torch.manual_seed(6)
    logs = bs.fit(theta, states, actions)
    torch.cuda.synchronize()
    m = bs.model
    assert B._lib.load().bsig_fit_is_persistent(m._plan) == 1
    return logs, m._flat.clone(), m._exp_avg.clone(), m._exp_avg_sq.clone(), getattr(m, '_block_launches', 0)


def _same(a, b):
    assert len(a[0]) == len(b[0])
    for c, (la, lb) in enumerate(zip(a[0], b[0])):
        for key in ('train_loss', 'test_loss'):
            assert np.array_equal(np.array(la[key], dtype=np.float64).view(np.int64),
                                  np.array(lb[key], dtype=np.float64).view(np.int64)), (c, key, la[key], lb[key])
    for i in (1, 2, 3):
        assert torch.equal(a[i], b[i]), ('params', 'exp_avg', 'exp_avg_sq')[i - 1]
    assert not torch.equal(a[1], torch.zeros_like(a[1]))


# K = 4: the DPP row; K = 10: the padded row (cfg2).  n: 3 chunks + a remainder of 400 pairs (320 + 80 held
# out) / of 7 pairs (5 + 2: fewer training rows than a minibatch, another n_test)
@pytest.mark.parametrize('eps', [None, 0.0])
@pytest.mark.parametrize('n', [3400, 3007])
@pytest.mark.parametrize('d,k,n_feat', [(3, 4, 256), (13, 10, 384)])
def test_block_launch_equals_one_launch_per_chunk(B, d, k, n_feat, n, eps):
    blk = _fit(B, d, k, n_feat, n, False, eps)
    one = _fit(B, d, k, n_feat, n, True, eps)
    assert blk[4] == 1 and one[4] == 0        # one block launch of 4 chunks / the switch selects the old path
    assert len(blk[0]) == 4
    _same(blk, one)


def test_a_one_pair_remainder_runs_on_its_own(B):
    blk = _fit(B, 3, 4, 256, 2001, False)
    one = _fit(B, 3, 4, 256, 2001, True)
    assert blk[4] == 1 and len(blk[0]) == 3
    _same(blk, one)


def test_the_most_chunks_of_a_block_at_a_tiny_shape(B):
    """FIT_BLOCK_CHUNKS chunks of 40 pairs, 7 updates of 16 rows each, an evaluation after EVERY update: the flag
    and granule tags run through the whole range of a launch, two evaluations are under way at every update."""
    B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH, B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 40, 7, 16
    n = 40 * B.BayesSim.FIT_BLOCK_CHUNKS
    blk = _fit(B, 3, 4, 256, n, False)
    one = _fit(B, 3, 4, 256, n, True)
    assert blk[4] == 1 and one[4] == 0 and len(blk[0]) == B.BayesSim.FIT_BLOCK_CHUNKS
    _same(blk, one)


def test_the_plan_runs_per_call_after_a_block_launch(B):
    """After a block launch the plan holds a complete binding of the block's first chunk: begin + run through the
    C ABI on it (what a caller timing one call's launch does) reads only buffers that are in place, and gives
    finite losses."""
    import bench
    cfg = dict(task='synthetic', model='MDRFF', summarizer='summary_start', t=11, sd=5, ad=2, d=3, k=4,
               hidden=[], n_feat=256, pairs=3000)
    theta, states, actions = bench.synth_pairs(cfg, 3000, 3, DEV)
    bs = bench.build_gpu_model(B, cfg, DEV, 77)
    bs.fit(theta, states, actions)
    m, L = bs.model, B._lib
    assert getattr(m, '_block_launches', 0) == 1
    lib, st = L.load(), L.stream()
    out = torch.zeros(13, device=DEV)
    for rep in range(2):
        L.check(lib.bsig_fit_begin(m._plan, 1234 + rep, 100, st))
        L.check(lib.bsig_fit_run(m._plan, 100, st))
    L.check(lib.bsig_fit_pack_logs(m._plan, 100, L.ptr(out), st))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[12] == 0 and np.all(np.isfinite(host[:12]))
