"""Held-out evaluations in kernels BEHIND the persistent update launch of the linear heads (the default: the
launch snapshots its weight tiles at the evaluation points, fit_deferred_eval.hip evaluates from the snapshots)
against the same fit with the evaluations INSIDE the launch (BSIG_EVAL_IN_LAUNCH=1): per-chunk logs, parameters
and both Adam moment buffers bit for bit, once through a block launch and once with one launch per chunk."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('BSIG_FIT_CHUNK_PER_LAUNCH', 'BSIG_EVAL_IN_LAUNCH', 'BSIG_DEFERRED_EVAL_CAP_MB')
CONSTS = ('NUM_TRAIN_TRAJ_PER_BATCH', 'NUM_GRAD_UPDATES', 'MINIBATCH_SIZE')


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
    consts = {k: getattr(pkg.BayesSim, k) for k in CONSTS}
    yield
    pkg.MDNN.EPS_NOISE = old
    for k, v in consts.items():
        setattr(pkg.BayesSim, k, v)
    for k in SWITCHES:
        os.environ.pop(k, None)


def _fit(B, d, k, n_feat, n, per_chunk, in_launch, eps=None, cap_mb=None):
    """-> (logs, params, exp_avg, exp_avg_sq, block launches, [launches evaluated behind, inside, bytes held])"""
    import bench
    for key in SWITCHES:
        os.environ.pop(key, None)
    if per_chunk:
        os.environ['BSIG_FIT_CHUNK_PER_LAUNCH'] = '1'
    if in_launch:
        os.environ['BSIG_EVAL_IN_LAUNCH'] = '1'
    if cap_mb is not None:
        os.environ['BSIG_DEFERRED_EVAL_CAP_MB'] = str(cap_mb)
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
    lib = B._lib.load()
    assert lib.bsig_fit_is_persistent(m._plan) == 1
    where = (C.c_int64 * 3)()
    B._lib.check(lib.bsig_debug_fit_deferred(m._plan, where))
    return logs, m._flat.clone(), m._exp_avg.clone(), m._exp_avg_sq.clone(), getattr(m, '_block_launches', 0), list(where)


def _same(a, b):
    assert len(a[0]) == len(b[0])
    for c, (la, lb) in enumerate(zip(a[0], b[0])):
        for key in ('train_loss', 'test_loss'):
            assert np.array_equal(np.array(la[key], dtype=np.float64).view(np.int64),
                                  np.array(lb[key], dtype=np.float64).view(np.int64)), (c, key, la[key], lb[key])
    for i in (1, 2, 3):
        assert torch.equal(a[i], b[i]), ('params', 'exp_avg', 'exp_avg_sq')[i - 1]
    assert not torch.equal(a[1], torch.zeros_like(a[1]))


def _behind_equals_inside(B, d, k, n_feat, n, per_chunk, n_chunks, eps=None):
    new = _fit(B, d, k, n_feat, n, per_chunk, False, eps)
    old = _fit(B, d, k, n_feat, n, per_chunk, True, eps)
    assert new[4] == old[4] == (0 if per_chunk else 1)
    # every launch of the plan evaluated behind itself / inside itself (and then holds no snapshot memory); the
    # counters are the plan's, and a remainder chunk of another size may have been given a plan of its own
    assert new[5][0] >= 1 and new[5][1] == 0 and new[5][2] > 0
    assert old[5][0] == 0 and old[5][1] >= 1 and old[5][2] == 0
    if not per_chunk:
        assert new[5][0] == 1 and old[5][1] == 1
    assert len(new[0]) == n_chunks
    assert all(np.all(np.isfinite(c['test_loss'])) for c in new[0])
    _same(new, old)


# K = 4: the DPP row, NT = 1; K = 10: the padded row (cfg2's), NT = 2.  n: 3 chunks + a remainder of 400 pairs
# (320 + 80 held out) / of 7 pairs (5 + 2: fewer training rows than a minibatch, another n_test)
@pytest.mark.parametrize('per_chunk', [False, True])
@pytest.mark.parametrize('eps', [None, 0.0])
@pytest.mark.parametrize('n', [3400, 3007])
@pytest.mark.parametrize('d,k,n_feat', [(3, 4, 256), (13, 10, 384)])
def test_evaluations_behind_the_launch_equal_those_inside(B, d, k, n_feat, n, eps, per_chunk):
    _behind_equals_inside(B, d, k, n_feat, n, per_chunk, 4, eps)


@pytest.mark.parametrize('per_chunk', [False, True])
def test_sixty_held_out_rows_at_a_minibatch_of_64(B, per_chunk):
    """300 pairs per chunk, 37 updates of 64 rows: n_test = 60, one partial pass of held-out rows; evaluations
    every 7 updates and after the last."""
    B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH, B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 300, 37, 64
    _behind_equals_inside(B, 3, 4, 256, 600, per_chunk, 2)


@pytest.mark.parametrize('per_chunk', [False, True])
def test_two_passes_of_held_out_rows(B, per_chunk):
    """A 1000-pair chunk at a minibatch of 100: 200 held-out rows, two passes, the second full."""
    _behind_equals_inside(B, 3, 4, 256, 2000, per_chunk, 2)


@pytest.mark.parametrize('per_chunk', [False, True])
def test_a_snapshot_in_every_wait(B, per_chunk):
    """FIT_BLOCK_CHUNKS chunks of 40 pairs, 7 updates of 16 rows, an evaluation after EVERY update: every update
    snapshots, the snapshot of a chunk's last evaluation and that of the next chunk's first fall in consecutive
    waits, and the block's evaluations run in more than one group only if their products need it."""
    B.BayesSim.NUM_TRAIN_TRAJ_PER_BATCH, B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 40, 7, 16
    chunks = B.BayesSim.FIT_BLOCK_CHUNKS
    _behind_equals_inside(B, 3, 4, 256, 40 * chunks, per_chunk, chunks)


def test_a_plan_over_the_snapshot_cap_evaluates_inside_the_launch(B):
    """A cap below the block's snapshots (here: no snapshot memory at all) keeps the block's evaluations inside
    its launch, allocates nothing and gives the same logs."""
    ref = _fit(B, 3, 4, 256, 3400, False, False)
    capped = _fit(B, 3, 4, 256, 3400, False, False, cap_mb=0)
    assert ref[4] == 1 and ref[5][:2] == [1, 0] and ref[5][2] > 0
    assert capped[4] == 1 and capped[5] == [0, 1, 0]
    _same(capped, ref)
