"""The chunk protocol of run_training as every update engine leaves it in the device state block
(csrc/fit_protocol.h; bayes_sim_ig_amd/protocol.py): after a call of n_updates updates the block holds
step = n_updates, the evaluation counter = the number of logging points of mdnn.py:235, a clear flag
word, and -- the fp32 engines -- the jitter RNG pair (seed, 1 + n_updates + n_evals): fit_begin starts
the streams at 1 and every update and every evaluation takes one.  The Adam words (beta^t as doubles,
the two bias-correction floats) are bitwise those of the per-phase fp32 engine, and that engine's are
bitwise the closed form (running products in double, rounded to float once).  The fp64 engine keeps its
stream counter on the host: step, evaluations and flag only.

n_updates 1, 2, 6, 11, 12: `every` is 1 (1, 2, 6: every update is a logging point) or 2 (11, 12); the
last update's index is a multiple of `every` (11: index 10, the schedule holds its evaluation already)
or is not (12: index 11, the evaluation after the last update comes on top); calls shorter than five
updates (1, 2).  All assertions are exact."""
import functools
import os

import numpy as np
import pytest
import torch

from bayes_sim_ig_amd import protocol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENV = ('BSIG_NO_PERSISTENT', 'BSIG_NO_STREAMED_W1', 'BSIG_NO_STREAM_EVAL', 'BSIG_NO_WIDE_EVAL')
N_PAIRS, BATCH, D, K = 60, 7, 2, 3
ST_STEP, ST_EVAL, ST_FLAGS, ST_ADAM0, ST_RNG, ST_BETA_POW = 0, 1, 2, 4, 8, 12     # csrc/fit_protocol.h

RFF = dict(task='synthetic', model='MDRFF', summarizer='summary_start', t=11, sd=3, ad=1, d=D, k=K,
           hidden=[], n_feat=64, pairs=N_PAIRS)
TRUNK = dict(RFF, model='MDNN', hidden=[128, 128], n_feat=0)
# The smallest chunk tests/test_gpu_persistent_stream.py streams: its SMALL (I = 15362, D = 3, K = 5) on 60
# pairs with minibatches of 100.  Whether a first layer is streamed is decided by the workgroup count: 61
# k-slices x 4 tiles + the row owners + the small-weight workgroups.  At minibatch 7 this is 244 + 7 + 5 =
# 256 workgroups, the layer stays resident and the plan is the 'mdnn' engine again; at 100 it is streamed.
STREAMED = dict(TRUNK, summarizer='summary_corrdiff', t=8, sd=21, ad=12, d=3, k=5)
# engine: (config, minibatch, environment, double, lazy summaries, bsig_fit_is_persistent)
ENGINES = {'phase_f32': (RFF, BATCH, {'BSIG_NO_PERSISTENT': '1'}, False, False, 0),
           'linear': (RFF, BATCH, {}, False, False, 1),
           'mdnn': (TRUNK, BATCH, {}, False, False, 2),
           'mdnn_streamed': (STREAMED, 100, {}, False, True, 2),
           'phase_f64': (RFF, BATCH, {}, True, False, None)}


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
    yield
    pkg.MDNN.EPS_NOISE = old
    for k in ENV:
        os.environ.pop(k, None)


def _run(B, engine, n_updates):
    """(logs, state block as int32 on the host, seed of the call, model) of one call on `engine`."""
    import bench
    cfg, batch, env, double, lazy, _ = ENGINES[engine]
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    B.MDNN.EPS_NOISE = 1e-5
    theta, states, actions = bench.synth_pairs(cfg, N_PAIRS, 3, DEV)
    bs = bench.build_gpu_model(B, cfg, DEV, 77)
    if double:
        bs.model.double()
    seeds, draw = [], bs.model._seed
    bs.model._seed = lambda: seeds.append(draw()) or seeds[-1]
    summ = bs._summarize(states, actions, lazy=lazy)
    ids = np.random.RandomState(5).randint(0, protocol.split_rows(N_PAIRS, 0.2)[0], (n_updates, batch))
    logs = bs.model.run_training(summ, theta, n_updates, batch, ids_table=ids)
    torch.cuda.synchronize()
    assert len(seeds) == 1
    return logs, bs.model._bufs['state'].cpu().numpy().copy(), seeds[0], bs.model


@functools.lru_cache(maxsize=None)
def _phase_f32_adam_words(n_updates):
    """Words 4..5 and 12..15 of the block the per-phase fp32 engine leaves after n_updates updates."""
    import bayes_sim_ig_amd as pkg
    _, state, _, model = _run(pkg, 'phase_f32', n_updates)
    assert pkg._lib.load().bsig_fit_is_persistent(model._plan) == 0
    # closed form: the hyper-parameters are the plan's floats widened to double; IEEE double products, one
    # division and one square root, each correctly rounded on either side, then one rounding to float
    c = model._cfg()
    lr, beta1, beta2 = float(c.lr), float(c.beta1), float(c.beta2)
    b1t = b2t = 1.0
    for _ in range(n_updates):
        b1t, b2t = b1t * beta1, b2t * beta2
    assert state[ST_BETA_POW:ST_BETA_POW + 4].tobytes() == np.array([b1t, b2t], dtype=np.float64).tobytes()
    adam = np.array([lr / (1.0 - b1t), 1.0 / np.sqrt(1.0 - b2t)], dtype=np.float64).astype(np.float32)
    assert state[ST_ADAM0:ST_ADAM0 + 2].tobytes() == adam.tobytes()
    return state[ST_ADAM0:ST_ADAM0 + 2].tobytes(), state[ST_BETA_POW:ST_BETA_POW + 4].tobytes()


@pytest.mark.parametrize('n_updates', [1, 2, 6, 11, 12])
@pytest.mark.parametrize('engine', list(ENGINES))
def test_state_block_after_a_call(B, engine, n_updates):
    logs, state, seed, model = _run(B, engine, n_updates)
    lib = B._lib.load()
    _, _, _, double, _, kind = ENGINES[engine]
    if double:
        assert model._f64 and state.size >= 32
    else:
        assert lib.bsig_fit_is_persistent(model._plan) == kind
        if engine.startswith('mdnn'):     # (a streamed first layer answers 0: include/bsig.h)
            assert bool(lib.bsig_fit_accepts_factors(model._plan)) == (engine == 'mdnn')
    n_evals = len(protocol.eval_updates(n_updates)[1])
    assert len(logs['train_loss']) == len(logs['test_loss']) == n_evals
    assert int(state[ST_STEP]) == n_updates
    assert int(state[ST_EVAL]) == n_evals
    assert int(state[ST_FLAGS]) == 0
    if double:
        return
    rng = np.frombuffer(state[ST_RNG:ST_RNG + 4].tobytes(), dtype=np.uint64)
    assert (int(rng[0]), int(rng[1])) == (seed, 1 + n_updates + n_evals)
    adam, beta_pow = _phase_f32_adam_words(n_updates)
    assert state[ST_BETA_POW:ST_BETA_POW + 4].tobytes() == beta_pow
    assert state[ST_ADAM0:ST_ADAM0 + 2].tobytes() == adam
