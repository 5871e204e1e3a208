"""GPU checks of the summarizers' fp64 mode (``dtype=torch.float64``: csrc/f64/summarizers_f64.hip,
include/bsig_f64.h) through the public Python functions, against oracle/summarize.py and
oracle/signature.py run on the CPU on the same double inputs (torch.randn, fixed seeds).

Bounds -- derived, none of them tuned (U = 2^-53):
  * summary_start / summary_waypts, the products sf[i] * af[j] of the cross-correlation: bitwise (copies; one
    subtraction and one multiply have no order to disagree on).
  * mean and std of the S state features: 4 (S + 8) U max|sf| per row -- the summation bound of S terms, the
    deviation from the mean being at most 2 max|sf|.
  * signature: (L + 6) 2^-52 Sabs per element against signature_brute, Sabs = the same element of the signature
    of the path whose increments are the absolute values of this path's increments, i.e. the sum of the
    absolute values of all terms of the iterated sum: a rounding count times a condition number.

The measured worst ratios are recorded in profiles/f64_NOTES.md."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -53
F64 = torch.float64


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@functools.lru_cache(maxsize=None)
def _traj(n, t, ta, sd, ad):
    """Double trajectories (CPU), the same for every test that names the shape.  Never modified."""
    gen = torch.Generator().manual_seed(1000 * n + 100 * t + 10 * sd + ad)
    return torch.randn(n, t, sd, dtype=F64, generator=gen), torch.randn(n, ta, ad, dtype=F64, generator=gen)


def _gpu(*ts):
    return [t.to(DEV) for t in ts]


def _check_rows(got, n, width):
    assert got.dtype == F64 and got.is_cuda and tuple(got.shape) == (n, width)
    # a [:, :F] view of rows at a 16-byte aligned pitch
    assert got.stride(1) == 1 and (n == 1 or got.stride(0) % 2 == 0) and got.data_ptr() % 16 == 0


# ------------------------------------------------------------------ 1. summary_start / summary_waypts
START_SHAPES = [(1, 3, 2, 1, 1), (5, 12, 11, 3, 2), (3, 10, 10, 2, 1)]     # pads both | crops | as long as max_t = 10


@pytest.mark.parametrize('max_t', [10, 4])
@pytest.mark.parametrize('shape', START_SHAPES)
def test_start_and_waypts_are_bitwise_the_oracle(B, shape, max_t):
    from oracle import summarize as osum
    n, _, _, sd, ad = shape
    states, actions = _traj(*shape)
    s, a = _gpu(states, actions)
    got = B.summary_start(s, a, max_t=max_t, dtype=F64)
    _check_rows(got, n, max_t * (sd + ad))
    assert torch.equal(got.cpu(), osum.summary_start(states, actions, max_t))
    got = B.summary_waypts(s, a, n_waypts=max_t, dtype=F64)
    _check_rows(got, n, max_t * (sd + ad))
    assert torch.equal(got.cpu(), osum.summary_waypts(states, actions, max_t))


# ------------------------------------------------------------------ 2. cross-correlation
# (N, T, Ta, sd, ad): shorter than the window | waypoint selection | sd > 50: five waypoints | the fewest features |
# S + A = 8400 doubles, 67 200 B of LDS: the smallest launch that has to raise the kernel's dynamic-LDS limit
CC_SHAPES = [(2, 3, 3, 2, 1), (4, 20, 20, 3, 3), (2, 12, 12, 52, 1), (1, 2, 2, 2, 1), (2, 4, 4, 2100, 1)]


@pytest.mark.parametrize('use_diff', [False, True])
@pytest.mark.parametrize('shape', CC_SHAPES)
def test_cross_correlation_against_the_oracle(B, shape, use_diff):
    from oracle import summarize as osum
    n = shape[0]
    states, actions = _traj(*shape)
    ref = osum.cross_correlation(states, actions, use_diff)
    sf, af = osum.crosscorr_features(states, actions, use_diff)
    s_dim, a_dim = sf.shape[1], af.shape[1]
    got = B.cross_correlation(*_gpu(states, actions), use_state_diff=use_diff, dtype=F64)
    _check_rows(got, n, s_dim * a_dim + 2)
    got = got.cpu()
    assert torch.equal(got[:, :s_dim * a_dim], ref[:, :s_dim * a_dim])
    tol = 4 * (s_dim + 8) * U * sf.abs().max(dim=1).values
    for col, what in ((-2, 'mean'), (-1, 'std')):
        ratio = ((got[:, col] - ref[:, col]).abs() / tol).max().item()
        print('crosscorr %s diff=%d %s: worst |err| / bound = %.3g' % (shape, use_diff, what, ratio))
        assert ratio <= 1.0, (what, ratio)
    # the named summarizers are the same call
    named = (B.summary_corrdiff if use_diff else B.summary_corr)(*_gpu(states, actions), dtype=F64)
    assert torch.equal(named.cpu(), got)


def test_cross_correlation_of_equal_state_features_has_std_zero(B):
    """The fewest features a call can have are S = 2 (T > 1 is asserted, sd >= 2).  Equal ones: the mean is that
    value and every deviation from it is zero, so the two-pass std is 0 exactly (a one-pass
    sum-of-squares formula would leave a rounding residue)."""
    states = torch.full((1, 2, 2), 0.75, dtype=F64)
    actions = torch.randn(1, 2, 1, dtype=F64, generator=torch.Generator().manual_seed(3))
    got = B.summary_corr(*_gpu(states, actions), dtype=F64).cpu()
    assert got[0, -2].item() == 0.75 and got[0, -1].item() == 0.0


def test_cross_correlation_nan_raises_like_the_fp32_path(B):
    states, actions = _traj(4, 20, 20, 3, 3)
    states = states.clone()
    states[2, 1, 0] = float('nan')
    for fn in (B.summary_corr, B.summary_corrdiff):
        with pytest.raises(AssertionError):
            fn(*_gpu(states, actions), dtype=F64)
        with pytest.raises(AssertionError):
            fn(*_gpu(states, actions))


@pytest.mark.parametrize('use_diff', [False, True])
def test_fp32_inputs_are_widened_exactly(B, use_diff):
    states, actions = (t.float() for t in _traj(4, 20, 20, 3, 3))
    a = B.cross_correlation(*_gpu(states, actions), use_state_diff=use_diff, dtype=F64)
    b = B.cross_correlation(*_gpu(states.double(), actions.double()), use_state_diff=use_diff, dtype=F64)
    assert a.dtype == F64 and torch.equal(a, b)
    # and the fp32 path still narrows a double input: no caller sees a change
    c = B.cross_correlation(*_gpu(states.double(), actions.double()), use_state_diff=use_diff)
    assert c.dtype == torch.float32 and torch.equal(c, B.cross_correlation(*_gpu(states, actions),
                                                                           use_state_diff=use_diff))


# ------------------------------------------------------------------ 3. signature
def _grid_cap():
    header = open(os.path.join(ROOT, 'include', 'bsig_f64.h')).read()
    return int(re.search(r'#define\s+BSIG_F64_SUMMARY_GRID_CAP\s+(\d+)', header).group(1))


# (N, L, sd, ad, depth): one segment | odd d | the cartpole_more row, width 258 | d = 22, the widest depth 3
# (86 064 B of LDS: above the 64 KB a launch gets without the kernel's limit raised) | d = 23: depth 2 |
# d = 111: depth 1 | depth 2 forced | more trajectories than workgroups (N filled in below) | depth 2 forced on
# L * d = 90 * 101 doubles, 72 720 B of LDS: the depth-1/2 kernel's limit raised
SIG_CASES = [(3, 2, 1, 1, None), (3, 5, 2, 1, None), (2, 20, 4, 1, None), (2, 3, 18, 3, None),
             (2, 4, 19, 3, None), (2, 3, 100, 10, None), (2, 5, 2, 1, 2), ('cap+37', 2, 1, 1, None),
             (2, 90, 90, 10, 2)]
SIG_DEPTHS = [3, 3, 3, 3, 2, 1, 2, 3, 2]


def _signature_refs(paths, depth):
    """signature_brute of every path and of its absolute-increment companion (the condition number's path:
    the running sums of |increments|, whose increments are those absolute values to within their rounding)."""
    from oracle.signature import signature_brute
    x = paths.numpy()
    steps = np.abs(x[:, 1:] - x[:, :-1])
    xabs = np.concatenate([np.zeros_like(x[:, :1]), np.cumsum(steps, axis=1)], axis=1)
    ref = np.stack([signature_brute(p, depth) for p in x])
    sabs = np.stack([signature_brute(p, depth) for p in xabs])
    return ref, sabs


@pytest.mark.parametrize('case,want_depth', list(zip(SIG_CASES, SIG_DEPTHS)), ids=[str(c) for c in SIG_CASES])
def test_signature_against_the_brute_force_iterated_sums(B, case, want_depth):
    from oracle import summarize as osum
    n, length, sd, ad, depth = case
    if n == 'cap+37':
        n = _grid_cap() + 37
    states, actions = _traj(n, length, length, sd, ad)
    d = 1 + sd + ad
    assert (depth or osum.signature_depth(d)) == want_depth
    got = B.summary_signatory(*_gpu(states, actions), depth=depth, dtype=F64)
    _check_rows(got, n, sum(d ** k for k in range(1, want_depth + 1)))
    ref, sabs = _signature_refs(osum.signature_paths(states, actions), want_depth)
    bound = (length + 6) * 2.0 ** -52 * sabs
    assert (bound > 0).all()
    ratio = (np.abs(got.cpu().numpy() - ref) / bound).max()
    print('signature %s: worst |err| / bound = %.3g' % (case, ratio))
    assert ratio <= 1.0, ratio


def test_signature_depth_3_refuses_what_does_not_fit(B):
    """d = 22 at L = 240: path + increments + d^3 stage is 169 KB, more than the 160 KB of a workgroup:
    refused, not spilled.  A forced depth 3 beyond d = 22 is refused too."""
    states, actions = _traj(1, 240, 240, 18, 3)
    with pytest.raises(NotImplementedError, match='LDS'):
        B.summary_signatory(*_gpu(states, actions), dtype=F64)
    with pytest.raises(NotImplementedError, match='path dim'):
        B.summary_signatory(*_gpu(*_traj(2, 4, 4, 19, 3)), depth=3, dtype=F64)


# ------------------------------------------------------------------ 4. out=
def test_out_buffer_is_filled_in_place(B):
    calls = [(lambda s, a, **kw: B.summary_start(s, a, max_t=4, **kw), (5, 12, 11, 3, 2)),
             (lambda s, a, **kw: B.summary_corrdiff(s, a, **kw), (4, 20, 20, 3, 3)),
             (lambda s, a, **kw: B.summary_signatory(s, a, **kw), (3, 5, 5, 2, 1))]
    for fn, shape in calls:
        s, a = _gpu(*_traj(*shape))
        plain = fn(s, a, dtype=F64)
        n, width = plain.shape
        buf = torch.full((n + 1, width + 5), float('nan'), dtype=F64, device=DEV)      # a wider, odd pitch
        res = fn(s, a, out=buf, dtype=F64)
        assert res.data_ptr() == buf.data_ptr() and res.stride(0) == width + 5 and tuple(res.shape) == (n, width)
        assert torch.equal(buf[:n, :width], plain)
        assert torch.isnan(buf[:n, width:]).all() and torch.isnan(buf[n]).all()        # nothing else is written
        with pytest.raises(AssertionError):
            fn(s, a, out=torch.empty(n, width + 5, dtype=torch.float32, device=DEV), dtype=F64)
        with pytest.raises(AssertionError):          # and the fp32 path keeps refusing a double buffer
            fn(s, a, out=buf)


# ------------------------------------------------------------------ 5. BayesSim
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_signatory', 'trainTrajLen': 8, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3, 'dtype': 'float64', 'summaryDtype': 'float64'}


def _bayes_sim(B, cfg):
    torch.manual_seed(11)          # the start weights
    return B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01, 0.01]),
                      params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)


def test_bayessim_summarizes_fits_and_predicts_in_double(B):
    theta, states, actions = B.pairs.pendulum_pairs(120, 7, policy='random', seed=4, device=DEV)
    assert states.shape[1] == 8
    bs, twin = _bayes_sim(B, CFG), _bayes_sim(B, CFG)
    assert bs.model._f64
    rows = bs._summarize(states, actions)
    assert rows.dtype == F64
    assert torch.equal(rows, B.summary_signatory(states, actions, dtype=F64))
    old = (B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE)
    B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = 10, 8
    try:
        np.random.seed(21), torch.manual_seed(22)
        logs = bs.fit(theta, states, actions)
        np.random.seed(21), torch.manual_seed(22)
        ref = twin.model.run_training(rows, theta, 10, 8, test_frac=B.BayesSim.TEST_FRACTION)
    finally:
        B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = old
    assert len(logs) == 1
    for key in ('train_loss', 'test_loss'):
        assert len(logs[0][key]) == 6 and np.isfinite(logs[0][key]).all()
        assert np.array_equal(np.asarray(logs[0][key]), np.asarray(ref[key])), key
    mog = bs.predict(states[:1], actions[:1])
    assert mog.a.dtype == np.float64 and np.isfinite(mog.a).all() and abs(mog.a.sum() - 1.0) <= 1e-12
    # the fp32 rows would have been another fit: the double rows are not the fp32 rows widened
    assert not torch.equal(rows, B.summary_signatory(states, actions).double())


def test_bayessim_summary_dtype_with_corrdiff_and_without_the_key(B):
    _, states, actions = B.pairs.pendulum_pairs(120, 7, policy='random', seed=4, device=DEV)
    bs = _bayes_sim(B, dict(CFG, summarizerFxn='summary_corrdiff'))
    rows = bs._summarize(states, actions)
    assert rows.dtype == F64 and torch.equal(rows, B.summary_corrdiff(states, actions, dtype=F64))
    # (what fit() asks for: a deferred flag, lazy rows -- a double model gets materialised double rows)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert torch.equal(bs._summarize(states, actions, flag, lazy=True), rows) and int(flag.item()) == 0
    for name in ('summary_signatory', 'summary_corrdiff'):
        cfg = {k: v for k, v in dict(CFG, summarizerFxn=name).items() if k != 'summaryDtype'}
        plain = _bayes_sim(B, cfg)
        assert plain.model._f64
        rows = plain._summarize(states, actions)
        assert rows.dtype == torch.float32 and torch.equal(rows, getattr(B, name)(states, actions))
