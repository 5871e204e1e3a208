"""GPU checks of the summarizers' fp64 mode (``dtype=torch.float64``: the double instantiation of csrc/summaries.h,
csrc/f64/summarizers_f64.hip, include/bsig_f64.h) through the public Python functions, against oracle/summarize.py and
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


def _views(n, width):
    """(flat NaN-filled buffer, its [n, width] view) twice: 16-byte aligned rows at an even pitch -- the 16-byte
    stores of the shared kernels -- and rows that start one element in at an odd pitch -- their element loops."""
    even = width + width % 2
    for off, pitch in ((0, even + 2), (1, even + 3)):
        buf = torch.full(((n + 1) * pitch + off,), float('nan'), dtype=F64, device=DEV)
        view = buf[off:off + n * pitch].view(n, pitch)[:, :width]
        assert view.data_ptr() % 16 == 8 * off and view.stride(0) % 2 == off
        yield buf, view


def _assert_untouched(buf, view):
    """every element of the buffer outside the view is still NaN"""
    n, width = view.shape
    pitch, off = view.stride(0), (view.data_ptr() - buf.data_ptr()) // 8
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[off:off + n * pitch].view(n, pitch)[:, :width] = False
    assert torch.isnan(buf[outside]).all() and not torch.isnan(view).any()


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


@functools.lru_cache(maxsize=None)
def _crosscorr_ref(shape, use_diff):
    """(oracle rows, S, A, the bound on mean and std per row) of a shape's trajectories.  Never modified."""
    from oracle import summarize as osum
    states, actions = _traj(*shape)
    sf, af = osum.crosscorr_features(states, actions, use_diff)
    return (osum.cross_correlation(states, actions, use_diff), sf.shape[1], af.shape[1],
            4 * (sf.shape[1] + 8) * U * sf.abs().max(dim=1).values)


def _assert_crosscorr(got, shape, use_diff):
    """the products bitwise, mean and std within the summation bound"""
    ref, s_dim, a_dim, tol = _crosscorr_ref(shape, use_diff)
    got = got.cpu()
    assert tuple(got.shape) == tuple(ref.shape) == (shape[0], s_dim * a_dim + 2)
    assert torch.equal(got[:, :s_dim * a_dim], ref[:, :s_dim * a_dim])
    for col, what in ((-2, 'mean'), (-1, 'std')):
        ratio = ((got[:, col] - ref[:, col]).abs() / tol).max().item()
        print('crosscorr %s diff=%d %s: worst |err| / bound = %.3g' % (shape, use_diff, what, ratio))
        assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('use_diff', [False, True])
@pytest.mark.parametrize('shape', CC_SHAPES)
def test_cross_correlation_against_the_oracle(B, shape, use_diff):
    states, actions = _traj(*shape)
    _, s_dim, a_dim, _ = _crosscorr_ref(shape, use_diff)
    got = B.cross_correlation(*_gpu(states, actions), use_state_diff=use_diff, dtype=F64)
    _check_rows(got, shape[0], s_dim * a_dim + 2)
    _assert_crosscorr(got, shape, use_diff)
    # the named summarizers are the same call
    named = (B.summary_corrdiff if use_diff else B.summary_corr)(*_gpu(states, actions), dtype=F64)
    assert torch.equal(named, got)


# The branches of crosscorr_kernel<double> (csrc/summaries.h), each at the smallest shape that reaches it, through
# both views of _views.  Rows of at most 2048 products (kSmallRow) take the lean variant: features fetched in place,
# every product checked, element stores into either view.  Longer rows take the fp32 body: into 16-byte aligned rows
# of even pitch it stores 16-byte words (a word of action features per thread where A is even and A <= 512, else the
# generic word loop, with an element tail where S A is odd), into the offset view elements.  (N, T, Ta, sd, ad):
CC_BRANCHES = {
    'lean': (3, 4, 4, 3, 1),                  # S = 8, A = 4
    'lean_even': (2, 3, 3, 3, 1),             # S A = 18
    'lean_odd': (2, 5, 5, 2, 1),              # S A = 25
    'lean_edge': (2, 8, 8, 33, 1),            # S A = 256 * 8 = 2048: the last lean row
    'lean_above_cap': ('cap+5', 3, 3, 2, 1),  # five workgroups take a second trajectory
    'prefetch_word': (2, 8, 8, 34, 1),        # S A = 264 * 8 = 2112: features prefetched in registers; a word per thread
    'inplace_tail': (2, 3, 3, 258, 1),        # sd - 1 = 257 > 256: fetched in place; S A = 771 * 3 is odd: tail
    'generic': (2, 5, 5, 85, 1),              # A = 5 is odd, S A = 420 * 5 even: the generic loop, no tail
    'generic_tail': (2, 5, 5, 84, 1),         # S A = 415 * 5: one element behind the last full word
    'wide_a': (2, 10, 10, 2, 52),             # A = 520 is even and above 512: the generic loop
    'above_cap': ('cap+5', 8, 8, 34, 1),      # five workgroups store a second trajectory, fetched by their prefetch
}


@pytest.mark.parametrize('use_diff', [False, True])
@pytest.mark.parametrize('name', list(CC_BRANCHES))
def test_cross_correlation_branches_of_the_shared_kernel(B, name, use_diff):
    shape = CC_BRANCHES[name]
    if shape[0] == 'cap+5':
        shape = (_grid_cap() + 5,) + shape[1:]
    s, a = _gpu(*_traj(*shape))
    _, s_dim, a_dim, _ = _crosscorr_ref(shape, use_diff)
    for buf, view in _views(shape[0], s_dim * a_dim + 2):
        got = B.cross_correlation(s, a, use_state_diff=use_diff, out=view, dtype=F64)
        assert got.data_ptr() == view.data_ptr()
        _assert_crosscorr(view, shape, use_diff)
        _assert_untouched(buf, view)


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


@functools.lru_cache(maxsize=None)
def _signature_case_refs(n, length, sd, ad, depth):
    """(signature_brute rows, their bound) of a case's trajectories.  Never modified."""
    from oracle import summarize as osum
    ref, sabs = _signature_refs(osum.signature_paths(*_traj(n, length, length, sd, ad)), depth)
    bound = (length + 6) * 2.0 ** -52 * sabs
    assert (bound > 0).all()
    return ref, bound


# The branches of signature3_kernel<double, DMAX> and signature12_kernel<double> (csrc/summaries.h), each through
# both views of _views (aligned rows: head, 16-byte words on whole lines, tail; the offset view: elements).
# (N, L, sd, ad, depth): d = 3, DMAX 8, odd d | d = 9, DMAX 16 | d = 17, DMAX 24 | d = 22, the widest, even d --
# all four with L sd <= threads: the next trajectory prefetched | L sd = 160 > 64 threads: fetched in place, even d |
# depth 2 and depth 1 at d = 23 and d = 111
SIG_BRANCHES = [(3, 5, 1, 1, 3), (2, 3, 6, 2, 3), (2, 3, 13, 3, 3), (2, 3, 18, 3, 3), (2, 40, 4, 1, 3),
                (2, 4, 19, 3, 2), (2, 4, 19, 3, 1), (2, 3, 100, 10, 2), (2, 3, 100, 10, 1)]


@pytest.mark.parametrize('case', SIG_BRANCHES, ids=[str(c) for c in SIG_BRANCHES])
def test_signature_branches_of_the_shared_kernels(B, case):
    n, length, sd, ad, depth = case
    d = 1 + sd + ad
    s, a = _gpu(*_traj(n, length, length, sd, ad))
    ref, bound = _signature_case_refs(*case)
    for buf, view in _views(n, sum(d ** k for k in range(1, depth + 1))):
        got = B.summary_signatory(s, a, depth=depth, out=view, dtype=F64)
        assert got.data_ptr() == view.data_ptr()
        ratio = (np.abs(view.cpu().numpy() - ref) / bound).max()
        print('signature %s pitch %d: worst |err| / bound = %.3g' % (case, view.stride(0), ratio))
        assert ratio <= 1.0, ratio
        _assert_untouched(buf, view)


def _signature_chen_longdouble(path):
    """Levels 1..3 of one path [L, d] by Chen's identity per segment in numpy's longdouble (x87: 2^-64 against the
    2^-53 of the values under test), for the one path too long for signature_brute's O(L^3) ordered triples.  The
    same definition (oracle/signature.py: S <- S (x) exp(delta)); its own rounding is 2^-11 of the bound."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    x = np.asarray(path, dtype=np.longdouble)
    d = x.shape[1]
    s1, s2, s3 = np.zeros(d, np.longdouble), np.zeros((d, d), np.longdouble), np.zeros((d, d, d), np.longdouble)
    for dl in x[1:] - x[:-1]:
        e2 = np.multiply.outer(dl, dl) / 2
        e3 = np.multiply.outer(e2, dl) / 3
        s3 = s3 + np.multiply.outer(s2, dl) + np.multiply.outer(s1, e2) + e3
        s2 = s2 + np.multiply.outer(s1, dl) + e2
        s1 = s1 + dl
    return np.concatenate([s1, s2.reshape(-1), s3.reshape(-1)])


def test_signature_depth_3_at_the_edge_of_a_workgroups_lds(B):
    """d = 22: path, increments and stage are 8 (44 L - 22 + 10648) bytes (profiles/f64_NOTES.md): 163 504 at
    L = 223, inside the 163 840 of a workgroup, and 163 856 at L = 224, refused with the message it always had.
    A forced depth 3 at d = 23 is refused as well."""
    from oracle import summarize as osum
    states, actions = _traj(1, 223, 223, 18, 3)
    got = B.summary_signatory(*_gpu(states, actions), dtype=F64)
    _check_rows(got, 1, 22 + 22 ** 2 + 22 ** 3)
    x = osum.signature_paths(states, actions)[0].numpy()
    steps = np.abs(x[1:] - x[:-1])
    xabs = np.concatenate([np.zeros_like(x[:1]), np.cumsum(steps, axis=0)], axis=0)
    ref, sabs = _signature_chen_longdouble(x), _signature_chen_longdouble(xabs)
    bound = (223 + 6) * 2.0 ** -52 * sabs
    assert (bound > 0).all()
    ratio = float((np.abs(got.cpu().numpy()[0].astype(np.longdouble) - ref) / bound).max())
    print('signature d = 22, L = 223: worst |err| / bound = %.3g' % ratio)
    assert ratio <= 1.0, ratio
    with pytest.raises(NotImplementedError) as refused:
        B.summary_signatory(*_gpu(*_traj(1, 224, 224, 18, 3)), dtype=F64)
    assert str(refused.value) == 'signature_f64: 163856 B of LDS needed (163840 in a workgroup)'
    with pytest.raises(NotImplementedError) as refused:
        B.summary_signatory(*_gpu(*_traj(2, 4, 4, 19, 3)), depth=3, dtype=F64)
    assert str(refused.value) == 'signature_f64: depth 3 needs path dim <= 22 (got 23)'


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
