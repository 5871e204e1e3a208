"""GPU checks of the general signature kernel (include/bsig_signature.h, csrc/signature_ex.h): depth 4..6, and
any depth on a chosen subset of channels, through ``summary_signatory(..., depth=, channels=)`` and BayesSim's
``sigDepth`` / ``sigChannels``.

The bound is derived, not measured: |got - ref| <= (L + 4 depth) u Sabs per term, u = 2^-24 (fp32) or 2^-53
(fp64).  One rounding per segment added to a term, at most four per Horner step (the reciprocal constant, its
multiply, the add, the multiply by the increment), ``depth`` steps.  Sabs is the same term of the signature of
the path whose increments are the absolute values of this path's increments: the sum of the absolute values of
every product that makes up the term, so a wrong term cannot hide behind a large row maximum.  The fp32 results
are compared with oracle/signature.py in fp64; the fp64 results with Chen's identity in exact rationals (a
fp64 reference's own error is the size of the bound) or, where those take too long -- thousands of rows, ten
thousand terms --, with Chen's identity in numpy's extended precision, whose own error is 2^-11 of the bound.

The worst ratios measured are recorded in profiles/signature_ex_NOTES.md."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@functools.lru_cache(maxsize=None)
def _traj(n, length, sd, ad, dtype=F32):
    """CPU trajectories, the same for every test that names the shape; never modified.  The double ones are
    the fp32 ones plus a 1e-3 * rand in double: genuine doubles."""
    gen = torch.Generator().manual_seed(100000 * n + 1000 * length + 10 * sd + ad)
    states, actions = torch.randn(n, length, sd, generator=gen), torch.rand(n, length, ad, generator=gen)
    if dtype == F64:
        states = states.double() + 1e-3 * torch.rand(n, length, sd, dtype=F64, generator=gen)
        actions = actions.double() + 1e-3 * torch.rand(n, length, ad, dtype=F64, generator=gen)
    return states, actions


def _gpu(*ts):
    return [t.to(DEV) for t in ts]


def _paths(states, actions, channels=None):
    """[t = 1..L | picked channels] in double."""
    n, length, _ = states.shape
    both = torch.cat([states, actions], dim=-1).double()
    if channels is not None:
        both = both[..., list(channels)]
    t = torch.arange(1, length + 1, dtype=F64).view(1, -1, 1).expand(n, -1, -1)
    return torch.cat([t, both], dim=-1)


def _oracle_refs(paths, depth):
    """oracle.signature.signature (fp64) of the paths and of their absolute-increment companions."""
    from oracle.signature import signature
    steps = (paths[:, 1:] - paths[:, :-1]).abs()
    pabs = torch.cat([torch.zeros_like(paths[:, :1]), torch.cumsum(steps, dim=1)], dim=1)
    return signature(paths, depth).numpy(), signature(pabs, depth).numpy()


def _extended_refs(paths, depth):
    """Chen's identity in numpy's extended precision (x87: a 64-bit significand) for the shapes where exact
    rationals take too long: its own error is about (L + depth) 2^-64 Sabs, 2^-11 of the fp64 bound."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63

    def chen(incs):
        n, _, d = incs.shape
        outer = lambda a, b: (a[:, :, None] * b[:, None, :]).reshape(n, -1)
        levels = [np.ones((n, 1), np.longdouble)] + [np.zeros((n, d ** k), np.longdouble) for k in range(1, depth + 1)]
        for step in range(incs.shape[1]):
            expo = [np.ones((n, 1), np.longdouble)]
            for k in range(1, depth + 1):
                expo.append(outer(expo[-1], incs[:, step]) / k)
            levels = [levels[0]] + [sum(outer(levels[j], expo[k - j]) for j in range(k + 1))
                                    for k in range(1, depth + 1)]
        return np.concatenate(levels[1:], axis=1)
    x = paths.numpy().astype(np.longdouble)
    incs = x[:, 1:] - x[:, :-1]
    return chen(incs), chen(np.abs(incs))


def _exact_signature(incs, depth):
    """Chen's identity in exact rationals: ``incs`` [L-1][d] Fractions -> the levels 1..depth, concatenated,
    each flattened in C order.  S <- S (x) exp(inc) per segment, exp(inc)_k = inc^(x)k / k!."""
    d = len(incs[0])
    outer = lambda a, b: [x * y for x in a for y in b]
    levels = [[Fraction(1)]] + [[Fraction(0)] * d ** k for k in range(1, depth + 1)]
    for inc in incs:
        expo = [[Fraction(1)]]
        for k in range(1, depth + 1):
            expo.append([x / k for x in outer(expo[-1], inc)])
        new = [levels[0]]
        for k in range(1, depth + 1):
            acc = [Fraction(0)] * d ** k
            for j in range(k + 1):
                acc = [p + q for p, q in zip(acc, outer(levels[j], expo[k - j]))]
            new.append(acc)
        levels = new
    return [x for lv in levels[1:] for x in lv]


def _exact_refs(path, depth):
    """One double path [L, d] -> (signature, Sabs), both exact."""
    rows = [[Fraction(float(v)) for v in row] for row in path.tolist()]
    incs = [[b - a for a, b in zip(r0, r1)] for r0, r1 in zip(rows[:-1], rows[1:])]
    return _exact_signature(incs, depth), _exact_signature([[abs(v) for v in inc] for inc in incs], depth)


def _check(what, got, ref, sabs, length, depth, dtype, times=1):
    bound = times * (length + 4 * depth) * U[dtype] * np.asarray(sabs)
    assert (bound > 0).all()
    ratio = float((np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(ref)) / bound).max())
    print('%s: worst |err| / bound = %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def _check_rows(got, n, width, dtype):
    assert got.dtype == dtype and got.is_cuda and tuple(got.shape) == (n, width)
    assert got.stride(1) == 1 and got.data_ptr() % 16 == 0


def _width(d, depth):
    return sum(d ** k for k in range(1, depth + 1))


# ------------------------------------------------------------------ 1. fp32 against the fp64 oracle
# (n, L, sd, ad, depth): one segment, odd d = 3 | Pendulum, 3905 terms | cartpole_more, 1554 terms |
# d = 10, the widest depth 4 | depth 6 | d = 4 at depth 6 and L = 64, the longest covered path |
# d = 11 at depth 4 (bsig_signature_ex_fits accepts it in fp32): 82 176 B of LDS, the fp32 kernel's dynamic-LDS
# limit raised (every other fp32 case stays below 64 KB)
DEEP = [(3, 2, 1, 1, 4), (2, 20, 3, 1, 5), (2, 20, 4, 1, 4), (2, 11, 7, 2, 4), (2, 50, 1, 1, 6), (2, 64, 2, 1, 6),
        (2, 3, 8, 2, 4)]


@pytest.mark.parametrize('case', DEEP, ids=[str(c) for c in DEEP])
def test_fp32_beyond_depth_3_against_the_fp64_oracle(B, case):
    n, length, sd, ad, depth = case
    states, actions = _traj(n, length, sd, ad)
    got = B.summary_signatory(*_gpu(states, actions), depth=depth)
    _check_rows(got, n, _width(1 + sd + ad, depth), F32)
    ref, sabs = _oracle_refs(_paths(states, actions), depth)
    _check('fp32 %s' % (case,), got.cpu().numpy(), ref, sabs, length, depth, F32)


# ------------------------------------------------------------------ 2. fp64 against exact rationals
# (L, sd, ad, depth, channels); the last two: the general kernel at depth 3 and 2, through a channel list
EXACT = [(2, 1, 1, 4, None), (5, 1, 1, 6, None), (6, 2, 1, 5, None), (4, 2, 1, 4, None),
         (5, 2, 1, 3, (0, 1, 2)), (4, 3, 2, 2, (4, 0))]


@pytest.mark.parametrize('case', EXACT, ids=[str(c) for c in EXACT])
def test_fp64_against_exact_rationals(B, case):
    length, sd, ad, depth, channels = case
    states, actions = _traj(2, length, sd, ad, F64)
    got = B.summary_signatory(*_gpu(states, actions), depth=depth, dtype=F64, channels=channels)
    _check_rows(got, 2, _width(1 + (sd + ad if channels is None else len(channels)), depth), F64)
    got = got.cpu().numpy()
    for r, path in enumerate(_paths(states, actions, channels)):
        ref, sabs = _exact_refs(path, depth)
        err = [abs(Fraction(float(g)) - x) for g, x in zip(got[r], ref)]
        bound = [(length + 4 * depth) * Fraction(U[F64]) * s for s in sabs]
        assert all(b > 0 for b in bound)
        ratio = max(float(e / b) for e, b in zip(err, bound))
        print('fp64 %s row %d: worst |err| / bound = %.3g' % (case, r, ratio))
        assert ratio <= 1.0, ratio


# (n, L, sd, ad, depth, channels): more than 64 KB of LDS in double -- d = 10 at depth 4, the widest covered
# (108 KB), and d = 22 at depth 3 through the identity list (99 KB)
WIDE64 = [(2, 11, 7, 2, 4, None), (2, 11, 17, 4, 3, tuple(range(21)))]


@pytest.mark.parametrize('case', WIDE64, ids=[str(c[:5]) for c in WIDE64])
def test_fp64_widest_shapes_against_an_extended_precision_reference(B, case):
    n, length, sd, ad, depth, channels = case
    states, actions = _traj(n, length, sd, ad, F64)
    got = B.summary_signatory(*_gpu(states, actions), depth=depth, dtype=F64, channels=channels)
    _check_rows(got, n, _width(1 + sd + ad, depth), F64)
    ref, sabs = _extended_refs(_paths(states, actions, channels), depth)
    _check('fp64 %s' % (case[:5],), got.cpu().numpy(), ref, sabs, length, depth, F64)


# ------------------------------------------------------------------ 3. known answer
@pytest.mark.parametrize('dtype', [F32, F64])
def test_two_point_path_is_the_exponential_of_its_increment(B, dtype):
    """[(1, 0, 0), (2, 2, 3)]: level k is D^(x)k / k! with D = (1, 2, 3); every term within 4 ulp."""
    states = torch.tensor([[[0.0], [2.0]]], dtype=dtype)
    actions = torch.tensor([[[0.0], [3.0]]], dtype=dtype)
    got = B.summary_signatory(*_gpu(states, actions), depth=4, dtype=dtype).cpu().numpy()[0]
    exact = _exact_signature([[Fraction(1), Fraction(2), Fraction(3)]], 4)
    assert len(exact) == 120 and exact[:3] == [1, 2, 3] and exact[-1] == Fraction(81, 24)
    np_dtype = np.float32 if dtype == F32 else np.float64
    for g, x in zip(got, exact):
        ulp = Fraction(float(np.spacing(np_dtype(float(x)))))
        assert abs(Fraction(float(g)) - x) <= 4 * ulp, (g, x)


# ------------------------------------------------------------------ 4. the general kernel at the old depths
OLD = [(3, 5, 2, 1, 3), (2, 11, 17, 4, 3), (3, 9, 30, 2, 2), (2, 11, 211, 20, 1)]


@pytest.mark.parametrize('case', OLD, ids=[str(c) for c in OLD])
def test_identity_channel_list_runs_the_general_kernel_at_depth_1_to_3(B, case, dtype=F32):
    n, length, sd, ad, depth = case
    states, actions = _traj(n, length, sd, ad, dtype)
    s, a = _gpu(states, actions)
    got = B.summary_signatory(s, a, depth=depth, channels=list(range(sd + ad)), dtype=dtype)
    _check_rows(got, n, _width(1 + sd + ad, depth), dtype)
    ref, sabs = _oracle_refs(_paths(states, actions), depth)
    _check('identity list %s' % (case,), got.cpu().numpy(), ref, sabs, length, depth, dtype)
    # channels=None: the existing kernels; both results lie within the bound of the exact value
    old = B.summary_signatory(s, a, depth=depth, dtype=dtype)
    _check('identity list against channels=None %s %s' % (case, dtype), got.cpu().numpy(), old.cpu().numpy(),
           sabs, length, depth, dtype, times=2)
    # the default depth with a list is the reference's rule on 1 + len(channels)
    assert B.signature_depth(1 + sd + ad) == depth
    assert torch.equal(B.summary_signatory(s, a, channels=list(range(sd + ad)), dtype=dtype), got)


# ------------------------------------------------------------------ 5. channel subsets
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_scrambled_picks_are_bitwise_the_rearranged_tensors(B, dtype):
    states, actions = _traj(3, 7, 4, 2, dtype)
    both = torch.cat([states, actions], dim=-1)
    s2, a2 = both[..., [5, 0]].contiguous(), both[..., [2]].contiguous()
    got = B.summary_signatory(*_gpu(states, actions), depth=4, channels=[5, 0, 2], dtype=dtype)
    _check_rows(got, 3, _width(4, 4), dtype)
    assert torch.equal(got, B.summary_signatory(*_gpu(s2, a2), depth=4, dtype=dtype))
    ref, sabs = _extended_refs(_paths(states, actions, [5, 0, 2]), 4)
    _check('scrambled picks %s' % dtype, got.cpu().numpy(), ref, sabs, 7, 4, dtype)


def test_shadowhand_shaped_subset_at_depth_3(B):
    """21 of 231 channels -- the first and the last of either tensor among them -- give d = 22: depth 3,
    11 154 terms, where the whole path allows depth 1 only."""
    states, actions = _traj(2, 11, 211, 20)
    picked = [0, 210, 211, 230] + list(range(40, 57))
    assert len(picked) == 21
    got = B.summary_signatory(*_gpu(states, actions), channels=picked)        # default depth: 3
    _check_rows(got, 2, 11154, F32)
    ref, sabs = _oracle_refs(_paths(states, actions, picked), 3)
    _check('ShadowHand subset', got.cpu().numpy(), ref, sabs, 11, 3, F32)
    again = B.summary_signatory(*_gpu(states, actions), channels=tuple(picked), depth=3)
    assert torch.equal(again, got)
    assert len([k for k in B.summarizers._channel_vectors if k[0] == tuple(picked)]) == 1     # uploaded once


def test_a_repeated_channel(B):
    states, actions = _traj(2, 6, 2, 1)
    got = B.summary_signatory(*_gpu(states, actions), depth=4, channels=[1, 1])
    _check_rows(got, 2, _width(3, 4), F32)
    ref, sabs = _oracle_refs(_paths(states, actions, [1, 1]), 4)
    _check('repeated channel', got.cpu().numpy(), ref, sabs, 6, 4, F32)


# ------------------------------------------------------------------ 6. more trajectories than workgroups
def _grid_cap(dtype):
    if dtype == F64:
        header = open(os.path.join(ROOT, 'include', 'bsig_f64.h')).read()
        return int(re.search(r'#define\s+BSIG_F64_SUMMARY_GRID_CAP\s+(\d+)', header).group(1))
    source = open(os.path.join(ROOT, 'bayes_sim_ig_amd', 'csrc', 'common.h')).read()
    a, b = re.search(r'constexpr int64_t kSummaryGridCap = (\d+) \* (\d+);', source).groups()
    return int(a) * int(b)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_more_trajectories_than_workgroups(B, dtype):
    n = _grid_cap(dtype) + 37
    assert n in (16384 + 37, 4096 + 37)
    states, actions = _traj(n, 2, 1, 1, dtype)
    got = B.summary_signatory(*_gpu(states, actions), depth=4, dtype=dtype)
    _check_rows(got, n, 120, dtype)
    ref, sabs = _extended_refs(_paths(states, actions), 4)
    _check('grid stride %s' % dtype, got.cpu().numpy(), ref, sabs, 2, 4, dtype)


# ------------------------------------------------------------------ 7. out= views
@pytest.mark.parametrize('dtype,start', [(F32, 2), (F64, 2), (F64, 1)], ids=['fp32+2', 'fp64+2', 'fp64+1'])
def test_out_view_with_a_wider_pitch_and_an_unaligned_start(B, dtype, start):
    states, actions = _traj(3, 7, 4, 2, dtype)
    s, a = _gpu(states, actions)
    plain = B.summary_signatory(s, a, depth=4, channels=[5, 0, 2], dtype=dtype)
    n, width = plain.shape
    pitch = width + 7
    base = torch.full((start + (n + 1) * pitch,), -77.0, dtype=dtype, device=DEV)
    view = base[start:].view(n + 1, pitch)
    assert view.data_ptr() % 16 == (start * base.element_size()) % 16
    res = B.summary_signatory(s, a, depth=4, channels=[5, 0, 2], out=view, dtype=dtype)
    assert res.data_ptr() == view.data_ptr() and res.stride(0) == pitch and tuple(res.shape) == (n, width)
    assert torch.equal(view[:n, :width], plain)
    assert (view[:n, width:] == -77.0).all() and (view[n] == -77.0).all() and (base[:start] == -77.0).all()


# ------------------------------------------------------------------ 8. reproducibility
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_two_runs_are_bitwise_equal(B, dtype):
    s, a = _gpu(*_traj(2, 20, 3, 1, dtype))
    first = B.summary_signatory(s, a, depth=5, dtype=dtype).clone()
    assert torch.equal(B.summary_signatory(s, a, depth=5, dtype=dtype), first)


# ------------------------------------------------------------------ 9. BayesSim
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_signatory', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (32, 32), 'lr': 1e-3, 'sigDepth': 4, 'sigChannels': [0, 1, 3]}


def _bayes_sim(B, cfg):
    torch.manual_seed(11)          # the start weights
    return B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01, 0.01]),
                      params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)


@functools.lru_cache(maxsize=None)
def _pendulum(B):
    theta, states, actions = B.pairs.pendulum_pairs(1000, 20, policy='random', seed=4, device=DEV)
    assert states.shape[1] == 21
    return theta, states, actions


def test_bayessim_fits_and_predicts_on_depth_4_of_three_channels(B):
    theta, states, actions = _pendulum(B)
    bs, twin = _bayes_sim(B, CFG), _bayes_sim(B, CFG)
    assert bs.model.input_dim == 340 and not bs.model._f64
    rows = B.summary_signatory(states, actions, depth=4, channels=[0, 1, 3])
    assert torch.equal(bs._summarize(states, actions), rows)
    np.random.seed(21), torch.manual_seed(22)
    logs = bs.fit(theta, states, actions)
    np.random.seed(21), torch.manual_seed(22)
    ref = twin.model.run_training(rows, theta, 100, 100)
    assert len(logs) == 1
    for key in ('train_loss', 'test_loss'):
        assert len(logs[0][key]) == 6 and np.isfinite(logs[0][key]).all()
        assert np.array_equal(np.asarray(logs[0][key]), np.asarray(ref[key])), key
    mog = bs.predict(states[:1], actions[:1])
    assert np.isfinite(mog.eval(theta[:1].cpu().numpy().astype(np.float64))).all()


def test_bayessim_in_double_on_depth_4_of_three_channels(B):
    theta, states, actions = _pendulum(B)
    bs = _bayes_sim(B, dict(CFG, dtype='float64', summaryDtype='float64'))
    assert bs.model.input_dim == 340 and bs.model._f64
    rows = bs._summarize(states, actions)
    assert rows.dtype == F64 and tuple(rows.shape) == (1000, 340)
    assert torch.equal(rows, B.summary_signatory(states, actions, depth=4, channels=[0, 1, 3], dtype=F64))
    np.random.seed(21), torch.manual_seed(22)
    logs = bs.fit(theta, states, actions)
    assert len(logs) == 1
    for key in ('train_loss', 'test_loss'):
        assert len(logs[0][key]) == 6 and np.isfinite(logs[0][key]).all()
