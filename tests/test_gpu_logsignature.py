"""GPU checks of the log-signature kernel (include/bsig_logsignature.h, csrc/logsignature.h) through
``summary_logsignature(..., depth=, channels=)`` and BayesSim's ``'summarizerFxn': 'summary_logsignature'``.

What is compared with: tests/logsig_cases.py -- the tensor-log SERIES on a signature made by Chen's identity
(fp64: oracle.signature.signature; exact rationals; numpy's extended precision), read at Lyndon words that were
enumerated by their definition.  The kernel evaluates something else, the per-word sum over cuts.

The bounds are derived, not measured.  u = 2^-24 (fp32) or 2^-53 (fp64), k = |w|, c = L + 4 depth the
per-term constant of the signature (tests/test_gpu_signature_ex.py: |S^_u - S_u| <= c u Sabs_u, Sabs the
signature of the absolute-increment path, so |S_u| <= Sabs_u), and
    A_w = sum over the 2^(k-1) cuts of w into u1..un of (1/n) Sabs_u1 ... Sabs_un.
The kernel computes, per cut, p = S^_u1 * ... * S^_un from the left (n - 1 roundings), then
acc = fma(p, +-rcp[n], acc) in ascending mask order, starting from acc = S^_w (the cut with n = 1).
  * The factors.  To first order the error of a product of n <= k factors is the sum of the factors' errors
    times the other factors: at most n c u prod Sabs_ui <= k c u prod Sabs_ui.  Summed over the cuts with the
    weights 1/n: k c u A_w.
  * The product's own roundings.  n - 1 multiplies, the constant 1/n (one rounding; exact for n = 1, 2, 4),
    and the multiply by it -- fused here, counted all the same: at most n + 1 <= k + 1 roundings, each u times
    a term that is at most (1/n) prod Sabs_ui.  Summed over the cuts: (k + 1) u A_w.
  * The sum.  2^(k-1) - 1 additions, each rounds a partial sum that is at most A_w (to first order):
    (2^(k-1) - 1) u A_w.
End to end: |got_w - ref_w| <= (k c + 2^(k-1) + k + 1) u A_w, to first order in u as the signature's bound
is.  With the factors GIVEN -- the device's own signature S^, which the kernel holds bit for bit -- the first
item is gone: |got_w - log(S^)_w| <= (2^(k-1) + k + 1) u A^_w with A^_w made of |S^|.  For k = 1 the output
is S^_w itself and the test asks for equal bits.

The worst ratios measured, and the fp32 error relative to the value, are in profiles/logsignature_NOTES.md."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import logsig_cases as LC
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


@functools.lru_cache(maxsize=None)
def _words(d, depth):
    words = LC.lyndon_words(d, depth)
    assert len(words) == LC.witt(d, depth)
    return words


def _factor(words, length, depth, end_to_end=True):
    """per word: k c + 2^(k-1) + k + 1, or 2^(k-1) + k + 1 with the factors given"""
    c = length + 4 * depth
    return np.array([(len(w) * c if end_to_end else 0) + 2 ** (len(w) - 1) + len(w) + 1 for w in words],
                    dtype=np.float64)


def _check(what, got, ref, mag, factor, dtype):
    bound = factor[None, :] * U[dtype] * np.asarray(mag, dtype=np.longdouble)
    assert (bound > 0).all()
    err = np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    ratio = float((err / bound).max())
    tiny = np.finfo(np.float32 if dtype == F32 else np.float64).tiny
    rel = float((err / np.maximum(np.abs(np.asarray(ref, dtype=np.longdouble)), tiny)).max())
    print('%s: worst |err| / bound = %.3g, worst |err| / max(|value|, tiny) = %.3g' % (what, ratio, rel))
    assert ratio <= 1.0, (what, ratio)


def _check_rows(got, n, width, dtype):
    assert got.dtype == dtype and got.is_cuda and tuple(got.shape) == (n, width)
    assert got.stride(1) == 1 and got.data_ptr() % 16 == 0


def _fp64_refs(paths, depth):
    """(log-signature by the series on oracle.signature.signature, A_w), everything in fp64."""
    from oracle.signature import signature
    d = paths.shape[2]
    steps = (paths[:, 1:] - paths[:, :-1]).abs()
    pabs = torch.cat([torch.zeros_like(paths[:, :1]), torch.cumsum(steps, dim=1)], dim=1)
    words = _words(d, depth)
    return (LC.logsignature(signature(paths, depth).numpy(), d, depth, words),
            LC.magnitude(signature(pabs, depth).numpy(), words, d))


def _extended_refs(paths, depth):
    """The same in numpy's extended precision (x87: a 64-bit significand), Chen's identity restated: its own
    error is 2^-11 of the fp64 bound."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    d = paths.shape[2]
    incs, absincs = LC.increments(paths)
    words = _words(d, depth)
    return (LC.logsignature(LC.chen(incs, depth), d, depth, words),
            LC.magnitude(LC.chen(absincs, depth), words, d))


# ------------------------------------------------------------------ 1. the epilogue in isolation
ISOLATED = [(5, 1, 1, 6), (6, 2, 1, 5), (11, 7, 2, 4)]


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', ISOLATED, ids=[str(c) for c in ISOLATED])
def test_epilogue_on_the_devices_own_signature(B, case, dtype):
    """The log kernel holds, when a path ends, the bits summary_signatory returns through the identity channel
    list (the same path loop): the series on THAT signature, in extended precision, is the reference, and the
    bound has no term for the signature's error."""
    length, sd, ad, depth = case
    d = 1 + sd + ad
    s, a = _gpu(*_traj(3, length, sd, ad, dtype))
    sig = B.summary_signatory(s, a, depth=depth, channels=list(range(sd + ad)), dtype=dtype)
    got = B.summary_logsignature(s, a, depth=depth, dtype=dtype)
    words = _words(d, depth)
    _check_rows(got, 3, len(words), dtype)
    assert torch.equal(got[:, :d], sig[:, :d])                           # level 1: equal bits
    assert torch.equal(B.summary_logsignature(s, a, depth=depth, channels=list(range(sd + ad)), dtype=dtype), got)
    sig = sig.cpu().numpy().astype(np.longdouble)
    ref = LC.logsignature(sig, d, depth, words)
    _check('epilogue %s %s' % (case, dtype), got.cpu().numpy(), ref, LC.magnitude(np.abs(sig), words, d),
           _factor(words, length, depth, end_to_end=False), dtype)


# ------------------------------------------------------------------ 2. fp32 end to end against the fp64 series
# (n, L, sd, ad, depth): one segment, odd d | Pendulum at depth 5 | d = 10, the widest depth 4 | depth 6 |
# d = 4 at depth 6 and L = 64, the longest covered path | d = 22: 3795 words, more than the 1024 threads |
# d = 11 at depth 4 (bsig_signature_ex_fits accepts it in fp32): 82 176 B of LDS, the fp32 kernel's dynamic-LDS
# limit raised (every other fp32 case stays below 64 KB; in double WIDE64's first case plans 107 568 B)
DEEP = [(3, 2, 1, 1, 4), (2, 20, 3, 1, 5), (2, 11, 7, 2, 4), (2, 50, 1, 1, 6), (2, 64, 2, 1, 6), (2, 11, 19, 2, 3),
        (2, 3, 8, 2, 4)]


@pytest.mark.parametrize('case', DEEP, ids=[str(c) for c in DEEP])
def test_fp32_against_the_fp64_series(B, case):
    n, length, sd, ad, depth = case
    states, actions = _traj(n, length, sd, ad)
    got = B.summary_logsignature(*_gpu(states, actions), depth=depth)
    words = _words(1 + sd + ad, depth)
    _check_rows(got, n, len(words), F32)
    ref, mag = _fp64_refs(_paths(states, actions), depth)
    _check('fp32 %s' % (case,), got.cpu().numpy(), ref, mag, _factor(words, length, depth), F32)


# ------------------------------------------------------------------ 3. fp64 end to end
# (L, sd, ad, depth, channels)
EXACT = [(2, 1, 1, 4, None), (5, 1, 1, 6, None), (6, 2, 1, 5, None), (5, 2, 1, 3, (0, 1, 2))]


@pytest.mark.parametrize('case', EXACT, ids=[str(c) for c in EXACT])
def test_fp64_against_exact_rationals(B, case):
    length, sd, ad, depth, channels = case
    d = 1 + (sd + ad if channels is None else len(channels))
    states, actions = _traj(2, length, sd, ad, F64)
    got = B.summary_logsignature(*_gpu(states, actions), depth=depth, dtype=F64, channels=channels)
    words = _words(d, depth)
    _check_rows(got, 2, len(words), F64)
    got = got.cpu().numpy()
    incs, absincs = LC.increments(_paths(states, actions, channels), exact=True)
    ref = LC.logsignature(LC.chen(incs, depth), d, depth, words)
    mag = LC.magnitude(LC.chen(absincs, depth), words, d)
    factor = _factor(words, length, depth)
    worst = 0.0
    for r in range(2):
        for col in range(len(words)):
            bound = int(factor[col]) * Fraction(U[F64]) * mag[r, col]
            assert bound > 0
            worst = max(worst, float(abs(Fraction(float(got[r, col])) - ref[r, col]) / bound))
    print('fp64 %s: worst |err| / bound = %.3g' % (case, worst))
    assert worst <= 1.0, worst


# more than 64 KB of LDS in double: d = 10 at depth 4, the widest covered, and d = 22 at depth 3
WIDE64 = [(2, 11, 7, 2, 4), (2, 11, 19, 2, 3)]


@pytest.mark.parametrize('case', WIDE64, ids=[str(c) for c in WIDE64])
def test_fp64_widest_shapes_against_an_extended_precision_reference(B, case):
    n, length, sd, ad, depth = case
    states, actions = _traj(n, length, sd, ad, F64)
    got = B.summary_logsignature(*_gpu(states, actions), depth=depth, dtype=F64)
    words = _words(1 + sd + ad, depth)
    _check_rows(got, n, len(words), F64)
    ref, mag = _extended_refs(_paths(states, actions), depth)
    _check('fp64 %s' % (case,), got.cpu().numpy(), ref, mag, _factor(words, length, depth), F64)


# ------------------------------------------------------------------ 4. known answers, without the helper's series
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_two_point_path_is_its_increment(B, dtype):
    """[(1, 0, 0), (2, 2, 3)]: log exp(D) = D.  Level 1 is D = (1, 2, 3); every longer word is 0 within the
    bound, whose A_w comes from exp(|D|): Sabs_u = prod D_ui / |u|!."""
    states = torch.tensor([[[0.0], [2.0]]], dtype=dtype)
    actions = torch.tensor([[[0.0], [3.0]]], dtype=dtype)
    got = B.summary_logsignature(*_gpu(states, actions), depth=5, dtype=dtype).cpu().numpy()
    words = _words(3, 5)
    incs = np.array([[[1.0, 2.0, 3.0]]], dtype=np.longdouble)
    mag = LC.magnitude(LC.chen(incs, 5), words, 3)
    ref = np.zeros((1, len(words)))
    ref[0, :3] = [1.0, 2.0, 3.0]
    assert got[0, :3].tolist() == [1.0, 2.0, 3.0]
    _check('two points %s' % dtype, got, ref, mag, _factor(words, 2, 5), dtype)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_level_2_is_the_levy_area(B, dtype):
    """Words ij, i < j: 1/2 sum_l (X^i_l - X^i_0) dX^j_l - (X^j_l - X^j_0) dX^i_l, from the path in fp64
    (summed in extended precision: a sum in fp64 would carry an error the size of the fp64 bound)."""
    length, sd, ad, depth = 9, 3, 1, 4
    states, actions = _traj(3, length, sd, ad, dtype)
    got = B.summary_logsignature(*_gpu(states, actions), depth=depth, dtype=dtype).cpu().numpy()
    x = _paths(states, actions).numpy().astype(np.longdouble)          # the fp64 path; the sums in extended
    d = x.shape[2]
    words = _words(d, depth)
    inc = x[:, 1:] - x[:, :-1]
    rel = x[:, :-1] - x[:, :1]                       # X_l - X_0 at the start of segment l
    # (on a segment, X - X_0 = rel + s inc: the s inc parts of the two terms cancel)
    area = {(i, j): (rel[:, :, i] * inc[:, :, j] - rel[:, :, j] * inc[:, :, i]).sum(axis=1) / 2
            for i in range(d) for j in range(i + 1, d)}
    pairs = [w for w in words if len(w) == 2]
    assert pairs == sorted(area) and len(pairs) == d * (d - 1) // 2
    cols = [words.index(w) for w in pairs]
    _, mag = _extended_refs(_paths(states, actions), depth)
    _check('Levy area %s' % dtype, got[:, cols], np.stack([area[w] for w in pairs], axis=1), mag[:, cols],
           _factor(pairs, length, depth), dtype)


# ------------------------------------------------------------------ 5. channel subsets
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_scrambled_picks_are_bitwise_the_rearranged_tensors(B, dtype):
    states, actions = _traj(3, 7, 4, 2, dtype)
    both = torch.cat([states, actions], dim=-1)
    s2, a2 = both[..., [5, 0]].contiguous(), both[..., [2]].contiguous()
    got = B.summary_logsignature(*_gpu(states, actions), depth=4, channels=[5, 0, 2], dtype=dtype)
    words = _words(4, 4)
    _check_rows(got, 3, 90, dtype)
    assert torch.equal(got, B.summary_logsignature(*_gpu(s2, a2), depth=4, dtype=dtype))
    ref, mag = _extended_refs(_paths(states, actions, [5, 0, 2]), 4)
    _check('scrambled picks %s' % dtype, got.cpu().numpy(), ref, mag, _factor(words, 7, 4), dtype)


def test_shadowhand_shaped_subset_at_depth_3(B):
    """21 of 231 channels -- the first and the last of either tensor among them -- give d = 22: 3 795
    coordinates at the default depth 3 where the signature has 11 154."""
    states, actions = _traj(2, 11, 211, 20)
    picked = [0, 210, 211, 230] + list(range(40, 57))
    got = B.summary_logsignature(*_gpu(states, actions), channels=picked)        # default depth: 3
    words = _words(22, 3)
    _check_rows(got, 2, 3795, F32)
    ref, mag = _fp64_refs(_paths(states, actions, picked), 3)
    _check('ShadowHand subset', got.cpu().numpy(), ref, mag, _factor(words, 11, 3), F32)
    again = B.summary_logsignature(*_gpu(states, actions), channels=tuple(picked), depth=3)
    assert torch.equal(again, got)
    assert len([k for k in B.summarizers._word_vectors if k[:2] == (22, 3)]) == 1            # uploaded once


def test_a_repeated_channel(B):
    states, actions = _traj(2, 6, 2, 1)
    got = B.summary_logsignature(*_gpu(states, actions), depth=4, channels=[1, 1])
    words = _words(3, 4)
    _check_rows(got, 2, 32, F32)
    ref, mag = _fp64_refs(_paths(states, actions, [1, 1]), 4)
    _check('repeated channel', got.cpu().numpy(), ref, mag, _factor(words, 6, 4), F32)


# ------------------------------------------------------------------ 6. launch mechanics
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
    got = B.summary_logsignature(*_gpu(states, actions), depth=4, dtype=dtype)
    words = _words(3, 4)
    _check_rows(got, n, 32, dtype)
    ref, mag = _extended_refs(_paths(states, actions), 4)
    _check('grid stride %s' % dtype, got.cpu().numpy(), ref, mag, _factor(words, 2, 4), dtype)


@pytest.mark.parametrize('dtype,start', [(F32, 2), (F64, 2), (F64, 1)], ids=['fp32+2', 'fp64+2', 'fp64+1'])
def test_out_view_with_a_wider_pitch_and_an_unaligned_start(B, dtype, start):
    states, actions = _traj(3, 7, 4, 2, dtype)
    s, a = _gpu(states, actions)
    plain = B.summary_logsignature(s, a, depth=4, channels=[5, 0, 2], dtype=dtype)
    n, width = plain.shape
    pitch = width + 7
    base = torch.full((start + (n + 1) * pitch,), -77.0, dtype=dtype, device=DEV)
    view = base[start:].view(n + 1, pitch)
    assert view.data_ptr() % 16 == (start * base.element_size()) % 16
    res = B.summary_logsignature(s, a, depth=4, channels=[5, 0, 2], out=view, dtype=dtype)
    assert res.data_ptr() == view.data_ptr() and res.stride(0) == pitch and tuple(res.shape) == (n, width)
    assert torch.equal(view[:n, :width], plain)
    assert (view[:n, width:] == -77.0).all() and (view[n] == -77.0).all() and (base[:start] == -77.0).all()


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_two_runs_are_bitwise_equal_and_the_signature_is_left_alone(B, dtype):
    s, a = _gpu(*_traj(2, 20, 3, 1, dtype))
    ident = list(range(4))
    before = [B.summary_signatory(s, a, depth=5, dtype=dtype).clone(),
              B.summary_signatory(s, a, depth=3, dtype=dtype).clone(),                      # the tuned kernel
              B.summary_signatory(s, a, depth=3, channels=ident, dtype=dtype).clone()]
    first = B.summary_logsignature(s, a, depth=5, dtype=dtype).clone()
    assert torch.equal(B.summary_logsignature(s, a, depth=5, dtype=dtype), first)
    B.summary_logsignature(s, a, depth=3, dtype=dtype)
    after = [B.summary_signatory(s, a, depth=5, dtype=dtype), B.summary_signatory(s, a, depth=3, dtype=dtype),
             B.summary_signatory(s, a, depth=3, channels=ident, dtype=dtype)]
    for x, y in zip(before, after):
        assert torch.equal(x, y)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_depth_1_is_the_signatures_level_1(B, dtype):
    s, a = _gpu(*_traj(3, 9, 3, 1, dtype))
    got = B.summary_logsignature(s, a, depth=1, dtype=dtype)
    _check_rows(got, 3, 5, dtype)
    assert torch.equal(got, B.summary_signatory(s, a, depth=1, dtype=dtype))
    picked = B.summary_logsignature(s, a, depth=1, channels=[3, 0], dtype=dtype)
    assert torch.equal(picked, B.summary_signatory(s, a, depth=1, channels=[3, 0], dtype=dtype))


# ------------------------------------------------------------------ 7. BayesSim
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_logsignature', 'trainTrajLen': 21, 'components': 3,
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


def test_bayessim_fits_and_predicts_on_the_log_signature(B):
    theta, states, actions = _pendulum(B)
    bs, twin = _bayes_sim(B, CFG), _bayes_sim(B, CFG)
    assert bs.model.input_dim == 90 and not bs.model._f64
    rows = B.summary_logsignature(states, actions, depth=4, channels=[0, 1, 3])
    assert tuple(rows.shape) == (1000, 90)
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


def test_bayessim_in_double_on_the_log_signature(B):
    theta, states, actions = _pendulum(B)
    cfg = dict(CFG, dtype='float64', summaryDtype='float64')
    bs, twin = _bayes_sim(B, cfg), _bayes_sim(B, cfg)
    assert bs.model.input_dim == 90 and bs.model._f64
    rows = bs._summarize(states, actions)
    assert rows.dtype == F64 and tuple(rows.shape) == (1000, 90)
    assert torch.equal(rows, B.summary_logsignature(states, actions, depth=4, channels=[0, 1, 3], dtype=F64))
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
