"""GPU checks of the kernel mean embedding summary (include/bsig_kme.h, csrc/kme.h) through
``KernelMeanEmbedding``, ``summary_kme`` and BayesSim's ``'summarizerFxn': 'summary_kme'``.

What is compared with: tests/kme_cases.py -- the definition restated in numpy, in double, on seeded CPU
trajectories of fp32-representable values, which both precisions take exactly, and on the coefficients as the
kernel gets them (bsig_kme_coeff's, which are numpy's bit for bit).

The bound is derived, not measured: the docstring of tests/kme_cases.py gives the derivation.  In short, with
u = 2^-24 (fp32) or 2^-53 (fp64), gamma(k) = k u / (1 - k u), E_t,j = gamma(d + 3) sum_k |x_t,k| |coeff_j,k| and
S = 3e-6 (fp32) or 8 u (double) for the sine and cosine themselves:
    |got - ref| <= a [ (1/M) sum_t (E_t,j + S) + gamma(M + 3) (1 + S + max_t E_t,j) ],   a = sqrt(1/m).
Every comparison prints its worst |err| / bound; the worst per case are in profiles/kme_NOTES.md."""
import functools

import numpy as np
import pytest
import torch

import input_norm_cases as NC
import kme_cases as KC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
NP = {F32: np.float32, F64: np.float64}
BOTH = pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
BITS_CASES = ['pendulum', 'm100_time', 'edge_ts65', 'ant', 'five_tiles_two_blocks']


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


def _itemsize(dtype):
    return 8 if dtype == F64 else 4


def _group(B, name, dtype):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    g = B._lib.load().bsig_kme_group(ts, ta, sd, ad, m, diff, time, _itemsize(dtype))
    assert g >= 1
    return g


def _rows(B, name, dtype):
    n = KC.CASES[name][0]
    return 2 * _group(B, name, dtype) + 1 if n is None else n


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """The inputs of a case at ``n`` rows as CPU tensors, and per precision the coefficients (numpy's restatement
    of bsig_kme_coeff), the fp64 reference rows and the bounds: made once, shared, never modified."""
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    states, actions, freqs, inv_std = KC.case_inputs(name, n)
    kap = KC.kappa(1.0, KC.row_dim(sd, ad, diff, time))
    per = {}
    for dt in (F32, F64):
        coeff = KC.coefficients(freqs, inv_std, kap, NP[dt])
        per[dt] = (coeff, KC.reference(states, actions, coeff, diff, time),
                   KC.bounds(states, actions, coeff, diff, time, _itemsize(dt)))
    return torch.from_numpy(states), torch.from_numpy(actions), freqs, inv_std, per


def _embedding(B, name, n):
    """The module of a case: the case's frequencies, its scale given from the host."""
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    _, _, freqs, inv_std, _ = _case(name, n)
    emb = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, diff=bool(diff), time=bool(time), freqs=freqs, device=DEV)
    return emb.set_scale(inv_std, count=n)


def _check_rows(got, n, width, dtype, device='cuda'):
    assert got.dtype == dtype and got.device.type == device and tuple(got.shape) == (n, width)
    assert got.stride(1) == 1
    if device == 'cuda':
        assert got.data_ptr() % 16 == 0 and got.stride(0) % (16 // got.element_size()) == 0


def _check(what, got, ref, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    print('%s: worst |err| / bound = %.3g (bounds %.3g .. %.3g, largest |value| %.3g)'
          % (what, ratio.max(), bound.min(), bound.max(), np.abs(ref).max()))
    assert ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))


# ------------------------------------------------------------------ 1. against the definition
def _case_ids():
    return [(name, dt) for name in sorted(KC.CASES) for dt in (F32, F64) if dt == F32 or name in KC.IN_DOUBLE]


@pytest.mark.parametrize('name,dtype', _case_ids(), ids=['%s-%s' % (n, 'fp64' if d == F64 else 'fp32')
                                                         for n, d in _case_ids()])
def test_rows_are_the_definition_within_the_derived_bound(B, name, dtype):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    n_all = _rows(B, name, dtype)
    states, actions, freqs, inv_std, per = _case(name, n_all)
    coeff, ref, bound = per[dtype]
    assert ref.shape == (n_all, 2 * m) and (bound > 0).all()
    emb = _embedding(B, name, n_all)
    # the coefficients the kernel reads are the restatement's, bit for bit; the padding columns are zero
    dev_coeff = emb.coefficients(dtype)
    assert dev_coeff.dtype == dtype and np.array_equal(dev_coeff.cpu().numpy(), coeff)
    s, a = states.to(DEV), actions.to(DEV)
    counts = KC.group_counts(_group(B, name, dtype)) if KC.CASES[name][0] is None else [n_all]
    assert counts[-1] == n_all
    for n in counts:
        got = B.summary_kme(s[:n], a[:n], emb, dtype=dtype)
        _check_rows(got, n, 2 * m, dtype)
        _check('%s %s n=%d' % (name, dtype, n), got, ref[:n], bound[:n])
    if name in KC.CONSTANT_ACTION:
        assert inv_std[sd] == 0 and (dev_coeff[:, sd] == 0).all()


def test_the_long_shadowhand_trajectory_is_beyond_a_workgroups_lds_and_runs(B):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES['shadowhand_long']
    assert KC.steps(ts, diff) * KC.row_dim(sd, ad, diff, time) * 4 > 160 * 1024
    assert B._lib.load().bsig_kme_fits(ts, ta, sd, ad, m, diff, time, 8) == B._lib.BSIG_OK


# the workgroup caps of the summarizers (csrc/common.h kSummaryGridCap): beyond cap * G trajectories a workgroup
# strides on to further ones
def test_workgroups_stride_over_more_trajectories_than_the_grid_holds(B):
    """2 cap G + 5 one-block trajectories of two states: every workgroup takes a second batch, some a third, and
    the last batch is partly empty."""
    sd, ad, ts, m = 3, 1, 2, 2
    g = B._lib.load().bsig_kme_group(ts, ts, sd, ad, m, 1, 0, 4)
    assert g == 8
    n = 2 * 256 * 64 * g + 5
    states, actions = KC.trajectories(n, ts, ts, sd, ad)
    freqs = np.random.RandomState(2).standard_normal((m, 7)).astype(np.float32)
    inv_std = KC.flat_rule_inv_std(KC.rows(states[:256], actions[:256], 1, 0).reshape(-1, 7))
    coeff = KC.coefficients(freqs, inv_std, KC.kappa(1.0, 7), np.float32)
    emb = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, freqs=freqs, device=DEV).set_scale(inv_std)
    got = emb(torch.from_numpy(states).to(DEV), torch.from_numpy(actions).to(DEV))
    _check_rows(got, n, 2 * m, F32)
    _check('strided', got, KC.reference(states, actions, coeff, 1, 0), KC.bounds(states, actions, coeff, 1, 0, 4))


# ------------------------------------------------------------------ 2. out=, n == 0, CPU inputs
@BOTH
@pytest.mark.parametrize('name,extra', [('pendulum', 4), ('pendulum', 3), ('m100_time', 5), ('edge_ts65', 2)])
def test_out_with_a_wider_pitch_keeps_the_bytes_beyond_the_width(B, name, extra, dtype):
    m = KC.CASES[name][5]
    n = _rows(B, name, dtype)
    states, actions, _, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    emb = _embedding(B, name, n)
    plain = emb(s, a, dtype=dtype)
    sentinel = -123.25
    out = torch.full((n + 1, 2 * m + extra), sentinel, dtype=dtype, device=DEV)
    got = emb(s, a, dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, 2 * m) and got.stride(0) == 2 * m + extra
    assert torch.equal(got, plain)
    assert (out[:n, 2 * m:] == sentinel).all() and (out[n] == sentinel).all()


@BOTH
def test_an_empty_batch_touches_nothing(B, dtype):
    states, actions, _, _, _ = _case('pendulum', _rows(B, 'pendulum', dtype))
    emb = _embedding(B, 'pendulum', _rows(B, 'pendulum', dtype))
    out = torch.full((2, 256), -5.0, dtype=dtype, device=DEV)
    got = emb(states[:0].to(DEV), actions[:0].to(DEV), dtype=dtype, out=out)
    assert tuple(got.shape) == (0, 256) and (out == -5.0).all()
    assert tuple(emb(states[:0].to(DEV), actions[:0].to(DEV), dtype=dtype).shape) == (0, 256)


def test_cpu_inputs_come_back_on_the_cpu(B):
    states, actions, _, _, per = _case('ta_t_minus_1', 21)
    emb = _embedding(B, 'ta_t_minus_1', 21)
    got = B.summary_kme(states, actions, emb)
    _check_rows(got, 21, 32, F32, device='cpu')
    assert torch.equal(got, emb(states.to(DEV), actions.to(DEV)).cpu())
    _check('cpu inputs', got, per[F32][1], per[F32][2])


# ------------------------------------------------------------------ 3. bits
@BOTH
@pytest.mark.parametrize('name', BITS_CASES)
def test_two_runs_are_bitwise_equal_and_rows_do_not_depend_on_their_neighbours(B, name, dtype):
    n = _rows(B, name, dtype)
    states, actions, _, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    emb = _embedding(B, name, n)
    first = emb(s, a, dtype=dtype).clone()
    assert torch.equal(emb(s, a, dtype=dtype), first)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n)).to(DEV)
    assert torch.equal(emb(s[perm], a[perm], dtype=dtype), first[perm])
    # every row alone (another slot of another workgroup, another N) has the bits it has in the batch
    for i in range(n):
        assert torch.equal(emb(s[i:i + 1], a[i:i + 1], dtype=dtype), first[i:i + 1]), i


# ------------------------------------------------------------------ 4. non-finite values
@BOTH
@pytest.mark.parametrize('name', ['pendulum', 'edge_ts65'])
def test_a_nan_raises_the_flag_and_touches_only_its_own_row(B, name, dtype):
    n = _rows(B, name, dtype)
    states, actions, _, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    emb = _embedding(B, name, n)
    clean = emb(s, a, dtype=dtype).clone()
    hit = n // 2
    s_bad = s.clone()
    s_bad[hit, 3, 1] = float('nan')
    with pytest.raises(AssertionError):
        emb(s_bad, a, dtype=dtype)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = emb(s_bad, a, dtype=dtype, check_finite=flag)
    assert int(flag.item()) == 1
    others = [r for r in range(n) if r != hit]
    assert torch.equal(got[others], clean[others]) and torch.isnan(got[hit]).all()
    flag.zero_()
    emb(s, a, dtype=dtype, check_finite=flag)
    assert int(flag.item()) == 0
    a_bad = a.clone()
    a_bad[hit, 0, 0] = float('inf')
    emb(s, a_bad, dtype=dtype, check_finite=flag)
    assert int(flag.item()) == 1
    quiet = emb(s_bad, a, dtype=dtype, check_finite=False)
    assert torch.equal(quiet[others], clean[others])


# ------------------------------------------------------------------ 5. the rows, the coefficients, the scale
@BOTH
@pytest.mark.parametrize('name', ['pendulum', 'm100_time', 'ta_1', 'ta_above_t', 'm1_raw_time', 'ant'])
def test_the_rows_are_numpys_bit_for_bit(B, name, dtype):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    n = _rows(B, name, dtype)
    states, actions, _, _, _ = _case(name, n)
    emb = _embedding(B, name, n)
    got = emb.rows(states.to(DEV), actions.to(DEV), dtype=dtype)
    d = KC.row_dim(sd, ad, diff, time)
    assert got.dtype == dtype and tuple(got.shape) == (n * KC.steps(ts, diff), d)
    want = KC.rows(states.numpy(), actions.numpy(), diff, time, dtype=NP[dtype])
    if dtype == F64 and time:
        # the header's tau: t times the rounded reciprocal, two roundings -- not the definition's quotient
        steps = KC.steps(ts, diff)
        want = want.copy()
        want[:, :, 0] = np.arange(steps, dtype=np.float64) * (1.0 / max(steps - 1, 1))
    assert np.array_equal(got.cpu().numpy(), want.reshape(-1, d))


@BOTH
def test_the_coefficients_are_the_restatement_bit_for_bit_and_zero_behind_the_width(B, dtype):
    lib, _lib = B._lib.load(), B._lib
    m, d, ld_f, ld_c = 37, 7, 9, 12
    rng = np.random.RandomState(8)
    freqs = rng.standard_normal((m, d)).astype(np.float32)
    inv_std = np.abs(rng.standard_normal(d)) * np.array([1e-3, 1.0, 0.0, 7.0, 1e3, 1.0 / 3.0, 1.0])
    kap = KC.kappa(0.7, d)
    f = torch.full((m, ld_f), float('nan'), dtype=F32, device=DEV)
    f[:, :d] = torch.from_numpy(freqs).to(DEV)
    out = torch.full((m + 1, ld_c), -9.0, dtype=dtype, device=DEV)
    prec = _lib.F64 if dtype == F64 else _lib.F32
    prec.kme_coeff(_lib.ptr(f), ld_f, _lib.ptr(torch.from_numpy(inv_std).to(DEV)), kap, _lib.ptr(out), ld_c, m, d,
                   _lib.stream())
    got = out.cpu().numpy()
    assert np.array_equal(got[:m, :d], KC.coefficients(freqs, inv_std, kap, NP[dtype]))
    assert (got[:m, d:] == 0).all() and (got[m] == -9.0).all() and (got[:m, 2] == 0).all()


@BOTH
@pytest.mark.parametrize('name', ['pendulum', 'constant_action', 'ant'])
def test_fit_scale_is_the_input_statistics_of_the_rows(B, name, dtype):
    _lib = B._lib
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    n = _rows(B, name, dtype)
    states, actions, freqs, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    emb = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, diff=bool(diff), time=bool(time), freqs=freqs, device=DEV)
    assert not emb.ready
    emb.fit_scale(s, a, dtype=dtype)
    assert emb.ready and int(emb.count) == n
    d = emb.row_dim
    x = emb.rows(s, a, dtype=dtype)
    mean = torch.empty(d, dtype=F64, device=DEV)
    inv = torch.empty(d, dtype=F64, device=DEV)
    need = int(_lib.load().bsig_input_norm_workspace_bytes(x.shape[0], d))
    ws = torch.empty(need // 8, dtype=F64, device=DEV)
    prec = _lib.F64 if dtype == F64 else _lib.F32
    prec.input_norm_stats(_lib.ptr(x), x.stride(0), x.shape[0], d, _lib.ptr(mean), _lib.ptr(inv), _lib.ptr(ws),
                          need, _lib.stream())
    assert torch.equal(emb.inv_std, inv)
    # and within the statistics kernels' bound against the long-double definition (tests/test_gpu_input_norm.py)
    xs = x.cpu().numpy()
    ref_mean, ref_std, ref_flat = NC.reference_stats(xs)
    got = emb.inv_std.cpu().numpy()
    assert np.array_equal(got == 0.0, ref_flat) and np.isfinite(got).all()
    kept = ~ref_flat
    err = np.abs(1.0 / got[kept].astype(np.longdouble) - ref_std[kept])
    assert (err <= 8 * xs.shape[0] * NC.U53 * (ref_std + np.abs(ref_mean))[kept]).all()
    if name in KC.CONSTANT_ACTION:
        assert got[sd] == 0 and kept.sum() == d - 1
        out = emb(s, a, dtype=dtype)
        assert torch.isfinite(out).all() and (emb.coefficients(dtype)[:, sd] == 0).all()
    # the first 256 trajectories at most
    if name == 'pendulum':
        big_s, big_a = KC.trajectories(300, ts, ta, sd, ad)
        big_s, big_a = torch.from_numpy(big_s).to(DEV), torch.from_numpy(big_a).to(DEV)
        capped = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, device=DEV).fit_scale(big_s, big_a, dtype=dtype)
        first = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, device=DEV).fit_scale(big_s[:256], big_a[:256], dtype=dtype)
        assert int(capped.count) == 256 and torch.equal(capped.inv_std, first.inv_std)


def test_a_new_scale_makes_new_coefficients(B):
    n = _rows(B, 'pendulum', F32)
    states, actions, _, inv_std, _ = _case('pendulum', n)
    s, a = states.to(DEV), actions.to(DEV)
    emb = _embedding(B, 'pendulum', n)
    first = emb(s, a).clone()
    emb.set_scale(inv_std * 2.0)
    assert not torch.equal(emb(s, a), first)
    emb.set_scale(inv_std)
    assert torch.equal(emb(s, a), first)
    twin = B.KernelMeanEmbedding(3, 1, n_feat=256, seed=5, device=DEV)
    twin.load_state_dict(emb.state_dict())
    assert twin.ready and torch.equal(twin(s, a), first)


# ------------------------------------------------------------------ 6. BayesSim (the plumbing; no accuracy claim)
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_kme', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (32, 32), 'lr': 1e-3, 'kmeFeatures': 64}


def _bayes_sim(B, cfg):
    torch.manual_seed(11)          # the start weights
    return B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01, 0.01]),
                      params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)


@functools.lru_cache(maxsize=None)
def _pendulum(B):
    theta, states, actions = B.pairs.pendulum_pairs(2000, 20, policy='random', seed=4, device=DEV)
    assert states.shape[1] == 21
    return theta, states, actions


@pytest.mark.parametrize('extra', [{}, {'dtype': 'float64', 'summaryDtype': 'float64'}], ids=['fp32', 'fp64'])
def test_bayessim_fits_and_predicts_on_the_embedding(B, extra, monkeypatch):
    theta, states, actions = _pendulum(B)
    cfg = dict(CFG, **extra)
    double = 'dtype' in extra
    dtype = F64 if double else F32
    other = {k: v for k, v in cfg.items() if k != 'kmeFeatures'}
    plain_keys = list(_bayes_sim(B, dict(other, summarizerFxn='summary_start')).model.state_dict())
    runs = []
    for no_block in ('0', '1'):
        monkeypatch.setenv('BSIG_NO_FIT_PREPROJECT', no_block)
        bs = _bayes_sim(B, cfg)
        assert bs.model.input_dim == 64 and bs.model._f64 == double and not bs.embedding.ready
        np.random.seed(31), torch.manual_seed(32)
        logs = bs.fit(theta, states, actions)
        assert len(logs) == 2
        for chunk in logs:
            for key in ('train_loss', 'test_loss'):
                assert len(chunk[key]) > 0 and np.isfinite(chunk[key]).all()
        emb = bs.embedding
        assert emb.ready and int(emb.count) == 256
        runs.append((bs, logs, bs._summarize(states, actions).clone()))
    monkeypatch.delenv('BSIG_NO_FIT_PREPROJECT')
    (bs, logs, summ), (bs_chunks, logs_chunks, summ_chunks) = runs
    # the block path and the chunk path: equal scale bits, equal summary bits
    assert torch.equal(bs.embedding.inv_std, bs_chunks.embedding.inv_std)
    assert summ.dtype == dtype and tuple(summ.shape) == (2000, 64) and torch.equal(summ, summ_chunks)
    # the scale is that of the first 256 trajectories, and the summary the module's
    alone = B.KernelMeanEmbedding(3, 1, n_feat=64, device=DEV).fit_scale(states[:256], actions[:256], dtype=dtype)
    assert torch.equal(alone.inv_std, bs.embedding.inv_std) and torch.equal(alone.freqs, bs.embedding.freqs)
    assert torch.equal(alone(states, actions, dtype=dtype), summ)
    mog = bs.predict(states[:1], actions[:1])
    assert isinstance(mog, B.pdf.MoG)
    assert np.isfinite(mog.a).all() and abs(float(np.sum(mog.a)) - 1.0) <= 1e-6
    # a state_dict round trip of the embedding
    fresh = _bayes_sim(B, dict(cfg, kmeSeed=7))
    assert not fresh.embedding.ready and not torch.equal(fresh.embedding.freqs, bs.embedding.freqs)
    fresh.embedding.load_state_dict(bs.embedding.state_dict())
    assert fresh.embedding.ready and torch.equal(fresh._summarize(states, actions), summ)
    # the model's state_dict has the keys it has with any other summarizer
    assert list(bs.model.state_dict()) == plain_keys
    # a scale that exists is kept: a second fit makes no new one
    before = bs.embedding.inv_std.clone()
    bs.fit(theta[:1000], states[1000:], actions[1000:])
    assert torch.equal(bs.embedding.inv_std, before) and int(bs.embedding.count) == 256


def test_run_training_makes_the_scale_and_fit_embedding_scale_is_the_explicit_form(B):
    theta, states, actions = _pendulum(B)
    bs = _bayes_sim(B, CFG)
    np.random.seed(21), torch.manual_seed(22)
    logs = bs.run_training(theta[:1000], states[:1000], actions[:1000])
    assert np.isfinite(logs['train_loss']).all() and bs.embedding.ready and int(bs.embedding.count) == 256
    explicit = _bayes_sim(B, CFG).fit_embedding_scale(states[:256], actions[:256])
    assert torch.equal(explicit.embedding.inv_std, bs.embedding.inv_std)
    bad = states[:256].clone()
    bad[3, 2, 0] = float('nan')
    with pytest.raises(AssertionError, match='non-finite'):
        _bayes_sim(B, CFG).fit_embedding_scale(bad, actions[:256])
