"""GPU checks of the least-squares dynamics kernel (include/bsig_sysid.h, csrc/sysid.h) through
``summary_sysid(..., ridge=)`` and BayesSim's ``'summarizerFxn': 'summary_sysid'``.

What is compared with: tests/sysid_cases.py -- the definition restated in numpy, in double (refined in long
double), on seeded CPU trajectories of fp32-representable values, which both precisions take exactly.

The bounds are derived, not measured: the docstring of tests/sysid_cases.py gives the derivation from the
backward-error results for inner products and Cholesky solves (Higham, ch. 3 and 10), for the system the kernel
solves at each shape (primal for p <= M, dual otherwise).  They are per output column and normwise: on
||W^_:j - W_:j||_2 and on |r^_j - r_j|.  Every comparison prints its worst error / bound; the worst per test are
in profiles/sysid_NOTES.md."""
import functools

import numpy as np
import pytest
import torch

import sysid_cases as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
U = {F32: SC.U32, F64: SC.U64}
BOTH = pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


def _group(B, name, dtype):
    _, ts, ta, sd, ad, _, _ = SC.CASES[name]
    g = B._lib.load().bsig_sysid_group(ts, ta, sd, ad, 8 if dtype == F64 else 4)
    assert g >= 1
    return g


def _rows(B, name, dtype):
    n = SC.CASES[name][0]
    return 3 * _group(B, name, dtype) + 2 if n is None else n


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """(states, actions) as CPU float32 tensors, the fp64 reference rows and the fp32 / fp64 bounds of a case at
    ``n`` rows: made once, shared by every test that names the case, never modified."""
    _, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    states, actions = SC.trajectories(n, ts, ta, sd, ad)
    ref = SC.reference(states, actions, ridge)
    bound = {dt: SC.bounds(states, actions, ridge, U[dt]) for dt in (F32, F64)}
    return torch.from_numpy(states), torch.from_numpy(actions), ref, bound


def _check_rows(got, n, width, dtype):
    assert got.dtype == dtype and got.device.type == 'cuda' and tuple(got.shape) == (n, width)
    assert got.stride(1) == 1 and got.data_ptr() % 16 == 0 and got.stride(0) % (16 // got.element_size()) == 0


def _check(what, got, ref, bound, sd, ad):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    q_w, q_r = SC.ratios(got, ref, bound[0], bound[1], sd, ad)
    print('%s: worst error / bound: W %.3g, r %.3g' % (what, q_w, q_r))
    assert q_w <= 1.0 and q_r <= 1.0, (what, q_w, q_r)


def _covered(names):
    """parametrize over (name, dtype): fp32, and double where the case is covered there."""
    pairs = [(name, dt) for name in names for dt in (F32, F64) if dt == F32 or SC.CASES[name][6]]
    return pytest.mark.parametrize('name,dtype', pairs,
                                   ids=['%s-%s' % (name, 'fp64' if dt == F64 else 'fp32') for name, dt in pairs])


# ------------------------------------------------------------------ 1. against the definition
@_covered(sorted(SC.CASES))
def test_rows_are_the_definition_within_the_derived_bounds(B, name, dtype):
    _, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    n_all = _rows(B, name, dtype)
    states, actions, ref, bound = _case(name, n_all)
    width = SC.width(sd, ad)
    assert ref.shape == (n_all, width) == (n_all, B.sysid_dim(sd, ad))
    s, a = states.to(DEV), actions.to(DEV)
    counts = SC.group_counts(_group(B, name, dtype)) if SC.CASES[name][0] is None else [n_all]
    assert counts[-1] == n_all
    for n in counts:
        got = B.summary_sysid(s[:n], a[:n], ridge=ridge, dtype=dtype)
        _check_rows(got, n, width, dtype)
        _check('%s %s n=%d' % (name, dtype, n), got, ref[:n], [b[:n] for b in bound[dtype]], sd, ad)


@pytest.mark.parametrize('name', sorted(SC.ILL))
def test_an_ill_conditioned_fit_in_double(B, name):
    n, ts, ta, sd, ad, ridge = SC.ILL[name]
    states, actions = SC.trajectories(n, ts, ta, sd, ad)
    got = B.summary_sysid(torch.from_numpy(states).to(DEV), torch.from_numpy(actions).to(DEV), ridge=ridge,
                          dtype=F64)
    _check('%s fp64' % name, got, SC.reference(states, actions, ridge), SC.bounds(states, actions, ridge, SC.U64),
           sd, ad)


def test_default_arguments_are_ridge_1e_3_and_a_double_input_is_narrowed(B):
    states, actions, ref, bound = _case('pendulum', _rows(B, 'pendulum', F32))
    got = B.summary_sysid(states.to(DEV), actions.to(DEV))
    _check_rows(got, states.shape[0], 18, F32)
    _check('defaults', got, ref, bound[F32], 3, 1)
    assert torch.equal(got, B.summary_sysid(states.to(DEV).double(), actions.to(DEV).double()))
    cpu = B.summary_sysid(states, actions)
    assert cpu.device.type == 'cpu' and torch.equal(cpu, got.cpu())


# the workgroup caps of the summarizers (csrc/common.h kSummaryGridCap, include/bsig_f64.h
# BSIG_F64_SUMMARY_GRID_CAP): beyond cap * G trajectories a workgroup strides on to further ones
GRID_CAP = {F32: 256 * 64, F64: 4096}


@BOTH
def test_workgroups_stride_over_more_trajectories_than_the_grid_holds(B, dtype):
    """cap G + 5 Pendulum trajectories: some workgroups take a second batch, the last one partly empty.  The
    rows are those of the same trajectories in a batch the grid holds."""
    g = _group(B, 'pendulum', dtype)
    assert g == 16
    few = 3 * g + 2
    states, actions, ref, bound = _case('pendulum', few)
    n = GRID_CAP[dtype] * g + 5
    reps = -(-n // few)
    s, a = states.to(DEV).repeat(reps, 1, 1)[:n], actions.to(DEV).repeat(reps, 1, 1)[:n]
    got = B.summary_sysid(s, a, dtype=dtype)
    _check_rows(got, n, 18, dtype)
    small = B.summary_sysid(states.to(DEV), actions.to(DEV), dtype=dtype)
    _check('strided %s' % dtype, small, ref, bound[dtype], 3, 1)
    assert torch.equal(got, small.repeat(reps, 1)[:n])


# ------------------------------------------------------------------ 2. exact zeros, bits
@BOTH
@pytest.mark.parametrize('sd,ad,ts', [(3, 1, 21), (3, 1, 4), (60, 8, 50), (60, 8, 100)])
def test_a_constant_trajectory_gives_exact_positive_zeros(B, sd, ad, ts, dtype):
    states = torch.full((3, ts, sd), 1.5, device=DEV) * torch.arange(1, sd + 1, device=DEV)
    actions = torch.full((3, ts, ad), -0.75, device=DEV)
    got = B.summary_sysid(states, actions, ridge=1e-1, dtype=dtype)
    assert (got == 0).all() and not torch.signbit(got).any()


@_covered(['pendulum', 'boundary_m4', 'tile_17', 'ant_t50', 'ant_t100', 'shadowhand'])
def test_two_runs_are_bitwise_equal_and_rows_do_not_depend_on_their_neighbours(B, name, dtype):
    _, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    n = _rows(B, name, dtype)
    states, actions, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    first = B.summary_sysid(s, a, ridge=ridge, dtype=dtype).clone()
    assert torch.equal(B.summary_sysid(s, a, ridge=ridge, dtype=dtype), first)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n)).to(DEV)
    assert not torch.equal(perm, torch.arange(n, device=DEV))
    assert torch.equal(B.summary_sysid(s[perm], a[perm], ridge=ridge, dtype=dtype), first[perm])
    # a row alone (another slot of another workgroup) has the bits it has in the batch
    mid = n // 2
    assert torch.equal(B.summary_sysid(s[mid:mid + 1], a[mid:mid + 1], ridge=ridge, dtype=dtype),
                       first[mid:mid + 1])


# ------------------------------------------------------------------ 3. out=
@BOTH
@pytest.mark.parametrize('name,extra', [('pendulum', 5), ('odd', 3), ('ant_t50', 4), ('ant_t100', 1)])
def test_out_with_a_wider_pitch_and_an_unaligned_start_keeps_everything_outside_the_view(B, name, extra, dtype):
    _, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    n = _rows(B, name, dtype)
    states, actions, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    width = SC.width(sd, ad)
    plain = B.summary_sysid(s, a, ridge=ridge, dtype=dtype)
    sentinel = -123.25
    pitch = width + extra + 1
    pitch += pitch % 2                                # even: row 1, column 1 starts an odd count of elements in
    whole = torch.full((n + 2, pitch), sentinel, dtype=dtype, device=DEV)
    out = whole[1:, 1:]
    assert out.data_ptr() % 16 != 0
    got = B.summary_sysid(s, a, ridge=ridge, dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, width)
    assert got.stride(0) == pitch
    assert torch.equal(got, plain)
    assert (whole[0] == sentinel).all() and (whole[:, 0] == sentinel).all()
    assert (whole[1:n + 1, 1 + width:] == sentinel).all() and (whole[n + 1] == sentinel).all()


# ------------------------------------------------------------------ 4. non-finite values
@BOTH
@pytest.mark.parametrize('name', ['pendulum', 'ant_t50', 'ant_t100'])
def test_a_nan_makes_its_row_nan_raises_the_flag_and_leaves_the_other_rows_alone(B, name, dtype):
    _, ts, ta, sd, ad, ridge, _ = SC.CASES[name]
    n = _rows(B, name, dtype)
    states, actions, _, _ = _case(name, n)
    s, a = states.to(DEV), actions.to(DEV)
    clean = B.summary_sysid(s, a, ridge=ridge, dtype=dtype).clone()
    hit = n // 2
    others = [r for r in range(n) if r != hit]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for where, value in (('state', float('nan')), ('last state', float('inf')), ('action', float('-inf'))):
        s_bad, a_bad = s.clone(), a.clone()
        if where == 'state':
            s_bad[hit, 3, 1] = value
        elif where == 'last state':
            s_bad[hit, ts - 1, 0] = value
        else:
            a_bad[hit, 0, 0] = value
        flag.zero_()
        got = B.summary_sysid(s_bad, a_bad, ridge=ridge, dtype=dtype, check_finite=flag)
        assert int(flag.item()) == 1, where
        assert torch.isnan(got[hit]).all(), where
        assert torch.equal(got[others], clean[others]), where
    with pytest.raises(AssertionError):
        B.summary_sysid(s_bad, a_bad, ridge=ridge, dtype=dtype)
    quiet = B.summary_sysid(s_bad, a_bad, ridge=ridge, dtype=dtype, check_finite=False)
    assert torch.equal(quiet[others], clean[others]) and torch.isnan(quiet[hit]).all()
    # an action the definition ignores (step M of ts actions) changes nothing
    a_ign = a.clone()
    a_ign[hit, ts - 1, 0] = float('nan')
    flag.zero_()
    assert torch.equal(B.summary_sysid(s, a_ign, ridge=ridge, dtype=dtype, check_finite=flag), clean)
    assert int(flag.item()) == 0


@BOTH
def test_a_large_finite_trajectory_leaves_the_flag_clear(B, dtype):
    states, actions, _, _ = _case('pendulum', _rows(B, 'pendulum', dtype))
    s, a = states.to(DEV) * 1e6, actions.to(DEV) * 1e4
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = B.summary_sysid(s, a, dtype=dtype, check_finite=flag)
    assert int(flag.item()) == 0 and torch.isfinite(got).all()


def test_a_refused_shape_is_unsupported_with_the_message_of_fits(B):
    lib = B._lib.load()
    states, actions = torch.zeros(2, 50, 211, device=DEV), torch.zeros(2, 50, 20, device=DEV)
    assert tuple(B.summary_sysid(states, actions, ridge=1e-1).shape) == (2, 49163)         # fp32: covered
    assert lib.bsig_sysid_fits(50, 50, 211, 20, 8) == B._lib.BSIG_EUNSUPPORTED
    message = lib.bsig_last_error().decode()
    assert 'LDS' in message
    with pytest.raises(NotImplementedError) as caught:
        B.summary_sysid(states, actions, ridge=1e-1, dtype=F64)
    assert str(caught.value) == message
    out = torch.zeros(2, 49164, dtype=F64, device=DEV)
    s64, a64 = states.double(), actions.double()
    rc = lib.bsig_sysid_f64(B._lib.ptr(s64), B._lib.ptr(a64), B._lib.ptr(out), 2, 50, 50, 211, 20, 1e-1, 49164,
                            None, B._lib.stream())
    assert rc == B._lib.BSIG_EUNSUPPORTED and lib.bsig_last_error().decode() == message
    assert (out == 0).all()


# ------------------------------------------------------------------ 5. BayesSim (the plumbing; no accuracy claim)
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_sysid', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (32, 32), 'lr': 1e-3}


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
def test_bayessim_fits_and_predicts_on_the_summary(B, extra, monkeypatch):
    theta, states, actions = _pendulum(B)
    cfg = dict(CFG, **extra)
    double = 'dtype' in extra
    dtype = F64 if double else F32
    plain_keys = list(_bayes_sim(B, dict(cfg, summarizerFxn='summary_start')).model.state_dict())
    rows = B.summary_sysid(states, actions, dtype=dtype)
    assert tuple(rows.shape) == (2000, 18) and rows.dtype == dtype
    runs = []
    for no_block in ('0', '1'):
        monkeypatch.setenv('BSIG_NO_FIT_PREPROJECT', no_block)
        bs = _bayes_sim(B, cfg)
        assert bs.model.input_dim == 18 and bs.model._f64 == double and bs.embedding is None
        seen, summarizer = [], bs.summarizer_fxn

        def recorder(*args, **kw):
            seen.append((kw, summarizer(*args, **kw)))
            return seen[-1][1]
        bs.summarizer_fxn = recorder
        np.random.seed(31), torch.manual_seed(32)
        logs = bs.fit(theta, states, actions)
        bs.summarizer_fxn = summarizer
        assert len(logs) == 2
        for chunk in logs:
            for key in ('train_loss', 'test_loss'):
                assert len(chunk[key]) > 0 and np.isfinite(chunk[key]).all()
        assert all(kw['ridge'] == 1e-3 and torch.is_tensor(kw['check_finite']) for kw, _ in seen)
        runs.append((bs, torch.cat([summary for _, summary in seen])))
    monkeypatch.delenv('BSIG_NO_FIT_PREPROJECT')
    # the block path and the chunk path see the same summaries, those of one call, bit for bit
    assert torch.equal(runs[0][1], rows) and torch.equal(runs[1][1], rows)
    bs = runs[0][0]
    assert torch.equal(bs._summarize(states, actions), rows)
    assert list(bs.model.state_dict()) == plain_keys
    mog = bs.predict(states[:1], actions[:1])
    assert isinstance(mog, B.pdf.MoG)
    assert np.isfinite(mog.a).all() and abs(float(np.sum(mog.a)) - 1.0) <= 1e-6
    assert np.isfinite(mog.eval(theta[:1].cpu().numpy().astype(np.float64))).all()


def test_a_nan_trajectory_fails_the_fits_deferred_assert(B):
    theta, states, actions = _pendulum(B)
    bad = states.clone()
    bad[1500, 7, 2] = float('nan')
    bs = _bayes_sim(B, CFG)
    np.random.seed(31), torch.manual_seed(32)
    with pytest.raises(AssertionError):
        bs.fit(theta, bad, actions)
