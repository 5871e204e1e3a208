"""GPU checks of the per-trajectory lengths of ``summary_xcorr`` and ``summary_kme`` (include/bsig_ragged.h) through
the summarizers' ``lengths=``, ``KernelMeanEmbedding`` and BayesSim's ``traj_lengths`` / ``lengths``.

What is compared with: tests/ragged_cases.py -- per trajectory the fixed-length definitions of tests/xcorr_cases.py
and tests/kme_cases.py on ``states[i:i + 1, :L_i]``, in double, with THEIR derived bounds evaluated at the
trajectory's own length (no new number); and, bit for bit, the fixed-length entry points on the same slices, which
the parents' tests hold against the same definitions.  Every comparison with a bound prints its worst |err| / bound.
"""
import functools

import numpy as np
import pytest
import torch

import input_norm_cases as NC
import kme_cases as KC
import ragged_cases as RC
import xcorr_cases as XC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
NP = {F32: np.float32, F64: np.float64}
U = {F32: XC.U32, F64: XC.U64}
NAN = float('nan')


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


def _itemsize(dtype):
    return 8 if dtype == F64 else 4


def _bits(t):
    """The bit patterns: equal only for equal bits (the sign of a zero and a NaN's payload included)."""
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _ids():
    out = [('xcorr', name, dt) for name in RC.XCORR for dt in (F32, F64)
           if dt == F64 or name not in RC.XCORR_IN_DOUBLE_ONLY]
    out += [('kme', name, dt) for name in RC.KME for dt in (F32, F64) if dt == F32 or name in KC.IN_DOUBLE]
    return out


EVERY_CASE = pytest.mark.parametrize('kind,name,dtype', _ids(), ids=['%s-%s-%s' % (k, n, 'fp64' if d == F64 else 'fp32')
                                                                     for k, n, d in _ids()])


def _group(B, kind, name, dtype):
    lib = B._lib.load()
    if kind == 'xcorr':
        _, ts, ta, sd, ad, k, diff = XC.CASES[name]
        return lib.bsig_xcorr_group(ts, ta, sd, ad, k, int(diff), _itemsize(dtype))
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    return lib.bsig_kme_group(ts, ta, sd, ad, m, diff, time, _itemsize(dtype))


def _counts(B, kind, name, dtype):
    """The row counts a case runs at: its n, or the parent's counts around G."""
    n = (RC.XCORR if kind == 'xcorr' else RC.KME)[name]
    if n is not None:
        return [n]
    g = _group(B, kind, name, dtype)
    assert g > 1
    return (XC if kind == 'xcorr' else KC).group_counts(g)


@functools.lru_cache(maxsize=None)
def _inputs(kind, name, n):
    """(states, actions, lengths) of a case at ``n`` rows as CPU tensors, and for kme the frequencies and the
    scale: made once, shared, never modified."""
    if kind == 'xcorr':
        _, ts, ta, sd, ad, _, _ = XC.CASES[name]
        states, actions = XC.trajectories(n, ts, ta, sd, ad)
        extra = ()
    else:
        states, actions, freqs, inv_std = KC.case_inputs(name, n)
        extra = (freqs, inv_std)
    lengths = RC.lengths_for(name, n, kind)
    return (torch.from_numpy(states), torch.from_numpy(actions), torch.from_numpy(lengths)) + extra


@functools.lru_cache(maxsize=None)
def _reference(kind, name, n, dtype):
    """The fp64 reference rows and the bounds of a case in ``dtype``, per trajectory at its own length."""
    states, actions, lengths = (t.numpy() for t in _inputs(kind, name, n)[:3])
    if kind == 'xcorr':
        k, diff = XC.CASES[name][5:7]
        return (RC.xcorr_reference(states, actions, lengths, k, diff),
                RC.xcorr_bounds(states, actions, lengths, k, diff, U[dtype]))
    _, _, _, sd, ad, m, diff, time = KC.CASES[name]
    freqs, inv_std = _inputs(kind, name, n)[3:]
    coeff = KC.coefficients(freqs, inv_std, KC.kappa(1.0, KC.row_dim(sd, ad, diff, time)), NP[dtype])
    return (RC.kme_reference(states, actions, lengths, coeff, diff, time),
            RC.kme_bounds(states, actions, lengths, coeff, diff, time, _itemsize(dtype)))


class Summary:
    """One shape's summarizer: ``run(states, actions, lengths=None, **kw)`` and ``sliced(states, actions, L)``, the
    fixed-length call on trajectories cut at L, in the layout of the shape's row.  xcorr: ``k`` lags; kme: the
    embedding ``emb``."""

    def __init__(self, B, kind, dtype, ts, ta, sd, ad, diff, k=0, emb=None):
        self.B, self.kind, self.dtype = B, kind, dtype
        self.ts, self.ta, self.sd, self.ad, self.diff, self.k, self.emb = ts, ta, sd, ad, bool(diff), k, emb
        self.width = XC.width(sd, ad, k) if kind == 'xcorr' else emb.n_feat
        self.lmin = 2 if self.diff else 1

    @classmethod
    def of_case(cls, B, kind, name, n, dtype):
        if kind == 'xcorr':
            _, ts, ta, sd, ad, k, diff = XC.CASES[name]
            return cls(B, kind, dtype, ts, ta, sd, ad, diff, k=k)
        _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
        freqs, inv_std = _inputs(kind, name, n)[3:]
        emb = B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, diff=bool(diff), time=bool(time), freqs=freqs, device=DEV)
        return cls(B, kind, dtype, ts, ta, sd, ad, diff, emb=emb.set_scale(inv_std, count=n))

    def run(self, states, actions, lengths=None, **kw):
        if lengths is not None:
            kw['lengths'] = lengths
        if self.kind == 'xcorr':
            return self.B.summary_xcorr(states, actions, max_lag=self.k, state_diff=self.diff, dtype=self.dtype, **kw)
        return self.B.summary_kme(states, actions, self.emb, dtype=self.dtype, **kw)

    def sliced(self, states, actions, length):
        s, a = states[:, :length], actions
        if self.kind == 'kme':
            return self.emb(s, a, dtype=self.dtype)
        m_i = length - (1 if self.diff else 0)
        k_i = min(self.k, m_i - 1)
        small = self.B.summary_xcorr(s, a, max_lag=k_i, state_diff=self.diff, dtype=self.dtype)
        row = torch.zeros((states.shape[0], self.width), dtype=self.dtype, device=small.device)      # +0
        cross = (k_i + 1) * self.sd * self.ad
        row[:, :cross] = small[:, :cross]
        row[:, -2 * self.sd:] = small[:, cross:]
        return row


def _check(what, got, ref, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = ratio.max(axis=1)
    print('%s: worst |err| / bound = %.3g (trajectory %d)' % (what, worst.max(), int(worst.argmax())))
    for i in range(got.shape[0]):                      # per trajectory
        assert worst[i] <= 1.0, (what, i, float(worst[i]), int(ratio[i].argmax()))


# ------------------------------------------------------------------ 1. against the definition
@EVERY_CASE
def test_rows_are_the_definition_within_the_derived_bounds(B, kind, name, dtype):
    counts = _counts(B, kind, name, dtype)
    n_all = counts[-1]
    states, actions, lengths = _inputs(kind, name, n_all)[:3]
    ref, bound = _reference(kind, name, n_all, dtype)
    fn = Summary.of_case(B, kind, name, n_all, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    assert ref.shape == (n_all, fn.width)
    for n in counts:
        got = fn.run(s[:n], a[:n], lengths[:n])
        assert got.dtype == dtype and got.is_cuda and tuple(got.shape) == (n, fn.width)
        assert got.data_ptr() % 16 == 0 and got.stride(0) % (16 // got.element_size()) == 0
        _check('%s %s %s n=%d' % (kind, name, dtype, n), got, ref[:n], bound[:n])
    if kind == 'xcorr':
        one_step = RC.steps_of(lengths.numpy(), fn.diff) == 1
        assert one_step.any() and (got[torch.from_numpy(one_step).to(DEV), -fn.sd:] == 0).all()      # sigma at M = 1


# ------------------------------------------------------------------ 2. the bits of the fixed-length entry points
@EVERY_CASE
def test_row_i_is_bitwise_the_fixed_length_call_on_trajectory_i_cut_at_its_length(B, kind, name, dtype):
    n = _counts(B, kind, name, dtype)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    fn = Summary.of_case(B, kind, name, n, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    got = fn.run(s, a, lengths)
    for i, length in enumerate(lengths.tolist()):
        assert _same_bits(got[i:i + 1], fn.sliced(s[i:i + 1], a[i:i + 1], length)), (i, length)
    # lengths on the device, int32 or int64, are the same call; every length = ts is the fixed-length call
    assert _same_bits(fn.run(s, a, lengths.to(DEV)), got)
    assert _same_bits(fn.run(s, a, lengths.to(DEV).to(torch.int32)), got)
    assert _same_bits(fn.run(s, a, [fn.ts] * n), fn.run(s, a))
    assert _same_bits(fn.run(s, a, torch.full((n,), fn.ts, device=DEV)), fn.run(s, a))


# ------------------------------------------------------------------ 3. nothing beyond the length is read
@EVERY_CASE
def test_nothing_at_or_beyond_a_length_reaches_an_output(B, kind, name, dtype):
    n = _counts(B, kind, name, dtype)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    fn = Summary.of_case(B, kind, name, n, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    s_bad, a_bad = s.clone(), a.clone()
    hit = 0
    for i, length in enumerate(lengths.tolist()):
        m_i = length - (1 if fn.diff else 0)
        s_bad[i, length:] = NAN
        if m_i <= fn.ta:            # (with fewer actions than steps the last action is legitimately reused)
            a_bad[i, m_i:] = NAN
        hit += (fn.ts - length) + max(fn.ta - m_i, 0)
    assert hit > 0 or fn.ts == fn.lmin
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    clean = fn.run(s, a, lengths, check_finite=flag).clone()
    got = fn.run(s_bad, a_bad, lengths, check_finite=flag)
    assert int(flag.item()) == 0 and _same_bits(got, clean)


# ------------------------------------------------------------------ 4. a length outside the range
@pytest.mark.parametrize('kind,name,dtype', [('xcorr', 'pendulum_k4', F32), ('xcorr', 'ant', F64), ('xcorr', 'shadowhand', F32),
                                             ('kme', 'pendulum', F32), ('kme', 'edge_ts66', F64), ('kme', 'ant', F32)])
def test_a_device_length_outside_the_range_makes_its_row_nan_and_raises_the_flag(B, kind, name, dtype):
    """A defined result: the kernel clamps the length before it indexes anything (read in csrc/ragged.h), the row
    is NaN, the flag is raised, the other rows keep their bits and the stream goes on."""
    n = _counts(B, kind, name, dtype)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    assert n >= 5
    fn = Summary.of_case(B, kind, name, n, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    clean = fn.run(s, a, lengths).clone()
    bad = lengths.clone()
    rows = {1: 0, 2: fn.ts + 1, n - 1: -7}
    if fn.diff:
        rows[3] = 1                                   # below Lmin = 2 as well
    for i, value in rows.items():
        bad[i] = value
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = fn.run(s, a, bad.to(DEV), check_finite=flag)
    assert int(flag.item()) == 1
    others = [i for i in range(n) if i not in rows]
    assert torch.isnan(got[sorted(rows)]).all()
    assert _same_bits(got[others], clean[others])
    with pytest.raises(AssertionError):
        fn.run(s, a, bad.to(DEV))                     # check_finite=True reads the flag back
    quiet = fn.run(s, a, bad.to(DEV), check_finite=False)
    assert _same_bits(quiet[others], clean[others])
    # the same lengths on the host never reach the GPU
    with pytest.raises(ValueError, match=r'lengths\[1\] = 0 is outside'):
        fn.run(s, a, bad)
    flag.zero_()
    assert _same_bits(fn.run(s, a, lengths.to(DEV), check_finite=flag), clean) and int(flag.item()) == 0


# ------------------------------------------------------------------ 5. a lag with no term
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name', ['pendulum_k4', 'pendulum_raw_k20', 'ant', 'odd_ad_wide', 'two_a_workgroup'])
def test_xcorr_lag_blocks_without_a_term_are_exactly_plus_zero(B, name, dtype):
    n = _counts(B, 'xcorr', name, dtype)[-1]
    states, actions, lengths = _inputs('xcorr', name, n)[:3]
    fn = Summary.of_case(B, 'xcorr', name, n, dtype)
    got = _bits(fn.run(states.to(DEV), actions.to(DEV), lengths)).cpu()
    block, seen = fn.sd * fn.ad, 0
    for i, m_i in enumerate(RC.steps_of(lengths.numpy(), fn.diff)):
        for tau in range(fn.k + 1):
            words = got[i, tau * block:(tau + 1) * block]
            if tau >= m_i:
                assert (words == 0).all(), (i, tau)          # all bits clear: +0.0, not -0.0, not 0 * inf
                seen += 1
            else:
                assert (words != 0).any(), (i, tau)
    assert seen > 0


# ------------------------------------------------------------------ 6. general properties
BITS = pytest.mark.parametrize('kind,name,dtype', [
    ('xcorr', 'pendulum_k4', F32), ('xcorr', 'pendulum_k4', F64), ('xcorr', 'ant', F32), ('xcorr', 'shadowhand', F64),
    ('kme', 'pendulum', F32), ('kme', 'pendulum', F64), ('kme', 'edge_ts66', F32), ('kme', 'five_tiles_two_blocks', F32)])


@BITS
def test_two_runs_are_bitwise_equal_and_rows_do_not_depend_on_their_neighbours_or_on_n(B, kind, name, dtype):
    n = _counts(B, kind, name, dtype)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    fn = Summary.of_case(B, kind, name, n, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    first = fn.run(s, a, lengths).clone()
    assert _same_bits(fn.run(s, a, lengths), first)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n))
    assert not torch.equal(perm, torch.arange(n))
    assert _same_bits(fn.run(s[perm.to(DEV)], a[perm.to(DEV)], lengths[perm]), first[perm.to(DEV)])
    for i in (0, 1, n // 2, n - 1):                 # a row alone: another slot, another workgroup, another N
        assert _same_bits(fn.run(s[i:i + 1], a[i:i + 1], lengths[i:i + 1]), first[i:i + 1]), i


@BITS
def test_out_with_a_wider_pitch_keeps_the_bytes_beyond_the_width(B, kind, name, dtype):
    n = _counts(B, kind, name, dtype)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    fn = Summary.of_case(B, kind, name, n, dtype)
    s, a = states.to(DEV), actions.to(DEV)
    plain = fn.run(s, a, lengths)
    for extra in (3, 4):                            # a multiple of the 16-byte word (fp32) or not
        out = torch.full((n + 1, fn.width + extra), -123.25, dtype=dtype, device=DEV)
        got = fn.run(s, a, lengths, out=out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, fn.width)
        assert _same_bits(got, plain)
        assert (out[:n, fn.width:] == -123.25).all() and (out[n] == -123.25).all()


@pytest.mark.parametrize('kind,name', [('xcorr', 'ta_t_minus_1'), ('kme', 'ta_1')])
def test_cpu_inputs_come_back_on_the_cpu_and_an_empty_batch_touches_nothing(B, kind, name):
    n = _counts(B, kind, name, F32)[-1]
    states, actions, lengths = _inputs(kind, name, n)[:3]
    fn = Summary.of_case(B, kind, name, n, F32)
    got = fn.run(states, actions, lengths)
    assert got.device.type == 'cpu' and tuple(got.shape) == (n, fn.width)
    assert _same_bits(got, fn.run(states.to(DEV), actions.to(DEV), lengths.to(DEV)).cpu())
    out = torch.full((2, fn.width), -5.0, device=DEV)
    for empty in ([], lengths[:0], lengths[:0].to(DEV)):
        none = fn.run(states[:0].to(DEV), actions[:0].to(DEV), empty, out=out)
        assert tuple(none.shape) == (0, fn.width) and (out == -5.0).all()


GRID_CAP = {F32: 256 * 64, F64: 4096}


def _by_length(fn, s, a, lengths):
    """The rows by the FIXED-length entry point: one call per distinct length on the trajectories that have it."""
    want = torch.empty((s.shape[0], fn.width), dtype=fn.dtype, device=DEV)
    for length in sorted(set(lengths.tolist())):
        idx = torch.nonzero(lengths == length).flatten().to(DEV)
        want[idx] = fn.sliced(s[idx], a[idx], length)
    return want


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('sd,ad,ts', [(3, 1, 4), (16, 8, 6)], ids=['16-a-workgroup', '1-a-workgroup'])
def test_xcorr_workgroups_stride_over_more_trajectories_than_the_grid_holds(B, sd, ad, ts, dtype):
    """The parent's shapes, 2 cap G + 5 trajectories, with lengths in 2..ts: every workgroup takes a second batch
    of other lengths, some a third, the last batch is partly empty.  Against the fixed-length entry point, bit for
    bit (which the parent's test holds to the definition)."""
    g = B._lib.load().bsig_xcorr_group(ts, ts, sd, ad, 0, 1, _itemsize(dtype))
    n = 2 * GRID_CAP[dtype] * g + 5
    states, actions = XC.trajectories(n, ts, ts, sd, ad)
    lengths = torch.from_numpy(np.random.RandomState(5).randint(2, ts + 1, size=n))
    fn = Summary(B, 'xcorr', dtype, ts, ts, sd, ad, True)
    s, a = torch.from_numpy(states).to(DEV), torch.from_numpy(actions).to(DEV)
    got = fn.run(s, a, lengths.to(DEV))
    assert _same_bits(got, _by_length(fn, s, a, lengths))


def test_kme_workgroups_stride_over_more_trajectories_than_the_grid_holds(B):
    """The parent's shape with one state more (two states leave one length only): 2 cap G + 5 one-block
    trajectories of lengths 2 and 3."""
    sd, ad, ts, m = 3, 1, 3, 2
    g = B._lib.load().bsig_kme_group(ts, ts, sd, ad, m, 1, 0, 4)
    assert g == 8
    n = 2 * GRID_CAP[F32] * g + 5
    states, actions = KC.trajectories(n, ts, ts, sd, ad)
    lengths = torch.from_numpy(np.random.RandomState(5).randint(2, ts + 1, size=n))
    freqs = np.random.RandomState(2).standard_normal((m, 7)).astype(np.float32)
    inv_std = KC.flat_rule_inv_std(KC.rows(states[:256], actions[:256], 1, 0).reshape(-1, 7))
    fn = Summary(B, 'kme', F32, ts, ts, sd, ad, True,
                 emb=B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, freqs=freqs, device=DEV).set_scale(inv_std))
    s, a = torch.from_numpy(states).to(DEV), torch.from_numpy(actions).to(DEV)
    got = fn.run(s, a, lengths.to(DEV))
    assert _same_bits(got, _by_length(fn, s, a, lengths))


# ------------------------------------------------------------------ 7. the compacted rows and the scale
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name', ['pendulum', 'm100_time', 'm1_raw_time', 'ta_1', 'ta_above_t', 'edge_ts66'])
def test_the_compacted_rows_are_numpys_bit_for_bit(B, name, dtype):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    n = _counts(B, 'kme', name, dtype)[-1]
    states, actions, lengths = _inputs('kme', name, n)[:3]
    fn = Summary.of_case(B, 'kme', name, n, dtype)
    want = RC.kme_rows_compacted(states.numpy(), actions.numpy(), lengths.numpy(), diff, time, NP[dtype],
                                 header_tau=True)
    total, d = int(RC.steps_of(lengths.numpy(), diff).sum()), KC.row_dim(sd, ad, diff, time)
    assert want.shape == (total, d)
    for given in (lengths, lengths.tolist(), lengths.to(DEV)):
        got = fn.emb.rows(states.to(DEV), actions.to(DEV), dtype=dtype, lengths=given)
        assert got.dtype == dtype and tuple(got.shape) == (total, d)
        assert np.array_equal(got.cpu().numpy(), want)
    # the entry point itself: rows beyond the total, and the columns beyond d, are not touched
    _lib = B._lib
    prec = _lib.F64 if dtype == F64 else _lib.F32
    s, a = states.to(DEV).to(dtype).contiguous(), actions.to(DEV).to(dtype).contiguous()
    steps = lengths - (1 if diff else 0)
    offsets = (torch.cumsum(steps, 0) - steps).to(DEV)
    buf = torch.full((total + 3, d + 2), -9.0, dtype=dtype, device=DEV)
    prec.kme_rows_ragged(_lib.ptr(s), _lib.ptr(a), _lib.ptr(lengths.to(DEV).to(torch.int32)), _lib.ptr(offsets),
                         _lib.ptr(buf), n, ts, ta, sd, ad, diff, time, d + 2, _lib.stream())
    assert np.array_equal(buf[:total, :d].cpu().numpy(), want)
    assert (buf[total:] == -9.0).all() and (buf[:, d:] == -9.0).all()


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name', ['pendulum', 'm100_time', 'ant'])
def test_fit_scale_with_lengths_is_the_flat_rule_of_the_valid_rows(B, name, dtype, monkeypatch):
    _, ts, ta, sd, ad, m, diff, time = KC.CASES[name]
    n = _counts(B, 'kme', name, dtype)[-1]
    states, actions, lengths, freqs, _ = _inputs('kme', name, n)
    ended = B.pairs.end_episodes(states, actions, lengths)
    s, a = ended[0].to(DEV), ended[1].to(DEV)

    def fresh():
        return B.KernelMeanEmbedding(sd, ad, n_feat=2 * m, diff=bool(diff), time=bool(time), freqs=freqs, device=DEV)
    emb = fresh().fit_scale(s, a, dtype=dtype, lengths=lengths)
    assert emb.ready and int(emb.count) == n
    # the comparison tests/test_gpu_kme.py makes for the fixed-length scale, on the valid rows
    xs = RC.kme_rows_compacted(ended[0].numpy(), ended[1].numpy(), lengths.numpy(), diff, time, NP[dtype],
                               header_tau=True)
    assert np.array_equal(emb.rows(s, a, dtype=dtype, lengths=lengths).cpu().numpy(), xs)
    ref_mean, ref_std, ref_flat = NC.reference_stats(xs)
    got = emb.inv_std.cpu().numpy()
    assert np.array_equal(got == 0.0, ref_flat) and np.isfinite(got).all()
    kept = ~ref_flat
    err = np.abs(1.0 / got[kept].astype(np.longdouble) - ref_std[kept])
    assert (err <= 8 * xs.shape[0] * NC.U53 * (ref_std + np.abs(ref_mean))[kept]).all()
    # the repeated tail changes the scale: without lengths, on the padded episodes, it is another one
    padded = fresh().fit_scale(s, a, dtype=dtype)
    assert not torch.equal(padded.inv_std, emb.inv_std)
    # lengths on the device: the same bits; the one read-back is the first 256 lengths at most
    dev = fresh().fit_scale(s, a, dtype=dtype, lengths=lengths.to(DEV))
    assert torch.equal(dev.inv_std, emb.inv_std)

    def no_item(self):
        raise RuntimeError('read-back')
    host, fresh_dev = fresh(), fresh()
    monkeypatch.setattr(torch.Tensor, 'item', no_item)
    monkeypatch.setattr(torch.Tensor, 'cpu', no_item)
    with pytest.raises(RuntimeError, match='read-back'):
        fresh_dev.fit_scale(s, a, dtype=dtype, lengths=lengths.to(DEV))    # lengths on the device: the one
    host.fit_scale(s, a, dtype=dtype, lengths=lengths)                      # lengths on the host: none
    monkeypatch.undo()
    assert torch.equal(host.inv_std, emb.inv_std)


# ------------------------------------------------------------------ 8. BayesSim
CFGS = {
    'summary_xcorr': {'modelClass': 'MDNN', 'summarizerFxn': 'summary_xcorr', 'trainTrajLen': 21, 'components': 3,
                      'hiddenLayers': (16, 16), 'lr': 1e-3, 'xcorrLags': 4},
    'summary_kme': {'modelClass': 'MDNN', 'summarizerFxn': 'summary_kme', 'trainTrajLen': 21, 'components': 3,
                    'hiddenLayers': (16, 16), 'lr': 1e-3, 'kmeFeatures': 64},
}
DOUBLE = {'dtype': 'float64', 'summaryDtype': 'float64'}
MODES = pytest.mark.parametrize('name,extra', [(n, e) for n in sorted(CFGS) for e in ({}, DOUBLE)],
                                ids=['%s-%s' % (n[8:], 'fp64' if e else 'fp32') for n in sorted(CFGS) for e in ({}, DOUBLE)])


def _bayes_sim(B, cfg):
    torch.manual_seed(11)          # the start weights
    return B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01, 0.01]),
                      params_highs=np.array([2.0, 2.0]), prior=None, device=DEV)


@functools.lru_cache(maxsize=None)
def _pendulum(B):
    """2000 pairs = two protocol chunks, their episodes ended at seeded lengths in 6..21."""
    theta, states, actions = B.pairs.pendulum_pairs(2000, 20, policy='random', seed=4, device=DEV)
    lengths = torch.from_numpy(np.random.RandomState(12).randint(6, 22, size=2000))
    ended = B.pairs.end_episodes(states, actions, lengths)
    return theta, states, actions, lengths, ended[0], ended[1]


def _fit(B, cfg, *args, **kw):
    bs = _bayes_sim(B, cfg)
    np.random.seed(31), torch.manual_seed(32)
    return bs, bs.fit(*args, **kw)


def _same_logs(a, b):
    assert len(a) == len(b) == 2
    for chunk_a, chunk_b in zip(a, b):
        for key in ('train_loss', 'test_loss'):
            assert len(chunk_a[key]) > 0 and np.isfinite(chunk_a[key]).all()
            assert np.array_equal(np.asarray(chunk_a[key]), np.asarray(chunk_b[key])), key


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


@MODES
def test_fit_with_every_length_the_whole_trajectory_is_fit_without_lengths(B, name, extra):
    theta, states, actions = _pendulum(B)[:3]
    cfg = dict(CFGS[name], **extra)
    plain, logs_plain = _fit(B, cfg, theta, states, actions)
    for lengths in ([21] * 2000, torch.full((2000,), 21, dtype=torch.int32, device=DEV)):
        bs, logs = _fit(B, cfg, theta, states, actions, traj_lengths=lengths)
        _same_logs(logs, logs_plain)
        _same_state(bs.model, plain.model)
        if bs.embedding is not None:
            _same_state(bs.embedding, plain.embedding)


@MODES
def test_fit_with_lengths_is_the_same_on_the_block_path_and_chunk_by_chunk(B, name, extra, monkeypatch):
    theta, _, _, lengths, states, actions = _pendulum(B)
    cfg = dict(CFGS[name], **extra)
    dtype = F64 if extra else F32
    runs = []
    for no_block in ('0', '1'):
        monkeypatch.setenv('BSIG_NO_FIT_PREPROJECT', no_block)
        bs = _bayes_sim(B, cfg)
        calls, summarizer = [], bs.summarizer_fxn
        bs.summarizer_fxn = lambda *args, **kw: (calls.append(kw), summarizer(*args, **kw))[1]
        np.random.seed(31), torch.manual_seed(32)
        logs = bs.fit(theta, states, actions, traj_lengths=lengths)
        bs.summarizer_fxn = summarizer
        # one launch for the block, one per chunk without it; the lengths are cut with the trajectories
        assert [int(kw['lengths'].shape[0]) for kw in calls] == ([2000] if no_block == '0' else [1000, 1000])
        assert all(kw['lengths'].is_cuda and torch.is_tensor(kw['check_finite']) for kw in calls)
        runs.append((bs, logs))
    monkeypatch.delenv('BSIG_NO_FIT_PREPROJECT')
    (bs, logs), (bs_chunks, logs_chunks) = runs
    _same_logs(logs, logs_chunks)
    _same_state(bs.model, bs_chunks.model)
    # and not the fit on the padded episodes without lengths
    _, logs_padded = _fit(B, cfg, theta, states, actions)
    assert not np.array_equal(np.asarray(logs[0]['train_loss']), np.asarray(logs_padded[0]['train_loss']))
    if bs.embedding is not None:
        _same_state(bs.embedding, bs_chunks.embedding)
        # the scale: from the first 256 training trajectories' valid rows
        alone = B.KernelMeanEmbedding(3, 1, n_feat=64, device=DEV).fit_scale(states[:256], actions[:256], dtype=dtype,
                                                                            lengths=lengths[:256])
        assert int(bs.embedding.count) == 256 and torch.equal(alone.inv_std, bs.embedding.inv_std)
    # the summaries the model saw are the summarizer's with lengths
    rows = bs._summarize(states, actions, lengths=lengths)
    assert rows.dtype == dtype and torch.isfinite(rows).all()
    assert not torch.equal(rows, bs._summarize(states, actions))
    # predict: a finite mixture, the mixture of the one trajectory cut at its length
    i = int(torch.nonzero(lengths < 21)[0])
    length = int(lengths[i])
    torch.manual_seed(42)          # (a prediction draws the seed of its covariance jitter from torch's generator)
    mog = bs.predict(states[i:i + 1], actions[i:i + 1], lengths=[length])
    torch.manual_seed(42)
    cut = bs.predict(states[i:i + 1, :length], actions[i:i + 1])
    assert isinstance(mog, B.pdf.MoG) and np.isfinite(mog.a).all() and abs(float(np.sum(mog.a)) - 1.0) <= 1e-6
    assert np.array_equal(mog.a, cut.a)
    at = theta[:8].cpu().numpy().astype(np.float64)
    assert np.isfinite(mog.eval(at)).all() and np.array_equal(mog.eval(at), cut.eval(at))
    assert not np.array_equal(mog.a, bs.predict(states[i:i + 1], actions[i:i + 1]).a)


def test_run_training_alone_makes_the_kme_scale_from_the_valid_rows(B):
    theta, _, _, lengths, states, actions = _pendulum(B)
    bs = _bayes_sim(B, CFGS['summary_kme'])
    np.random.seed(21), torch.manual_seed(22)
    logs = bs.run_training(theta[:1000], states[:1000], actions[:1000], traj_lengths=lengths[:1000])
    assert np.isfinite(logs['train_loss']).all() and bs.embedding.ready and int(bs.embedding.count) == 256
    alone = B.KernelMeanEmbedding(3, 1, n_feat=64, device=DEV).fit_scale(states[:256], actions[:256],
                                                                        lengths=lengths[:256])
    assert torch.equal(alone.inv_std, bs.embedding.inv_std)
    explicit = _bayes_sim(B, CFGS['summary_kme']).fit_embedding_scale(states[:256], actions[:256], lengths=lengths[:256])
    assert torch.equal(explicit.embedding.inv_std, bs.embedding.inv_std)
    without = _bayes_sim(B, CFGS['summary_kme']).fit_embedding_scale(states[:256], actions[:256])
    assert not torch.equal(without.embedding.inv_std, bs.embedding.inv_std)


@pytest.mark.parametrize('name', sorted(CFGS))
def test_a_device_length_of_zero_inside_a_chunk_fails_the_fits_deferred_assert(B, name):
    theta, _, _, lengths, states, actions = _pendulum(B)
    bad = lengths.to(DEV)
    bad[1500] = 0
    bs = _bayes_sim(B, CFGS[name])
    np.random.seed(31), torch.manual_seed(32)
    with pytest.raises(AssertionError):
        bs.fit(theta, states, actions, traj_lengths=bad)
    # on the host the same length never reaches the GPU
    with pytest.raises(ValueError, match=r'lengths\[1500\] = 0 is outside 2\.\.21'):
        _bayes_sim(B, CFGS[name]).fit(theta, states, actions, traj_lengths=bad.cpu())
