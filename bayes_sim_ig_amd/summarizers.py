"""Trajectory summarizers on MI355X — host-side mirror of the reference's
bayes_sim_ig/utils/summarizers.py (same names, arguments and error
behaviour); the arithmetic runs in libbsig_hip (csrc/summarizers.hip).

Every function maps states[N,T,sd], actions[N,Ta,ad] (fp32) to a [N,F]
tensor on the inputs' device.  The rows live in HBM with a 16-byte aligned
pitch (ld = F rounded up to 4 floats) and the returned tensor is the [:, :F]
view, so the estimator's GEMM loaders can use 128-bit loads.

``dtype=torch.float64`` on any of them computes the summary in double instead
(csrc/f64/summarizers_f64.hip): the inputs are widened -- exact for fp32 data --
or taken as they are, the rows are float64 at a pitch of F rounded up to 2
doubles.  ``None`` / ``torch.float32`` is the fp32 path, which narrows a
float64 input.  Which library entry point a call reaches is decided by the
precision seam (``_lib.F32`` / ``_lib.F64``).
"""
import ctypes as C
import operator

import numpy as np
import torch

from . import _lib

KIND_START, KIND_CORR, KIND_CORRDIFF, KIND_SIGNATURE = 0, 1, 2, 3


def _precision(dtype):
    """The precision a summarizer call computes in: ``_lib.F32`` for ``None`` / float32, ``_lib.F64``."""
    if dtype is None or dtype == torch.float32:
        return _lib.F32
    if dtype == torch.float64:
        return _lib.F64
    raise ValueError('summarizers compute in torch.float32 or torch.float64, got dtype=%r' % (dtype,))


def _need_trajectories(states, actions):
    assert len(states.shape) == 3, 'Need states: ntraj x n_steps x state_dim'
    assert len(actions.shape) == 3, 'Need actions: ntraj x n_steps x state_dim'


def _prep(states, actions, prec=_lib.F32, device=None):
    """The trajectories in ``prec`` on a GPU -- ``device`` (they move there as they are, then convert), else
    their own, else the current one -- and the device they came from."""
    _need_trajectories(states, actions)
    assert states.shape[0] == actions.shape[0]
    _lib.require_gpu()
    home = states.device
    if device is not None:
        states, actions = states.to(device), actions.to(device)
    dev = states.device if states.is_cuda else torch.device('cuda', torch.cuda.current_device())
    if prec.itemsize == 8:      # the smaller form crosses the bus: widened (exactly) on the device
        s = states.to(device=dev).to(prec.dtype).contiguous()
        a = actions.to(device=dev).to(prec.dtype).contiguous()
    else:
        s = states.to(device=dev, dtype=prec.dtype).contiguous()
        a = actions.to(device=dev, dtype=prec.dtype).contiguous()
    return s, a, home


def _alloc(n, width, device, out, prec=_lib.F32):
    ld = _lib.round_up(width, 16 // prec.itemsize)
    if out is not None:
        assert out.is_cuda and out.dtype == prec.dtype and out.dim() == 2
        assert out.shape[0] >= n and out.stride(1) == 1 and out.stride(0) >= width
        return out, out.stride(0)
    return torch.empty((n, ld), dtype=prec.dtype, device=device), ld


def _finish(buf, n, width, home, out):
    res = buf[:n, :width]
    if out is None and home != buf.device:
        res = res.to(home)
    return res


def _finite_flag(check_finite, device):
    """The flag word a cross-correlation kernel raises on a non-finite feature, and whether this call reads it
    back.  ``check_finite`` may be a 1-element int32 device tensor: the kernel raises its flag there and the
    caller asserts later (BayesSim.fit: one read-back for all chunks); None / False: no flag."""
    if torch.is_tensor(check_finite):
        return check_finite, False
    if not check_finite:
        return None, False
    return torch.zeros(1, dtype=torch.int32, device=device), True


def _assert_finite(flag, read_back):
    if read_back:
        assert int(flag.item()) == 0  # summarizers.py:120


def _launch_summary(states, actions, prec, width, out, check_finite, launch, device=None):
    """The host side of every ``[N, F]`` summary: the trajectories on a GPU (``_prep``), THAT device current and
    its stream the library's, the rows (``out=`` or new), the finite flag (none for ``check_finite=False``), the
    one library call ``launch(s, a, buf, ld, flag, stream)``, the flag's read-back, the ``[:n, :width]`` view back
    where the inputs live.  ``width``: F, or ``(s, a) -> F`` where it, or an assert on the shapes, has to follow
    the move to the GPU."""
    s, a, home = _prep(states, actions, prec, device)
    if callable(width):
        width = width(s, a)
    with _lib.device_stream(s.device) as stream:
        buf, ld = _alloc(s.shape[0], width, s.device, out, prec)
        flag, read_back = _finite_flag(check_finite, s.device)
        launch(s, a, buf, ld, flag, stream)
        _assert_finite(flag, read_back)
    return _finish(buf, s.shape[0], width, home, out)


def check_lengths(lengths, n, ts, diff, name='lengths'):
    """``lengths`` of ``summary_xcorr`` / ``summary_kme`` (include/bsig_ragged.h) before any GPU call: an int32 /
    int64 tensor, a numpy integer array or a list of ``n`` values, the valid STATES of every trajectory.
    ValueError for another shape or a dtype that is not an integer's.  Lengths on the host are range-checked
    here -- ``Lmin..ts``, Lmin = 2 where differences are formed (``diff``), else 1 -- and the ValueError names the
    first index outside; they come back as a CPU int32 tensor.  Lengths on the device come back as they are and
    are never read back: a length outside the range makes its row NaN and raises the finite flag."""
    if torch.is_tensor(lengths):
        if lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError('%s must hold integers (int32 or int64), got dtype %s' % (name, lengths.dtype))
        if tuple(lengths.shape) != (n,):
            raise ValueError('%s must hold one value per trajectory, shape (%d,), got %r'
                             % (name, n, tuple(lengths.shape)))
        if lengths.is_cuda:
            return lengths
        host = lengths.detach().numpy()
    else:
        host = np.asarray(lengths)
        if host.size == 0 and host.ndim == 1:      # (an empty list has no dtype of its own)
            host = host.astype(np.int64)
        if host.dtype.kind not in 'iu':
            raise ValueError('%s must hold integers, got dtype %s' % (name, host.dtype))
        if host.shape != (n,):
            raise ValueError('%s must hold one value per trajectory, shape (%d,), got %r'
                             % (name, n, tuple(host.shape)))
    lmin = 2 if diff else 1
    outside = np.flatnonzero((host < lmin) | (host > ts))
    if outside.size:
        i = int(outside[0])
        raise ValueError('%s[%d] = %d is outside %d..%d (the valid states of a trajectory of %d)'
                         % (name, i, int(host[i]), lmin, ts, ts))
    return torch.from_numpy(host.astype(np.int32))


def _lengths_on(lengths, device):
    """What ``check_lengths`` returned as the contiguous int32 device vector the kernels read."""
    if lengths.dtype == torch.int64:      # (a device value beyond int32 stays outside every range)
        lengths = lengths.clamp(min=-1, max=2 ** 31 - 1)
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def summary_dim(name, traj_len, obs_dim, act_dim, depth=0):
    """Width F of ``name``'s output without touching the GPU (what
    bayes_sim.py:57-60 obtains by pushing a zero trajectory through)."""
    kind = {'summary_start': 0, 'summary_waypts': 0, 'summary_corr': 1,
            'summary_corrdiff': 2, 'summary_signatory': 3}[name]
    return int(_lib.load().bsig_summary_dim(kind, traj_len, obs_dim, act_dim, depth))


def pad_states_actions(states, actions, tgt_actions_len=None):
    """Reference summarizers.py:20-62 (plain slicing / repeat; no arithmetic).
    Unlike the reference, padding works for any batch size: each trajectory
    repeats its own last step."""
    _need_trajectories(states, actions)
    if tgt_actions_len is None:
        tgt_actions_len = states.shape[1]

    def fit(seq):
        if seq.shape[1] >= tgt_actions_len:
            return seq[:, :tgt_actions_len, :]
        tail = seq[:, -1:, :].expand(-1, tgt_actions_len - seq.shape[1], -1)
        return torch.cat([seq, tail], dim=1)
    states, actions = fit(states), fit(actions)
    assert states.shape[1] == actions.shape[1]
    return states, actions


def summary_start(states, actions, max_t=10, out=None, dtype=None):
    """Reference summarizers.py:65-70."""
    prec = _precision(dtype)

    def launch(s, a, buf, ld, flag, stream):
        prec.summary_start(
            _lib.ptr(s), _lib.ptr(a), _lib.ptr(buf), s.shape[0], s.shape[1], a.shape[1],
            s.shape[2], a.shape[2], max_t, ld, stream)
    return _launch_summary(states, actions, prec, lambda s, a: max_t * (s.shape[2] + a.shape[2]), out, False,
                           launch)


def summary_waypts(states, actions, n_waypts=10, out=None, dtype=None):
    """Reference summarizers.py:73-87: the crop to ``n_waypts`` precedes the
    stride computation, so the waypoints are the first ``n_waypts`` steps."""
    return summary_start(states, actions, max_t=n_waypts, out=out, dtype=dtype)


class CrossCorrFactors:
    """A cross-correlation summary that is not materialised.

    summarizers.py:106-119 builds, per trajectory, the outer product of S state features
    and A action features (+ mean and std of the state features): 47 KB per Ant row,
    420 KB per ShadowHand row, 98 % of it products of the same S + A numbers.  This handle
    keeps the factor rows ``[sf | af | mean | std | 1]`` (S + A + 3 floats per trajectory,
    include/bsig.h) and behaves like the ``[N, S*A + 2]`` summary wherever the estimator
    only needs its rows: ``MDNN.run_training`` hands the factor rows to the fit engine,
    whose first-layer tiles form ``sf[i] * af[j]`` on the fly -- the same single fp32
    multiply the summarizer does, so the first-layer inputs are bit-identical -- and no
    ``[N, S*A + 2]`` tensor, staging copy or per-update gather of 47 KB rows exists (only
    the held-out fifth of a chunk, read once per evaluation, is expanded into rows).
    ``materialize()`` (or any tensor use via ``torch.as_tensor`` semantics: indexing a
    column, ``.cpu()``, arithmetic) expands the rows with bsig_crosscorr_expand.
    """

    def __init__(self, factors, s_dim, a_dim):
        self.factors, self.s_dim, self.a_dim = factors, int(s_dim), int(a_dim)

    # --- the tensor surface BayesSim / MDNN.run_training touch
    @property
    def shape(self):
        return torch.Size((self.factors.shape[0], self.s_dim * self.a_dim + 2))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 2

    @property
    def device(self):
        return self.factors.device

    @property
    def is_cuda(self):
        return self.factors.is_cuda

    @property
    def dtype(self):
        return torch.float32

    def __len__(self):
        return self.factors.shape[0]

    def __getitem__(self, rows):
        """Row selection keeps the factored form; anything else materialises."""
        if isinstance(rows, slice) or (torch.is_tensor(rows) and rows.dim() == 1) or \
                isinstance(rows, (list, range)):
            return CrossCorrFactors(self.factors[rows], self.s_dim, self.a_dim)
        return self.materialize()[rows]

    def materialize(self, out=None):
        """The ``[N, S*A + 2]`` summary rows (16-byte aligned pitch, like the summarizers)."""
        lib = _lib.require_gpu()
        n, width = self.shape
        fac = self.factors if self.factors.stride(1) == 1 else self.factors.contiguous()
        with _lib.device_stream(fac.device) as stream:
            buf, ld = _alloc(n, width, fac.device, out)
            _lib.check(lib.bsig_crosscorr_expand(
                _lib.ptr(fac), fac.stride(0) if n > 1 else fac.shape[1], n, self.s_dim, self.a_dim,
                _lib.ptr(buf), ld, stream))
        return buf[:n, :width]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        # any torch function applied to a handle sees the materialised tensor
        def expand(a):
            if isinstance(a, CrossCorrFactors):
                return a.materialize()
            if isinstance(a, (list, tuple)):
                return type(a)(expand(v) for v in a)
            return a
        return func(*[expand(a) for a in args], **{k: expand(v) for k, v in (kwargs or {}).items()})

    def cpu(self):
        return self.materialize().cpu()

    def to(self, *args, **kwargs):
        return self.materialize().to(*args, **kwargs)


def cross_correlation(states, actions, use_state_diff=False, out=None,
                      check_finite=True, lazy=False, dtype=None):
    """Reference summarizers.py:90-122.  ``lazy=True`` returns a CrossCorrFactors handle
    instead of the materialised ``[N, S*A + 2]`` tensor (fp32 only)."""
    prec = _precision(dtype)
    if lazy:
        if prec is _lib.F64:
            raise NotImplementedError(
                'lazy=True with dtype=torch.float64: there are no factor rows in double -- the fp64 fit '
                'refuses them (bsig_fit64_bind: BSIG_X_CROSSCORR_FACTORS is BSIG_EUNSUPPORTED)')
        return _cross_correlation_factors(states, actions, use_state_diff, check_finite)

    def width(s, a):
        assert s.shape[1] > 1         # summarizers.py:94
        return summary_dim('summary_corrdiff' if use_state_diff else 'summary_corr',
                           s.shape[1], s.shape[2], a.shape[2])

    def launch(s, a, buf, ld, flag, stream):
        n, t, sd = s.shape
        prec.crosscorr(
            _lib.ptr(s), _lib.ptr(a), _lib.ptr(buf), n, t, a.shape[1], sd, a.shape[2],
            1 if use_state_diff else 0, ld, _lib.ptr(flag), stream)
    return _launch_summary(states, actions, prec, width, out, check_finite, launch)


def _cross_correlation_factors(states, actions, use_state_diff, check_finite):
    s, a, home = _prep(states, actions)
    n, t, sd = s.shape
    ad = a.shape[2]
    assert t > 1                      # summarizers.py:94
    lib = _lib.load()
    s_dim, a_dim = C.c_int32(), C.c_int32()
    _lib.check(lib.bsig_crosscorr_factor_dims(t, sd, ad, C.byref(s_dim), C.byref(a_dim)))
    ld = _lib.round_up(s_dim.value + a_dim.value + 3, 4)
    fac = torch.empty((n, ld), dtype=torch.float32, device=s.device)
    flag, read_back = _finite_flag(check_finite, s.device)
    with _lib.device_stream(s.device) as stream:
        _lib.check(lib.bsig_crosscorr_factors(
            _lib.ptr(s), _lib.ptr(a), _lib.ptr(fac), n, t, a.shape[1], sd, ad,
            1 if use_state_diff else 0, ld, _lib.ptr(flag), stream))
    _assert_finite(flag, read_back)
    return CrossCorrFactors(fac, s_dim.value, a_dim.value)


def summary_corrdiff(states, actions, out=None, check_finite=True, lazy=False, dtype=None):
    return cross_correlation(states, actions, use_state_diff=True, out=out,
                             check_finite=check_finite, lazy=lazy, dtype=dtype)


def summary_corr(states, actions, out=None, check_finite=True, lazy=False, dtype=None):
    return cross_correlation(states, actions, use_state_diff=False, out=out,
                             check_finite=check_finite, lazy=lazy, dtype=dtype)


def xcorr_dim(obs_dim, act_dim, max_lag=0):
    """Width of a ``summary_xcorr`` row, ``(max_lag + 1) * obs_dim * act_dim + 2 * obs_dim``, without touching
    the GPU (bsig_xcorr_dim, include/bsig_xcorr.h).  ValueError for a dimension below 1, a negative
    ``max_lag`` or a width past 2^31 - 1."""
    width = int(_lib.load().bsig_xcorr_dim(int(obs_dim), int(act_dim), _xcorr_lag(max_lag)))
    if width < 0:
        raise ValueError('no cross-correlation row for obs_dim=%r, act_dim=%r, max_lag=%r (dimensions >= 1, '
                         'max_lag >= 0, width below 2^31)' % (obs_dim, act_dim, max_lag))
    return width


def _xcorr_lag(max_lag):
    """``max_lag`` as an int that fits the C ABI; ValueError if it is not an integer (a bool is not)."""
    if isinstance(max_lag, bool):
        raise ValueError('max_lag must be an int >= 0, got %r' % (max_lag,))
    try:
        lag = operator.index(max_lag)
    except TypeError:
        raise ValueError('max_lag must be an int >= 0, got %r' % (max_lag,)) from None
    return max(min(lag, 2 ** 31 - 1), -1)


def summary_xcorr(states, actions, max_lag=0, state_diff=True, out=None, check_finite=True, dtype=None,
                  lengths=None):
    """The time-lagged cross-correlation summary of the BayesSim paper (RSS 2019, section IV.F; not in the
    reference, whose ``cross_correlation`` is another statistic): with ``f_t = s_(t+1) - s_t``, the difference
    in TIME (``state_diff=False``: ``f_t = s_t``), M such steps, and the actions padded as
    ``pad_states_actions`` leaves them, the row is ``[c_0 | ... | c_max_lag | mu | sigma]`` --
    ``c_tau[i, j] = 1/(M - tau) * sum_t f_(t+tau),i * a_t,j`` flattened with i major, then the mean and the
    population standard deviation of every ``f_.,i`` -- ``xcorr_dim(sd, ad, max_lag)`` numbers from the whole
    trajectory, whatever its length (include/bsig_xcorr.h, csrc/xcorr.h).

    ``lengths`` (include/bsig_ragged.h; ``check_lengths``): the valid states ``L_n`` of every trajectory, for
    recorded episodes that end early and whose tail the recorder filled.  Row n is then, bit for bit, the row of
    ``states[n:n + 1, :L_n]`` and ``actions[n:n + 1]``; a lag with no term (``tau >= M_n``) is a block of zeros;
    ``max_lag`` is still checked against the M of the whole tensor.  Lengths on the host are range-checked
    here; lengths on the device are never read back: one outside ``2..ts`` (``1..ts`` without ``state_diff``)
    makes its row NaN and fails the finite check.  ``None``: the call it always was.

    ``out=``, ``check_finite`` and ``dtype=torch.float64`` are ``cross_correlation``'s.  ValueError (before
    any GPU call) for a ``max_lag`` outside ``0..M-1``; NotImplementedError when a trajectory does not fit a
    workgroup's LDS."""
    prec = _precision(dtype)
    lag = _xcorr_lag(max_lag)
    _need_trajectories(states, actions)
    m = states.shape[1] - (1 if state_diff else 0)
    assert m >= 1, 'Need %d states or more' % (2 if state_diff else 1)
    if not 0 <= lag <= m - 1:
        raise ValueError('max_lag %r is outside 0..%d: the feature series has %d steps' % (max_lag, m - 1, m))
    if lengths is not None:
        lengths = check_lengths(lengths, states.shape[0], states.shape[1], state_diff)

    def launch(s, a, buf, ld, flag, stream):
        n, t, sd = s.shape
        tail = (n, t, a.shape[1], sd, a.shape[2], lag, 1 if state_diff else 0, ld, _lib.ptr(flag), stream)
        if lengths is None:
            prec.xcorr(_lib.ptr(s), _lib.ptr(a), _lib.ptr(buf), *tail)
        else:
            lens = _lengths_on(lengths, s.device)
            prec.xcorr_ragged(_lib.ptr(s), _lib.ptr(a), _lib.ptr(lens), _lib.ptr(buf), *tail)
    return _launch_summary(states, actions, prec, lambda s, a: xcorr_dim(s.shape[2], a.shape[2], lag), out,
                           check_finite, launch)


def _obs_act_width(what, dim_fn, obs_dim, act_dim, *flags):
    """``sysid_dim`` and ``kme_row_dim``: what the library's ``dim_fn`` answers for ints in 1..2^31 - 1, asked
    for nothing else; ValueError for anything else or a negative answer (no ``what`` row)."""
    try:
        sd, ad = operator.index(obs_dim), operator.index(act_dim)
    except TypeError:
        raise ValueError('obs_dim and act_dim must be ints >= 1, got %r, %r' % (obs_dim, act_dim)) from None
    ok = 1 <= sd < 2 ** 31 and 1 <= ad < 2 ** 31
    width = int(getattr(_lib.load(), dim_fn)(sd, ad, *flags)) if ok else -1
    if width < 0:
        raise ValueError('no %s row for obs_dim=%r, act_dim=%r (dimensions >= 1, width below 2^31)'
                         % (what, obs_dim, act_dim))
    return width


def sysid_dim(obs_dim, act_dim):
    """Width of a ``summary_sysid`` row, ``(1 + obs_dim + act_dim) * obs_dim + obs_dim``, without touching the
    GPU (bsig_sysid_dim, include/bsig_sysid.h).  ValueError for a dimension below 1 or a width past 2^31 - 1."""
    return _obs_act_width('dynamics-fit', 'bsig_sysid_dim', obs_dim, act_dim)


def sysid_ridge(ridge, name='ridge'):
    """``ridge`` of ``summary_sysid`` as a float; ValueError unless it is a positive finite float (an int or a
    bool is not) that stays positive in fp32."""
    if not isinstance(ridge, float) or not (np.isfinite(ridge) and np.float32(ridge) > 0.0):
        raise ValueError('%s must be a positive float, got %r' % (name, ridge))
    return ridge


def summary_sysid(states, actions, ridge=1e-3, out=None, check_finite=True, dtype=None):
    """The least-squares dynamics summary of every trajectory (not in the reference): the ridge fit of
    ``y_t = s_(t+1) - s_t`` on ``phi_t = [1 | s_t | a_t]`` over the trajectory's own M = T - 1 steps, the
    actions padded as ``pad_states_actions`` leaves them.  With ``G = 1/M sum phi_t phi_t^T``,
    ``B = 1/M sum phi_t y_t^T`` and ``rho = ridge * trace(G) / p``, p = 1 + sd + ad, the row is
    ``[W | r]``: ``W = (G + rho I)^-1 B`` row-major, then ``r_j = sqrt(1/M sum_t (y_tj - phi_t . W_:j)^2)`` --
    ``sysid_dim(sd, ad)`` deterministic numbers, whatever the trajectory's length (include/bsig_sysid.h,
    csrc/sysid.h).  The condition number of the solved system is at most ``1 + p / ridge``: where
    ``p^2 * 6e-8 / ridge`` nears 1, compute in double.

    ``out=``, ``check_finite`` and ``dtype=torch.float64`` are ``cross_correlation``'s; a trajectory with a
    non-finite value, or whose factorisation meets a pivot that is not positive, has a row of NaN and fails
    the finite check.  ValueError (before any GPU call) for a ``ridge`` that is not a positive float or
    fewer than two states; NotImplementedError when a trajectory does not fit a workgroup's LDS."""
    prec = _precision(dtype)
    ridge = sysid_ridge(ridge)
    _need_trajectories(states, actions)
    if states.shape[1] < 2:
        raise ValueError('summary_sysid needs 2 states or more, got %d' % (states.shape[1],))
    if actions.shape[1] < 1:
        raise ValueError('summary_sysid needs 1 action or more, got %d' % (actions.shape[1],))
    width = sysid_dim(states.shape[2], actions.shape[2])

    def launch(s, a, buf, ld, flag, stream):
        n, t, sd = s.shape
        prec.sysid(_lib.ptr(s), _lib.ptr(a), _lib.ptr(buf), n, t, a.shape[1], sd, a.shape[2], ridge, ld,
                   _lib.ptr(flag), stream)
    return _launch_summary(states, actions, prec, width, out, check_finite, launch)


def kme_row_dim(obs_dim, act_dim, diff=True, time=False):
    """Width d of a transition row ``[tau? | s | a | ds?]`` of ``summary_kme``: ``2 * obs_dim + act_dim`` with
    the differences, ``obs_dim + act_dim`` without, one more with the time column -- without touching the GPU
    (bsig_kme_row_dim, include/bsig_kme.h).  ValueError for a dimension below 1 or a width past 2^31 - 1."""
    return _obs_act_width('transition', 'bsig_kme_row_dim', obs_dim, act_dim, 1 if diff else 0, 1 if time else 0)


def summary_kme(states, actions, embedding, out=None, check_finite=True, dtype=None, lengths=None):
    """The random-feature kernel mean embedding of the trajectories' transitions (not in the reference): with
    the rows ``x_t = [tau_t? | s_t | a_t | s_(t+1) - s_t]``, M of them, the actions padded as
    ``pad_states_actions`` leaves them, and ``z_t = coeff x_t``, the row is
    ``[a/M sum_t cos z_t | a/M sum_t sin z_t]``: ``embedding.n_feat`` numbers from the whole trajectory,
    whatever its length and dimensions (include/bsig_kme.h, csrc/kme.h).  ``embedding`` is a
    ``kme.KernelMeanEmbedding``: the frequencies, the per-column scale and the row's layout.

    ``lengths``: as ``summary_xcorr``'s (include/bsig_ragged.h): row n is, bit for bit, the row of the one
    trajectory sliced to its ``L_n`` valid states; ``None``: the call it always was.

    ``out=``, ``check_finite`` and ``dtype=torch.float64`` are ``cross_correlation``'s.  RuntimeError while the
    embedding has no scale; NotImplementedError when a block of rows does not fit a workgroup's LDS."""
    if lengths is None:
        return embedding(states, actions, out=out, check_finite=check_finite, dtype=dtype)
    return embedding(states, actions, out=out, check_finite=check_finite, dtype=dtype, lengths=lengths)


def signature_depth(ndim):
    """Reference summarizers.py:133-141."""
    max_output_dim = 110 ** 2
    for depth in reversed(range(4)):
        if ndim ** depth <= max_output_dim:
            return depth
    return 1


def signature_dim(path_dim, depth):
    """Width of a signature row, ``sum(path_dim ** k for k in 1..depth)``, without touching the GPU
    (bsig_signature_ex_dim, include/bsig_signature.h).  ValueError for ``path_dim < 2``, a depth outside
    1..6 or a width past 2^31 - 1."""
    width = int(_lib.load().bsig_signature_ex_dim(int(path_dim), int(depth)))
    if width < 0:
        raise ValueError('no signature row for path_dim=%r, depth=%r (path_dim >= 2, depth in 1..%d, width '
                         'below 2^31)' % (path_dim, depth, _lib.SIGNATURE_MAX_DEPTH))
    return width


def signature_channels(channels, sd, ad):
    """``channels`` of summary_signatory as a tuple of ints, checked on the host (the library cannot
    range-check a device array): ValueError if it is empty, not integers, or out of ``[0, sd + ad)``."""
    try:
        picked = tuple(operator.index(c) for c in channels)
    except TypeError:
        raise ValueError('channels must be a sequence of ints, got %r' % (channels,)) from None
    if not picked:
        raise ValueError('channels is empty: pick at least one of the %d channels' % (sd + ad))
    for c in picked:
        if not 0 <= c < sd + ad:
            raise ValueError('channel %d is out of [0, %d): %d state and %d action channels'
                             % (c, sd + ad, sd, ad))
    return picked


_channel_vectors = {}      # (picked channels, device) -> their int32 vector on that device


def _channel_vector(picked, device):
    """The index vector of a channel list on ``device``: uploaded once per distinct list."""
    key = (picked, str(device))
    vec = _channel_vectors.get(key)
    if vec is None:
        vec = _channel_vectors[key] = torch.tensor(picked, dtype=torch.int32).to(device)
    return vec


def _signature_args(states, actions, depth, dtype, channels):
    """What summary_signatory and summary_logsignature do with their arguments: the host checks (asserts, then
    ValueErrors, all before any GPU call), the path and its default depth: (prec, picked, path_dim, depth)."""
    prec = _precision(dtype)
    assert len(states.shape) == 3, 'states should be batch x time x state_dim'
    assert len(actions.shape) == 3, 'Need actions: ntraj x n_steps x state_dim'
    picked = None if channels is None else signature_channels(channels, states.shape[2], actions.shape[2])
    if depth is not None and depth > _lib.SIGNATURE_MAX_DEPTH:
        raise ValueError('depth %r is above %d' % (depth, _lib.SIGNATURE_MAX_DEPTH))
    path_dim = 1 + (states.shape[2] + actions.shape[2] if picked is None else len(picked))
    if depth is None:
        depth = signature_depth(path_dim)
    return prec, picked, path_dim, depth


def summary_signatory(states, actions, depth=None, out=None, dtype=None, channels=None):
    """Reference summarizers.py:144-168 with the signature computed by
    csrc/summarizers.hip instead of ``signatory``.  All N rows are returned
    (the reference drops N % 10 rows when N > 10000).

    ``depth`` up to 6 and ``channels`` (include/bsig_signature.h): ``channels`` is a sequence of ints
    that picks the path's columns after the time channel -- ``c < sd`` is ``states[..., c]``, any other
    ``actions[..., c - sd]``; any order, repeats allowed -- so the path is ``[t | picked channels]`` and
    the default depth is ``signature_depth(1 + len(channels))``.  The channels are gathered by the
    kernel's loader: no sliced copy of the trajectories is made.  ``channels=None`` at depth <= 3 is the
    call it always was (signature3_kernel / signature12_kernel); anything else, the identity list
    included, runs the general kernel of csrc/signature_ex.h.  ValueError (before any GPU call) for a
    bad channel list or a depth above 6; NotImplementedError when the levels do not fit a workgroup's LDS."""
    prec, picked, path_dim, depth = _signature_args(states, actions, depth, dtype, channels)
    general = not (picked is None and depth <= 3)      # the kernel of csrc/signature_ex.h

    def width(s, a):
        assert a.shape[1] == s.shape[1]
        if general:
            return signature_dim(path_dim, depth)
        return summary_dim('summary_signatory', s.shape[1], s.shape[2], a.shape[2], depth)

    def launch(s, a, buf, ld, flag, stream):
        tail = (_lib.ptr(buf), s.shape[0], s.shape[1], s.shape[2], a.shape[2], depth, ld, stream)
        if general:
            vec = None if picked is None else _channel_vector(picked, s.device)
            prec.signature_ex(_lib.ptr(s), _lib.ptr(a), _lib.ptr(vec), len(picked or ()), *tail)
        else:
            prec.signature(_lib.ptr(s), _lib.ptr(a), *tail)
    return _launch_summary(states, actions, prec, width, out, False, launch)


def logsignature_dim(path_dim, depth):
    """Width of a log-signature row: the number of Lyndon words of length 1..depth over ``path_dim`` letters
    (Witt's formula), without touching the GPU (bsig_logsignature_dim, include/bsig_logsignature.h).
    ValueError where ``signature_dim`` raises it."""
    width = int(_lib.load().bsig_logsignature_dim(int(path_dim), int(depth)))
    if width < 0:
        raise ValueError('no log-signature row for path_dim=%r, depth=%r (path_dim >= 2, depth in 1..%d, '
                         'signature width below 2^31)' % (path_dim, depth, _lib.SIGNATURE_MAX_DEPTH))
    return width


_word_offsets = {}         # (path_dim, depth) -> the library's offset table, a tuple of ints
_word_vectors = {}         # (path_dim, depth, device) -> the table as an int32 vector on that device


def _lyndon_offsets(path_dim, depth):
    """bsig_logsignature_words: per output element, the flat offset of its word in the signature row."""
    key = (int(path_dim), int(depth))
    table = _word_offsets.get(key)
    if table is None:
        width = logsignature_dim(*key)
        buf = (C.c_int32 * width)()
        _lib.check(_lib.load().bsig_logsignature_words(key[0], key[1], buf, width))
        table = _word_offsets[key] = tuple(buf)
    return table


def lyndon_words(path_dim, depth):
    """The Lyndon words of length 1..depth over the letters ``0 < 1 < ... < path_dim - 1`` (0: the time
    channel) as tuples of letters, in the order of a ``summary_logsignature`` row: by length, then
    lexicographically.  Read off the offsets the library hands the kernel, not made a second time."""
    words, base, k = [], 0, 1
    for at in _lyndon_offsets(path_dim, depth):
        while at >= base + path_dim ** k:
            base += path_dim ** k
            k += 1
        rem, letters = at - base, []
        for _ in range(k):
            rem, letter = divmod(rem, path_dim)
            letters.append(letter)
        words.append(tuple(reversed(letters)))
    return words


def _word_vector(path_dim, depth, device):
    """The offset table of (path_dim, depth) on ``device``: uploaded once."""
    key = (int(path_dim), int(depth), str(device))
    vec = _word_vectors.get(key)
    if vec is None:
        vec = _word_vectors[key] = torch.tensor(_lyndon_offsets(path_dim, depth), dtype=torch.int32).to(device)
    return vec


def summary_logsignature(states, actions, depth=None, out=None, dtype=None, channels=None):
    """The log-signature of the path ``[t | picked channels]`` at the Lyndon words -- ``signatory``'s
    ``logsignature(path, depth, mode="words")`` -- by an epilogue on the general signature kernel
    (include/bsig_logsignature.h, csrc/logsignature.h): ``logsignature_dim(d, depth)`` coordinates that
    determine the ``signature_dim(d, depth)`` terms of ``summary_signatory``, in the order of
    ``lyndon_words(d, depth)``.  The signature itself is never written to memory.

    Arguments, checks, default depth (``signature_depth(d)``), ``out=``, ``dtype=torch.float64`` and errors
    are those of ``summary_signatory``.  Depth 1 is the signature's level 1; every other call, whatever
    ``channels``, runs the log-signature kernel.  In fp32 the log cancels: see the README for the error
    relative to the value at depth 6; ``dtype=torch.float64`` is the remedy."""
    prec, picked, path_dim, depth = _signature_args(states, actions, depth, dtype, channels)

    def width(s, a):
        assert a.shape[1] == s.shape[1]
        return logsignature_dim(path_dim, depth)

    def launch(s, a, buf, ld, flag, stream):
        n, length, sd = s.shape
        vec = None if picked is None else _channel_vector(picked, s.device)
        words = None if depth == 1 else _word_vector(path_dim, depth, s.device)
        prec.logsignature(
            _lib.ptr(s), _lib.ptr(a), _lib.ptr(vec), len(picked or ()), _lib.ptr(words), _lib.ptr(buf), n, length,
            sd, a.shape[2], depth, ld, stream)
    return _launch_summary(states, actions, prec, width, out, False, launch)
