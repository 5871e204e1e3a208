"""The random-feature kernel mean embedding of a trajectory's transitions (include/bsig_kme.h, csrc/kme.h): the
summary ``(1/M) sum_t phi(x_t)`` with random Fourier features ``phi`` of the rows
``x_t = [tau_t? | s_t | a_t | s_(t+1) - s_t]`` -- ``n_feat`` numbers whatever the task's dimensions and
length, made from every step.  Not in the reference.

``KernelMeanEmbedding`` holds what the summary depends on beside the trajectories: the frequencies (drawn
once, from a generator of their own) and the per-column scale ``inv_std`` (made once on the device from sample
trajectories, or given).  The coefficients the kernel reads, ``freqs * inv_std / (scale sqrt(d))``, follow from
both on the device; nothing is read back.
"""
import math
import operator

import numpy as np
import torch

from . import _lib
from . import summarizers as _summ
from .frozen import FrozenStatistic, column_statistics


def _flag(value, name):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError('%s must be a bool, got %r' % (name, value))
    return bool(value)


def check_features(n_feat, name='n_feat'):
    """``n_feat`` as an int: even and >= 2 (a cosine and a sine per frequency); ValueError otherwise."""
    if isinstance(n_feat, bool):
        raise ValueError('%s must be an even int >= 2, got %r' % (name, n_feat))
    try:
        n = operator.index(n_feat)
    except TypeError:
        raise ValueError('%s must be an even int >= 2, got %r' % (name, n_feat)) from None
    if n < 2 or n % 2 or n > 2 ** 30:
        raise ValueError('%s must be an even int >= 2, got %r' % (name, n_feat))
    return n


def check_scale(scale, name='scale'):
    """``scale`` as a float: positive and finite; ValueError otherwise."""
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating)) or \
            not (np.isfinite(scale) and scale > 0):
        raise ValueError('%s must be a positive float, got %r' % (name, scale))
    return float(scale)


class KernelMeanEmbedding(FrozenStatistic):
    """``emb(states, actions)`` -> ``[N, n_feat]``: ``[a/M sum_t cos z_t | a/M sum_t sin z_t]`` with
    ``z_t,j = sum_k x_t,k coeff_j,k``, ``a = sqrt(2 / n_feat)``, ``coeff = freqs * inv_std / (scale sqrt(d))``.

    Buffers: ``freqs`` (fp32 ``[n_feat / 2, d]``: ``np.random.RandomState(seed).standard_normal`` rounded to
    fp32 -- the global numpy and torch generators are not touched -- or the given ``freqs``), ``inv_std``
    (float64 ``[d]``: the reciprocal standard deviation of every column of ``x``, 0 for a flat column, which then
    drops out of every ``z``) and ``count`` (the trajectories the scale was made from).  Device, dtypes and
    ``ready`` are FrozenStatistic's.

    ``diff=False`` leaves the state differences out of the rows, ``time=True`` puts the step's position in
    [0, 1] in front.  ``scale`` multiplies the bandwidth of every column (its standard deviation times
    ``sqrt(d)``)."""
    MAX_SCALE_TRAJECTORIES = 256      # fit_scale takes the first ones: their rows are written out for the statistics
    NOT_READY = ('the scale of this kernel mean embedding does not exist yet: BayesSim.fit / '
                 'run_training make it from their first training trajectories; or call fit_scale '
                 '/ set_scale / load_state_dict first')
    NOT_READY_PARALLEL = ("a data-parallel model on 'summary_kme' needs the embedding's scale before the fit "
                          '(every rank would make it from its own first chunk): call fit_embedding_scale, '
                          'bs.embedding.set_scale or bs.embedding.load_state_dict with the same values on '
                          'every rank first')

    def __init__(self, obs_dim, act_dim, n_feat=256, scale=1.0, seed=0, diff=True, time=False, freqs=None,
                 device='cpu'):
        n_feat, scale = check_features(n_feat), check_scale(scale)
        diff, time = _flag(diff, 'diff'), _flag(time, 'time')
        m, d = n_feat // 2, _summ.kme_row_dim(int(obs_dim), int(act_dim), diff, time)
        if freqs is None:
            draw = np.random.RandomState(seed).standard_normal((m, d)).astype(np.float32)
        else:
            draw = np.asarray(torch.as_tensor(freqs).detach().cpu().numpy(), dtype=np.float32)
            if draw.shape != (m, d):
                raise ValueError('freqs must be [n_feat / 2, d] = [%d, %d], got %r' % (m, d, tuple(draw.shape)))
        super().__init__(device, freqs=torch.from_numpy(np.ascontiguousarray(draw)),
                         inv_std=torch.ones(d, dtype=torch.float64))
        self.n_feat, self.scale, self.seed, self.diff, self.time = n_feat, scale, seed, diff, time
        self.obs_dim, self.act_dim, self.row_dim = int(obs_dim), int(act_dim), d
        self._coeff = {}                  # itemsize -> the coefficient rows [m, ld] of the current scale

    def _apply(self, fn, *args, **kwargs):
        self._coeff = {}
        return super()._apply(fn, *args, **kwargs)

    def _value_changed(self):
        self._coeff = {}

    def _on_gpu(self):
        _lib.require_gpu()
        if not self.freqs.is_cuda:
            raise RuntimeError('a KernelMeanEmbedding computes on the GPU: build it with device= a GPU or move '
                               'it there (no CPU fallback)')
        return self.freqs.device

    def rows(self, states, actions, dtype=None, lengths=None):
        """The rows ``x_t`` of the trajectories as ``[N * M, d]`` device rows (bsig_kme_rows): what the scale's
        statistics are made from; never on the fit path.  ``lengths`` (``summarizers.check_lengths``): the valid
        rows only, compacted, ``[sum_n M_n, d]``, trajectory after trajectory (bsig_kme_rows_ragged); their
        offsets and their number are made on the host, so lengths that live on the device are READ BACK here
        (4 bytes a trajectory; one outside the range counts as the nearest inside, as in the kernel)."""
        prec = _summ._precision(dtype)
        if lengths is not None:
            return self._valid_rows(states, actions, prec, lengths)
        dev = self._on_gpu()
        with _lib.device_stream(dev) as stream:
            s, a, _ = _summ._prep(states, actions, prec, dev)
            n, ts, sd = s.shape
            assert (sd, a.shape[2]) == (self.obs_dim, self.act_dim), 'trajectories of other dimensions'
            steps = ts - (1 if self.diff else 0)
            assert steps >= 1, 'Need %d states or more' % (2 if self.diff else 1)
            ld = _lib.round_up(self.row_dim, 16 // prec.itemsize)
            buf = torch.empty((n * steps, ld), dtype=prec.dtype, device=dev)
            prec.kme_rows(_lib.ptr(s), _lib.ptr(a), _lib.ptr(buf), n, ts, a.shape[1], sd, a.shape[2],
                          int(self.diff), int(self.time), ld, stream)
        return buf[:, :self.row_dim]

    def _valid_rows(self, states, actions, prec, lengths):
        assert len(states.shape) == 3 and len(actions.shape) == 3, 'Need trajectories: ntraj x n_steps x dim'
        n, ts = int(states.shape[0]), int(states.shape[1])
        lengths = _summ.check_lengths(lengths, n, ts, self.diff)
        if lengths.is_cuda:
            # the one read-back: the offsets and the number of rows are host arithmetic.  A length outside the
            # range is clamped as the kernel clamps it: the summaries' NaN row and finite flag report it
            lengths = lengths.cpu().clamp(min=2 if self.diff else 1, max=ts)
        steps = lengths.to(torch.int64) - (1 if self.diff else 0)
        offsets = torch.cumsum(steps, 0) - steps
        total = int(steps.sum())
        dev = self._on_gpu()
        with _lib.device_stream(dev) as stream:
            s, a, _ = _summ._prep(states, actions, prec, dev)
            sd = s.shape[2]
            assert (sd, a.shape[2]) == (self.obs_dim, self.act_dim), 'trajectories of other dimensions'
            ld = _lib.round_up(self.row_dim, 16 // prec.itemsize)
            buf = torch.empty((total, ld), dtype=prec.dtype, device=dev)
            lens, offs = _summ._lengths_on(lengths, dev), offsets.to(dev)
            prec.kme_rows_ragged(_lib.ptr(s), _lib.ptr(a), _lib.ptr(lens), _lib.ptr(offs), _lib.ptr(buf), n, ts,
                                 a.shape[1], sd, a.shape[2], int(self.diff), int(self.time), ld, stream)
        return buf[:, :self.row_dim]

    def fit_scale(self, states, actions, dtype=None, lengths=None):
        """``inv_std`` <- the reciprocal standard deviation of every column of the rows ``x_t`` of the given
        trajectories (the first MAX_SCALE_TRAJECTORIES at most; bsig_kme_rows, then bsig_input_norm_stats:
        the flat rule of include/bsig_input_norm.h), in ``dtype`` (fp32 rows by default), frozen from here on.
        Asynchronous: nothing is read back, ``count`` is written on the stream.

        ``lengths``: the statistics are made from the VALID rows only (bsig_kme_rows_ragged into compacted rows,
        then the same statistics).  The rows' offsets and their number come from the first
        MAX_SCALE_TRAJECTORIES lengths on the host: lengths that live on the device cost ONE read-back of at
        most 1 KB, once per embedding -- the only read-back lengths add anywhere; lengths on the host add
        none."""
        n = min(int(states.shape[0]), self.MAX_SCALE_TRAJECTORIES)
        assert n >= 1, 'the scale needs at least one trajectory'
        prec = _summ._precision(dtype)
        if lengths is not None:
            lengths = _summ.check_lengths(lengths, int(states.shape[0]), int(states.shape[1]), self.diff)[:n]
        x = self.rows(states[:n], actions[:n], dtype, lengths=lengths)
        dev = x.device
        with _lib.device_stream(dev):      # (column_statistics launches on the current device's stream)
            mean = torch.empty(self.row_dim, dtype=torch.float64, device=dev)
            column_statistics(prec, x, x.stride(0), x.shape[0], self.row_dim, mean, self.inv_std,
                              lambda numel: torch.empty(numel, dtype=torch.float64, device=dev))
            self.made_from(n)
        return self

    def set_scale(self, inv_std, count=1):
        """The host-given form of ``fit_scale``: ``inv_std`` ``[d]``, finite and >= 0 (0: the column drops
        out).  ``count``: the trajectories behind it where known (any positive number: ready)."""
        inv = np.asarray(torch.as_tensor(inv_std).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        if inv.shape != (self.row_dim,):
            raise ValueError('set_scale: inv_std must hold %d values' % self.row_dim)
        if not (np.isfinite(inv).all() and (inv >= 0).all()) or int(count) < 1:
            raise ValueError('set_scale: inv_std must be finite and >= 0, and count >= 1')
        self.inv_std.copy_(torch.from_numpy(inv))
        self.made_from(int(count))
        return self

    @property
    def kappa(self):
        """1 / (scale sqrt(d)), in double: the factor of every coefficient beside ``inv_std``."""
        return 1.0 / (self.scale * math.sqrt(float(self.row_dim)))

    def coefficients(self, dtype=None):
        """The coefficient rows ``[n_feat / 2, d]`` of the current scale in ``dtype`` (bsig_kme_coeff): made on
        the device on first use, kept until the scale changes."""
        prec = _summ._precision(dtype)
        self.require_ready()
        dev = self._on_gpu()
        if prec.itemsize not in self._coeff:
            m, d = self.n_feat // 2, self.row_dim
            ld = _lib.round_up(d, 16 // prec.itemsize)
            buf = torch.empty((m, ld), dtype=prec.dtype, device=dev)
            with _lib.device_stream(dev) as stream:
                prec.kme_coeff(_lib.ptr(self.freqs), d, _lib.ptr(self.inv_std), self.kappa, _lib.ptr(buf), ld, m,
                               d, stream)
            self._coeff[prec.itemsize] = buf
        return self._coeff[prec.itemsize][:, :self.row_dim]

    def forward(self, states, actions, out=None, check_finite=True, dtype=None, lengths=None):
        """The embedding rows ``[N, n_feat]``.  ``out=``, ``check_finite`` and ``dtype=torch.float64`` are
        ``cross_correlation``'s.  RuntimeError before the scale exists; NotImplementedError when a block of
        rows does not fit a workgroup's LDS.  ``lengths`` (``summarizers.check_lengths``,
        include/bsig_ragged.h): the valid states of every trajectory -- row n is, bit for bit, the row of the
        one trajectory sliced to them; lengths on the device are never read back here (one outside the range
        makes its row NaN and fails the finite check); ``None``: the call it always was."""
        prec = _summ._precision(dtype)
        self.require_ready()
        _summ._need_trajectories(states, actions)
        assert (states.shape[2], actions.shape[2]) == (self.obs_dim, self.act_dim), \
            'trajectories of other dimensions'
        steps = states.shape[1] - (1 if self.diff else 0)
        assert steps >= 1, 'Need %d states or more' % (2 if self.diff else 1)
        if lengths is not None:
            lengths = _summ.check_lengths(lengths, int(states.shape[0]), int(states.shape[1]), self.diff)
        dev = self._on_gpu()

        def launch(s, a, buf, ld, flag, stream):
            coeff = self.coefficients(dtype)
            tail = (_lib.ptr(coeff), coeff.stride(0), _lib.ptr(buf), s.shape[0], s.shape[1], a.shape[1], s.shape[2],
                    a.shape[2], self.n_feat // 2, int(self.diff), int(self.time), ld, _lib.ptr(flag), stream)
            if lengths is None:
                prec.kme(_lib.ptr(s), _lib.ptr(a), *tail)
            else:
                lens = _summ._lengths_on(lengths, dev)
                prec.kme_ragged(_lib.ptr(s), _lib.ptr(a), _lib.ptr(lens), *tail)
        return _summ._launch_summary(states, actions, prec, self.n_feat, out, check_finite, launch, device=dev)
