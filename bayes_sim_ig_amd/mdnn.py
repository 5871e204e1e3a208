"""Mixture Density NN estimator on MI355X — mirror of the reference's
bayes_sim_ig/models/mdnn.py (class MDNN: same constructor keywords, methods,
attributes, ``state_dict`` keys and error behaviour).

All arithmetic runs in libbsig_hip (csrc/): the parameters live in ONE flat
fp32 device buffer (the named ``nn.Parameter``s are views into it, so
``state_dict`` / ``load_state_dict`` keep working), the trunk / head products
are fp32-MFMA GEMMs, the mixture head + NLL + backward is one fused kernel,
Adam runs over the flat buffer, and ``run_training`` replays the whole update
from a HIP graph (csrc/estimator.hip).  There is no CPU fallback.

``model.double()`` switches the model to the fp64 mode (include/bsig_f64.h, csrc/f64/): the flat
buffers become float64 -- the reference under ``torch.set_default_dtype(torch.float64)``;
``model.float()`` goes back.  Every entry point below is written once: which library functions, struct
and sizes it uses comes from ``self._prec``, one of ``_lib.F32`` / ``_lib.F64``, and nowhere else.

``model.set_matmul_precision('split_bf16')`` (include/bsig_matmul.h; the process default comes from the
environment variable BSIG_MATMUL_PRECISION, read when a model is constructed) lets the fit plan's products
run on the bf16 matrix pipes with every fp32 operand split into three bf16 pieces: fp32-grade results that
are not bitwise the reference's fp32 arithmetic.  The default, 'float32', is.

``MDNN(..., input_norm=True)`` (not in the reference, which normalises the targets only) adds a standardisation
of the summaries to the model: per-column mean and reciprocal standard deviation (include/bsig_input_norm.h),
made once on the device, kept in ``state_dict`` and applied by every entry point that takes summaries.

``MDRFF(..., sigma='median')`` (not in the reference either) sets the feature map's bandwidth by the median
heuristic (include/bsig_rff_bandwidth.h): one double on the device, made once from the first training rows as
the estimator sees them, frozen, kept in ``state_dict``; the section "kernel bandwidth" below is its plumbing.
"""
import contextlib
import ctypes as C
import functools
import os
import warnings
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import pdf
from . import dp as _dp
from .frozen import FrozenStatistic, column_statistics
from .protocol import eval_updates, split_rows
from .summarizers import CrossCorrFactors

_ACT_CODES = {nn.Tanh: _lib.ACT_TANH, nn.ReLU: _lib.ACT_RELU,
              nn.LeakyReLU: _lib.ACT_LEAKY_RELU, nn.Sigmoid: _lib.ACT_SIGMOID,
              nn.Identity: _lib.ACT_IDENTITY}


def _on_model_device(fn):
    """Run a method with the model's GPU as the current HIP device and its torch stream
    as the launch stream (a model built with device='cuda:1' must not launch on cuda:0)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        flat = getattr(self, '_flat', None)
        if flat is None or not flat.is_cuda or flat.device.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with _lib.on_device(flat.device):
            return fn(self, *args, **kwargs)
    return wrapped


class PersistentTimeout(RuntimeError):
    """A bounded cross-workgroup poll of a persistent update kernel gave up: its workgroups (one
    per CU) were not all resident -- the GPU is shared or partitioned.  The call's parameters and
    Adam moments are partially updated; MDNN.run_training / BayesSim.fit catch this, restore the
    state they saved at the start and repeat the work on the per-phase kernels."""


class _BlockLogs:
    """The packed logs of every chunk of a block launch: read back ONCE, by the first chunk that asks."""

    def __init__(self, packed):
        self.packed, self._host = packed, None

    def row(self, c):
        if self._host is None:
            self._host = self.packed.cpu().tolist()
        return self._host[c]


class PendingLogs:
    """The 6+6 losses and the non-finite flag of one run_training call, still on
    the device; ``result()`` is the call's single host read-back.  BayesSim.fit
    defers it to the end of the chunk loop so the GPU never waits for the host."""

    def __init__(self, packed, n_e, n_test, verbose, dp=None, block=None):
        self.packed, self.n_e, self.n_test, self.verbose = packed, n_e, n_test, verbose
        self.dp = dp      # (eval_its, n_updates, world): `packed` is bsig_fit_run_dp's reduced_logs
        self.block = block   # (_BlockLogs, chunk): a chunk of a block launch, whose chunks share one read-back

    def result(self):
        host = self.block[0].row(self.block[1]) if self.block is not None else self.packed.cpu().tolist()
        n_e = self.n_e
        if self.dp is not None:
            eval_its, n_updates, world = self.dp
            train_list = [host[it] / world for it in eval_its]
            n_test_all = host[n_updates + n_e]
            test_list = [v / max(n_test_all, 1.0) for v in host[n_updates:n_updates + n_e]]
            bad = ((_lib.FLAG_NONFINITE if host[n_updates + n_e + 1] > 0 else 0) |
                   (_lib.FLAG_TIMEOUT if host[n_updates + n_e + 2] > 0 else 0))
            self.n_test = int(n_test_all)
        else:
            train_list, test_list, bad = host[:n_e], host[n_e:2 * n_e], host[2 * n_e]
        if int(bad) & _lib.FLAG_TIMEOUT:      # a bounded cross-workgroup poll of the persistent kernel gave up
            raise PersistentTimeout('persistent update kernel timed out waiting for another workgroup: its '
                                    'workgroups (one per CU) were not all resident -- is the GPU shared with '
                                    'another process or partitioned?  The parameters and Adam moments of this '
                                    'call are partially updated; set BSIG_NO_PERSISTENT=1 to use the '
                                    'per-phase kernels')
        assert bad == 0, 'non-finite value in forward / loss (mdnn.py:120-124,162-174)'
        if self.n_test == 0:
            test_list = [float('nan')] * n_e   # mean over an empty test split
        if self.verbose:
            for a, b in zip(train_list, test_list):
                print(f'loss: train {a:0.4f} test {b:0.4f}')
        return {'train_loss': train_list, 'test_loss': test_list}


class _FusedNLL(torch.autograd.Function):
    """Autograd node behind ``mdn_loss_fn(*model(x), y)``: the value is the
    loss already computed; backward runs the fused HIP forward+NLL+backward
    (bsig_mdn_loss_grad) into a scratch flat buffer and hands autograd one
    gradient per parameter, so ``loss.backward(); optimizer.step()`` behaves as
    in the reference (mdnn.py:231-234)."""

    @staticmethod
    def forward(ctx, loss_value, model, x, y, noise, seed, *params):
        ctx.model, ctx.x, ctx.y, ctx.noise, ctx.seed = model, x, y, noise, seed
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        m = ctx.model
        tmp = torch.empty_like(m._flat_grad)
        m.loss_and_grad(ctx.x, ctx.y, noise=ctx.noise, seed=ctx.seed, grads_out=tmp)
        grads = [tmp[o:o + int(np.prod(full))].view(full)[tuple(slice(0, d) for d in shape)] * grad_out
                 for o, full, shape in m._param_slices]
        return (None, None, None, None, None, None, *grads)


def _flat_rule(mean, std, dtype):
    """inv_std of include/bsig_input_norm.h from host-given statistics: 0 where std <= 8 u |mean| (u: the unit
    roundoff of the rows' type ``dtype``), else 1 / std.  float64 numpy in and out."""
    u = 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23
    flat = std <= 8.0 * u * np.abs(mean)
    with np.errstate(divide='ignore'):
        return np.where(flat, 0.0, 1.0 / np.where(flat, 1.0, std))


class InputNorm(FrozenStatistic):
    """The statistics of a model built with ``input_norm=True``: ``mean`` and ``inv_std`` (float64
    [input_dim]: include/bsig_input_norm.h) and ``count`` (the number of rows they were made from).  Device,
    dtypes and ``ready`` are FrozenStatistic's."""
    NOT_READY = ('the input statistics of this model do not exist yet: run_training makes them '
                 'from its first training rows; or call fit_input_norm / set_input_norm / '
                 'load_state_dict first')
    NOT_READY_PARALLEL = ('a data-parallel model with input_norm needs its input statistics before '
                          'run_training (every rank would fit them on its own first chunk): call '
                          'fit_input_norm or set_input_norm with the same values on every rank first')

    def __init__(self, width, device):
        super().__init__(device, mean=torch.zeros(int(width), dtype=torch.float64),
                         inv_std=torch.ones(int(width), dtype=torch.float64))
        self.width = int(width)


class RffBandwidth(FrozenStatistic):
    """The bandwidth of an ``MDRFF(sigma='median')``: ``sigma`` (float64 scalar: ``scale`` times the median
    pairwise distance of the rows it was made from, include/bsig_rff_bandwidth.h) and ``count`` (the number of
    those rows).  Device, dtypes and ``ready`` are FrozenStatistic's.  ``version`` counts the times the value
    was given or loaded: what was derived from an earlier one (freqs / sigma) is stale."""
    NOT_READY = ("the kernel bandwidth of this model (sigma='median') does not exist yet: "
                 'run_training / BayesSim.fit make it from their first training rows; or call '
                 'fit_rff_bandwidth / set_rff_bandwidth / load_state_dict first')
    NOT_READY_PARALLEL = ("a data-parallel model with sigma='median' needs its bandwidth before run_training "
                          '(every rank would fit it on its own first chunk): call fit_rff_bandwidth or '
                          'set_rff_bandwidth with the same value on every rank first')

    def __init__(self, scale, device):
        super().__init__(device, sigma=torch.ones((), dtype=torch.float64))
        self.scale = float(scale)
        self.version = 0

    def _value_changed(self):
        self.version += 1


class MDNN(nn.Module):
    LL_LIMIT = 1.0e5     # limit log likelihood to avoid large gradients
    MIN_WEIGHT = 1.0e-5  # minimum component weights to enable updates
    EPS_NOISE = 1.e-5    # small noise e.g. for numerical stability
    VERBOSE = True       # print the 6 train/test losses per call like the reference
    USE_GRAPH = True     # replay the update from a HIP graph
    PAD_TRUNK_TO = 128   # hidden width the persistent update kernel is built for
    rff = None           # the feature map of an MDRFF
    _dtype = torch.float32   # torch.float64 after .double(): the fp64 mode
    _plan = None         # (a model whose construction failed is still finalised: __del__)
    _plan_prec = None    # the _lib.Precision that created _plan: the one that may destroy it
    _matmul = 'float32'  # matmul precision of the fit plan's products (set_matmul_precision)
    _matmul_set = False  # ... chosen by set_matmul_precision (else: the process default of BSIG_MATMUL_PRECISION)

    def __init__(self, input_dim, output_dim, output_lows, output_highs,
                 n_gaussians, full_covariance, hidden_layers, activation, lr,
                 device='cpu', **kwargs):
        """Same arguments as the reference (mdnn.py:26-52).  ``device`` must
        name a GPU for anything beyond construction.  ``input_norm=True`` (a keyword of ``**kwargs``, default
        False): the model standardises its summaries (``fit_input_norm``)."""
        super(MDNN, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.output_lows = None
        self.output_highs = None
        if output_lows is not None:
            self.output_lows = torch.from_numpy(np.asarray(output_lows)).float().to(device)
            self.output_highs = torch.from_numpy(np.asarray(output_highs)).float().to(device)
        self.n_gaussians = n_gaussians
        self.activation = activation
        self.lr = lr
        self.device = device
        if activation not in _ACT_CODES:
            raise NotImplementedError('activation %r has no HIP epilogue' % (activation,))
        # Same submodules, created in the same order on the CPU so that the
        # torch-RNG initialisation matches the reference bit for bit
        # (mdnn.py:68-86), then flattened onto the device.
        net = OrderedDict()
        width = input_dim
        for l, layer_size in enumerate(hidden_layers):
            net['fcon%d' % l] = nn.Linear(width, layer_size)
            net['nl%d' % l] = activation()
            width = layer_size
        self.net = nn.Sequential(net) if len(hidden_layers) > 0 else None
        self.pi = nn.Linear(width, n_gaussians)
        self.mu = nn.Linear(width, output_dim * n_gaussians)
        self.Diag = nn.Sequential(nn.Linear(width, output_dim * n_gaussians))
        self.Lower = None
        self.L_size = int(0.5 * output_dim * (output_dim - 1))
        if self.L_size > 0 and full_covariance:
            self.Lower = nn.Linear(width, self.L_size * n_gaussians)
        self._hidden = [int(h) for h in hidden_layers]
        # A two-layer tanh trunk narrower than 128 is STORED zero-padded to [128, 128] (the
        # parameters are views of the leading blocks): the padding units see zero weights, put
        # out tanh(0) = 0 and receive exactly zero gradients, so Adam leaves them at zero and
        # the network is the reference's bit for bit -- and the persistent update kernel, which
        # is built for the reference's default [128, 128] trunk, covers it (the reference's own
        # tests/regression_tests.py:59 uses (24, 24)).
        self._hidden_stored = list(self._hidden)
        if (len(self._hidden) == 2 and max(self._hidden) <= self.PAD_TRUNK_TO and
                min(self._hidden) >= 1 and self._hidden != [self.PAD_TRUNK_TO] * 2 and
                activation is nn.Tanh and os.environ.get('BSIG_NO_TRUNK_PAD') != '1'):
            self._hidden_stored = [self.PAD_TRUNK_TO] * 2
        self._rff_feats = int(kwargs.get('_rff_feats', 0))
        self._rff_scale = float(kwargs.get('_rff_scale', 0.0))
        self._plan = None
        self._plan_key = None
        self._bufs = {}
        self._dp = None
        # the time-out ladder (_retrying / _give_up_a_level): what this model has given up so far
        self._no_persistent = False
        self._no_block_launch = False
        self._block_launches = 0
        self._matmul = _lib.default_matmul_precision()      # (BSIG_MATMUL_PRECISION; ValueError on a bad value)
        self._flatten(device)
        # after every submodule of the reference, and nothing drawn from an RNG: the initialisation and the
        # state_dict keys of a default model are untouched
        if kwargs.get('input_norm', False):
            self.input_norm = InputNorm(kwargs.get('_input_norm_dim', input_dim), device)

    # ------------------------------------------------------------ plumbing
    def _cfg(self):
        cfg = _lib.MdnCfg()
        cfg.input_dim = int(self.input_dim)
        cfg.n_hidden = len(self._hidden)
        for i, h in enumerate(self._hidden_stored):
            cfg.hidden[i] = h
        cfg.activation = _ACT_CODES[self.activation]
        cfg.rff_feats = self._rff_feats
        cfg.rff_cos_only = 0
        cfg.rff_scale = self._rff_scale
        cfg.head.out_dim = int(self.output_dim)
        cfg.head.n_comp = int(self.n_gaussians)
        cfg.head.full_cov = 1 if self.Lower is not None else 0
        cfg.head.eps_noise = float(type(self).EPS_NOISE)
        cfg.head.min_weight = float(type(self).MIN_WEIGHT)
        cfg.head.ll_limit = float(type(self).LL_LIMIT)
        cfg.lr, cfg.beta1, cfg.beta2, cfg.adam_eps = float(self.lr), 0.9, 0.999, 1e-8
        return cfg

    def _linears(self):
        mods = [self.net[2 * l] for l in range(len(self._hidden))]
        mods += [self.pi, self.mu, self.Diag[0]]
        if self.Lower is not None:
            mods.append(self.Lower)
        return mods

    def _flatten(self, device, dtype=None):
        """Move every parameter into one flat buffer of the model's dtype (fp32, or fp64 after
        .double(); layout: bsig_mdn_param_offsets) and re-point the nn.Parameters at views.  A
        change of dtype carries the gradients and both Adam moments over; the values are widened,
        or rounded to fp32 (exact for values an fp32 holds)."""
        lib = _lib.load()
        dtype = dtype or self._dtype
        carried = [getattr(self, n, None) for n in ('_flat_grad', '_exp_avg', '_exp_avg_sq')] \
            if dtype != self._dtype else [None] * 3
        self._dtype = dtype
        cfg = self._cfg()
        total = int(lib.bsig_mdn_param_count(C.byref(cfg)))
        assert total > 0, lib.bsig_last_error().decode()
        n_off = 2 * (len(self._hidden) + 4)
        offs = (C.c_int64 * n_off)()
        _lib.check(lib.bsig_mdn_param_offsets(C.byref(cfg), offs, n_off))
        flat = torch.zeros(total, dtype=dtype, device=device)
        grads = torch.zeros(total, dtype=dtype, device=device)
        self._param_slices = []
        # stored input width of every Linear: the (possibly padded) width of the layer below
        widths = [self.input_dim if self._rff_feats == 0 else self._rff_feats] + self._hidden_stored
        with torch.no_grad():
            for i, mod in enumerate(self._linears()):
                l = min(i, len(self._hidden))            # trunk layer l, or the heads (on the last width)
                rows = self._hidden_stored[i] if i < len(self._hidden) else mod.weight.shape[0]
                for j, prm in enumerate((mod.weight, mod.bias)):
                    o = int(offs[2 * i + j])
                    full = (rows, widths[l]) if j == 0 else (rows,)
                    real = tuple(prm.shape)
                    sub = tuple(slice(0, d) for d in real)
                    self._param_slices.append((o, full, real))
                    view = flat[o:o + int(np.prod(full))].view(full)[sub]
                    view.copy_(prm.detach().to(dtype=dtype))
                    prm.data = view
                    prm.grad = grads[o:o + int(np.prod(full))].view(full)[sub]
        self._flat, self._flat_grad = flat, grads
        self._exp_avg = torch.zeros_like(flat)
        self._exp_avg_sq = torch.zeros_like(flat)
        for new, old in zip((grads, self._exp_avg, self._exp_avg_sq), carried):
            if old is not None and old.numel() == total:
                new.copy_(old.to(device=flat.device, dtype=dtype))
        if self.output_lows is not None:
            self.output_lows = self.output_lows.to(device=device, dtype=dtype)
            self.output_highs = self.output_highs.to(device=device, dtype=dtype)
        self.device = str(device) if not isinstance(device, str) else device
        self._drop_plan()

    def _apply(self, fn, *args, **kwargs):
        if self._matmul != 'float32' and fn(torch.empty(0, dtype=self._dtype)).dtype == torch.float64:
            if not self._matmul_set:
                # the process default is for fp32 models: a model that goes double leaves it behind
                self._matmul = 'float32'
                if self.rff is not None:
                    self.rff.matmul_precision = 'float32'
        if self._matmul != 'float32' and fn(torch.empty(0, dtype=self._dtype)).dtype == torch.float64:
            # refuse BEFORE converting: the model stays as it was
            raise ValueError("a model set to matmul precision %r cannot become double: the fp64 mode has one "
                             "arithmetic; set_matmul_precision('float32') first" % (self._matmul,))
        if self._dp is not None:
            # refuse BEFORE converting: the model stays as it was
            if fn(torch.empty(0, dtype=self._dtype)).dtype == torch.float64:
                self._f64_dp_error()
        super()._apply(fn, *args, **kwargs)
        prm = next(self.parameters())
        if prm.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError('the HIP estimator computes in fp32 or fp64 only')
        self._flatten(prm.device, prm.dtype)
        return self

    @property
    def _f64(self):
        return self._dtype == torch.float64

    @property
    def _prec(self):
        """The precision seam (_lib.Precision) of the model's dtype."""
        return _lib.F64 if self._f64 else _lib.F32

    @property
    def matmul_precision(self):
        """'float32' or 'split_bf16': see set_matmul_precision."""
        return self._matmul

    def set_matmul_precision(self, name):
        """'float32' (the default: the reference's fp32 arithmetic on the fp32 MFMAs, bit for bit) or
        'split_bf16': every product of the fit plan -- ``run_training`` / ``fit``: forward and backward
        passes, weight gradients with the fused Adam step, the feature cache and the held-out evaluations
        -- may run on the bf16 matrix pipes, each fp32 operand element split into three bf16 pieces and six
        of the nine piece products kept (include/bsig_matmul.h).  fp32-grade (the error against the fp64
        product is about that of an fp32 chain) and bitwise reproducible, but not bitwise the 'float32'
        results.  A plan that a persistent update kernel covers keeps that kernel, which computes in fp32.
        An MDRFF's ``rff`` follows its model in every projection it makes (``to_features``, the block
        pre-projection of ``BayesSim.fit``, ``predict_MoGs``).  ``forward``, ``loss_and_grad`` and the head
        products of ``predict_MoGs`` take no plan: they stay fp32.
        Edge behaviour of 'split_bf16': a non-finite operand element gives non-finite outputs (NaN where
        fp32 gives inf); |x| above the largest bf16 (3.39e38) becomes inf; an element below 2^-100 in
        magnitude may carry fewer than 24 bits.
        Drops the plan.  ValueError on any other value, and on a double model; ``.double()`` on a model SET
        to 'split_bf16' raises too (one that only took the process default goes back to 'float32')."""
        _lib.matmul_precision(name)
        if name != 'float32' and self._f64:
            raise ValueError('a double model has one arithmetic (include/bsig_f64.h): matmul precision %r '
                             'applies to fp32 models only' % (name,))
        self._matmul, self._matmul_set = name, True
        if self.rff is not None:
            self.rff.matmul_precision = name
        self._drop_plan()
        return self

    @staticmethod
    def _f64_dp_error():
        raise NotImplementedError('a double MDNN cannot be data-parallel: the fp64 mode has no gradient '
                                  'exchange (include/bsig_f64.h); use .float() or a single rank')

    def _check_f64_dp(self):
        if self._f64 and self._dp is not None:
            self._f64_dp_error()

    def _hyper(self):
        """The hyper-parameters as the Python floats (doubles) the reference computes with in fp64 mode."""
        cls = type(self)
        return _lib.F64Hyper(float(self.lr), 0.9, 0.999, 1e-8, float(cls.EPS_NOISE), float(cls.MIN_WEIGHT),
                             float(cls.LL_LIMIT), float(self._rff_scale))

    def _drop_plan(self, bufs=True):
        """Release the plan through the precision that created it; with ``bufs`` the call buffers too."""
        if self._plan:
            self._plan_prec.fit_destroy(self._plan)
        self._plan, self._plan_key, self._plan_prec = None, None, None
        if bufs:
            self._bufs = {}

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass

    # ---- robustness of the persistent launches: every workgroup of such a launch must be resident
    #      at once; when the GPU turns out to be shared, the bounded polls give up and the call is
    #      repeated from a snapshot on the per-phase kernels
    def _snapshot(self):
        """(parameters, Adam moments, numpy / torch RNG states) as of now."""
        return (self._flat.clone(), self._exp_avg.clone(), self._exp_avg_sq.clone(),
                np.random.get_state(), torch.get_rng_state())

    def _restore(self, snap):
        self._flat.copy_(snap[0]); self._exp_avg.copy_(snap[1]); self._exp_avg_sq.copy_(snap[2])
        np.random.set_state(snap[3]); torch.set_rng_state(snap[4])

    def _may_time_out(self):
        """Could the next call run a persistent kernel?  (Unknown before the first plan exists.)"""
        if not self._flat.is_cuda or self._no_persistent or os.environ.get('BSIG_NO_PERSISTENT') == '1':
            return False
        if self._f64:        # the fp64 mode is per-phase launches only
            return False
        return self._plan is None or bool(self._plan_prec.is_persistent(self._plan))

    def _retrying(self, fn):
        """``fn()``, the work of one run_training or one BayesSim.fit whose logs it reads itself -- repeated
        from a snapshot, one level further down (_give_up_a_level), after each of its first two time-outs;
        a third one propagates, and so does any where no persistent kernel could have run.  A data-parallel
        group does this TOGETHER: the time-out bit travels in the logs every call sums over the ranks
        (bsig_fit_run_dp) and the rank that timed out keeps enqueueing its all-reduces, so every rank reads
        the same flag in the same call, restores and repeats it with its peers."""
        if not self._may_time_out():
            return fn()
        snap = self._snapshot()
        for attempt in range(3):
            calls0 = self._dp.resident_calls() if self._dp is not None else 0
            blocks0 = self._block_launches
            try:
                return fn()
            except PersistentTimeout:
                if attempt == 2:
                    raise
                self._restore(snap)
                self._give_up_a_level(calls0, blocks0)

    def _give_up_a_level(self, resident_calls_before, block_launches_before=None):
        """After a persistent launch timed out.  A data-parallel rank that stayed resident across the
        gradient exchange in the calls since ``resident_calls_before`` first goes back to one launch per
        update (the exchange stream was not served in time: the launch itself had the chip); a model that
        ran blocks of chunks in one launch since ``block_launches_before`` first goes back to one launch per
        chunk; a time-out after that, or without either: the per-phase kernels."""
        if block_launches_before is not None and self._block_launches > block_launches_before:
            warnings.warn('bayes_sim_ig_amd: a persistent launch over a block of chunks timed out; this model '
                          'continues with one launch per chunk', RuntimeWarning, stacklevel=4)
            self._no_block_launch = True
            return
        if self._dp is not None and self._dp.resident_calls() > resident_calls_before:
            warnings.warn('bayes_sim_ig_amd: a data-parallel launch that stays resident across the gradient '
                          'exchange timed out waiting for the exchange; this model continues with one launch '
                          'per update', RuntimeWarning, stacklevel=4)
            self._dp.set_resident(False)
            return
        self._disable_persistent()

    def _disable_persistent(self):
        """From now on this model's plans use the per-phase kernels."""
        warnings.warn('bayes_sim_ig_amd: a persistent update launch timed out waiting for another workgroup '
                      '(GPU shared with another process?); this model continues on the per-phase kernels, '
                      'which are slower', RuntimeWarning, stacklevel=4)
        self._no_persistent = True
        self._drop_plan()

    def _gpu(self):
        lib = _lib.require_gpu()
        if not self._flat.is_cuda:
            raise RuntimeError("MDNN was built with device=%r: the estimator runs on "
                               "MI355X only, construct it with device='cuda:N' "
                               "(no CPU fallback)" % (self.device,))
        return lib

    def _buf(self, name, numel, dtype=None):
        dtype = dtype or self._dtype
        t = self._bufs.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=self._flat.device)
            self._bufs[name] = t
        return t

    def _rff_args(self):
        return None, 0, None   # (coeff, ld_coeff, offset); MDRFF overrides

    def _seed(self):
        """A fresh Philox seed drawn from torch's global RNG (the reference
        consumes the torch RNG for rand_like, mdnn.py:116)."""
        if type(self).EPS_NOISE == 0.0:
            return 0
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    # ------------------------------------------------- input standardisation
    @property
    def _inorm(self):
        """The InputNorm submodule of a model built with ``input_norm=True``, else None."""
        return self._modules.get('input_norm')

    @property
    def input_norm_ready(self):
        """True once a model built with ``input_norm=True`` has its statistics (``fit_input_norm``,
        ``set_input_norm``, the first ``run_training``, ``load_state_dict``).  False for any other model."""
        return self._inorm is not None and self._inorm.ready

    def _require_inorm(self, ready=False):
        norm = self._inorm
        if norm is None:
            raise RuntimeError('this model was built without input_norm=True')
        return norm.require_ready() if ready else norm

    def _require_statistics(self, bandwidth=True):
        """RuntimeError while a statistic this model standardises or projects by does not exist yet
        (``bandwidth=False``: the bandwidth is about to be made)."""
        for stat in (self._inorm, self._rffbw if bandwidth else None):
            if stat is not None:
                stat.require_ready()

    def _check_statistics_dp(self, input_norm=True):
        """ValueError, before anything is enqueued, where this call would make a statistic under data parallel
        (``input_norm=False``: the rows come standardised)."""
        for stat in (self._inorm if input_norm else None, self._rffbw):
            if stat is not None:
                stat.refuse_data_parallel(self._dp)

    def _stats_of(self, xs, ld, n, prec):
        """mean / inv_std <- the statistics of the first ``n`` rows of ``xs`` (a device tensor of
        ``prec``'s dtype), frozen from here on.  Asynchronous: ``count`` is written on the stream."""
        self._gpu()
        norm = self._inorm
        column_statistics(prec, xs, ld, n, norm.width, norm.mean, norm.inv_std,
                          lambda numel: self._buf('inorm_ws', numel, torch.float64))
        norm.made_from(n)

    def _input_rows(self, x, dtype=None):
        """``x`` as device rows of ``dtype`` (default: its own where that is fp32 or fp64, else fp32)."""
        if hasattr(x, 'materialize'):
            x = x.materialize()
        if dtype is None:
            dtype = torch.float64 if x.dtype == torch.float64 else torch.float32
        xs, ld = _lib.as_rows(x, self._flat.device, dtype)
        assert xs.shape[1] == self._inorm.width, 'expected rows of %d columns' % self._inorm.width
        return xs, ld, (_lib.F64 if dtype == torch.float64 else _lib.F32)

    @_on_model_device
    def fit_input_norm(self, x):
        """Make the statistics from ALL rows of ``x`` on the device and freeze them: no later call refits.
        The rows are taken in the model's precision, as ``run_training`` takes them when it makes the
        statistics itself (an fp32 model narrows double rows first, a double model widens fp32 rows)."""
        self._require_inorm()
        self._gpu()
        xs, ld, prec = self._input_rows(x, self._prec.dtype)
        self._stats_of(xs, ld, xs.shape[0], prec)
        return self

    def set_input_norm(self, mean, std, count=1, dtype=None):
        """The host-given form of ``fit_input_norm``: ``mean`` and ``std`` [input_dim]; ``inv_std`` follows
        by the flat rule of include/bsig_input_norm.h with the unit roundoff of ``dtype`` (default: the
        model's).  ``count``: the number of rows behind them where known (any positive number: ready)."""
        norm = self._require_inorm()
        mean = np.asarray(torch.as_tensor(mean).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        std = np.asarray(torch.as_tensor(std).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        if mean.shape != (norm.width,) or std.shape != (norm.width,):
            raise ValueError('set_input_norm: mean and std must hold %d values' % norm.width)
        if not (std >= 0).all() or int(count) < 1:
            raise ValueError('set_input_norm: std must be >= 0 and count >= 1')
        inv = _flat_rule(mean, std, dtype or self._dtype)
        norm.mean.copy_(torch.from_numpy(mean))
        norm.inv_std.copy_(torch.from_numpy(inv))
        norm.made_from(int(count))
        return self

    @_on_model_device
    def normalize_inputs(self, x, out=None):
        """The counterpart of ``normalize_samples`` for the other side: (x - mean) * inv_std of summary rows
        ``x``, in ``x``'s own type (the fp32 or the double kernel).  ``out``: rows of the same type and shape
        on the device, last dimension contiguous; ``out is x`` standardises in place."""
        norm = self._require_inorm(ready=True)
        self._gpu()
        xs, ld, prec = self._input_rows(x)
        if out is None:
            out = torch.empty(xs.shape, dtype=prec.dtype, device=xs.device)
        if not (out.is_cuda and out.dtype == prec.dtype and out.shape == xs.shape and out.stride(1) == 1):
            raise AssertionError('normalize_inputs: out must be device rows of the type and shape of x')
        ld_out = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)
        prec.input_norm_apply(_lib.ptr(xs), ld, _lib.ptr(norm.mean), _lib.ptr(norm.inv_std), _lib.ptr(out),
                              ld_out, xs.shape[0], norm.width, _lib.stream())
        return out

    def _standardised(self, x):
        """Fresh rows of the model's precision: ``x`` standardised (the model has ready statistics)."""
        xs, _, _ = self._input_rows(x, self._prec.dtype)
        return self.normalize_inputs(xs)

    # ------------------------------------------------------ kernel bandwidth
    @property
    def _rffbw(self):
        """The RffBandwidth submodule of an ``MDRFF(sigma='median')``, else None."""
        return self._modules.get('rff_bandwidth')

    @property
    def rff_bandwidth_ready(self):
        """True once an ``MDRFF(sigma='median')`` has its bandwidth (``fit_rff_bandwidth``,
        ``set_rff_bandwidth``, the first ``run_training``, ``load_state_dict``).  False for any other model."""
        return self._rffbw is not None and self._rffbw.ready

    def _require_rffbw(self, ready=False):
        bw = self._rffbw
        if bw is None:
            raise RuntimeError("this model was built without sigma='median'")
        return bw.require_ready() if ready else bw

    def _bandwidth_of(self, xs, ld, n, prec):
        """sigma <- scale x the median pairwise distance of the first ``n`` rows (at most
        _lib.RFF_BANDWIDTH_MAX_ROWS of them) of ``xs``, device rows of ``prec``'s dtype as the projection will
        see them; frozen from here on.  Asynchronous: sigma and ``count`` are written on the stream."""
        lib, bw = self._gpu(), self._rffbw
        need = int(lib.bsig_rff_bandwidth_workspace_bytes(n, self.input_dim))
        assert need > 0, 'the median bandwidth needs at least two rows'
        ws = self._buf('rffbw_ws', need // 8, torch.float64)
        prec.rff_bandwidth_median(_lib.ptr(xs), ld, n, self.input_dim, bw.scale, _lib.ptr(bw.sigma), _lib.ptr(ws),
                                  ws.numel() * 8, _lib.stream())
        bw.made_from(min(n, _lib.RFF_BANDWIDTH_MAX_ROWS))

    def _bandwidth_of_rows(self, x):
        """``_bandwidth_of`` all rows of ``x`` (fp32 or double; anything else as fp32), taken in their own type:
        a widened fp32 row gives the bits of the fp32 row."""
        dtype = torch.float64 if x.dtype == torch.float64 else torch.float32
        xs, ld = _lib.as_rows(x, self._flat.device, dtype)
        assert xs.shape[1] == self.input_dim, 'expected rows of %d columns' % self.input_dim
        self._bandwidth_of(xs, ld, xs.shape[0], _lib.F64 if dtype == torch.float64 else _lib.F32)

    @_on_model_device
    def fit_rff_bandwidth(self, x):
        """Make the bandwidth from the rows of ``x`` (the first _lib.RFF_BANDWIDTH_MAX_ROWS at most) on the
        device and freeze it: no later call refits.  A model with ``input_norm`` standardises the rows first,
        in its own precision (RuntimeError while it has no statistics)."""
        self._require_rffbw()
        self._require_statistics(bandwidth=False)
        self._gpu()
        if hasattr(x, 'materialize'):
            x = x.materialize()
        x = x[:_lib.RFF_BANDWIDTH_MAX_ROWS]
        self._bandwidth_of_rows(x if self._inorm is None else self._standardised(x))
        return self

    def set_rff_bandwidth(self, sigma):
        """The host-given form of ``fit_rff_bandwidth``: ``sigma``, a positive finite number, taken as it is
        (``sigma_scale`` is not applied to it)."""
        bw = self._require_rffbw()
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError('set_rff_bandwidth: sigma must be a positive finite number, got %r' % (sigma,))
        bw.sigma.fill_(sigma)
        bw.made_from(1)
        return self

    # ----------------------------------------------------------- forward
    @_on_model_device
    def _head_forward(self, x, is_feat=False):
        """The raw head outputs of rows ``x`` -- or, with ``is_feat``, of an MDRFF's already projected
        feature rows (the heads are a linear-head estimator over them: same parameter layout)."""
        lib, prec = self._gpu(), self._prec
        cfg = self._cfg()
        if is_feat:
            cfg.input_dim, cfg.rff_feats = self._rff_feats, 0
        xs, ldx = _lib.as_rows(x, self._flat.device, prec.dtype)
        assert xs.shape[1] == cfg.input_dim
        b = xs.shape[0]
        nh = int(lib.bsig_head_width(C.byref(cfg.head)))
        out = torch.empty((b, nh), dtype=prec.dtype, device=xs.device)
        ws = self._buf('fwd_ws', int(prec.mdn_workspace_bytes(C.byref(cfg), b)) // prec.itemsize + 1)
        coeff, ldc, off = (None, 0, None) if is_feat else self._rff_args()
        prec.head_forward(
            C.byref(cfg), C.byref(self._hyper()), _lib.ptr(self._flat), _lib.ptr(coeff), ldc, _lib.ptr(off),
            _lib.ptr(xs), ldx, None, b, _lib.ptr(out), nh, _lib.ptr(ws),
            ws.numel() * prec.itemsize, _lib.stream())
        return cfg, out

    @_on_model_device
    def forward(self, x, noise=None, _is_feat=False):
        """Reference mdnn.py:89-125 -> (weights[B,K], mu[B,D,K], L_d[B,D,K],
        L[B,L_size,K] | None).  ``noise`` injects the rand_like draw.  Takes no plan: its products
        are fp32 whatever the model's matmul precision.  A model with ``input_norm`` standardises ``x``
        first (RuntimeError while it has no statistics; likewise an ``MDRFF(sigma='median')`` without its
        bandwidth)."""
        norm = self._inorm if not _is_feat else None
        if not _is_feat:
            self._require_statistics()
        self._gpu()
        prec = self._prec
        cfg, out = self._head_forward(x if norm is None else self._standardised(x), _is_feat)
        b, d, k = out.shape[0], self.output_dim, self.n_gaussians
        dev, dt = out.device, self._dtype
        weights = torch.empty((b, k), dtype=dt, device=dev)
        mu = torch.empty((b, d, k), dtype=dt, device=dev)
        l_d = torch.empty((b, d, k), dtype=dt, device=dev)
        low = None
        if self.Lower is not None:
            low = torch.empty((b, self.L_size, k), dtype=dt, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        nz = None if noise is None else noise.to(dev, dt).contiguous()
        seed = self._seed()
        ws = self._buf('head_ws', 64 + int(prec.head_workspace_bytes(C.byref(cfg.head), b)) // prec.itemsize)
        prec.head_outputs(
            C.byref(cfg.head), C.byref(self._hyper()), _lib.ptr(out), out.stride(0), b, _lib.ptr(nz),
            seed, 0, _lib.ptr(weights), _lib.ptr(mu), _lib.ptr(l_d),
            _lib.ptr(low), _lib.ptr(flag), _lib.ptr(ws), ws.numel() * prec.itemsize, _lib.stream())
        assert int(flag.item()) == 0      # isfinite asserts, mdnn.py:120-124
        # remembered so that mdn_loss_fn(*model(x), y).backward() works (below)
        self._fwd_ctx = (weights, x, nz, seed) if torch.is_grad_enabled() and not _is_feat else None
        return weights, mu, l_d, low

    @_on_model_device
    def mdn_loss_fn(self, weights, mu, L_d, L, y):
        """Reference mdnn.py:127-178 -> 0-dim loss tensor."""
        self._gpu()
        prec = self._prec
        cfg = self._cfg()
        dev = self._flat.device
        b = y.size()[0]
        dt = self._dtype
        ys, ldy = _lib.as_rows(y, dev, dt)
        w = weights.to(dev, dt).contiguous()
        m = mu.to(dev, dt).contiguous()
        s = L_d.to(dev, dt).contiguous()
        lo = None if L is None else L.to(dev, dt).contiguous()
        head = cfg.head
        head.full_cov = 0 if lo is None else 1
        loss = torch.zeros(1, dtype=dt, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = self._buf('head_ws', 64 + int(prec.head_workspace_bytes(C.byref(head), b)) // prec.itemsize)
        prec.nll_from_tuple(
            C.byref(head), C.byref(self._hyper()), _lib.ptr(w), _lib.ptr(m), _lib.ptr(s), _lib.ptr(lo),
            _lib.ptr(ys), ldy, b, _lib.ptr(loss), _lib.ptr(flag), _lib.ptr(ws),
            ws.numel() * prec.itemsize, _lib.stream())
        assert int(flag.item()) == 0      # mdnn.py:172-174
        ctx = getattr(self, '_fwd_ctx', None)
        if torch.is_grad_enabled() and ctx is not None and ctx[0] is weights:
            # the reference pattern loss = mdn_loss_fn(*model(x), y); loss.backward():
            # the backward is the fused forward+NLL+backward pass on the same x, y, noise
            return _FusedNLL.apply(loss[0], self, ctx[1], ys, ctx[2], ctx[3], *self.parameters())
        return loss[0]

    @_on_model_device
    def loss_and_grad(self, x, y, rows=None, noise=None, norm_batch=None, seed=None,
                      grads_out=None):
        """forward + mdn_loss_fn + backward for one minibatch
        (mdnn.py:229-233): returns the 0-dim loss; gradients land in every
        parameter's ``.grad`` (views of the flat gradient buffer).  ``y`` is
        already normalised; ``x`` is not standardised yet (a model with ``input_norm`` does that here)."""
        self._require_statistics()
        self._gpu()
        prec = self._prec
        cfg = self._cfg()
        dev = self._flat.device
        xs, ldx = _lib.as_rows(x if self._inorm is None else self._standardised(x), dev, prec.dtype)
        ys, ldy = _lib.as_rows(y, dev, prec.dtype)
        ridx = None
        b = xs.shape[0]
        if rows is not None:
            ridx = torch.as_tensor(rows, dtype=torch.int32, device=dev).contiguous()
            b = ridx.numel()
        loss = torch.zeros(1, dtype=self._dtype, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        nz = None if noise is None else noise.to(dev, self._dtype).contiguous()
        coeff, ldc, off = self._rff_args()
        ws = self._buf('grad_ws', int(prec.mdn_workspace_bytes(C.byref(cfg), b)) // prec.itemsize + 1)
        prec.loss_grad(
            C.byref(cfg), C.byref(self._hyper()), _lib.ptr(self._flat), _lib.ptr(coeff), ldc, _lib.ptr(off),
            _lib.ptr(xs), ldx, _lib.ptr(ys), ldy, _lib.ptr(ridx), b,
            int(norm_batch or b), _lib.ptr(nz), self._seed() if seed is None else int(seed), 0,
            _lib.ptr(self._flat_grad if grads_out is None else grads_out), _lib.ptr(loss),
            _lib.ptr(flag), _lib.ptr(ws), ws.numel() * prec.itemsize, _lib.stream())
        assert int(flag.item()) == 0
        return loss[0]

    @_on_model_device
    def adam_step(self, t):
        """One torch.optim.Adam step (defaults) over the flat buffers; t is
        the 1-based step number since the optimizer was created."""
        self._gpu()
        self._prec.adam_flat(
            _lib.ptr(self._flat), _lib.ptr(self._flat_grad), _lib.ptr(self._exp_avg),
            _lib.ptr(self._exp_avg_sq), self._flat.numel(), float(self.lr), 0.9, 0.999,
            1e-8, int(t), _lib.stream())

    # ---------------------------------------------------------- training
    def enable_data_parallel(self, group=None, transport=None):
        """Shard run_training's minibatch over the ranks of ``group``: every
        rank keeps a full replica, computes the gradient of its B/R rows and
        the flat gradient buffer is all-reduced (RCCL) before the identical
        Adam step.  Parameters are broadcast from rank 0.
        The exchange is the C ABI's communicator (bsig_comm_*: RCCL, or with
        ``transport='torch'`` the group's own collectives behind the same entry
        points) and run_training's update loop is bsig_fit_run_dp."""
        if self._f64:
            self._f64_dp_error()
        self._dp = _dp.DataParallel(group)
        if self._flat.is_cuda:
            with _lib.on_device(self._flat.device):
                self._dp.init_comm(self._flat.device, transport)
        self._dp.broadcast(self._flat)
        self._dp_sync_extra()
        return self

    def _dp_sync_extra(self):
        """Replica state outside the flat parameter buffer (MDRFF: the RFF frequencies)."""

    def run_training(self, x_data, y_data, n_updates, batch_size, test_frac=0.2,
                     ids_table=None, _defer=False, _feats=None, _standardized=False):
        """Reference mdnn.py:180-243.  Returns {'train_loss': [...],
        'test_loss': [...]} with the same 6 logging points.  ``ids_table``
        [n_updates, batch] (optional) overrides the numpy-RNG minibatch draw
        (teacher forcing for parity tests).

        A model with ``input_norm`` standardises ``x_data`` on its way into the chunk staging (the fp32
        staging copy is the standardising copy; a double model standardises into a buffer of its own).
        While it has no statistics, the call makes them from its own training rows -- the first ``n_train``
        of the split, never the held-out rows -- and freezes them: the reference's chunk protocol takes them
        from the first chunk's 800 training rows.  Under ``enable_data_parallel`` that would give every
        replica another scale: ValueError, before anything is enqueued.  A ``CrossCorrFactors`` input is
        materialised first (the standardised outer product does not factor): the call then behaves as under
        BSIG_NO_FUSED_SUMMARY=1, on whatever plan the engine has for summary rows.

        An ``MDRFF(sigma='median')`` without its bandwidth makes it here too, at the same point: from the
        staged training rows, standardised where the model does that, before anything is projected; under
        ``enable_data_parallel`` that is the same ValueError."""
        self._check_f64_dp()
        self._check_statistics_dp(input_norm=not _standardized)

        def once():
            return self._run_training_once(x_data, y_data, n_updates, batch_size, test_frac,
                                           ids_table, _defer, _feats, _standardized)
        # (deferred logs: the caller -- BayesSim.fit -- holds the snapshot and repeats its loop)
        return once() if _defer else self._retrying(once)

    def _ensure_plan(self, cfg, batch_size, n_train, n_test, n_updates):
        """The fit plan (graphs, persistent-kernel geometry), keyed by everything baked into it."""
        prec = self._prec
        key = (batch_size, max(n_test, self._bufs.get('cap_test', 0)), n_updates,
               cfg.head.eps_noise, cfg.lr, cfg.head.min_weight, cfg.head.ll_limit,
               max(n_train, self._bufs.get('cap_train', 0)), prec.dtype, self._matmul)
        if self._plan is None or self._plan_key != key:
            self._drop_plan(bufs=False)
            # (a model that met a persistent-launch time-out stays on the per-phase kernels: a plan
            # option, not the process-wide environment switch)
            flags = _lib.PLAN_NO_PERSISTENT if self._no_persistent else 0
            if self._matmul == 'split_bf16':
                flags |= _lib.PLAN_SPLIT_BF16
            self._plan = prec.fit_create(C.byref(cfg), C.byref(self._hyper()), batch_size, key[7], key[1],
                                         n_updates, flags)
            self._plan_key, self._plan_prec = key, prec
            self._bufs['cap_test'], self._bufs['cap_train'] = key[1], key[7]

    @staticmethod
    def block_prefix(sizes, test_frac):
        """How many leading chunks of ``sizes`` pairs a block launch can take: those with at least one
        held-out row (a chunk without one evaluates nothing inside a launch: it runs on its own)."""
        k = 0
        for n_tot in sizes:
            if split_rows(n_tot, test_frac)[1] < 1:
                break
            k += 1
        return k

    # ---- what a per-chunk call and a block launch share: staging, the pinned upload, the binding
    def _row_capacity(self, n_tot):
        """Rows the chunk staging buffers hold (fixed addresses across calls: graph replay), grown to
        ``n_tot``."""
        if n_tot > self._bufs.get('cap_rows', 0):
            self._bufs.pop('x_stage', None), self._bufs.pop('y_stage', None)
            self._bufs['cap_rows'] = n_tot
        return self._bufs['cap_rows']

    def _stage_targets(self, ys, ldy_src, y_stage, ldy, rows, st):
        """``y_stage`` <- the targets, normalised to the unit box where the model has one (mdnn.py:204-205)."""
        if self.output_lows is not None:
            self._prec.normalize_rows(
                _lib.ptr(ys), ldy_src, _lib.ptr(self.output_lows),
                _lib.ptr(self.output_highs), _lib.ptr(y_stage), ldy, rows, self.output_dim, st)
        else:
            self._prec.copy_rows(_lib.ptr(ys), ldy_src, None, _lib.ptr(y_stage), ldy, rows, self.output_dim, st)

    @contextlib.contextmanager
    def _pinned_upload(self, ring, dst, n):
        """Yields ``n`` pinned host int32 for the caller to fill; on exit they are on their way to
        ``dst[:n]``.  A truly asynchronous upload: a pageable source would make the copy wait for the
        stream to drain.  ``ring`` names the four staging slots, each reused once its last copy is done."""
        ring = self._bufs.setdefault(ring, {'slots': [], 'next': 0})
        if not ring['slots'] or ring['slots'][0][0].numel() < n:
            ring['slots'] = [[torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True), None]
                             for _ in range(4)]
        slot = ring['slots'][ring['next'] % 4]
        ring['next'] += 1
        if slot[1] is not None:
            slot[1].synchronize()
        yield slot[0].numpy()[:n]
        # (a copy KERNEL reading the pinned buffer across PCIe instead of this DMA copy was measured:
        # 487.5 k against 489.0 k pairs/s -- the ~20 us "gap before the next fit_begin_kernel" of the
        # chunk timeline is not the copy engine's hand-off)
        dst[:n].copy_(slot[0][:n], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()

    def _bind_flags(self):
        return (_lib.FIT_GRAPH if type(self).USE_GRAPH and self._prec.replays_graphs else 0) | \
            (_lib.FIT_SPLIT_ADAM if self._dp is not None else 0)

    def _bind(self, flags, x_stage, ldx, y_stage, ldy, n_train, n_test, ids_ptr, train_loss, test_loss,
              factors=None):
        """Bind the plan to one chunk: ``n_train`` training rows of ``x_stage`` / ``y_stage`` with the
        ``n_test`` held-out rows behind them, its ids and its log slots.  ``factors`` = (s_dim, a_dim,
        x_held) when the rows of ``x_stage`` are cross-correlation factor rows: the held-out pairs are then
        evaluated from the summary rows ``x_held``, or, without them, from their factor rows too."""
        prec = self._prec
        state = self._buf('state', prec.state_words, torch.int32)
        ws = self._buf('fit_ws', int(prec.fit_workspace_bytes(self._plan)) // prec.itemsize + 1)
        coeff, ldc, off = self._rff_args()
        held_x = x_stage.data_ptr() + prec.itemsize * n_train * ldx
        fb = prec.Buffers()
        fb.params, fb.grads = self._flat.data_ptr(), self._flat_grad.data_ptr()
        fb.exp_avg, fb.exp_avg_sq = self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr()
        fb.rff_coeff, fb.ld_coeff, fb.rff_offset = _lib.ptr(coeff), ldc, _lib.ptr(off)
        fb.x_train, fb.ldx_train, fb.n_train = x_stage.data_ptr(), ldx, n_train
        fb.y_train, fb.ldy_train = y_stage.data_ptr(), ldy
        fb.x_test, fb.ldx_test, fb.n_test = held_x, ldx, n_test
        fb.y_test, fb.ldy_test = y_stage.data_ptr() + prec.itemsize * n_train * ldy, ldy
        fb.ids_table = ids_ptr
        fb.train_loss, fb.test_loss = train_loss.data_ptr(), test_loss.data_ptr()
        fb.state, fb.workspace, fb.workspace_bytes = state.data_ptr(), ws.data_ptr(), ws.numel() * prec.itemsize
        fb.x_kind = _lib.X_ROWS
        if factors is not None:
            s_dim, a_dim, x_held = factors
            fb.x_kind, fb.x_s, fb.x_a = _lib.X_CROSSCORR_FACTORS, s_dim, a_dim
            if n_test > 0:      # the held-out pairs' factor rows lie behind the training rows
                fb.x_test_factors, fb.ldx_test_factors = held_x, ldx
                fb.x_test, fb.ldx_test = (None, 0) if x_held is None else (x_held.data_ptr(), x_held.stride(0))
        prec.fit_bind(self._plan, C.byref(fb), flags)

    @_on_model_device
    def run_training_block(self, feats, y_data, sizes, n_updates, batch_size, test_frac=0.2):
        """run_training (reference mdnn.py:180-243) on consecutive chunks of ``sizes`` pairs whose RFF
        features ``feats`` and targets ``y_data`` lie behind each other, as ONE launch of the persistent
        update kernel (bsig_fit_run_block).  Returns the chunks' PendingLogs, or None when this model's plan
        runs one chunk per launch (the caller then calls run_training per chunk; nothing has been drawn
        from an RNG).  The minibatch ids and jitter seeds are drawn chunk by chunk with the calls of the
        per-chunk path, in its order."""
        if (self._dp is not None or not self._flat.is_cuda or self._no_block_launch
                or self.rff is None or len(sizes) < 1 or self._f64):
            return None
        lib = self._gpu()
        self.train()
        cfg = self._cfg()
        dev = self._flat.device
        d, rows = self.output_dim, int(sum(sizes))
        assert feats.shape[0] == rows == y_data.shape[0] and feats.is_cuda and feats.dtype == torch.float32
        split = [split_rows(n, test_frac) for n in sizes]
        n_train, n_test = max(a for a, _ in split), max(b for _, b in split)
        self._ensure_plan(cfg, batch_size, n_train, n_test, n_updates)
        st = _lib.stream()
        n_chunks, n_ids = len(sizes), len(sizes) * n_updates * batch_size
        n_e = len(eval_updates(n_updates)[1])
        ldx, ldy = _lib.round_up(self.input_dim, 4), _lib.round_up(d, 4)
        y_stage = self._buf('blk_y', rows * ldy)
        stage = self._buf('blk_stage', 16 * n_chunks + n_ids, torch.int32)       # [chunk table | ids]
        train_loss, test_loss = self._buf('blk_train_loss', n_chunks * n_updates), self._buf('blk_test_loss', n_chunks * n_e)
        # The binding is a complete one of the block's FIRST chunk (its rows, held-out rows, ids and log slots
        # are the first of the block's): whoever drives the plan through the per-call entry points afterwards
        # finds every buffer it reads in place.  The summary rows themselves are not staged, as in a
        # per-chunk call whose features are handed over.
        x_stage = self._buf('x_stage', self._row_capacity(sizes[0]) * ldx)
        self._bind(self._bind_flags(), x_stage, ldx, y_stage, ldy, *split[0],
                   stage.data_ptr() + 64 * n_chunks, train_loss, test_loss)
        if n_chunks > int(self._prec.block_chunks(self._plan, n_train)):
            return None
        ys, ldy_src = _lib.as_f32_rows(y_data, dev)
        assert ys.shape[1] == d
        self._stage_targets(ys, ldy_src, y_stage, ldy, rows, st)        # once over the block's rows
        # ids (mdnn.py:219-222) and seeds: one numpy draw and one torch draw per chunk, as the per-chunk calls
        seeds = []
        with self._pinned_upload('blk_ring', stage, 16 * n_chunks + n_ids) as host:
            for c, (n_tr, _) in enumerate(split):
                lo = 16 * n_chunks + c * n_updates * batch_size
                host[lo:lo + n_updates * batch_size] = np.random.randint(
                    0, n_tr, (n_updates, batch_size), dtype=np.int32).reshape(-1) + np.int32(sum(sizes[:c]))
                seeds.append(self._seed())
            table = _lib.fit_chunk_table(sizes, seeds, n_updates, batch_size, test_frac)
            host[:16 * n_chunks] = table.view(np.int32)
        packed = torch.empty(n_chunks, 2 * n_e + 1, dtype=torch.float32, device=dev)
        _lib.check(lib.bsig_fit_run_block(
            self._plan, _lib.ptr(feats), feats.stride(0), rows, _lib.ptr(y_stage), ldy,
            C.c_void_p(stage.data_ptr() + 64 * n_chunks), n_ids, C.c_void_p(table.ctypes.data),
            _lib.ptr(stage), n_chunks, _lib.ptr(train_loss), _lib.ptr(test_loss), _lib.ptr(packed),
            batch_size, st))
        self._block_launches += 1
        shared = _BlockLogs(packed)
        return [PendingLogs(packed[c], n_e, split[c][1], type(self).VERBOSE, block=(shared, c)) for c in range(n_chunks)]

    @_on_model_device
    def _run_training_once(self, x_data, y_data, n_updates, batch_size, test_frac=0.2,
                           ids_table=None, _defer=False, _feats=None, _standardized=False):
        assert x_data.shape[0] == y_data.shape[0]
        lib, prec = self._gpu(), self._prec
        self.train()
        cfg = self._cfg()
        dev = self._flat.device
        d, n_tot = self.output_dim, x_data.shape[0]
        n_train, n_test = split_rows(n_tot, test_frac)
        st = _lib.stream()
        self._ensure_plan(cfg, batch_size, n_train, n_test, n_updates)
        flags = self._bind_flags()
        # a cross-correlation summary may arrive as factor rows (summarizers.CrossCorrFactors):
        # plans whose first layer lives in the persistent kernel consume them as they are
        factors = None
        if isinstance(x_data, CrossCorrFactors) and \
                not prec.accepts_factor_rows(self._plan, x_data.s_dim, x_data.a_dim):
            x_data = x_data.materialize()
        # input_norm: summary rows of the model's precision; the statistics, where they do not exist yet,
        # from this call's training rows (``_standardized``: the caller -- BayesSim.fit -- has done both)
        norm = None if _standardized else self._inorm
        if norm is not None:
            x_data, ld_raw, _ = self._input_rows(x_data, prec.dtype)
            if not norm.ready:
                self._stats_of(x_data, ld_raw, n_train, prec)
        make_bw = self._rffbw is not None and not self._rffbw.ready
        if make_bw and isinstance(x_data, CrossCorrFactors):
            x_data = x_data.materialize()
        ldy = _lib.round_up(d, 4)
        ys, ldy_src = _lib.as_rows(y_data, dev, prec.dtype)
        assert x_data.shape[1] == self.input_dim and ys.shape[1] == d
        cap_rows = self._row_capacity(n_tot)
        if isinstance(x_data, CrossCorrFactors):
            # bound where they lie: 1.3 KB per Ant row instead of a 47 KB summary row
            x_stage, _ = _lib.as_f32_rows(x_data.factors, dev)
            ldx = x_stage.stride(0) if n_tot > 1 else x_stage.shape[1]
            # the held-out rows, read once per evaluation, as summary rows -- unless the launch
            # evaluates from the held-out pairs' factor rows too (a streamed first layer): then no
            # [n, I] block exists at all
            eval_fac = bool(prec.evaluates_from_factors(self._plan, x_data.s_dim, x_data.a_dim, flags))
            x_held = x_data[n_train:].materialize() if n_test > 0 and not eval_fac else None
            self._bufs['x_keepalive'] = (x_stage, x_held)
            factors = (x_data.s_dim, x_data.a_dim, x_held)
        elif not prec.replays_graphs:
            # no graph to replay in this precision: the (widened) rows are bound where they lie
            x_stage, ldx = _lib.as_rows(x_data, dev, prec.dtype)
            if norm is not None:      # ... and standardised into a buffer of the model's
                ldx = self.input_dim
                x_stage = self.normalize_inputs(x_stage, self._buf('x_norm', n_tot * ldx)[:n_tot * ldx].view(n_tot, ldx))
            self._bufs['x_keepalive'] = (x_stage, None)
        else:
            # chunk staging: fixed addresses (graph replay) and 16-B aligned rows
            xs, ldx_src = _lib.as_rows(x_data, dev, prec.dtype)
            ldx = _lib.round_up(self.input_dim, 4)
            x_stage = self._buf('x_stage', cap_rows * ldx)
            # (an MDRFF whose rows' features are handed over never reads the summaries themselves)
            if _feats is None or not prec.takes_features(self._plan, n_train):
                if norm is not None:      # the staging copy IS the standardising copy: no further pass
                    prec.input_norm_apply(_lib.ptr(xs), ldx_src, _lib.ptr(norm.mean), _lib.ptr(norm.inv_std),
                                          _lib.ptr(x_stage), ldx, n_tot, self.input_dim, st)
                else:
                    prec.copy_rows(_lib.ptr(xs), ldx_src, None, _lib.ptr(x_stage), ldx, n_tot, self.input_dim, st)
        if make_bw:
            # the bandwidth of the rows the projection is about to see: the staged training rows, never the
            # held-out ones (BayesSim.fit makes it from the same rows of its first block, with the same bits)
            self._bandwidth_of(x_stage, ldx, n_train, prec)
        y_stage = self._buf('y_stage', cap_rows * ldy)
        self._stage_targets(ys, ldy_src, y_stage, ldy, n_tot, st)
        n_ids = n_updates * batch_size
        ids_dev = self._buf('ids', max(n_ids, 1), torch.int32)

        def upload_ids():
            """Minibatch ids in the reference's numpy-RNG order (mdnn.py:219-222), drawn on the host."""
            if ids_table is None:
                # (dtype=int32: the SAME draws from the same stream as the reference's int64 default --
                # tests/test_ids_draw.py -- in half the host time and without the astype pass: at 122 x
                # 8192 ids the draw is what the GPU waits for when the host is busy)
                ids_np = np.random.randint(0, n_train, (n_updates, batch_size), dtype=np.int32)
            else:
                ids_np = np.asarray(ids_table)
                assert ids_np.shape == (n_updates, batch_size)
            with self._pinned_upload('ids_ring', ids_dev, n_ids) as host:
                host[:] = ids_np.reshape(-1)

        # A large table (the scaled-batch fit: 122 x 8192 ids, 8 ms of numpy) is drawn AFTER the
        # begin call has been enqueued, so that begin's device work -- the RFF projection of the
        # chunk's rows, 7 ms at 100k rows -- runs under it.  Only where begin does not read the table
        # (a plan that projects the gathered minibatch rows instead of each row once does).
        late_ids = n_ids >= (1 << 16) and (cfg.rff_feats == 0 or
                                           bool(prec.takes_features(self._plan, n_train)))
        if not late_ids:
            upload_ids()
        eval_its = eval_updates(n_updates)[1]
        train_loss = self._buf('train_loss', n_updates)
        test_loss = self._buf('test_loss', len(eval_its))
        self._bind(flags, x_stage, ldx, y_stage, ldy, n_train, n_test, ids_dev.data_ptr(),
                   train_loss, test_loss, factors)
        if _feats is not None:
            # MDRFF: the rows' RFF features, already projected by the caller (BayesSim.fit)
            assert _feats.shape[0] == n_tot and _feats.is_cuda and _feats.dtype == torch.float32
            # (a plan without a per-row feature cache declines: bsig_fit_begin then projects)
            prec.fit_set_features(self._plan, _lib.ptr(_feats), _feats.stride(0), n_tot, st)
        world = 1 if self._dp is None else self._dp.world
        prec.fit_begin(self._plan, self._seed(), batch_size * world, st)
        if late_ids:
            upload_ids()
        if self._dp is None:
            prec.fit_run(self._plan, n_updates, st)
            # single read-back per call: 6+6 losses and the isfinite flag
            # (a fresh allocation per call -- no kernel: BayesSim.fit reads all chunks' logs at the end)
            packed = torch.empty(2 * len(eval_its) + 1, dtype=prec.dtype, device=dev)
            prec.fit_pack_logs(self._plan, n_updates, len(eval_its), _lib.ptr(packed), st)
            pending = PendingLogs(packed, len(eval_its), n_test, type(self).VERBOSE)
        else:
            # data parallel (fp32 only: refused for a double model): grad -> all-reduce -> apply per update,
            # driven from C
            self._dp._on_gpu = True
            logs = torch.empty(n_updates + len(eval_its) + 3, dtype=torch.float32, device=dev)
            _lib.check(lib.bsig_fit_run_dp(self._plan, self._dp.comm, n_updates, _lib.ptr(logs), st))
            if self._dp._error is not None:
                err, self._dp._error = self._dp._error, None
                raise err
            pending = PendingLogs(logs, len(eval_its), n_test, type(self).VERBOSE,
                                  dp=(eval_its, n_updates, world))
        return pending if _defer else pending.result()

    fit = run_training   # the north-star name for the same call

    @_on_model_device
    def normalize_samples(self, params):
        """Reference mdnn.py:245-248."""
        self._gpu()
        ps, ldp = _lib.as_rows(params, self._flat.device, self._dtype)
        out = torch.empty_like(ps)
        self._prec.normalize_rows(
            _lib.ptr(ps), ldp, _lib.ptr(self.output_lows), _lib.ptr(self.output_highs),
            _lib.ptr(out), out.stride(0), ps.shape[0], ps.shape[1], _lib.stream())
        return out

    def predict_MoGs(self, xs, noise=None):
        """Reference mdnn.py:250-289: one pdf.MoG per row of ``xs`` with
        de-normalised means and [diag | strict-lower] factors.  The
        full-covariance row indexing bug of mdnn.py:281 (``L[:, :, comp_id]``
        instead of ``L[pt, :, comp_id]``) is not reproduced.  A model with ``input_norm`` standardises
        ``xs`` first (before an MDRFF's projection)."""
        ntest, dim = xs.size()
        self._require_statistics()
        if self.rff is not None and self._matmul != 'float32':
            # the projection follows the model's matmul precision; the head products stay fp32
            feats = self.rff.to_features(xs if self._inorm is None else self._standardised(xs))
            w, mu, l_d, low = self.forward(feats, noise=noise, _is_feat=True)
        else:
            w, mu, l_d, low = self.forward(xs, noise=noise)
        w, mu, l_d = w.cpu().numpy(), mu.cpu().numpy(), l_d.cpu().numpy()
        low = None if low is None else low.cpu().numpy()
        normalize = self.output_lows is not None
        if normalize:
            lows = self.output_lows.cpu().numpy()
            rng = self.output_highs.cpu().numpy() - lows
        rows, _ = np.tril_indices(self.output_dim, -1)
        npdt = self._prec.np_dtype      # the mixtures follow the model's dtype
        mogs = []
        for pt in range(ntest):
            ms, ls = [], []
            for k in range(self.n_gaussians):
                m = mu[pt, :, k]
                diag = l_d[pt, :, k]
                lower = None if low is None else low[pt, :, k]
                if normalize:           # Rng * T: row i scaled by rng[i]
                    m = m * rng + lows
                    diag = diag * rng
                    lower = None if lower is None else lower * rng[rows]
                ms.append(m.astype(npdt))
                ls.append((diag if lower is None else np.concatenate([diag, lower]))
                          .astype(npdt))
            mogs.append(pdf.MoG(a=w[pt, :], ms=ms, Ls=ls))
        return mogs
