"""Mixture Density NN on Random Fourier Features — mirror of the reference's
bayes_sim_ig/models/mdrff.py (class MDRFF).  ``forward`` = RFF projection
(fp32-MFMA GEMM + sincos epilogue) followed by the MDNN heads.  The reference
projects the gathered minibatch inside every update (mdrff.py:28-30 inside
mdnn.py:231); the features are a pure function of the row, so ``run_training``
projects every distinct row of the chunk ONCE per call (feature cache,
csrc/estimator.hip) and ``BayesSim.fit`` projects blocks of chunks in one GEMM --
bitwise the same features, 12.5x fewer row projections.

``sigma='median'`` (not in the reference): the bandwidth is ``sigma_scale`` times the median pairwise distance of
the first training rows, made on the device and frozen (include/bsig_rff_bandwidth.h; MDNN.fit_rff_bandwidth)."""
import numpy as np
import torch

from . import _lib
from .mdnn import MDNN, RffBandwidth
from .rff import RFF


class MDRFF(MDNN):
    def __init__(self, input_dim, output_dim, output_lows, output_highs,
                 n_gaussians, lr, activation, full_covariance, device='cpu',
                 n_feat=500, kernel='RBF', sigma=1.0, freqs=None, sigma_scale=1.0, **kwargs):
        """Same arguments as the reference (mdrff.py:15-17); ``freqs``
        optionally injects the [n_feat/2, input_dim] frequency matrix; ``input_norm=True`` (a keyword of
        ``**kwargs``): the summaries are standardised before the projection (MDNN.fit_input_norm);
        ``sigma='median'``: the bandwidth is ``sigma_scale`` (a positive number) times the median pairwise
        distance of the first training rows (MDNN.fit_rff_bandwidth); ``sigma_scale`` with any other sigma
        is a ValueError."""
        median = isinstance(sigma, str)
        if median and sigma != 'median':
            raise ValueError("sigma must be a number, a list of numbers or 'median', got %r" % (sigma,))
        if isinstance(sigma_scale, bool) or not isinstance(sigma_scale, (int, float)) or \
                not (np.isfinite(sigma_scale) and sigma_scale > 0):
            raise ValueError('sigma_scale must be a positive number, got %r' % (sigma_scale,))
        if not median and float(sigma_scale) != 1.0:
            raise ValueError("sigma_scale applies to sigma='median', not to sigma=%r" % (sigma,))
        self._rff_input_dim = input_dim
        a = (2.0 / float(n_feat)) ** 0.5          # rff.py:107
        super().__init__(n_feat, output_dim, output_lows, output_highs,
                         n_gaussians, hidden_layers=[], lr=lr,
                         activation=activation,
                         full_covariance=full_covariance, device=device,
                         _rff_feats=n_feat, _rff_scale=a,
                         # (the statistics are those of the summary rows, before the projection)
                         input_norm=kwargs.get('input_norm', False), _input_norm_dim=input_dim)
        # heads see n_feat inputs; the estimator's rows are input_dim wide
        self.input_dim = input_dim
        # (a submodule only on such a model, after every other: a default model's state_dict keys are untouched)
        if median:
            self.rff_bandwidth = RffBandwidth(sigma_scale, device)
        self.rff = RFF(n_feat, input_dim, 1.0 if median else sigma, cos_only=False,
                       quasi_random=False if input_dim > 100 else True,
                       kernel=kernel, device=device, freqs=freqs, bandwidth=self._rffbw)
        self._rff_scale = float(self.rff.a)
        self.rff.matmul_precision = self._matmul     # the feature map follows its model (set_matmul_precision)
        if MDNN.VERBOSE:
            print('MDRFF n_feat', n_feat, 'sigma', sigma)
            print(self)

    def _cfg(self):
        cfg = super()._cfg()
        cfg.input_dim = int(self._rff_input_dim)
        return cfg

    def _rff_args(self):
        if self._f64:
            # fp64 mode: the widened fp32 draws, divided in double (what the reference's rff.py:130
            # computes once freqs and sigma are doubles); features are projected in double per call
            bw = self._rffbw
            if bw is not None:
                return self._coeff64_from_bandwidth(bw.require_ready())
            co = self._bufs.get('coeff64')
            if co is None:
                dev = self._flat.device
                co = (self.rff.freqs.to(dev).double() / self.rff.sigma.to(dev).double()).contiguous()
                self._bufs['coeff64'] = co
            return co, co.stride(0), None
        co = self.rff.coeff()
        return co, co.stride(0), None

    def _coeff64_from_bandwidth(self, bw):
        """The fp64 mode's coefficient from the device scalar (bsig_rff_coeff_dev_f64), redone when the
        bandwidth has been given anew."""
        co, version = self._bufs.get('coeff64_bw', (None, None))
        if co is None or version != bw.version:
            dev, rff = self._flat.device, self.rff
            if co is None:
                co = torch.empty((rff.m_feat, rff.d), dtype=torch.float64, device=dev)
            fr = rff.freqs.to(dev).contiguous()
            _lib.F64.rff_coeff_dev(_lib.ptr(fr), _lib.ptr(bw.sigma.to(dev)), _lib.ptr(co), rff.m_feat, rff.d,
                                   rff.d, _lib.stream())
            self._bufs['coeff64_bw'] = (co, bw.version)
        return co, co.stride(0), None

    def _dp_sync_extra(self):
        """Data-parallel replicas must share the feature map: the frequencies come from
        the global numpy RNG (rff.py:111-120), which ranks may have seeded differently, and
        are not part of the flat parameter buffer -- rank 0's are broadcast."""
        rff = self.rff
        # (a median bandwidth is not broadcast: _check_statistics_dp asks for the same value on every rank)
        for name in ('freqs', 'offset') if self._rffbw is not None else ('freqs', 'sigma', 'offset'):
            t = getattr(rff, name)
            if t is None:
                continue
            flat = t.to(self._flat.device, torch.float32).contiguous().view(-1).clone()
            self._dp.broadcast(flat)
            setattr(rff, name, flat.view(t.shape).to(t.device))
        rff._coeff = None
