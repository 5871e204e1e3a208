"""Random Fourier Features on MI355X — mirror of the reference's
bayes_sim_ig/models/rff.py (class RFF, same constructor and attributes).

The frequency draw is host-side, one-off and consumes the GLOBAL numpy RNG
exactly like the reference (rff.py:111-120, 135-184), so seeded runs get
bit-identical frequencies.  The projection ``a*[cos|sin](x (freqs/sigma)^T)``
(rff.py:122-132) is the fp32-MFMA GEMM with fused sincos epilogue in
csrc/gemm_f32.hip.

``bandwidth`` (not in the reference): the RffBandwidth of an ``MDRFF(sigma='median')``.  The coefficient is then
``freqs / sigma`` with the ONE double that submodule holds on the device (bsig_rff_coeff_dev,
include/bsig_rff_bandwidth.h), and the reference's ``sigma`` attribute is filled from it when somebody reads it.
"""
import numpy as np
import torch
from scipy.special import erfinv

from . import _lib

_STUDENT_NU = {'Laplace': 1, 'Matern12': 1, 'Matern32': 3, 'Matern52': 5}


HALTON_SEED = 20231002   # fixed: the reference's sequence is deterministic too


def halton_points(m, d):
    """m low-discrepancy points in (0,1)^d for the quasi-random frequency draw.

    The reference uses ``ghalton.GeneralizedHalton(ghalton.EA_PERMS[:d])`` (rff.py:113-116):
    a Halton sequence whose digits are permuted per dimension -- a third-party module whose
    permutation tables are not available here (PARITY UNPINNED for input_dim <= 100; pass
    ``freqs=`` to inject the reference's frequencies).  The stand-in is scipy's Owen-scrambled
    Halton sequence with a fixed seed: like the generalized sequence it breaks the
    dimension-to-dimension correlation of the plain one, whose coordinates with a prime
    base above m are all the same ramp i/p (for m = 100, d = 40, the pendulum MDRFF of
    regression_tests.py:104-128, 16 % of the coordinate pairs of the PLAIN sequence
    correlate above 0.5 and 14 coordinates are one-sided; tests/test_host_logic.py bounds
    both here)."""
    from scipy.stats import qmc
    pts = qmc.Halton(d=int(d), scramble=True, seed=HALTON_SEED).random(int(m))
    tiny = 2.0 ** -24
    return np.clip(pts, tiny, 1.0 - tiny)


def _inv_cdf(kernel, u):
    """Spectral-density inverse CDFs, rff.py:139-184."""
    if kernel == 'RBF':
        return erfinv(2 * u - 1) * np.sqrt(2)
    if kernel in ('Laplace', 'Matern12'):
        return np.tan(np.pi * (u - 0.5))
    if kernel == 'Matern32':
        return (2 * u - 1) / np.sqrt(2 * u * (1 - u))
    alpha = 4 * u * (1 - u)
    p = 4 * np.cos(np.arccos(np.sqrt(alpha)) / 3) / np.sqrt(alpha)
    return np.sign(u - 0.5) * np.sqrt(p - 4)


def draw_freqs(kernel, m, d, quasi_random):
    """rff.py:111-120."""
    if kernel != 'RBF' and kernel not in _STUDENT_NU:
        raise ValueError("Kernel {} is not recognised.".format(kernel))
    if quasi_random:
        return _inv_cdf(kernel, halton_points(m, d))
    if kernel == 'RBF':
        return np.random.normal(0.0, 1.0, (m, d))
    nu = _STUDENT_NU[kernel]
    g = np.random.normal(0, 1, (m, d))
    return g * np.sqrt(nu / np.random.chisquare(nu, (m, d)))


class RFF:
    """Random Fourier Features, vanilla or quasi-random (reference rff.py:43-132).

    Attributes kept from the reference: n_feat, d, sigma [1,d], freqs
    [m,d], offset, a, device, to_features.
    """

    def __init__(self, n_feat, d, sigma, cos_only=False, quasi_random=True,
                 kernel='RBF', device='cpu', freqs=None, bandwidth=None):
        self.n_feat, self.d, self.device = n_feat, int(d), device
        self.cos_only = bool(cos_only)
        self.bandwidth = bandwidth      # (mdnn.RffBandwidth | None; ``sigma`` is then a placeholder)
        self._coeff_version = None
        if isinstance(sigma, list):
            assert len(sigma) == d
            sig = np.array(sigma, dtype=np.float32)
        else:
            sig = np.ones(d, dtype=np.float32) * sigma
        self.sigma = torch.from_numpy(sig).float().reshape(1, -1).to(device)
        if kernel != 'RBF' and kernel not in _STUDENT_NU:
            raise ValueError("Kernel {} is not recognised.".format(kernel))
        self.offset = None
        if cos_only:
            f = draw_freqs(kernel, n_feat, d, quasi_random) if freqs is None else freqs
            self.offset = torch.from_numpy(
                2.0 * np.pi * np.random.rand(1, n_feat)).float().to(device)
            self.a = np.sqrt(1.0 / float(n_feat))
            self.to_features = self._to_cos_only_features
        else:
            assert self.n_feat % 2 == 0
            f = draw_freqs(kernel, n_feat // 2, d, quasi_random) if freqs is None else freqs
            self.a = np.sqrt(1.0 / float(n_feat / 2))
            self.to_features = self._to_cos_sin_features
        self.freqs = torch.from_numpy(np.asarray(f)).float().to(device)
        self._coeff = None       # freqs / sigma, [m, ld] device, built lazily
        # 'float32' | 'split_bf16' (include/bsig_matmul.h): an MDRFF's feature map follows its model
        self.matmul_precision = 'float32'
        self._ws = None

    # -- device-side state -------------------------------------------------
    @property
    def m_feat(self):
        return self.freqs.shape[0]

    @property
    def sigma(self):
        """The reference's [1, d] attribute.  With ``bandwidth``: filled from the device scalar when read (a
        host read-back; nothing on the fit path asks)."""
        if self.bandwidth is not None:
            bw = self.bandwidth.require_ready()
            return torch.full((1, self.d), float(bw.sigma.item()), dtype=torch.float32, device=self.device)
        return self._sigma

    @sigma.setter
    def sigma(self, value):
        self._sigma = value

    def _coeff_from_bandwidth(self):
        """freqs / sigma from the device scalar, in the one buffer the plans bind; redone when the bandwidth
        has been given anew."""
        bw = self.bandwidth.require_ready()
        lib = _lib.require_gpu()
        if self._coeff is None or self._coeff_version != bw.version:
            dev = self.freqs.device if self.freqs.is_cuda else torch.device(
                'cuda', torch.cuda.current_device())
            fr = self.freqs.to(dev).contiguous()
            ld = _lib.round_up(self.d, 4)
            if self._coeff is None or self._coeff.device != dev:
                self._coeff = torch.empty((self.m_feat, ld), dtype=torch.float32, device=dev)
            with _lib.device_stream(dev) as stream:
                _lib.check(lib.bsig_rff_coeff_dev(_lib.ptr(fr), _lib.ptr(bw.sigma.to(dev)), _lib.ptr(self._coeff),
                                                  self.m_feat, self.d, ld, stream))
            self._coeff_version = bw.version
        return self._coeff

    def coeff(self, sigma=None):
        """freqs / sigma (rff.py:124,130), pitch rounded up to 4 floats."""
        if sigma is None and self.bandwidth is not None:
            return self._coeff_from_bandwidth()
        lib = _lib.require_gpu()
        if sigma is not None or self._coeff is None:
            dev = self.freqs.device if self.freqs.is_cuda else torch.device(
                'cuda', torch.cuda.current_device())
            fr = self.freqs.to(dev).contiguous()
            sg = (self.sigma if sigma is None else sigma).to(dev).float().contiguous()
            ld = _lib.round_up(self.d, 4)
            co = torch.empty((self.m_feat, ld), dtype=torch.float32, device=dev)
            with _lib.device_stream(dev) as stream:
                _lib.check(lib.bsig_rff_coeff(_lib.ptr(fr), _lib.ptr(sg), _lib.ptr(co),
                                              self.m_feat, self.d, ld, stream))
            if sigma is not None:
                return co
            self._coeff = co
        return self._coeff

    def _project(self, x, sigma, cos_only):
        if sigma is None and self.bandwidth is not None:
            self.bandwidth.require_ready()
        lib = _lib.require_gpu()
        home = x.device
        co = self.coeff(sigma)
        xs, ldx = _lib.as_f32_rows(x, co.device)
        b = xs.shape[0]
        assert xs.shape[1] == self.d
        feats = torch.empty((b, self.n_feat), dtype=torch.float32, device=co.device)
        need = int(lib.bsig_gemm_workspace_bytes(b, self.m_feat, self.d))
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty(max(need // 4 + 1, 1), dtype=torch.float32,
                                   device=co.device)
        off = self.offset.to(co.device).contiguous() if cos_only else None
        with _lib.device_stream(co.device) as stream:
            args = (_lib.ptr(xs), ldx, None, _lib.ptr(co), co.stride(0), _lib.ptr(off),
                    _lib.ptr(feats), feats.stride(0), b, self.d, self.m_feat,
                    float(self.a), 1 if cos_only else 0, _lib.ptr(self._ws),
                    self._ws.numel() * 4, stream)
            if self.matmul_precision == 'float32':
                _lib.check(lib.bsig_rff_project(*args))
            else:
                _lib.check(lib.bsig_rff_project_ex(*args, _lib.matmul_precision(self.matmul_precision)))
        return feats if home == feats.device else feats.to(home)

    def _to_cos_only_features(self, x, sigma=None):
        return self._project(x, sigma, True)

    def _to_cos_sin_features(self, x, sigma=None):
        return self._project(x, sigma, False)
