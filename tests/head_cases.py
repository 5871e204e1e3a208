"""Shared pieces of the mixture-density head tests (tests/test_host_logic.py,
tests/test_gpu_head_paths.py): a numpy Philox4x32-10 that mirrors
bayes_sim_ig_amd/csrc/common.h, the two ways the head kernels map a jitter
draw to an element (row, d, k), and the table of head shapes with the device
path bsig_debug_head_geometry must report for each."""
import numpy as np

# bsig_debug_head_geometry out[0]
PATH_WAVE2 = 0      # mdn_nll_diag_wave_kernel<8, 2>: one wavefront per row, at most two sweeps
PATH_WAVE8 = 1      # mdn_nll_diag_wave_kernel<8, 8>: row body of 4 or 8 sweeps
PATH_DIAG = 2       # mdn_nll_kernel<false>: thread per component, R rows per workgroup
PATH_FULL = 3       # mdn_nll_kernel<true>: full covariance
PATH_NAMES = {PATH_WAVE2: 'wave2', PATH_WAVE8: 'wave8', PATH_DIAG: 'diag', PATH_FULL: 'full'}

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, stream_id, ctr):
    """Philox4x32-10 of common.h: counter (ctr lo, ctr hi, stream lo, stream hi), key (seed lo,
    seed hi).  `ctr` is an array of uint64 counters; returns uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0 = ctr & _LO
    c1 = ctr >> np.uint64(32)
    c2 = np.full_like(ctr, int(stream_id) & 0xFFFFFFFF)
    c3 = np.full_like(ctr, (int(stream_id) >> 32) & 0xFFFFFFFF)
    k0, k1 = np.uint32(int(seed) & 0xFFFFFFFF), np.uint32((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & _LO
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & _LO
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = np.uint32((int(k0) + int(_W0)) & 0xFFFFFFFF)
        k1 = np.uint32((int(k1) + int(_W1)) & 0xFFFFFFFF)
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(x):
    """common.h u01: the top 24 bits as a float in [0, 1) (exact in fp32)"""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0


def draws_wave(batch, d, k, seed, stream_id):
    """u[b, d, k] of the one-wavefront-per-row paths (head_device.h diag_row_body): element (d, k)
    sits on lane (d % groups) * K + k in sweep q = d // groups, groups = 64 // K; lane l of row b
    draws counter (b * 64 + l) * 2 + q // 4 and takes word q % 4."""
    groups = 64 // k
    b_ = np.arange(batch, dtype=np.uint64)[:, None, None]
    dd = np.arange(d)[None, :, None]
    kk = np.arange(k)[None, None, :]
    lane = ((dd % groups) * k + kk).astype(np.uint64)
    q = dd // groups
    ctr = (b_ * np.uint64(64) + lane) * np.uint64(2) + (q // 4).astype(np.uint64)
    words = philox4x32_10(seed, stream_id, ctr)
    word = np.broadcast_to(q % 4, ctr.shape)
    return u01(np.take_along_axis(words, word[..., None], axis=-1)[..., 0])


def draws_flat(batch, d, k, seed, stream_id):
    """u[b, d, k] of the thread-per-component kernels and mdn_outputs_kernel: counter = the flat
    element index (b * D + d) * K + k, word 0."""
    ctr = np.arange(batch * d * k, dtype=np.uint64).reshape(batch, d, k)
    return u01(philox4x32_10(seed, stream_id, ctr)[..., 0])


def draws_for_path(path, batch, d, k, seed, stream_id):
    fn = draws_wave if path in (PATH_WAVE2, PATH_WAVE8) else draws_flat
    return fn(batch, d, k, seed, stream_id)


# (batch, D, K, full, path, row-body sweeps (0: not a wavefront path), more than one finish slab)
CASES = [
    (1, 1, 1, False, PATH_WAVE2, 2, False),
    (7, 2, 10, False, PATH_WAVE2, 2, False),
    (300, 12, 10, False, PATH_WAVE2, 2, False),      # D = 2 * (64 / K): the last two-sweep shape
    (1001, 3, 7, False, PATH_WAVE2, 2, False),
    (1, 40, 3, False, PATH_WAVE2, 2, False),
    (1025, 5, 16, False, PATH_WAVE2, 2, True),
    (7, 13, 10, False, PATH_WAVE8, 4, False),        # D = 2 * (64 / K) + 1 (anymal_yaml, cfg2)
    (1001, 17, 10, False, PATH_WAVE8, 4, False),     # ant_yaml
    (64, 24, 10, False, PATH_WAVE8, 4, False),       # D = 4 * (64 / K)
    (1025, 13, 10, False, PATH_WAVE8, 4, True),
    (8193, 13, 10, False, PATH_WAVE8, 4, True),
    (7, 25, 10, False, PATH_WAVE8, 8, False),        # D = 4 * (64 / K) + 1
    (100, 32, 10, False, PATH_WAVE8, 8, False),      # shadow_more
    (1025, 32, 10, False, PATH_WAVE8, 8, True),
    (8193, 32, 10, False, PATH_WAVE8, 8, True),
    (33, 48, 10, False, PATH_WAVE8, 8, False),       # eight sweeps, the last wavefront shape at K10
    (9, 8, 33, False, PATH_WAVE8, 8, False),         # one d-slot per sweep, 31 idle lanes
    (5, 8, 64, False, PATH_WAVE8, 8, False),
    (7, 49, 10, False, PATH_DIAG, 0, False),         # nine sweeps: thread per component
    (1001, 49, 10, False, PATH_DIAG, 0, False),      # R = 8: a last workgroup of one row
    (1025, 9, 33, False, PATH_DIAG, 0, True),
    (8193, 9, 64, False, PATH_DIAG, 0, True),
    (1, 9, 64, False, PATH_DIAG, 0, False),
    (9, 5, 3, True, PATH_FULL, 0, False),
    (300, 3, 7, True, PATH_FULL, 0, False),
    (7, 32, 10, True, PATH_FULL, 0, False),          # R = 1 (the LDS loop)
    (1025, 4, 16, True, PATH_FULL, 0, True),
]

# the full-covariance shape the LDS loop refuses (R = 1 needs more than 64 KB)
REFUSED = (4, 48, 10, True)


def case_id(c):
    b, d, k, full, path, nq, _ = c
    return 'b%d_d%d_k%d_%s%s' % (b, d, k, PATH_NAMES[path], nq or '')
