#!/usr/bin/env python3
"""A/B of two builds of the library (BSIG_LIB_PATH) over the start, cross-correlation and signature summaries
(csrc/summaries.h).  Two builds that print the same hashes plan their launches alike and compute the same bits.

--host (no GPU, no torch): one sha256 over bsig_debug_summary_path's return code and 16 words (and, where it
refuses, bsig_last_error's text) for the shapes of tests/summary_cases.py and the grid sd in {2, 3, 17, 60, 211}
x ad in {1, 8, 20} x traj_len in {2, 5, 10, 11, 200} x kinds 0..3 x depth 0..3 x aligned / unaligned x
factors on / off x two batch sizes x three pitches.

default (MI355X): per case one line with a sha256 of the output bytes of summary_start, summary_corr,
summary_corrdiff and summary_signatory (depths 1 to 3, where the case's shape has them) in both dtypes on
seeded inputs, each into a fresh buffer, a 16-byte aligned `out` view of even pitch and a view that starts one
element in with an odd pitch.  The cases: tests/summary_cases.py and the shapes of
tests/test_gpu_summaries_f64.py.  A call the library refuses prints the exception's name.

--time (MI355X): the double kernels, HIP events, 9 repetitions after a warm-up: every repetition in us.  The events
bracket the Python call, so a figure holds the call's share of the host's submission path as well as the kernel:
both builds run the same wrapper.
usage: [BSIG_LIB_PATH=...] python tools/summaries_ab.py [--host | --time] [--only SUBSTRING]"""
import ctypes as C
import hashlib
import itertools
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from bayes_sim_ig_amd import _lib     # noqa: E402
import summary_cases as S             # noqa: E402

# (n, t, ta, sd, ad) of tests/test_gpu_summaries_f64.py: START_SHAPES, CC_SHAPES, SIG_CASES, the new branch shapes
F64_SHAPES = [(1, 3, 2, 1, 1), (5, 12, 11, 3, 2), (3, 10, 10, 2, 1), (2, 3, 3, 2, 1), (4, 20, 20, 3, 3),
              (2, 12, 12, 52, 1), (1, 2, 2, 2, 1), (2, 4, 4, 2100, 1), (3, 2, 2, 1, 1), (3, 5, 5, 2, 1),
              (2, 20, 20, 4, 1), (2, 3, 3, 18, 3), (2, 4, 4, 19, 3), (2, 3, 3, 100, 10), (2, 5, 5, 2, 1),
              (2, 90, 90, 90, 10), (3, 4, 4, 3, 1), (2, 3, 3, 258, 1), (2, 40, 40, 4, 1), (2, 3, 3, 7, 1),
              (2, 3, 3, 13, 3), (1, 223, 223, 18, 3), (2, 5, 5, 2, 2), (2, 6, 6, 4, 22), (2, 8, 8, 33, 1),
              (2, 8, 8, 34, 1), (2, 5, 5, 85, 1), (2, 5, 5, 84, 1), (2, 10, 10, 2, 52)]
N_BIG = 4096 + 5      # above the double grid cap (BSIG_F64_SUMMARY_GRID_CAP) by a few rows


def host():
    lib = _lib.load()
    digest, count = hashlib.sha256(), 0
    out = (C.c_int32 * 16)()

    def record(*args):
        nonlocal count
        for i in range(16):
            out[i] = -7
        rc = lib.bsig_debug_summary_path(*args, out)
        digest.update(struct.pack('<i16i', rc, *out) + (lib.bsig_last_error() if rc else b''))
        count += 1

    for c in S.CASES:
        record(*S.query_args(c))
        record(*S.query_args(c, n=S.N_PF))
    for _, kind, t, sd, ad, depth, factors in S.REFUSED:
        record(kind, 3, t, t, sd, ad, depth, 10, 1 << 40, 1, 1 if factors else 0)
    for sd, ad, t, kind, depth, align, factors, n in itertools.product(
            (2, 3, 17, 60, 211), (1, 8, 20), (2, 5, 10, 11, 200), (0, 1, 2, 3), (0, 1, 2, 3), (1, 0), (0, 1),
            (5, S.N_PF)):
        if (depth and kind != 3) or (factors and kind not in (1, 2)):
            continue
        width = int(lib.bsig_summary_dim(kind, t, sd, ad, depth))
        if factors:
            w = S.window(t, sd)
            width = w * (sd - 1) + w * ad + 3
        for ld in (-(-width // 4) * 4, width + 1, width - 1):
            record(kind, n, t, max(t - 1, 1), sd, ad, depth, 10, ld, align, factors)
    print('host: %d queries  sha256 %s' % (count, digest.hexdigest()))


def _inputs(torch, n, t, ta, sd, ad, dtype):
    gen = torch.Generator().manual_seed(1000 * n + 100 * t + 10 * sd + ad)
    s, a = torch.randn(n, t, sd, dtype=torch.float64, generator=gen), torch.randn(n, ta, ad, dtype=torch.float64,
                                                                                  generator=gen)
    return s.to(dtype).to('cuda:0'), a.to(dtype).to('cuda:0')


def _shapes():
    seen, shapes = set(), []
    for c in S.CASES:
        n = min(c.n, N_BIG)
        shapes.append((c.name, (n, c.t, c.ta, c.sd, c.ad), c.max_t))
    for shp in F64_SHAPES + [(N_BIG, 2, 2, 1, 1), (N_BIG, 4, 4, 3, 1), (N_BIG, 8, 8, 34, 1)]:
        shapes.append(('f64_n%d_t%d_%d_sd%d_ad%d' % shp, shp, 10))
    for name, shp, max_t in shapes:
        if shp not in seen:
            seen.add(shp)
            yield name, shp, max_t


def device(only):
    import torch
    import bayes_sim_ig_amd as B
    _lib.require_gpu()

    def sha(fn, n, elems, dtype):
        """fn(out=...) into a fresh buffer, an aligned view of even pitch, a view one element in of odd pitch"""
        parts = []
        try:
            plain = fn(out=None)
        except (NotImplementedError, AssertionError, RuntimeError, ValueError) as e:
            return type(e).__name__
        width = plain.shape[1]
        for off, pitch in ((0, -(-width // elems) * elems + 2 * elems), (1, -(-width // 2) * 2 + 3)):
            buf = torch.full(((n + 1) * pitch + off + 8,), float('nan'), dtype=dtype, device='cuda:0')
            view = buf[off:off + n * pitch].view(n, pitch)[:, :width]
            fn(out=view)
            parts.append(buf)
        torch.cuda.synchronize()
        h = hashlib.sha256(plain.contiguous().cpu().numpy().tobytes())
        for p in parts:
            h.update(p.cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    for name, (n, t, ta, sd, ad), max_t in _shapes():
        if only and only not in name:
            continue
        for dtype, tag in ((torch.float32, 'fp32'), (torch.float64, 'fp64')):
            s, a = _inputs(torch, n, t, ta, sd, ad, dtype)
            kw = dict(dtype=dtype) if dtype == torch.float64 else {}
            elems = 16 // s.element_size()
            cols = ['start ' + sha(lambda out: B.summary_start(s, a, max_t=max_t, out=out, **kw), n, elems, dtype)]
            if sd >= 2 and t > 1:
                cols.append('corr ' + sha(lambda out: B.summary_corr(s, a, out=out, **kw), n, elems, dtype))
                cols.append('corrdiff ' + sha(lambda out: B.summary_corrdiff(s, a, out=out, **kw), n, elems, dtype))
            if t == ta and t >= 2:
                for depth in (1, 2, 3):
                    if (1 + sd + ad) ** depth <= 40000:
                        cols.append('sig%d ' % depth + sha(
                            lambda out: B.summary_signatory(s, a, depth=depth, out=out, **kw), n, elems, dtype))
            print('%-28s %s  %s' % (name, tag, '  '.join(cols)), flush=True)


# the double kernels' timed shapes: (what, n, L, sd, ad)
TIMED = [('corrdiff', 4096, 200, 3, 1), ('corrdiff', 4096, 200, 28, 8), ('signature3', 4096, 3, 18, 3)]


def timing():
    import torch
    import bayes_sim_ig_amd as B
    _lib.require_gpu()
    for what, n, t, sd, ad in TIMED:
        s, a = _inputs(torch, n, t, t, sd, ad, torch.float64)
        fn = B.summary_corrdiff if what == 'corrdiff' else B.summary_signatory
        out = fn(s, a, dtype=torch.float64).clone()
        kw = dict(check_finite=False) if what == 'corrdiff' else {}
        for _ in range(3):
            fn(s, a, out=out, dtype=torch.float64, **kw)
        torch.cuda.synchronize()
        reps = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(s, a, out=out, dtype=torch.float64, **kw)
            e1.record()
            e1.synchronize()
            reps.append(e0.elapsed_time(e1) * 1e3)
        print('%-10s n=%d L=%d sd=%d ad=%d fp64  median %.1f us  slowest %.1f  fastest %.1f  all %s'
              % (what, n, t, sd, ad, sorted(reps)[4], max(reps), min(reps), ' '.join('%.1f' % r for r in reps)),
              flush=True)


if __name__ == '__main__':
    if '--host' in sys.argv:
        host()
    elif '--time' in sys.argv:
        timing()
    else:
        device(sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None)
