"""Timing of the summaries with per-trajectory lengths (include/bsig_ragged.h) for profiles/ragged_NOTES.md, by the
method of tools/signature_ex_timing.py -- HIP events, a warm-up, median and range of REPS repeats, the variants of
a comparison alternating in one process -- with INNER launches between two events, so that a window is
milliseconds, not one short launch.  N = 32 000 trajectories at the README's Pendulum (3, 1, T 21), Ant (60, 8,
T 50) and ShadowHand (211, 20, T 50) shapes, in fp32 and in double, summary_xcorr at lag 0 and summary_kme with 256
features; no read-back in any of them.

    python tools/ragged_timing.py --parent PATH/libbsig_hip.so

``--parent``: the library built from the PARENT commit (BSIG_OUT_DIR=... ./build.sh in a checkout of it), loaded
next to this commit's in the same process.  Per shape, on the same inputs:
  (i)   the ragged entry point with every length = ts  /  the parent's fixed-length entry point;
  (ii)  the ragged entry point with lengths uniform in [ts / 4, ts]  /  the same two;
  (iii) this commit's fixed-length entry point  /  the parent's (the templates are shared: did their code move?);
and the run-to-run spread, (max - min) / median of the parent's launches.  The outputs of the parent's, this
commit's and the all-lengths-ts launch are compared bit for bit first.

``--stats xcorr|kme TASK fp32|fp64``: the four launches of one shape alone, five times each, for a
``rocprofv3 --kernel-trace --stats`` run of its own (the parent's kernel and this commit's carry different names:
the template has one argument more)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

N = 32000
N_FEAT = 256
INNER = 10
SHAPES = (('Pendulum', 3, 1, 21), ('Ant', 60, 8, 50), ('ShadowHand', 211, 20, 50))


def parent_library(path):
    """The parent commit's build with the prototypes of the four fixed-length entry points."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for header, names in (('bsig_xcorr.h', ('bsig_xcorr', 'bsig_xcorr_f64')), ('bsig_kme.h', ('bsig_kme', 'bsig_kme_f64'))):
        for name in names:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = B._lib.HEADERS[header][name]
    assert not hasattr(lib, 'bsig_xcorr_ragged'), 'this is not the parent commit: it has the ragged entry points'
    return lib


def variants(summary, sd, ad, length, dtype, parent):
    """{name: (launch(), its output)} of one shape, and what the launches share."""
    _lib, lib = B._lib, B._lib.load()
    prec = _lib.F64 if dtype == torch.float64 else _lib.F32
    f64 = '_f64' if prec.itemsize == 8 else ''
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV).to(dtype)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV).to(dtype)
    whole = torch.full((N,), length, dtype=torch.int32, device=DEV)
    mixed = torch.randint(max(length // 4, 2), length + 1, (N,), generator=gen).to(torch.int32).to(DEV)
    ptr, st = _lib.ptr, _lib.stream()
    if summary == 'xcorr':
        width = B.xcorr_dim(sd, ad, 0)
        ld = _lib.round_up(width, 16 // prec.itemsize)
        tail = (N, length, length, sd, ad, 0, 1, ld, None, st)

        def fixed(which, out):
            fn = getattr(which, 'bsig_xcorr' + f64)
            return lambda: _lib.check(fn(ptr(states), ptr(actions), ptr(out), *tail))

        def ragged(lengths, out):
            fn = getattr(lib, 'bsig_xcorr_ragged' + f64)
            return lambda: _lib.check(fn(ptr(states), ptr(actions), ptr(lengths), ptr(out), *tail))
    else:
        width = N_FEAT
        ld = _lib.round_up(width, 16 // prec.itemsize)
        emb = B.KernelMeanEmbedding(sd, ad, n_feat=N_FEAT, device=DEV).fit_scale(states, actions, dtype=dtype)
        coeff = emb.coefficients(dtype)
        tail = (N, length, length, sd, ad, N_FEAT // 2, 1, 0, ld, None, st)

        def fixed(which, out):
            fn = getattr(which, 'bsig_kme' + f64)
            return lambda: _lib.check(fn(ptr(states), ptr(actions), ptr(coeff), coeff.stride(0), ptr(out), *tail))

        def ragged(lengths, out):
            fn = getattr(lib, 'bsig_kme_ragged' + f64)
            return lambda: _lib.check(fn(ptr(states), ptr(actions), ptr(lengths), ptr(coeff), coeff.stride(0), ptr(out),
                                         *tail))
    outs = {k: torch.zeros(N, ld, dtype=dtype, device=DEV) for k in ('parent', 'fixed', 'ragged_whole', 'ragged_mixed')}
    fns = {'parent': fixed(parent, outs['parent']), 'fixed': fixed(lib, outs['fixed']),
           'ragged_whole': ragged(whole, outs['ragged_whole']), 'ragged_mixed': ragged(mixed, outs['ragged_mixed'])}
    keep = (states, actions, whole, mixed, outs)
    return fns, outs, width, keep


def one_shape(summary, task, precision, parent):
    sd, ad, length = {name: (sd, ad, length) for name, sd, ad, length in SHAPES}[task]
    fns, _, _, keep = variants(summary, sd, ad, length, torch.float64 if precision == 'fp64' else torch.float32, parent)
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()


def main(argv):
    assert '--parent' in argv, __doc__
    parent = parent_library(argv[argv.index('--parent') + 1])
    if '--stats' in argv:
        return one_shape(*argv[argv.index('--stats') + 1:][:3], parent)
    print('# csrc: %s' % csrc_hash())
    print('# %s, N = %d, %d repeats of %d launches; us per launch: median (min .. max)'
          % (torch.cuda.get_device_name(0), N, REPS, INNER))
    for summary in ('xcorr', 'kme'):
        for task, sd, ad, length in SHAPES:
            for dtype in (torch.float32, torch.float64):
                fns, outs, width, keep = variants(summary, sd, ad, length, dtype, parent)
                for fn in fns.values():
                    fn()
                torch.cuda.synchronize()
                same = all(torch.equal(outs['parent'][:, :width].view(torch.uint8), outs[k][:, :width].view(torch.uint8))
                           for k in ('fixed', 'ragged_whole'))
                assert torch.isfinite(outs['ragged_mixed'][:, :width]).all()
                res = timed({k: (lambda fn=fn: [fn() for _ in range(INNER)]) for k, fn in fns.items()})
                res = {k: tuple(v / INNER for v in r) for k, r in res.items()}
                par = res['parent']
                print('%s %s T %d %s: parent %.1f (%.1f .. %.1f), spread %.1f %%; fixed %.1f (%.1f .. %.1f); ragged, all = ts '
                      '%.1f (%.1f .. %.1f); ragged, ts/4 .. ts %.1f (%.1f .. %.1f); (i) %.3f  (ii) %.3f of the parent, '
                      '%.3f of all = ts  (iii) %.3f; parent, fixed and all = ts bitwise equal: %s'
                      % ((summary, task, length, 'fp64' if dtype == torch.float64 else 'fp32') + par +
                         (100.0 * (par[2] - par[1]) / par[0],) + res['fixed'] + res['ragged_whole'] + res['ragged_mixed'] +
                         (res['ragged_whole'][0] / par[0], res['ragged_mixed'][0] / par[0],
                          res['ragged_mixed'][0] / res['ragged_whole'][0], res['fixed'][0] / par[0], same)), flush=True)
                del fns, outs, keep
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1:])
