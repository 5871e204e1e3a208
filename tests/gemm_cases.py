"""The case table of the fp32 GEMM tests (tests/test_gemm_cases_host.py, tests/test_gpu_gemm_routes.py):
one row per call of bsig_gemm_f32 with the route gemm_run (csrc/gemm_f32.hip) takes for it -- the
(kernel id, tile m, tile n, K slices) bsig_debug_gemm_path must report.  The expectations are written
down from the rules of plan_gemm / gemm_run, not read back from the library: a planner change that moves
a row to another route fails the host test before any GPU test runs on the wrong kernel.

Operand storage of a row (what the GPU helper builds):
    k-contiguous  [rows, k]  at a pitch of lda / ldb floats (0: k)
    k-major       [k, rows]  at a pitch of lda / ldb floats (0: A ceil16(m), B n -- the dense forms
                             bsig_debug_gemm_path assumes)
    gather        'a' / 'b' / 'ab': the rows of a k-contiguous operand or the contraction index of a
                  k-major one go through an index vector with repeated and out-of-order entries
The pitch beyond the operand is filled with NaN: no kernel may let it reach an output."""
import collections

# csrc/gemm_split_bf16.h
MFMA, LEAN, WIDE_FORWARD, WIDE_GRADIENT, F64ACC = range(5)
KERNEL_NAMES = {MFMA: 'mfma', LEAN: 'lean', WIDE_FORWARD: 'wide_fwd', WIDE_GRADIENT: 'wide_grad', F64ACC: 'f64acc'}
EPI_NONE, EPI_BIAS = 0, 1
BK = 32
TILES = [(64, 64), (128, 128), (128, 32), (128, 64), (128, 96), (96, 128)]     # BSIG_GEMM_TILE = 0..5
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
WIDE = 272                                                                    # ceil16 of the head widths 257..272

Case = collections.namedtuple('Case', [
    'group',        # the test parameter this row runs under
    'm', 'n', 'k', 'akm', 'bkm',
    'gather',       # '', 'a', 'b', 'ab'
    'lda', 'ldb',   # 0: dense (see above)
    'epi',          # the epilogue that is part of the route (the wide forward takes NONE and BIAS only)
    'env',          # environment switches around the call, all read per call
    'ws',           # workspace bytes; None: what bsig_gemm_workspace_bytes asks for
    'c_offset',     # also run with c one float off a 16-byte boundary
    'kernel', 'tile_m', 'tile_n', 'splits',      # what bsig_debug_gemm_path must report
    'kernel_from_debug',   # False: the debug entry assumes dense aligned operands and cannot name the kernel
])


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def slices(k, asked):
    """K slices of `asked` wanted ones: whole BK steps per slice, no empty slice (plan_gemm's last lines)"""
    chunk = round_up(ceil_div(k, max(asked, 1)), BK)
    return max(ceil_div(k, chunk), 1)


def pitches(c):
    lda = c.lda or (round_up(c.m, 16) if c.akm else c.k)
    ldb = c.ldb or (c.n if c.bkm else c.k)
    return lda, ldb


def lean_ok(c):
    """gemm_run's rule: both operands move as aligned 16-byte items (the storage itself is 16-byte aligned)"""
    lda, ldb = pitches(c)
    return lda % 4 == 0 and ldb % 4 == 0


def _case(group, m, n, k, akm=0, bkm=0, gather='', lda=0, ldb=0, epi=EPI_NONE, env=None, ws=None,
          c_offset=False, kernel=None, tile=None, splits=1, kernel_from_debug=True):
    c = Case(group, m, n, k, akm, bkm, gather, lda, ldb, epi, dict(env or {}), ws, c_offset, kernel,
             tile[0], tile[1], splits, kernel_from_debug)
    if kernel is None:      # a generic route: the lean kernel wherever it may run
        c = c._replace(kernel=LEAN if c.env.get('BSIG_GEMM_LEAN', '1') != '0' and lean_ok(c) else MFMA)
    return c


CASES = []

# ---- generic kernels: both kernels x forced tiles 0..5 x four layouts x 1 / 3 slices x direct / gathered
# (300, 260, 530) ragged in M, N and K for every tile; (129, 97, 64) a full tile plus a one-row and a
# one-column remainder; (1, 1, 1); (33, 65, 31) k < BK; (128, 128, 32) no edge at all.
# With BSIG_GEMM_LEAN=1 the lean kernel runs where lean_ok holds (k-contiguous operands: k % 4 == 0;
# k-major B: n % 4 == 0) and gemm_mfma_kernel elsewhere -- the unaligned-quad or the scalar loader.
# (A gathered k-major operand on a 96-row tile -- A on tile 5, B on tile 4 -- is handed back by
# launch_lean (LeanLoader::kSame) and runs gemm_mfma_kernel, bit-identical by construction; the debug
# entry takes no note of which operand is gathered and reports LEAN for it.)
GENERIC_SHAPES = [(300, 260, 530), (129, 97, 64), (1, 1, 1), (33, 65, 31), (128, 128, 32)]
for (m, n, k) in GENERIC_SHAPES:
    for lean in ('0', '1'):
        for tile in range(6):
            for li, (akm, bkm) in enumerate(LAYOUTS):
                for want in (1, 3):
                    for gather in ('', 'ab'):
                        env = {'BSIG_GEMM_LEAN': lean, 'BSIG_GEMM_TILE': str(tile), 'BSIG_GEMM_SPLITS': str(want)}
                        # the workspace holds exactly the slabs of the forced split: the guard behind it is sharp
                        CASES.append(_case('generic-%dx%dx%d-lean%s' % (m, n, k, lean), m, n, k, akm, bkm, gather,
                                           env=env, ws=4 * m * n * want if want > 1 else None,
                                           c_offset=(tile + li) % 3 == 0, tile=TILES[tile], splits=slices(k, want)))

# ---- planner-chosen routes, nothing forced.  m <= 128 and n >= 64: 128 x 32 tiles, ceil(512 / 3) slices
# wanted, at most k / 128 = 2 taken; the fall-through: 64 x 64 tiles, 25 of them, ceil(512 / 25) = 21 slices
# wanted, at most 530 / 128 = 4 taken.  No workspace: one slice.
for (m, n, k, tile, want) in ((100, 96, 302, (128, 32), 2), (300, 260, 530, (64, 64), 4)):
    for (akm, bkm) in ((0, 0), (1, 1)):
        for ws in (None, 0):
            for lean in ('0', '1'):
                CASES.append(_case('planner', m, n, k, akm, bkm, env={'BSIG_GEMM_LEAN': lean}, ws=ws, c_offset=True,
                                   tile=tile, splits=slices(k, want) if ws is None else 1))

# ---- reduce kernels.  gemm_reduce_kernel: 27 slices (k = 859: k_chunk = 32, the last slice 27 long) walk
# its 16-, 8- and remainder branches in one run; k = 500 gives 8 slices of 64 (the last 52) and 16 of 32
# (the last 20).  gemm_reduce_adam4_kernel<false>: EPI_NONE, m n = 2^18, n % 4 == 0; n = 510: its scalar twin.
for (m, n, k, want) in ((33, 65, 859, 27), (33, 65, 500, 8), (33, 65, 500, 16), (130, 72, 859, 27)):
    for (akm, bkm) in LAYOUTS:
        tile = (128, 32) if m <= 128 else (64, 64)
        CASES.append(_case('reduce', m, n, k, akm, bkm, env={'BSIG_GEMM_SPLITS': str(want)}, ws=4 * m * n * want,
                           c_offset=akm == bkm, tile=tile, splits=want))
for n in (512, 510):
    for (akm, bkm) in ((0, 0), (1, 1)):
        CASES.append(_case('reduce-quads', 512, n, 256, akm, bkm, env={'BSIG_GEMM_SPLITS': '2'}, ws=4 * 512 * n * 2,
                           c_offset=akm == 1, tile=(64, 64), splits=2))

# ---- unaligned quads: k-contiguous operands at a pitch that is no multiple of 4 floats (the shifted last
# quad), A only, B only, both; pitches k and k + 1; k % 4 in {0, 1, 2, 3}; k < BK.  The other operand sits
# at an aligned pitch.  And a k-major operand at such a pitch (VEC = 1), and the scalar fallback of the
# k-contiguous ones (BSIG_GEMM_NO_UNALIGNED=1).
# bsig_debug_gemm_path assumes dense aligned operands: the kernel id of these rows is MFMA by gemm_run's
# lean_ok rule (an operand that does not move as aligned 16-byte items) and is not asserted through it.
for k in (4, 5, 30, 302, 303):
    for ld in (k, k + 1):
        if ld % 4 == 0:
            continue
        for which in ('a', 'b', 'ab'):
            for no_unal in ((False, True) if ld == k + 1 or k == 303 else (False,)):
                CASES.append(_case('unaligned', 100, 96, k, 0, 0, gather='a' if which == 'b' else '',
                                   lda=ld if 'a' in which else round_up(k, 4) + 4,
                                   ldb=ld if 'b' in which else round_up(k, 4),
                                   env={'BSIG_GEMM_NO_UNALIGNED': '1'} if no_unal else {}, c_offset=which == 'ab',
                                   kernel=MFMA, tile=(128, 32), splits=slices(k, k // 128), kernel_from_debug=False))
for (akm, bkm, lda, ldb) in ((1, 0, 101, 304), (0, 1, 304, 97), (1, 1, 113, 99), (1, 0, 101, 303)):
    CASES.append(_case('unaligned', 100, 96, 302, akm, bkm, gather='ab', lda=lda, ldb=ldb, kernel=MFMA,
                       tile=(128, 32), splits=2, kernel_from_debug=False))

# ---- whole-width forward: m = 2090 (>= 2048, ragged against the 64-row tile), the whole range of
# gemm_wide_covers, k = 1056 gives slices of unequal length (288, 288, 288, 192).  33 row tiles: the cost
# model takes min(8, k / 256) = 4 slices where the workspace holds them (slabs of m x 272 floats); a workspace
# of exactly one slab: 1 slice through the pitched reduce.  The same calls with BSIG_GEMM_WIDE=0: 64 x 64
# tiles, 165 of them, ceil(512 / 165) = 4 slices wanted, as many as the workspace holds [m, n] slabs of.
M_WIDE = 2090
for n in (257, 260, 272):
    for k in (1024, 1056):
        for epi in (EPI_NONE, EPI_BIAS):
            for gather in ('', 'a'):
                for slabs in (4, 1):
                    ws = 4 * M_WIDE * WIDE * slabs
                    CASES.append(_case('wide-forward-n%d' % n, M_WIDE, n, k, gather=gather, epi=epi, ws=ws,
                                       c_offset=(k == 1056 and gather == 'a'), kernel=WIDE_FORWARD, tile=(64, WIDE),
                                       splits=slices(k, slabs)))
                    CASES.append(_case('wide-forward-off-n%d' % n, M_WIDE, n, k, gather=gather, epi=epi, ws=ws,
                                       env={'BSIG_GEMM_WIDE': '0'}, tile=(64, 64),
                                       splits=slices(k, min(4, ws // (4 * M_WIDE * n)))))

# ---- whole-width gradient: A k-major at the padded pitch of 272 floats, B k-major with the contraction
# rows gathered, n a multiple of 64.  n / 64 = 1 or 3 column tiles: 1 / c + 0.02 c is least at c = 7 of
# min(8, k / 256) = 8; k = 2048 and 2080: seven slices of 320 (the last 128 / 160).  The workspace holds
# exactly the seven slabs.
for m in (257, 260, 272):
    for n in (64, 192):
        for k in (2048, 2080):
            CASES.append(_case('wide-gradient', m, n, k, 1, 1, gather='b', lda=WIDE, ws=4 * m * n * 7,
                               c_offset=(k == 2080), kernel=WIDE_GRADIENT, tile=(WIDE, 64), splits=7))
            if m == 260 and k == 2080:
                CASES.append(_case('wide-gradient', m, n, k, 1, 1, gather='b', lda=WIDE, ws=4 * m * n * 7,
                                   env={'BSIG_GEMM_WIDE': '0'}, tile=(64, 64), splits=slices(k, 7)))

# ---- the fp64-accumulating kernel: one thread per output, every layout, gathered and direct
for (akm, bkm) in LAYOUTS:
    for gather in ('', 'ab'):
        CASES.append(_case('f64acc', 33, 65, 130, akm, bkm, gather, env={'BSIG_DEBUG_F64_ACC_MIN_K': '1'},
                           c_offset=bool(gather), kernel=F64ACC, tile=(0, 0), splits=1))

GROUPS = sorted({c.group for c in CASES}, key=[c.group for c in CASES].index)


def group(name):
    return [c for c in CASES if c.group == name]


def case_id(c):
    return '%s %dx%dx%d akm%d bkm%d g[%s] ld(%d,%d) epi%d ws%s %s' % (
        c.group, c.m, c.n, c.k, c.akm, c.bkm, c.gather, c.lda, c.ldb, c.epi, c.ws,
        ' '.join('%s=%s' % (key[5:], v) for key, v in sorted(c.env.items())))
