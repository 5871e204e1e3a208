"""CPU-side check of the fp32 GEMM case table (tests/gemm_cases.py): bsig_debug_gemm_path, called as
tests/test_matmul_host.py calls it with the row's environment set and restored, reports for every row the
kernel, tile and number of K slices the row expects -- and the table reaches every route, every tile shape
on both generic kernels and every slice count it claims, so the GPU tests of tests/test_gpu_gemm_routes.py
run what they say they run."""
import ctypes
import os

import pytest

import gemm_cases as G

from bayes_sim_ig_amd import _lib


def _path(m, n, k, akm=0, bkm=0, gathered=0, epi=0, ws=0):
    out = (ctypes.c_int32 * 8)()
    rc = _lib.load().bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, ws, _lib.MATMUL_FP32, out)
    assert rc == 0, _lib.load().bsig_last_error()
    return dict(zip(('kernel', 'tile_m', 'tile_n', 'splits', 'k_chunk', 'workgroups', 'declined'), list(out)[:7]))


def _report(c, monkeypatch):
    for key in ('BSIG_GEMM_TILE', 'BSIG_GEMM_SPLITS', 'BSIG_GEMM_LEAN', 'BSIG_GEMM_WIDE', 'BSIG_DEBUG_F64_ACC_MIN_K',
                'BSIG_GEMM_NO_LARGE_PLAN', 'BSIG_GEMM_NO_UNALIGNED'):
        monkeypatch.delenv(key, raising=False)
    for key, val in c.env.items():
        monkeypatch.setenv(key, val)
    ws = int(_lib.load().bsig_gemm_workspace_bytes(c.m, c.n, c.k)) if c.ws is None else c.ws
    return _path(c.m, c.n, c.k, c.akm, c.bkm, int(bool(c.gather)), c.epi, ws)


@pytest.mark.parametrize('group', G.GROUPS)
def test_every_row_takes_its_route(group, monkeypatch):
    rows = G.group(group)
    assert rows
    for c in rows:
        got = _report(c, monkeypatch)
        if c.kernel_from_debug:
            assert got['kernel'] == c.kernel, (G.case_id(c), got)
        else:
            # unaligned operands: gemm_run keeps them off the lean kernel; the debug entry takes them as dense
            assert c.kernel == G.MFMA and got['kernel'] in (G.MFMA, G.LEAN), (G.case_id(c), got)
        assert (got['tile_m'], got['tile_n'], got['splits']) == (c.tile_m, c.tile_n, c.splits), (G.case_id(c), got)
        assert got['declined'] == 0
        if c.kernel != G.F64ACC:
            assert got['k_chunk'] % G.BK == 0 and got['k_chunk'] * (got['splits'] - 1) < c.k <= got['k_chunk'] * got['splits']
        if c.ws is not None and c.kernel not in (G.F64ACC,):      # the slabs fit the workspace the row hands over
            slab = c.m * (G.WIDE if c.kernel == G.WIDE_FORWARD else c.n)
            assert c.splits == 1 and c.kernel != G.WIDE_FORWARD or 4 * slab * c.splits <= c.ws, G.case_id(c)


def test_the_table_reaches_what_it_claims(monkeypatch):
    reported = [(c, _report(c, monkeypatch)) for c in G.CASES]
    kernels = {got['kernel'] for _, got in reported}
    assert kernels == {G.MFMA, G.LEAN, G.WIDE_FORWARD, G.WIDE_GRADIENT, G.F64ACC}
    for kernel in (G.MFMA, G.LEAN):
        tiles = {(got['tile_m'], got['tile_n']) for c, got in reported if got['kernel'] == kernel and c.kernel_from_debug}
        assert tiles == set(G.TILES), (kernel, tiles)
        # ... and every tile runs one slice and three on each of them
        for tile in G.TILES:
            assert {1, 3} <= {got['splits'] for _, got in reported
                              if got['kernel'] == kernel and (got['tile_m'], got['tile_n']) == tile}, (kernel, tile)
    assert {1, 3, 8, 16, 27} <= {got['splits'] for _, got in reported}
    # every layout, direct and gathered, on both generic kernels
    for kernel in (G.MFMA, G.LEAN):
        seen = {(c.akm, c.bkm, bool(c.gather)) for c, got in reported if got['kernel'] == kernel}
        assert seen == {(a, b, g) for (a, b) in G.LAYOUTS for g in (False, True)}, kernel
    # the whole-width rows report a generic route with BSIG_GEMM_WIDE=0, and take 1 slice on a one-slab workspace
    off = [got for c, got in reported if c.env.get('BSIG_GEMM_WIDE') == '0']
    assert off and all(got['kernel'] in (G.MFMA, G.LEAN) for got in off)
    assert {got['splits'] for c, got in reported if got['kernel'] == G.WIDE_FORWARD} == {1, 4}
    # the planner rows without a workspace take one slice
    assert all(got['splits'] == 1 for c, got in reported if c.ws == 0)
    assert any(c.ws == 0 for c in G.CASES)


def test_a_forced_tile_that_is_not_built_is_refused(monkeypatch):
    """BSIG_GEMM_TILE indexes the tile table: a value beyond it, or (in a build without the whole-width tiles)
    one of its two empty entries, is an error that names the value -- not a read past the table or another
    tile's kernel on this tile's slice count."""
    lib = _lib.load()
    out = (ctypes.c_int32 * 8)()
    before = os.environ.get('BSIG_GEMM_TILE')
    for key in ('BSIG_GEMM_SPLITS', 'BSIG_DEBUG_F64_ACC_MIN_K'):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv('BSIG_GEMM_TILE', '7')
    wide_tiles_built = lib.bsig_debug_gemm_path(300, 260, 530, 0, 0, 0, 0, 0, _lib.MATMUL_FP32, out) == 0
    for value in ('8', '1000') + (() if wide_tiles_built else ('6', '7')):
        monkeypatch.setenv('BSIG_GEMM_TILE', value)
        assert lib.bsig_debug_gemm_path(300, 260, 530, 0, 0, 0, 0, 0, _lib.MATMUL_FP32, out) == _lib.BSIG_EINVAL
        message = lib.bsig_last_error().decode()
        assert 'BSIG_GEMM_TILE=%s ' % value in message and ('0..7' if wide_tiles_built else '0..5') in message, message
        assert list(out) == [0] * 8
    monkeypatch.setenv('BSIG_GEMM_TILE', '5')
    assert _path(300, 260, 530)['tile_m'] == 96
    monkeypatch.undo()
    assert os.environ.get('BSIG_GEMM_TILE') == before


def test_the_table_keeps_the_shapes_the_edges_need():
    shapes = {(c.m, c.n, c.k) for c in G.CASES}
    assert set(G.GENERIC_SHAPES) <= shapes
    assert {(100, 96, k) for k in (4, 5, 30, 302, 303)} <= shapes
    assert {(G.M_WIDE, n, k) for n in (257, 260, 272) for k in (1024, 1056)} <= shapes
    assert {(m, n, k) for m in (257, 260, 272) for n in (64, 192) for k in (2048, 2080)} <= shapes
    assert {(512, 512, 256), (512, 510, 256), (33, 65, 130)} <= shapes
    unal = [c for c in G.CASES if c.group == 'unaligned' and not c.akm and not c.bkm]
    assert {k % 4 for c in unal for k in [c.k]} == {0, 1, 2, 3}
    assert {(c.lda % 4 != 0, c.ldb % 4 != 0) for c in unal} == {(True, False), (False, True), (True, True)}
    assert {c.lda - c.k for c in unal if c.lda % 4} == {0, 1}
    assert any(c.env.get('BSIG_GEMM_NO_UNALIGNED') == '1' for c in unal)
    assert not os.environ.get('BSIG_GEMM_TILE')           # nothing of a row's environment is left behind
