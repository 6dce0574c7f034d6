"""The GEMM tile table of csrc/gemm.hip (kTiles) and the automatic tile choice, asked of the library without a device
(nnr_gemm_tile_info, nnr_gemm_tile_for: host-only, they dereference nothing, so A / B / C are fake aligned addresses).  The expected
ids, shapes and names are written out here as an independent statement: the literals the host side carried before it read the table,
and tile choices derived by hand from the chain in choose_tile."""
import ctypes as C

import pytest

from nnr_amd import _lib as L, ops, profile

# id -> (rows, cols, bk or None where no earlier statement existed, profile suffix, {layout: kernel as rocprofv3 prints it})
TILES = {
    2: (64, 80, 16, '64x80', {'nt': 'gemm_kernel<1, 5, false, false, 16>', 'nn': 'gemm_kernel<1, 5, false, true, 16>', 'tn': 'gemm_kernel<1, 5, true, true, 16>'}),
    3: (128, 208, 16, '128x208', {'nt': 'gemm_kernel<2, 13, false, false, 16>'}),
    4: (128, 80, 16, '128x80', {'nt': 'gemm_kernel<2, 5, false, false, 16>', 'nn': 'gemm_kernel<2, 5, false, true, 16>', 'tn': 'gemm_kernel<2, 5, true, true, 16>'}),
    5: (128, 80, 32, '128x80k32', {'nt': 'gemm_kernel<2, 5, false, false, 32>'}),
    6: (64, 80, 64, '64x80k64', {'nt': 'gemm_kernel<1, 5, false, false, 64>', 'nn': 'gemm_kernel<1, 5, false, true, 64>', 'tn': 'gemm_kernel<1, 5, true, true, 64>'}),
    7: (16, 80, None, '16x80skinny', {}),
    9: (128, 80, None, 'pipe2_128x80', {'nt': 'gemm_nt_pipe2_kernel<2, 5, 3, 2>'}),
    15: (128, 80, None, 'pipe128x80', {'nt': 'gemm_nt_pipe_kernel<2, 5, 16, 3, 4>'}),        # (was '..., 4, 0>' while the kernel had its PRIO parameter)
    16: (128, 80, None, 'pipe128x80s2', {'nt': 'gemm_nt_pipe_kernel<2, 5, 16, 2, 5>'}),      # (was '..., 5, 0>')
    20: (128, 80, 16, 'pipe128x80', {'tn': 'gemm_tn_pipe_kernel<2, 5, 3, 3>'}),              # (was '..., 3, 0>')
    26: (128, 80, 16, 'pipe2_128x80', {'tn': 'gemm_tn_pipe2_kernel<2, 5, 3, 3>'}),
    27: (128, 208, 16, 'pipe2_128x208', {'tn': 'gemm_tn_pipe2_kernel<2, 13, 3, 2>'}),
    30: (128, 160, 16, 'pipe2_128x160', {'tn': 'gemm_tn_pipe2_kernel<2, 10, 3, 2>'}),
    32: (64, 208, 16, 'pipe2_64x208', {'tn': 'gemm_tn_pipe2_kernel<1, 13, 3, 2>'}),
    50: (128, 80, None, 'bx3_128x80', {'nt': 'gemm_nt_bx3_kernel<2, 5, 2>'}),
    51: (64, 80, None, 'bx3_64x80', {'nt': 'gemm_nt_bx3_kernel<1, 5, 2>'}),
}
PA, PB, PC, PX = 0x10000, 0x20000, 0x30000, 0x40000        # fake device addresses, 16-byte aligned


def test_table_states_every_live_tile_once():
    index, ids = 0, []
    dims, suffix, kernel = (C.c_int * 6)(), C.create_string_buffer(64), C.create_string_buffer(64)
    while True:
        rcs = [L.lib().nnr_gemm_tile_info(index, ta, tb, dims, suffix, kernel, 64) for ta, tb in ((0, 0), (0, 1), (1, 1))]
        if L.NNR_ERR_ARG in rcs:
            break
        assert 0 in rcs and set(rcs) <= {0, L.NNR_ERR_UNSUPPORTED}
        ids.append(dims[0])
        index += 1
    assert ids == sorted(TILES) and len(ids) == 16
    tiles = L.gemm_tiles()
    assert sorted(tiles) == sorted(TILES)
    for tid, (rows, cols, bk, sfx, kern) in TILES.items():
        t = tiles[tid]
        assert (t.rows, t.cols, t.suffix) == (rows, cols, sfx), tid
        assert bk is None or t.bk == bk, tid
        for lay, k in kern.items():
            assert t.kernels[lay] == k and profile.KERNEL_OF['gemm_%s_%s' % (lay, sfx)] == k, (tid, lay)
    assert set(tiles[7].kernels) == {'nt', 'nn'} and not any(tiles[7].kernels.values())      # the skinny tile picks its wave count per launch
    assert all(set(tiles[t].kernels) == {'nt', 'nn', 'tn'} for t in (2, 3, 4, 5, 6))
    assert all(set(tiles[t].kernels) == {'nt'} for t in (9, 15, 16, 50, 51)) and all(set(tiles[t].kernels) == {'tn'} for t in (20, 26, 27, 30, 32))
    assert {tiles[t].occ for t in (20, 26)} == {3} and {tiles[t].occ for t in (27, 30, 32)} == {2}      # = the kernels' launch bounds: the slab reduction's slots
    gone = {'gemm_nt_256x80', 'gemm_nn_256x80', 'gemm_tn_256x80', 'gemm_nt_pipe2_128x64', 'gemm_tn_pipe128x208'}
    assert not gone & set(profile.KERNEL_OF) and profile.KERNEL_OF['lstm_bwd'] == 'lstm_bwd_pair_kernel<13, true>'


def test_tn_tile_returns_the_tuples_it_always_did():
    assert ops.tn_tile(900, 900, 4352) == (26, 128, 80, 2048)
    assert ops.tn_tile(400, 400, 5000) == (0, 64, 80, 2048)
    assert ops.tn_tile(1664, 300, 20000) == (30, 128, 160, 2048)
    assert ops.tn_tile(200, 400, 20000) == (32, 64, 208, 640) and ops.tn_tile(832, 200, 20000, gather=True) == (32, 64, 208, 640)
    assert ops.tn_tile(256, 200, 20000) == (27, 128, 208, 640)
    assert ops.tn_tile(832, 256, 20000, gather=True) == (20, 128, 80, 2048)
    assert ops.tn_tile(512, 256, 20000) == (26, 128, 80, 2048)


def _args(M, N, K, tn=False, **kw):
    """NT with lda = ldb = K, ldc = N unless stated; tn: A [K, M], B [K, N]."""
    g = L.GemmArgs()
    g.A, g.B, g.C, g.M, g.N, g.K, g.ldc, g.alpha, g.split_k, g.batch = PA, PB, PC, M, N, K, N, 1.0, 1, 1
    g.lda, g.ldb = (M, N) if tn else (K, K)
    g.trans_a = g.trans_b = int(tn)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


CHOICE = [
    (dict(M=320, N=400, K=400), 7),
    (dict(M=320, N=400, K=400, drop_target=3, drop_p=0.2, drop_cols=400), 7),
    (dict(M=320, N=400, K=60), 2),
    (dict(M=320, N=400, K=400, pre_add=PX, ldpre=400), 6),
    (dict(M=2000, N=400, K=400, a_idx=PX), 6),
    (dict(M=32768, N=80, K=128), 7),
    (dict(M=32769, N=80, K=128), 16),
    (dict(M=4352, N=900, K=400), 16),
    (dict(M=4352, N=900, K=900), 9),
    (dict(M=4352, N=900, K=900, a_idx=PX), 16),
    (dict(M=4352, N=400, K=400, dyn_dev=PX, dyn_dim=1), 15),
    (dict(M=65536, N=400, K=400), 15),
    (dict(M=65536, N=400, K=402), 5),
    (dict(M=65536, N=400, K=400, trans_b=1, ldb=400), 4),
    (dict(M=2000, N=400, K=4000, k_chunk=512, atomic=1), 5),
    (dict(M=1000, N=200, K=400, rowdot_w=PX, rowdot_out=PX + 0x1000), 3),
    (dict(M=400, N=400, K=5000, tn=True, split_k=8, atomic=1), 2),
    (dict(M=1664, N=300, K=20000, tn=True, split_k=16, atomic=1), 2),
]


@pytest.mark.parametrize('kw, tile', CHOICE, ids=['-'.join(k if v >= PA else '%s%s' % (k, v) for k, v in kw.items()) for kw, _ in CHOICE])
def test_automatic_choice(kw, tile):
    assert L.lib().nnr_gemm_tile_for(C.byref(_args(**kw))) == tile


def test_explicit_tiles_pass_their_predicate_or_are_refused():
    q = L.lib().nnr_gemm_tile_for
    tn = dict(M=400, N=400, K=20000, tn=True, split_k=8, atomic=1)
    assert q(C.byref(_args(tile=26, **tn))) == 26
    assert q(C.byref(_args(tile=26, b_idx=PX, **tn))) == L.NNR_ERR_ARG
    assert q(C.byref(_args(tile=20, b_idx=PX, **tn))) == 20
    nt = dict(M=4352, N=400, K=400)
    assert q(C.byref(_args(tile=50, B3=PX, ldb3=400, b3_stride=400 * 400, **nt))) == 50
    assert q(C.byref(_args(tile=50, **nt))) == L.NNR_ERR_ARG
    assert q(C.byref(_args(tile=9, **nt))) == 9
    assert q(C.byref(_args(tile=9, a_idx=PX, **nt))) == L.NNR_ERR_ARG
    for unknown in (1, 8, 28, 29, 99):
        assert q(C.byref(_args(tile=unknown, **nt))) == L.NNR_ERR_ARG
    assert q(C.byref(_args(M=0, N=400, K=400))) == 0            # an empty product: nnr_gemm_f32 answers NNR_OK and launches nothing
    assert q(None) == L.NNR_ERR_ARG and q(C.byref(_args(k_chunk=48, **nt))) == L.NNR_ERR_ARG


def test_profile_family_is_the_launched_tile():
    """The four launch classes the profile's own copy of the choice named wrongly (or would have): small TN, C-element dropout on the
    skinny tile, pre_add, and k_chunk slices counted as ceil(K / k_chunk)."""
    assert ops.gemm_family(_args(**CHOICE[16][0])) == 'gemm_tn_64x80'
    assert ops.gemm_family(_args(**CHOICE[1][0])) == 'gemm_nt_16x80skinny'
    assert ops.gemm_family(_args(**CHOICE[3][0])) == 'gemm_nt_64x80k64'
    assert ops.gemm_family(_args(**CHOICE[14][0])) == 'gemm_nt_128x80k32'
    with pytest.raises(L.NnrHipError):
        ops.gemm_family(_args(M=320, N=400, K=400, tile=50))
