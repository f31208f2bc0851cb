"""ipnn_plan_query (include/ipnn_hip.h) through ipnn.plan_query: what ipnn_create would choose for a shape, computed without a
device.  The figures below are worked out by hand from the padded widths Dp = [rup(16 F + F (F - 1) / 2 + 2, 64),
rup(h + 1, 64) .., 64] and the tile rule of the strip kernels:

  forward, the whole stack    tile A holds layers 0, 2, 4 ..; tile B layers 1, 3, ..; the output unit is in no tile
  backward, the whole stack   tile A holds delta l_{L+1}, delta l_{L-1} ..; tile B delta l_L ..; layer 0 (dz1) is in no tile
  bytes                       a 32-example bf16 strip and a 16-example f32 strip both take 64 bytes per column: 64 (A + B),
                              at most 160 KiB = 2560 columns

Handles of up to 32 fields, and every layer 0 of at most 1024 columns, keep two equal tiles as wide as the widest layer.
"""
import ctypes as C

import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, ipnn
from deep_ctr_amd.engine import FNNError

L3, L7 = [400, 400, 200], [1000, 800, 600, 400, 200, 100, 50]
LAUNCHES = ('stack_fwd', 'stack_bwd', 'wide_fwd', 'wide_bwd', 'tail_fwd', 'tail_bwd', 'tail_fused')
LDS = 160 * 1024


def rup(a, m):
    return (a + m - 1) // m * m


def tiles(q, name):
    t = q[name]
    return t['cap_a'], t['cap_b'], t['lds_bytes']


@pytest.mark.parametrize("prec", ['bf16', 'f32'])
def test_fnn_ip_l3_at_39_fields_runs_strips(built, prec):
    """Dp = 1408, 448, 448, 256, 64.  Forward: A = max(1408, 448), B = max(448, 256): 1856 columns, 118,784 B.  Backward:
    A = max(64, 448), B = max(256, 448): 896 columns."""
    q = ipnn.plan_query(39, 11, L3, precision=prec)
    assert q['padded'] == [1408, 448, 448, 256, 64]
    assert q['strips'] and q['shares_step'] and q['shares_eval']
    assert tiles(q, 'stack_fwd') == (1408, 448, 118784)
    assert tiles(q, 'stack_bwd') == (448, 448, 57344)
    assert q['lds_max'] == 118784
    assert (q['rows_fwd'], q['rows_bwd']) == ('narrow', 'many')
    assert q['pairs'] == (prec == 'bf16')
    if prec == 'f32':                                       # no pairs, no split: five launches the handle never issues
        assert all(tiles(q, n) == (0, 0, 0) for n in LAUNCHES[2:])
    else:
        # cut = 2 (448 / 64 = 7 blocks, 256 / 64 = 4 < 5).  Wide forward: layers 0, 1, 2 (the last one leaves from its tile);
        # wide backward: delta l_2 in A, delta l_1 in B.  Tail over Dp[2..4] = 448, 256, 64 on 16-example strips (32 B a column):
        # forward A = 448, B = 256; backward A = max(64, 448), B = 256
        assert q['cut'] == 2
        assert tiles(q, 'wide_fwd') == (1408, 448, 118784) and tiles(q, 'wide_bwd') == (448, 448, 57344)
        assert tiles(q, 'tail_fwd') == tiles(q, 'tail_bwd') == tiles(q, 'tail_fused') == (448, 256, 32 * 704)


@pytest.mark.parametrize("prec", ['bf16', 'f32'])
def test_fnn_ip_l7_at_39_fields_runs_strips(built, prec):
    """Dp = 1408, 1024, 832, 640, 448, 256, 128, 64, 64.  Forward: A = 1408 (layers 0, 2, 4, 6), B = 1024 (1, 3, 5, 7): 2432
    columns, 155,648 B.  Backward: A = max(64, 128, 448, 832), B = max(64, 256, 640, 1024)."""
    q = ipnn.plan_query(39, 11, L7, precision=prec)
    assert q['strips'] and q['shares_step']
    assert tiles(q, 'stack_fwd') == (1408, 1024, 155648)
    assert tiles(q, 'stack_bwd') == (832, 1024, 64 * 1856)
    assert q['lds_max'] == 155648 <= LDS


@pytest.mark.parametrize("prec", ['bf16', 'f32'])
def test_exactly_2560_columns_fit(built, prec):
    """[1100] at 39 fields: Dp = 1408, 1152, 64: 2560 columns, the whole 160 KiB.  [1200]: 1216 -> 2624 columns, the GEMM path."""
    q = ipnn.plan_query(39, 11, [1100], precision=prec)
    assert q['strips'] and tiles(q, 'stack_fwd') == (1408, 1152, LDS) and tiles(q, 'stack_bwd') == (64, 1152, 64 * 1216)
    q = ipnn.plan_query(39, 11, [1200], precision=prec)
    assert q['padded'] == [1408, 1216, 64]
    assert not q['strips'] and not q['shares_step'] and not q['shares_eval']
    assert all(tiles(q, n) == (0, 0, 0) for n in LAUNCHES) and q['lds_max'] == 0


def test_a_layer_at_an_even_position_wider_than_layer_0(built):
    """[64, 1100, 64] at 33 fields: Dp = 1088, 128, 1152, 128, 64: layer 2 shares tile A with layer 0 and is the wider one."""
    q = ipnn.plan_query(33, 11, [64, 1100, 64])
    assert q['padded'] == [1088, 128, 1152, 128, 64]
    assert q['strips'] and tiles(q, 'stack_fwd') == (1152, 128, 64 * 1280)
    assert tiles(q, 'stack_bwd') == (1152, 128, 64 * 1280)           # A: 64, 1152; B: 128, 128


@pytest.mark.parametrize("F,K,hidden", [(43, 11, L7), (64, 4, [64]), (64, 16, L3)], ids=['F43-L7', 'F64-64', 'F64-L3'])
def test_shapes_that_do_not_fit_keep_the_gemm_path(built, F, K, hidden):
    """43 fields: Dp0 = rup(688 + 903 + 2, 64) = 1600, + 1024 = 2624 columns.  64 fields with pairs: Dp0 = 3072 alone."""
    for prec in ('bf16', 'f32'):
        q = ipnn.plan_query(F, K, hidden, precision=prec)
        assert q['padded'][0] == rup(16 * F + F * (F - 1) // 2 + 2, 64)
        assert not q['strips'] and not q['shares_step'] and not q['shares_eval'] and q['lds_max'] == 0
        # the 16-example forward's tile passes the LDS from 46 fields with pairs; the 4-example backward runs from 33
        assert (q['rows_fwd'], q['rows_bwd']) == ('many' if F >= 46 else 'narrow', 'many')


def test_16_fields_keep_two_equal_tiles(built, monkeypatch):
    """(16, 11, L7): Dp0 = 384 and the widest layer 1024: capA == capB == 1024 in every launch of whole strips, 128 KiB, as before
    the tiles had two widths; IPNN_STRIP_L0=0 changes nothing there."""
    ref, ref32 = ipnn.plan_query(16, 11, L7), ipnn.plan_query(16, 11, L7, precision='f32')
    assert ref32['strips'] and not ref32['pairs'] and tiles(ref32, 'stack_fwd') == tiles(ref32, 'stack_bwd') == (1024, 1024, 131072)
    assert ref['strips'] and ref['pairs'] and ref['shares_step'] and (ref['rows_fwd'], ref['rows_bwd']) == ('narrow', 'narrow')
    for n in ('stack_fwd', 'stack_bwd', 'wide_fwd', 'wide_bwd'):
        assert tiles(ref, n) == (1024, 1024, 131072), n
    # cut = 4 (448 / 64 = 7 blocks): the tail's widest layer is 448, two equal tiles on 16-example strips
    assert ref['cut'] == 4 and tiles(ref, 'tail_fused') == tiles(ref, 'tail_fwd') == tiles(ref, 'tail_bwd') == (448, 448, 2 * 32 * 448)
    assert not ipnn.plan_query(16, 11, [1100])['strips']              # a hidden layer too wide for equal tiles: as before
    monkeypatch.setenv('IPNN_STRIP_L0', '0')
    assert ipnn.plan_query(16, 11, L7) == ref
    assert ipnn.plan_query(16, 11, L7, precision='f32') == ref32


def test_strip_l0_knob_restores_the_gemm_path_above_32_fields(built, monkeypatch):
    cases = [(39, 11, L3), (39, 11, L7), (39, 11, [1100]), (33, 11, [64, 1100, 64]), (33, 1, [8]), (45, 16, [300, 70])]
    for F, K, hidden in cases:
        assert ipnn.plan_query(F, K, hidden)['strips'], (F, K, hidden)
    monkeypatch.setenv('IPNN_STRIP_L0', '0')
    for F, K, hidden in cases:
        q = ipnn.plan_query(F, K, hidden)
        assert not q['strips'] and not q['shares_step'] and not q['shares_eval'] and q['lds_max'] == 0, (F, K, hidden)
    monkeypatch.setenv('IPNN_STRIP', '0')
    monkeypatch.delenv('IPNN_STRIP_L0')
    assert not ipnn.plan_query(39, 11, L3)['strips'] and not ipnn.plan_query(16, 11, L7)['strips']


def test_sweep_over_the_field_counts(built):
    """F = 2 .. 64 at k = 4, 16 and (up to 32 fields) 20, hidden [300, 70], with and without pairs: the handle shares the group
    step's launches exactly when it runs strips on narrow rows; it runs strips exactly when the columns fit -- two equal tiles of
    the widest layer up to 32 fields and up to a layer 0 of 1024 columns, Dp0 + 320 <= 2560 above -- and no launch passes
    160 KiB."""
    for F in range(2, 65):
        for K in (4, 16, 20):
            if K > 16 and F > 32:
                with pytest.raises(FNNError):
                    ipnn.plan_query(F, K, [300, 70])
                continue
            for pairs in (True, False):
                rw = 16 if K <= 16 else rup(K, 4)
                Dp0 = rup(F * rw + (F * (F - 1) // 2 if pairs else 0) + 2, 64)
                q = ipnn.plan_query(F, K, [300, 70], pairs=pairs)
                assert q['padded'] == [Dp0, 320, 128, 64]
                assert q['strips'] == (Dp0 <= 1024 or (F > 32 and Dp0 + 320 <= 2560)), (F, K, pairs)
                assert q['shares_step'] == (q['strips'] and K <= 16), (F, K, pairs)
                assert q['shares_eval'] == q['strips']
                assert q['lds_max'] <= LDS and (q['lds_max'] > 0) == q['strips']
                if q['strips'] and Dp0 > 1024:
                    assert tiles(q, 'stack_fwd') == (Dp0, 320, 64 * (Dp0 + 320)) and tiles(q, 'stack_bwd') == (320, 128, 64 * 448)     # A: 64, 320; B: 128
                assert q['rows_bwd'] == ('wide' if K > 16 else 'many' if F >= 33 else 'narrow')
                # the 16-example forward wherever its tile of 16 (17 F + Dp0) floats fits the LDS
                assert q['rows_fwd'] == ('wide' if K > 16 else 'many' if F >= 33 and 16 * (17 * F + Dp0) * 4 > LDS else 'narrow')


def test_refusals_and_the_struct(built):
    lib = _capi.load()
    assert lib.ipnn_plan_info_size() == C.sizeof(_capi.ipnn_plan_info) == 192
    assert lib.ipnn_cfg_size() == C.sizeof(_capi.ipnn_cfg) == 96
    info = _capi.ipnn_plan_info()
    assert lib.ipnn_plan_query(None, C.byref(info)) == _capi.FNN_ERR_ARG
    with pytest.raises(FNNError) as ei:
        ipnn.plan_query(65, 4, [8])
    assert ei.value.code == _capi.FNN_ERR_ARG and 'n_fields = 65' in str(ei.value)
    with pytest.raises(FNNError) as ei:
        ipnn.plan_query(16, 11, [5000])
    assert 'hidden size out of range' in str(ei.value)
