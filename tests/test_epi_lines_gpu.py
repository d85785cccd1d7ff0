"""Row-contiguous NT epilogues (aew_set_nt_epi_lines, csrc/aew_gemm.hip: nt_epilogue_lines) on the MI355X.

Every case runs ONE descriptor twice in one process - setter 0 (MFMA-layout epilogue) and setter 1 (accumulators
exchanged across lanes, whole 128-byte lines per wave access) - and asserts torch.equal on every output buffer.  The
buffers start from the same random bytes, so rows and channel octets a mask must leave alone are compared as well.

Shapes: M = 300 (a full 256-row tile plus a ragged one of 44 rows: no multiple of 16 or 8), batch 2, ragged channel
octets (N = 368 in N_pad = 384), views whose row window cuts through a tile, aux views shifted by d so that masked aux
rows occur at both ends.  K = 128: the launcher's ABI wants bf16 segments in multiples of 64 channels (a K of 96 is
refused with AEW_E_ARG, asserted below), so 128 = four K tiles is the smallest K that runs the 3-stage ring past its
prologue."""
import ctypes as C

import pytest
import torch

from ae_wavenet_amd import _lib as L, config, model as M, plan as PLN
from ae_wavenet_amd.plan import Mat, Plan, Workspace, make_nt
from tests.test_gpu_parity import DEV, _fill, _mirror, np_weights, stream

pytestmark = pytest.mark.gpu
BF, F3 = L.BF16, L.F32
B, M_, K, ROWS = 2, 300, 128, 330


def _alloc(ws, gen):
    ws.alloc("A", B * 340 * 256, torch.bfloat16)
    ws.alloc("W", 512 * 256, torch.bfloat16)
    for n in ("O0", "O1", "X0", "X1"):
        ws.alloc(n, B * ROWS * 512, torch.bfloat16)
    ws.alloc("O0f", B * ROWS * 384, torch.float32)
    ws.alloc("bias", B * 384, torch.float32)
    for n in ("A", "X0", "X1", "O0", "O1", "O0f", "bias"):
        _fill(ws, n, gen)
    _fill(ws, "W", gen, 0.08)


def _store_case(ws, flags, d, fp32_out=False):
    A = Mat(ws, "A", B, 340, 256, BF)
    Wm = Mat(ws, "W", 1, 384, K, BF)
    O0 = Mat(ws, "O0f", B, ROWS, 384, F3) if fp32_out else Mat(ws, "O0", B, ROWS, 384, BF)
    O1, X0, X1 = (Mat(ws, n, B, ROWS, 384, BF) for n in ("O1", "X0", "X1"))
    segs = [A.seg(64, row_off=0), A.seg(64, row_off=7, col_off=64, hi=330)]
    kw = {}
    if flags & L.EF_BIAS:
        kw = dict(bias_ptr=ws.get("bias").data_ptr(), bias_bs=384)
    return make_nt(BF, M_, 368, 384, B, segs, Wm.ptr, flags=flags, out0=O0.view(row_off=5, lo=20, hi=290),
                   out1=O1.view(row_off=2), aux0=X0.view(row_off=-d, hi=270), aux1=X1.view(row_off=-d, hi=ROWS - 40), **kw)


def _dfg_case(ws, d):
    A = Mat(ws, "A", B, 340, 256, BF)
    Wm = Mat(ws, "W", 1, 256, K, BF)
    O0 = Mat(ws, "O0", B, ROWS, 512, BF)
    X0, X1 = (Mat(ws, n, B, ROWS, 256, BF) for n in ("X0", "X1"))
    segs = [A.seg(64, row_off=3), A.seg(64, row_off=0, col_off=128)]
    return make_nt(BF, M_, 256, 256, B, segs, Wm.ptr, epi=L.EPI_DFG, out0=O0.view(row_off=5, lo=20, hi=290),
                   aux0=X0.view(row_off=-d, hi=270), aux1=X1.view(row_off=-d, hi=ROWS - 40))


def _win_case(ws, flags, d):
    """the input-gradient shape of a dilated layer: dfg[t], dfg[t - d] of ONE buffer (the one-window body)"""
    A = Mat(ws, "A", B, 340, 256, BF)
    Wm = Mat(ws, "W", 1, 384, 2 * K, BF)
    O0, O1, X0, X1 = (Mat(ws, n, B, ROWS, 384, BF) for n in ("O0", "O1", "X0", "X1"))
    segs = [A.seg(K, hi=M_ - 8), A.seg(K, row_off=-d, hi=M_ - 8)]
    kw = {}
    if flags & L.EF_BIAS:
        kw = dict(bias_ptr=ws.get("bias").data_ptr(), bias_bs=384)
    return make_nt(BF, M_, 368, 384, B, segs, Wm.ptr, flags=flags, out0=O0.view(row_off=5, lo=20, hi=290),
                   out1=O1.view(row_off=2), aux0=X0.view(row_off=-d, hi=270), aux1=X1.view(row_off=-d, hi=ROWS - 40), **kw)


def _ab(case, outs, kernel, rows192=0, window=64):
    """runs case(ws) under setter 0 and 1; every buffer of `outs` must come out bit-equal"""
    lib = L.load()
    ws_c = Workspace("cpu")
    _alloc(ws_c, torch.Generator().manual_seed(17))
    res = {}
    try:
        lib.aew_set_nt_small_tiles(0)                        # (few tiles: the launcher would take its 64-row shapes)
        lib.aew_set_nt_rows192(rows192)
        lib.aew_set_nt_window(window)
        for on in (0, 1):
            lib.aew_set_nt_epi_lines(on)
            ws_g = _mirror(ws_c, DEV)
            p = Plan("nt")
            op = p.add(L.OP_GEMM_NT, case(ws_g), "nt")
            assert lib.aew_nt_kernel(C.byref(op.u.nt)) == kernel
            p.run(stream())
            torch.cuda.synchronize()
            res[on] = {n: ws_g.get(n).cpu() for n in outs}
    finally:
        lib.aew_set_nt_epi_lines(L.NT_EPI_LINES_DEFAULT)
        lib.aew_set_nt_small_tiles(128)
        lib.aew_set_nt_rows192(1)
        lib.aew_set_nt_window(64)
    for n in outs:
        assert not torch.equal(res[0][n], ws_c.get(n)), (n, "the launch wrote nothing")
        assert torch.equal(res[0][n].view(torch.int16 if res[0][n].dtype == torch.bfloat16 else torch.int32),
                           res[1][n].view(torch.int16 if res[1][n].dtype == torch.bfloat16 else torch.int32)), n


STORE_FLAGS = [0, L.EF_ADD_AUX0, L.EF_MUL_POS1, L.EF_BIAS | L.EF_RELU | L.EF_OUT1_PRE]


def test_k_of_96_is_not_a_legal_bf16_descriptor():
    lib = L.load()
    ws = Workspace("cpu")
    ws.alloc("A", B * 340 * 256, torch.bfloat16); ws.alloc("W", 384 * 96, torch.bfloat16); ws.alloc("O0", B * ROWS * 384, torch.bfloat16)
    A, Wm, O0 = Mat(ws, "A", B, 340, 256, BF), Mat(ws, "W", 1, 384, 96, BF), Mat(ws, "O0", B, ROWS, 384, BF)
    g = make_nt(BF, M_, 368, 384, B, [A.seg(96)], Wm.ptr, out0=O0.view())
    assert lib.aew_nt_kernel(C.byref(g)) == L.E_ARG


@pytest.mark.parametrize("rows192", [0, 2])
@pytest.mark.parametrize("d", [1, 16])
@pytest.mark.parametrize("flags", STORE_FLAGS)
def test_store_epilogue_is_bit_identical_in_both_layouts(flags, d, rows192):
    outs = ["O0"] + (["O1"] if flags & L.EF_OUT1_PRE else [])
    _ab(lambda ws: _store_case(ws, flags, d), outs, kernel=0, rows192=rows192)


def test_store_with_both_aux_operands_and_post_relu_mask():
    """aux0 and aux1 in use at once: aux1 is fetched in step (one prefetched operand), OUT1_POS1 writes the masked copy"""
    fl = L.EF_ADD_AUX0 | L.EF_MUL_POS1 | L.EF_OUT1_POS1 | L.EF_RELU_POST
    _ab(lambda ws: _store_case(ws, fl, 16), ["O0", "O1"], kernel=0)


def test_fp32_out0_keeps_the_mfma_layout_epilogue():
    _ab(lambda ws: _store_case(ws, L.EF_ADD_AUX0, 1, fp32_out=True), ["O0f"], kernel=0)


@pytest.mark.parametrize("rows192", [0, 2])
@pytest.mark.parametrize("d", [1, 16])
def test_dfg_epilogue_is_bit_identical_in_both_layouts(d, rows192):
    _ab(lambda ws: _dfg_case(ws, d), ["O0"], kernel=0, rows192=rows192)


@pytest.mark.parametrize("rows192", [0, 2])
@pytest.mark.parametrize("d", [1, 4, 16, 64])
def test_window_kernel_store_epilogue_is_bit_identical_in_both_layouts(d, rows192):
    for flags in STORE_FLAGS:
        outs = ["O0"] + (["O1"] if flags & L.EF_OUT1_PRE else [])
        _ab(lambda ws: _win_case(ws, flags, d), outs, kernel=6, rows192=rows192)


def _stack_engine(seed=5):
    """a 2-layer decoder stack at B = 2, w = 64, both directions chained (forced onto the 256-row bodies)"""
    hps = config.make_hps("vqvae-ema", n_win_batch=64, n_blocks=1, n_block_layers=2, bn_vq_n_embed=256)
    eng = M.TrainEngine(hps, B=2, device=DEV, n_mel=39, update_codebook_every_step=False)
    wts = np_weights({k: eng.ps.shape[k] for k in eng.ps.names()}, seed)
    for k, v in wts.items():
        eng.ps.view(k).copy_(torch.from_numpy(v))
    gen = torch.Generator().manual_seed(seed + 1)
    eng.emb.copy_(torch.randn(256, hps.bn_n_out, generator=gen) * 0.7)
    eng.init_ema_from_emb()
    g = eng.geom
    wav = torch.randint(0, 256, (2, g.enc_in_len), generator=gen).float()
    mel = torch.randn(2, 39, g.mel_len, generator=gen)
    voice = torch.randint(0, 40, (2,), generator=gen)
    jitter = torch.arange(g.embed_len).repeat(2, 1)
    eng.set_inputs(wav.to(DEV), mel.to(DEV), voice.to(DEV), jitter.to(DEV))
    return eng


def test_chained_stack_is_bit_identical_in_both_layouts(monkeypatch):
    """forward and backward chains (stages with write-through out0 and device-scope aux loads) captured and run under
    setter 0 and under setter 1 (the launch picks the form): loss and the whole gradient buffer bit-equal, no hand-off
    wait gave up"""
    lib = L.load()
    monkeypatch.delenv("AEW_NT_CHAIN", raising=False)
    monkeypatch.setattr(M.TrainEngine, "nt_chain", 64)
    monkeypatch.setattr(M.TrainEngine, "nt_chain_bwd", 64)
    monkeypatch.setattr(M.TrainEngine, "nt_chain_force", True)
    res = {}
    try:
        for on in (0, 1):
            lib.aew_set_nt_epi_lines(on)
            eng = _stack_engine()
            chains = [lab for pl in (eng.fwd_b, eng.bwd) for lab in getattr(pl, "nt_chains", {})]
            assert len(chains) >= 2, chains                    # (at least the stack forward and its backward)
            outs = []
            for rep in range(2):
                loss = float(eng.forward())
                eng.backward()
                torch.cuda.synchronize()
                for pl in (eng.fwd_b, eng.bwd):
                    assert PLN.chain_timeouts(pl) == [], PLN.chain_stats(pl)
                outs.append((loss, eng.ps.grads[:eng.ps.numel].clone()))
            res[on] = outs
            del eng
            torch.cuda.empty_cache()
    finally:
        lib.aew_set_nt_epi_lines(L.NT_EPI_LINES_DEFAULT)
    for (l0, g0), (l1, g1) in zip(res[0], res[1]):
        assert l0 == l1, (l0, l1)
        assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), (g0 - g1).abs().max().item()
