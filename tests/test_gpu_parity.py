"""GPU parity tests (run with `-m gpu` on the MI355X).  Everything goes through the C ABI
(aew_run_plan).  Checkers: the CPU plan interpreter (tests/plan_emulator.py, itself pinned to
the reference goldens by tests/test_plan_cpu.py), the golden vectors directly, the exact-order
C oracle (bit-exact sub-path) and the torch fp32 oracle (full-width training step).

Stated tolerances (bf16 decoder, fp32 accumulate; fp32 exact encoder/VQ):
  VQ code indices, EMA counts ............ exact
  encoder / ze (fp32 MFMA fmaf chain) ..... bit-exact vs oracle/exact_chain.c
  logits (full width) ..................... |err| <= 0.06 abs  (logit scale ~ 1-5)
  loss .................................... 1 % relative
  gradients ............................... max-normalised error <= 15 % per tensor, cosine >= 0.99
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, config, geometry, model as M, plan as PL
from ae_wavenet_amd.plan import Mat, Plan, Workspace, make_nt, make_tn, null_view
from tests.plan_emulator import Emu

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from weights import grad_sketch, np_weights  # noqa: E402

DEV = "cuda:0"
BF, F3 = L.BF16, L.F32


def load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


def stream():
    return torch.cuda.current_stream().cuda_stream


def test_selftest_lane_mappings():
    """MFMA C/D + operand maps, fp32 MFMA = k-ascending fmaf chain, ds_read_b64_tr_b16 and
    LDS-DMA placement behave as the kernels assume."""
    lib = L.load()
    scratch = torch.zeros(1 << 18, dtype=torch.uint8, device=DEV)
    detail = (C.c_int32 * 8)()
    rc = lib.aew_selftest(scratch.data_ptr(), scratch.numel(), None, detail)
    assert rc == 0, f"selftest rc={rc} detail={list(detail)[:5]}"


# ----------------------------------------------------------------------------------------------
# single GEMM ops, random descriptors: GPU MFMA kernel and GPU check kernel vs CPU interpreter
# ----------------------------------------------------------------------------------------------
def _fill(ws, name, gen, scale=1.0):
    t = ws.get(name)
    v = (torch.rand(t.shape, generator=gen) * 2 - 1) * scale
    t.copy_(v.to(t.dtype))


def _mirror(ws_cpu, dev):
    ws = Workspace(dev)
    for n, t in ws_cpu.bufs.items():
        ws.bufs[n] = t.to(dev)
    return ws


def _nt_case(ws, dtype, epi, impl):
    B, M_, K1, K2, N_pad = 2, 300, 128, 256, 256
    pitchA = 256
    A1 = Mat(ws, "A1", B, 340, pitchA, dtype)
    A2 = Mat(ws, "A2", B, 400, pitchA, dtype)
    Wm = Mat(ws, "W", 1, N_pad, 2 * K1 + K2, dtype)
    segs = [A1.seg(K1, row_off=0), A1.seg(K1, row_off=7, col_off=64, hi=330), A2.seg(K2, row_off=-5, row_step=1)]
    odt = F3 if dtype == F3 else BF
    O0 = Mat(ws, "O0", B, 320, 512, odt)
    O1 = Mat(ws, "O1", B, 320, 256, F3 if epi == L.EPI_RES_SKIP else odt)
    O2 = Mat(ws, "O2", B, 320, 256, BF)
    X0 = Mat(ws, "X0", B, 320, 256, odt)
    X1 = Mat(ws, "X1", B, 320, 256, odt)
    bias = ws.get("bias")
    kw = dict(impl=impl)
    if epi == L.EPI_STORE:
        return make_nt(dtype, M_, 248, N_pad, B, segs, Wm.ptr, flags=L.EF_BIAS | L.EF_RELU | L.EF_OUT1_PRE
                       | L.EF_ADD_AUX0, out0=O0.view(row_off=3, row_step=1), out1=O1.view(),
                       aux0=X0.view(row_off=-2), bias_ptr=bias.data_ptr(), bias_bs=256, **kw)
    if epi == "mask":
        return make_nt(dtype, M_, N_pad, N_pad, B, segs, Wm.ptr, flags=L.EF_OUT1_POS1 | L.EF_ADD_AUX0,
                       out0=O0.view(), out1=O1.view(), aux0=X0.view(row_off=4, hi=250), aux1=X1.view(), **kw)
    if epi == L.EPI_GATED:
        return make_nt(dtype, M_, 128, N_pad, B, segs, Wm.ptr, epi=epi, out0=O0.view(), out1=O1.view(),
                       out2=O2.view(), bias_ptr=bias.data_ptr(), bias_bs=256, **kw)
    if epi == L.EPI_RES_SKIP:
        return make_nt(dtype, M_, N_pad, N_pad, B, segs, Wm.ptr, epi=epi, flags=L.EF_ACCUM | L.EF_OUT2_RELU,
                       out0=O0.view(), aux0=X0.view(row_off=9), out1=O1.view(row_off=-200, hi=100),
                       out2=O2.view(row_off=-200, hi=100), n_split=128, **kw)
    if epi == L.EPI_DFG:
        return make_nt(dtype, M_, 256, N_pad, B, segs, Wm.ptr, epi=epi, out0=O0.view(), aux0=X0.view(),
                       aux1=X1.view(), **kw)


def _alloc_nt(ws, dtype, epi):
    tdt = PL.TORCH_DT[dtype]
    odt = torch.float32 if dtype == F3 else torch.bfloat16
    ws.alloc("A1", 2 * 340 * 256, tdt); ws.alloc("A2", 2 * 400 * 256, tdt)
    ws.alloc("W", 256 * 512, tdt)
    ws.alloc("O0", 2 * 320 * 512, odt)
    ws.alloc("O1", 2 * 320 * 256, torch.float32 if epi == L.EPI_RES_SKIP else odt)
    ws.alloc("O2", 2 * 320 * 256, torch.bfloat16)
    ws.alloc("X0", 2 * 320 * 256, odt); ws.alloc("X1", 2 * 320 * 256, odt)
    ws.alloc("bias", 2 * 256, torch.float32)


@pytest.mark.parametrize("dtype,epi", [(BF, L.EPI_STORE), (BF, "mask"), (BF, L.EPI_GATED), (BF, L.EPI_RES_SKIP),
                                       (BF, L.EPI_DFG), (F3, L.EPI_STORE), (F3, "mask")])
def test_gemm_nt(dtype, epi):
    gen = torch.Generator().manual_seed(1)
    ws_c = Workspace("cpu")
    _alloc_nt(ws_c, dtype, epi)
    for n in ("A1", "A2", "X0", "X1", "O1", "bias"):
        _fill(ws_c, n, gen)
    _fill(ws_c, "W", gen, 0.08)
    results = {}
    lib = L.load()
    try:
        # impl 0 under every tile / wave shape of the bf16 kernel (64: 8 waves of 64x64, 128: 4 waves of
        # 128x64, 256: 256x256 tiles where N_pad allows, 512: those as 16 waves of 64x64 - RES_SKIP stays on the default
        # body); the shapes must agree bit for bit
        # (impl, shape, pipe, small): small = tile-count threshold of the 64-row tiles (0: plain 256x128)
        # small < 0: 192-row tiles forced (small tiles off)
        for impl, shape, pipe, small in ((0, 64, 1, 0), (1, 64, 1, 0), (0, 64, 1, 128), (0, 64, 1, -1), (0, 0, 1, 0), (0, 1, 1, 0),
                                         (0, 128, 1, 0), (0, 128, 0, 0), (0, 256, 0, 0), (0, 256, 1, 0), (0, 256, 2, 0), (0, 512, 1, 0)):
            lib.aew_set_nt_rows192(2 if small < 0 else 0)
            small = max(small, 0)
            lib.aew_set_nt_wave_rows(shape)
            lib.aew_set_nt_pipe(pipe)
            lib.aew_set_nt_small_tiles(small)
            ws_g = _mirror(ws_c, DEV)
            p = Plan("nt")
            p.add(L.OP_GEMM_NT, _nt_case(ws_g, dtype, epi, impl), "nt")
            p.run(stream())
            torch.cuda.synchronize()
            res = {n: ws_g.get(n).float().cpu() for n in ("O0", "O1", "O2")}
            if shape == 64 and small == 0 and impl not in results:
                results[impl] = res
            else:
                for n in res:
                    assert torch.equal(res[n], results[0][n]), (n, "shape", shape, "pipe", pipe, "small", small)
        # the 64-row shape in its three forms: 8 waves + 5-stage ring (default for small launches), 2 waves + 5 stages,
        # 2 waves + 2 stages; the fp32 kernel with the deep (one block per CU) and the shallow ring, with and without
        # its dedicated loader waves
        # (... and the 8-wave form as 64 x 64 tiles - the default for launches of few blocks - or as 64 x 128)
        for waves, deep, nf_deep, nf_ld, n64 in ((8, 256, 256, 1, 128), (8, 256, 256, 1, 0), (2, 256, 0, 1, 128), (2, 0, 256, 0, 0), (8, 256, 0, 0, 0)):
            lib.aew_set_nt_rows192(0)
            lib.aew_set_nt_wave_rows(64)
            lib.aew_set_nt_pipe(1)
            lib.aew_set_nt_small_tiles(128)
            lib.aew_set_nt_small_waves(waves)
            lib.aew_set_nt_small_deep(deep)
            lib.aew_set_nf_deep(nf_deep)
            lib.aew_set_nf_loaders(nf_ld)
            lib.aew_set_nt_small_n64(n64)
            ws_g = _mirror(ws_c, DEV)
            p = Plan("nt")
            p.add(L.OP_GEMM_NT, _nt_case(ws_g, dtype, epi, 0), "nt")
            p.run(stream())
            torch.cuda.synchronize()
            for n in ("O0", "O1", "O2"):
                assert torch.equal(ws_g.get(n).float().cpu(), results[0][n]), (n, "small-launch form", waves, deep, nf_deep, nf_ld, n64)
    finally:
        lib.aew_set_nt_wave_rows(64)
        lib.aew_set_nt_pipe(1)
        lib.aew_set_nt_small_tiles(128)
        lib.aew_set_nt_rows192(1)
        lib.aew_set_nt_small_waves(8)
        lib.aew_set_nt_small_deep(256)
        lib.aew_set_nf_deep(256)
        lib.aew_set_nf_loaders(1)
        lib.aew_set_nt_small_n64(256)
    ws_e = Workspace("cpu")
    for n, t in ws_c.bufs.items():
        ws_e.bufs[n] = t.clone()
    p = Plan("nt")
    p.add(L.OP_GEMM_NT, _nt_case(ws_e, dtype, epi, 0), "nt")
    Emu(ws_e).run(p)
    tol = 2e-2 if dtype == BF else 2e-5
    for n in ("O0", "O1", "O2"):
        ref = ws_e.get(n).float()
        for impl in (1, 0):
            err = (results[impl][n] - ref).abs().max().item()
            assert err <= tol * max(1.0, ref.abs().max().item()), (n, "impl", impl, err)
    if dtype == F3:
        # same fmaf chain in the same order: MFMA kernel == scalar check kernel bit for bit
        assert torch.equal(results[0]["O0"], results[1]["O0"])


@pytest.mark.parametrize("epi", [L.EPI_STORE, L.EPI_GATED, L.EPI_RES_SKIP, L.EPI_DFG, "mask", "mid"])
def test_gemm_nt_small_split(epi):
    """aew_gemm_nt_t.k_split as a hint on a bf16 launch of few 64 x 64 blocks: S copies of the tile grid contract S ranges
    of K, the partial accumulators meet in ascending order in the workgroup that arrives last.  Every epilogue, ranges that
    start at a segment boundary (S = 2 over 2 + 2 + 4 K tiles) and inside a segment ("mid": S = 3 over 6 + 6); against the
    CPU plan interpreter at the tolerance of test_gemm_nt, against the unsplit launch (same operands, another fp32 order:
    a few bf16 round-offs apart), and replay after replay bit for bit (the tickets reset themselves)."""
    gen = torch.Generator().manual_seed(5)
    ws_c = Workspace("cpu")
    _alloc_nt(ws_c, BF, epi if epi != "mid" else L.EPI_STORE)
    for n in ("A1", "A2", "X0", "X1", "O1", "bias"):
        _fill(ws_c, n, gen)
    _fill(ws_c, "W", gen, 0.08)
    lib = L.load()

    def case(ws):
        if epi != "mid":
            return _nt_case(ws, BF, epi, 0)
        A1 = Mat(ws, "A1", 2, 340, 256, BF)
        A2 = Mat(ws, "A2", 1, 200, 1024, BF)                 # (the same buffer, read 384 wide)
        Wm = Mat(ws, "W", 1, 128, 768, BF)
        O0 = Mat(ws, "O0", 2, 320, 512, BF)
        X0 = Mat(ws, "X0", 2, 320, 256, BF)
        return make_nt(BF, 150, 120, 128, 1, [A2.seg(384, row_off=2), A2.seg(384, row_off=-3, col_off=512)], Wm.ptr,
                       flags=L.EF_ADD_AUX0 | L.EF_RELU, out0=O0.view(row_off=3), aux0=X0.view(row_off=-2), impl=0)

    want = 3 if epi == "mid" else 2
    res = {}
    for split in (0, 1):
        ws_g = _mirror(ws_c, DEV)
        g = case(ws_g)
        if split:
            S, nbytes, ntk = C.c_int(1), C.c_int64(0), C.c_int(0)
            L.check(lib.aew_gemm_nt_small_split(C.byref(g), 256 if epi != "mid" else 48, C.byref(S), C.byref(nbytes), C.byref(ntk)), "hint")
            assert S.value == want and nbytes.value > 0 and ntk.value > 0, (S.value, nbytes.value, ntk.value)
            slab = ws_g.alloc("ks.ws", nbytes.value // 4, torch.float32, zero=False)
            slab.fill_(float("nan"))
            tk = ws_g.alloc("ks.tk", ntk.value, torch.int32)
            g.k_split, g.ksplit_ws, g.ksplit_tickets = S.value, slab.data_ptr(), tk.data_ptr()
        p = Plan("nt")
        p.add(L.OP_GEMM_NT, g, "nt")
        for rep in range(4 if split else 1):
            if rep:                                            # (accumulating / in-place forms: restore the outputs)
                for n in ("O0", "O1", "O2"):
                    ws_g.get(n).copy_(ws_c.get(n))
            p.run(stream())
            torch.cuda.synchronize()
            out = {n: ws_g.get(n).float().cpu() for n in ("O0", "O1", "O2")}
            if rep:
                assert all(torch.equal(out[n], res[1][n]) for n in out), ("replay", rep)
            res[split] = out
        if split:
            assert int(tk[:ntk.value].abs().sum()) == 0
    ws_e = Workspace("cpu")
    for n, t in ws_c.bufs.items():
        ws_e.bufs[n] = t.clone()
    p = Plan("nt")
    p.add(L.OP_GEMM_NT, case(ws_e), "nt")
    Emu(ws_e).run(p)
    moved = 0
    for n in ("O0", "O1", "O2"):
        ref = ws_e.get(n).float()
        scale = max(1.0, ref.abs().max().item())
        assert (res[1][n] - ref).abs().max().item() <= 2e-2 * scale, n
        d = (res[1][n] - res[0][n]).abs()
        moved += int((d > 0).sum())
        assert d.max().item() <= 2.0 ** -6 * scale, (n, d.max().item())      # a bf16 round-off or two of the largest value
        assert float((d > 1e-5 * scale).float().mean()) < 0.05, n                 # (fp32 outputs differ in their last bits)
    assert float(res[1]["O0"].abs().max()) > 0
    print(f"split S = {want}: {moved} output elements differ from the unsplit launch by a bf16 round-off")


@pytest.mark.parametrize("epi", [L.EPI_DFG, "g2"])
def test_gemm_nt_mem128(epi):
    """The 128-row tile forms of the memory-bound launches (aew_set_nt_mem128: dz with its DFG epilogue, wavenet.py:100-102
    backward, and the K = 256 residual 1x1 + add, wavenet.py:108-109) are bit-identical to the 256-row tiles."""
    gen = torch.Generator().manual_seed(3)
    ws_c = Workspace("cpu")
    _alloc_nt(ws_c, BF, L.EPI_STORE)
    for n in ("A1", "A2", "X0", "X1", "O1", "bias"):
        _fill(ws_c, n, gen)
    _fill(ws_c, "W", gen, 0.08)
    lib = L.load()

    def case(ws):
        if epi == L.EPI_DFG:
            return _nt_case(ws, BF, L.EPI_DFG, 0)
        A2 = Mat(ws, "A2", 2, 400, 256, BF)
        Wm = Mat(ws, "W", 1, 256, 256, BF)
        O0 = Mat(ws, "O0", 2, 320, 512, BF)
        X0 = Mat(ws, "X0", 2, 320, 256, BF)
        return make_nt(BF, 300, 248, 256, 2, [A2.seg(256, row_off=-5)], Wm.ptr, flags=L.EF_ADD_AUX0,
                       out0=O0.view(row_off=3), aux0=X0.view(row_off=-2), impl=0)
    ref = None
    try:
        lib.aew_set_nt_small_tiles(0)
        for mode, deep in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2)):     # deep: the deep-ring A/B shapes (aew_set_nt_deep)
            lib.aew_set_nt_mem128(mode)
            lib.aew_set_nt_deep(deep)
            ws_g = _mirror(ws_c, DEV)
            p = Plan("nt")
            p.add(L.OP_GEMM_NT, case(ws_g), "nt")
            p.run(stream())
            torch.cuda.synchronize()
            res = ws_g.get("O0").float().cpu()
            if ref is None:
                ref = res
                assert float(ref.abs().max()) > 0
            else:
                assert torch.equal(res, ref), ("mem128 mode", mode, "deep", deep)
    finally:
        lib.aew_set_nt_mem128(0)
        lib.aew_set_nt_deep(0)
        lib.aew_set_nt_small_tiles(128)


def test_tuned_run_uses_the_callers_record_and_leaves_the_process_state_alone():
    """aew_run_plan_tuned: a caller's aew_tuning_t applies to that call only.  The same GEMM through three records (fat
    waves, 192-row tiles, 128-row memory-bound tiles) gives the bit-identical result of the default shape, and the
    process-wide record - what aew_nt_kernel and every untuned call see - is untouched."""
    import ctypes as C
    gen = torch.Generator().manual_seed(9)
    ws_c = Workspace("cpu")
    _alloc_nt(ws_c, BF, L.EPI_DFG)
    for n in ("A1", "A2", "X0", "X1", "O1", "bias"):
        _fill(ws_c, n, gen)
    _fill(ws_c, "W", gen, 0.08)
    lib = L.load()
    before = L.Tuning()
    lib.aew_tuning_get(C.byref(before))
    ref = None
    for over in ({}, dict(nt_wave_rows=128), dict(nt_rows192=2, nt_small_tiles=0), dict(nt_mem128=1, nt_small_tiles=0),
                 dict(nt_wave_rows=256, nt_pipe=0)):
        ws_g = _mirror(ws_c, DEV)
        p = Plan("nt")
        g = _nt_case(ws_g, BF, L.EPI_DFG, 0)
        p.add(L.OP_GEMM_NT, g, "nt")
        p.run(stream(), tuning=L.default_tuning(**over) if over else None)
        torch.cuda.synchronize()
        res = ws_g.get("O0").float().cpu()
        if ref is None:
            ref = res
            assert float(ref.abs().max()) > 0
        assert torch.equal(res, ref), over
        after = L.Tuning()
        lib.aew_tuning_get(C.byref(after))
        assert bytes(after) == bytes(before), over


def _win_case(ws, kind, d, impl):
    """The two shapes the decoder runs on the window kernel: the gated layer (wavenet.py:100-101: x[t], x[t+d] of one
    tensor + the conditioning projection) and its input gradient (dfg[t], dfg[t-d], rows outside dfg read as zero)."""
    B = 2
    if kind == "gated":
        Lin, K, Kc, Np = 777, 384, 128, 256
        X = Mat(ws, "X", B, Lin, K, BF)
        Cn = Mat(ws, "C", B, Lin + 40, Kc, BF)
        Wm = Mat(ws, "W", 1, Np, 2 * K + Kc, BF)
        O0, O1, O2 = (Mat(ws, n, B, Lin, 128, BF) for n in ("O0", "O1", "O2"))
        segs = [X.seg(K), X.seg(K, row_off=d), Cn.seg(Kc, row_off=d + 3)]
        return make_nt(BF, Lin - d, 128, Np, B, segs, Wm.ptr, epi=L.EPI_GATED, out0=O0.view(), out1=O1.view(),
                       out2=O2.view(), bias_ptr=ws.get("bias").data_ptr(), bias_bs=256, impl=impl)
    Lout, K, Np = 700, 256, 384
    Dm = Mat(ws, "X", B, Lout, K, BF)
    Wm = Mat(ws, "W", 1, Np, 2 * K, BF)
    O0 = Mat(ws, "O0", B, Lout + d, Np, BF)
    A0 = Mat(ws, "A0", B, Lout + d, Np, BF)
    segs = [Dm.seg(K), Dm.seg(K, row_off=-d)]
    return make_nt(BF, Lout + d, 368, Np, B, segs, Wm.ptr, flags=L.EF_ADD_AUX0, out0=O0.view(),
                   aux0=A0.view(row_off=-d, hi=Lout), impl=impl)


@pytest.mark.parametrize("kind", ["gated", "dx"])
@pytest.mark.parametrize("d", [1, 2, 4, 8, 16, 32, 64, 5, 48])
def test_gemm_nt_window(kind, d):
    """k_gemm_nt_bf16_win (one LDS window for both dilation taps) against the two-segment kernel (same products,
    other summation order: agreement to fp32 rounding, i.e. at most one bf16 ulp in a few outputs), the scalar check
    kernel and the CPU interpreter."""
    gen = torch.Generator().manual_seed(11 + d)
    ws_c = Workspace("cpu")
    ws_c.alloc("X", 2 * 777 * 384, torch.bfloat16); ws_c.alloc("C", 2 * 817 * 128, torch.bfloat16)
    ws_c.alloc("W", 384 * 896, torch.bfloat16)
    for n in ("O0", "O1", "O2", "A0"):
        ws_c.alloc(n, 2 * 800 * 384, torch.bfloat16)
    ws_c.alloc("bias", 2 * 256, torch.float32)
    for n in ("X", "C", "A0", "bias"):
        _fill(ws_c, n, gen)
    _fill(ws_c, "W", gen, 0.06)
    lib = L.load()
    res = {}
    try:
        lib.aew_set_nt_small_tiles(0)
        # win192: the 192-row tile form of the window kernel (what the cost model picks for the shorter layers)
        for tag, impl, win, r192 in (("win", 0, 64, 0), ("win192", 0, 64, 2), ("two", 0, 0, 0), ("chk", 1, 0, 0)):
            lib.aew_set_nt_window(win)
            lib.aew_set_nt_rows192(r192)
            ws_g = _mirror(ws_c, DEV)
            p = Plan("nt")
            op = p.add(L.OP_GEMM_NT, _win_case(ws_g, kind, d, impl), "nt")
            assert lib.aew_nt_kernel(C.byref(op.u.nt)) == {"win": 6, "win192": 6, "two": 0, "chk": 4}[tag]
            p.run(stream())
            torch.cuda.synchronize()
            res[tag] = {n: ws_g.get(n).float().cpu() for n in ("O0", "O1", "O2")}
    finally:
        lib.aew_set_nt_small_tiles(128)
        lib.aew_set_nt_window(64)
        lib.aew_set_nt_rows192(1)
    ws_e = Workspace("cpu")
    for n, t in ws_c.bufs.items():
        ws_e.bufs[n] = t.clone()
    p = Plan("nt")
    p.add(L.OP_GEMM_NT, _win_case(ws_e, kind, d, 0), "nt")
    Emu(ws_e).run(p)
    for n in ("O0", "O1", "O2"):
        ref = ws_e.get(n).float()
        scale = max(1.0, ref.abs().max().item())
        for tag in ("win", "win192", "two", "chk"):
            err = (res[tag][n] - ref).abs().max().item()
            assert err <= 2e-2 * scale, (n, tag, err)
        assert torch.equal(res["win"][n], res["win192"][n]), n                    # same chain per output, other tiling
        dw = (res["win"][n] - res["two"][n]).abs()
        assert dw.max().item() <= 2.0 ** -7 * scale, (n, dw.max().item())        # one bf16 ulp at the top binade
        assert (dw > 0).float().mean().item() < 0.05, (n, (dw > 0).float().mean().item())


@pytest.mark.parametrize("dtype", [BF, F3])
@pytest.mark.parametrize("safe,Mc", [(0, 777), (1, 777), (0, 5000)])
def test_gemm_tn(dtype, safe, Mc):
    """Mc=777 folds the batch into one slab; Mc=5000 exercises split-K slabs."""
    if dtype == F3 and safe:
        pytest.skip("safe mode only affects the bf16 transpose read")
    lib = L.load()
    gen = torch.Generator().manual_seed(2)
    tdt = PL.TORCH_DT[dtype]
    B, Np, K1, K2 = 2, 256, 128, 256
    R0 = Mc + 43
    ws_c = Workspace("cpu")
    ws_c.alloc("G", B * R0 * Np, tdt); ws_c.alloc("A1", B * R0 * 256, tdt); ws_c.alloc("A2", B * R0 * 256, tdt)
    for n in ("G", "A1", "A2"):
        _fill(ws_c, n, gen)

    def build(ws, impl):
        Gm = Mat(ws, "G", B, R0, Np, dtype)
        A1 = Mat(ws, "A1", B, R0, 256, dtype)
        A2 = Mat(ws, "A2", B, R0, 256, dtype)
        t = make_tn(dtype, Mc, B, Np, Np, Gm.seg(Np, row_off=3, hi=Mc - 77),
                    [A1.seg(K1, row_off=11), A1.seg(K1, row_off=-4, col_off=128), A2.seg(K2, row_step=1, row_off=0)],
                    impl=impl)
        slabs = L.tn_slabs(t)
        if "out" not in ws.bufs:
            ws.alloc("out", slabs * Np * t.K_total, torch.float32)
        t.out, t.out_batch_stride = ws.get("out").data_ptr(), Np * t.K_total
        return t, slabs

    res = {}
    lib.aew_set_tn_safe(safe)
    try:
        for impl in (0, 1):
            ws_g = _mirror(ws_c, DEV)
            t, slabs = build(ws_g, impl)
            p = Plan("tn"); p.add(L.OP_GEMM_TN, t, "tn"); p.run(stream())
            torch.cuda.synchronize()
            res[impl] = ws_g.get("out")[:slabs * Np * t.K_total].view(slabs, Np, t.K_total).sum(0).cpu()
    finally:
        lib.aew_set_tn_safe(0)
    ws_e = Workspace("cpu")
    for n, tt in ws_c.bufs.items():
        ws_e.bufs[n] = tt.clone()
    t, slabs = build(ws_e, 0)
    p = Plan("tn"); p.add(L.OP_GEMM_TN, t, "tn"); Emu(ws_e).run(p)
    ref = ws_e.get("out")[:slabs * Np * t.K_total].view(slabs, Np, t.K_total).sum(0)
    scale = ref.abs().max().item()
    for impl in (1, 0):
        err = (res[impl] - ref).abs().max().item()
        assert err <= (2e-3 if dtype == BF else 2e-5) * scale, ("impl", impl, "safe", safe, err, scale)


def test_tuned_record_cannot_change_a_built_split_k_plan():
    """the slab buffers of a TN op are sized at plan build time under the process-wide record (aew_tn_slabs).  A
    caller's per-call record (aew_run_plan_tuned) with other split-K fields must not make the launch write a different
    number of slabs: those fields are pinned to the process-wide values, so the tuned run writes exactly the slabs the
    untuned one does - bit for bit, guard region untouched."""
    gen = torch.Generator().manual_seed(4)
    B, Np, K1, Mc = 2, 256, 256, 5000
    R0 = Mc + 8
    ws = Workspace(DEV)
    for n, cols in (("G", Np), ("A1", K1)):
        ws.alloc(n, B * R0 * cols, torch.bfloat16)
        ws.get(n)[:B * R0 * cols].copy_(torch.randn(B * R0 * cols, generator=gen).to(torch.bfloat16))
    Gm, A1 = Mat(ws, "G", B, R0, Np, BF), Mat(ws, "A1", B, R0, K1, BF)
    t = make_tn(BF, Mc, B, Np, Np, Gm.seg(Np), [A1.seg(K1)])
    slabs = L.tn_slabs(t)
    assert slabs > B                                       # a split-K plan (not the folded single slab)
    n_out = slabs * Np * t.K_total
    guard = 4 * Np * t.K_total
    out = ws.alloc("out", n_out + guard, torch.float32)
    t.out, t.out_batch_stride = out.data_ptr(), Np * t.K_total
    p = Plan("tn")
    p.add(L.OP_GEMM_TN, t, "tn")
    res = []
    for over in (None, dict(tn_target_blocks=4 * 512, tn_fold_rows=1 << 20), dict(tn_target_blocks=8, tn_small_tiles=64, tn_small_target=8),
                 dict(tn_big=1, tn_big_target=64)):
        out.fill_(-7.0)
        p.run(stream(), tuning=L.default_tuning(**over) if over else None)
        torch.cuda.synchronize()
        assert bool((out[n_out:n_out + guard] == -7.0).all()), over        # nothing beyond the planned slabs
        assert bool((out[:n_out] != -7.0).all()), over                     # every planned slab written
        res.append(out[:n_out].clone())
    for r in res[1:]:
        assert torch.equal(r, res[0])


@pytest.mark.parametrize("tile", [128, 256, 384])
def test_gemm_tn_group(tile):
    """AEW_OP_GEMM_TN_GROUP: several weight-gradient descriptors in one launch, each output tile contracted over all
    rows of all batch elements in one block (one result, no slabs), plus the running per-batch snapshots of the
    ones-channel column.  Against the CPU interpreter and against the per-matrix TN ops + slab sum."""
    from ae_wavenet_amd.plan import TnGroupBuilder
    gen = torch.Generator().manual_seed(5)
    B = 3

    def build(ws):
        G1 = Mat(ws, "G1", B, 700, 256, BF)
        A1 = Mat(ws, "A1", B, 740, 384, BF)
        A2 = Mat(ws, "A2", B, 760, 128, BF)
        G2 = Mat(ws, "G2", B, 650, 384, BF)
        Z = Mat(ws, "Z", B, 650, 256, BF)
        descs = []
        t = make_tn(BF, 690, B, 256, 256, G1.seg(256), [A1.seg(384), A1.seg(384, row_off=9), A2.seg(128, row_off=31)])
        t.out, t.out_batch_stride = ws.get("o1").data_ptr(), 256 * 896
        t.snap_out, t.snap_bs, t.snap_k = ws.get("snap").data_ptr(), 256, 368
        t.colsum_out = ws.get("cs1").data_ptr()
        descs.append(t)
        t = make_tn(BF, 650, B, 368, 384, G2.seg(384, hi=640), [Z.seg(256)])
        t.out, t.out_batch_stride = ws.get("o2").data_ptr(), 384 * 256
        t.colsum_out = ws.get("cs2").data_ptr()          # 368 real columns: entries 368.. must stay untouched
        t.snap_out, t.snap_bs, t.snap_k = ws.get("snap2").data_ptr(), 384, -1     # running column sums of G2 itself
        descs.append(t)
        t = make_tn(BF, 33, B, 256, 256, G1.seg(256, row_off=5), [Z.seg(256, row_off=-2)])    # shorter than one stage pair
        t.out, t.out_batch_stride = ws.get("o3").data_ptr(), 256 * 256
        descs.append(t)
        if tile == 128:                                  # a split descriptor: partial sums per (batch element, row chunk)
            t = make_tn(BF, 650, B, 128, 128, G2.seg(128, row_off=3), [Z.seg(256, row_off=1), Z.seg(256)])
            t.out, t.out_batch_stride = ws.get("o4").data_ptr(), 128 * 512
            descs.append(t)
        return descs

    ws_c = Workspace("cpu")
    for n, sz in (("G1", B * 700 * 256), ("A1", B * 740 * 384), ("A2", B * 760 * 128), ("G2", B * 650 * 384), ("Z", B * 650 * 256)):
        ws_c.alloc(n, sz, torch.bfloat16)
        _fill(ws_c, n, gen)
    ws_c.get("A1").view(-1)[:B * 740 * 384].view(B * 740, 384)[:, 368] = 1.0        # the ones channel
    for n, sz in (("o1", 256 * 896), ("o2", 384 * 256), ("o3", 256 * 256), ("snap", B * 256), ("snap2", B * 384)):
        ws_c.alloc(n, sz, torch.float32)
        ws_c.alloc(n + ".ref", 8 * sz, torch.float32)
    ws_c.alloc("o4", 9 * 128 * 512, torch.float32)       # 3 batch elements x 3 chunks of 224 rows
    ws_c.alloc("cs1", 256, torch.float32)
    ws_c.alloc("cs2", 384, torch.float32)
    ws_c.get("cs2")[368:384] = -7.0                    # guard: columns beyond N belong to the next gradient
    ws_g = _mirror(ws_c, DEV)
    for ws in (ws_c, ws_g):
        gb = TnGroupBuilder(ws, "tng", tile)
        for i, t in enumerate(build(ws)):
            if i == 3:
                assert gb.set_split(t, 220) == 9 and (t.grp_splits, t.grp_rows) == (3, 224)
            gb.add(t, f"d{i}")
        p = Plan("g")
        gb.emit(p, "group")
        if ws is ws_g:
            tm = gb.tile_map()
            # (384: the 8-wave tiles - 128 x 256 for descriptors 0 and 2, 256 x 128 for descriptor 1 whose N_pad = 384)
            counts = {128: (14, 6, 4), 256: (4, 2, 1), 384: (7, 3, 2)}[tile]
            want = [(d << 22) | tl for d, n in enumerate(counts) for tl in range(n)]
            if tile == 128:
                want += [(3 << 22) | (c << 12) | tl for c in range(9) for tl in range(4)]
            assert sorted(r for r in tm if r >= 0) == sorted(want)
            p.run(stream())
            torch.cuda.synchronize()
        else:
            Emu(ws).run(p)
    assert torch.all(ws_g.get("cs2")[368:384].cpu() == -7.0)
    for n in ("o1", "o2", "o3", "snap", "snap2", "cs1", "cs2") + (("o4",) if tile == 128 else ()):
        ref, got = ws_c.get(n).float(), ws_g.get(n).float().cpu()
        err = (got - ref).abs().max().item()
        assert err <= 2e-3 * max(1.0, ref.abs().max().item()), (n, err)
    if tile == 128:
        # the same launch on v_mfma_f32_32x32x16_bf16 (aew_tuning_t.tn_mfma32): half the MFMA instructions, the same products in
        # 16-row instead of 32-row partial sums - equal to fp32 rounding, by-products and the split descriptor included
        keep = {n: ws_g.get(n).clone() for n in ("o1", "o2", "o3", "o4", "snap", "snap2", "cs1", "cs2")}
        for n in ("o1", "o2", "o3", "o4", "snap", "snap2", "cs1"):
            ws_g.get(n).zero_()
        p.run(stream(), tuning=L.current_tuning(tn_mfma32=1))
        torch.cuda.synchronize()
        for n, ref in keep.items():
            got = ws_g.get(n)
            err = (got - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (n, err)
            assert n in ("cs2",) or not torch.equal(got, torch.zeros_like(got)), n
        assert torch.all(ws_g.get("cs2")[368:384].cpu() == -7.0)
    # the per-matrix ops (split-K slabs summed afterwards) give the same matrices
    for i, (t, n) in enumerate(zip(build(ws_g), ("o1", "o2", "o3"))):
        slabs = L.tn_slabs(t)
        assert slabs <= 8
        t.out = ws_g.get(n + ".ref").data_ptr()
        p = Plan("t")
        p.add(L.OP_GEMM_TN, t, "tn")
        p.run(stream())
        torch.cuda.synchronize()
        numel = t.N_pad * t.K_total
        ref = ws_g.get(n + ".ref")[:slabs * t.out_batch_stride].view(slabs, -1)[:, :numel].sum(0).cpu()
        got = ws_g.get(n)[:numel].cpu()
        assert (got - ref).abs().max().item() <= 1e-3 * max(1.0, ref.abs().max().item()), n
    # snapshots: running sums over the batch elements of column 368 (= column sums of G1 rows, since A1[:, 368] = 1)
    g1 = ws_c.get("G1")[:B * 700 * 256].view(B, 700, 256).float()
    run_sum = torch.cumsum(g1[:, :690].sum(1), 0)
    assert (ws_g.get("snap")[:B * 256].view(B, 256).cpu() - run_sum).abs().max().item() <= 2e-3 * run_sum.abs().max().item()
    # snap_k = -1: the same for a matrix without a ones channel (rows of G2 below its row limit 640, all 384 columns)
    g2 = ws_c.get("G2")[:B * 650 * 384].view(B, 650, 384).float()
    run_sum2 = torch.cumsum(g2[:, :640].sum(1), 0)
    assert (ws_g.get("snap2")[:B * 384].view(B, 384).cpu() - run_sum2).abs().max().item() <= 2e-3 * run_sum2.abs().max().item()
    if tile == 384:
        # the 8-wave tiles accumulate every output element over the same 32-row products in the same order as the 128-tile
        # launch: bit-identical, by-products included
        ws_1 = _mirror(ws_c, DEV)
        for n in ("o1", "o2", "o3", "snap", "snap2", "cs1"):
            ws_1.get(n).zero_()
        gb = TnGroupBuilder(ws_1, "tng128", 128)
        for i, t in enumerate(build(ws_1)):
            gb.add(t, f"d{i}")
        p = Plan("g128")
        gb.emit(p, "group")
        p.run(stream())
        torch.cuda.synchronize()
        for n in ("o1", "o2", "o3", "snap", "snap2", "cs1", "cs2"):
            assert torch.equal(ws_1.get(n), ws_g.get(n)), n
    if tile == 128:
        # the same launch paced by the row cursor (aew_gemm_tn_group_t.cursors, aew_set_tn_cursor): the tiles of a matrix
        # wait for each other every few stages, which changes when a row is read and nothing about what is summed
        lib = L.load()
        ws_2 = _mirror(ws_c, DEV)
        for n in ("o1", "o2", "o3", "o4", "snap", "snap2", "cs1"):
            ws_2.get(n).zero_()
        gb = TnGroupBuilder(ws_2, "tngc", tile)
        gb.cursor = True
        for i, t in enumerate(build(ws_2)):
            if i == 3:
                gb.set_split(t, 220)
            gb.add(t, f"d{i}")
        p = Plan("g")
        gb.emit(p, "group")
        assert p.labels[0].startswith("zero:") and len(p.ops) == 2
        try:
            for epoch, slack in ((3, 1), (4, 2), (0, 0)):                   # (0, -): the defaults 4 / 2
                assert lib.aew_set_tn_cursor(epoch, slack) == 0
                epoch = epoch or 4
                p.run(stream())
                torch.cuda.synchronize()
                prog = ws_2.get("tngc.cursors").view(-1, 64).cpu()
                stages = 3 * ((690 + 31) // 32)
                assert int(prog[0, :14].min()) == int(prog[0, :14].max()) == (stages - 1) // epoch, prog[0, :16]
                assert int(prog[2].max()) == 0 or 3 * 2 > epoch            # the 33-row matrix has 6 stages
                for n in ("o1", "o2", "o3", "o4", "snap", "snap2", "cs1", "cs2"):
                    assert torch.equal(ws_2.get(n), ws_g.get(n)), (n, epoch, slack)
            assert lib.aew_set_tn_cursor(1, 1) != 0 and lib.aew_set_tn_cursor(4, 9) != 0
            assert lib.aew_set_tn_cursor(-1, 0) == 0                        # veto: the unpaced kernel, counters untouched
            ws_2.get("tngc.cursors").fill_(7)
            p.ops = p.ops[1:]                                               # (without the op that zeroes them)
            p.labels = p.labels[1:]
            p._arr = None
            p.run(stream())
            torch.cuda.synchronize()
            assert int(ws_2.get("tngc.cursors").min()) == 7 and torch.equal(ws_2.get("o1"), ws_g.get("o1"))
        finally:
            lib.aew_set_tn_cursor(0, 0)


@pytest.mark.parametrize("Np,ks", [(256, (128, 128, 256)), (384, (128, 256)), (128 * 5, (384, 384, 128)), (512, (384, 384, 128))])
def test_gemm_tn_big_tiles(Np, ks):
    """256 x 256-tile wgrad kernel (k_gemm_tn_bf16_big) against the 128 x 128 kernel and the scalar check kernel: halves of
    128 columns, so K_total / N_pad that are odd multiples of 128 and tiles that straddle two segments are covered."""
    lib = L.load()
    gen = torch.Generator().manual_seed(5)
    B, Mc = 3, 2500
    R0 = Mc + 43
    ws_c = Workspace("cpu")
    ws_c.alloc("G", B * R0 * Np, torch.bfloat16)
    ws_c.alloc("A1", B * R0 * 384, torch.bfloat16); ws_c.alloc("A2", B * R0 * 384, torch.bfloat16)
    for n in ("G", "A1", "A2"):
        _fill(ws_c, n, gen)

    def build(ws, impl):
        Gm = Mat(ws, "G", B, R0, Np, BF)
        A1 = Mat(ws, "A1", B, R0, 384, BF)
        A2 = Mat(ws, "A2", B, R0, 384, BF)
        segs = [(A1 if i % 2 == 0 else A2).seg(k, row_off=(0, 16, -4)[i % 3], hi=R0 - 5 if i == 1 else None) for i, k in enumerate(ks)]
        t = make_tn(BF, Mc, B, Np - 8, Np, Gm.seg(Np, row_off=3, hi=Mc - 77), segs, impl=impl)
        slabs = L.tn_slabs(t)
        ws.alloc("out", slabs * Np * t.K_total, torch.float32)
        t.out, t.out_batch_stride = ws.get("out").data_ptr(), Np * t.K_total
        return t, slabs

    res = {}
    try:
        for tag, big, impl in (("big", 1, 0), ("small", 0, 0), ("check", 0, 1)):
            lib.aew_set_tn_big(big, 0)
            ws_g = _mirror(ws_c, DEV)
            t, slabs = build(ws_g, impl)
            p = Plan("tn"); p.add(L.OP_GEMM_TN, t, "tn"); p.run(stream())
            torch.cuda.synchronize()
            res[tag] = ws_g.get("out")[:slabs * Np * t.K_total].view(slabs, Np, t.K_total).sum(0).cpu()
    finally:
        lib.aew_set_tn_big(0, 0)                              # the library default
    scale = res["check"].abs().max().item()
    assert scale > 0
    for tag in ("big", "small"):
        err = (res[tag] - res["check"]).abs().max().item()
        assert err <= 2e-3 * scale, (tag, err, scale)


@pytest.mark.parametrize("tiled", [True, False])
def test_copy_table_transposing_records(tiled):
    """AEW_OP_COPY_TABLE on the record shapes of the weight packs (conv weight [o][c][k] -> dgrad layout [(c, k)][o],
    gate-permuted groups, a k = 1 transpose into a wider matrix, ragged extents, fp32 and bf16 destinations, a scale),
    tiled through LDS and element-wise: both bit-identical to the interpreter's definition of the op."""
    gen = torch.Generator().manual_seed(11)
    ws_c = Workspace("cpu")
    ws_c.alloc("src", 768 * 2304 + 64, torch.float32); _fill(ws_c, "src", gen)
    for n, sz, dt in (("d_bf", 2304 * 768 + 64, torch.bfloat16), ("d_f", 2304 * 768 + 64, torch.float32), ("d_g", 16 * 1024 * 40, torch.bfloat16),
                      ("d_r", 117 * 768 + 64, torch.bfloat16), ("d_o", 130 * 77 + 64, torch.bfloat16), ("d_w", 368 * 640 + 64, torch.bfloat16),
                      ("d_e", 64 * 2304, torch.float32), ("d_i", 64 * 2304, torch.float32), ("d_t", 16 * 736, torch.float32),
                      ("d_s", 64 * 120, torch.float32), ("d_p", 16 * 28672 + 64, torch.bfloat16)):
        ws_c.alloc(n, sz, dt)
    cases = [  # name, dims, source strides, destination strides, destination type, scale, expected to be tiled
        ("d_bf", (768, 768, 3), (2304, 3, 1), (1, 2304, 768), BF, 1.0, True),        # encoder conv -> [c][k][o]
        ("d_f", (768, 768, 3), (2304, 3, 1), (1, 2304, 768), F3, 0.5, True),
        ("d_g", (16, 368, 2, 16), (11776, 2, 1, 736), (32, 1024, 512, 1), BF, 1.0, False),  # gate-permuted: 16-wide runs, element-wise
        ("d_r", (768, 39, 3), (117, 3, 1), (1, 2304, 768), BF, 1.0, True),           # 117 = 3.66 tiles of 32
        ("d_o", (77, 130), (130, 1), (1, 77), BF, 1.0, True),                        # odd extents: 2-byte stores
        ("d_w", (368, 256), (256, 1), (1, 640), BF, 1.0, True),                      # k = 1 transpose into a wider matrix
        ("d_e", (64, 768, 3), (2304, 3, 1), (2304, 1, 768), F3, 1.0, False),         # [c][k] -> [k][c] inside a row: element-wise
        ("d_i", (64, 3, 768), (2304, 768, 1), (2304, 1, 3), F3, 1.0, False),         # ... and back (gradient unpack)
        ("d_t", (16, 2, 368), (896, 384, 1), (736, 1, 2), F3, 1.0, False),           # two taps
        ("d_s", (64, 40, 3), (120, 3, 1), (120, 1, 40), F3, 1.0, False),             # 40 channels: interleave form too
        ("d_p", (16, 16, 368, 2), (11776, 736, 2, 1), (28672, 896, 1, 384), BF, 0.25, False)]   # decoder pack: two taps -> bf16 planes

    ilv = {"d_e": -3, "d_i": -3, "d_t": -2, "d_s": -3, "d_p": -2}                      # the (de)interleaves: register-permutation form, k taps

    def build(ws):
        keep = PL.CopyTableBuilder.tiled, PL.CopyTableBuilder.interleave
        PL.CopyTableBuilder.tiled = PL.CopyTableBuilder.interleave = tiled
        try:
            tb = PL.CopyTableBuilder(ws, "t.tbl")
            for name, dims, ss, ds, dt, scale, _ in cases:
                tb.add(ws.get("src").data_ptr() + 4 * 8, ws.get(name).data_ptr(), dims, ss, ds, F3, dt, scale=scale)
        finally:
            PL.CopyTableBuilder.tiled, PL.CopyTableBuilder.interleave = keep
        assert [r.tr_a > 0 for r in tb.recs] == [c[-1] and tiled for c in cases]
        assert [r.tr_a for r in tb.recs if r.tr_a < 0] == ([ilv[c[0]] for c in cases if c[0] in ilv] if tiled else [])
        p = Plan("t")
        tb.emit(p, "copy")
        return p
    ws_g = _mirror(ws_c, DEV)
    build(ws_g).run(stream())
    torch.cuda.synchronize()
    ws_e = Workspace("cpu")
    for n, t in ws_c.bufs.items():
        ws_e.bufs[n] = t.clone()
    Emu(ws_e).run(build(ws_e))
    for name in ("d_bf", "d_g", "d_r", "d_o", "d_w", "d_p"):
        assert torch.equal(ws_g.get(name).cpu().view(torch.int16), ws_e.get(name).view(torch.int16)), name
    for name in ("d_f", "d_e", "d_i", "d_t", "d_s"):
        assert torch.equal(ws_g.get(name).cpu(), ws_e.get(name)), name


@pytest.mark.parametrize("dtype", [BF, F3])
def test_moments_and_vq_stats_ops(dtype):
    """The two small reductions added in round 2 against the plan interpreter: AEW_OP_MOMENTS over a strided view with
    rows outside the view (read as zero), both storage types; VQ_STATS in its few-queries form (one wave per query owns
    its code) on a collapsed assignment (every query on two codes: the 16-rows-in-flight path) - bit-identical to the
    interpreter's ascending-order sums, like the many-queries form."""
    gen = torch.Generator().manual_seed(3)
    ws_c = Workspace("cpu")
    B, R, pitch, cols = 3, 57, 128, 39
    ws_c.alloc("x", B * R * pitch, PL.TORCH_DT[dtype])
    _fill(ws_c, "x", gen)
    ws_c.alloc("mom", 8, torch.float32)
    Q, K, d = 232, 4096, 32
    ws_c.alloc("ze", Q * 64, torch.float32); _fill(ws_c, "ze", gen)
    ind = torch.randint(0, K, (Q,), generator=gen)
    ind[5:] = torch.where(torch.arange(Q - 5) % 3 == 0, torch.tensor(17), torch.tensor(4000))     # two crowded codes
    ws_c.bufs["ind"] = ind.clone()
    for n, sz in (("zsum", K * d), ("nsum", K), ("hist", K)):
        ws_c.alloc(n, sz, torch.float32)
    ws_c.get("hist").fill_(2.0)

    def build(ws):
        x = Mat(ws, "x", B, R, pitch, dtype)
        mo = L.Moments()
        mo.x, mo.rows, mo.cols, mo.batch = x.view(row_off=-3, hi=R - 4), R, cols, B        # 3 + 4 rows read as zero
        mo.out = ws.get("mom").data_ptr()
        vs = L.VqStats()
        vs.ze, vs.ind, vs.Q, vs.K, vs.d, vs.d_pitch = ws.get("ze").data_ptr(), ws.get("ind").data_ptr(), Q, K, d, 64
        vs.z_sum, vs.n_sum, vs.hist = ws.get("zsum").data_ptr(), ws.get("nsum").data_ptr(), ws.get("hist").data_ptr()
        p = Plan("t")
        p.add(L.OP_MOMENTS, mo, "moments")
        p.add(L.OP_VQ_STATS, vs, "vq.stats")
        return p
    ws_g = _mirror(ws_c, DEV)
    build(ws_g).run(stream())
    torch.cuda.synchronize()
    ws_e = Workspace("cpu")
    for n, t in ws_c.bufs.items():
        ws_e.bufs[n] = t.clone()
    Emu(ws_e).run(build(ws_e))
    got, ref = ws_g.get("mom")[:4].cpu(), ws_e.get("mom")[:4]
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-6), (got, ref)
    # ascending-q fp32 chains, restated here (vqema_bn.py:172-188 sums in this order)
    ze = ws_c.get("ze")[:Q * 64].view(Q, 64)[:, :d].numpy()
    zs = np.zeros((K, d), np.float32)
    ns = np.zeros(K, np.float32)
    for q in range(Q):
        k = int(ind[q])
        zs[k] = zs[k] + ze[q]
        ns[k] += 1.0
    assert np.array_equal(ws_g.get("zsum")[:K * d].cpu().numpy().reshape(K, d), zs)
    assert np.array_equal(ws_g.get("nsum")[:K].cpu().numpy(), ns)
    assert np.array_equal(ws_g.get("hist")[:K].cpu().numpy(), ns + 2.0)
    assert torch.allclose(ws_e.get("zsum")[:K * d].view(K, d), torch.from_numpy(zs), rtol=1e-6, atol=1e-6)     # the interpreter too


# ----------------------------------------------------------------------------------------------
# whole training steps on the reduced-width golden models: GPU vs interpreter vs golden
# ----------------------------------------------------------------------------------------------
def tiny_hps(z, **over):
    h = json.loads(str(z["hps_json"]))
    n_mel = h.pop("n_mel_ch", None)
    return config.make_hps(**{k: v for k, v in h.items() if k not in over}, **over), n_mel


def build_pair(z, kind, n_mel, **kw):
    hps, nm = tiny_hps(z, global_model=kind)
    B = z["wav"].shape[0]
    engs = []
    for dev in ("cpu", DEV):
        e = M.TrainEngine(hps, B=B, device=dev, n_mel=n_mel or nm, take_compat=True,
                          update_codebook_every_step=False, **kw)
        for k in e.ps.names():
            e.ps.view(k).copy_(torch.from_numpy(z["w." + k]))
        if e.bn_type == "vqvae-ema":
            e.emb.copy_(torch.from_numpy(z["emb0"]))
            e.init_ema_from_emb()
        engs.append(e)
    return hps, engs[0], engs[1]


def run_pair(ec, eg, z, eps=None):
    args = [torch.from_numpy(z[k]) for k in ("wav", "mel", "voice", "jitter")]
    ec.set_inputs(*args, eps=eps)
    eg.set_inputs(*[a.to(DEV) for a in args], eps=None if eps is None else eps.to(DEV))
    emu = Emu(ec.ws)
    for name in ("fwd_a", "fwd_b", "bwd"):
        emu.run(getattr(ec, name))
    eg.forward()
    eg.backward()
    torch.cuda.synchronize()


def diff_workspaces(ec, eg, skip_prefix=("tbl.", "in.", "adam.", "scratch.")):
    """First buffers (in allocation order) whose GPU content deviates from the interpreter."""
    bad = []
    for n, tc in ec.ws.bufs.items():
        if n.startswith(skip_prefix) or ".wg." in n or n.startswith("enc.wg") or n.startswith("bn.wg") or "tbl." in n \
                or n == "bn.vq_part" or ".tng" in n or n.startswith("tng") or "det." in n:
            continue                     # wgrad slabs / search scratch: implementation detail; tables hold pointers
        tg = eg.ws.get(n).cpu()
        if tc.dtype in (torch.int64, torch.int32):
            if n == "diag.amax_pos":
                # arg-max class per position: the two forwards differ by bf16 rounding noise, near-ties may flip
                if (tc != tg).float().mean().item() > 0.02:
                    bad.append((n, "arg-max classes differ in more than 2 % of the positions"))
            elif not torch.equal(tc, tg):
                bad.append((n, "int mismatch"))
            continue
        a, b = tc.float(), tg.float()
        scale = max(a.abs().max().item(), 1e-6)
        err = (a - b).abs().max().item() / scale
        lim = 3e-2 if tc.dtype == torch.bfloat16 else 2e-2
        if not np.isfinite(err) or err > lim:
            bad.append((n, round(err, 5)))
    return bad


def grads_vs_golden(eng, z, tag, lim=0.25):
    cs = []
    for k in eng.ps.names():
        ref = z[f"{tag}.{k}"]
        got = eng.ps.view(k, grad=True).cpu().numpy()
        if ref.size == 0:
            assert np.abs(got).max() == 0, k
            continue
        # toy-width nets under bf16: ReLU-mask flips move small tensors by O(1/width); the tight
        # check is GPU-vs-interpreter above, here the direction vs the fp32 golden: every tensor, and - so that a
        # regression shows before a single tensor falls through the floor - the distribution over the tensors
        cos = float((got * ref).sum() / max(np.linalg.norm(got) * np.linalg.norm(ref), 1e-30))
        cs.append((cos, k))
        assert cos > COS_FLOOR, (k, cos)
    cs.sort()
    med, p10 = cs[len(cs) // 2][0], cs[len(cs) // 10][0]
    print(f"gradient cosines vs golden ({tag}): min {cs[0][0]:.4f} ({cs[0][1]}), 10th percentile {p10:.4f}, median {med:.5f}")
    assert med > COS_MEDIAN and p10 > COS_P10, (cs[0], p10, med)


# measured over the seven golden cases: min 0.968 (one gated bias of the jittered MFCC-inverter case), everything else
# >= 0.9997; 10th percentile >= 0.987, median >= 0.9927
COS_FLOOR, COS_P10, COS_MEDIAN = 0.95, 0.98, 0.99


@pytest.mark.parametrize("tag", ["identity", "jitter"])
def test_mfcc_inverter_step(golden_dir, tag):
    z = load(golden_dir, f"mi_tiny_{tag}.npz")
    hps, ec, eg = build_pair(z, "mfcc_inverter", 7)
    run_pair(ec, eg, z)
    bad = diff_workspaces(ec, eg)
    assert not bad, bad[:8]
    pred = eg.logits()[:, :-1, :].permute(0, 2, 1).cpu().numpy()
    np.testing.assert_allclose(pred, z["pred"], rtol=5e-2, atol=3e-2)
    assert abs(float(eg.loss_buf[0]) - float(z["loss"])) < 2e-2
    grads_vs_golden(eg, z, "grad")


@pytest.mark.parametrize("name,gtag,ltag,kw", [
    ("ae_tiny_vqvae-ema_random.npz", "gint", "loss_intended", dict(loss_mode="intended")),
    ("ae_tiny_vqvae-ema_identity.npz", "ghead", "loss_head", dict(loss_mode="head")),
    ("ae_tiny_ae_identity.npz", "g", "loss", {}),
    ("ae_tiny_vqvae_identity.npz", "gint", "loss_intended", {}),
])
def test_autoencoder_step(golden_dir, name, gtag, ltag, kw):
    z = load(golden_dir, name)
    hps, ec, eg = build_pair(z, "autoencoder", None, **kw)
    run_pair(ec, eg, z)
    bad = diff_workspaces(ec, eg)
    assert not bad, bad[:8]
    if "min_ind" in z:
        assert np.array_equal(eg.ind[:eg.Q].view(eg.B, -1).cpu().numpy(), z["min_ind"])       # bit-exact
    assert abs(float(eg.loss_buf[0]) / float(z[ltag]) - 1) < 1e-2
    grads_vs_golden(eg, z, gtag)
    if hps.bn_type == "vqvae-ema":
        np.testing.assert_array_equal(eg.n_sum.cpu().numpy(), z["n_sum"])
        np.testing.assert_allclose(eg.z_sum.cpu().numpy(), z["z_sum"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(eg.ema_numer.cpu().numpy(), z["ema_numer"], rtol=1e-5, atol=1e-7)
        from tests.test_plan_cpu import check_diagnostics
        check_diagnostics(np.concatenate([eg.diag.cpu().numpy()[:6], eg.diag_pk.cpu().numpy()[6:9]]), z, exact=False)
        eg.update_codebook()
        np.testing.assert_allclose(eg.emb.cpu().numpy(), z["emb1"], rtol=1e-4, atol=1e-6)


def test_autoencoder_vae_step(golden_dir):
    z = load(golden_dir, "ae_tiny_vae_random.npz")
    hps, _ = tiny_hps(z, global_model="autoencoder")
    hps = config.make_hps(**{**dict(hps), "bn_free_nats": float(z["free_nats"])})
    engs = []
    for dev in ("cpu", DEV):
        e = M.TrainEngine(hps, B=2, device=dev, n_mel=9, take_compat=True)
        for k in e.ps.names():
            e.ps.view(k).copy_(torch.from_numpy(z["w." + k]))
        e.set_anneal_weight(float(z["anneal"]))
        engs.append(e)
    ec, eg = engs
    run_pair(ec, eg, z, eps=torch.from_numpy(z["eps"]))
    bad = diff_workspaces(ec, eg)
    assert not bad, bad[:8]
    assert abs(float(eg.loss_buf[0]) / float(z["loss"]) - 1) < 1e-2
    grads_vs_golden(eg, z, "g")


@pytest.mark.parametrize("B", [16, 20, 37])
def test_speaker_and_bias_gradients_at_large_batch(B):
    """Round-3 ADVICE: the speaker backward kept B and G in registers (B <= 16 only) and, with the grouped wgrads, recovers
    the per-batch column sums of dfg as differences of running fp32 snapshots - worse cancellation for later batch
    elements.  B = 16 (the reference default n_batch: the edge of the old kernel), B = 20 and 37 (two and three chunks of
    16 batch elements: partial sums added with atomics): gated biases, speaker projections, speaker embedding against the
    CPU interpreter of the same plans."""
    hps = config.make_hps("mi", n_res=32, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, n_global_embed=10, n_speakers=7,
                          n_blocks=2, n_block_layers=3, n_win_batch=40, n_lc_in=12)
    engs = []
    for dev in ("cpu", DEV):
        e = M.TrainEngine(hps, B=B, device=dev, n_mel=12)
        gen = torch.Generator().manual_seed(17)
        for k in e.ps.names():
            e.ps.view(k).copy_(torch.randn(e.ps.shape[k], generator=gen) * 0.25)
        engs.append(e)
    ec, eg = engs
    assert len([op for op in eg.bwd.ops if op.kind == L.OP_SPK_BWD]) == 1
    g = ec.geom
    gen = torch.Generator().manual_seed(18)
    z = {"wav": torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().numpy(),
         "mel": torch.randn(B, 12, g.mel_len, generator=gen).numpy(),
         "voice": torch.randint(0, 7, (B,), generator=gen).numpy(),
         "jitter": torch.arange(g.embed_len).repeat(B, 1).numpy()}
    run_pair(ec, eg, z)
    checked = 0
    for k in ec.ps.names():
        if not ("speaker_embedding" in k or ".proj_" in k or k.endswith("conv_signal.bias") or k.endswith("conv_gate.bias")):
            continue
        ref, got = ec.ps.view(k, grad=True), eg.ps.view(k, grad=True).cpu()
        scale = float(ref.abs().max())
        assert scale > 0, k
        err = float((got - ref).abs().max()) / scale
        cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0))
        assert err < 3e-2 and cos > 0.999, (k, err, cos)
        checked += 1
    assert checked == 2 + 4 * len(g.layers)


# ----------------------------------------------------------------------------------------------
# bit-exact sub-path at full width: encoder -> linear -> VQ vs the exact-order C oracle
# ----------------------------------------------------------------------------------------------
def seeded_full_engine(B, w, seed=3, n_embed=4096):
    hps = config.make_hps("vqvae-ema", n_win_batch=w, bn_vq_n_embed=n_embed)
    eng = M.TrainEngine(hps, B=B, device=DEV, n_mel=39, update_codebook_every_step=False)
    shapes = {k: eng.ps.shape[k] for k in eng.ps.names()}
    wts = np_weights(shapes, seed)
    for k, v in wts.items():
        eng.ps.view(k).copy_(torch.from_numpy(v))
    rs = np.random.RandomState(seed + 1)
    emb = (rs.standard_normal((n_embed, hps.bn_n_out)) * 0.7).astype(np.float32)
    eng.emb.copy_(torch.from_numpy(emb))
    eng.init_ema_from_emb()
    g = eng.geom
    wav = torch.from_numpy(rs.randint(0, 256, (B, g.enc_in_len)).astype(np.float32))
    mel = torch.from_numpy(rs.standard_normal((B, 39, g.mel_len)).astype(np.float32))
    voice = torch.from_numpy(rs.randint(0, 40, (B,)).astype(np.int64))
    jitter = torch.arange(g.embed_len).repeat(B, 1)
    return hps, eng, wts, emb, (wav, mel, voice, jitter)


def test_encoder_vq_bit_exact_full_width():
    from oracle import exact
    hps, eng, wts, emb, inp = seeded_full_engine(B=2, w=100)
    eng.set_inputs(*[t.to(DEV) for t in inp])
    eng.fwd_a.run(stream())
    torch.cuda.synchronize()
    mel_cl = inp[1].permute(0, 2, 1).contiguous().numpy()
    enc = exact.encoder_cl(wts, "encoder.", mel_cl)
    got_enc = eng.enc.y[9].tensor()[:, :, :768].cpu().numpy()
    assert np.array_equal(got_enc, enc), f"encoder not bit-exact: max diff {np.abs(got_enc - enc).max()}"
    ze = exact.linear_cl(enc, wts["bottleneck.linear.weight"])
    got_ze = eng.lin.tensor()[:, :, :32].cpu().numpy()
    assert np.array_equal(got_ze, ze)
    ind, dist, sec = exact.vq_nearest(ze.reshape(-1, 32), emb, "scaled_l2")
    assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), ind)
    assert np.array_equal(eng.min_dist[:eng.Q].cpu().numpy(), dist)
    z_sum, n_sum = exact.vq_stats(ze.reshape(-1, 32), ind, 4096)
    assert np.array_equal(eng.z_sum.cpu().numpy(), z_sum) and np.array_equal(eng.n_sum.cpu().numpy(), n_sum)
    numer, denom = exact.ema(emb * np.float32(1 - 0.99), np.full(4096, 1 - 0.99, np.float32), z_sum, n_sum, 0.99)
    eng.fwd_b.run(stream())
    torch.cuda.synchronize()
    assert np.array_equal(eng.ema_numer.cpu().numpy(), numer) and np.array_equal(eng.ema_denom.cpu().numpy(), denom)
    eng.update_codebook()
    assert np.array_equal(eng.emb.cpu().numpy(), exact.codebook(numer, denom))
    print(f"min top-2 margin (relative): {((sec - dist) / dist).min():.3e}")


@pytest.mark.parametrize("S", [2, 4])
def test_encoder_split_k_is_exact_in_its_own_order(monkeypatch, S):
    """aew_gemm_nt_t.k_split: the exact fp32 GEMMs as S contiguous k-ranges on separate workgroups, combined in the fixed
    order (p0 + p1) + (p2 + p3) by whichever arrives last.  Bit-identical to the C oracle restating THAT order
    (aewo_conv_cl_split), replay after replay (the arrival order must not enter the result), and the code indices still
    equal the torch oracle's on this input.  (Measured no faster than the single chain: off by default.)"""
    from oracle import exact
    from ae_wavenet_amd import engine as E
    monkeypatch.setattr(E.EncoderPlan, "k_split", S)
    monkeypatch.setattr(exact, "KSPLIT", S)
    hps, eng, wts, emb, inp = seeded_full_engine(B=2, w=100)
    assert eng.fwd_a.ops[[i for i, lab in enumerate(eng.fwd_a.labels) if lab == "enc.1"][0]].u.nt.k_split == S
    assert eng.fwd_a.ops[eng.fwd_a.labels.index("enc.0")].u.nt.k_split == 0          # 39 mel channels: padded, not split
    eng.set_inputs(*[t.to(DEV) for t in inp])
    mel_cl = inp[1].permute(0, 2, 1).contiguous().numpy()
    enc = exact.encoder_cl(wts, "encoder.", mel_cl)
    ze = exact.linear_cl(enc, wts["bottleneck.linear.weight"])
    ind, dist, sec = exact.vq_nearest(ze.reshape(-1, 32), emb, "scaled_l2")
    for rep in range(3):
        eng.init_ema_from_emb()
        eng.fwd_a.run(stream())
        torch.cuda.synchronize()
        assert np.array_equal(eng.enc.y[9].tensor()[:, :, :768].cpu().numpy(), enc), rep
        assert np.array_equal(eng.lin.tensor()[:, :, :32].cpu().numpy(), ze), rep
        assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), ind), rep
    monkeypatch.setattr(exact, "KSPLIT", 1)
    assert not np.array_equal(exact.encoder_cl(wts, "encoder.", mel_cl), enc)          # (the orders do differ)


def test_small_launch_split_k_hint(monkeypatch):
    """aew_gemm_nt_t.k_split as a hint on bf16 launches of a few dozen 64 x 64 blocks (the upsampler / encoder data
    gradients at the headline batch: wavenet.py:275, wave_encoder.py:39 backward): S copies of the tile grid contract S
    ranges of K; the partial accumulators meet in ascending order in the workgroup that arrives last.  Same operands, fp32
    accumulation in another order: every gradient within bf16 round-off of the unsplit step's, and the same bits replay
    after replay (the arrival order must not enter the result)."""
    B, w = 8, 5000
    _, e0, _, _, inp = seeded_full_engine(B=B, w=w)
    monkeypatch.setattr(M.TrainEngine, "small_split", 256)
    _, e1, _, _, _ = seeded_full_engine(B=B, w=w)
    made = dict(e1.small_split_made)
    assert not e0.small_split_made and made.get("d.ups0", 0) >= 2 and any(k.startswith("d.enc") for k in made), made
    assert all(2 <= s <= 8 for s in made.values())
    outs = []
    for e in (e0, e1, e1):
        e.init_ema_from_emb()
        e.set_inputs(*[t.to(DEV) for t in inp])
        loss = float(e.forward())
        e.backward()
        torch.cuda.synchronize()
        outs.append((loss, e.enc.dy[0].tensor().clone(), {k: e.ps.view(k, grad=True).clone() for k in e.ps.names()}))
    (l0, m0, g0), (l1, m1, g1), (l2, m2, _) = outs
    assert torch.equal(m1, m2) and l1 == l2                  # the mel gradient: the end of every split launch's chain
    assert abs(l1 / l0 - 1) < 1e-4
    worst = max(((g1[k] - g0[k]).norm().item() / max(g0[k].norm().item(), 1e-30), k) for k in g0 if g0[k].abs().max() > 0)
    mel = (m1 - m0).norm().item() / m0.norm().item()
    print(f"split-K hint on {len(made)} launches ({made}): loss rel dev {abs(l1 / l0 - 1):.2e}, mel gradient rel L2 {mel:.2e}, "
          f"worst gradient rel L2 {worst[0]:.2e} ({worst[1]})")
    # (measured 5.1e-2 / 5.1e-2: all of it from the two FORWARD launches, ups0 / ups1 - a conditioning vector a bf16
    # round-off apart moves the encoder-side gradients by 2.6-4.6 % while the loss moves by 4e-7: the sensitivity DESIGN 4
    # describes, the same size as the step's distance to the fp32 oracle; the backward launches move them by 1e-4 .. 5e-3
    # each: tools/split_debug.py)
    assert worst[0] < 0.12 and mel < 0.12


# ----------------------------------------------------------------------------------------------
# full-width training step vs the torch fp32 oracle
# ----------------------------------------------------------------------------------------------
REL_L2_MEDIAN, REL_L2_WORST = 0.10, 0.13         # measured 0.084 / 0.105 (deterministic kernels: the same on every box)


def test_full_width_step_vs_oracle():
    from oracle import ref_model as R
    hps, eng, wts, emb, inp = seeded_full_engine(B=2, w=100)
    eng.set_inputs(*[t.to(DEV) for t in inp])
    loss = eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in wts.items()}
    out = R.ae_run(sd, {"emb": torch.from_numpy(emb)}, hps, eng.geom, *inp, loss_mode="intended", take_compat=False)
    out["loss"].backward()
    assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), out["min_ind"].reshape(-1).numpy()), \
        "end-to-end code indices differ from the fp32 oracle"
    lg = eng.logits().permute(0, 2, 1).cpu()
    err = (lg - out["quant"].detach()).abs().max().item()
    print(f"logit max abs err {err:.4f} (scale {out['quant'].abs().max().item():.2f})")
    assert err <= 0.06
    rel = abs(float(loss) / float(out["loss"]) - 1)
    print(f"loss {float(loss):.5f} vs oracle {float(out['loss']):.5f}: rel {rel:.2e}")
    assert rel < 1e-4            # (measured <= 1e-5: the logit errors of the bf16 decoder average out over the positions)
    worst = (0.0, "")
    rl2 = []
    for k in eng.ps.names():
        ref = sd[k].grad
        got = eng.ps.view(k, grad=True).cpu()
        if ref is None:
            continue
        scale = ref.abs().max().item()
        if scale == 0:
            continue
        e = (got - ref).abs().max().item() / scale
        cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
        worst = max(worst, (e, k))
        rl2.append(((got - ref).norm().item() / ref.norm().item(), k))
        assert e < 0.15 and cos > 0.99, (k, e, cos)
    print("worst gradient max-normalised error:", worst)
    # whole-tensor view next to the worst-element bound above (whose margin is thin: one ReLU-mask flip moves one element
    # of one gradient by a whole contribution): relative L2 per tensor.  A regression shows here long before the
    # max-normalised bound goes
    rl2.sort()
    med, hi = rl2[len(rl2) // 2][0], rl2[-1]
    print(f"relative L2 of the {len(rl2)} gradient tensors: median {med:.4f}, worst {hi[0]:.4f} ({hi[1]})")
    assert med < REL_L2_MEDIAN and hi[0] < REL_L2_WORST, (med, hi)


def test_full_width_step_vs_interpreter_buffer_by_buffer():
    """The tight full-width check: the same plans executed by the CPU interpreter with the REAL storage types (bf16
    decoder buffers) on the full-width model (768-wide encoder, K = 4096 codes, 20 x 368/256 decoder; B = 2, w = 100).

    Forward: every workspace buffer GPU vs interpreter at the toy-width limits (3e-2 of the buffer's maximum for bf16,
    2e-2 for fp32).  Backward: TEACHER-FORCED - the interpreter starts from the GPU's own forward state.  Free-running,
    the two forwards differ by bf16 rounding noise (~0.8 % relative L2 in h0 / h1 after 20 layers), which flips the
    ReLU mask of the ~0.3 % of units whose pre-activation lies inside it; every flip swaps a whole gradient
    contribution, so ANY two correct implementations differ by sqrt(2 * 0.003) ~ 8 % relative L2 in every gradient
    (measured: 7.8 % in dh1, 10 % downstream) - the same effect that sets the 15 % bound against the fp32 oracle.  With
    the masks pinned, every backward buffer and every parameter gradient has to agree to bf16 rounding: an indexing
    error that moves one column of one tensor shows up here."""
    hps, eg, wts, emb, inp = seeded_full_engine(B=2, w=100)
    ec = M.TrainEngine(hps, B=2, device="cpu", n_mel=39, update_codebook_every_step=False)
    for k, v in wts.items():
        ec.ps.view(k).copy_(torch.from_numpy(v))
    ec.emb.copy_(torch.from_numpy(emb))
    ec.init_ema_from_emb()
    ec.set_inputs(*inp)
    eg.set_inputs(*[t.to(DEV) for t in inp])
    emu = Emu(ec.ws)
    for name in ("fwd_a", "fwd_b"):
        emu.run(getattr(ec, name))
    eg.forward()
    torch.cuda.synchronize()
    assert torch.equal(ec.ind[:ec.Q], eg.ind[:eg.Q].cpu())
    bad = diff_workspaces(ec, eg)
    assert not bad, ("forward", bad[:12])
    worst_fwd = 0.0
    for n in ("decoder.h0", "decoder.h1", "decoder.logits", "decoder.cond", "decoder.x19", "decoder.z10", "bn.zq"):
        a, b = ec.ws.get(n).float(), eg.ws.get(n).cpu().float()
        worst_fwd = max(worst_fwd, float((a - b).norm() / a.norm()))
    print(f"forward, free-running: worst relative L2 of the sampled activation buffers {worst_fwd:.3e}")
    assert worst_fwd < 2e-2
    # ---- backward from the GPU's forward state
    for n, t in ec.ws.bufs.items():
        if "tbl." not in n and ".tng" not in n:                                 # (the copy tables hold each workspace's own pointers)
            t.copy_(eg.ws.get(n).cpu())
    emu.run(ec.bwd)
    eg.backward()
    torch.cuda.synchronize()
    bad = diff_workspaces(ec, eg)
    assert not bad, ("backward", bad[:12])
    rows = []
    for k in eg.ps.names():
        a, b = ec.ps.view(k, grad=True).float(), eg.ps.view(k, grad=True).cpu().float()
        na = float(a.norm())
        if na == 0:
            assert float(b.abs().max()) == 0, k
            continue
        rows.append((float((a - b).norm()) / na, float((a - b).abs().max()) / float(a.abs().max()), k))
    rows.sort(reverse=True)
    print("relative-L2 / max-normalised error of the parameter gradients, GPU vs interpreter (worst 8 of %d):" % len(rows))
    for r in rows[:8]:
        print("   %.3e  %.3e  %s" % r)
    print("   median relative L2 %.3e" % sorted(r[0] for r in rows)[len(rows) // 2])
    assert rows[0][0] < 2e-2, rows[0]
    assert max(r[1] for r in rows) < 3e-2, max(rows, key=lambda r: r[1])


DEEP_REL_L2_MEDIAN, DEEP_REL_L2_WORST = 0.12, 0.17         # measured 0.102 / 0.146


def test_deep_decoder_step_vs_oracle():
    """BASELINE configs[4] architecture (30 dilation layers x 512 residual channels), short window: one training step
    against the fp32 oracle - code indices exact, logits / loss / gradients within the stated bf16 tolerances."""
    from oracle import ref_model as R
    hps = config.make_hps("deep", n_win_batch=64, bn_vq_n_embed=512)
    B = 1
    eng = M.TrainEngine(hps, B=B, device=DEV, n_mel=39, update_codebook_every_step=False)
    assert len(eng.geom.layers) == 30 and hps.n_res == 512
    shapes = {k: eng.ps.shape[k] for k in eng.ps.names()}
    wts = np_weights(shapes, 21)
    for k, v in wts.items():
        eng.ps.view(k).copy_(torch.from_numpy(v))
    rs = np.random.RandomState(22)
    emb = (rs.standard_normal((512, hps.bn_n_out)) * 0.7).astype(np.float32)
    eng.emb.copy_(torch.from_numpy(emb))
    eng.init_ema_from_emb()
    g = eng.geom
    inp = (torch.from_numpy(rs.randint(0, 256, (B, g.enc_in_len)).astype(np.float32)),
           torch.from_numpy(rs.standard_normal((B, 39, g.mel_len)).astype(np.float32)),
           torch.from_numpy(rs.randint(0, 40, (B,)).astype(np.int64)), torch.arange(g.embed_len).repeat(B, 1))
    eng.set_inputs(*[t.to(DEV) for t in inp])
    loss = eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in wts.items()}
    out = R.ae_run(sd, {"emb": torch.from_numpy(emb)}, hps, g, *inp, loss_mode="intended", take_compat=False)
    out["loss"].backward()
    assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), out["min_ind"].reshape(-1).numpy())
    lg = eng.logits().permute(0, 2, 1).cpu()
    err = (lg - out["quant"].detach()).abs().max().item()
    print(f"DEEP: logit max abs err {err:.4f} (scale {out['quant'].abs().max().item():.2f})")
    assert err <= 0.08
    rel = abs(float(loss) / float(out["loss"].detach()) - 1)
    print(f"DEEP: loss {float(loss):.5f} vs oracle {float(out['loss'].detach()):.5f}: rel {rel:.2e}")
    assert rel < 1e-3
    worst = (0.0, "")
    rl2 = []
    for k in eng.ps.names():
        ref = sd[k].grad
        if ref is None or ref.abs().max().item() == 0:
            continue
        got = eng.ps.view(k, grad=True).cpu()
        e = (got - ref).abs().max().item() / ref.abs().max().item()
        cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
        worst = max(worst, (e, k))
        rl2.append(((got - ref).norm().item() / ref.norm().item(), k))
        assert e < 0.2 and cos > 0.985, (k, e, cos)
    print("DEEP: worst gradient max-normalised error:", worst)
    rl2.sort()
    med, hi = rl2[len(rl2) // 2][0], rl2[-1]
    print(f"DEEP: relative L2 of the {len(rl2)} gradient tensors: median {med:.4f}, worst {hi[0]:.4f} ({hi[1]})")
    assert med < DEEP_REL_L2_MEDIAN and hi[0] < DEEP_REL_L2_WORST, (med, hi)


def test_full_window_forward_vs_oracle():
    """BASELINE configs[1] window (w = 5000, full width), one window: logits of all 5000 positions, loss and
    code indices against the fp32 oracle (forward only: the oracle needs ~2 s for it on the host)."""
    from oracle import ref_model as R
    hps, eng, wts, emb, inp = seeded_full_engine(B=1, w=5000, seed=13)
    eng.set_inputs(*[t.to(DEV) for t in inp])
    loss = float(eng.forward())
    torch.cuda.synchronize()
    with torch.no_grad():
        sd = {k: torch.from_numpy(v) for k, v in wts.items()}
        out = R.ae_run(sd, {"emb": torch.from_numpy(emb)}, hps, eng.geom, *inp, loss_mode="intended", take_compat=False)
    assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), out["min_ind"].reshape(-1).numpy())
    lg = eng.logits().permute(0, 2, 1).cpu()
    ref = out["quant"]
    err = (lg - ref).abs().max().item()
    rms = ((lg - ref) ** 2).mean().sqrt().item() / (ref ** 2).mean().sqrt().item()
    print(f"w=5000 logit max abs err {err:.4f} (scale {ref.abs().max().item():.2f}), relative rms {rms:.2e}")
    assert err <= 0.06 and rms < 2e-2          # measured 0.019 / 0.93e-2 (bf16 activations through 20 layers)
    rel = abs(loss / float(out["loss"]) - 1)
    print(f"w=5000 loss {loss:.5f} vs oracle {float(out['loss']):.5f}: rel {rel:.2e}")
    assert rel < 1e-4


@pytest.mark.parametrize("fixture", ["mi_full.npz", "mi_full_real.npz"])
def test_mfcc_inverter_full_width_vs_reference_golden(golden_dir, fixture):
    """BASELINE configs[0] shape (mfcc-inverter, B=2, w=100, full width, 13.5 M parameters):
    the GPU path against tensors captured from the UNMODIFIED reference MfccInverter.run
    (tests/golden/mi_full.npz; weights regenerated from the recorded seed).  mi_full_real.npz: the same with
    windows of real mu-law audio cut from the reference's dat/librispeech.some.dat, the file configs[0] names."""
    z = load(golden_dir, fixture)
    z["wav"] = z["wav"].astype(np.float32)
    hps = config.make_hps("mi", n_win_batch=100)
    eng = M.TrainEngine(hps, B=2, device=DEV, n_mel=39, take_compat=True)
    shapes = json.loads(str(z["param_names"]))
    assert shapes == {k: list(eng.ps.shape[k]) for k in eng.ps.names()}
    wts = np_weights(shapes, int(z["seed"]))
    for k, v in wts.items():
        eng.ps.view(k).copy_(torch.from_numpy(v))
    eng.set_inputs(*[torch.from_numpy(z[k]).to(DEV) for k in ("wav", "mel", "voice", "jitter")])
    loss = eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) / float(z["loss"]) - 1) < 5e-3, (float(loss), float(z["loss"]))
    pred = eng.logits()[:, :-1, :].permute(0, 2, 1)[:, :, ::9].cpu().numpy()
    assert np.abs(pred - z["pred_sub"]).max() <= 0.06
    tgt = eng.in_wav[:, eng.geom.wav_out_off + 1: eng.geom.wav_out_off + 100].cpu().numpy()
    assert np.array_equal(tgt, z["target"])
    mg = eng.dec.dlc_src.tensor()[:, :, :39].permute(0, 2, 1).cpu().numpy()
    cos = (mg * z["mel_grad"]).sum() / (np.linalg.norm(mg) * np.linalg.norm(z["mel_grad"]))
    assert cos > 0.99, cos
    for k in z:
        if k.startswith("grad."):
            got, ref = eng.ps.view(k[5:], grad=True).cpu().numpy(), z[k]
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12)
            assert err < 0.15, (k, err)
    # EVERY gradient as a whole tensor: relative L2 distance to the reference's gradient, estimated from the seeded
    # random projections the fixture recorded (weights.grad_sketch; the estimator is good to +-25 %), and the norms.
    # bf16 storage on a random-init net costs ~8 % relative L2 (ReLU-mask flips; measured worst 16 %): bound 22 %.
    sk = grad_sketch(list(shapes), {k: eng.ps.view(k, grad=True).cpu().numpy() for k in shapes})
    worst = (0.0, "")
    for k in shapes:
        ref = z["gsketch." + k]
        if float(z["gnorm." + k]) == 0.0:
            continue
        rel = float(np.linalg.norm(sk[k] - ref) / np.linalg.norm(ref))
        worst = max(worst, (rel, k))
        assert rel < 0.22, (k, rel)
        gn = float(np.linalg.norm(eng.ps.view(k, grad=True).cpu().numpy().astype(np.float64)))
        assert abs(gn / float(z["gnorm." + k]) - 1) < 0.08, (k, gn, float(z["gnorm." + k]))
    print(f"{fixture}: worst whole-tensor relative L2 (sketch estimate) {worst}")


def test_vae_and_deep_configs_full_size():
    """BASELINE configs[3] (VAE bottleneck, jitter on, B=8, w=5000) and configs[4] per-GPU
    shape (30 layers x 512 residual channels, 64k-sample windows, B=4 per GPU): the step runs,
    is finite, and is reproducible."""
    from ae_wavenet_amd import config as C_
    rs = np.random.RandomState(0)
    for arch, B, w, kw in (("vae", 8, 5000, {}), ("deep", 4, 65536, {})):
        hps = C_.make_hps(arch, n_win_batch=w, **kw)
        eng = M.TrainEngine(hps, B=B, device=DEV, n_mel=39, update_codebook_every_step=False)
        gen = torch.Generator().manual_seed(1)
        for k in eng.ps.names():
            t = torch.empty(eng.ps.shape[k])
            if t.dim() >= 2:
                torch.nn.init.xavier_uniform_(t, generator=gen)
            else:
                t.zero_()
            eng.ps.view(k).copy_(t)
        g = eng.geom
        if arch == "deep":
            assert (g.enc_in_len, g.embed_len, g.dec_in_len) == (73520, 222, 68605)
            eng.emb.normal_(generator=None)
            eng.init_ema_from_emb()
        wav = torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(DEV)
        mel = torch.randn(B, 39, g.mel_len, generator=gen).to(DEV)
        voice = torch.randint(0, 40, (B,), generator=gen).to(DEV)
        j = np.arange(g.embed_len)[None, :] + rs.randint(-1, 2, size=(B, g.embed_len))      # jitter on
        jitter = torch.from_numpy(np.clip(j, 0, g.embed_len - 1)).to(DEV)
        eps = torch.randn(B, g.embed_len, hps.bn_n_out, generator=gen).to(DEV) if arch == "vae" else None
        if arch == "vae":
            eng.set_anneal_weight(0.3)
        eng.set_inputs(wav, mel, voice, jitter, eps=eps)
        l0 = float(eng.forward())
        eng.backward()
        g0 = eng.ps.grads[:eng.ps.numel].clone()
        assert np.isfinite(l0) and torch.isfinite(g0).all() and g0.abs().max() > 0
        eng.set_inputs(wav, mel, voice, jitter, eps=eps)
        if arch == "deep":
            eng.init_ema_from_emb()
        l1 = float(eng.forward())
        assert l1 == l0
        if arch == "vae":
            # the anneal weight lives in device memory: changing it takes effect in the already captured
            # graphs (chassis.py:148-149 changes it every step), loss = nll + a * max(KL, free_nats)
            kl = max(float(eng.loss_buf[2]), float(hps.bn_free_nats))
            eng.set_anneal_weight(0.6)
            l2 = float(eng.forward())
            assert abs((l2 - l0) - 0.3 * kl) <= 1e-4 * abs(l0) + 1e-3, (l0, l2, kl)
            eng.backward()
            g1 = eng.ps.grads[:eng.ps.numel].clone()
            assert torch.isfinite(g1).all() and not torch.equal(g1, g0)
        del eng
        torch.cuda.empty_cache()


def test_module_surface_trains():
    """Drop-in surface: run() -> loss.backward() -> FusedAdam.step() reduces the loss on a
    fixed batch; torch.optim.Adam on the same parameters gives the same first update."""
    from ae_wavenet_amd import autoencoder_model as ae, optim
    hps = config.make_hps("vqvae-ema", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64,
                          bn_n_out=16, bn_vq_n_embed=128, n_win_batch=256, n_blocks=2, n_block_layers=5)
    torch.manual_seed(0)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    opt = optim.FusedAdam(m, lr=1e-3)
    g = m.geom
    gen = torch.Generator().manual_seed(1)
    wav = torch.randint(0, 256, (4, g.enc_in_len), generator=gen).float().to(DEV)
    mel = torch.randn(4, 39, g.mel_len, generator=gen).to(DEV)
    voice = torch.randint(0, 40, (4,), generator=gen).to(DEV)
    jitter = torch.arange(g.embed_len).repeat(4, 1).to(DEV)
    losses = []
    for it in range(12):
        opt.zero_grad()
        pred, target, loss = m.run(wav, mel, voice, jitter)
        assert pred.shape == (4, 256, 255) and target.shape == (4, 255)
        loss.backward()
        if it == 0:
            n_with_grad = sum(1 for p in m.parameters() if p.grad is not None and p.grad.abs().sum() > 0)
            assert n_with_grad > 0.9 * len(list(m.parameters()))
        opt.step()
        losses.append(float(m.objective.metrics["rec"]))
    assert losses[-1] < losses[0] - 0.2, losses
    sd = m.state_dict()
    assert "decoder.conv_layers.3.conv_signal.weight" in sd and "bottleneck.emb" in sd


@pytest.mark.parametrize("width,steps,lr", [("reduced", 10, 1e-3), ("full", 3, 1e-4)])
def test_multi_step_trajectory_vs_oracle(width, steps, lr):
    """K steps of the harness loop - zero_grad -> run -> backward -> optimizer step -> update_codebook
    (chassis.py:151-176, vqema_bn.py:190-222) - through the module surface, against the fp32 oracle driven by
    torch.optim.Adam on the same initial state: the loss trajectory, the code indices (exact wherever the oracle's own
    top-2 margin exceeds what a bf16 decoder can move the encoder by), the EMA accumulators and the refreshed codebook.
    One-step tests cannot see an error in what a step hands to the next one (Adam moments, step count, EMA state,
    the codebook the NEXT forward quantises against, re-packed weights)."""
    from ae_wavenet_amd import autoencoder_model as ae, optim
    from oracle import ref_model as R
    if width == "reduced":
        hps = config.make_hps("vqvae-ema", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64,
                              bn_n_out=16, bn_vq_n_embed=128, n_win_batch=256, n_blocks=2, n_block_layers=5)
        B = 4
    else:
        hps = config.make_hps("vqvae-ema", n_win_batch=100)
        B = 2
    torch.manual_seed(21)
    m = ae.AutoEncoder(hps, n_mel=39, update_codebook_every_step=False)
    names = [n for n, _ in m.named_parameters()]
    sd = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    emb = m._buffers["bn_emb"].clone()
    numer, denom = m._buffers["bn_ema_numer"].clone(), m._buffers["bn_ema_denom"].clone()
    m = m.to(DEV)
    opt = optim.FusedAdam(m, lr=lr)
    adam = torch.optim.Adam([sd[n] for n in names], lr=lr)
    g = m.geom
    gen = torch.Generator().manual_seed(22)
    pool = [(torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float(), torch.randn(B, 39, g.mel_len, generator=gen),
             torch.randint(0, 40, (B,), generator=gen), torch.arange(g.embed_len).repeat(B, 1)) for _ in range(2)]
    K, gamma = hps.bn_vq_n_embed, hps.bn_vq_ema_gamma
    worst_loss, n_mismatch, n_checked, n_total = 0.0, 0, 0, 0
    for it in range(steps):
        wav, mel, voice, jitter = pool[it % 2]                      # two alternating batches
        # ---- MI355X
        opt.zero_grad()
        pred, target, loss = m.run(wav.to(DEV), mel.to(DEV), voice.to(DEV), jitter.to(DEV))
        loss.backward()
        opt.step()
        m.bottleneck.update_codebook()
        eng = m._engine
        torch.cuda.synchronize()
        # ---- oracle
        adam.zero_grad()
        out = R.ae_run(sd, {"emb": emb}, hps, g, wav, mel, voice, jitter, loss_mode="intended", take_compat=False)
        out["loss"].backward()
        z_sum, n_sum = R.vqema_stats(out["ze"], out["min_ind"], K)
        numer, denom = R.vqema_ema(numer, denom, z_sum, n_sum, gamma)
        adam.step()
        emb_prev, emb = emb, R.vqema_codebook(numer, denom)
        # ---- compare
        rel = abs(float(loss.detach()) / float(out["loss"].detach()) - 1)
        worst_loss = max(worst_loss, rel)
        got_ind = eng.ind[:eng.Q].cpu().numpy()
        ref_ind = out["min_ind"].reshape(-1).numpy()
        # the oracle's own margin between its best and second-best code (relative to the best distance)
        d2 = R.scaled_l2(out["ze"].detach(), emb_prev).permute(0, 2, 1).reshape(-1, K)       # (queries, codes)
        top2 = torch.topk(d2, 2, dim=1, largest=False).values
        # ... against how far the device's encoder outputs moved every distance of that query: a gap of more than twice
        # that cannot close.  (Step 0: identical weights - the exact fp32 chain against torch's summation order.  Later
        # steps: the encoder weights have taken Adam steps from gradients that came through the bf16 decoder.)
        ze_dev = eng.lin.tensor()[:, :, :hps.bn_n_out].cpu().permute(0, 2, 1)
        ze_err = float((ze_dev - out["ze"].detach()).abs().max()) / float(out["ze"].detach().abs().max())
        assert ze_err < (1e-5 if it == 0 else 0.25), (it, ze_err)
        moved = (R.scaled_l2(ze_dev, emb_prev).permute(0, 2, 1).reshape(-1, K) - d2).abs().max(dim=1).values
        clear = ((top2[:, 1] - top2[:, 0]) > 2 * moved + 1e-5 * top2[:, 0]).numpy()
        n_total += len(ref_ind)
        n_checked += int(clear.sum())
        bad = int((got_ind[clear] != ref_ind[clear]).sum())
        n_mismatch += int((got_ind != ref_ind).sum())
        print(f"step {it}: ze rel err {ze_err:.1e}; loss {float(loss.detach()):.4f} oracle {float(out['loss'].detach()):.4f} rel {rel:.2e}; indices: {bad} of "
              f"{int(clear.sum())} clear-margin differ, {int((got_ind != ref_ind).sum())} of {len(ref_ind)} overall")
        assert rel < 1e-3, (it, float(loss.detach()), float(out["loss"].detach()))     # (measured <= 3.5e-4 over the 13 steps)
        assert bad == 0, (it, bad)
        # EMA accumulators and refreshed codebook, on every code that both sides assigned identically (a query that
        # sits on a near-tie may go either way; the two codes it chose between are left out): they differ only by what the
        # slightly different encoder outputs add
        keep = torch.ones(K, dtype=torch.bool)
        mism = got_ind != ref_ind
        keep[torch.from_numpy(np.concatenate([got_ind[mism], ref_ind[mism]]).astype(np.int64))] = False
        for nm, a, b in (("ema_numer", eng.ema_numer, numer), ("ema_denom", eng.ema_denom, denom), ("emb", eng.emb, emb)):
            a = a.cpu()
            e = float((a[keep] - b[keep]).abs().max()) / max(float(b.abs().max()), 1e-12)
            # step 0: identical weights on both sides - fp32 round-off.  Later: Adam's normalised update moves every
            # weight by ~lr per step whatever the size of its gradient, in the direction of the gradient's SIGN - which
            # bf16 noise decides for the smallest gradients - so the encoder outputs (and what they add to the
            # accumulators, (1 - gamma) z_sum against rows of magnitude (1 - gamma) |emb|) agree to a few per cent
            assert e < (2e-6 if it == 0 else 6e-2), (it, nm, e)
        assert float((eng.ema_denom.cpu()[keep] - denom[keep]).abs().max()) < 1e-6
        # the quantiser is discrete: after ONE near-tie went the other way the two codebooks differ for good and every
        # later comparison would only measure that.  The oracle therefore continues from the device's EMA state (weights
        # and Adam moments stay free-running on both sides): each step checks one transition from a common codebook.
        numer, denom, emb = eng.ema_numer.cpu().clone(), eng.ema_denom.cpu().clone(), eng.emb.cpu().clone()
    # parameters after the last step: Adam's normalised update moves a parameter by ~lr per step whatever the size of
    # its gradient, so the drift is bounded by steps * lr per element; most elements agree far better
    drift = []
    for n in names:
        a, b = dict(m.named_parameters())[n].detach().cpu(), sd[n].detach()
        assert float((a - b).abs().max()) <= 2.05 * steps * lr, n
        drift.append(float((a - b).norm()) / max(float((b - 0).norm()), 1e-12))
    print(f"worst loss deviation {worst_loss:.2e}; index mismatches {n_mismatch} / {n_total} ({n_checked} with a clear margin); "
          f"relative L2 drift of the parameters: median {sorted(drift)[len(drift) // 2]:.2e}, worst {max(drift):.2e}")
    assert sorted(drift)[len(drift) // 2] < 5e-2
    assert n_mismatch <= max(2, n_total // 8) and n_checked >= n_total // 2


# ----------------------------------------------------------------------------------------------
# size-independent properties at BASELINE.json's full size (B=8, w=5000)
# ----------------------------------------------------------------------------------------------
def test_full_size_properties():
    hps, eng, wts, emb, inp = seeded_full_engine(B=8, w=5000, seed=7)
    wav, mel, voice, jitter = [t.to(DEV) for t in inp]
    eng.set_inputs(wav, mel, voice, jitter)
    l0 = float(eng.forward())
    eng.backward()
    torch.cuda.synchronize()
    lg0 = eng.logits().clone()
    ind0 = eng.ind[:eng.Q].clone()
    g0 = eng.ps.grads[:eng.ps.numel].clone()
    assert np.isfinite(l0) and torch.isfinite(g0).all()
    # (1) determinism of the integer path and of the forward
    eng.init_ema_from_emb()
    l1 = float(eng.forward())
    assert torch.equal(eng.ind[:eng.Q], ind0) and l1 == l0 and torch.equal(eng.logits(), lg0)
    # (2) batch-permutation equivariance: permuting the windows permutes logits/indices and
    #     leaves the (sum-type) loss and the gradients unchanged up to summation order
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device=DEV)
    eng.init_ema_from_emb()
    eng.set_inputs(wav[perm], mel[perm], voice[perm], jitter[perm])
    l2 = float(eng.forward())
    eng.backward()
    torch.cuda.synchronize()
    Ne = eng.geom.embed_len
    assert torch.equal(eng.ind[:eng.Q].view(8, Ne), ind0.view(8, Ne)[perm])
    assert torch.equal(eng.logits(), lg0[perm])
    assert abs(l2 / l0 - 1) < 1e-5
    g2 = eng.ps.grads[:eng.ps.numel]
    rel = (g2 - g0).abs().max().item() / g0.abs().max().item()
    assert rel < 2e-3, rel
    # (3) causality of the valid-conv stack: the target-independent logits do not change when
    #     the wav samples after the last decoder input are altered
    wav2 = wav.clone()
    wav2[:, eng.geom.trim_dec_in[1]:] = 0
    eng.init_ema_from_emb()
    eng.set_inputs(wav2, mel, voice, jitter)
    eng.forward()
    assert torch.equal(eng.logits(), lg0)


def test_half_batch_chains_and_tail_branch_are_bit_identical_to_the_serial_plan(monkeypatch):
    """DecoderPlan.split_chains / split_chains_bwd (the gated stack and its dgrad chain as two half-batch chains on lanes
    4 / 5) and tail_lane (the last grouped weight-gradient launch as a branch) only re-schedule: captured as graph branches
    (TrainEngine.graph_lanes) or run serially they must give the one-chain engine's loss and gradients, replay after
    replay - a missing dependency shows as a mismatch."""
    from ae_wavenet_amd import engine as E
    for k in ("split_chains", "split_chains_bwd", "tail_lane"):
        monkeypatch.setattr(E.DecoderPlan, k, 0)
    hps, eng0, wts, emb, inp = seeded_full_engine(B=8, w=5000, seed=11)
    wav, mel, voice, jitter = [t.to(DEV) for t in inp]

    def step(eng):
        eng.init_ema_from_emb()
        loss = float(eng.forward())
        eng.backward()
        torch.cuda.synchronize()
        return loss, eng.ps.grads[:eng.ps.numel].clone()

    eng0.set_inputs(wav, mel, voice, jitter)
    assert not any(op.lane >= 4 for op in eng0.bwd.ops + eng0.fwd_b.ops)
    l_ref, g_ref = step(eng0)
    atomic = [n for n in eng0.ps.names() if n.endswith(".bias") or "speaker_embedding" in n]
    mask = torch.ones(eng0.ps.numel, dtype=torch.bool, device=DEV)
    for n in atomic:                                   # fp32-atomic column sums: round-off, as in the lane test below
        o = (eng0.ps.view(n, True).data_ptr() - eng0.ps.grads.data_ptr()) // 4
        mask[o:o + eng0.ps.numel_of(n)] = False
    del eng0
    torch.cuda.empty_cache()
    for cfg in (dict(split_chains=1, split_chains_bwd=1), dict(tail_lane=4)):
        for k in ("split_chains", "split_chains_bwd", "tail_lane"):
            monkeypatch.setattr(E.DecoderPlan, k, cfg.get(k, 0))
        _, eng, _, _, _ = seeded_full_engine(B=8, w=5000, seed=11)
        eng.set_inputs(wav, mel, voice, jitter)
        assert any(op.lane >= 4 for op in eng.bwd.ops)
        assert eng.graph_lanes == 2 and eng.use_graphs
        for rep in range(4):
            l, g = step(eng)
            assert l == l_ref, (cfg, rep, l, l_ref)
            assert torch.equal(g[mask], g_ref[mask]), (cfg, rep)
            d = (g[~mask] - g_ref[~mask]).abs().max().item()
            assert d <= 2e-6 * g_ref[~mask].abs().max().item(), (cfg, rep, d)
        eng.use_graphs = False                         # eager: serial plan order (lanes stay off outside a capture)
        l, g = step(eng)
        assert l == l_ref and torch.equal(g[mask], g_ref[mask]), cfg
        del eng
        torch.cuda.empty_cache()


def test_two_lane_schedule_is_bit_identical_to_serial():
    """The side-lane assignment (wgrads / column sums off the dgrad chain, aew_op_t.lane) must not
    change any result: serial plan order is the reference schedule.  Replayed several times in graph
    and eager form so a missing dependency shows as a mismatch."""
    hps, eng, wts, emb, inp = seeded_full_engine(B=8, w=5000, seed=11)
    wav, mel, voice, jitter = [t.to(DEV) for t in inp]
    eng.set_inputs(wav, mel, voice, jitter)
    lib = L.load()

    def step():
        eng.init_ema_from_emb()
        loss = float(eng.forward())
        eng.backward()
        torch.cuda.synchronize()
        return loss, eng.ps.grads[:eng.ps.numel].clone()

    def recapture():
        for pl in (eng.fwd_a, eng.fwd_b, eng.bwd):
            pl.invalidate_graph()

    assert any(op.lane == 1 for op in eng.bwd.ops) and any(op.join for op in eng.bwd.ops)
    # bias-type gradients are column sums accumulated with fp32 atomics (k_colsum, k_spk_bwd): their
    # summation order is not fixed even serially, so they are compared at round-off; everything that
    # comes out of the GEMM / slab-reduction path must match bit for bit
    atomic = [n for n in eng.ps.names() if n.endswith(".bias") or "speaker_embedding" in n]
    mask = torch.ones(eng.ps.numel, dtype=torch.bool, device=DEV)
    for n in atomic:
        o = (eng.ps.view(n, True).data_ptr() - eng.ps.grads.data_ptr()) // 4
        mask[o:o + eng.ps.numel_of(n)] = False

    def same(l, g, l_ref, g_ref):
        assert l == l_ref
        assert torch.equal(g[mask], g_ref[mask])
        d = (g[~mask] - g_ref[~mask]).abs().max().item()
        assert d <= 2e-6 * g_ref[~mask].abs().max().item(), d

    try:
        lib.aew_set_lanes(0)
        recapture()
        l_ref, g_ref = step()
        lib.aew_set_lanes(1)
        recapture()
        for _ in range(4):
            same(*step(), l_ref, g_ref)
        # the split form used by the overlapped all-reduce (decoder part | hook | encoder part)
        calls = []

        def step_split():
            eng.init_ema_from_emb()
            loss = float(eng.forward())
            eng.backward(after_decoder=lambda: calls.append(1))
            torch.cuda.synchronize()
            return loss, eng.ps.grads[:eng.ps.numel].clone()

        same(*step_split(), l_ref, g_ref)
        assert calls == [1]
        eng.use_graphs = False                      # eager: two real streams + events
        for _ in range(2):
            same(*step(), l_ref, g_ref)
    finally:
        eng.use_graphs = True
        lib.aew_set_lanes(0)                        # the library's default
