"""Every TN (weight-gradient) kernel body against the bits of the commit BEFORE the by-product and store helpers the bodies
share were factored out: SHA-256 of every raw output buffer - the split-K slabs unsummed, the
grouped results, the running snapshots and the column sums - equals tests/data/tn_bits_parent.json, which
tests/data/tn_bits_gen.py wrote on an MI355X at that commit with the build functions below.  Each launch writes every
output element from one block in one fixed order, so equal hashes are the expected result, not a tolerance."""
import hashlib
import json
import os

import pytest
import torch

from ae_wavenet_amd import _lib as L, plan as PL
from ae_wavenet_amd.plan import Mat, Plan, TnGroupBuilder, Workspace, make_tn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F3 = L.BF16, L.F32
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "tn_bits_parent.json")


def _inputs(names, seed):
    """CPU workspace with the named (name, numel, dtype) buffers filled uniformly in [-1, 1)."""
    gen = torch.Generator().manual_seed(seed)
    ws = Workspace("cpu")
    for n, sz, dt in names:
        ws.alloc(n, sz, dt)
        t = ws.get(n)
        t.copy_(((torch.rand(t.shape, generator=gen) * 2 - 1)).to(t.dtype))
    return ws


def _mirror(ws_cpu):
    ws = Workspace(DEV)
    for n, t in ws_cpu.bufs.items():
        ws.bufs[n] = t.to(DEV)
    return ws


def _run(p, kernel):
    """Run plan p, whose last op is the TN launch; where the library exports its pick (the commit the table was recorded at does
    not), the launch is on `kernel`: a switch that failed to engage would otherwise pass on another body's equal bits."""
    lib, op, pick = L.load(), p.ops[-1], L.TnPick() if hasattr(L, "TnPick") else None
    if pick is not None:
        fn, desc = (lib.aew_tn_group_pick, op.u.tng) if op.kind == L.OP_GEMM_TN_GROUP else (lib.aew_tn_pick, op.u.tn)
        assert fn(L.C.byref(desc), L.C.byref(pick)) == 0 and pick.name.decode() == kernel, (pick.name, kernel)
    p.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def group_case(tile, mfma32=False, cursor=None):
    """The group of test_gemm_tn_group (B = 3; Mc 690 / 650 / 33; at tile 128 the split descriptor too)."""
    B = 3
    ws_c = _inputs((("G1", B * 700 * 256, torch.bfloat16), ("A1", B * 740 * 384, torch.bfloat16), ("A2", B * 760 * 128, torch.bfloat16),
                    ("G2", B * 650 * 384, torch.bfloat16), ("Z", B * 650 * 256, torch.bfloat16)), 5)
    ws_c.get("A1").view(-1)[:B * 740 * 384].view(B * 740, 384)[:, 368] = 1.0        # the ones channel
    ins = dict(ws_c.bufs)
    outs = [("o1", 256 * 896), ("o2", 384 * 256), ("o3", 256 * 256), ("snap", B * 256), ("snap2", B * 384), ("cs1", 256), ("cs2", 384)]
    if tile == 128:
        outs.append(("o4", 9 * 128 * 512))               # 3 batch elements x 3 chunks of 224 rows
    for n, sz in outs:
        ws_c.alloc(n, sz, torch.float32)
        ws_c.get(n).fill_(-7.0)                          # (elements no block writes keep the fill)
    ws = _mirror(ws_c)
    G1, A1, A2 = Mat(ws, "G1", B, 700, 256, BF), Mat(ws, "A1", B, 740, 384, BF), Mat(ws, "A2", B, 760, 128, BF)
    G2, Z = Mat(ws, "G2", B, 650, 384, BF), Mat(ws, "Z", B, 650, 256, BF)
    gb = TnGroupBuilder(ws, "tng", tile)
    gb.cursor = cursor is not None
    t = make_tn(BF, 690, B, 256, 256, G1.seg(256), [A1.seg(384), A1.seg(384, row_off=9), A2.seg(128, row_off=31)])
    t.out, t.out_batch_stride = ws.get("o1").data_ptr(), 256 * 896
    t.snap_out, t.snap_bs, t.snap_k = ws.get("snap").data_ptr(), 256, 368
    t.colsum_out = ws.get("cs1").data_ptr()
    gb.add(t, "d0")
    t = make_tn(BF, 650, B, 368, 384, G2.seg(384, hi=640), [Z.seg(256)])
    t.out, t.out_batch_stride = ws.get("o2").data_ptr(), 384 * 256
    t.colsum_out = ws.get("cs2").data_ptr()
    t.snap_out, t.snap_bs, t.snap_k = ws.get("snap2").data_ptr(), 384, -1
    gb.add(t, "d1")
    t = make_tn(BF, 33, B, 256, 256, G1.seg(256, row_off=5), [Z.seg(256, row_off=-2)])
    t.out, t.out_batch_stride = ws.get("o3").data_ptr(), 256 * 256
    gb.add(t, "d2")
    if tile == 128:
        t = make_tn(BF, 650, B, 128, 128, G2.seg(128, row_off=3), [Z.seg(256, row_off=1), Z.seg(256)])
        t.out, t.out_batch_stride = ws.get("o4").data_ptr(), 128 * 512
        assert gb.set_split(t, 220) == 9
        gb.add(t, "d3")
    p = Plan("g")
    gb.emit(p, "group")
    lib = L.load()
    keep, rec = L.current_tuning(), L.current_tuning(tn_mfma32=int(mfma32))
    try:
        assert lib.aew_tuning_set(L.C.byref(rec)) == 0 and (cursor is None or lib.aew_set_tn_cursor(*cursor) == 0)
        _run(p, {256: "k_gemm_tn_bf16_big_grp", 384: "k_gemm_tn_bf16_grp8"}.get(
            tile, "k_gemm_tn_bf16_grp_cur" if cursor else "k_gemm_tn_bf16_grp32" if mfma32 else "k_gemm_tn_bf16_grp"))
    finally:
        lib.aew_tuning_set(L.C.byref(keep))
    return ins, {n: ws.get(n)[:sz] for n, sz in outs}


def alone_case(dtype, Mc, safe):
    """The stand-alone op of test_gemm_tn: Mc = 777 folds the batch into one slab, Mc = 5000 is split-K slabs."""
    tdt = PL.TORCH_DT[dtype]
    B, Np, K1, K2 = 2, 256, 128, 256
    R0 = Mc + 43
    ws_c = _inputs((("G", B * R0 * Np, tdt), ("A1", B * R0 * 256, tdt), ("A2", B * R0 * 256, tdt)), 2)
    ws = _mirror(ws_c)
    Gm, A1, A2 = Mat(ws, "G", B, R0, Np, dtype), Mat(ws, "A1", B, R0, 256, dtype), Mat(ws, "A2", B, R0, 256, dtype)
    t = make_tn(dtype, Mc, B, Np, Np, Gm.seg(Np, row_off=3, hi=Mc - 77),
                [A1.seg(K1, row_off=11), A1.seg(K1, row_off=-4, col_off=128), A2.seg(K2, row_step=1, row_off=0)])
    return ws_c.bufs, _slabs(ws, t, dict(tn_safe=safe), "k_gemm_tn_f32" if dtype == F3 else f"k_gemm_tn_bf16<{safe}>")


def big_case(Np, ks):
    """test_gemm_tn_big_tiles with tn_big = 1: halves of 128 columns, tiles that straddle two segments."""
    B, Mc = 3, 2500
    R0 = Mc + 43
    ws_c = _inputs((("G", B * R0 * Np, torch.bfloat16), ("A1", B * R0 * 384, torch.bfloat16), ("A2", B * R0 * 384, torch.bfloat16)), 5)
    ws = _mirror(ws_c)
    Gm, A1, A2 = Mat(ws, "G", B, R0, Np, BF), Mat(ws, "A1", B, R0, 384, BF), Mat(ws, "A2", B, R0, 384, BF)
    segs = [(A1 if i % 2 == 0 else A2).seg(k, row_off=(0, 16, -4)[i % 3], hi=R0 - 5 if i == 1 else None) for i, k in enumerate(ks)]
    t = make_tn(BF, Mc, B, Np - 8, Np, Gm.seg(Np, row_off=3, hi=Mc - 77), segs)
    return ws_c.bufs, _slabs(ws, t, dict(tn_big=1), "k_gemm_tn_bf16_big")


def _slabs(ws, t, over, kernel):
    """Run the stand-alone op t under the process-wide record with `over`, on `kernel`; its slabs, unsummed."""
    lib = L.load()
    keep, rec = L.current_tuning(), L.current_tuning(**over)
    assert lib.aew_tuning_set(L.C.byref(rec)) == 0
    try:
        slabs = L.tn_slabs(t)
        n = slabs * t.N_pad * t.K_total
        out = ws.alloc("out", n, torch.float32)
        out.fill_(-7.0)
        t.out, t.out_batch_stride = out.data_ptr(), t.N_pad * t.K_total
        p = Plan("tn")
        p.add(L.OP_GEMM_TN, t, "tn")
        _run(p, kernel)
    finally:
        lib.aew_tuning_set(L.C.byref(keep))
    return {"slabs": ws.get("out")[:n]}


CASES = {
    "group128": lambda: group_case(128),
    "group128_mfma32": lambda: group_case(128, mfma32=True),
    "group128_cursor": lambda: group_case(128, cursor=(4, 2)),
    "group256": lambda: group_case(256),
    "group384": lambda: group_case(384),
    "bf16_fold": lambda: alone_case(BF, 777, 0),
    "bf16_fold_safe": lambda: alone_case(BF, 777, 1),
    "bf16_split": lambda: alone_case(BF, 5000, 0),
    "bf16_split_safe": lambda: alone_case(BF, 5000, 1),
    "f32_split": lambda: alone_case(F3, 5000, 0),
    "big384": lambda: big_case(384, (128, 256)),
    "big640": lambda: big_case(640, (384, 384, 128)),
}


def digests(bufs):
    """{name: SHA-256 of the buffer's bytes}"""
    return {n: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for n, t in bufs.items()}


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_holds_every_case(table):
    assert sorted(table) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_tn_bits_equal_the_parent(table, name):
    ins, outs = CASES[name]()
    want = table[name]
    assert digests(ins) == want["in"], "the inputs differ from the recorded ones: re-record at the parent"
    got = digests(outs)
    assert sorted(got) == sorted(want["out"])
    assert got == want["out"], [n for n in got if got[n] != want["out"][n]]
