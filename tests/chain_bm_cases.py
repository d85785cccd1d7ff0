"""Stage descriptors for the tests of the chained launch on 128-row tiles (test_chain_bm_cpu.py, test_chain_bm_gpu.py):
the backward of the gated stack in miniature - dz (DFG: the residual 1x1's input gradient times the saved gate
derivatives) and dx (STORE: both taps of the dilated pair, plus the gradient that arrives through the residual path) -
built exactly as DecoderPlan._bwd_stack builds them, at M = 300 rows (three 128-row tiles, the last one ragged; two
256-row tiles).  Rows outside [0, M) are masked by the descriptors' row limits, as in the engine."""
import ctypes as C

import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Mat, Plan, Workspace, insert_nt_chains, make_nt, null_view

B, M, SP = 2, 300, 64
BF = L.BF16


class Case:
    """ws, plan (the stage ops, one launch each), outs (names of the buffers the stages write)."""

    def __init__(self, device):
        self.ws = Workspace(device)
        self.plan = Plan("chain_bm")
        self.outs = []
        self.n = 0

    def mat(self, name, rows, pitch, batch=B, fill=True, scale=1.0):
        m = Mat.new(self.ws, name, batch, rows, pitch, BF)
        if fill and self.ws.device.type != "cpu":
            g = torch.Generator().manual_seed(1000 + len(self.ws.bufs))
            t = self.ws.get(name)
            t.copy_((torch.randn(t.numel(), generator=g) * scale).to(torch.bfloat16))
        return m

    def weight(self, n_pad, k):
        self.n += 1
        return self.mat(f"w{self.n}", n_pad, k, batch=1, scale=k ** -0.5)

    def dz(self, tag, dp, n, x, rp, dskp):
        """dfg = (x | dskp) W^T * (pf | pg): N_pad = dp, n <= dp real channels"""
        pf, pg = self.mat(f"pf.{tag}", M, dp), self.mat(f"pg.{tag}", M, dp)
        dfg = self.mat(f"dfg.{tag}", M, 2 * dp, fill=False)
        W = self.weight(dp, rp + SP)
        g = make_nt(BF, M, n, dp, B, [x.seg(rp, hi=M), dskp.seg(SP)], W.ptr, epi=L.EPI_DFG, aux0=pf.view(), aux1=pg.view(),
                    out0=dfg.view())
        self.plan.add(L.OP_GEMM_NT, g, f"dz.{tag}")
        self.outs.append(dfg.name)
        return dfg

    def dx(self, tag, dfg, dp, rp, d, add=None):
        """dx = dfg[t] Wf^T + dfg[t - d] Wg^T (+ add[t - d]): the two taps of wavenet.py:100, N_pad = rp"""
        dx = self.mat(f"dx.{tag}", M, rp, fill=False)
        W = self.weight(rp, 4 * dp)
        g = make_nt(BF, M, rp, rp, B, [dfg.seg(2 * dp), dfg.seg(2 * dp, row_off=-d)], W.ptr,
                    flags=L.EF_ADD_AUX0 if add is not None else 0, out0=dx.view(hi=M),
                    aux0=add.view(row_off=-d, hi=M) if add is not None else null_view())
        self.plan.add(L.OP_GEMM_NT, g, f"dx.{tag}")
        self.outs.append(dx.name)
        return dx


def pair(device, dp, rp, d, n=None):
    """dz -> dx: dx waits for the dz row tiles that hold rows [m0 - d, m_last]"""
    c = Case(device)
    dxn, dskp = c.mat("dx.above", M, rp), c.mat("dskp", M, SP)
    dfg = c.dz("l", dp, n or dp, dxn, rp, dskp)
    c.dx("l", dfg, dp, rp, d, add=dxn)
    return c


def triple(device, dp, rp, d, n=None):
    """dx.a -> dz -> dx: dz reads dx.a through its K loop, dx reads dfg through both taps and dx.a through its epilogue"""
    c = Case(device)
    dfg_a, dskp = c.mat("dfg.above", M, 2 * dp), c.mat("dskp", M, SP)
    dxa = c.dx("a", dfg_a, dp, rp, d)
    dfg = c.dz("l", dp, n or dp, dxa, rp, dskp)
    c.dx("l", dfg, dp, rp, d, add=dxa)
    return c


def chained(case, bm, name="chain.t"):
    """A copy of the case's plan with its stages as ONE chained launch on row tiles of `bm` (a number or one per stage)."""
    sub = Plan("chained")
    sub.ops, sub.labels = list(case.plan.ops), list(case.plan.labels)
    hs = dict(zip(sub.labels, bm)) if isinstance(bm, (tuple, list)) else None
    made = insert_nt_chains(sub, case.ws, name, lambda lab: True, force=True, bm=(lambda lab: hs[lab]) if hs else bm)
    assert made == [(1, len(case.plan.ops))], made
    return sub


def build_table(descs, bms, force=1):
    """aew_nt_chain_build_bm on host descriptors: (rc, stages, blocks, counters, set)"""
    n = len(descs)
    arr = (L.GemmNT * n)(*descs)
    st = (L.NtStage * n)()
    bmap = (C.c_uint16 * 4096)()
    nb, nc, se = C.c_int(0), C.c_int(0), C.c_int(0)
    hs = (C.c_int32 * n)(*bms) if bms is not None else None
    rc = L.load().aew_nt_chain_build_bm(C.byref(arr), n, C.byref(st), C.byref(bmap), 8 * 4096, C.byref(nb), C.byref(nc),
                                        C.byref(se), force, None, C.byref(hs) if hs is not None else None)
    return rc, st, nb.value, nc.value, se.value, bmap
