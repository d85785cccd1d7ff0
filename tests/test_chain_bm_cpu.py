"""The chained launch on 128-row tiles, HOST side (aew_nt_chain_build_bm, aew_nt_chain_dep_tiles) - no GPU.

M = 300: three 128-row tiles, the last one of 44 rows.  Dilations 1 and 4 (one-window body for d <= 16), 32 (one-window
body for d <= 64), 128 and 512 (plain body; 512 is longer than the matrix, so the shifted tap reads nothing).  For every
tile of every stage the producer row tiles a dependency record names are compared with the row intervals re-derived from
the plain segment / view records, tile by tile and row by row; then the launch is replayed under random schedules that
honour only the table's waits and in-order dispatch (what pruning an implied dependency must not break)."""
import ctypes as C
import random

import numpy as np
import pytest

from ae_wavenet_amd import _lib as L
from tests import chain_bm_cases as CS

DILS = [1, 4, 32, 128, 512]
KIND_128 = 4


def _bm(s):
    return 128 if s.kind & KIND_128 else 256


def _inputs(g):
    rec = lambda v: (v.ptr or 0, v.row_step, v.row_off, v.row_lo, v.row_hi)
    ins = [rec(g.seg[i]) for i in range(g.n_segs)]
    if g.epi == L.EPI_DFG or (g.epi == L.EPI_STORE and g.flags & L.EF_ADD_AUX0):
        ins.append(rec(g.aux0))
    if g.epi == L.EPI_DFG or (g.epi == L.EPI_STORE and g.flags & (L.EF_MUL_POS1 | L.EF_OUT1_POS1)):
        ins.append(rec(g.aux1))
    return [r for r in ins if r[0]]


def _rows_read(ref, m0, m1):
    """buffer rows that GEMM rows m0..m1 read through `ref`, one by one"""
    ptr, step, off, lo, hi = ref
    return {m * step + off for m in range(m0, m1 + 1) if lo <= m * step + off < hi}


def _dep_tiles(s, d, m0):
    lo, hi = C.c_int(0), C.c_int(0)
    L.check(L.load().aew_nt_chain_dep_tiles(C.byref(s), d, m0, C.byref(lo), C.byref(hi)), "dep_tiles")
    return set(range(lo.value, hi.value + 1))


def _check_records(stages):
    """every dependency record, per consumer tile: the producer tiles it names = the tiles that hold the rows read"""
    n_checked = 0
    for si, s in enumerate(stages):
        bm = _bm(s)
        for d in range(s.n_deps):
            dep = s.dep[d]
            p = next(q for q in range(si) if stages[q].cnt_base == dep.cnt_base)
            P = stages[p]
            assert dep.bm == _bm(P) and dep.n_mt == P.n_mt == -(-P.g.M // dep.bm) and dep.need == P.n_nt and P.publish
            o = P.g.out0
            for mt in range(s.n_mt):
                m0, m1 = mt * bm, min(mt * bm + bm, s.g.M) - 1
                want = set()
                for ref in _inputs(s.g):
                    if ref[0] != o.ptr:
                        continue
                    for r in _rows_read(ref, m0, m1):
                        if o.row_lo <= r < o.row_hi and 0 <= r - o.row_off < P.g.M:     # a row the producer writes
                            want.add((r - o.row_off) // dep.bm)
                got = _dep_tiles(s, d, m0)
                assert want <= got, (si, d, mt, want, got)
                assert (min(got), max(got)) == (min(want), max(want)) if want else not got, (si, d, mt, want, got)
                n_checked += 1
    return n_checked


def _simulate(stages, seed, slots):
    """Workgroups are dispatched in index order into `slots` resident slots; a resident tile whose waits are satisfied
    may run at any later time.  Every row a tile reads from a buffer the run writes must be complete."""
    rng = random.Random(seed)
    written = {s.g.out0.ptr: np.zeros(s.g.out0.row_hi + 1, dtype=bool) for s in stages}
    done = [np.zeros(s.n_mt, dtype=np.int32) for s in stages]
    order = [(si, mt, nt) for si, s in enumerate(stages) for mt in range(s.n_mt) for nt in range(s.n_nt)]
    nxt, resident = 0, []
    while nxt < len(order) or resident:
        while nxt < len(order) and len(resident) < slots:
            resident.append(order[nxt])
            nxt += 1
        ready = []
        for si, mt, nt in resident:
            s = stages[si]
            ok = True
            for d in range(s.n_deps):
                p = next(q for q in range(si) if stages[q].cnt_base == s.dep[d].cnt_base)
                ok = ok and all(done[p][u] >= s.dep[d].need for u in _dep_tiles(s, d, mt * _bm(s)))
            if ok:
                ready.append((si, mt, nt))
        assert ready, "deadlock: a wait names a tile that is dispatched later"
        t = rng.choice(ready) if rng.random() < 0.7 else ready[-1]
        resident.remove(t)
        si, mt, nt = t
        s = stages[si]
        bm = _bm(s)
        m0, m1 = mt * bm, min(mt * bm + bm, s.g.M) - 1
        for ref in _inputs(s.g):
            if ref[0] in written:
                rows = sorted(_rows_read(ref, m0, m1))
                assert all(written[ref[0]][r] for r in rows), f"stage {si} tile {mt} reads rows that are not complete"
        done[si][mt] += 1
        if done[si][mt] == s.n_nt:
            o = s.g.out0
            for m in range(m0, m1 + 1):
                r = m * o.row_step + o.row_off
                if o.row_lo <= r < o.row_hi:
                    written[o.ptr][r] = True


@pytest.mark.parametrize("d", DILS)
@pytest.mark.parametrize("bms", [(128, 128, 128), (128, 256, 128), (256, 128, 256)])
def test_dependencies_at_128_rows_against_row_intervals(d, bms):
    case = CS.triple("cpu", 128, 256, d)
    descs = [op.u.nt for op in case.plan.ops]
    rc, st, nb, nc, se, bmap = CS.build_table(descs, bms)
    assert rc == 0 and se == 1
    body = 0 if d > 64 else (1 if d <= 16 else 2)
    for s, h, want_kind in zip(st, bms, (body, 0, body)):                     # dx.a, dz, dx
        assert s.kind == want_kind + (KIND_128 if h == 128 else 0)
        assert s.n_mt == -(-CS.M // h) and s.n_nt == s.g.N_pad // 128
        assert s.n_blocks == -(-s.n_mt * CS.B // 8) * 8 * s.n_nt and s.first_block % 8 == 0
    assert all(b.first_block == a.first_block + a.n_blocks and b.cnt_base == a.cnt_base + a.n_mt * CS.B for a, b in zip(st, st[1:]))
    assert nb == sum(s.n_blocks for s in st) and nc == sum(s.n_mt * CS.B for s in st)
    for s_i, s in enumerate(st):                                              # the block map: stage of every group of 8
        assert all(bmap[i8] == s_i for i8 in range(s.first_block // 8, (s.first_block + s.n_blocks) // 8))
    # dz waits for dx.a row for row; dx for dfg rows [m0 - d, m_last]; its epilogue's read of dx.a is implied by dz's wait
    assert st[0].n_deps == 0 and st[1].n_deps == 1 and (st[1].dep[0].d_lo, st[1].dep[0].d_hi) == (0, 0)
    # (d = 512: no row m - d of the shifted tap exists, so that segment contributes nothing to the record)
    assert st[2].n_deps == 1 and (st[2].dep[0].d_lo, st[2].dep[0].d_hi) == (-d if d < CS.M else 0, 0)
    assert st[2].dep[0].cnt_base == st[1].cnt_base
    assert _check_records(st) == st[1].n_mt + st[2].n_mt
    for seed in range(3):
        _simulate(st, seed, slots=5)


@pytest.mark.parametrize("d", DILS)
def test_pair_at_128_rows(d):
    case = CS.pair("cpu", 256, 384, d, n=248)
    rc, st, nb, nc, se, _ = CS.build_table([op.u.nt for op in case.plan.ops], (128, 128))
    assert rc == 0 and se == 1 and [s.n_mt for s in st] == [3, 3]
    assert _check_records(st) == 3
    # the tiles the ragged last tile (rows 256..299) of dx waits for: rows [256 - d, 299] of dfg (d = 512: no shifted row exists)
    assert _dep_tiles(st[1], 0, 256) == set(range(max(256 - (d if d < CS.M else 0), 0) // 128, 3))
    for seed in range(3):
        _simulate(st, seed, slots=4)


def test_256_rows_throughout_is_the_recorded_builder():
    """stage_bm = NULL or all 256: the table of aew_nt_chain_build, byte for byte"""
    case = CS.triple("cpu", 128, 256, 4)
    descs = [op.u.nt for op in case.plan.ops]
    n = len(descs)
    arr, ref = (L.GemmNT * n)(*descs), (L.NtStage * n)()
    bmap = (C.c_uint16 * 4096)()
    nb, nc, se = C.c_int(0), C.c_int(0), C.c_int(0)
    L.check(L.load().aew_nt_chain_build(C.byref(arr), n, C.byref(ref), C.byref(bmap), 8 * 4096, C.byref(nb), C.byref(nc), C.byref(se), 1), "build")
    for bms in (None, (256, 256, 256)):
        rc, st, nb2, nc2, se2, bmap2 = CS.build_table(descs, bms)
        assert rc == 0 and (nb2, nc2, se2) == (nb.value, nc.value, se.value)
        assert bytes(st) == bytes(ref) and bytes(bmap2) == bytes(bmap)


def test_builder_refuses_other_heights_and_the_forward_set():
    case = CS.triple("cpu", 128, 256, 4)
    descs = [op.u.nt for op in case.plan.ops]
    assert CS.build_table(descs, (128, 64, 128))[0] == L.E_ARG
    # a run without a DFG stage or a one-window STORE stage launches the forward body set: no 128-row bodies there
    plain = CS.triple("cpu", 128, 256, 128)
    assert CS.build_table([plain.plan.ops[0].u.nt], (128,))[0] == L.E_UNSUP
    assert CS.build_table([plain.plan.ops[0].u.nt], (256,))[0] == 0


def test_default_backward_chain_and_data_parallel_ranks(monkeypatch):
    """By default the backward is ONE chained launch with d.post / dz on 128-row tiles and dx on 256; a rank of a
    data-parallel group keeps the backward unchained (the cross-rank maximum of the guard word is issued before the second
    half of the decoder backward has run), the forward chain stays."""
    import torch
    from ae_wavenet_amd import config, model as M
    monkeypatch.delenv("AEW_NT_CHAIN", raising=False)
    hps = config.make_hps("vqvae-ema", n_win_batch=5000)
    eng = M.TrainEngine(hps, 8, "cpu", n_mel=39)
    (lab, (stages, _)), = eng.bwd.nt_chains.items()
    assert lab == "chain[d.post2..dx.0]" and len(stages) == 2 * len(eng.geom.layers) + 2
    for i, s in enumerate(stages):
        is_dx = i >= 2 and i % 2 == 1
        assert bool(s.kind & KIND_128) == (not is_dx) and s.n_mt == -(-s.g.M // _bm(s))
    for seed in range(2):
        _simulate(stages[:6], seed, slots=64)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    eng = M.TrainEngine(hps, 8, "cpu", n_mel=39)
    assert not getattr(eng.bwd, "nt_chains", {}) and eng.nt_chain_bwd_used == 0
    assert len(eng.fwd_b.nt_chains) == 2
