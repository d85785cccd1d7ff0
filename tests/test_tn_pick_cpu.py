"""The TN (weight-gradient) launch selection against the table recorded from the launchers it replaced
(tests/data/tn_pick_parent.json, see tests/data/tn_pick_gen.py: every descriptor under the default record, a thinned sweep
under the others): for every recorded tuning record x descriptor, aew_tn_pick
and aew_tn_group_pick name the same kernel instantiation on the same grid with the same block, LDS bytes, plan arguments
and return code; aew_tn_slabs, aew_tn_fold and aew_tn_group_check answer as recorded.  Host logic only - no device, nothing
is launched."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Mat, TnGroupBuilder, make_tn

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("tn_pick_gen", os.path.join(HERE, "data", "tn_pick_gen.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# every instantiation the two launchers can run: k_gemm_tn_bf16<0>, <1>, _big, _grp, _grp_cur, _grp32, _big_grp, _grp8,
# k_gemm_tn_f32, k_gemm_tn_check<uint16_t>, <float>
N_KERNELS = 11


@pytest.fixture(scope="module")
def table():
    with open(gen.TABLE) as f:
        return json.load(f)


TILES = {"k_gemm_tn_bf16_big": (256, 256), "k_gemm_tn_bf16_big_grp": (256, 256), "k_gemm_tn_bf16_grp8": (128, 256),
         "k_gemm_tn_f32": (64, 64), "k_gemm_tn_check<uint16_t>": (64, 1), "k_gemm_tn_check<float>": (64, 1)}     # others: 128 x 128


def same(p, launch, kernels):
    name, gx, gy, gz, threads, lds = launch[:6]
    assert (p.name.decode(), list(p.grid), p.threads, p.lds_bytes) == (kernels[name], [gx, gy, gz], threads, lds)
    assert (p.bk, p.bn) == TILES.get(kernels[name], (128, 128)), kernels[name]
    return kernels[name]


def test_pick_reproduces_every_recorded_launch(table):
    lib = L.load()
    keys, kernels = table["case_keys"], table["kernels"]
    assert len(kernels) == N_KERNELS and len(set(kernels)) == N_KERNELS
    descs = [gen.descriptor(dict(zip(keys, case))) for case in table["cases"]]
    groups = [gen.group(dict(zip(table["group_keys"], case))) for case in table["group_cases"]]
    seen, cur = set(), None
    rows = {}
    for r in table["rows"]:
        rows.setdefault(r[0], []).append(r)
    grows = {}
    for r in table["group_rows"]:
        grows.setdefault(r[0], []).append(r)
    assert len(rows[0]) == len(descs)                                # the default record: every case
    try:
        for ti, over in enumerate(table["tunings"]):
            gen.set_tuning(lib, over)
            for _, ci, rc, launch, slabs, fold in rows.get(ti, ()):
                g, what = descs[ci], (over, table["cases"][ci])
                p = L.TnPick()
                assert lib.aew_tn_pick(C.byref(g), C.byref(p)) == rc, what
                assert (lib.aew_tn_slabs(C.byref(g)), lib.aew_tn_fold(C.byref(g))) == (slabs, fold), what
                if rc == 0:
                    seen.add(same(p, launch, kernels))
                    assert [p.splits, p.rows_per_split, p.fold] == launch[6:9] and (p.slabs, p.fold) == (slabs, fold), what
                    assert (p.tile, p.rc) == ((128, 32) if g.dtype == L.BF16 else (64, 32)) and p.cursor == 0, what
            for _, gi, rc, launch in grows.get(ti, ()):
                gp, what = groups[gi], (over, table["group_cases"][gi])
                p = L.TnPick()
                assert lib.aew_tn_group_pick(C.byref(gp), C.byref(p)) == rc, what
                if rc == 0:
                    name = same(p, launch, kernels)
                    seen.add(name)
                    assert p.cursor == (name == "k_gemm_tn_bf16_grp_cur") and p.tile == gp.tile, what
                    if p.cursor:                                     # the arguments the cursor kernel is handed
                        assert [gp.cursor_stride, p.cursor_epoch, p.cursor_slack] == launch[6:9], what
    finally:
        gen.set_tuning(lib, {})
    assert seen == set(kernels), "table rows that were not compared"
    assert [lib.aew_tn_group_check(C.byref(g)) for g in descs] == table["group_check"]
    assert lib.aew_tn_pick(None, None) == L.E_ARG and lib.aew_tn_group_pick(None, None) == L.E_ARG
    assert lib.aew_tn_group_check(None) == L.E_ARG


def test_every_refusal_is_recorded(table):
    """One refused case per check of the stand-alone launcher and per grouped-only rule, each with its code."""
    keys = table["case_keys"]
    rc = {(c[keys.index("bad")], c[keys.index("dt")]): (r[2], gc) for c, r, gc in
          zip(table["cases"], [r for r in table["rows"] if r[0] == 0], table["group_check"])}
    for dt in (L.BF16, L.F32):
        for bad in gen.BAD:
            want = L.E_ALIGN if bad == "misalign" else L.E_ARG
            assert rc[(bad, dt)] == (want, want if dt == L.BF16 else L.E_ARG), (bad, dt)
    for bad in gen.GROUP_BAD:                                        # fine as stand-alone ops; as grouped descriptors:
        assert rc[(bad, L.BF16)] == (0, 0 if bad in ("snap_ok", "split_ok") else L.E_ARG), bad
    assert rc[("", L.F32)] == (0, L.E_ARG) and rc[("", L.BF16)] == (0, 0)      # grouped launches are bf16 only


def test_group_tiles_of_the_grouped_parity_descriptors():
    """aew_tn_group_tiles for the three descriptors of test_gemm_tn_group (N_pad x K_total = 256 x 896, 384 x 256,
    256 x 256): what TnGroupBuilder lays its tile map out on."""
    lib = L.load()
    sp = gen.AddrSpace()
    G, A = Mat.new(sp, "G", 3, 700, 384, L.BF16), Mat.new(sp, "A", 3, 760, 384, L.BF16)
    sp.alloc("o", 64, 0)
    descs = [make_tn(L.BF16, 690, 3, 256, 256, G.seg(256), [A.seg(384), A.seg(384, row_off=9), A.seg(128, row_off=31)]),
             make_tn(L.BF16, 650, 3, 368, 384, G.seg(384, hi=640), [A.seg(256)]),
             make_tn(L.BF16, 33, 3, 256, 256, G.seg(256, row_off=5), [A.seg(256, row_off=-2)])]
    nkt, nnt = C.c_int(), C.c_int()
    for tile, counts, grids in ((128, (14, 6, 4), ((7, 2), (2, 3), (2, 2))), (256, (4, 2, 1), ((4, 1), (1, 2), (1, 1))),
                                (384, (7, 3, 2), ((7, 1), (1, 3), (2, 1)))):
        gb = TnGroupBuilder(sp, "tng", tile)
        for t, n, grid in zip(descs, counts, grids):
            t.out = sp.ptr("o")
            assert lib.aew_tn_group_tiles(C.byref(t), tile, C.byref(nkt), C.byref(nnt)) == 0
            assert (nkt.value, nnt.value) == grid and nkt.value * nnt.value == n and gb._grid(t) == grid
            gb.add(t, "d")
        assert sorted(gb.tile_map()) == sorted([-1] * (len(gb.tile_map()) - sum(counts)) +
                                               [(d << 22) | tl for d, n in enumerate(counts) for tl in range(n)])
    assert lib.aew_tn_group_tiles(C.byref(descs[0]), 100, C.byref(nkt), C.byref(nnt)) == L.E_ARG
    assert lib.aew_tn_group_tiles(None, 128, C.byref(nkt), C.byref(nnt)) == L.E_ARG
