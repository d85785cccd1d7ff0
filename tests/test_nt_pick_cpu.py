"""The NT kernel selection against the table recorded from the launcher it replaced (tests/data/nt_pick_parent.json, see
tests/data/nt_pick_gen.py): for every recorded tuning record x descriptor, aew_nt_pick names the same kernel
instantiation on the same grid with the same block, LDS bytes and return code; aew_gemm_nt_small_split and
aew_nt_chain_build answer as recorded.  Host logic only - no device, nothing is launched."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from ae_wavenet_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("nt_pick_gen", os.path.join(HERE, "data", "nt_pick_gen.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# instantiations the recorded launcher could reach: 65 of k_gemm_nt_bf16 / _pipe / _p64 (17 shapes x 4 epilogues less the
# 128-row memory-bound tile for GATED / RES_SKIP and the 16-wave tile for RES_SKIP, which no record selects), 6 window
# kernels, 8 fp32, 2 check, 14 full-N
N_REACHABLE = 65 + 6 + 8 + 2 + 14


@pytest.fixture(scope="module")
def table():
    with open(gen.TABLE) as f:
        return json.load(f)


def pick(lib, g):
    out = L.NtPick()
    rc = lib.aew_nt_pick(C.byref(g), C.byref(out))
    return rc, out


def test_pick_reproduces_every_recorded_launch(table):
    lib = L.load()
    keys, kernels = table["case_keys"], table["kernels"]
    assert len(kernels) == N_REACHABLE and len(set(kernels)) == N_REACHABLE
    descs = [(dict(zip(keys, case)), gen.descriptor(dict(zip(keys, case)))) for case in table["cases"]]
    seen, cur = set(), None

    def same(p, launch, what):
        name, grid, threads, lds = launch
        name = kernels[name]
        seen.add(name)
        if p.kernel == 2:                                            # full-N kernels keep their own launcher (name "k_fn", no LDS figure)
            assert name.startswith("k_fn<") and (p.name.decode(), p.grid, p.threads, p.variant) == ("k_fn", grid, threads, -1), what
        else:
            assert (p.name.decode(), p.grid, p.threads, p.lds_bytes) == (name, grid, threads, lds), what
            assert p.variant >= 0 and (p.dwp != 0) == name.startswith("k_gemm_nt_bf16_win") == (p.kernel == 6), what

    try:
        for ti, ci, rc, launches, split, chain in table["rows"]:
            if ti != cur:
                gen.set_tuning(lib, table["tunings"][ti])
                cur = ti
            c, g = descs[ci]
            got, p = pick(lib, g)
            what = (table["tunings"][ti], c)
            assert got == rc, what
            if rc == 0:
                same(p, launches[0], what)
                # a fused gated layer that runs unfused is two launches: the pick is the first, the GATED one; the
                # STORE | ADD_AUX0 GEMM over z that follows goes through the pick as a descriptor of its own
                assert len(launches) == 1 or (c["w2"] and len(launches) == 2), what
                if len(launches) == 2:
                    got2, p2 = pick(lib, gen.second_launch(g))
                    assert got2 == 0, what
                    same(p2, launches[1], what)
                assert lib.aew_nt_kernel(C.byref(g)) == p.kernel, what
            if split is not None:
                assert gen.small_split(lib, g) == split, what
            if chain is not None:
                assert gen.chain_codes(lib, c) == chain, what
    finally:
        gen.set_tuning(lib, {})
    assert seen == set(kernels), "table rows that were not compared"


def test_pick_kernel_codes_under_the_default_record():
    """aew_nt_kernel = the pick's code; under the default record: small launches 1, the window pair 6, full-N 2, else 0."""
    lib = L.load()
    base = dict(dt=L.BF16, epi=L.EPI_GATED, M=6000, B=8, Np=512, K=768, seg="near", impl=0, w2=0, ks=1, nsplit=128, bad="")
    code = lambda **kw: pick(lib, gen.descriptor(dict(base, **kw)))[1].kernel
    assert (code(), code(seg="far"), code(M=70), code(impl=2), code(impl=1), code(dt=L.F32, epi=L.EPI_STORE)) == (6, 0, 1, 2, 4, 3)
    try:
        # the deep-ring A/B shapes replace the window kernel: the query follows the launcher
        gen.set_tuning(lib, dict(nt_deep=1))
        rc, p = pick(lib, gen.descriptor(base))
        assert (rc, p.kernel, p.dwp, p.name.decode()) == (0, 5, 0, "k_gemm_nt_bf16<1,false,4,1,256,6>")
    finally:
        gen.set_tuning(lib, {})


def test_ablation_build_pairs_the_grid_with_the_kernel():
    """Tools build (-DAEW_FN_ABLATE=1): a descriptor with ablation switches takes an ablation variant only where the
    shape picked has one, so the grid is always the launched kernel's own.  Skips unless somebody has compiled the tools
    library next to the product one (the build does not: add -DAEW_FN_ABLATE=1 -o .../lib/libaewavenet_hip_abl.so to its
    hipcc line); the product build has no ablation variants."""
    path = os.path.join(os.path.dirname(L.LIB_PATH), "libaewavenet_hip_abl.so")
    if not os.path.exists(path):
        pytest.skip("tools library not built")
    lib = C.CDLL(path)
    base = dict(dt=L.BF16, epi=L.EPI_GATED, M=6000, B=8, Np=512, K=768, seg="far", impl=0, w2=0, ks=1, nsplit=128, bad="")
    g = gen.descriptor(base)
    g.reserved = 1
    try:
        for rows, want in ((512, "k_gemm_nt_bf16<1,false,4,2>"), (64, "k_gemm_nt_bf16<1,true,4>"), (256, "k_gemm_nt_bf16<1,true,8,2>")):
            gen.set_tuning(lib, dict(nt_wave_rows=rows, nt_rows192=0, nt_pipe=0))
            out = L.NtPick()
            assert lib.aew_nt_pick(C.byref(g), C.byref(out)) == 0
            assert out.name.decode() == want
            assert out.grid == (((g.M + out.bm - 1) // out.bm * g.batch + 7) // 8) * 8 * (g.N_pad // out.bn)
            assert out.bn == (256 if rows != 64 else 128)
    finally:
        gen.set_tuning(lib, {})
