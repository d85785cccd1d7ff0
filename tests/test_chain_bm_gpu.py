"""The chained launch on 128-row tiles (csrc/aew_chain.hip, aew_nt_chain_build_bm) on the MI355X.

Kernel level: a forced dz -> dx pair and a three-stage run (dx.a -> dz -> dx: K-loop and epilogue reads of an earlier
stage), B = 2, M = 300 (three 128-row tiles, a ragged last one), N_pad in {128, 256, 384}, dilation 1 (one-window body)
and 128 (plain body), DFG and STORE | ADD_AUX0 - every output byte-equal to the same ops launched one by one, under both
epilogue forms, no hand-off wait given up.  The launcher's small-launch shapes are switched off for the module, so that
the stand-alone launches run the bodies (plain / one-window K order) the chain runs.

Engine level: two training steps of the tiny vqvae-ema golden model with the backward chained on 128 rows against the
unchained engine: gradients, parameters and codebook bit-equal."""
import pytest
import torch

from ae_wavenet_amd import _lib as L, model as M, plan as PLN
from tests import chain_bm_cases as CS
from tests.test_gpu_parity import DEV, load, tiny_hps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big_shapes():
    lib = L.load()
    was = L.current_tuning()
    lib.aew_set_nt_small_tiles(0)
    yield lib
    lib.aew_set_nt_small_tiles(int(was.nt_small_tiles))
    lib.aew_set_nt_epi_lines(L.NT_EPI_LINES_DEFAULT)


def _run(plan, case):
    for n in case.outs:
        case.ws.get(n).zero_()
    plan.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [case.ws.get(n).clone() for n in case.outs]


def _ran(sub):
    """the launch's counters after the run: every row tile of a stage that is waited for was published by all its N tiles"""
    (stages, cd), = sub.nt_chains.values()
    cnt = cd.cpu().tolist()
    for s in stages:
        want = s.n_nt if s.publish else 0
        assert cnt[s.cnt_base:s.cnt_base + s.n_mt * s.g.batch] == [want] * (s.n_mt * s.g.batch)
    assert PLN.chain_timeouts(sub) == [], PLN.chain_stats(sub)


@pytest.mark.parametrize("d", [1, 128])
@pytest.mark.parametrize("dp,rp,n", [(128, 256, None), (256, 384, 248), (384, 128, None)])
@pytest.mark.parametrize("shape", ["pair", "triple"])
def test_128_row_stages_are_byte_equal_to_one_launch_per_op(big_shapes, shape, dp, rp, n, d):
    lib = big_shapes
    case = getattr(CS, shape)(DEV, dp, rp, d, n=n)
    ns = len(case.plan.ops)
    subs = {"128": CS.chained(case, 128, "chain.a"), "mixed": CS.chained(case, ((128, 256) * 2)[:ns], "chain.b"),
            "256": CS.chained(case, 256, "chain.c")}
    body = 1 if d <= 16 else 0
    for lab, sub in subs.items():
        (stages, _), = sub.nt_chains.values()
        hs = {"128": [128] * ns, "mixed": [128, 256, 128][:ns], "256": [256] * ns}[lab]
        assert [s.kind for s in stages] == [(0 if s.g.epi == L.EPI_DFG else body) + (4 if h == 128 else 0) for s, h in zip(stages, hs)]
    for lines in (0, 1):
        lib.aew_set_nt_epi_lines(lines)
        ref = _run(case.plan, case)
        assert all(bool(r.float().abs().sum() > 0) for r in ref)
        for lab, sub in subs.items():
            got = _run(sub, case)
            _ran(sub)
            for name, a, b in zip(case.outs, ref, got):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (lab, lines, name)


def _tiny_engine(z, golden):
    hps, nm = tiny_hps(z, global_model="autoencoder")
    e = M.TrainEngine(hps, B=z["wav"].shape[0], device=DEV, n_mel=nm, take_compat=True, update_codebook_every_step=False,
                      loss_mode="intended")
    for k in e.ps.names():
        e.ps.view(k).copy_(torch.from_numpy(z["w." + k]))
    e.emb.copy_(torch.from_numpy(z["emb0"]))
    e.init_ema_from_emb()
    e.set_inputs(*[torch.from_numpy(z[k]).to(DEV) for k in ("wav", "mel", "voice", "jitter")])
    return e


def test_two_steps_with_the_backward_chained_on_128_rows(big_shapes, golden_dir, monkeypatch):
    monkeypatch.delenv("AEW_NT_CHAIN", raising=False)
    monkeypatch.setattr(M.TrainEngine, "nt_chain_force", True)
    z = load(golden_dir, "ae_tiny_vqvae-ema_random.npz")
    res = {}
    for key, bwd in (("serial", 0), ("chained", (64, 128))):
        monkeypatch.setattr(M.TrainEngine, "nt_chain_bwd", bwd)
        eng = _tiny_engine(z, golden_dir)
        chains = getattr(eng.bwd, "nt_chains", {})
        steps = []
        for _ in range(2):
            eng.forward()
            eng.backward()
            torch.cuda.synchronize()
            grads = eng.ps.grads.clone()
            if key == "chained":                                # the chained launch ran: its counters, no wait gave up
                (stages, cd), = chains.values()                 # d.post2, d.post1, then dz / dx of every layer
                assert all(s.kind & 4 for s in stages) and len(stages) == 2 * len(eng.geom.layers) + 2
                cnt = cd.cpu().tolist()
                assert all(cnt[s.cnt_base:s.cnt_base + s.n_mt * s.g.batch] == [s.n_nt if s.publish else 0] * (s.n_mt * s.g.batch)
                           for s in stages)
                assert any(s.publish for s in stages) and PLN.chain_timeouts(eng.bwd) == []
            else:
                assert not chains
            eng.adam_step(1e-3)
            eng.update_codebook()
            torch.cuda.synchronize()
            steps.append((grads, eng.ps.params.clone(), eng.emb.clone()))
        assert int(eng.chain_guard[0]) == 0
        res[key] = steps
        del eng
    for i, (a, b) in enumerate(zip(res["serial"], res["chained"])):
        for what, x, y in zip(("gradients", "parameters", "codebook"), a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (i, what)
