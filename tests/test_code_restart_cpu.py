"""Restart of dead codes (AEW_OP_VQ_RESTART) without a GPU: the row rule, the engine method and the module surface on a
CPU engine run by the interpreter of tests/code_restart_emulator.py, the launcher's refusals through ctypes (they come
before any launch), and the data-parallel path on two gloo ranks."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import autoencoder_model as ae, dp, model as M
from tests.code_restart_emulator import emulate_restart, restart_ab, restart_reference, restart_rows
from tests.test_dp_gloo import _free_port, _global_batch, _seed_engine, _tiny

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_USAGE = 0.005          # under the count of a code no sample chose in the first step (0.99 * 0.01), above the dead ones'
DEAD = {2: 0.001, 7: float("nan"), 11: 0.0}


def bits(t):
    return t.detach().cpu().numpy().tobytes()


# ----------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 2, 7, 12, 232, 1024])
def test_rows_are_distinct_and_the_stride_is_coprime(Q):
    rs = np.random.RandomState(Q)
    pairs = [(0, 0), (0, 1), (2 ** 64 - 1, 2 ** 64 - 1)] + [(int(rs.randint(0, 2 ** 62)), int(rs.randint(0, 2 ** 31)))
                                                           for _ in range(197)]
    assert len(pairs) == 200
    for seed, call in pairs:
        a, b = restart_ab(Q, seed, call)
        assert 0 <= a < Q and 1 <= b <= max(1, Q - 1) and math.gcd(b, Q) == 1
        rows = restart_rows(Q, min(Q, 1024), seed, call)
        assert len(set(rows)) == len(rows) and all(0 <= q < Q for q in rows)
    assert len({restart_ab(Q, s, c) for s, c in pairs}) > (1 if Q > 2 else 0)      # the counters do choose


@pytest.mark.parametrize("K,Q,n_dead,max_codes", [(16, 7, 0, 64), (16, 7, 3, 64), (16, 7, 16, 64), (300, 232, 300, 64),
                                                  (300, 232, 300, 1024), (40, 232, 40, 1024), (16, 1, 5, 64)])
def test_restarted_count_is_the_minimum(K, Q, n_dead, max_codes):
    rs = np.random.RandomState(K + Q)
    d = 3
    ze = rs.randn(Q, 8).astype(np.float32)
    emb, numer = rs.randn(K, d).astype(np.float32), rs.randn(K, d).astype(np.float32)
    denom = np.ones(K, np.float32)
    dead = np.sort(rs.permutation(K)[:n_dead])
    denom[dead] = 0.0
    e, nu, de, out, pairs = restart_reference(ze, emb, numer, denom, max_codes, 0.5, 0.37, 3, 4, total=10)
    n = min(n_dead, Q, max_codes)
    assert out.tolist() == [n_dead, n, 10 + n, 0]
    assert pairs[:n, 0].tolist() == dead[:n].tolist() and (pairs[n:] == -1).all()
    assert pairs[:n, 1].tolist() == restart_rows(Q, n, 3, 4)
    keep = np.setdiff1d(np.arange(K), dead[:n])
    assert e[keep].tobytes() == emb[keep].tobytes() and nu[keep].tobytes() == numer[keep].tobytes()
    assert de[keep].tobytes() == denom[keep].tobytes() and (de[dead[:n]] == np.float32(0.37)).all()
    for k, q in pairs[:n]:
        assert nu[k].tobytes() == (ze[q, :d] * np.float32(0.37)).tobytes()


# ----------------------------------------------------------------------------------------------
# the engine, run by the interpreter
# ----------------------------------------------------------------------------------------------
def _engine(bn="vqvae-ema", B=2):
    eng = emulate_restart(M.TrainEngine(_tiny(bn), B=B, device="cpu", n_mel=5))
    _seed_engine(eng)
    eng.set_inputs(*_global_batch(eng.geom, 5, B))
    return eng


def _codebook(eng):
    return [t.numpy().copy() for t in (eng.emb, eng.ema_numer, eng.ema_denom)]


def _ze(eng):
    return eng.lin.tensor().numpy().reshape(eng.Q, eng.nlin_p).copy()


def test_engine_restarts_exactly_the_dead_codes():
    eng = _engine()
    assert (eng.K, eng.d) == (16, 4)
    with pytest.raises(L.AewError, match="forward"):
        eng.restart_codes(MIN_USAGE, 5)
    assert eng.restart_buf is None, "a refused call allocates nothing"
    eng.forward()
    eng.backward()
    for k, v in DEAD.items():
        eng.ema_denom[k] = v
    assert sorted(k for k in range(eng.K) if not float(eng.ema_denom[k]) >= MIN_USAGE) == sorted(DEAD)
    ze, before = _ze(eng), _codebook(eng)
    want = restart_reference(ze, *before, 64, MIN_USAGE, 1.0, 0, 5)
    eng.restart_codes(MIN_USAGE, 5)
    got = _codebook(eng)
    for g, w, name in zip(got, want[:3], ("emb", "ema_numer", "ema_denom")):
        assert g.tobytes() == w.tobytes(), name
    rows = restart_rows(eng.Q, 3, 0, 5)
    pairs = eng.restart_pairs().numpy()
    assert pairs[:3].tolist() == [[k, q] for k, q in zip(sorted(DEAD), rows)] and (pairs[3:64] == -1).all()
    for k, q in pairs[:3]:                                           # denom_init = 1: the code IS the encoder output
        assert got[0][k].tobytes() == ze[q, :eng.d].tobytes() and got[2][k] == 1.0
    keep = [k for k in range(eng.K) if k not in DEAD]
    for g, b in zip(got, before):
        assert g[keep].tobytes() == b[keep].tobytes()
    assert eng.restart_out().tolist() == [3, 3, 3, 0]
    eng.restart_codes(MIN_USAGE, 6)                                 # nothing is dead any more
    assert eng.restart_out().tolist() == [0, 0, 3, 0]
    assert all(g.tobytes() == a.tobytes() for g, a in zip(got, _codebook(eng)))
    assert (eng.restart_pairs().numpy()[:64] == -1).all()
    # the sticky word of the chained launches raised: nothing is written
    eng.ema_denom[3] = 0.0
    eng.chain_guard[0] = 4
    held, pairs_held = _codebook(eng), bits(eng.restart_pairs())
    eng.restart_codes(MIN_USAGE, 7)
    assert all(h.tobytes() == a.tobytes() for h, a in zip(held, _codebook(eng)))
    assert eng.restart_out().tolist() == [0, 0, 3, 0] and bits(eng.restart_pairs()) == pairs_held
    eng.chain_guard[0] = 0
    eng.restart_codes(MIN_USAGE, 7, max_codes=1, denom_init=0.37)
    assert eng.restart_out().tolist() == [1, 1, 4, 0]
    q = restart_rows(eng.Q, 1, 0, 7)[0]
    nu = ze[q, :eng.d] * np.float32(0.37)
    assert eng.ema_numer[3].numpy().tobytes() == nu.tobytes()
    assert eng.emb[3].numpy().tobytes() == (nu / np.float32(0.37)).tobytes() and float(eng.ema_denom[3]) == float(np.float32(0.37))
    for bad in (dict(max_codes=0), dict(max_codes=1025), dict(denom_init=0.0), dict(denom_init=float("inf")), dict(seed=-1)):
        with pytest.raises(ValueError):
            eng.restart_codes(MIN_USAGE, 8, **bad)
    with pytest.raises(ValueError):
        eng.restart_codes(float("nan"), 8)


def test_engine_applies_a_deferred_ema_first():
    """A pending EMA accumulation would overwrite the restarted accumulators: restart_codes() finishes it first."""
    eng = _engine()
    eng.forward()
    order = []
    eng._ema_work = type("W", (), {"wait": lambda self: order.append("wait")})()
    run = eng._run
    eng._run = lambda plan, timing=False: (order.append(plan.name), run(plan, timing))
    inner = eng.restart.run
    eng.restart.run = lambda stream=0: (order.append("restart"), inner(stream))
    eng.restart_codes(MIN_USAGE, 1)
    assert order == ["wait", "ema", "restart"] and eng._ema_work is None


def test_other_bottlenecks_refuse():
    eng = _engine("vae")
    eng.forward()
    with pytest.raises(L.AewError, match="vqvae-ema"):
        eng.restart_codes(MIN_USAGE, 1)
    with pytest.raises(L.AewError, match="vqvae-ema"):
        eng.restart_out()
    assert not any(n.startswith("restart") for n in eng.ws.bufs)


def test_nothing_is_allocated_before_the_first_restart():
    """The buffer names of a freshly built engine are the parent's: the recording of tests/test_plan_parent_cpu.py for
    the default vqvae-ema configuration, and no `restart.` buffer nor restart op until the first call."""
    spec = importlib.util.spec_from_file_location("plan_gen", os.path.join(HERE, "data", "plan_gen.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.TABLE) as f:
        table = json.load(f)
    name = "default.vqvae-ema"
    eng = gen.build(gen.configs()[name])
    assert gen.record(eng)[0] == table["configs"][name]["alloc"]
    names = list(eng.ws.bufs)
    assert not any(n.startswith("restart") for n in names) and eng.restart.ops == [] and eng.restart_buf is None
    eng.restart_out()
    assert list(eng.ws.bufs) == names + ["restart.out", "restart.pairs"] and len(eng.restart.ops) == 1
    assert eng.restart.labels == ["vq.restart"] and eng.restart.ops[0].kind == L.OP_VQ_RESTART == 29
    eng.restart_pairs()
    assert list(eng.ws.bufs) == names + ["restart.out", "restart.pairs"] and len(eng.restart.ops) == 1


# ----------------------------------------------------------------------------------------------
# the module surface
# ----------------------------------------------------------------------------------------------
def _surface(**kw):
    hps = _tiny("vqvae-ema")
    torch.manual_seed(5)
    model = ae.AutoEncoder(hps, n_mel=5, **kw)
    eng = emulate_restart(M.TrainEngine(hps, B=2, device="cpu", n_mel=5))
    model._adopt_engine(eng)
    calls = []
    inner = eng.restart_codes
    eng.restart_codes = lambda *a, **k: (calls.append((a, k)), inner(*a, **k))[1]
    return model, eng, _global_batch(eng.geom, 5, 2), calls


def _steps(model, eng, batch, n):
    for _ in range(n):
        model.zero_grad()
        _, _, loss = model.run(*batch)
        loss.backward()
        eng.adam_step(1e-3)


def test_surface_restarts_every_second_step_and_reports_it():
    on, eng, batch, calls = _surface(codebook_restart=dict(every=2, min_usage=MIN_USAGE))
    seen = []
    for t in range(1, 5):
        _steps(on, eng, batch, 1)
        seen.append(len(calls))
    assert seen == [0, 1, 1, 2]                                     # on the backward of steps 2 and 4 only
    kw = dict(max_codes=64, denom_init=1.0, seed=0)
    assert calls == [((MIN_USAGE, 2), kw), ((MIN_USAGE, 4), kw)]
    m = on.objective.metrics
    assert m["vq_restarted"].dim() == 0 and m["vq_restarted"].dtype == torch.int32
    assert m["vq_restarted"].data_ptr() == eng.restart_out().data_ptr() + 4
    assert on.bottleneck.restart_counts.data_ptr() == eng.restart_out().data_ptr()
    # the explicit call: defaults from the option, call = the engine's step count
    on.bottleneck.restart_dead_codes()
    on.bottleneck.restart_dead_codes(min_usage=0.5, call=77)
    assert calls[2:] == [((MIN_USAGE, 4), kw), ((0.5, 77), kw)]
    n = min(eng.K, eng.Q, 64)
    assert on.bottleneck.restart_counts.tolist()[:2] == [eng.K, n] and int(m["vq_restarted"]) == n
    # off: today's metrics, no call, nothing allocated - and the same state_dict keys either way
    off, eng2, batch2, calls2 = _surface()
    _steps(off, eng2, batch2, 2)
    assert calls2 == [] and eng2.restart_buf is None
    assert set(m) - set(off.objective.metrics) == {"vq_restarted"} and set(off.objective.metrics) <= set(m)
    assert list(on.state_dict()) == list(off.state_dict())
    with pytest.raises(L.AewError, match="min_usage"):
        off.bottleneck.restart_dead_codes()
    off.bottleneck.restart_dead_codes(min_usage=MIN_USAGE)
    assert calls2 == [((MIN_USAGE, 2), kw)]


def test_surface_option_validation():
    hps = _tiny("vqvae-ema")
    good = dict(every=3, min_usage=0.1)
    for bad in (3, "x", {}, dict(every=3), dict(min_usage=0.1), dict(good, every=0), dict(good, every=1.5), dict(good, every=True),
                dict(good, min_usage=0.0), dict(good, min_usage=-1.0), dict(good, min_usage=float("nan")),
                dict(good, min_usage=float("inf")), dict(good, min_usage="x"), dict(good, max_codes=0),
                dict(good, max_codes=1025), dict(good, max_codes=2.0), dict(good, denom_init=0.0),
                dict(good, denom_init=float("inf")), dict(good, seed=-1), dict(good, seed=0.5), dict(good, often=1)):
        with pytest.raises(ValueError):
            ae.AutoEncoder(hps, n_mel=5, codebook_restart=bad)
    m = ae.AutoEncoder(hps, n_mel=5, codebook_restart=dict(good, max_codes=np.int64(7), min_usage=np.float32(0.25), seed=9))
    assert m._restart == dict(every=3, min_usage=0.25, max_codes=7, denom_init=1.0, seed=9)
    assert ae.AutoEncoder(hps, n_mel=5)._restart is None
    with pytest.raises(ValueError, match="vqvae-ema"):
        ae.AutoEncoder(_tiny("vae"), n_mel=5, codebook_restart=good)
    with pytest.raises(L.AewError, match="vqvae-ema"):
        ae.AutoEncoder(_tiny("vae"), n_mel=5).bottleneck.restart_dead_codes(min_usage=0.1)
    with pytest.raises(L.AewError):                                 # no engine yet: no encoder outputs to take
        m.bottleneck.restart_dead_codes()


# ----------------------------------------------------------------------------------------------
# the launcher's refusals: host memory, no launch
# ----------------------------------------------------------------------------------------------
def _record(host, **over):
    op = L.Op()
    op.kind = L.OP_VQ_RESTART
    r = op.u.vqr
    base = (C.addressof(host) + 63) & ~63
    r.ze, r.emb, r.numer, r.denom = base, base + 4096, base + 8192, base + 12288
    r.out, r.pairs, r.guard = base + 16384, base + 16400, None
    r.Q, r.d, r.d_pitch, r.K, r.max_codes = 4, 4, 8, 16, 8
    r.min_usage, r.denom_init, r.seed, r.call = 0.5, 1.0, 1, 2
    for k, v in over.items():
        setattr(r, k, v(base) if callable(v) else v)
    return op


def test_argument_errors_come_before_any_launch():
    lib = L.load()
    assert lib.aew_abi_version() >= 25 and lib.aew_sizeof(18) == C.sizeof(L.VqRestart) and L.VQ_RESTART_MAX == 1024
    host = (C.c_uint8 * (20480 + 64))()
    cases = [(dict(Q=0), L.E_ARG), (dict(K=0), L.E_ARG), (dict(d=0), L.E_ARG), (dict(Q=-3), L.E_ARG), (dict(d_pitch=3), L.E_ARG),
             (dict(max_codes=0), L.E_ARG), (dict(max_codes=1025), L.E_ARG), (dict(denom_init=0.0), L.E_ARG),
             (dict(denom_init=-1.0), L.E_ARG), (dict(denom_init=float("inf")), L.E_ARG),
             (dict(denom_init=float("nan")), L.E_ARG), (dict(min_usage=float("nan")), L.E_ARG)]
    cases += [({f: None}, L.E_ARG) for f in ("ze", "emb", "numer", "denom", "out")]
    cases += [({f: (lambda off: (lambda b: b + off))(off)}, L.E_ALIGN)
              for f, off in (("ze", 2), ("emb", 4097), ("numer", 8194), ("denom", 12291), ("out", 16386), ("pairs", 16401),
                             ("guard", 18002))]
    for over, want in cases:
        fail = C.c_int(-1)
        op = _record(host, **over)
        assert lib.aew_run_plan(C.byref(op), 1, None, C.byref(fail)) == want, over
        assert fail.value == 0
    assert bytes(host) == bytes(20480 + 64)


# ----------------------------------------------------------------------------------------------
# two gloo ranks
# ----------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = emulate_restart(M.TrainEngine(_tiny("vqvae-ema"), B=1, device="cpu", n_mel=5))
        _seed_engine(eng)                                           # the same codebook state on every rank ...
        for k, v in DEAD.items():
            eng.ema_denom[k] = v
        eng.lin.tensor().copy_(torch.randn(eng.lin.tensor().shape, generator=torch.Generator().manual_seed(50 + rank)))
        eng.lin_live = True                                         # ... and each rank's own encoder outputs
        d = dp.DataParallel()
        before, ze = _codebook(eng), _ze(eng)
        d.restart_codes(eng, MIN_USAGE, 9, max_codes=64, denom_init=0.37, seed=3)
        first = (_codebook(eng), eng.restart_out().tolist())
        # a second restart that rank 1's own guard word turns into a no-op there: codebook, counts and pairs still come
        # out as rank 0's on both ranks
        eng.ema_denom[5] = 0.0
        eng.chain_guard[0] = rank
        mid = _codebook(eng)
        d.restart_codes(eng, MIN_USAGE, 10, max_codes=8, denom_init=1.0, seed=3)
        q.put((rank, ze, before, first[0], first[1], mid, _codebook(eng), eng.restart_out().tolist(),
               eng.restart_pairs().numpy()[:8].copy()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_replicas_take_rank_zeros_rows():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, ze0, before0, after0, out0, mid0, last0, lout0, lpairs0), (_, ze1, before1, after1, out1, _, last1, lout1, lpairs1) = res
    assert ze0.tobytes() != ze1.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(before0, before1))
    want = restart_reference(ze0, *before0, 64, MIN_USAGE, 0.37, 3, 9)
    own1 = restart_reference(ze1, *before1, 64, MIN_USAGE, 0.37, 3, 9)
    n = min(3, ze0.shape[0])
    assert out0 == out1 == [3, n, n, 0] == want[3].tolist()
    assert want[0].tobytes() != own1[0].tobytes(), "the ranks would have seeded different vectors"
    for a0, a1, w, name in zip(after0, after1, want[:3], ("emb", "ema_numer", "ema_denom")):
        assert a0.tobytes() == w.tobytes() and a1.tobytes() == w.tobytes(), name
    want2 = restart_reference(ze0, *mid0, 8, MIN_USAGE, 1.0, 3, 10, total=n)
    assert lout0 == lout1 == want2[3].tolist() == [1, 1, n + 1, 0]
    assert lpairs0.tobytes() == lpairs1.tobytes() == want2[4].tobytes() and lpairs0[0, 0] == 5
    for a0, a1, w, name in zip(last0, last1, want2[:3], ("emb", "ema_numer", "ema_denom")):
        assert a0.tobytes() == w.tobytes() and a1.tobytes() == w.tobytes(), name
