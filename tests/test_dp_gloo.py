"""Data-parallel path on CPU: world_size 2, gloo.  Covers the sampler sharding rule, the
bucketed gradient all-reduce, the EMA-statistics all-reduce and the parameter broadcast of
ae_wavenet_amd.dp (the GPU run uses the same code over RCCL)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import config, dp, model as M


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = config.make_hps("vqvae-ema", n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2,
                              n_speakers=3, n_blocks=1, n_block_layers=2, enc_n_out=8, bn_n_out=4,
                              bn_vq_n_embed=16, n_win_batch=5)
        eng = M.TrainEngine(hps, B=1, device="cpu", n_mel=5)          # plans only; buffers on CPU
        d = dp.DataParallel(bucket_mb=0.001)                           # tiny buckets -> several all-reduces
        n = eng.ps.numel
        torch.manual_seed(100 + rank)
        eng.ps.params[:n].normal_()
        eng.emb.normal_()
        d.broadcast_params(eng, src=0)
        p_sum = eng.ps.params[:n].sum().item()
        eng.ps.grads[:n].copy_(torch.arange(n, dtype=torch.float32) * (rank + 1))
        d.allreduce_grads(eng)
        g_bucketed = eng.ps.grads[:n].tolist()
        # overlapped exchange: the engine's backward is replaced by one that writes the two halves of the
        # gradient buffer at the two points the real plans would (decoder tail first, then the head)
        lo = eng.dec_grad_offset
        assert 0 < lo < n and eng.bwd_a.ops and eng.bwd_b.ops
        assert len(eng.bwd_a.ops) + len(eng.bwd_b.ops) == len(eng.bwd.ops)
        order = []

        def fake_backward(timing=False, after_decoder=None):
            eng.ps.grads[:n].zero_()
            eng.ps.grads[lo:n].copy_(torch.arange(lo, n, dtype=torch.float32) * (rank + 1))
            order.append("dec")
            after_decoder()
            order.append("hook")
            eng.ps.grads[:lo].copy_(torch.arange(lo, dtype=torch.float32) * (rank + 1))
            order.append("enc")

        eng.backward = fake_backward
        d.backward_allreduce(eng)
        assert order == ["dec", "hook", "enc"]
        g_overlap = eng.ps.grads[:n].tolist()
        # full overlapped step (EMA statistics async + deferred, decoder / encoder gradient halves, ranged Adam)
        calls = []

        def fake_forward(ema_allreduce=None, timing=False):
            eng.z_sum.fill_(10.0 * (rank + 1))
            eng.n_sum.fill_(100.0 * (rank + 1))
            w = ema_allreduce(eng.z_sum, eng.n_sum)
            assert w is not None                      # async handle -> the engine defers the EMA accumulation
            eng._ema_work = w
            calls.append("fwd")

        def fake_backward2(timing=False, after_decoder=None):
            fake_backward(timing, after_decoder)
            eng._ema_work.wait()
            eng._ema_work = None
            calls.append(("ema", eng.z_sum[0, 0].item(), eng.n_sum[-1].item()))

        def fake_adam(lr, gs=1.0, lo=0, hi=None, count=True, **kw):
            hi = n if hi is None else hi
            calls.append(("adam", lo, hi, count, eng.ps.grads[lo].item(), eng.ps.grads[hi - 1].item()))

        eng.forward, eng.backward, eng.adam_step = fake_forward, fake_backward2, fake_adam
        order.clear()
        d.train_step(eng, 1e-3)
        assert calls[0] == "fwd" and calls[1] == ("ema", 30.0, 300.0)            # summed over both ranks
        assert calls[2] == ("adam", lo, n, True, 3.0 * lo, 3.0 * (n - 1))          # decoder range first, reduced
        assert calls[3] == ("adam", 0, lo, False, 0.0, 3.0 * (lo - 1))            # then the head, same step count
        eng.z_sum.fill_(rank + 1.0)
        eng.n_sum.fill_(2.0 * (rank + 1))
        d.allreduce_ema(eng.z_sum, eng.n_sum)
        q.put((rank, p_sum, g_overlap, eng.z_sum[0, 0].item(), eng.n_sum[0].item(),
               eng.emb.sum().item(), d.grad_scale(True), d.grad_scale(False), g_bucketed))
    finally:
        dist.destroy_process_group()


def test_dp_world2_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, ps0, g0, z0, n0, e0, gm0, gs0, gb0), (r1, ps1, g1, z1, n1, e1, gm1, gs1, gb1) = res
    assert gb0 == gb1 == g0                               # bucketed and overlapped exchange agree
    assert ps0 == ps1 and e0 == e1                       # broadcast made the replicas identical
    assert g0 == g1 and g0 == [3.0 * i for i in range(len(g0))]      # SUM over ranks, every bucket
    assert z0 == z1 == 3.0 and n0 == n1 == 6.0            # EMA statistics summed over ranks
    assert gm0 == 0.5 and gs0 == 1.0                      # mean-type losses scale by 1/world


def test_shard_indices_match_reference_rule():
    """data.py:100-106: rank r of W takes range(r, n, W) permuted with seed epoch*W + r."""
    n, W = 23, 4
    seen = []
    for r in range(W):
        idx = dp.shard_indices(n, r, W, epoch=3)
        g = torch.Generator().manual_seed(3 * W + r)
        vals = list(range(r, n, W))
        perm = torch.randperm(len(vals), generator=g).tolist()
        assert idx == [vals[i] for i in perm]
        seen += idx
    assert sorted(seen) == list(range(n))                 # the shards partition the dataset


# ----------------------------------------------------------------------------------------------
# real training steps on two ranks (plans executed by the CPU interpreter) vs ONE process on the global batch
# ----------------------------------------------------------------------------------------------
def _tiny(bn):
    return config.make_hps(bn, n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=3,
                           n_blocks=1, n_block_layers=2, enc_n_out=8, bn_n_out=4, bn_vq_n_embed=16, n_win_batch=6)


def _seed_engine(eng, seed=7):
    gen = torch.Generator().manual_seed(seed)
    n = eng.ps.numel
    eng.ps.params[:n].copy_(torch.randn(n, generator=gen) * 0.3)
    if eng.bn_type == "vqvae-ema":
        eng.emb.copy_(torch.randn(eng.emb.shape, generator=gen))
        eng.init_ema_from_emb()
    zero = torch.zeros(n)
    eng.load_opt_state(M.OptState(0, zero, zero))


def _global_batch(eng_geom, n_mel, world, seed=3):
    gen = torch.Generator().manual_seed(seed)
    g = eng_geom
    wav = torch.randint(0, 256, (world, g.enc_in_len), generator=gen).float()
    mel = torch.randn(world, n_mel, g.mel_len, generator=gen)
    voice = torch.randint(0, 3, (world,), generator=gen)
    jitter = torch.arange(g.embed_len).repeat(world, 1)
    return wav, mel, voice, jitter


def _real_worker(rank, world, port, bn, q, wg=None):
    from tests.plan_emulator import emulate
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny(bn)
        eng = emulate(M.TrainEngine(hps, B=1, device="cpu", n_mel=5, wgrad_group=wg))
        if wg is not None:
            # two grouped weight-gradient launches: the upper layer's region is exchanged on its own, after bwd_a1
            assert eng.dec_hi_offset is not None and eng.dec_grad_offset < eng.dec_hi_offset < eng.ps.numel
            assert eng.bwd_a1.labels[-1] == "unpack grads (decoder, upper layers)" and "spk_bwd (upper layers)" in eng.bwd_a1.labels
            assert len(eng.bwd_a1.ops) + len(eng.bwd_a2.ops) == len(eng.bwd_a.ops)
        d = dp.DataParallel()
        d.prepare_vae(eng)
        if world == 8:
            # every region splits into 8 shards of a multiple of 4 elements PLUS a replicated remainder (all-reduced, updated
            # by every rank): the tiny model's regions are not multiples of 32
            rems = []
            for a, b in d._regions(eng):
                s_, rem = d._split(a, b)
                assert s_ > 0 and s_ % 4 == 0 and 0 <= b - rem < 32, (a, b, s_, rem)
                rems.append(b - rem)
            assert any(r > 0 for r in rems), rems                  # (at least one region is not a multiple of 32)
        batch = _global_batch(eng.geom, 5, world)
        mine = [t[rank:rank + 1] for t in batch]
        eps_all = None
        if bn == "vae":                                           # the same noise in the N-rank and the 1-process run
            eps_all = torch.randn(world, eng.eps.shape[1], eng.eps.shape[2], generator=torch.Generator().manual_seed(11))
            eng.set_anneal_weight(0.3)
            d.prepare_vae(eng)
        gs = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
        out = {}
        n = eng.ps.numel
        for name in ("allreduce", "sharded", "sharded_bf16"):
            _seed_engine(eng)
            eng.set_inputs(*mine, eps=None if eps_all is None else eps_all[rank:rank + 1])
            # two steps: the second sees the exchanged state.  bf16 transport is held to ONE step: its rounding moves a
            # few parameters by ~lr in step 1, after which code assignments can flip and the trajectories part for real
            for it in range(1 if name.endswith("bf16") else 2):
                if name == "allreduce":
                    d.train_step(eng, 1e-2, gs)
                else:
                    d.train_step_sharded(eng, 1e-2, gs, bf16_grads=name.endswith("bf16"))
                    if name == "sharded" and it == 0:
                        # the parameter all-gathers stay in flight: the head's (what the encoder forward reads) was issued
                        # first - collectives complete in issue order - and is the only one the next forward waits for
                        # before its first plan; the decoder's weights are packed at the head of the second plan
                        tags = [t for t, _ in d._pending]
                        assert tags and tags[0] == "head" and set(tags[1:]) == {"dec"}, tags
                        assert "pack weights (decoder)" in eng.fwd_b.labels and "pack weights (decoder)" not in eng.fwd_a.labels
                        d.finish("head")
                        assert [t for t, _ in d._pending] == tags[1:]
            d.finish()
            assert d._pending == []
            if name != "allreduce":
                d.gather_moments(eng)
            out[name] = (eng.ps.params[:n].numpy().copy(), eng.adam_m[:n].numpy().copy(),
                         eng.emb.numpy().copy() if eng.bn_type == "vqvae-ema" else None)    # numpy: pickled by value
        ref = None
        if rank == 0:                                             # the same two steps in ONE process, global batch
            one = emulate(M.TrainEngine(hps, B=world, device="cpu", n_mel=5))      # (one grouped launch, one region)
            _seed_engine(one)
            one.set_inputs(*batch, eps=eps_all)
            if bn == "vae":
                one.set_anneal_weight(0.3)
            ref = []
            for it in range(2):
                one.forward(); one.backward(); one.adam_step(1e-2, 1.0)
                ref.append((one.ps.params[:n].numpy().copy(), one.adam_m[:n].numpy().copy(),
                            one.emb.numpy().copy() if one.bn_type == "vqvae-ema" else None))
        q.put((rank, out, ref))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bn,world,wg", [("vqvae-ema", 2, None), ("ae", 2, None), ("vqvae-ema", 3, None), ("vae", 2, None),
                                         ("vqvae-ema", 2, 1), ("vqvae-ema", 3, 1),
                                         # the world size of the target machine (BASELINE configs[2]: 8 x MI355X): shards of
                                         # 1/8 with a replicated remainder in every region, the three-region exchange, the
                                         # deferred all-gather order and the EMA sum over 8 ranks
                                         ("vqvae-ema", 8, None), ("vqvae-ema", 8, 1)])
def test_dp_real_steps_match_single_process_global_batch(bn, world, wg):
    """Sum-type loss (VQ-VAE-EMA: summed gradients, one codebook from summed EMA statistics) and mean-type loss (AE:
    the optimizer scales the summed gradient by 1 / world): N ranks with one window each == one process with all N.
    world = 3: shards that do not divide the regions (the replicated remainder), a ring that is not a power of two.
    VAE (vae_bn.py:90-116): mean-type NLL + the KL SUM over all windows of the global batch behind a free-nats clamp - the
    gate has to see the global KL (one scalar all-reduce) and the KL gradient must not be divided by world.
    wg = 1: the engines of the ranks emit the stack's weight gradients as TWO grouped launches (AEW_WGRAD_GROUP) and the
    sharded schedule exchanges three regions - the upper layer's as soon as bwd_a1 has run; same parameters, moments and
    codebook as the single process with its one launch."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_real_worker, args=(r, world, port, bn, q, wg)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, o0, ref), (_, o1, _) = res[0], res[-1]
    for _, ok, _ in res[1:-1]:                                    # every rank in between holds the same replica
        for name in ok:
            assert (ok[name][0] == o0[name][0]).all() and (ok[name][1] == o0[name][1]).all(), name
    T = lambda a: None if a is None else torch.from_numpy(a)
    o0 = {k: tuple(T(a) for a in v) for k, v in o0.items()}
    o1 = {k: tuple(T(a) for a in v) for k, v in o1.items()}
    # bf16 transport: Adam's normalised update moves a parameter by up to lr whatever the size of its gradient, so
    # rounding a near-zero summed gradient can cost a sizeable part of lr = 1e-2 on a few parameters
    for name, tol in (("allreduce", 2e-5), ("sharded", 2e-5), ("sharded_bf16", 1.5e-2)):
        p_ref, m_ref, e_ref = (T(a) for a in ref[0 if name.endswith("bf16") else 1])
        scale = float(p_ref.abs().max())
        pa, ma, ea = o0[name]
        pb, mb, eb = o1[name]
        assert torch.equal(pa, pb), name                                   # the replicas stay identical
        assert torch.equal(ma, mb), name                                   # gathered moments too
        # (bf16 transport: a summed gradient near zero may change SIGN in the rounding, and Adam's first step is lr * sign(g):
        # 2 lr on such a parameter - seen at world 8, where seven more hops round)
        bound = max(tol * scale, 2.05e-2) if name.endswith("bf16") else tol * scale
        assert float((pa - p_ref).abs().max()) <= bound, (name, float((pa - p_ref).abs().max()), scale)
        # (bf16 transport rounds every summed gradient to 8 bits of mantissa; Adam's normalised update then moves
        # near-zero-gradient parameters differently in step 1, which step 2's moments see: looser bound)
        mtol = 1e-2 if name.endswith("bf16") else tol             # one step: m = (1 - beta1) g, g rounded to bf16
        assert float((ma - m_ref).abs().max()) <= mtol * max(float(m_ref.abs().max()), 1e-12), name
        if e_ref is not None:
            assert torch.equal(ea, eb)
            assert float((ea - e_ref).abs().max()) <= (1e-3 if name.endswith("bf16") else 1e-5) * float(e_ref.abs().max()), name
    assert torch.equal(o0["allreduce"][0], o0["sharded"][0]) or \
        float((o0["allreduce"][0] - o0["sharded"][0]).abs().max()) <= 1e-6 * scale


# ----------------------------------------------------------------------------------------------
# sharded optimizer state at the module surface: sync_optimizer_state, the collective checkpoint.save, and the loud
# error instead of one rank's shard posing as the whole state (round-2 ADVICE fix; chassis.py:171, checkpoint.py:82-102)
# ----------------------------------------------------------------------------------------------
def _state_worker(rank, world, port, tmpdir, q):
    from tests.plan_emulator import emulate
    from ae_wavenet_amd import _lib as L, autoencoder_model as ae, checkpoint as ckpt, optim
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny("vqvae-ema")
        torch.manual_seed(5)                                       # the same initial weights on every rank
        model = ae.AutoEncoder(hps, n_mel=5)
        eng = emulate(M.TrainEngine(hps, B=1, device="cpu", n_mel=5))
        model._adopt_engine(eng)          # (what _ensure_engine does once it has an engine: it refuses to build one off the GPU)
        d = dp.DataParallel()
        d.attach(model, sharded=True)
        opt = optim.FusedAdam(model, lr=1e-2)
        batch = _global_batch(eng.geom, 5, world)
        eng.set_inputs(*[t[rank:rank + 1] for t in batch])
        n = eng.ps.numel
        for _ in range(2):
            d.train_step_sharded(eng, 1e-2, d.grad_scale(M.MEAN_LOSS[eng.bn_type]))
        # (1) the moments are sharded now: reading optimizer state must fail loudly, on every rank
        raised = False
        try:
            opt.state_dict()
        except L.AewError as e:
            raised = "sync_optimizer_state" in str(e)
        mine_before = eng.adam_m[:n].clone()
        # (2) the collective save: every rank calls it, only rank 0 names a file
        path = os.path.join(tmpdir, "dp.ckpt") if rank == 0 else None
        ckpt.save(path, model, opt, hps, epoch=1, step=2, optim_step=3, with_rng=False)
        # (3) ... after which the state is complete and readable everywhere
        sd = opt.state_dict()
        flat_m = torch.cat([sd["state"][i]["exp_avg"].reshape(-1) for i in range(len(sd["state"]))])
        steps = {float(s["step"]) for s in sd["state"].values()}
        changed = float((eng.adam_m[:n] - mine_before).abs().max())     # the gather filled in the other rank's shards
        # (4) explicit call is idempotent and keeps the state complete across another sync
        d.sync_optimizer_state(model)
        ok_again = torch.equal(eng.adam_m[:n], torch.cat(
            [torch.cat([sd["state"][i]["exp_avg"].reshape(-1), torch.zeros((-sd["state"][i]["exp_avg"].numel()) % 4)])
             for i in range(len(sd["state"]))])[:n])
        q.put((rank, raised, flat_m.numpy().copy(), steps, changed, ok_again, eng.ps.params[:n].numpy().copy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_sharded_optimizer_state_sync_and_collective_checkpoint(tmp_path, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_state_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rk in res[1:-1]:                                          # (world 8: the ranks in between agree with rank 0)
        assert rk[1] and (rk[2] == res[0][2]).all() and (rk[6] == res[0][6]).all() and rk[4] > 0 and rk[5]
    (_, r0, m0, s0, c0, a0, p0), (_, r1, m1, s1, c1, a1, p1) = res[0], res[-1]
    assert r0 and r1                                              # FusedAdam.state_dict() refused the sharded moments
    assert (m0 == m1).all() and (p0 == p1).all()                  # after the sync both ranks hold the same, complete state
    assert s0 == s1 == {2.0}
    assert c0 > 0 and c1 > 0                                      # each rank really was missing the other's shards
    assert a0 and a1
    # the file rank 0 wrote is what the reference's loader reads (checkpoint.py:25-67): stock torch.load, the
    # state dict into a plain module's parameters, torch.optim.Adam.load_state_dict
    f = os.path.join(str(tmp_path), "dp.ckpt")
    assert os.path.exists(f) and len(os.listdir(str(tmp_path))) == 1
    ck = torch.load(f, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["step"] == 2 and ck["optim_step"] == 3
    shapes = [v.shape for k, v in ck["model_state_dict"].items() if not k.startswith("bottleneck.e") and "ind_hist" not in k]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    assert len(params) == len(ck["optim"]["state"])
    adam = torch.optim.Adam(params, lr=1e-4)
    adam.load_state_dict(ck["optim"])
    got = torch.cat([adam.state[p]["exp_avg"].reshape(-1) for p in params]).numpy()
    assert (got == m0).all() and float(abs(got).max()) > 0
    assert all(float(adam.state[p]["step"]) == 2.0 for p in params)


# ----------------------------------------------------------------------------------------------
# the chained launches' sticky timeout word under data parallel: a wait that gave up on ONE rank poisons, through the
# gradient exchange, every rank's gradients - so the guard is MAX-reduced in front of the first gradient collective
# and every rank's optimizer step becomes a no-op (dp.DataParallel._guard_sync; aew_adam_t.guard)
# ----------------------------------------------------------------------------------------------
def _guard_worker(rank, world, port, q):
    from tests.plan_emulator import emulate
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny("vqvae-ema")
        eng = emulate(M.TrainEngine(hps, B=1, device="cpu", n_mel=5))
        # (the CPU engine chains nothing - small launches are refused - so the predicate that says "this engine has chained
        # launches to watch" is forced; the guard word and the ops that read it are the engine's own)
        eng._chain_flag_views = [("chain[forced]", eng.chain_guard[:1])]
        d = dp.DataParallel()
        batch = _global_batch(eng.geom, 5, world)
        mine = [t[rank:rank + 1] for t in batch]
        n = eng.ps.numel
        res = {}
        for name in ("allreduce", "sharded"):
            _seed_engine(eng)
            eng.set_inputs(*mine)
            eng.chain_guard.zero_()
            step = (lambda: d.train_step(eng, 1e-2, 1.0)) if name == "allreduce" else (lambda: d.train_step_sharded(eng, 1e-2, 1.0))
            before = eng.ps.params[:n].clone()
            emb0 = eng.emb.clone()
            if rank == 1:
                eng.chain_guard[0] = 7                             # "stage 6 gave up" - on this rank only
            step()
            d.finish()
            poisoned_same = bool(torch.equal(eng.ps.params[:n], before)) and bool(torch.equal(eng.emb, emb0))
            guard_seen = int(eng.chain_guard[0])
            eng.chain_guard.zero_()                                # re-armed everywhere: the next step trains
            step()
            d.finish()
            res[name] = (poisoned_same, guard_seen, float((eng.ps.params[:n] - before).abs().max()))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_timeout_guard_is_shared_by_all_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, r in res:
        for name, (same, guard, moved) in r.items():
            assert same, (rank, name, "a step poisoned on rank 1 reached the parameters / codebook")
            assert guard == 7, (rank, name, guard)                 # both ranks hold the MAX
            assert moved > 0, (rank, name)                         # and the re-armed step trains again
