#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - parameter groups under the data-parallel schedules, RCCL on ONE GPU (the pattern of
tests/update_ratio_rccl_one_rank.py; started by tests/test_adam_groups_gpu.py in a fresh process).

A process group of one rank over "nccl" and DataParallel(force_collectives=True): FusedAdam(groups=..., max_grad_norm=...,
track_update_ratio=True).step() takes the schedule's own path - range / shard Adam calls with the group record, the clip
norm over the trainable part of the shards and remainders - with every collective really issued.  One rank makes them
identities, so parameters and moments must equal those of the plain engine path (one whole-buffer launch) bit for bit and the
norm up to the summation order.  A small model, two steps.  argv[1]: "allreduce" | "sharded".  Prints one JSON line."""
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, B = 2, 2
MAX_NORM = 1e6          # never reached: the coefficient is 1.0f on both paths, so the parameters can be compared bit for bit
GROUPS = [dict(params=["encoder.*", "bottleneck.*"], frozen=True),
          dict(params="decoder.*.bias", lr=5e-4),
          dict(params="decoder.*", lr=2e-4, weight_decay=0.1)]


def main():
    schedule = sys.argv[1]
    import torch
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0, device_id=dev)
    from ae_wavenet_amd import autoencoder_model as ae, config, model as M, optim
    from ae_wavenet_amd.dp import DataParallel
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "steps": STEPS, "schedule": schedule}

    def run(parallel):
        hps = config.make_hps("vqvae-ema", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, enc_n_out=64, bn_n_out=8,
                              bn_vq_n_embed=64, n_win_batch=96, n_blocks=2, n_block_layers=3, n_global_embed=4, n_speakers=5)
        M.TrainEngine.merge_packs = False if parallel else None    # (the plans of a real data-parallel rank)
        torch.manual_seed(11)
        model = ae.AutoEncoder(hps, n_mel=39).to(dev)
        opt = optim.FusedAdam(model, lr=1e-3, max_grad_norm=MAX_NORM, track_update_ratio=True, groups=GROUPS)
        eng = model._ensure_engine(B)
        calls = [0]
        if parallel:
            dp = DataParallel(force_collectives=True)
            dp.attach(model, sharded=schedule == "sharded")
            dp.broadcast_params(eng)
            inner = eng.adam_step

            def counted(*a, **kw):
                calls[0] += 1
                assert kw.get("groups") is not None
                return inner(*a, **kw)
            eng.adam_step = counted
        n = eng.ps.numel
        start = eng.ps.params[:n].clone()
        g = model.geom
        gen = torch.Generator().manual_seed(77)
        norms = []
        for i in range(STEPS):
            wav = torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(dev)
            mel = torch.randn(B, 39, g.mel_len, generator=gen).to(dev)
            voice = torch.randint(0, 5, (B,), generator=gen).to(dev)
            jitter = torch.arange(g.embed_len).repeat(B, 1).to(dev)
            opt.zero_grad()
            _, _, loss = model.run(wav, mel, voice, jitter)
            loss.backward()
            opt.step()
            norms.append([float(opt.grad_norm), float(opt.clip_coef)])
        if parallel:
            dp.sync_optimizer_state(model)
            dp.finish()
        torch.cuda.synchronize()
        frozen = [k for k in eng.ps.names() if k.startswith(("encoder.", "bottleneck."))]
        still = all(torch.equal(eng.ps.view(k), start[eng.ps.off[k]:eng.ps.off[k] + eng.ps.numel_of(k)].view(eng.ps.shape[k]))
                    for k in frozen)
        state = {"params": eng.ps.params[:n].clone(), "m": eng.adam_m[:n].clone(), "v": eng.adam_v[:n].clone()}
        M.TrainEngine.merge_packs = None
        return state, norms, calls[0], still, bool(not torch.equal(state["params"], start)), len(frozen)

    ref, ref_norms, _, ref_still, ref_moved, n_frozen = run(False)
    got, got_norms, calls, still, moved, _ = run(True)
    out["adam_calls"] = calls
    out["frozen_tensors"], out["frozen_still"], out["moved"] = n_frozen, bool(still and ref_still), bool(moved and ref_moved)
    out["norm_rel"] = max(abs(a[0] / b[0] - 1) for a, b in zip(got_norms, ref_norms))
    out["coef_rel"] = max(abs(a[1] / b[1] - 1) for a, b in zip(got_norms, ref_norms))
    out["coefs"] = [a[1] for a in got_norms]
    out["bit_equal"] = {k: bool(torch.equal(got[k], ref[k])) for k in ref}
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
