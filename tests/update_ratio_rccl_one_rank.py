#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - update / weight ratios under the sharded data-parallel step, RCCL on ONE GPU (the pattern of
tools/dp_rccl_clip_one_rank.py; started by tests/test_update_ratio_gpu.py in a fresh process).

A process group of one rank over "nccl" and DataParallel(force_collectives=True): FusedAdam(track_update_ratio=True)
.step() then takes dp.optimizer_step - shard Adam calls with the tracking record, the remainder calls on rank 0, the
finalize = 0 launch, the all-reduce of the 2 P fp64 words, the finalize = 1 launch that reads those words alone - with
every collective really issued.  One rank makes them identities, so norms and ratios must equal those of the plain engine
path (one whole-buffer launch) up to the summation order, and parameters and moments bit for bit.  A small model, two
steps.  Prints one JSON line."""
import json
import math
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, B = 2, 2


def main():
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
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "steps": STEPS, "ratio_launches": {},
           "collectives": {"all_reduce_2P_f64": 0}}
    real_all_reduce = dist.all_reduce
    n_tensors = [0]

    def counting_all_reduce(t, *a, **kw):
        if t.dtype == torch.float64 and t.numel() == 2 * n_tensors[0]:
            out["collectives"]["all_reduce_2P_f64"] += 1
        return real_all_reduce(t, *a, **kw)

    def run(sharded):
        hps = config.make_hps("vqvae-ema", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, enc_n_out=64, bn_n_out=8,
                              bn_vq_n_embed=64, n_win_batch=96, n_blocks=2, n_block_layers=3, n_global_embed=4, n_speakers=5)
        M.TrainEngine.merge_packs = False if sharded else None     # (the plans of a real data-parallel rank)
        torch.manual_seed(11)
        model = ae.AutoEncoder(hps, n_mel=39).to(dev)
        opt = optim.FusedAdam(model, lr=1e-3, track_update_ratio=True)
        eng = model._ensure_engine(B)
        n_tensors[0] = eng.uw_n
        dp = None
        if sharded:
            dp = DataParallel(force_collectives=True)
            dp.attach(model, sharded=True)
            dp.broadcast_params(eng)
        launches = [0]
        inner = eng.ratio_step

        def counted(*a, **kw):
            launches[0] += 1
            return inner(*a, **kw)
        eng.ratio_step = counted
        g = model.geom
        gen = torch.Generator().manual_seed(77)
        words = []
        for i in range(STEPS):
            wav = torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(dev)
            mel = torch.randn(B, 39, g.mel_len, generator=gen).to(dev)
            voice = torch.randint(0, 5, (B,), generator=gen).to(dev)
            jitter = torch.arange(g.embed_len).repeat(B, 1).to(dev)
            opt.zero_grad()
            _, _, loss = model.run(wav, mel, voice, jitter)
            loss.backward()
            opt.step()
            words.append(eng.update_ratios().double().cpu().clone())
        if dp is not None:
            dp.sync_optimizer_state(model)
        torch.cuda.synchronize()
        n = eng.ps.numel
        out["ratio_launches"]["sharded" if sharded else "engine"] = launches[0]
        state = {"params": eng.ps.params[:n].clone(), "m": eng.adam_m[:n].clone(), "v": eng.adam_v[:n].clone()}
        M.TrainEngine.merge_packs = None
        return state, words

    ref, ref_words = run(False)
    dist.all_reduce = counting_all_reduce
    try:
        got, got_words = run(True)
    finally:
        dist.all_reduce = real_all_reduce
    rel = {"update_norm": 0.0, "weight_norm": 0.0, "ratio": 0.0}
    same_class, finite = True, 0
    for a, b in zip(got_words, ref_words):
        for row, key in enumerate(rel):
            for x, y in zip(a[row].tolist(), b[row].tolist()):
                if math.isfinite(y) and y != 0.0:
                    rel[key] = max(rel[key], abs(x / y - 1))
                    finite += row == 2
                else:
                    same_class = same_class and ((x == y) or (math.isnan(x) and math.isnan(y)))
    out["tensors"], out["finite"] = n_tensors[0], finite // STEPS
    out["max_rel"], out["same_class"] = rel, same_class
    out["bit_equal"] = {k: bool(torch.equal(got[k], ref[k])) for k in ref}
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
