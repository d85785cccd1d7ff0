"""Configurations of the training-step plan recording (tests/data/plan_parent.json) and its generator.

The recording pins what TrainEngine built at the commit BEFORE DecoderPlan.build_backward was restructured around one
weight-gradient router: for every configuration below, every plan of an engine built on device "cpu" in a canonical
form.  Per op, in order: label, kind, tag, lane, join and every payload field; every address inside a workspace buffer
as [buffer name, element offset]; the tables an op points to (copy-table records and block map, TN-group descriptors,
tile map and cursor words, the speaker ops' offset tables, chain stage tables and block maps) in the same form and in
record order.  Plus the ordered list of workspace allocations (name, elements, dtype).  The file holds one line per op -
label and a digest of its canonical form - and one digest per configuration for the allocation list; plans shared by
several configurations are stored once, and a plan whose ops are a slice of another plan's (bwd_a1 / bwd_a2 / bwd_b of
bwd, fwd_b_noema / ema of fwd_b) as [plan, start, stop].  The weight-pack plans are spliced into fwd_a / fwd_b by the
engine and are recorded there.

The configurations of late_configs() also pin the plans that the optimizer stage of TrainEngine._build and the lazily
completed state make (LATE_PLANS: opt, clip, ratio, swap, restart, the evaluation plans, the encode and conditioning sub-plans), as
built at the commit BEFORE the plan builder was split into stages and BottleneckPlan: after the record above is taken,
complete() finishes that state on the "cpu" engine (nothing runs), and the same canonical form goes under the keys
"late" and "alloc_late" (the allocation list once more, with the buffers the completion added).

    python tests/data/plan_gen.py            # rewrites plan_parent.json - ONLY from the commit the recording pins

tests/test_plan_parent_cpu.py rebuilds the engines and compares; on a mismatch it prints canon_op() of the first
differing op, to be diffed against `python tests/data/plan_gen.py CONFIG PLAN INDEX` run at the pinned commit.
"""
import bisect
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ae_wavenet_amd import _lib as L, config, engine as E, model as M      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "plan_parent.json")
GOLDEN = os.path.join(os.path.dirname(HERE), "golden")
MODELS = {"mi": ("mi_tiny_jitter.npz", "mfcc_inverter", 7), "vqvae-ema": ("ae_tiny_vqvae-ema_random.npz", "autoencoder", None),
          "vae": ("ae_tiny_vae_random.npz", "autoencoder", None), "ae": ("ae_tiny_ae_identity.npz", "autoencoder", None),
          "vqvae": ("ae_tiny_vqvae_identity.npz", "autoencoder", None)}
PLANS = ("fwd_a", "fwd_b", "bwd", "bwd_a", "bwd_a1", "bwd_a2", "bwd_b", "cb", "fwd_b_noema", "ema_plan")
# name in the recording -> attribute of the engine
LATE_PLANS = {"opt": "opt", "clip": "clip", "ratio": "ratio", "swap": "swap", "restart": "restart", "eval_a": "eval_a",
              "eval_b": "eval_b", "eval_fin": "eval_fin", "encode": "_encode_plan", "conditioning_a": "_cond_plan_a",
              "conditioning": "_cond_plan"}
FN_ALL = frozenset(("layer", "G1", "dx", "dz", "skip", "dcond", "post"))
FOLD_ROWS = 4096                                                        # the library's default (aew_set_tn_fold_rows)


def configs():
    """name -> dict(model=, dec= DecoderPlan attributes, eng= TrainEngine attributes, env=, fold_rows=, hps= overrides,
    kw= constructor arguments, half_group= wgrad_group = layers // 2)."""
    out = {}
    for m in MODELS:
        out[f"default.{m}"] = dict(model=m)
    for m in ("mi", "vqvae-ema"):
        out[f"group0.{m}"] = dict(model=m, dec=dict(wgrad_group=0))
        out[f"group0_unfolded.{m}"] = dict(model=m, dec=dict(wgrad_group=0), fold_rows=0)     # the column-R colsum table
        out[f"dp.{m}"] = dict(model=m, half_group=True, eng=dict(merge_packs=False))          # bwd_a1 / bwd_a2
        out[f"impl1.{m}"] = dict(model=m, kw=dict(impl=1))
    for g, s, t in ((64, 0, 256), (64, 0, 128), (8, 0, 256), (3, 0, 128), (1, 0, 256), (64, 3, 256)):
        out[f"grouped_{g}_{s}_{t}.mi"] = dict(model="mi", dec=dict(wgrad_group=g, wgrad_split_layers=s, wgrad_tile=t))
    out["chains.mi"] = dict(model="mi", dec=dict(split_chains=True, split_chains_bwd=True))
    out["chains_one_lane.mi"] = dict(model="mi", dec=dict(split_chains=True, split_chains_bwd=True, split_one_lane=True))
    out["tail.mi"] = dict(model="mi", dec=dict(tail_lane=4))
    out["tail_cursor.mi"] = dict(model="mi", dec=dict(tail_lane=4, wgrad_cursor=True))
    out["tail.vqvae-ema"] = dict(model="vqvae-ema", dec=dict(tail_lane=4))
    for m in ("mi", "vqvae-ema"):
        out[f"multiseg.{m}"] = dict(model=m, dec=dict(split_multiseg=True))
    for n in (1, 2):
        out[f"lanes{n}.mi"] = dict(model="mi", dec=dict(n_side_lanes=n))
        out[f"lanes{n}_group0.vqvae-ema"] = dict(model="vqvae-ema", dec=dict(n_side_lanes=n, wgrad_group=0))
    out["side_inputs_late.mi"] = dict(model="mi", dec=dict(side_inputs_first=False))
    # (the shape tests/test_plan_cpu.py::test_split_grouped_descriptor_keeps_its_bias_gradient builds)
    small = dict(n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=3, n_blocks=1, n_block_layers=2,
                 n_win_batch=2500, n_lc_in=4)
    for grp in (64, 0):
        out[f"ups_split_{grp}"] = dict(make=("mi", small), B=3, n_mel=4, dec=dict(ups_split_rows=16), kw=dict(wgrad_group=grp))
    out["fn_ops.mi"] = dict(model="mi", dec=dict(fn_ops=FN_ALL))
    out["nobias.mi"] = dict(model="mi", hps=dict(bias=False))
    out["nobias_group0.mi"] = dict(model="mi", hps=dict(bias=False), dec=dict(wgrad_group=0))
    # (combinations whose rules meet in the weight-gradient routing)
    out["dp_tail_cursor.mi"] = dict(model="mi", half_group=True, dec=dict(tail_lane=4, wgrad_cursor=True), eng=dict(merge_packs=False))
    out["dp_chains.mi"] = dict(model="mi", half_group=True, dec=dict(split_chains=True, split_chains_bwd=True))
    out["multiseg_group0.mi"] = dict(model="mi", dec=dict(split_multiseg=True, wgrad_group=0))
    out["multiseg_chains.mi"] = dict(model="mi", dec=dict(split_multiseg=True, split_chains=True, split_chains_bwd=True))
    out["split_layers_tail.mi"] = dict(model="mi", dec=dict(wgrad_split_layers=2, tail_lane=4, n_side_lanes=3))
    out["nt_chain_2_2.mi"] = dict(model="mi", env=dict(AEW_NT_CHAIN="2,2"))
    out["nt_chain_2_2_forced.mi"] = dict(model="mi", env=dict(AEW_NT_CHAIN="2,2"), eng=dict(nt_chain_force=True))
    return out


@contextlib.contextmanager
def applied(cfg):
    """Class attributes, environment and the fold-rows switch of a configuration, restored afterwards."""
    saved = [(cls, k, cls.__dict__.get(k, cls)) for cls, kv in ((E.DecoderPlan, cfg.get("dec", {})), (M.TrainEngine, cfg.get("eng", {})))
             for k in kv]
    env = {k: os.environ.get(k) for k in ("AEW_NT_CHAIN", "AEW_FN_OPS", "AEW_WGRAD_GROUP")}
    try:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(cfg.get("env", {}))
        for cls, kv in ((E.DecoderPlan, cfg.get("dec", {})), (M.TrainEngine, cfg.get("eng", {}))):
            for k, v in kv.items():
                setattr(cls, k, v)
        if "fold_rows" in cfg:
            L.load().aew_set_tn_fold_rows(cfg["fold_rows"])
        yield
    finally:
        if "fold_rows" in cfg:
            L.load().aew_set_tn_fold_rows(FOLD_ROWS)
        for cls, k, v in saved:
            delattr(cls, k) if v is cls else setattr(cls, k, v)
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def late_configs():
    return [n for n in configs() if n.startswith(("default.", "dp."))]


def build(cfg):
    """The engine of a configuration, on device "cpu" (plans only)."""
    with applied(cfg):
        if "make" in cfg:
            hps, B, n_mel, kind = config.make_hps(cfg["make"][0], **cfg["make"][1]), cfg["B"], cfg["n_mel"], None
        else:
            fixture, kind, n_mel = MODELS[cfg["model"]]
            z = np.load(os.path.join(GOLDEN, fixture), allow_pickle=False)
            h = json.loads(str(z["hps_json"]))
            n_mel = n_mel or h.pop("n_mel_ch", None)
            h.pop("n_mel_ch", None)
            over = dict(cfg.get("hps", {}), global_model=kind)
            hps, B = config.make_hps(**{k: v for k, v in h.items() if k not in over}, **over), z["wav"].shape[0]
        kw = dict(cfg.get("kw", {}))
        if cfg.get("half_group"):
            kw["wgrad_group"] = hps.n_blocks * hps.n_block_layers // 2
        return M.TrainEngine(hps, B=B, device="cpu", n_mel=n_mel, take_compat=True, update_codebook_every_step=False, **kw)


class Resolver:
    """Workspace.resolve (the buffer that holds an address, element offset) over a sorted table of the buffers."""

    def __init__(self, ws):
        self.ws = ws
        self.tab = sorted((t.data_ptr(), t.numel() * t.element_size(), n) for n, t in ws.bufs.items())
        self.starts = [r[0] for r in self.tab]

    def __call__(self, addr):
        if not addr:
            return 0
        i = bisect.bisect_right(self.starts, addr) - 1
        if i >= 0 and addr <= self.tab[i][0] + self.tab[i][1]:           # (<=: one past the end is an address of the buffer too)
            p, _, n = self.tab[i]
            return [n, (addr - p) // self.ws.bufs[n].element_size()]
        raise KeyError(f"address {addr:#x} is not inside any workspace buffer")


def canon(obj, R):
    """Canonical form of a ctypes value: structures as [[field, value], ...], pointers through the resolver R."""
    if isinstance(obj, C.Structure):
        out = []
        for name, typ in obj._fields_:
            v = getattr(obj, name)
            out.append([name, R(v) if typ is C.c_void_p else canon(v, R)])
        return out
    if isinstance(obj, C.Array):
        return [R(v) for v in obj] if obj._type_ is C.c_void_p else [canon(v, R) for v in obj]
    if isinstance(obj, float):
        return repr(obj)
    if isinstance(obj, bytes):
        return obj.decode()
    return obj


def table(typ, addr, n):
    """n elements of ctypes type `typ` at host address addr (the workspace of a "cpu" engine is host memory)."""
    return (typ * n).from_buffer_copy(C.string_at(addr, n * C.sizeof(typ))) if addr and n > 0 else []


def canon_op(eng, plan, i, R=None):
    """Field-level canonical form of op i of a plan: head, payload, and the tables it points to."""
    R = R or Resolver(eng.ws)
    op, lab = plan.ops[i], plan.labels[i]
    u = getattr(op.u, L.OP_FIELD[op.kind])
    out = dict(label=lab, kind=op.kind, tag=op.tag, lane=op.lane, join=op.join, payload=canon(u, R))
    if op.kind == L.OP_COPY_TABLE:
        out["recs"] = [canon(r, R) for r in table(L.CopyRec, u.recs, u.n_recs)]
        out["block_rec"] = list(table(C.c_int32, u.block_rec, u.n_blocks))
    elif op.kind == L.OP_GEMM_TN_GROUP:
        out["descs"] = [canon(d, R) for d in table(L.GemmTN, u.descs, u.n_descs)]
        out["tile_map"] = list(table(C.c_int32, u.tile_map, u.n_blocks))
        out["cursors"] = list(table(C.c_int32, u.cursors, u.n_descs * u.cursor_stride))
    elif op.kind in (L.OP_SPK_BIAS, L.OP_SPK_BWD):
        for f in ("off_bias_sig", "off_bias_gate", "off_proj_sig", "off_proj_gate"):
            out[f] = list(table(C.c_int64, getattr(u, f), u.L))
    elif op.kind == L.OP_NT_CHAIN:
        out["stages"] = [canon(s, R) for s in table(L.NtStage, u.stages, u.n_stages)]
        name, off = R(u.block_stage)
        out["block_stage"] = eng.ws.bufs[name][off:].tolist()
    return out


def digest(v):
    return hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).hexdigest()[:10]


def allocations(eng):
    return [[n, t.numel(), str(t.dtype)] for n, t in eng.ws.bufs.items()]


def complete(eng):
    """Everything an engine builds at first use, without running a plan: the evaluation plans, the average and its swap
    op, the restart op, the encode and the conditioning sub-plans."""
    eng._run = lambda *a, **k: None
    eng.eval_plans()
    eng._avg_buffer()
    if getattr(eng, "cb", None) is not None:                             # (vqvae-ema)
        eng._restart_op()
    if eng.enc is not None:
        eng.encode()
    eng.conditioning()


def _lines(eng, names, plans, ops_of):
    """plans[name] for the plans `names` (name -> attribute) of the engine; ops_of: the op ids of plans stored in full."""
    R = Resolver(eng.ws)
    for nm, attr in names.items():
        plan = getattr(eng, attr, None)
        if plan is None:
            continue
        ids = [id(op) for op in plan.ops]
        for whole, wids in ops_of.items():                               # a slice of a plan already recorded
            at = wids.index(ids[0]) if ids and ids[0] in wids else -1
            if ids and at >= 0 and wids[at:at + len(ids)] == ids:
                plans[nm] = [whole, at, at + len(ids)]
                break
        else:
            plans[nm] = [[lab, digest(canon_op(eng, plan, i, R))] for i, lab in enumerate(plan.labels)]
            ops_of[nm] = ids
    return plans


def record(eng, late=False):
    """(allocation digest, {plan: [[label, digest], ...] or [plan, start, stop]}) of an engine; late=True: the same pair
    once more behind it, for LATE_PLANS after complete()."""
    alloc, ops_of = digest(allocations(eng)), {}
    plans = _lines(eng, {nm: nm for nm in PLANS}, {}, ops_of)
    if not late:
        return alloc, plans
    complete(eng)
    return alloc, plans, digest(allocations(eng)), _lines(eng, LATE_PLANS, {}, ops_of)


def main():
    cfgs = configs()
    pool, out = {}, {}
    for name, cfg in cfgs.items():
        rec = record(build(cfg), late=name in late_configs())
        out[name] = {}
        for key_a, key_p, alloc, plans in zip(("alloc", "alloc_late"), ("plans", "late"), rec[0::2], rec[1::2]):
            ent = {}
            for nm, lines in plans.items():
                if lines and isinstance(lines[0], list):
                    key = digest(lines)
                    pool[key] = lines
                    ent[nm] = key
                else:
                    ent[nm] = lines
            out[name].update({key_a: alloc, key_p: ent})
    with open(TABLE, "w") as f:
        f.write('{"configs": {\n')
        f.write(",\n".join(f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()))
        f.write('\n},\n"plans": {\n')
        f.write(",\n".join(f' {json.dumps(k)}: [\n' + ",\n".join(json.dumps(l, separators=(",", ":")) for l in lines) + "]"
                           for k, lines in pool.items()))
        f.write("\n}}\n")
    print(f"{len(out)} configurations, {len(pool)} plans, {sum(len(v) for v in pool.values())} ops, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    if len(sys.argv) == 4:                                               # CONFIG PLAN INDEX: one op, field by field
        eng = build(configs()[sys.argv[1]])
        if sys.argv[2] in LATE_PLANS:
            complete(eng)
        print(json.dumps(canon_op(eng, getattr(eng, LATE_PLANS.get(sys.argv[2], sys.argv[2])), int(sys.argv[3])), indent=1))
    else:
        main()
