"""Cases of the TN (weight-gradient) launch table (tests/data/tn_pick_parent.json) and its generator.

The table records what launch_gemm_tn and launch_gemm_tn_group of the commit BEFORE the TN launchers got their pick
launched for a sweep of tuning records x descriptors: kernel instantiation, grid, threads, dynamic LDS bytes, the plan
arguments the kernel was handed (splits, rows per split, fold | cursor stride, epoch, slack) and the return code, plus
aew_tn_slabs, aew_tn_fold and aew_tn_group_check.  It was recorded on a CPU from a host-only build of that commit whose
launch macro stored its arguments instead of launching (`int aew_rec_tn(const aew_gemm_tn_t*, rec_t out[], int cap,
int* n)`, `aew_rec_tn_group(const aew_gemm_tn_group_t*, ...)`, rec_t = {char name[96]; int grid[3], threads, lds,
arg[3]}).  tests/test_tn_pick_cpu.py rebuilds every descriptor with `descriptor()` / `group()` below and asks
aew_tn_pick / aew_tn_group_pick.

    python tests/data/tn_pick_gen.py /path/to/recording_library.so          # rewrites tn_pick_parent.json

The sweep is THINNED to the table's size limit: every descriptor is kept under the default record; under each other record only
the first and the last case of every distinct answer up to the grid and the rows per split (see main(), relevant()), so a
middle case of such a class is not compared.

No pointer is dereferenced by the host logic, so the descriptors point into a made-up address space.
"""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from ae_wavenet_amd import _lib as L                                    # noqa: E402
from ae_wavenet_amd.plan import Mat, make_tn                             # noqa: E402
from nt_pick_gen import AddrSpace, clean, set_tuning                     # noqa: E402

TABLE = os.path.join(HERE, "tn_pick_parent.json")
CASE_KEYS = ("dt", "impl", "Mc", "B", "Np", "ks", "bad")
GROUP_KEYS = ("tile", "cursors", "stride", "n_blocks", "descs")
SEGS = ((128,), (128, 128, 256), (384, 384, 128))
BAD = ("misalign", "klen", "ksum", "npad", "segs0", "segs33", "noout")
# grouped-only defects (aew_tn_group_check): the snap_k range, each grp_splits / grp_rows rule, more than 0xfff tiles
GROUP_BAD = ("snap_hi", "snap_lo", "snap_ok", "splits_neg", "splits_many", "rows0", "rows_odd", "rows_short", "split_snap",
             "split_colsum", "split_ok", "tiles")


def tunings():
    """Each TN field alone, the cursor pairs, then the records test_tuned_record_cannot_change_a_built_split_k_plan runs."""
    out = [{}, dict(tn_safe=1)]
    out += [dict(tn_big=b, tn_big_target=t) for b in (0, 1) for t in (0, 64)]
    out += [dict(tn_fold_rows=v) for v in (0, 1000, 1 << 20)] + [dict(tn_target_blocks=v) for v in (8, 2048)]
    out += [dict(tn_small_tiles=v) for v in (0, 64)] + [dict(tn_small_target=v) for v in (8, 256)]
    out += [dict(tn_mfma32=1)] + [dict(tn_cursor_epoch=e, tn_cursor_slack=d) for e, d in ((-1, 0), (0, 0), (3, 1), (4, 2))]
    out += [dict(tn_target_blocks=4 * 512, tn_fold_rows=1 << 20), dict(tn_target_blocks=8, tn_small_tiles=64, tn_small_target=8),
            dict(tn_big=1, tn_big_target=64)]
    uniq = []
    for t in out:
        if t not in uniq:
            uniq.append(t)
    return uniq


def cases():
    out = [dict(dt=dt, impl=impl, Mc=Mc, B=B, Np=Np, ks=ks, bad="")
           for dt, impl, Mc, B, Np, ks in itertools.product((L.BF16, L.F32), (0, 1), (1, 33, 777, 2500, 5000, 268000), (1, 3, 8),
                                                            (128, 256, 384, 640), range(len(SEGS)))]
    c0 = dict(impl=0, Mc=777, B=3, Np=256, ks=1)
    out += [dict(c0, dt=dt, bad=bad) for dt in (L.BF16, L.F32) for bad in BAD]
    out += [dict(c0, dt=L.BF16, bad=bad) for bad in GROUP_BAD]
    return out


def descriptor(c, sp=None):
    """The aew_gemm_tn_t of case c, its buffers in address space sp (a fresh one by default)."""
    sp = sp or AddrSpace()
    dt, Mc, B, Np = c["dt"], c["Mc"], c["B"], c["Np"]
    n = len(sp.addr)
    G, A = Mat.new(sp, f"G{n}", B, Mc + 43, 8320, dt), Mat.new(sp, f"A{n}", B, Mc + 43, 8320, dt)
    sp.alloc(f"o{n}", 64, 0)
    t = make_tn(dt, Mc, B, Np - 8, Np, G.seg(Np, row_off=3), [A.seg(k, row_off=i, col_off=384 * i) for i, k in enumerate(SEGS[c["ks"]])],
                impl=c["impl"])
    t.out, t.out_batch_stride = sp.ptr(f"o{n}"), Np * t.K_total
    bad, other = c["bad"], sp.ptr(f"o{n}") + 4096
    if bad == "misalign":
        t.seg[0].ptr += 8
    elif bad == "klen":
        t.seg[0].k_len += 32
        t.K_total += 32
    elif bad == "ksum":
        t.K_total += 128
    elif bad == "npad":
        t.N_pad += 32
    elif bad == "segs0":
        t.n_segs = 0
    elif bad == "segs33":
        t.n_segs = 33
    elif bad == "noout":
        t.out = None
    elif bad in ("snap_hi", "snap_lo", "snap_ok"):
        t.snap_out, t.snap_bs, t.snap_k = other, Np, dict(snap_hi=t.K_total, snap_lo=-2, snap_ok=t.K_total - 1)[bad]
    elif bad == "splits_neg":
        t.grp_splits = -1
    elif bad == "splits_many":
        t.grp_splits, t.grp_rows = 342, 32                               # x 3 batch elements: 1026 chunks > 0x3ff
    elif bad in ("rows0", "rows_odd", "rows_short", "split_ok", "split_snap", "split_colsum"):
        t.grp_splits, t.grp_rows = 4, dict(rows0=0, rows_odd=200, rows_short=192).get(bad, 224)
        if bad == "split_snap":
            t.snap_out, t.snap_bs, t.snap_k = other, Np, 0
        if bad == "split_colsum":
            t.colsum_out = other
    elif bad == "tiles":                                                 # 64 x 65 tiles of 128 x 128
        t.N_pad, t.g.k_len, t.seg[1].k_len, t.K_total = 8192, 8192, 128 + 8320 - 512, 8320
    return t


def group_cases():
    return [dict(tile=tile, cursors=cur, stride=stride, n_blocks=nb, descs=descs)
            for tile, cur, stride in itertools.product((128, 256, 384, 100), (0, 1), (0, 64))
            for nb, descs in ((24, 1), (0, 1), (24, 0)) if descs or (cur, stride) == (0, 0)]


def group(c):
    p = L.GemmTNGroup()
    p.descs, p.tile_map, p.n_descs, p.n_blocks = (1 << 32) if c["descs"] else None, 1 << 33, 3, c["n_blocks"]
    p.tile, p.cursor_stride, p.cursors = c["tile"], c["stride"], (1 << 34) if c["cursors"] else None
    return p


class Rec(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("grid", C.c_int * 3), ("threads", C.c_int), ("lds", C.c_int), ("arg", C.c_int * 3)]


def relevant(over, c):
    """Records a stand-alone case is recorded under: none of them reads the grouped launch's fields; fp32 ops and the check
    kernel do not read tn_safe.  The check kernel (the plan of the kernel it checks, one thread per element) is thinned
    to one batch size outside the default record."""
    keys = set(over)
    if keys & {"tn_mfma32", "tn_cursor_epoch", "tn_cursor_slack"} or (keys and c["impl"] == 1 and c["B"] != 3):
        return False
    return not (keys == {"tn_safe"} and (c["dt"] == L.F32 or c["impl"] == 1))


def main(path):
    lib = C.CDLL(path)
    cs, gcs, tus = cases(), group_cases(), tunings()
    descs = [descriptor(c) for c in cs]
    out, n = (Rec * 4)(), C.c_int()
    names, rows, grows = {}, [], []

    def launch(rc):
        assert n.value == (1 if rc == 0 else 0), (rc, n.value)
        r = out[0]
        return [names.setdefault(clean(r.name.decode()), len(names)), *r.grid, r.threads, r.lds, *r.arg] if rc == 0 else []

    for ti, over in enumerate(tus):
        set_tuning(lib, over)
        chosen = {}
        for ci, (c, g) in enumerate(zip(cs, descs)):
            if not relevant(over, c):
                continue
            rc = lib.aew_rec_tn(C.byref(g), out, 4, C.byref(n))
            la = launch(rc)
            row = [ti, ci, rc, la, lib.aew_tn_slabs(C.byref(g)), lib.aew_tn_fold(C.byref(g))]
            # Kept: every case under the default record; under the others, per distinct answer up to the grid and the rows
            # per split (kernel, block, LDS, splits, fold, slabs) the first and the last case
            key = (rc, tuple(la[:1] + la[4:7] + la[8:]), row[4]) if ti else ci
            chosen.setdefault(key, [row, row])[1] = row
        rows += sorted({(r[0], r[1]): r for pair in chosen.values() for r in pair}.values())
        if ti == 0 or set(over) & {"tn_safe", "tn_mfma32", "tn_cursor_epoch", "tn_big"}:
            for gi, c in enumerate(gcs):
                p = group(c)
                rc = lib.aew_rec_tn_group(C.byref(p), out, 4, C.byref(n))
                grows.append([ti, gi, rc, launch(rc)])
    set_tuning(lib, {})
    checks = [lib.aew_tn_group_check(C.byref(g)) for g in descs]
    with open(TABLE, "w") as f:
        f.write('{"case_keys": %s,\n "group_keys": %s,\n "tunings": %s,\n "kernels": %s,\n "cases": %s,\n "group_cases": %s,\n'
                ' "group_check": %s,\n "group_rows": %s,\n "rows": [\n'
                % (json.dumps(CASE_KEYS), json.dumps(GROUP_KEYS), json.dumps(tus), json.dumps(list(names)),
                   json.dumps([[c[k] for k in CASE_KEYS] for c in cs], separators=(",", ":")),
                   json.dumps([[c[k] for k in GROUP_KEYS] for c in gcs], separators=(",", ":")),
                   json.dumps(checks, separators=(",", ":")), json.dumps(grows, separators=(",", ":"))))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} rows, {len(grows)} group rows, {len(cs)} cases, {len(names)} kernel instantiations, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
