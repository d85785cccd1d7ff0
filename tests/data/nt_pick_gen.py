"""Cases of the NT kernel-selection table (tests/data/nt_pick_parent.json) and its generator.

The table records what launch_gemm_nt of the commit BEFORE the selector refactor launched for a sweep of tuning
records x descriptors: kernel instantiation, grid.x, threads, dynamic LDS bytes and the return code, plus
aew_gemm_nt_small_split's outputs and aew_nt_chain_build's accept / reject code for a two-stage chain.  It was
recorded on a CPU from a host-only build of that commit whose launch macro stored its arguments instead of launching
(`int aew_rec_nt(const aew_gemm_nt_t*, rec_t out[], int cap, int* n)`, rec_t = {char name[96]; int grid, threads,
lds}).  tests/test_nt_pick_cpu.py rebuilds every descriptor with `descriptor()` below and asks aew_nt_pick.

    python tests/data/nt_pick_gen.py /path/to/recording_library.so          # rewrites nt_pick_parent.json

No pointer is dereferenced by the host logic, so the descriptors point into a made-up address space.
"""
import ctypes as C
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ae_wavenet_amd import _lib as L                                    # noqa: E402
from ae_wavenet_amd.plan import Mat, Workspace, make_nt                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "nt_pick_parent.json")
ZERO_SPAN = 16384
CASE_KEYS = ("dt", "epi", "M", "B", "Np", "K", "seg", "impl", "w2", "ks", "nsplit", "bad")


class AddrSpace(Workspace):
    """A workspace of addresses only: 256-byte aligned ranges that never overlap, no memory behind them."""

    def __init__(self):
        super().__init__("cpu")
        self.addr, self.next = {}, 1 << 32

    def alloc(self, name, numel, dtype, zero=True):
        self.addr[name] = self.next
        self.next += (int(numel) * 4 + 4096 + 255) // 256 * 256

    def ptr(self, name, off=0):
        return self.addr[name] + off * 2


def tunings():
    """Each NT field alone over the values its setter accepts, then the combinations tests/test_gpu_parity.py runs."""
    single = dict(nt_wave_rows=(0, 1, 64, 128, 256, 512), nt_pipe=(0, 1, 2), nt_rows192=(0, 1, 2), nt_small_tiles=(0, 128),
                  nt_mem128=(0, 1, 2), nt_deep=(0, 1, 2, 3), nt_small_w8=(0, 1), nt_small_deep=(0, 256), nt_small_n64=(0, 128, 256),
                  nt_window=(0, 8, 64), nf_deep=(0, 256), nf_loaders=(0, 1), fn_enable=(0, 1), fn_ring3=(0, 4, 16))
    out = [{}]
    for k, vs in single.items():
        out += [{k: v} for v in vs]
    for shape, pipe, small in ((64, 1, 0), (64, 1, 128), (64, 1, -1), (0, 1, 0), (1, 1, 0), (128, 1, 0), (128, 0, 0), (256, 0, 0),
                               (256, 1, 0), (256, 2, 0), (512, 1, 0)):
        out.append(dict(nt_rows192=2 if small < 0 else 0, nt_wave_rows=shape, nt_pipe=pipe, nt_small_tiles=max(small, 0)))
    for waves, deep, nf_deep, nf_ld, n64 in ((8, 256, 256, 1, 128), (8, 256, 256, 1, 0), (2, 256, 0, 1, 128), (2, 0, 256, 0, 0),
                                             (8, 256, 0, 0, 0)):
        out.append(dict(nt_rows192=0, nt_small_w8=int(waves >= 8), nt_small_deep=deep, nf_deep=nf_deep, nf_loaders=nf_ld,
                        nt_small_n64=n64))
    for mode, deep in ((1, 0), (2, 0), (0, 1), (0, 2), (0, 3)):
        out.append(dict(nt_small_tiles=0, nt_mem128=mode, nt_deep=deep))
    out += [dict(nt_rows192=2, nt_small_tiles=0), dict(nt_wave_rows=256, nt_pipe=0), dict(nt_rows192=2, nt_window=0),
            dict(nt_deep=1, nt_window=0), dict(nt_wave_rows=512, nt_small_tiles=0)]
    default = dict(nt_wave_rows=64, nt_pipe=1, nt_rows192=1, nt_small_tiles=128, nt_mem128=0, nt_deep=0, nt_small_w8=1,
                   nt_small_deep=256, nt_small_n64=256, nt_window=64, nf_deep=256, nf_loaders=1, fn_enable=1, fn_ring3=16)
    seen, uniq = set(), []
    for t in out:
        key = tuple(sorted((k, v) for k, v in t.items() if default[k] != v))
        if key not in seen:
            seen.add(key)
            uniq.append(t)
    return uniq


def cases():
    """The thinned cross product of descriptors (dicts over CASE_KEYS)."""
    out = []
    Ms, Bs, Nps, Ks = (1, 64, 70, 192, 320, 5900, 6000), (1, 2, 8, 48), (128, 256, 384, 512), (64, 256, 768)
    dts = [(L.BF16, e) for e in (L.EPI_STORE, L.EPI_GATED, L.EPI_RES_SKIP, L.EPI_DFG)] + [(L.F32, L.EPI_STORE)]
    base = dict(impl=0, w2=0, ks=1, nsplit=128, bad="")
    for (dt, epi), M, B, Np, K, seg in itertools.product(dts, Ms, Bs, Nps, Ks, ("one", "near", "far", "long")):
        if seg in ("near", "far") and (K // 2) % (64 if dt == L.BF16 else 32):
            continue
        if seg == "long" and (K != 64 or B == 2):
            continue
        out.append(dict(base, dt=dt, epi=epi, M=M, B=B, Np=Np, K=K, seg=seg))
        if seg == "near" and B == 2 and dt == L.BF16:
            out.append(dict(out[-1], seg="mid"))                         # taps 48 rows apart: the four-piece window
    thin = [c for c in out if c["B"] in (1, 8) and c["M"] in (1, 70, 320, 6000) and c["seg"] in ("one", "near")]
    for c in thin:
        out += [dict(c, impl=1), dict(c, impl=2)]
        if c["dt"] == L.BF16 and c["epi"] == L.EPI_RES_SKIP and c["Np"] % 256 == 0:
            out.append(dict(c, nsplit=256))
        if c["dt"] == L.BF16 and c["epi"] == L.EPI_GATED and c["Np"] in (256, 512):
            out += [dict(c, w2=w, impl=i) for w in (1, 2) for i in (0, 1, 2)]
        for ks in (2, 4):
            out += [dict(c, ks=ks), dict(c, ks=ks, impl=2)]
    # both sides of each rule's limit under the default record: 128 | 129 tiles of 256 rows (nt_small_tiles), 256 | 257
    # blocks of 64 rows (nt_small_n64, nt_small_deep), 256 | 257 tiles of 192 rows (the 192-row cost model), 256 | 258 fp32
    # tiles of 16 and of 32 rows (nf_deep)
    for dt, epi in dts:
        for M in ((16384, 16385, 32768, 32769, 49152, 49153) if dt == L.BF16 else (2048, 2049, 4096, 4097)):
            out.append(dict(base, dt=dt, epi=epi, M=M, B=1, Np=128, K=256, seg="one", limit=1))
    c0 = dict(base, dt=L.BF16, epi=L.EPI_STORE, M=320, B=2, Np=256, K=256, seg="one")
    for bad in ("misalign", "ksum", "now", "segs0", "npad", "nsplit", "ksws", "ks3", "epi", "f32epi", "auxf32", "out2copy"):
        out += [dict(c0, bad=bad), dict(c0, bad=bad, impl=2), dict(c0, bad=bad, dt=L.F32), dict(c0, bad=bad, M=1, B=1, ks=2)]
    return out


def descriptor(c, sp=None):
    """The aew_gemm_nt_t of case c, its buffers in address space sp (a fresh one by default)."""
    sp = sp or AddrSpace()
    dt, epi, M, B, Np, K = c["dt"], c["epi"], c["M"], c["B"], c["Np"], c["K"]
    n = len(sp.addr)
    mat = lambda nm, pitch, d=dt: Mat.new(sp, f"{nm}{n}", B, 6200, pitch, d)
    x, y, W = mat("x", 8320), mat("y", 512), mat("W", 8320)
    if c["seg"] == "one":
        segs = [x.seg(K)]
    elif c["seg"] == "long":
        segs = [x.seg(ZERO_SPAN // 2 + 64)]
    else:
        segs = [x.seg(K // 2), x.seg(K // 2, row_off=dict(near=16, mid=48, far=128)[c["seg"]])]
    kw = dict(epi=epi, out0=y.view(), impl=c["impl"])
    if epi == L.EPI_GATED:
        kw.update(out1=mat("o1", 512).view(), out2=mat("o2", 512).view(), bias_ptr=mat("b", 512, L.F32).ptr)
    elif epi == L.EPI_RES_SKIP:
        kw.update(aux0=mat("a0", 512).view(), out1=mat("o1", 512, L.F32).view(), n_split=c["nsplit"])
    elif epi == L.EPI_DFG:
        kw.update(aux0=mat("a0", 512).view(), aux1=mat("a1", 512).view())
    if c["w2"]:
        kw.update(W2_ptr=mat("W2", 512).ptr, N2=128 * c["w2"] + (128 if Np == 512 else 0), N2_pad=128 * c["w2"] + (128 if Np == 512 else 0),
                  out3=mat("o3", 512).view(), aux0=mat("a0", 512).view())
    if c["ks"] > 1:
        kw.update(k_split=c["ks"], ksplit_ws_ptr=mat("ws", 512, L.F32).ptr, ksplit_tickets_ptr=mat("tk", 512, L.F32).ptr)
    g = make_nt(dt, M, Np, Np, B, segs, W.ptr, **kw)
    bad = c["bad"]
    if bad == "misalign":
        g.seg[0].ptr += 8
    elif bad == "ksum":
        g.K_total += 64
    elif bad == "now":
        g.W = None
    elif bad == "segs0":
        g.n_segs = 0
    elif bad == "npad":
        g.N_pad += 32
    elif bad == "nsplit":
        g.epi, g.n_split = L.EPI_RES_SKIP, 64
    elif bad == "ksws":
        g.k_split, g.ksplit_ws = 2, None
    elif bad == "ks3":
        g.k_split = 3
    elif bad == "epi":
        g.epi = 7
    elif bad == "f32epi":
        g.epi = L.EPI_GATED if dt == L.F32 else g.epi
    elif bad == "auxf32":
        g.aux0, g.flags = mat("a0", 512, L.F32).view(), L.EF_ADD_AUX0
    elif bad == "out2copy":
        g.flags = L.EF_OUT2_COPY
    return g


def set_tuning(lib, over):
    t = L.Tuning()
    lib.aew_tuning_default(C.byref(t))
    for k, v in over.items():
        setattr(t, k, v)
    assert lib.aew_tuning_set(C.byref(t)) == 0


def small_split(lib, g):
    ks, wsb, nt = C.c_int(), C.c_int64(), C.c_int()
    rc = lib.aew_gemm_nt_small_split(C.byref(g), 512, C.byref(ks), C.byref(wsb), C.byref(nt))
    return [rc, ks.value, wsb.value, nt.value]


def chain_codes(lib, c):
    """aew_nt_chain_build's return code, force 0 and 1, for the op followed by a copy of it with buffers of its own."""
    sp = AddrSpace()
    descs = (L.GemmNT * 2)(descriptor(c, sp), descriptor(c, sp))
    stages, bs = (L.NtStage * 2)(), (C.c_uint16 * (1 << 16))()
    nb, nc, st = C.c_int(), C.c_int(), C.c_int()
    return [lib.aew_nt_chain_build(C.cast(descs, C.c_void_p), 2, C.cast(stages, C.c_void_p), C.cast(bs, C.c_void_p), 1 << 19,
                                   C.byref(nb), C.byref(nc), C.byref(st), force) for force in (0, 1)]


def clean(name):
    name = "".join(name.split())
    return name[1:-1] if name.startswith("(") and name.endswith(")") else name


class Rec(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("grid", C.c_int), ("threads", C.c_int), ("lds", C.c_int)]


def second_launch(g):
    """The STORE | ADD_AUX0 GEMM over z that follows the GATED launch of a fused gated layer (W2) run unfused, as the
    launcher builds it."""
    b = L.GemmNT()
    b.dtype, b.impl, b.M, b.N, b.N_pad, b.batch = L.BF16, 0 if g.impl == 2 else g.impl, g.M, g.N2, g.N2_pad, g.batch
    b.n_segs, b.K_total = 1, g.N_pad // 2
    for f in ("ptr", "batch_stride", "row_pitch", "row_step", "row_off", "row_lo", "row_hi"):
        setattr(b.seg[0], f, getattr(g.out0, f))
    b.seg[0].k_len = g.N_pad // 2
    b.W, b.epi, b.flags, b.out0, b.aux0 = g.W2, L.EPI_STORE, L.EF_ADD_AUX0 if g.aux0.ptr else 0, g.out3, g.aux0
    return b


def relevant(over, c):
    """Records a case is recorded under: fp32 ops see the nf_* fields only, full-N ones fn_* and the check kernel none;
    the cases at a rule's limit are kept under the records that move the limit."""
    keys = set(over)
    if c["dt"] == L.F32:
        return not keys or any(k.startswith("nf_") for k in keys)
    if c["impl"] == 1:
        return not keys
    if c["impl"] == 2:
        return not keys or any(k.startswith("fn_") for k in keys) or keys == {"nt_wave_rows"}
    return True


def main(path):
    lib = C.CDLL(path)
    for fn in (lib.aew_tuning_default, lib.aew_tuning_set, lib.aew_nt_chain_build):
        fn.restype = C.c_int
    lib.aew_nt_chain_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.c_int]
    cs, tus = cases(), tunings()
    descs = [descriptor(c) for c in cs]
    out, n = (Rec * 8)(), C.c_int()
    chosen, names = {}, {}
    for ti, over in enumerate(tus):
        set_tuning(lib, over)
        for ci, (c, g) in enumerate(zip(cs, descs)):
            if not relevant(over, c):
                continue
            rc = lib.aew_rec_nt(C.byref(g), out, 8, C.byref(n))
            launches = [[clean(out[i].name.decode()), out[i].grid, out[i].threads, out[i].lds] for i in range(n.value)]
            bf = c["dt"] == L.BF16
            split = small_split(lib, g) if bf else None
            chain = chain_codes(lib, c) if bf and not c["bad"] and rc == 0 else None
            row = [ti, ci, rc, launches, split, chain]
            # Kept: per record and distinct answer (kernels with block and LDS, split, chain codes; refusals: per code, defect
            # and dtype) the case of the smallest grid; per record and kernel the case of the largest grid (many row tiles:
            # the grid then tells the row's tile); every case at a rule's limit
            ans = tuple((l[0], l[2], l[3]) for l in launches)
            grid = tuple(l[1] for l in launches)
            keys = [("a", ti if rc == 0 else c["bad"] + str(c["dt"]), rc, ans, bool(split and split[1] > 1), tuple(chain or ()))]
            keys += [("g", ti, l[0]) for l in launches]
            if c.get("limit"):
                keys.append(("l", ti, ci))
            for k in keys:
                best = chosen.get(k)
                if best is None or (grid < best[0] if k[0] == "a" else grid > best[0]):
                    chosen[k] = (grid, row)
    set_tuning(lib, {})
    rows = {}
    for _, row in chosen.values():
        rows[(row[0], row[1])] = row
    rows = [rows[k] for k in sorted(rows)]
    used = sorted({r[1] for r in rows})
    for r in rows:
        r[1] = used.index(r[1])
        for l in r[3]:                                               # (kernel names and cases are stored once, rows hold indices)
            l[0] = names.setdefault(l[0], len(names))
    with open(TABLE, "w") as f:
        f.write('{"case_keys": %s,\n "tunings": %s,\n "kernels": %s,\n "cases": %s,\n "rows": [\n'
                % (json.dumps(CASE_KEYS), json.dumps(tus), json.dumps(list(names)),
                   json.dumps([[cs[i][k] for k in CASE_KEYS] for i in used], separators=(",", ":"))))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} rows, {len(used)} cases, {len(names)} kernel instantiations, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
