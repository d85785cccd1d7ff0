"""Restart of dead codes on the GPU, through ctypes -> C ABI: AEW_OP_VQ_RESTART (aew_vq_restart_t) against the numpy
restatement of tests/code_restart_emulator.py, byte for byte and between canaries; the guard word; the module surface
on the tiny VQ-VAE-EMA model of tests/golden (restarted codes are found again by the nearest-code search, at distance
zero, and survive a codebook refresh); and a model with the option set but no restart due stays bit-equal to one
without it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from tests.code_restart_emulator import restart_reference
from tests.test_plan_cpu import load, tiny_hps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD = 64
F_CANARY, I_CANARY = -12345.5, -777
MIN_USAGE = 0.25           # live denominators are drawn from [0.5, 1.5), dead ones from [0, 0.2) or NaN


def stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """The op's six buffers, each in an allocation of its own with PAD canary elements in front and behind."""

    def __init__(self, K, d, d_pitch, Q, seed=0):
        self.K, self.d, self.d_pitch, self.Q = K, d, d_pitch, Q
        gen = torch.Generator().manual_seed(seed)
        self.host = dict(ze=torch.randn(Q * d_pitch, generator=gen), emb=torch.randn(K * d, generator=gen),
                         numer=torch.randn(K * d, generator=gen), denom=torch.rand(K, generator=gen) + 0.5,
                         out=torch.tensor([-5, -6, 10, -7], dtype=torch.int32),
                         pairs=torch.full((2 * L.VQ_RESTART_MAX,), -9, dtype=torch.int32))
        self.dev = {}
        for k, h in self.host.items():
            can = F_CANARY if h.dtype == torch.float32 else I_CANARY
            self.dev[k] = torch.full((h.numel() + 2 * PAD,), can, dtype=h.dtype, device=DEV)
        self.guard = torch.zeros(1, dtype=torch.int32, device=DEV)

    def view(self, k):
        return self.dev[k][PAD:PAD + self.host[k].numel()]

    def reset(self, dead=(), dead_values=None):
        denom = self.host["denom"].clone()
        for i, k in enumerate(dead):
            denom[k] = 0.0 if dead_values is None else dead_values[i]
        self.start = dict(self.host, denom=denom)
        for k, h in self.start.items():
            can = F_CANARY if h.dtype == torch.float32 else I_CANARY
            self.dev[k].fill_(can)
            self.view(k).copy_(h)

    def launch(self, max_codes, denom_init, seed, call, guard=False):
        op = L.Op()
        op.kind = L.OP_VQ_RESTART
        r = op.u.vqr
        r.ze, r.emb, r.numer, r.denom = (self.view(k).data_ptr() for k in ("ze", "emb", "numer", "denom"))
        r.out, r.pairs, r.guard = self.view("out").data_ptr(), self.view("pairs").data_ptr(), self.guard.data_ptr()
        r.Q, r.d, r.d_pitch, r.K, r.max_codes = self.Q, self.d, self.d_pitch, self.K, max_codes
        r.min_usage, r.denom_init, r.seed, r.call = MIN_USAGE, denom_init, seed, call
        self.guard.fill_(1 if guard else 0)
        fail = C.c_int(-1)
        rc = L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
        torch.cuda.synchronize()
        assert rc == 0, (rc, fail.value)

    def got(self):
        """{name: bytes of the whole allocation, canaries included}"""
        return {k: t.cpu().numpy().tobytes() for k, t in self.dev.items()}

    def want(self, max_codes, denom_init, seed, call):
        s = {k: v.numpy() for k, v in self.start.items()}
        emb, numer, denom, out, pairs = restart_reference(
            s["ze"].reshape(self.Q, self.d_pitch), s["emb"].reshape(self.K, self.d), s["numer"].reshape(self.K, self.d),
            s["denom"], max_codes, MIN_USAGE, denom_init, seed, call, total=int(s["out"][2]))
        full_pairs = s["pairs"].copy()
        full_pairs[:2 * max_codes] = pairs.reshape(-1)             # rows behind max_codes are not the launch's
        res = dict(ze=s["ze"], emb=emb.reshape(-1), numer=numer.reshape(-1), denom=denom, out=out, pairs=full_pairs)
        out_b = {}
        for k, v in res.items():
            can = np.full(PAD, F_CANARY if v.dtype == np.float32 else I_CANARY, v.dtype)
            out_b[k] = np.concatenate([can, v, can]).tobytes()
        return out_b, out, pairs


def dead_sets(K):
    rs = np.random.RandomState(K)
    edge = [k for k in (1023, 1024) if k < K] or [K - 1]           # a chunk boundary where K has one, else the last code
    half = np.sort(rs.permutation(K)[:K // 2]).tolist()
    nan_k = K // 3
    return [("none", [], None, 64), ("one", [0], None, 64), ("boundary", edge, None, 64),
            ("half", half, rs.uniform(0.0, 0.2, len(half)).astype(np.float32).tolist(), 64),
            ("all, 64 at most", list(range(K)), None, 64), ("all, 1024 at most", list(range(K)), None, 1024),
            ("nan", [nan_k], [float("nan")], 64)]


SHAPES = [(16, 4, 64, 7), (1500, 32, 64, 232), (4096, 64, 64, 232), (2049, 70, 128, 1), (1024, 32, 32, 1024)]


@pytest.mark.parametrize("K,d,d_pitch,Q", SHAPES)
def test_op_against_the_reference_byte_for_byte(K, d, d_pitch, Q):
    c = Case(K, d, d_pitch, Q, seed=K + Q)
    for name, dead, values, max_codes in dead_sets(K):
        for denom_init in (1.0, 0.37):
            seed, call = 11 + len(dead), 1000003 * K + max_codes
            c.reset(dead, values)
            c.launch(max_codes, denom_init, seed, call)
            got = c.got()
            want, out, pairs = c.want(max_codes, denom_init, seed, call)
            n = min(len(dead), Q, max_codes)
            assert out.tolist() == [len(dead), n, 10 + n, 0], name
            for k in ("out", "pairs", "denom", "numer", "emb", "ze"):
                assert got[k] == want[k], (name, denom_init, k)
            if denom_init == 1.0:                                   # the new code IS the encoder output
                emb, ze = c.view("emb").cpu().numpy().reshape(K, d), c.start["ze"].numpy().reshape(Q, d_pitch)
                assert len(set(pairs[:n, 1].tolist())) == n
                for k, q in pairs[:n]:
                    assert emb[k].tobytes() == ze[q, :d].tobytes(), (name, k, q)
            if name == "half":                                      # the same counters on the same buffers: the same bytes
                c.reset(dead, values)
                c.launch(max_codes, denom_init, seed, call)
                assert c.got() == got
                c.reset(dead, values)
                c.launch(max_codes, denom_init, seed, call + 1)     # ... and another call takes other rows
                assert Q == 1 or c.got()["pairs"] != got["pairs"]


def test_guard_word_set_nothing_is_written():
    c = Case(1500, 32, 64, 232, seed=1)
    c.reset(list(range(0, 1500, 7)))
    before = c.got()
    c.launch(64, 1.0, 1, 2, guard=True)
    assert c.got() == before
    c.launch(64, 1.0, 1, 2)
    after = c.got()
    assert after["ze"] == before["ze"] and all(after[k] != before[k] for k in ("emb", "numer", "denom", "out", "pairs"))


# ----------------------------------------------------------------------------------------------
# engine and module surface: the tiny VQ-VAE-EMA model of tests/golden (K = 10, d = 6, Q = 14)
# ----------------------------------------------------------------------------------------------
def _model(**kw):
    from ae_wavenet_amd import autoencoder_model as ae
    z = load(GOLDEN, "ae_tiny_vqvae-ema_random.npz")
    hps, n_mel = tiny_hps(z, global_model="autoencoder")
    torch.manual_seed(0)
    m = ae.AutoEncoder(hps, n_mel=n_mel, take_compat=True, **kw).to(DEV)
    emb0, comp = torch.from_numpy(z["emb0"]), 1.0 - hps.bn_vq_ema_gamma
    sd = {k: torch.from_numpy(z["w." + k]) for k, _ in m.named_parameters()}
    sd.update({"bottleneck.emb": emb0, "bottleneck.ema_numer": emb0 * comp,
               "bottleneck.ema_denom": torch.full((emb0.shape[0],), comp), "bottleneck.ind_hist": torch.zeros(emb0.shape[0])})
    m.load_state_dict(sd)
    batch = [torch.from_numpy(z[k]).to(DEV) for k in ("wav", "mel", "voice", "jitter")]
    return m, batch


def _step(m, opt, batch):
    opt.zero_grad()
    _, _, loss = m.run(*batch)
    loss.backward()
    opt.step()


def test_restarted_codes_are_found_again_and_survive_the_refresh():
    """One training step, then a forward whose encoder outputs the restart seeds from (the step changed the weights, so
    these are the outputs a further forward of the same batch reproduces).  The refresh is checked right behind the
    restart: a forward in between accumulates the EMA statistics of the restarted codes, and emb = numer / denom of
    those is the same vector only up to rounding."""
    from ae_wavenet_amd import optim
    m, batch = _model()
    _step(m, optim.FusedAdam(m, lr=1e-3), batch)
    m.run(*batch)
    eng = m._engine
    dead = [0, 3, 4, 8, 9]
    eng.ema_denom[dead] = 0.0
    m.bottleneck.restart_dead_codes(min_usage=0.005, call=7)
    counts = m.bottleneck.restart_counts.tolist()
    assert counts == [5, 5, 5, 0]
    pairs = eng.restart_pairs().cpu().numpy()
    assert pairs[:5, 0].tolist() == dead and (pairs[5:64] == -1).all()
    ze = eng.lin.tensor().cpu().numpy().reshape(eng.Q, eng.nlin_p)[:, :eng.d]
    assert len({ze[q].tobytes() for q in range(eng.Q)}) == eng.Q, "distinct rows: no other code can tie at distance 0"
    emb = eng.emb.cpu().numpy().copy()
    for k, q in pairs[:5]:
        assert emb[k].tobytes() == ze[q].tobytes()
    m.bottleneck.update_codebook()                                  # emb = numer / denom once more: the same bits
    assert eng.emb.cpu().numpy()[dead].tobytes() == emb[dead].tobytes()
    m.run(*batch)                                                   # the same batch, the same weights
    torch.cuda.synchronize()
    ze2 = eng.lin.tensor().cpu().numpy().reshape(eng.Q, eng.nlin_p)[:, :eng.d]
    assert ze2.tobytes() == ze.tobytes()
    ind, dist = eng.ind[:eng.Q].cpu().numpy(), eng.min_dist[:eng.Q].cpu().numpy()
    for k, q in pairs[:5]:
        assert ind[q] == k and dist[q] == 0.0, (k, q, ind[q], dist[q])
    assert "vq_restarted" not in m.objective.metrics                # no option, no metric


def test_an_option_that_is_not_due_changes_nothing():
    from ae_wavenet_amd import optim
    res = []
    for kw in (dict(), dict(codebook_restart=dict(every=1000, min_usage=0.005))):
        m, batch = _model(**kw)
        opt = optim.FusedAdam(m, lr=1e-3)
        for _ in range(3):
            _step(m, opt, batch)
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
        for i, s in opt.state_dict()["state"].items():
            sd.update({f"opt.{i}.{k}": np.asarray(v.cpu() if torch.is_tensor(v) else v).copy() for k, v in s.items()})
        res.append((sd, set(m.objective.metrics), m))
    (a, keys_a, _), (b, keys_b, mb) = res
    assert list(a) == list(b) and len(a) > 10
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert keys_b - keys_a == {"vq_restarted"} and keys_a <= keys_b
    assert mb.bottleneck.restart_counts.tolist() == [0, 0, 0, 0] and int(mb.objective.metrics["vq_restarted"]) == 0
