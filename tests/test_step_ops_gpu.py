"""The step's non-GEMM kernels one at a time on the device, against the fp64 definitions of tests/step_ops_reference.py.

Every case of tests/step_ops_cases.py runs as a one-op Plan with plan.run(stream) on a device Workspace mirrored from
the CPU one the interpreter test uses (tests/test_step_ops_cpu.py): the kernel and the interpreter see the same bytes.
Every buffer - outputs between their canary regions, inputs, pads, rows no op should touch - must come back bit-identical
except for the elements the reference says the op writes; those are held to the rules of step_ops_cases.py:

  exact       base_gather x / one-hot, lc_gather, amax, every pad column, the dropped position of nll / ptgt / dlogits,
              gradient rows of absent speakers, rows of codes nobody chose
  fp32 sums   spk_bias, spk_bwd, lc_scatter, vq_bwd, ae_norm: (n + c) 2^-24 S, derived, for any order of the sum
  intrinsics  outputs behind __expf / __logf: the coefficient of S is 8 x the worst error measured ONCE on an MI355X over
              exactly these cases against the fp64 reference (INTRINSIC below; dlogits adds one bf16 spacing)

Kernel forms no other test runs: the general path of k_softmax_nll (Q != 256 or a pitch off 4), k_base_gather (no
transposed table), k_lc_scatter (the zero-plus-atomic form, N > 4096), k_spk_bwd with several batch chunks (B > 16).
"""
import pytest
import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Plan
from tests import step_ops_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# tag: coefficient of S.  Worst (|got - ref| - extra) / S measured on an MI355X (gfx950, ROCm 7.2) over the cases of this
# file, in units of 2^-24, and the bound = 8 x that (the intrinsics' error depends on the argument and the seeds are
# fixed; a wrong formula or index is off by orders of magnitude more).  S is the expectation's (step_ops_cases.py).
MEASURED_ULP = {
    "nll": 1.345,          # bound 10.76 x 2^-24 S,  S = 1 + |l_tgt| + |max| + |log sum exp|
    "ptgt": 1.835,         # bound 14.68 x 2^-24 S,  S = ptgt x the S of nll
    "peak": 0.814,         # bound  6.51 x 2^-24 S,  S = 1 + |max| + |log sum exp|
    "dlogits": 0.0,        # bound  0: before the bf16 rounding no error showed beyond the one bf16 spacing 2^-7 |ref| the rule
                           #           grants anyway (the rounding itself takes half of it), so the spacing is the whole bound
    "vae_sample": 1.467,   # bound 11.74 x 2^-24 S,  S = |mu| + |sigma eps| (1 + |ls / 2|)
    "vae_kl": 0.474,       # bound  3.79 x 2^-24 S,  S = sum_j 2 + 2 r + mu^2 + 2 r sigma^2,  r = 1 + |ls / 2|
    "vae_dls": 2.283,      # bound 18.26 x 2^-24 S,  S = |dsample eps sigma / 2| r + |k| (1 + 2 r sigma^2) / 2   (the log-sigma half of dlin;
                           #           the mu half has no intrinsic and keeps the derived (2 + 16) 2^-24)
}
INTRINSIC = {k: 8.0 * v * K.U for k, v in MEASURED_ULP.items()}


def run_gpu(case, tuning=None, report=None, coef=INTRINSIC, check=True):
    ws_c = case.build()
    before = K.snapshot(ws_c)
    ws_g = K.clone_ws(ws_c, DEV)
    plan = Plan(case.name)
    for kind, payload, label in case.ops(ws_g):
        plan.add(kind, payload, label)
    plan.run(torch.cuda.current_stream().cuda_stream, tuning=tuning)
    torch.cuda.synchronize()
    after = K.snapshot(ws_g)
    if check:
        K.verify(case, before, after, coef=coef, report=report, what="kernel")
    return after


def det(on):
    return L.current_tuning(deterministic=on)


@pytest.mark.parametrize("Q,Qp,pitch", K.SOFTMAX_SHAPES)
def test_softmax_nll(Q, Qp, pitch):
    for case in [c for c in K.softmax_cases() if (c.Q, c.Q_pad, c.pitch) == (Q, Qp, pitch)]:
        run_gpu(case)


def test_softmax_general_path_agrees_with_register_path():
    """(256, 256, 258) is the data of (256, 256, 256) on an unaligned pitch: the general path on the register path's rows"""
    reg = [c for c in K.softmax_cases() if (c.Q, c.pitch) == (256, 256)]
    gen = [c for c in K.softmax_cases() if (c.Q, c.pitch) == (256, 258)]
    for a, b in zip(reg, gen):
        assert a.register_path() and not b.register_path() and (a.backward, a.gmul) == (b.backward, b.gmul)
        ra, rb = run_gpu(a), run_gpu(b)
        K.agree(a, ra, b, rb, INTRINSIC, only=("nll", "ptgt", "dlogits"), what="register vs general")


@pytest.mark.parametrize("T", K.BASE_T)
@pytest.mark.parametrize("R_,R_pad", K.BASE_R)
def test_base_gather_both_forms(T, R_, R_pad):
    """k_base_gather_t (Wt set) and k_base_gather (Wt = NULL): bit-identical to the reference and to each other"""
    for with_wt, without in K.base_gather_variants(T, R_, R_pad):
        a, b = run_gpu(with_wt), run_gpu(without)
        K.same_bits(a, b, ("x", "onehot"), with_wt.name)


@pytest.mark.parametrize("B,N,C,Cp", K.LC_SHAPES)
def test_lc_gather_scatter(B, N, C, Cp):
    for case in K.lc_cases(B, N, C, Cp):
        run_gpu(case)


@pytest.mark.parametrize("case", K.lc_big_cases(), ids=lambda c: c.name)
def test_lc_scatter_both_forms(case):
    """N = 4096: the gather form's last size; N = 4097: the zero-plus-atomic form (target pre-zeroed).  Both are held to
    the one reference under the one rule, which is what makes the two forms agree."""
    assert bool(L.load().aew_lc_scatter_needs_zero(case.N)) == (case.N > 4096)
    run_gpu(case)


@pytest.mark.parametrize("D,Dp,G,B", K.SPK_SHAPES)
def test_spk_bias_and_bwd(D, Dp, G, B):
    for spk_b, running in K.SPK_VARIANTS:
        run_gpu(K.SpkCase(D, Dp, G, B, spk_b=spk_b))
        case = K.SpkCase(D, Dp, G, B, spk_b=spk_b, running=running, backward=True)
        r1, r2, r0 = run_gpu(case, det(1)), run_gpu(case, det(1)), run_gpu(case, det(0))
        # two deterministic runs: the speaker-embedding sums are ticketed for every B; the bias / projection sums are
        # plain stores up to 16 batch elements, two commutative atomic adds up to 32, the scheduler's order beyond
        bp, spk, _ = case.regions()
        g1, g2 = (r["grads"][K.GUARD:].view(torch.int32) for r in (r1, r2))
        for s in spk:
            assert torch.equal(g1[torch.from_numpy(s)], g2[torch.from_numpy(s)]), (case.name, "speaker-embedding sums not reproducible")
        if B <= 32:
            assert torch.equal(g1[torch.from_numpy(bp)], g2[torch.from_numpy(bp)]), (case.name, "bias / projection sums not reproducible")
        K.agree(case, r1, case, r0, only=("grads",), what="deterministic 1 vs 0")
        split = K.SpkCase(D, Dp, G, B, spk_b=spk_b, running=running, backward=True, split=True)
        K.agree(case, r1, split, run_gpu(split, det(1)), only=("grads",), what="one op vs layer_range split")


@pytest.mark.parametrize("Q,d,dp,metric", K.VQ_SHAPES)
def test_vq_bwd(Q, d, dp, metric):
    for demb, gmul in K.VQ_VARIANTS:
        case = K.VqBwdCase(Q, d, dp, metric, demb, gmul)
        r1, r2, r0 = run_gpu(case, det(1)), run_gpu(case, det(1)), run_gpu(case, det(0))
        K.same_bits(r1, r2, ("dze", "demb"), case.name + ": two deterministic runs")
        K.agree(case, r1, case, r0, what="deterministic 1 vs 0")


@pytest.mark.parametrize("Q,d,dp", K.ROW_SHAPES)
def test_vae(Q, d, dp):
    for case in K.vae_cases(Q, d, dp):
        run_gpu(case)


@pytest.mark.parametrize("Q,d,dp", K.ROW_SHAPES)
def test_ae_norm(Q, d, dp):
    for case in K.ae_norm_cases(Q, d, dp):
        run_gpu(case)
