"""Penalised Viterbi decoding of codes, without a GPU: the numpy restatement of the rule (tests/segment_emulator.py) against
brute force and a float64 Viterbi, its end points against the nearest-code oracle, and aew_segment_host - the host twin
that runs the kernels' own __host__ __device__ arithmetic - bit for bit against the restatement on every shape of the
GPU list; the launcher's refusals, the work list and the ABI."""
import ctypes as C

import numpy as np
import pytest

from ae_wavenet_amd import _lib as L, codes as CD
from oracle import exact
from tests import segment_emulator as SE

F32 = np.float32
PENALTIES = (0.0, 0.5, 1.0, 2.5, 7.0, 64.0, np.inf)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the rule ------------------------------------------------------------------------------------------------------------
def _int_case(rs, T, K, d):
    return rs.randint(-4, 5, (T, d)).astype(F32), rs.randint(-4, 5, (K, d)).astype(F32)


def test_emulator_attains_the_brute_force_minimum_on_integer_cases():
    """sq_l2 on integer-valued frames and entries: every sum is exact in fp32 and in float64, so the minimum is one number."""
    rs = np.random.RandomState(1)
    n = 0
    for case in range(60):
        T, K, d = rs.randint(1, 7), rs.randint(1, 4), rs.randint(1, 5)
        z, e = _int_case(rs, T, K, d)
        c = SE.local_costs(z, e, "sq_l2")
        assert np.array_equal(c, ((z[:, None, :] - e[None]) ** 2).sum(2))
        for lam in PENALTIES:
            out = SE.viterbi(c, lam)
            best = SE.brute_force64(c, lam)
            assert SE.objective64(c, out["codes"], lam) == best, (case, lam)
            if np.isfinite(lam):
                assert float(out["cost"]) == best, (case, lam)
            n += 1
    assert n == 420


def test_segment_count_does_not_grow_with_the_penalty():
    rs = np.random.RandomState(2)
    for case in range(10):
        z, e = _int_case(rs, 40, 5, 3)
        c = SE.local_costs(z, e, "sq_l2")
        segs = [SE.viterbi(c, lam)["n_seg"] for lam in PENALTIES]
        assert all(a >= b for a, b in zip(segs[:-1], segs[1:])), segs
        assert segs[-1] == 1


@pytest.mark.parametrize("metric", ["scaled_l2", "sq_l2"])
def test_end_points_are_the_nearest_code_and_one_code(metric):
    rs = np.random.RandomState(3)
    z = rs.standard_normal((90, 8)).astype(F32)
    e = rs.standard_normal((33, 8)).astype(F32)
    e[20:30] = e[5:15]                                                       # duplicated rows: ties
    z[7] = e[9]                                                              # and a frame that sits on a duplicated entry
    ind, dist, _ = exact.vq_nearest(z, e, metric)
    out = SE.segment(z, e, metric, 0.0)
    assert np.array_equal(out["codes"], ind) and np.array_equal(_bits(out["dist"]), _bits(dist))
    assert out["codes"][7] == 9
    one = SE.segment(z, e, metric, np.inf)
    assert one["n_seg"] == 1 and len(set(one["codes"].tolist())) == 1
    c = SE.local_costs(z, e, metric)
    assert one["codes"][0] == int(np.argmin(c.astype(np.float64).sum(0)))


@pytest.mark.parametrize("metric", ["scaled_l2", "sq_l2"])
def test_fp32_recurrence_is_near_the_float64_optimum(metric):
    """One rounding per accumulated term: T additions along the path and d in each local cost - 4 * (T + d) * 2^-24."""
    T, K, d = 200, 130, 8
    bound = 4 * (T + d) * 2.0 ** -24
    rs = np.random.RandomState(4)
    worst = 0.0
    for case in range(4):
        z, e = rs.standard_normal((T, d)).astype(F32), rs.standard_normal((K, d)).astype(F32)
        c = SE.local_costs(z, e, metric)
        scale = float(np.median(c.min(1)))
        for lam in (0.0, 0.1 * scale, 0.5 * scale, scale, 3 * scale, 30 * scale):
            out = SE.viterbi(c, lam)
            got, best = SE.objective64(c, out["codes"], F32(lam)), SE.viterbi64(c, F32(lam))
            gap = (got - best) / best
            worst = max(worst, gap)
            assert -1e-12 <= gap <= bound, (case, lam, gap)
    print(f"worst relative gap {worst:.3g} against the bound {bound:.3g}")


# ---- the host twin -----------------------------------------------------------------------------------------------------------
def run_host(case, ws_short=0, table=None, K=None, n_out=None):
    """aew_segment_host over a case -> (rc, codes, dist, cost, n_seg, n_bad); outputs carry canaries."""
    frames, emb, off = case["frames"], np.ascontiguousarray(case["emb"]), case["offsets"]
    n, d_pitch = frames.shape
    K = len(emb) if K is None else K
    plan = CD.segment_plan(np.diff(off), min(K, L.SEG_MAX_K))
    tbl = plan.table if table is None else table
    if table is None:
        tbl["lam"] = case["lams"]
    U = len(tbl)
    codes, dist = np.full(n + 8, -9, np.int64), np.full(n + 8, -9.0, F32)
    cost, n_seg, n_bad = np.full(U + 8, -9.0, F32), np.full(U + 8, -9, np.int32), np.zeros(1, np.uint32)
    ws = np.zeros(max(plan.ws_bytes // 8, 1), np.int64)
    cs = L.CodeSegment()
    cs.frames, cs.n_elems = frames.ctypes.data, frames.size
    cs.emb, cs.K, cs.d, cs.d_pitch, cs.metric = emb.ctypes.data, K, case["d"], d_pitch, CD.VQ_METRICS[case["metric"]]
    cs.table_host, cs.U = tbl.ctypes.data, U
    cs.codes, cs.dist, cs.n_out = codes.ctypes.data, dist.ctypes.data, n if n_out is None else n_out
    cs.cost, cs.n_seg, cs.n_bad = cost.ctypes.data, n_seg.ctypes.data, n_bad.ctypes.data
    cs.ws, cs.ws_bytes = ws.ctypes.data, plan.ws_bytes - ws_short
    rc = L.load().aew_segment_host(C.byref(cs))
    assert (codes[n:] == -9).all() and (dist[n:] == -9.0).all() and (cost[U:] == -9.0).all() and (n_seg[U:] == -9).all()
    return rc, codes[:n], dist[:n], cost[:U], n_seg[:U], int(n_bad[0])


CASES = SE.gpu_cases()


def check_against_emulator(case, got):
    codes, dist, cost, n_seg, n_bad = got
    w_codes, w_dist, w_cost, w_seg, w_bad = SE.expected(case)
    assert np.array_equal(codes, w_codes), case["name"]
    assert np.array_equal(_bits(dist), _bits(w_dist)), case["name"]
    assert np.array_equal(_bits(cost), _bits(w_cost)), case["name"]
    assert np.array_equal(n_seg, w_seg) and n_bad == w_bad, case["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_equals_the_emulator_bit_for_bit(case):
    rc, *got = run_host(case)
    assert rc == 0
    check_against_emulator(case, got)


def test_the_shape_list_covers_what_it_names():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    by = {c["name"]: c for c in CASES}
    assert sum(SE.T_MIX) % SE.SLAB and sum(SE.T_MIX) > 5 * SE.SLAB and 0 in SE.T_MIX
    assert len(by["K257-sq_l2"]["emb"]) == SE.GROUP + 1 and len(by["K256-sq_l2"]["emb"]) == SE.GROUP
    assert len(set(by["K130-sq_l2"]["lams"].tolist())) >= 5
    assert np.isnan(by["d3"]["frames"][:, 3:]).all()                            # the pad channels are never read
    # the constructed ties bite: duplicated rows, and a step at which two entries hold the same r while neither stays
    t = by["ties-dup"]
    assert np.array_equal(t["emb"][5:], t["emb"][:5])
    c = SE.local_costs(t["frames"][:40, :3], t["emb"], "sq_l2")
    r = c[0].copy()
    equal_at_switch = 0
    for step in range(1, 40):
        m = r.min()
        p = r - m
        equal_at_switch += int(((p >= 1.0).sum() >= 2) and len(set(p[p >= 1.0].tolist())) < (p >= 1.0).sum())
        r = c[step] + np.minimum(p, F32(1.0))
    assert equal_at_switch > 0
    assert SE.expected(by["nan-mid"])[4] == 1 and SE.expected(by["nan-mid-sq"])[4] == 1


def test_nan_and_inf_frames_are_counted_and_follow_the_rule():
    for poison in (np.nan, np.inf, -np.inf):
        case = SE.make_case(f"poison{poison}", 20, 4, 6, (9, 12, 5), "scaled_l2", 11)
        case["frames"][9 + 6, 1] = poison
        case["frames"][9 + 12 + 4, 0] = poison                                 # the last frame of the last utterance
        rc, *got = run_host(case)
        assert rc == 0 and got[4] == 2
        check_against_emulator(case, got)
        assert np.isfinite(got[2][0]) and not np.isfinite(got[2][1:]).any()


def test_malformed_calls_are_refused_with_nothing_written():
    case = SE.make_case("refuse", 70, 4, 4, (6, 0, 9), "sq_l2", 12)
    W1 = (70 + 63) // 64 + 1
    good = CD.segment_plan([6, 0, 9], 70).table
    good["lam"] = 1.0
    assert run_host(case, table=good.copy())[0] == 0
    bad = []
    for field, u, value in (("lam", 0, -1.0), ("lam", 2, np.nan), ("lam", 0, -np.inf), ("n_frames", 0, -1),
                            ("first_frame", 2, 7), ("first_frame", 0, -1), ("n_frames", 2, 10),
                            ("back_base", 2, 15 * W1 - 9 * W1 + 1), ("back_base", 0, -1),
                            ("back_base", 2, 5 * W1)):                       # overlaps utterance 0's [0, 6 * W1)
        tbl = good.copy()
        tbl[field][u] = value
        bad.append((field, u, value, run_host(case, table=tbl)))
    for field, u, value, (rc, codes, dist, cost, n_seg, n_bad) in bad:
        assert rc == L.E_ARG, (field, u, value)
        assert (codes == -9).all() and (dist == -9.0).all() and (cost == -9.0).all() and (n_seg == -9).all() and n_bad == 0
    assert run_host(case, table=good.copy(), ws_short=8)[0] == L.E_ARG             # a short workspace
    assert run_host(case, table=good.copy(), n_out=14)[0] == L.E_ARG               # outputs shorter than the frame buffer
    big = dict(case, emb=np.zeros((L.SEG_MAX_K + 1, 4), F32))
    assert run_host(big, table=good.copy())[0] == L.E_ARG                          # K > AEW_SEG_MAX_K
    out = C.c_int64(-5)
    assert L.load().aew_segment_ws_bytes(15, L.SEG_MAX_K + 1, C.byref(out)) == L.E_ARG
    assert L.load().aew_segment_ws_bytes(-1, 4, C.byref(out)) == L.E_ARG and out.value == -5
    # U = 0 is a call that does nothing
    rc, codes, *_ = run_host(case, table=good[:0].copy())
    assert rc == 0 and (codes == -9).all()
    # the python front refuses a penalty before it builds anything
    for pen in (-1.0, float("nan"), [0.0, -0.5, 1.0]):
        with pytest.raises(L.AewError, match="penalty"):
            CD._penalties(pen, 3, "segment()")
    with pytest.raises(L.AewError, match="one per utterance"):
        CD._penalties([1.0, 2.0], 3, "segment()")
    assert CD._penalties(np.inf, 2, "x").tolist() == [np.inf, np.inf]


def test_segment_plan_agrees_with_the_library():
    lib = L.load()
    for K in (1, 63, 64, 65, 130, 4095, 4096):
        for counts in ([], [0], [5], [1, 0, 7, 64], [129, 3]):
            plan = CD.segment_plan(counts, K)
            n = int(sum(counts))
            out = C.c_int64(-1)
            assert lib.aew_segment_ws_bytes(n, K, C.byref(out)) == 0
            assert plan.ws_bytes == out.value == CD.segment_ws_bytes(n, K)
            assert plan.ws_bytes >= 4 * n * K and plan.ws_bytes % 8 == 0
            W1 = (K + 63) // 64 + 1
            assert plan.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist()
            assert plan.table["first_frame"].tolist() == plan.offsets[:-1].tolist()
            assert plan.table["back_base"].tolist() == (plan.offsets[:-1] * W1).tolist()
            assert plan.table["n_frames"].tolist() == list(counts) and not plan.table["lam"].any()
    with pytest.raises(ValueError):
        CD.segment_plan([3, -1], 8)
    with pytest.raises(ValueError):
        CD.segment_plan([3], 4097)


def test_abi_records_and_op_numbers():
    lib = L.load()
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(50) == -1 and lib.aew_sizeof(54) == -1
    assert lib.aew_sizeof(51) == C.sizeof(L.SegUtt) == np.dtype(L.SEG_UTT_DTYPE).itemsize == 24
    assert lib.aew_sizeof(52) == C.sizeof(L.FrameStitch) and lib.aew_sizeof(53) == C.sizeof(L.CodeSegment)
    assert C.sizeof(L.Op) == lib.aew_sizeof(0) == 16 + C.sizeof(L.GemmNT) == 1656     # the op record did not grow
    assert (L.OP_FRAME_STITCH, L.OP_CODE_SEGMENT) == (L.OP_SEQ_ALIGN + 1, L.OP_SEQ_ALIGN + 2)
    assert L.OP_FIELD[L.OP_FRAME_STITCH] == "fstitch" and L.OP_FIELD[L.OP_CODE_SEGMENT] == "cseg"
    assert "aew_segment_host" in L.EXPORTS and "aew_segment_ws_bytes" in L.EXPORTS
