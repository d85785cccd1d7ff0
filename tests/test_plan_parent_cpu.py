"""The training-step plans against the recording made at the commit before DecoderPlan.build_backward was restructured
(tests/data/plan_parent.json, see tests/data/plan_gen.py): for every recorded configuration, an engine built on device
"cpu" has the same ops in the same order in every plan - head, payload, and the contents of every table an op points
to, addresses as (buffer, offset) - and the same ordered workspace allocations.  A difference means the program that
runs on the device changed; the recording is regenerated only from the commit it pins.  For the default and the
data-parallel configurations the same holds for the optimizer, clip, ratio, swap, restart, evaluation, encode and
conditioning plans and the allocations behind them, as built before the plan builder was split into stages (the keys
"late" / "alloc_late").  Plans only - no device."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("plan_gen", os.path.join(HERE, "data", "plan_gen.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CONFIGS = gen.configs()


@pytest.fixture(scope="module")
def table():
    with open(gen.TABLE) as f:
        return json.load(f)


def test_recording_covers_every_configuration(table):
    assert set(table["configs"]) == set(CONFIGS)
    assert os.path.getsize(gen.TABLE) <= os.path.getsize(os.path.join(HERE, "data", "nt_pick_parent.json"))


def _compare(table, name, eng, plans, want, attr_of):
    assert set(plans) == set(want), "plans the engine has"
    for nm, got in plans.items():
        ref = want[nm]
        if not isinstance(ref, str):                                     # a slice of another plan: [plan, start, stop]
            assert got == ref, (nm, got, ref)
            continue
        ref = table["plans"][ref]
        for i, (g, r) in enumerate(zip(got, ref)):
            if g != r:
                print(json.dumps(gen.canon_op(eng, getattr(eng, attr_of.get(nm, nm)), i), indent=1))
                pytest.fail(f"{name}: plan {nm} op {i}: built {g}, recorded {r} (canonical form of the built op above)")
        assert len(got) == len(ref), (nm, [l for l, _ in got[len(ref):]], [l for l, _ in ref[len(got):]])


def _compare_alloc(eng, alloc, want):
    if alloc != want:
        print(json.dumps(gen.allocations(eng)))
    assert alloc == want, "workspace allocations (name, elements, dtype, in order; the built list above)"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_plans_equal_the_recording(table, name):
    want = table["configs"][name]
    eng = gen.build(CONFIGS[name])
    late = name in gen.late_configs()
    assert late == ("late" in want) == ("alloc_late" in want)
    alloc, plans, *rest = gen.record(eng, late=late)
    _compare(table, name, eng, plans, want["plans"], {})
    _compare_alloc(eng, alloc, want["alloc"])
    if late:                                                             # the plans and buffers of the state completed at first use
        assert set(want["late"]) >= set(gen.LATE_PLANS) - {"encode"}
        _compare(table, name, eng, rest[1], want["late"], gen.LATE_PLANS)
        _compare_alloc(eng, rest[0], want["alloc_late"])
