"""Mode D's float32 restatement (tests/dynamic_spec.py, tests/grip_spec.py) against tests/golden/dynamic_spec_bits.npz: the
SHA-256 of every output of every case of tests/golden/gen_dynamic_spec_bits.py, recorded from the layered restatement that
dynamic_spec.py replaced - so the one step, control step and rollout are held to bits they did not produce themselves.  The
fixture pins every path a separate module used to state: the default setting through the sub-stepping machinery (plain/*,
fuzz/*/0 with M = 1), the rate, slip, progress, ceiling and disc lines each off and on (fuzz/*, trace/*), the coupled, loaded
and aero steps in the rollout and in the identification (ident/*), and the plan trace's rows."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_dynamic_spec_bits", os.path.join(HERE, "golden", "gen_dynamic_spec_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURE = gen.load()
ENTRIES = gen.entries()


def test_the_fixture_holds_every_case_of_the_generator():
    assert sorted(FIXTURE) == sorted(ENTRIES)
    assert len(FIXTURE) >= 120 and sum(len(outputs) for _, outputs in FIXTURE.values()) >= 553   # (the list only grows)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_restatement_has_the_recorded_bits(name):
    assert name in FIXTURE, "%s is not in the fixture" % name
    want_inputs, want = FIXTURE[name]
    got_inputs, got = gen.digests(ENTRIES[name])
    assert got_inputs == want_inputs, "%s: the INPUTS differ from the recorded ones (the case generator or a problem drifted)" % name
    assert sorted(got) == sorted(want), "%s: outputs %s, recorded %s" % (name, sorted(got), sorted(want))
    for output in sorted(want):
        assert got[output] == want[output], "%s: output %s differs from the recorded bits" % (name, output)
