"""The stream-ordering tests (tests/test_gpu_streams.py) are not vacuous: for every stage of tests/stream_cases.py the model of the
poison inputs differs from the model of the true inputs in at least MIN_DIFFERENT words of every output, for the whole stage and
for the one call the library's positive control makes.  A stage that read its buffers too early would therefore be seen."""
import numpy as np
import pytest

from tests import stream_cases as cases

WITH_ORACLE = ("secondary", "lights", "queries")
STAGES = ("denoise", "temporal", "resample", "adaptive_check") + WITH_ORACLE


def _case(name, oracle):
    return getattr(cases, name)(oracle) if name in WITH_ORACLE else getattr(cases, name)()


@pytest.mark.parametrize("which", ["model", "control"])
@pytest.mark.parametrize("name", STAGES)
def test_the_poison_gives_another_result(oracle, name, which):
    c = _case(name, oracle)
    true, poison = c.want(which, "true"), c.want(which, "poison")
    assert sorted(true) == sorted(poison) and true
    for k in true:
        n = cases.differing(poison[k], true[k])
        print(name, which, k, n, "of", np.asarray(true[k]).size)
        assert n >= cases.MIN_DIFFERENT or (k in c.constant and n == 0), (name, which, k, n)


@pytest.mark.parametrize("name", STAGES)
def test_the_inputs_differ_and_are_left_alone(oracle, name):
    c = _case(name, oracle)
    before = {k: v.copy() for k, v in {**c.true, **{"poison " + k: v for k, v in c.poison.items()}}.items()}
    c.want("model", "true"), c.want("model", "poison")
    for k in c.true:
        assert cases.differing(c.poison[k], c.true[k]) >= cases.MIN_DIFFERENT, k
        assert np.array_equal(cases.bits(c.true[k]), cases.bits(before[k])) and np.array_equal(cases.bits(c.poison[k]), cases.bits(before["poison " + k]))
