"""The two native denoisers at model level -- forward, deep copy, eager and graphed sampling, gradients through autograd and into a
trainer's flat buffer, two DPTrainer steps, one dropout step -- against the bits RECORDED with the package from before the host-side
plumbing between the nn.Modules and the C ABI was last reworked (tests/golden/model_surface.json, written by
tools/record_sampling_fixtures.py --set models).  Such rework must not change a bit, and the yardstick for that is the earlier
package, not the code under test.  The properties that need no record (graph == eager, the flat buffer == the .grads, the deep copy ==
the original) are asserted by the cases themselves (tests/model_cases.py)."""
import pytest
import torch

from tests import model_cases as mc
from tests import sampling_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    from bsi_amd import _native
    _native.lib()
    return sc.load_fixture(mc.FIXTURE)


def test_the_record_names_every_case(fixture):
    assert sorted(fixture) == sorted(c for c, _ in mc.all_cases())


@pytest.mark.parametrize("case,thunk", mc.all_cases(), ids=[c for c, _ in mc.all_cases()])
def test_model_surface(fixture, case, thunk):
    got = thunk()
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert all(float(t.abs().max()) > 0 for t in got.values())
    sc.assert_matches(case, got, fixture)
