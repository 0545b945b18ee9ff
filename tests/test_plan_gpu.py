"""What mmg_create selects on this MI355X equals the recorded plan (tests/golden/plans_mi355x.json), caps included: a kernel
change that moves an occupancy fails here and the fixture is then re-recorded deliberately.  Handle creation only."""
import pytest

from multimodalgame_amd import _lib
from multimodalgame_amd.engine import Engine
from tests.test_plan_cpu import SHAPES, caps_line, entry, switches  # noqa: F401  (switches: fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", ["c2", "c3", "c4", "c4_r256", "c5"])
def test_engine_plan_equals_the_recorded_plan(shape, switches):
    e = entry(shape)
    eng = Engine(**SHAPES[shape])
    text = eng.plan_text()
    assert text.splitlines() == e["plan"] + [caps_line(e["caps"])]
    assert text == _lib.plan_for(eng.cfg, _lib.plan_caps(text))
