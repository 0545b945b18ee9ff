"""The kernel selection as a pure function (host_select.h: shape_pass + decide), pinned without a GPU through mmg_plan_for.

tests/golden/plans_mi355x.json holds, per shape and setting, the five lines the selection printed on an MI355X at the commit before
it was split into pure passes ("plan"), and the device's answers there ("caps": the CU count and one occupancy per role kernel,
-1 = not asked for this shape).  Shapes: BASELINE configs 1-5 (3 and 5 as one rank's shard), config 3 at B = 512, config 5 at
B = 2 048, config 4 at rec_hidden 256, the tile / mc_binary / mc_continuous shapes of tests/test_autograd_gpu.py, config 1 at
wv_dim 200.  Settings: default, MMG_NO_ROLES=1, cu_budget 48 and 16, MMG_TILE=1 on the fast shapes, message flips on configs 1-3."""
import json
import os

import pytest

from multimodalgame_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "plans_mi355x.json")))
SHAPES, ENTRIES = GOLDEN["shapes"], GOLDEN["entries"]
# every environment switch the selection reads (host_select.h: read_switches)
SWITCHES = ("MMG_NO_FAST", "MMG_NO_MERGE", "MMG_NO_MERGE_PREP", "MMG_NO_PERSIST_LL", "MMG_NO_RSAMPLE", "MMG_NO_RMSG", "MMG_NO_FUSED_S",
            "MMG_NO_MC", "MMG_NO_RC", "MMG_NO_TILE", "MMG_TILE", "MMG_NO_SPLIT", "MMG_NO_PERSIST", "MMG_NO_RC_BWD", "MMG_NO_RC_PERSIST",
            "MMG_NO_MC3P", "MMG_NO_GAME", "MMG_NO_WGRAD_OPT", "MMG_NO_ROLES", "HSA_CU_MASK", "ROC_GLOBAL_CU_MASK")
N_CU = (1, 8, 16, 48, 128, 240, 256)


def entry_id(e):
    return "%s-%s" % (e["shape"], e["setting"])


def entry(shape, setting="default"):
    return [e for e in ENTRIES if e["shape"] == shape and e["setting"] == setting][0]


def caps_line(caps):
    return "mmg_create: caps " + " ".join("%s %d" % kv for kv in zip(_lib.PLAN_CAPS, caps))


@pytest.fixture
def switches(monkeypatch):
    """Sets exactly the given switches for the test; every other one is unset."""
    def set_env(env):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    set_env({})
    return set_env


def plan(e, caps=None, cu_budget=None, flags=None):
    cfg = _lib.make_config(cu_budget=e["cu_budget"] if cu_budget is None else cu_budget, **SHAPES[e["shape"]])
    return _lib.plan_for(cfg, e["caps"] if caps is None else caps, e["flags"] if flags is None else flags)


def test_fixture_covers_the_matrix():
    assert tuple(GOLDEN["caps_order"]) == _lib.PLAN_CAPS
    assert set(SHAPES) == {"c1", "c2", "c3", "c4", "c5", "c3_b512", "c5_b2048", "c4_r256", "tile", "mc_binary", "mc_continuous", "c1_wv200"}
    ids = {entry_id(e) for e in ENTRIES}
    assert len(ids) == len(ENTRIES)
    for s in SHAPES:
        fast = entry(s)["plan"][0].startswith("mmg_create: family 0 ")
        want = {"default", "no_roles", "cu48", "cu16"} | ({"tile"} if fast else set()) | ({"flips"} if s in ("c1", "c2", "c3") else set())
        assert {e["setting"] for e in ENTRIES if e["shape"] == s} == want, s
    for e in ENTRIES:
        assert len(e["plan"]) == 5 and len(e["caps"]) == len(_lib.PLAN_CAPS)
        assert e["env"] == {"no_roles": {"MMG_NO_ROLES": "1"}, "tile": {"MMG_TILE": "1"}}.get(e["setting"], {})
        assert e["flags"] == (_lib.PLAN_FLIPS if e["setting"] == "flips" else 0)
        assert e["cu_budget"] == {"cu48": 48, "cu16": 16}.get(e["setting"], 0) and e["caps"][0] == (e["cu_budget"] or 256)


@pytest.mark.parametrize("e", ENTRIES, ids=entry_id)
def test_pure_selection_reproduces_the_recorded_plan(e, switches):
    switches(e["env"])
    assert plan(e).splitlines() == e["plan"] + [caps_line(e["caps"])]


@pytest.mark.parametrize("e", [e for e in ENTRIES if not e["cu_budget"]], ids=entry_id)
def test_cu_budget_equals_a_device_with_that_many_cus(e, switches):
    switches(e["env"])
    for c in (16, 48, 240, 256, 300):
        assert plan(e, cu_budget=c) == plan(e, caps=[min(e["caps"][0], c)] + e["caps"][1:], cu_budget=0), c


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_cu_count_selects_a_plan(shape, switches):
    e = entry(shape)
    for n in N_CU:
        for flags in (0, _lib.PLAN_NO_ROLES):
            text = plan(e, caps=[n] + e["caps"][1:], flags=flags)          # (raises MmgError on a negative status)
            assert (" no_roles %d n_cu %d " % (flags, n)) in text.splitlines()[0]


@pytest.mark.parametrize("e", ENTRIES, ids=entry_id)
def test_no_roles_flag_equals_the_switch(e, switches):
    switches(e["env"])
    by_flag = plan(e, flags=e["flags"] | _lib.PLAN_NO_ROLES)
    switches(dict(e["env"], MMG_NO_ROLES="1"))
    assert by_flag == plan(e)
    assert " no_roles 1 " in by_flag


def test_bad_arguments_are_refused():
    e = entry("c2")
    with pytest.raises(_lib.MmgError, match="caps expected"):
        plan(e, caps=e["caps"][:-1])
    with pytest.raises(_lib.MmgError, match="positive"):
        plan(e, caps=[0] + e["caps"][1:])
