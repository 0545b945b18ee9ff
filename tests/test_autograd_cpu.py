"""CPU-side checks of the autograd path of exchange(): the VJP entry point is declared, exported and bound, and the Python
layer exposes the opt-in without a GPU (the GPU behaviour: tests/test_autograd_gpu.py)."""
import inspect
import os
import re

from multimodalgame_amd import _lib, game
from multimodalgame_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exchange_vjp_is_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    m = re.search(r"int\s+mmg_exchange_vjp\s*\(([^)]*)\)", header)
    assert m, "include/mmg.h does not declare mmg_exchange_vjp"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 12
    assert "mmg_exchange_vjp" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "mmg_exchange_vjp")
    assert len(lib.mmg_exchange_vjp.argtypes) == 12
    assert lib.mmg_version() == 3


def test_vjp_tape_arrays_sit_before_the_job_tables():
    """k_wgrad's GEMM tiles may over-read the columns of their operand arrays' last row: every VJP operand lies inside the
    workspace, in front of the job tables; the four VJP job tables have a slot of their own."""
    cfg = _lib.make_config(64, 30, 512, 256, 32, 64, 100, 500, 10, fixed_exchange=False)
    tab = {e["name"]: e for e in _lib.tape_table(cfg)}
    for k in ("vdgi", "vdgh", "vdA", "vA", "vdC", "vPy2", "vdlw", "vg", "vdbar", "vdpre", "va", "vc", "vdlz", "vdhx",
              "vdc0", "vhid_s", "vhid_r", "vzr", "vdbs", "vdbr", "vdesc"):
        assert tab[k]["offset"] < tab["tables"]["offset"], k
    assert tab["vtables"]["offset"] > tab["tables"]["offset"]
    assert list(tab["vdA"]["dims"][:3]) == [10, 64, 64]


def test_autograd_is_opt_in():
    assert "autograd" in inspect.signature(game.Game.__init__).parameters
    assert inspect.signature(game.Game.__init__).parameters["autograd"].default is False
    assert hasattr(Engine, "vjp")
    for fn, agent in ((game._SenderVJP, "sender"), (game._ReceiverVJP, "receiver"),
                      (game._BaselineSenVJP, "baseline_sen"), (game._BaselineRecVJP, "baseline_rec")):
        assert fn.AGENT == agent and agent in _lib.AGENTS
