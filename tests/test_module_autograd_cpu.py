"""CPU-side checks of autograd through the agent modules' forward(): the three per-call VJP entry points are declared with their
argument counts, exported, bound and listed, and the Python layer has the nodes and the parameter version (the GPU behaviour:
tests/test_module_autograd_gpu.py)."""
import os
import re

import pytest

from multimodalgame_amd import _lib, agents
from multimodalgame_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,nargs", [("mmg_sender_vjp", 11), ("mmg_receiver_vjp", 16), ("mmg_baseline_vjp", 11)])
def test_per_call_vjp_is_declared_exported_and_bound(name, nargs):
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header)
    assert m, "include/mmg.h does not declare %s" % name
    assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
    assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == nargs
    assert lib.mmg_version() == 3


def test_exchange_vjp_keeps_its_arguments():
    assert len(_lib.load().mmg_exchange_vjp.argtypes) == 12


def test_per_call_scratch_sits_before_the_job_tables():
    """k_wgrad may over-read the last row of its operand arrays: the per-call operand copies lie in front of the job tables,
    and the job-table slot holds the exchange's four tables and the per-call four."""
    cfg = _lib.make_config(64, 30, 512, 256, 32, 64, 100, 500, 10, fixed_exchange=False)
    tab = {e["name"]: e for e in _lib.tape_table(cfg)}
    for k in ("vcz", "vch0", "vch1", "vchx", "vcdh"):
        assert tab[k]["offset"] < tab["tables"]["offset"], k
    assert list(tab["vch0"]["dims"][:2]) == [64, 64] and list(tab["vchx"]["dims"][:2]) == [64, 256]
    assert tab["vtables"]["dims"][0] == 8 * 32768


def test_module_nodes_and_parameter_version_exist():
    for fn in (agents._SenderCall, agents._ReceiverCall, agents._BaselineCall):
        assert issubclass(fn, agents._CallVJP)
    for m in ("sender_vjp", "receiver_vjp", "baseline_vjp", "bump_param_version"):
        assert callable(getattr(Engine, m))
    assert isinstance(Engine.param_version, property)
