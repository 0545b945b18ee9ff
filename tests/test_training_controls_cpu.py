"""Training controls without a GPU (include/mmg.h: mmg_set_trainable, mmg_set_learning_rate, mmg_set_entropy,
mmg_get_training_controls; Game.freeze / unfreeze / set_hyper).

1. The test-side reference itself: cpu_ref.train_minibatch with a FrozenOptimizer leaves a frozen agent's parameters and
   optimizer state bit-identical and the other agents exactly where the unfrozen loop puts them (Adam, three minibatches, the
   middle one frozen); Adam's bias correction of the frozen agent stands still.
2. The entries are declared, exported and bound; bad values are refused with their text before any handle is looked at.
3. Game: names, refusals, what lands in game.cfg, and the checkpoint fields' round trip through misc.torch_save / torch_load --
   also from a checkpoint that lacks them.
"""
import inspect
import os
import re

import pytest
import torch

from oracle import cpu_ref
from tests import common, training_controls_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(batch_size=3, img_feat_dim=8, img_h_dim=6, rec_w_dim=4, sender_out_dim=4, rec_hidden=5, wv_dim=6, baseline_hid_dim=7,
            max_exchange=3, fixed_exchange=True, use_binary=True, entropy_s=0.08, entropy_sen=0.01, entropy_rec=None, top_k_train=2)


def _tiny_meta(**over):
    meta = dict(cpu_ref.Flags(**dict(TINY, **over)).__dict__)
    meta.update(n_classes=3, batch=3, n_minibatches=3, seed_weights=11, seed_data=12, seed_uniforms=13)
    return meta


# ------------------------------------------------------------------ 1. the reference of the GPU tests
def test_frozen_optimizer_reproduces_the_reference_loop_without_that_step():
    meta = _tiny_meta(optim_type="Adam", learning_rate=1e-2)
    snaps, plain = [], []
    ref.oracle_loop(None, meta, [dict(), dict(frozen=("sender",)), dict(frozen=())], snapshots=snaps)
    ref.oracle_loop(None, meta, [dict(), dict(), dict()], snapshots=plain)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    # minibatch 0: the two loops are the same loop
    for a in ref.AGENTS:
        assert same(snaps[0][1][a]["params"], plain[0][1][a]["params"])
    # minibatch 1, sender frozen: parameters and state unchanged, bit for bit; the others as in the plain loop -- they read the
    # sender's messages, not its step, and the sender's parameters of this minibatch are the same in both loops
    before, after = snaps[1]
    assert same(before["sender"]["params"], after["sender"]["params"])
    for s0, s1 in zip(before["sender"]["state"], after["sender"]["state"]):
        assert set(s0) == set(s1) == {"step", "exp_avg", "exp_avg_sq"}
        assert all(torch.equal(torch.as_tensor(s0[k]), torch.as_tensor(s1[k])) for k in s0)
        assert float(s1["step"]) == 1.0
    for a in ("receiver", "baseline_rec", "baseline_sen"):
        assert same(after[a]["params"], plain[1][1][a]["params"]), a
        assert not same(before[a]["params"], after[a]["params"]), a
    assert not same(plain[1][0]["sender"]["params"], plain[1][1]["sender"]["params"])
    # minibatch 2, unfrozen again: the sender's second step, the others' third
    assert [float(s["step"]) for s in snaps[2][1]["sender"]["state"]] == [2.0] * len(snaps[2][1]["sender"]["state"])
    rec = [float(s["step"]) for s in snaps[2][1]["receiver"]["state"] if s]     # (Fixed exchange: the stop layer has no gradient, no state)
    assert rec and rec == [3.0] * len(rec)
    assert not same(snaps[2][0]["sender"]["params"], snaps[2][1]["sender"]["params"])


def test_schedule_values_reach_the_oracle():
    meta = _tiny_meta(optim_type="SGD", learning_rate=1e-2)
    got = ref.resolve([dict(), dict(frozen=("sender",), lr=5e-3), dict(entropy=dict(entropy_s=0.02)), dict(frozen=())], meta)
    assert [c["frozen"] for c in got] == [(), ("sender",), ("sender",), ()]
    assert [c["lr"] for c in got] == [1e-2, 5e-3, 5e-3, 5e-3]
    assert [c["entropy"]["entropy_s"] for c in got] == [0.08, 0.08, 0.02, 0.02] and got[3]["entropy"]["entropy_rec"] is None
    # lr = 0 on the oracle: an SGD step of size zero; another entropy weight: other receiver gradients
    snaps = []
    base = ref.oracle_loop(None, meta, [dict()])
    zero = ref.oracle_loop(None, meta, [dict(lr=0.0)], snapshots=snaps)
    assert all(torch.equal(snaps[0][0][a]["params"][k], snaps[0][1][a]["params"][k]) for a in ref.AGENTS for k in snaps[0][0][a]["params"])
    assert float(zero["mb0.gradnorm.receiver"]) == float(base["mb0.gradnorm.receiver"])
    meta_a = dict(meta, fixed_exchange=False)
    ent = ref.oracle_loop(None, meta_a, [dict(entropy=dict(entropy_s=0.5))])
    assert float(ent["mb0.gradnorm.receiver"]) != float(ref.oracle_loop(None, meta_a, [dict()])["mb0.gradnorm.receiver"])


# ------------------------------------------------------------------ 2. the entries
def test_entries_are_declared_exported_and_bound():
    from multimodalgame_amd import _lib
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    want = {"mmg_set_trainable": ["h", "mask"], "mmg_set_learning_rate": ["h", "lr"],
            "mmg_set_entropy": ["h", "entropy_s", "entropy_sen", "entropy_rec"],
            "mmg_get_training_controls": ["h", "mask", "lr", "entropy3"]}
    lib = _lib.load()
    for name, args in want.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, "include/mmg.h does not declare " + name
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == args
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == len(args)
    assert "#define MMG_VERSION 3" in header and lib.mmg_version() == 3
    assert _lib.agent_mask(_lib.AGENTS) == 15 and _lib.agent_mask(["sender"]) == 2 and _lib.agent_mask([]) == 0
    with pytest.raises(ValueError, match="no agent"):
        _lib.agent_mask(["speaker"])


def test_bad_values_are_refused_with_their_text():
    """The values are checked before the handle: without one, a bad value gives its own message and a good one "NULL handle"."""
    from multimodalgame_amd import _lib
    lib = _lib.load()
    err = lambda: lib.mmg_last_error().decode()
    for mask in (16, 0x1f, -1, 1 << 8):
        assert lib.mmg_set_trainable(None, mask) < 0 and "bits outside the four agents" in err(), mask
    for mask in (0, 1, 2, 15):
        assert lib.mmg_set_trainable(None, mask) < 0 and err() == "NULL handle", mask
    for lr in (-1e-4, float("nan"), float("inf"), -float("inf")):
        assert lib.mmg_set_learning_rate(None, lr) < 0 and "finite and >= 0" in err(), lr
    for lr in (0.0, 1e-4, 10.0):
        assert lib.mmg_set_learning_rate(None, lr) < 0 and err() == "NULL handle", lr
    for ent in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
        assert lib.mmg_set_entropy(None, *ent) < 0 and "must be finite" in err(), ent
    assert lib.mmg_set_entropy(None, 0.1, -0.2, 0.0) < 0 and err() == "NULL handle"
    assert lib.mmg_get_training_controls(None, None, None, None) < 0 and err() == "NULL handle"


def test_counter_holds_the_agents_frozen_steps_and_nothing_moved():
    from multimodalgame_amd import _lib
    cfg = _lib.make_config(batch=16, n_classes=30, feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=100, bas_hidden=500, max_exchange=10)
    table = _lib.tape_table(cfg)
    counter = [e for e in table if e["name"] == "counter"][0]
    assert counter["dims"] == [8] and counter["dtype"] == 2
    o = 0
    for e in table:                                             # every entry starts where the entries in front of it end
        assert e["offset"] == o, e["name"]
        n = 1
        for d in e["dims"]:
            n *= d
        o += (n * {0: 4, 1: 1, 2: 4, 3: 8}[e["dtype"]] + 255) & ~255


def _table_size(cfg, caps, frozen=()):
    """(gemm tiles, blocks of the fused launch = tiles + column blocks + 5, wgrad_opt_ok) of the job table with `frozen` agents left out."""
    from multimodalgame_amd import _lib
    line = _lib.plan_for(cfg, caps, _lib.agent_mask(frozen) << _lib.PLAN_FROZEN_SHIFT).splitlines()[0]
    m = re.search(r"\(gemm tiles (\d+)\) wgrad_opt_ok (\d) \(blocks (\d+),", line)
    return int(m.group(1)), int(m.group(3)), int(m.group(2))


def test_job_tables_hold_the_jobs_of_the_agents_in_training():
    """Every job belongs to one agent: the four agents' blocks add up to the whole table, a frozen agent's leave it, and what is decided
    from the table -- whether the optimizer fits inside k_wgrad's launch -- follows the table in use."""
    from multimodalgame_amd import _lib
    from tests.test_plan_cpu import entry
    caps = entry("c1")["caps"]
    kw = dict(batch=16, n_classes=30, feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=100, bas_hidden=500, max_exchange=10,
              fixed_exchange=False, entropy_s=0.08, entropy_sen=0.01, entropy_rec=0.01)
    cfg = _lib.make_config(**kw)
    tiles, blocks, opt_ok = _table_size(cfg, caps)
    assert tiles > 0 and blocks > tiles + 5 and opt_ok == 1
    own = {}
    for a in _lib.AGENTS:
        t, b, ok = _table_size(cfg, caps, (a,))
        own[a] = (tiles - t, blocks - b)
        assert 0 < t < tiles and ok == 1, a
    assert sum(v[0] for v in own.values()) == tiles and sum(v[1] for v in own.values()) == blocks - 5
    assert all(v[0] > 0 and v[1] > v[0] for v in own.values())          # every agent has matrices (tiles) and vectors (column blocks)
    t, b, _ = _table_size(cfg, caps, ("receiver", "baseline_rec", "baseline_sen"))
    assert (t, b - 5) == own["sender"]                                   # a sender-only phase runs the sender's blocks alone
    assert _table_size(cfg, caps, _lib.AGENTS)[:2] == (0, 5)            # nobody trains: the closing block and the norm roles
    # continuous messages: the receiver's jobs are the table; the other agents' bits change nothing
    cont = _lib.make_config(**dict(kw, use_binary=False, fixed_exchange=True, entropy_s=None, entropy_sen=None, entropy_rec=None))
    assert _table_size(cont, caps, ("sender", "baseline_rec", "baseline_sen")) == _table_size(cont, caps)
    assert _table_size(cont, caps, ("receiver",))[:2] == (0, 5)
    # a table past the co-residency budget of the fused launch fits again without the sender's tiles
    small = list(caps)
    small[_lib.PLAN_CAPS.index("n_cu")] = (blocks + 8) // caps[_lib.PLAN_CAPS.index("wgrad_opt")]      # one CU short of the whole table
    assert _table_size(cfg, small)[2] == 0 and _table_size(cfg, small, ("sender",))[2] == 1


# ------------------------------------------------------------------ 3. Game
def _game(relax=None, **over):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**dict(TINY, **over))
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    kw = dict(autograd=True, channel_grad=True, relax=relax) if relax else {}
    return Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cpu", **kw)


def test_game_freeze_unfreeze_and_set_hyper():
    from multimodalgame_amd import _lib
    from multimodalgame_amd.game import Game
    game = _game()
    assert game.trainable == _lib.AGENTS and set(game.models_dict()) == set(_lib.AGENTS)
    game.freeze("sender")
    assert game.trainable == ("receiver", "baseline_rec", "baseline_sen")
    game.freeze("baseline_rec", "baseline_sen")
    assert game.trainable == ("receiver",)
    game.unfreeze("sender")
    assert game.trainable == ("receiver", "sender")
    game.unfreeze()
    assert game.trainable == _lib.AGENTS
    game.freeze(*_lib.AGENTS)                                   # nobody trains: allowed
    assert game.trainable == ()
    game.unfreeze()
    with pytest.raises(ValueError, match="no agent"):
        game.freeze("speaker")
    assert game.trainable == _lib.AGENTS
    # values: kept in game.cfg, which every later engine is created from
    game.set_hyper(learning_rate=5e-5, entropy_s=0.02)
    assert game.cfg["learning_rate"] == 5e-5 and game.cfg["entropy_s"] == 0.02 and game.cfg["entropy_sen"] == 0.01
    game.set_hyper(entropy_rec=0.3)                             # None in the flags: stays absent, the argument is ignored
    assert game.cfg["entropy_rec"] is None
    game.set_hyper(learning_rate=0.0)
    assert game.cfg["learning_rate"] == 0.0
    for bad in (dict(learning_rate=-1.0), dict(learning_rate=float("nan")), dict(learning_rate=float("inf")),
                dict(entropy_s=float("nan")), dict(entropy_sen=float("inf"))):
        with pytest.raises(ValueError):
            game.set_hyper(**bad)
    assert game.cfg["learning_rate"] == 0.0 and game.cfg["entropy_s"] == 0.02
    sig = inspect.signature(Game.set_hyper).parameters
    assert list(sig)[1:] == ["learning_rate", "entropy_s", "entropy_sen", "entropy_rec"] and all(sig[k].default is None for k in list(sig)[1:])
    for fn in (Game.freeze, Game.unfreeze, Game.set_hyper):
        assert "EVERY rank" in fn.__doc__ or "world > 1" in fn.__doc__


def test_a_relaxed_game_refuses_the_controls():
    game = _game(relax=dict(tau_sen=1.0, tau_rec=1.0), entropy_rec=0.01)
    for call in (lambda: game.freeze("sender"), lambda: game.unfreeze(), lambda: game.set_hyper(learning_rate=1e-3)):
        with pytest.raises(NotImplementedError, match="REINFORCE step: a game with relaxed messages trains through exchange"):
            call()
    with pytest.raises(NotImplementedError, match="REINFORCE step: a game with relaxed messages trains through exchange"):
        game.train_step(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 6))


def test_checkpoint_fields_round_trip(tmp_path):
    from multimodalgame_amd import misc
    game = _game()
    game.freeze("sender", "baseline_sen")
    game.set_hyper(learning_rate=2.5e-5, entropy_s=0.04, entropy_sen=0.003)
    game.set_agent_step("receiver", 7)
    game.set_agent_step("sender", 4)
    game.set_agent_step("baseline_rec", 7)
    game.set_agent_step("baseline_sen", 0)
    sd = game.optimizers_dict()["optimizer_sen"].state_dict()
    assert sd["param_groups"][0]["lr"] == 2.5e-5
    assert sd["training_controls"] == dict(trainable=False, learning_rate=2.5e-5, entropy_s=0.04, entropy_sen=0.003, entropy_rec=None, step=4)
    path = str(tmp_path / "ckpt.pt")
    misc.torch_save(path, dict(step=7), game.models_dict(), game.optimizers_dict())
    other = _game()
    data = misc.torch_load(path, other.models_dict(), other.optimizers_dict())
    assert data == dict(step=7)
    assert other.trainable == ("receiver", "baseline_rec")
    assert other.cfg["learning_rate"] == 2.5e-5 and other.cfg["entropy_s"] == 0.04 and other.cfg["entropy_sen"] == 0.003
    assert other.cfg["entropy_rec"] is None
    assert other.agent_steps() == dict(receiver=7, sender=4, baseline_rec=7, baseline_sen=0)
    # a checkpoint from before the controls existed: the fields are missing, nothing new is set
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    for sd in ckpt["optimizers"].values():
        del sd["training_controls"]
    torch.save(ckpt, path)
    third = _game()
    third.freeze("receiver")
    third.set_hyper(learning_rate=3e-3)
    misc.torch_load(path, third.models_dict(), third.optimizers_dict())
    assert third.trainable == ("sender", "baseline_rec", "baseline_sen") and third.cfg["learning_rate"] == 3e-3
    # torch's own optimizers take the state dict with the extra key
    opt = torch.optim.RMSprop(game.modules["sender"].parameters(), lr=1.0)
    opt.load_state_dict(game.optimizers_dict()["optimizer_sen"].state_dict())
    assert opt.param_groups[0]["lr"] == 2.5e-5
