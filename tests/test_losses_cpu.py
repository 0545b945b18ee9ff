"""CPU-side checks of the loss functions' boundary (no GPU needed): include/mmg.h declares the handle-free loss entry points and
_lib.SYMBOLS lists them, the library exports them, the host-only size query answers, and multimodalgame_amd.losses refuses what it
cannot run on the device -- CPU tensors, None probabilities (continuous messages), lists of different lengths -- with ValueError."""
import os
import re

import pytest
import torch

from multimodalgame_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_SYMBOLS = ("mmg_loss_save_doubles", "mmg_loss_binary_forward", "mmg_loss_binary_vjp", "mmg_loss_bas_forward",
                "mmg_loss_bas_vjp", "mmg_rec_outp_forward", "mmg_rec_outp_vjp")


def test_header_declares_and_lib_lists_the_loss_symbols():
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    declared = set(re.findall(r"\b(mmg_[a-z_]+)\s*\(", header))
    lib = _lib.load()
    for sym in LOSS_SYMBOLS:
        assert sym in declared, "include/mmg.h does not declare " + sym
        assert sym in _lib.SYMBOLS, "_lib.SYMBOLS does not list " + sym
        fn = getattr(lib, sym)
        assert fn.argtypes is not None, sym + " has no argtypes"
    assert lib.mmg_version() == 3                               # additive: the ABI version stays


def test_each_declaration_cites_the_reference_lines():
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    for sym, lines in (("mmg_loss_binary_forward", "model.py:930-968"), ("mmg_loss_bas_forward", "model.py:971-988"),
                       ("mmg_rec_outp_forward", "model.py:879-904")):
        assert re.search(re.escape(sym) + r" <- [^\n]*" + re.escape(lines), header), (sym, lines)


def test_save_size_query_answers_without_a_gpu():
    lib = _lib.load()
    sizes = [int(lib.mmg_loss_save_doubles(n)) for n in (1, 2, 10, 64)]
    assert all(s >= 3 * n for s, n in zip(sizes, (1, 2, 10, 64)))        # at least n_t, den_t, c_t / n_t per step
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert lib.mmg_loss_save_doubles(0) < 0 and b"n_steps" in lib.mmg_last_error()
    assert lib.mmg_loss_save_doubles(1 << 20) < 0                           # a limit is an error return, never a truncation


def test_entry_points_reject_bad_shapes_before_touching_the_gpu():
    lib = _lib.load()
    assert lib.mmg_loss_bas_forward(None, None, None, 0, 4, None, None, None) < 0
    assert lib.mmg_loss_bas_forward(None, None, None, 3, 4, None, None, None) < 0 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_rec_outp_vjp(None, None, None, None, None, None, 1 << 20, 4, 4, None, None) < 0
    assert lib.mmg_loss_binary_vjp(None, None, None, None, None, None, None, None, 2, 2, 0, 0, 0.0, None, None) < 0


def _step(B=4, W=3):
    return torch.zeros(B, W), torch.full((B, W), 0.5), torch.zeros(B, 1), torch.zeros(B, 1)


def test_cpu_tensors_raise_value_error():
    from multimodalgame_amd import losses
    feat, prob, logs, score = _step()
    mask = torch.ones(4, 1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CPU"):
        losses.multistep_loss_binary([feat], [prob], logs, [score], None, 0.01)
    with pytest.raises(ValueError, match="CPU"):
        losses.calculate_loss_binary(feat, prob, logs, score, None)
    with pytest.raises(ValueError, match="CPU"):
        losses.multistep_loss_bas([score], logs, [mask])
    with pytest.raises(ValueError, match="CPU"):
        losses.calculate_loss_bas(score, logs)
    with pytest.raises(ValueError, match="CPU"):
        losses.get_rec_outp([prob], None)
    with pytest.raises(ValueError, match="CPU"):
        losses.reward_and_nll([prob], [mask], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="CPU"):
        losses.loglikelihood(prob, torch.zeros(4, 1, dtype=torch.int64))


def test_none_probabilities_raise_value_error():
    from multimodalgame_amd import losses
    feat, prob, logs, score = _step()
    with pytest.raises(ValueError, match="None"):
        losses.multistep_loss_binary([feat, feat], [None, None], logs, [score, score], None, None)
    with pytest.raises(ValueError, match="None"):
        losses.calculate_loss_binary(feat, None, logs, score, None)


def test_mismatched_list_lengths_raise_value_error():
    from multimodalgame_amd import losses
    feat, prob, logs, score = _step()
    mask = torch.ones(4, 1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="same length"):
        losses.multistep_loss_binary([feat], [prob, prob], logs, [score, score], None, None)
    with pytest.raises(ValueError, match="same length"):
        losses.multistep_loss_binary([feat, feat], [prob, prob], logs, [score], None, None)
    with pytest.raises(ValueError, match="same length"):
        losses.multistep_loss_binary([feat, feat], [prob, prob], logs, [score, score], [mask], None)
    with pytest.raises(ValueError, match="same length"):
        losses.multistep_loss_bas([score, score], logs, [mask, mask, mask])
    with pytest.raises(ValueError, match="same length"):
        losses.get_rec_outp([prob, prob], [mask])


def test_reference_names_are_where_a_model_py_user_looks():
    from multimodalgame_amd import losses, model
    for name in ("loglikelihood", "get_rec_outp", "calculate_loss_binary", "multistep_loss_binary", "calculate_loss_bas",
                 "multistep_loss_bas"):
        assert getattr(model, name) is getattr(losses, name), name
    from multimodalgame_amd import game
    assert game.get_rec_outp is not losses.get_rec_outp         # the host-side helper stays what it was
